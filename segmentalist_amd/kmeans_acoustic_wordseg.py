"""
Drop-in for segmentalist/kmeans_acoustic_wordseg.py: segmental k-means word segmentation.

`SegmentalKMeansWordseg` keeps the reference's constructor, attributes, methods and record
keys.  Two execution modes:

  sync="sequential" (default)  the reference's chain: utterances are visited one by one in
        `random.shuffle` order and the component statistics are updated between
        utterances, all on the device (score -> DP -> del/add/clean per utterance, enqueued
        asynchronously).  Bit-identical boundaries / assignments / means to the reference.
  sync="batch"                 every utterance of a sweep is scored against the statistics
        frozen at the start of the sweep (one MFMA GEMM over all embeddings), one workgroup
        per utterance runs the DP, and the statistics are rebuilt once per sweep in a fixed
        summation order; utterances shard over the ranks of a torch.distributed job.  A
        different (AD-LDA style) chain; bit-identical for 1/2/4/8 GPUs and to the CPU
        restatement of the same specification (oracle/np_oracle.py kmeans_batch_sweep).
        n_batches > 1: the sweep runs as that many steps, each resegmenting 1/n_batches of every
        statistics block against the means the previous step left (kmeans_minibatch_sweep):
        between the whole-sweep batch chain and the reference's per-utterance refresh.
"""
import ctypes as C
import logging
import os
import random
import time

import numpy as np

from . import _abi, rng
from .comm import get_comm
from .device import DeviceCorpus, KMeansBatchSweeper, Partition, to_dev
from .kmeans import KMeans, _consecutive
from .utterances import Utterances, process_embeddings

logger = logging.getLogger(__name__)
i_debug_monitor = 0          # kept for API compatibility (debug traces are not reproduced)
segment_debug_only = False


class SegmentalKMeansWordseg(object):
    def __init__(self, am_K, embedding_mats, vec_ids_dict, durations_dict, landmarks_dict,
                 seed_boundaries_dict=None, seed_assignments_dict=None, n_slices_min=0,
                 n_slices_max=20, min_duration=0, p_boundary_init=0.5, init_am_assignments="rand",
                 wip=0, sync="sequential", n_stat_blocks=8, flag_cap=None, process_group=None, n_batches=1,
                 shard_corpus=None):
        logger.info("Initializing")
        assert seed_assignments_dict is None or seed_boundaries_dict is not None
        assert sync in ("sequential", "batch")
        assert n_batches >= 1
        self.n_batches = int(n_batches)      # batch mode: statistics refreshed n_batches times per sweep (mini-batches)
        self.n_slices_min = n_slices_min
        self.n_slices_max = n_slices_max
        self.min_duration = min_duration
        self.wip = wip
        self.sync = sync

        embeddings, vec_ids, ids_to_utterance_labels = process_embeddings(embedding_mats, vec_ids_dict)
        self.ids_to_utterance_labels = ids_to_utterance_labels
        N = embeddings.shape[0]

        seed_boundaries = None
        if seed_boundaries_dict is not None:
            seed_boundaries = [seed_boundaries_dict[i] for i in ids_to_utterance_labels]
        lengths = [len(landmarks_dict[i]) for i in ids_to_utterance_labels]
        landmarks = [landmarks_dict[i] for i in ids_to_utterance_labels]
        durations = [durations_dict[i] for i in ids_to_utterance_labels]
        self.utterances = Utterances(
            lengths, vec_ids, durations, landmarks, seed_boundaries=seed_boundaries,
            p_boundary_init=p_boundary_init, n_slices_min=n_slices_min, n_slices_max=n_slices_max,
            min_duration=min_duration)

        # embeddings in the initial segmentation (kmeans_acoustic_wordseg.py:136-141)
        init_embeds = []
        for i in range(self.utterances.D):
            init_embeds.extend(self.utterances.get_segmented_embeds_i(i))
        init_embeds = np.array(init_embeds, dtype=int)
        init_embeds = init_embeds[np.where(init_embeds != -1)]
        logger.info("No. initial embeddings: " + str(init_embeds.shape[0]))

        assignments = -1 * np.ones(N, dtype=int)
        if seed_assignments_dict is not None:
            assert False, "to-do"                       # as the reference (:148-149)
        elif init_am_assignments == "rand":             # :183-194
            a = _consecutive(np.random.randint(0, am_K, len(init_embeds)))
            assignments[init_embeds] = a
        elif init_am_assignments == "spread":           # :196-205
            n = len(init_embeds)
            spread = (list(range(am_K)) * int(np.ceil(float(n) / am_K)))[:n]
            rng.shuffle(spread)
            assignments[init_embeds] = np.array(spread)
        elif init_am_assignments == "one-by-one":
            assert False, "to-do"                       # as the reference (:207-208)
        else:
            assert False, "invalid value for `init_am_assignments`: " + init_am_assignments

        # device images
        u = self.utterances
        # banded span tables for the DP kernels' fast path (windows of at most 8 slices, at most 64 landmarks)
        band = u.band_tables(n_slices_max) if (1 <= n_slices_max <= 8 and u.N_max <= 64) else None
        # Multi-rank batch mode ("each GPU keeps its shard's X rows"): this rank's device holds only the rows of
        # its own utterances -- the float32 matrix, both fp16 planes, the per-row work arrays -- numbered from 0; the span
        # tables name them by those local numbers.  shard_corpus=False keeps every row on every rank (needed to mix in
        # sequential-mode calls or KMeans.fit, which walk the whole matrix).
        comm = get_comm(process_group)
        if shard_corpus is None:
            shard_corpus = sync == "batch" and comm.world > 1
        shard = None
        if shard_corpus and comm.world > 1:
            assert sync == "batch", "a sharded corpus exists in batch mode only (the sequential chain does not shard)"
            pt = Partition(u.D, vec_ids.row_start, n_stat_blocks, comm.rank, comm.world)
            shard = (pt.row_lo, pt.row_hi)
            vi = np.full(np.asarray(u.vec_ids).shape, -1, dtype=np.int32)
            own = np.asarray(u.vec_ids)[pt.utt_lo:pt.utt_hi]
            vi[pt.utt_lo:pt.utt_hi] = np.where(own >= 0, own - pt.row_lo, -1)
            if band is not None:
                bi = np.full(band[0].shape, -1, dtype=np.int32)
                bown = band[0][pt.utt_lo:pt.utt_hi]
                bi[pt.utt_lo:pt.utt_hi] = np.where(bown >= 0, bown - pt.row_lo, -1)
                band = (bi, band[1])
            self._corpus = DeviceCorpus(embeddings[pt.row_lo:pt.row_hi], vi, u.durations, u.lengths, band=band)
        else:
            self._corpus = DeviceCorpus(embeddings, u.vec_ids, u.durations, u.lengths, band=band)
        self.acoustic_model = KMeans(embeddings, am_K, assignments, _corpus=self._corpus, _shard=shard)
        self._dk = self.acoustic_model.components.dev
        self._dev_bounds = to_dev(u.boundaries.astype(np.uint8))
        u.bind_device(self._dev_bounds, refresh=self._dk.ensure_boundaries)
        self._row_start = vec_ids.row_start

        # batch mode plumbing (single process unless torch.distributed is initialised)
        self._sweeper = None
        self.kmeans_refit_records = []       # segment(..., kmeans_sync="batch"): one fit-style record per sweep
        # flag_cap: tokens per statistics block and sweep that may found new components (more: an error, never a wrong result).
        # Default 4 096; 1 024 with a sharded corpus, whose records carry flag_cap embedding rows per block over the wire.
        if flag_cap is None:
            flag_cap = 1024 if shard is not None else 4096
        self._batch_args = (n_stat_blocks, flag_cap, comm)

    # ------------------------------------------------------------------ sequential mode
    def segment_i(self, i):
        """kmeans_acoustic_wordseg.py:225-332.  Returns the length-weighted objective of the
        utterance (computed with the means before the update, as in the reference)."""
        self._segment_i_async(i)
        self._dk.check_status()
        return float(self._dk.out_total[i].item())

    def _segment_i_async(self, i):
        self._dk.segment_utt_sequential(self._dev_bounds, i, self.n_slices_min, self.n_slices_max, self.wip)
        self.utterances.mark_device_dirty()

    def get_vec_embed_neg_len_sqrd_norms(self, vec_ids, durations):
        """kmeans_acoustic_wordseg.py:334-351 for arbitrary (vec_ids, durations) vectors."""
        vec_ids = np.asarray(vec_ids)
        out = -np.inf * np.ones(len(vec_ids))
        valid = np.where(vec_ids != -1)[0]
        if len(valid):
            mx, _, _ = self._dk.exact_max(vec_ids[valid].astype(np.int32))
            d = np.asarray(durations, dtype=np.float64)[valid]
            with np.errstate(invalid="ignore"):
                out[valid] = np.where(np.isnan(d), -np.inf, mx * d)
        return out + self.wip

    # ------------------------------------------------------------------ held-out utterances
    def decode(self, embedding_mats, vec_ids_dict, durations_dict, landmarks_dict, device_out=False):
        """Segment and label HELD-OUT utterances, read-only (specification tests/kmeans_decode.py; segk_kmd_decode,
        DESIGN.md 4.24).  The four dictionaries are the constructor's, for utterances that are in no model.  Per utterance,
        with the model's n_slices_min / n_slices_max / min_duration / wip, exactly segment_i (kmeans_acoustic_wordseg.py:225-332)
        up to and without its update (:314-320): the span scores of get_vec_embed_neg_len_sqrd_norms (:334-351) -- the
        maximum over all K_max rows of `means`, inactive rows included --, the boundaries and objective of
        forward_backward_kmeans_viterbi (:449-555) from cleared flags, and for every chosen segment the raw argmax row
        (argmax_neg_sqrd_norm_i, first maximum), min(row, K) -- the component add_item would give it (kmeans_components.py:
        103-106), K for "would found a new component" -- and the unscaled max_neg_sqrd_norm.  A chosen segment whose span
        has no embedding (only after the DP stepped back from a dead end) is kept with embedding -1, row -1, label -1 and
        score -inf.

        The model is not changed: no statistic, no boundary, no hint of the next sweep, no `random` / `np.random` draw;
        works on a sequential model and on a live batch state, whatever is pending after batch sweeps or refits.

        Returns a `KMeansDecoded`; with device_out=True its arrays are device tensors, enqueued without a synchronisation (the
        flat segment arrays then have n_utt * N_max entries, the first seg_offsets[-1] of them segments).
        Raises SegkError before any launch for: more than one rank or a sharded corpus, a held-out D other than the model's,
        a span id beyond the held-out rows, n_slices_min outside {0, 1}, and a band of spans beyond the LDS of a workgroup."""
        labels, cq = self._heldout_corpus(embedding_mats, vec_ids_dict, durations_dict, landmarks_dict)
        out = self._decode_corpus(labels, cq)
        return out if device_out else out.numpy()

    def _heldout_corpus(self, embedding_mats, vec_ids_dict, durations_dict, landmarks_dict):
        """The checks of decode() and the device image of the held-out utterances: (sorted keys, DeviceCorpus or None for an
        empty set).  Host work and one upload; nothing of the model is read on the device."""
        from ._abi import SegkError
        dk = self._dk
        if get_comm(self._batch_args[2]).world > 1:
            raise SegkError("decode runs in one process only (%d ranks): held-out utterances are not sharded"
                            % get_comm(self._batch_args[2]).world)
        if not embedding_mats:
            dk.check_decode(self._corpus.D, 1, self.n_slices_min, self.n_slices_max)
            return [], None
        embeddings, vec_ids, labels = process_embeddings(embedding_mats, vec_ids_dict)
        embeddings = np.asarray(embeddings)
        D = embeddings.shape[1] if embeddings.ndim == 2 else -1
        lengths = [len(landmarks_dict[i]) for i in labels]
        u = Utterances(lengths, vec_ids, [durations_dict[i] for i in labels], [landmarks_dict[i] for i in labels],
                       p_boundary_init=0, n_slices_min=self.n_slices_min, n_slices_max=self.n_slices_max,
                       min_duration=self.min_duration)
        dk.check_decode(D, u.N_max, self.n_slices_min, self.n_slices_max)
        if u.vec_ids.max(initial=-1) >= len(embeddings):
            raise SegkError("decode: a span id names row %d of %d held-out embeddings" % (u.vec_ids.max(), len(embeddings)))
        if len(embeddings) == 0:
            raise SegkError("decode: the held-out utterances have no embedding at all")
        # the banded span tables of the kernel's window (the constructor builds them for the fast path's shapes)
        band = u.band_tables(self.n_slices_max) if 1 <= self.n_slices_max <= 8 else None
        return labels, DeviceCorpus(embeddings.astype(self._corpus.x_np_dtype, copy=False), u.vec_ids, u.durations, u.lengths,
                                    band=band)

    def _decode_corpus(self, labels, cq):
        """decode() on the device image of the held-out utterances: a `KMeansDecoded` of device tensors, nothing read back."""
        import torch
        dk = self._dk
        if cq is None:
            e_i, e_f = np.zeros(0, np.int64), np.zeros(0)
            return KMeansDecoded([], np.zeros((0, 0), bool), e_f, np.zeros(1, np.int64), e_i, e_i, e_i, e_i, e_i, e_f,
                                 int(self.acoustic_model.components.K))
        o = dk.decode(cq, self.n_slices_min, self.n_slices_max, self.wip)
        # segment j of utterance i ends behind its j-th set flag and starts where segment j - 1 ends; the flat arrays are the
        # rows' first n_seg entries in utterance order (stable sorts: nothing is read back)
        n_utt, NM = o["boundaries"].shape
        flags = o["boundaries"] != 0
        end = torch.sort((~flags).to(torch.int8), dim=1, stable=True).indices + 1
        start = torch.cat([torch.zeros_like(end[:, :1]), end[:, :-1]], dim=1)
        valid = torch.arange(NM, device=end.device)[None, :] < o["n_seg"][:, None]
        order = torch.sort((~valid).flatten().to(torch.int8), stable=True).indices
        flat = [t.flatten().index_select(0, order) for t in (start, end, o["seg_embed"].long(), o["seg_row"].long(),
                                                              o["seg_label"].long(), o["seg_score"])]
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=end.device), torch.cumsum(o["n_seg"].long(), 0)])
        return KMeansDecoded(labels, flags, o["objective"], offsets, *flat, K=o["K"])

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self):
        from . import checkpoint
        return checkpoint.state_dict(self)

    def load_state_dict(self, sd):
        from . import checkpoint
        checkpoint.load_state_dict(self, sd)

    # ------------------------------------------------------------------ batch mode
    def _get_sweeper(self):
        if self._sweeper is None:
            n_blocks, cap, group = self._batch_args
            comm = get_comm(group)
            part = Partition(self.utterances.D, self._row_start, n_blocks, comm.rank, comm.world)
            self._sweeper = KMeansBatchSweeper(self._dk, part, cap, comm)
        return self._sweeper

    def batch_sweep_async(self):
        """Enqueue one batch-synchronous sweep; results stay on the device."""
        if self.n_batches > 1:
            self._get_sweeper().sweep_minibatch(self._dev_bounds, self.n_slices_min, self.n_slices_max, self.wip, self.n_batches)
        else:
            self._get_sweeper().sweep(self._dev_bounds, self.n_slices_min, self.n_slices_max, self.wip)
        self.utterances.mark_device_dirty()

    def kmeans_refit_async(self):
        """Enqueue one batch refit (sync="batch"): a Lloyd iteration over the current tokens with the statistics rebuilt in the
        batch sweep's fixed order (tests/kmeans_refit.py kmeans_batch_refit); results stay on the device.  The counterpart
        of the reference's acoustic_model.fit(1, consider_unassigned=False) between sweeps (kmeans_acoustic_wordseg.py:425),
        for any number of ranks and a sharded corpus; the segmentation does not change."""
        assert self.sync == "batch", "kmeans_refit_async needs sync=\"batch\""
        self._get_sweeper().refit(self._dev_bounds)

    def _kmeans_refit_record(self):
        """(n_mean_updates, K, n_tokens, sum_neg_sqrd_norm) of the refit just enqueued: one device-to-host copy, and with
        several ranks one exchange of the two per-rank values (every rank gets the same sums, in rank order)."""
        sw = self._get_sweeper()
        pt = sw.part
        moved, n_comp, n_tok, sum_neg = self._dk.refit_record(pt.utt_lo, pt.utt_hi, self._dk.refit_moved)
        if pt.world > 1:
            parts = sw.comm.all_gather_object((moved, sum_neg))
            moved, sum_neg = sum(p[0] for p in parts), float(sum(p[1] for p in parts))
        else:
            sw.note_token_count(n_tok)
        return moved, n_comp, n_tok, sum_neg

    def _kmeans_batch_fit(self, n_iter):
        """KMeans.fit(n_iter, consider_unassigned=False) as batch refits: same record keys, same early stop."""
        rec = {"sum_neg_sqrd_norm": [], "components": [], "n_mean_updates": [], "sample_time": []}
        for i_iter in range(n_iter):
            start_time = time.time()
            self.kmeans_refit_async()
            moved, n_comp, _, sum_neg = self._kmeans_refit_record()
            rec["sum_neg_sqrd_norm"].append(sum_neg)
            rec["components"].append(n_comp)
            rec["n_mean_updates"].append(moved)
            rec["sample_time"].append(time.time() - start_time)
            info = "k-means refit: " + str(i_iter)
            for key in sorted(rec):
                info += ", " + key + ": " + str(rec[key][-1])
            logger.info(info)
            if moved == 0:
                break
        return rec

    def _kmeans_device_fit(self, n_iter):
        """acoustic_model.fit(n_iter, consider_unassigned=False) with the iterations on the device.  A token spans at least one
        landmark, so the landmarks bound the rows with a label; a captured sweep holds the addresses of the score path's
        workspaces, which scoring an id list of another length may reallocate (as in KMeansBatchSweeper.refit): the next sweep
        runs eagerly and is captured again."""
        sw = self._sweeper
        if sw is not None and sw.use_graph:
            sw._drop_graph()
            sw._warm = 0
        return self.acoustic_model.fit(n_iter, consider_unassigned=False, on_device=True,
                                       _n_items_bound=int(self._corpus.lengths_np.sum()))

    # ------------------------------------------------------------------ driver
    def segment(self, n_iter, n_iter_inbetween_kmeans=0, kmeans_sync=None):
        """kmeans_acoustic_wordseg.py:353-426; same record keys.
        kmeans_sync: how the n_iter_inbetween_kmeans Lloyd iterations after every sweep run.  None / "sequential": the
        reference's acoustic_model.fit (item by item; needs the whole corpus on this device).  "batch" (sync="batch" only): up
        to that many batch refits (kmeans_refit_async), stopping after the first that moves nothing; their fit-style records
        are kept in self.kmeans_refit_records, one dict per sweep.  "device" (either sync): the reference's acoustic_model.fit
        with every iteration run on the device (KMeans.fit(..., on_device=True)): the results of None, bit for
        bit, without a launch per moved token; needs the whole corpus on this device like None."""
        import torch
        assert kmeans_sync in (None, "sequential", "batch", "device"), "invalid value for `kmeans_sync`: " + str(kmeans_sync)
        if kmeans_sync == "batch":
            assert self.sync == "batch", "kmeans_sync=\"batch\" needs a segmenter constructed with sync=\"batch\""
        self.kmeans_refit_records = []
        logger.info("Segmenting for " + str(n_iter) + " iterations")
        record_dict = {"sum_neg_sqrd_norm": [], "sum_neg_len_sqrd_norm": [], "components": [],
                       "sample_time": [], "n_tokens": []}
        c = self.acoustic_model.components
        for i_iter in range(n_iter):
            start_time = time.time()
            batch_rec = None
            if self.sync == "sequential":
                utt_order = list(range(self.utterances.D))
                rng.shuffle(utt_order)
                if segment_debug_only:
                    utt_order = [i_debug_monitor]
                # the whole chain of the sweep enqueued by one library call (float32 data); SEGK_SEQ_PER_UTT=1 keeps the
                # per-utterance calls (score through the filter machinery, DP, update + image refresh)
                if os.environ.get("SEGK_SEQ_PER_UTT", "0") == "1" or not self._dk.sequential_sweep(
                        self._dev_bounds, utt_order, self.n_slices_min, self.n_slices_max, self.wip):
                    for i_utt in utt_order:
                        self._segment_i_async(i_utt)
                self.utterances.mark_device_dirty()
                torch.cuda.synchronize()
                self._dk.check_status()
                totals = self._dk.out_total.cpu().numpy()
                # the reference's `sum += ...` over the utterances in visiting order: a running sum is that sequence of
                # additions (np.cumsum accumulates left to right; the Python loop over 10 000 numpy scalars took 2 ms)
                sum_neg_len_sqrd_norm = np.cumsum(totals[np.asarray(utt_order, dtype=np.int64)])[-1] if len(utt_order) else 0
            else:
                self.batch_sweep_async()
                pt = self._get_sweeper().part
                if pt.world == 1:
                    # every record value of the sweep from one device-to-host copy (the metric from the token lists)
                    sum_neg_len_sqrd_norm, n_comp, n_tok, sum_neg = self._dk.batch_record(pt.utt_lo, pt.utt_hi)
                    batch_rec = (sum_neg, n_comp, n_tok)
                    self._get_sweeper().note_token_count(n_tok)
                else:
                    torch.cuda.synchronize()
                    self._dk.check_status()
                    sum_neg_len_sqrd_norm = float(self._dk.out_scalars[0].item())
            record_dict["sample_time"].append(time.time() - start_time)
            if batch_rec is not None:
                record_dict["sum_neg_sqrd_norm"].append(batch_rec[0])
                record_dict["sum_neg_len_sqrd_norm"].append(sum_neg_len_sqrd_norm)
                record_dict["components"].append(batch_rec[1])
                record_dict["n_tokens"].append(batch_rec[2])
            else:
                record_dict["sum_neg_sqrd_norm"].append(c.sum_neg_sqrd_norm())
                record_dict["sum_neg_len_sqrd_norm"].append(sum_neg_len_sqrd_norm)
                record_dict["components"].append(c.K)
                record_dict["n_tokens"].append(self.acoustic_model.get_n_assigned())
            info = "iteration: " + str(i_iter)
            for key in sorted(record_dict):
                info += ", " + key + ": " + str(record_dict[key][-1])
            logger.info(info)
            if n_iter_inbetween_kmeans > 0:
                if kmeans_sync == "batch":
                    self.kmeans_refit_records.append(self._kmeans_batch_fit(n_iter_inbetween_kmeans))
                elif kmeans_sync == "device":
                    self._kmeans_device_fit(n_iter_inbetween_kmeans)
                else:
                    self.acoustic_model.fit(n_iter_inbetween_kmeans, consider_unassigned=False)
        return record_dict

    def get_unsup_transcript_i(self, i):
        return list(self.acoustic_model.components.get_assignments(
            self.utterances.get_segmented_embeds_i(i)))

    def get_max_unsup_transcript_i(self, i):
        return self.acoustic_model.components.get_max_assignments(
            self.utterances.get_segmented_embeds_i(i))


class KMeansDecoded(object):
    """What SegmentalKMeansWordseg.decode returns (the k-means sibling of unigram_acoustic_wordseg.Decoded).
    utterance_labels: the sorted keys; boundaries bool [n_utt, N_max]; objective [n_utt]: the length-weighted objective
    segment_i returns; segments of utterance i: the flat entries seg_offsets[i] .. seg_offsets[i + 1] - 1 of seg_start / seg_end
    (landmark indices: the segment spans the slices [start, end)), seg_embed (row of the stacked held-out matrix, utterances in
    sorted-key order; -1: no embedding), seg_row (the raw argmax row of `means`; -1: no embedding), seg_label (min(row, K):
    K stands for "would found a new component"; -1: no embedding) and seg_score (max_neg_sqrd_norm of the embedding, unscaled,
    as a double; -inf: none); K: the active components at the time of the call."""

    _fields = ("boundaries", "objective", "seg_offsets", "seg_start", "seg_end", "seg_embed", "seg_row", "seg_label", "seg_score",
               "K")

    def __init__(self, utterance_labels, boundaries, objective, seg_offsets, seg_start, seg_end, seg_embed, seg_row, seg_label,
                 seg_score, K):
        self.utterance_labels = list(utterance_labels)
        self.boundaries, self.objective, self.seg_offsets = boundaries, objective, seg_offsets
        self.seg_start, self.seg_end, self.seg_embed, self.seg_row = seg_start, seg_end, seg_embed, seg_row
        self.seg_label, self.seg_score, self.K = seg_label, seg_score, K

    def numpy(self):
        """The host form (waits for the device): NumPy arrays, the flat arrays cut to the segments, K an int."""
        if isinstance(self.K, int):
            return self
        h = {k: getattr(self, k).cpu().numpy() for k in self._fields}
        n = int(h["seg_offsets"][-1])
        for k in ("seg_start", "seg_end", "seg_embed", "seg_row", "seg_label", "seg_score"):
            h[k] = h[k][:n]
        h["K"] = int(h["K"].reshape(-1)[0])
        return KMeansDecoded(self.utterance_labels, **h)

    def transcript(self, i):
        """The labels of utterance i's segments, in order (a list of ints; reads the device arrays back if need be)."""
        r = self.numpy()
        return [int(k) for k in r.seg_label[r.seg_offsets[i]:r.seg_offsets[i + 1]]]


def _dp_tri(kind, vec, N, n_slices_min, n_slices_max, log_p_continue=0.0, anneal_temp=1.0, uniforms=None):
    """Run one triangular-layout DP problem on the device (segk_dp_tri)."""
    import torch
    vec_t = to_dev(np.asarray(vec, dtype=np.float64))
    dev = vec_t.device
    Ns = torch.tensor([N], dtype=torch.int32, device=dev)
    offs = torch.zeros(1, dtype=torch.int64, device=dev)
    bounds = torch.zeros(N, dtype=torch.uint8, device=dev)
    totals = torch.zeros(1, dtype=torch.float64, device=dev)
    nd = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.zeros(3 * N + 2, dtype=torch.float64, device=dev)
    u_t = to_dev(np.asarray(uniforms, dtype=np.float64)) if uniforms is not None else None
    _abi.check(_abi.lib().segk_dp_tri(
        _abi.ctx(), kind, _abi.ptr(vec_t), _abi.ptr(Ns), _abi.ptr(offs), 1, int(n_slices_min),
        int(n_slices_max), float(log_p_continue), float(anneal_temp), _abi.ptr(u_t),
        0 if u_t is None else u_t.numel(), _abi.ptr(bounds), N, _abi.ptr(totals), _abi.ptr(nd), _abi.ptr(st),
        _abi.ptr(work), 3 * N + 2, _abi.stream()))
    return float(totals.item()), bounds.cpu().numpy().astype(bool), int(nd.item()), int(st.item())


def forward_backward_kmeans_viterbi(vec_embed_neg_len_sqrd_norms, N, n_slices_min=0, n_slices_max=0,
                                    i_utt=None):
    """kmeans_acoustic_wordseg.py:449-555 on the device."""
    tot, bounds, _, _ = _dp_tri(0, vec_embed_neg_len_sqrd_norms, N, n_slices_min, n_slices_max)
    return tot, bounds

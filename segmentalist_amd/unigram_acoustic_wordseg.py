"""
Drop-in for segmentalist/unigram_acoustic_wordseg.py: unigram word segmentation of speech with a
Bayesian GMM over acoustic word embeddings, blocked Gibbs sampling -- on the device.

RNG protocol.  The reference consumes the process-global Python `random`
stream: `random.shuffle(utt_order)` once per sweep, then per utterance one `random.random()` per
backward-sampling step followed by one per new segment assignment.  Here a block of uniforms is
pre-drawn from the same stream, handed to the device, consumed there through a cursor in exactly
that order, and afterwards the host stream is rewound and advanced by the number actually
consumed -- so seeded runs stay aligned with the reference draw for draw.
"""
import logging
import os
import math
import random
import time

import numpy as np

from . import rng
from .device import DeviceCorpus, to_dev
from .kmeans import _consecutive
from .kmeans_acoustic_wordseg import _dp_tri
from .utterances import Utterances, process_embeddings  # noqa: F401  (re-exported as in the reference)

logger = logging.getLogger(__name__)
i_debug_monitor = 0
debug_gibbs_only = False


class UnigramAcousticWordseg(object):
    def __init__(self, am_class, am_alpha, am_K, am_param_prior, embedding_mats, vec_ids_dict, durations_dict,
                 landmarks_dict, seed_boundaries_dict=None, seed_assignments_dict=None, covariance_type="fixed",
                 n_slices_min=0, n_slices_max=20, min_duration=0, p_boundary_init=0.5, beta_sent_boundary=2.0,
                 lms=1., wip=0., fb_type="standard", init_am_assignments="rand", time_power_term=1.,
                 sync="sequential", n_gibbs_blocks=8, n_stat_blocks=8, batch_seed=0, process_group=None,
                 score_precision="f64"):
        """Same arguments as the reference (unigram_acoustic_wordseg.py:107-123), plus the execution
        mode: sync="sequential" is the reference's serial chain (draw for draw); sync="batch" the
        batch-synchronous blocked Gibbs sampler specified in oracle/np_fbgmm_batch.py
        (`n_gibbs_blocks` steps per sweep, statistics summed over `n_stat_blocks` slices, sharded
        over the ranks of `process_group` when torch.distributed is initialised).
        score_precision="f32" / "f16" (batch mode, fixed-variance components) evaluates the span
        scores on the matrix cores (fp32 MFMA, or two-way fp16 splits of the fp32 operands on the
        16-bit pipe) -- within the 1e-4 tolerance of the path, 5x / 10x faster; with diagonal
        components "f32" evaluates the Student-t terms in float32 with the hardware logarithm (same
        tolerance); "f64" reproduces the specification to the last draw.
        covariance_type="full" (D <= 64) is constructed with sync="sequential" and beta_sent_boundary=-1 only.  Its serial
        chain is the launches per utterance, the span scores of an utterance's triangle a lane per row (segk_fullcov.hip).
        Its batch sweeps (fp64 scores, one process) are reached from such an object: pass n_gibbs_blocks / n_stat_blocks /
        batch_seed here, then batch_sweep_async() / materialise(), or gibbs_sample(..., sync="batch")."""
        logger.info("Initializing")
        assert sync in ("sequential", "batch")
        if covariance_type == "full" and sync == "batch":
            raise NotImplementedError("the batch sampler is not reached through the constructor's sync='batch' with "
                                      "covariance_type='full': construct with sync='sequential' (and n_gibbs_blocks, "
                                      "n_stat_blocks, batch_seed), then call gibbs_sample(..., sync='batch') or "
                                      "batch_sweep_async() / materialise()")
        if covariance_type == "full" and beta_sent_boundary != -1:
            # (calc_p_continue asserts for any other value, here and in the reference: no sweep could run.  The other
            # covariance types keep the reference's behaviour -- construct, then fail at the first sweep --; for the
            # type this package added later the unusable configuration is refused where it is made.)
            raise NotImplementedError("full-covariance components in the unigram segmenter need beta_sent_boundary=-1: "
                                      "calc_p_continue supports no other value (unigram_acoustic_wordseg.py:513-531)")
        self.sync = sync
        self._batch_args = (n_gibbs_blocks, n_stat_blocks, batch_seed, process_group, score_precision)
        self._sweeper = None
        assert seed_assignments_dict is None or seed_boundaries_dict is not None
        self.n_slices_min = n_slices_min
        self.n_slices_max = n_slices_max
        self.min_duration = min_duration
        self.beta_sent_boundary = beta_sent_boundary
        self.wip = wip
        self.time_power_term = time_power_term
        self.set_fb_type(fb_type)

        embeddings, vec_ids, ids_to_utterance_labels = process_embeddings(embedding_mats, vec_ids_dict)
        self.ids_to_utterance_labels = ids_to_utterance_labels
        self._row_start = vec_ids.row_start
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
        u = self.utterances
        # (banded span tables: what the segmentation kernels read when no embedding lies outside the window)
        self._corpus = DeviceCorpus(embeddings, u.vec_ids, u.durations, u.lengths, band=u.complete_band_tables(n_slices_max))

        init_embeds = []
        for i in range(u.D):
            init_embeds.extend(u.get_segmented_embeds_i(i))
        init_embeds = np.array(init_embeds, dtype=int)
        init_embeds = init_embeds[np.where(init_embeds != -1)]

        assignments = -1 * np.ones(N, dtype=int)
        am_kw = dict(covariance_type=covariance_type, lms=lms, _corpus=self._corpus)
        if seed_assignments_dict is not None:                     # unigram_acoustic_wordseg.py:176-204
            self.seed_to_cluster = {}
            i_cluster = 0
            for i_utt, utt in enumerate(ids_to_utterance_labels):
                utt_init_embeds = np.array(u.get_segmented_embeds_i(i_utt), dtype=int)
                utt_init_assignments = np.array(seed_assignments_dict[utt][:])
                utt_init_assignments = utt_init_assignments[np.where(utt_init_embeds != -1)]
                utt_init_embeds = utt_init_embeds[np.where(utt_init_embeds != -1)]
                for seed in utt_init_assignments:
                    if seed not in self.seed_to_cluster:
                        if isinstance(seed, (int, np.integer)):
                            self.seed_to_cluster[seed] = seed
                        else:
                            self.seed_to_cluster[seed] = i_cluster
                            i_cluster += 1
                assignments[utt_init_embeds] = [self.seed_to_cluster[i] for i in utt_init_assignments]
            if am_K is None:
                am_K = max(self.seed_to_cluster.values()) + 1
            else:
                assert am_K >= max(self.seed_to_cluster.values()) + 1
            self.acoustic_model = am_class(embeddings, am_param_prior, am_alpha, am_K, assignments, **am_kw)
        elif init_am_assignments == "rand":                       # :206-223
            assignments[init_embeds] = _consecutive(np.random.randint(0, am_K, len(init_embeds)))
            self.acoustic_model = am_class(embeddings, am_param_prior, am_alpha, am_K, assignments, **am_kw)
        elif init_am_assignments == "one-by-one":                 # :225-236
            self.acoustic_model = am_class(embeddings, am_param_prior, am_alpha, am_K, assignments, **am_kw)
            for i_embed in init_embeds:
                self.acoustic_model.gibbs_sample_inside_loop_i(i_embed)
        else:
            assert False, "invalid value for `init_am_assignments`: " + init_am_assignments

        self._df = self.acoustic_model.components.dev
        self._dev_bounds = to_dev(u.boundaries.astype(np.uint8))
        u.bind_device(self._dev_bounds)

    def set_fb_type(self, fb_type):
        self.fb_type = fb_type
        if fb_type == "standard":
            self.fb_func = forward_backward
        elif fb_type == "viterbi":
            self.fb_func = forward_backward_viterbi
        else:
            assert False, "invalid `fb_type`: " + fb_type

    # ------------------------------------------------------------------ RNG stream plumbing
    def _open_stream(self, utts):
        """Pre-draw the uniforms a visit of `utts` can consume at most (two per landmark)."""
        n = int(sum(2 * self.utterances.lengths[i] for i in utts)) + 2
        self._rng_state = random.getstate()
        self._df.set_uniform_stream(np.array([random.random() for _ in range(n)]))

    def _close_stream(self):
        used = int(self._df.ucursor.item())
        random.setstate(self._rng_state)
        for _ in range(used):
            random.random()
        return used

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
            from .device import FbgmmBatchSweeper
            B, S, seed, group, prec = self._batch_args
            self._sweeper = FbgmmBatchSweeper(self._df, self._row_start, B, S, seed, group, prec)
        return self._sweeper

    def batch_sweep_async(self, anneal_temp=1, anneal_gibbs_am=False):
        """Enqueue one batch-synchronous sweep -- sampling with fb_type "standard", the MAP boundaries and slots with
        "viterbi" (the temperatures then have no effect); results stay on the device."""
        self._get_sweeper().sweep(self._dev_bounds, self.n_slices_min, self.n_slices_max, self.wip,
                                  self.time_power_term, anneal_temp, anneal_temp if anneal_gibbs_am else 1.0,
                                  viterbi=self.fb_type == "viterbi")
        self.utterances.mark_device_dirty()

    def am_batch_sweep_async(self, anneal_temp=1, score_precision=None):
        """Enqueue one ACOUSTIC-MODEL batch sweep: the boundaries stay, every current token is resampled (the batch form of
        the inner sweeps `acoustic_model.gibbs_sample(1, consider_unassigned=False)`); results stay on the device.
        score_precision: the precision of this sweep's token likelihoods -- None / "f64", or "f32" for diagonal components (on
        a segmenter of either `score_precision`; statistics and draws stay fp64)."""
        self._get_sweeper().am_sweep(self._dev_bounds, anneal_temp, score_precision)

    def materialise(self):
        """Bring the reference's view (components.K / assignments / statistics) up to date with the
        batch state."""
        if self._sweeper is not None:
            self._sweeper.materialise(self._dev_bounds)
            self.utterances.mark_device_dirty()

    def _leave_batch(self):
        if self._sweeper is not None and self._sweeper.in_batch_state:
            self.materialise()
            self._sweeper.invalidate()

    # ------------------------------------------------------------------ held-out utterances
    def decode(self, embedding_mats, vec_ids_dict, durations_dict, landmarks_dict, device_out=False):
        """Segment and label HELD-OUT utterances, read-only (specification tests/wordseg_decode.py; segk_fbd_decode,
        DESIGN.md 4.23).  The four dictionaries are the constructor's, for utterances that are in no model: their candidate
        embeddings are unassigned items appended to X, seen against the statistics of all tokens that hold a component.
        Per utterance, with the model's n_slices_min / n_slices_max / min_duration / wip / time_power_term / lms / alpha:
        the span scores of get_vec_embed_log_probs (:474-511) on the held-out log density of FBGMM.score_samples, the
        boundaries and log probability of forward_backward_viterbi (:759-864), and for every chosen segment
        map_assign_i's choice for its embedding (no lms) in the reference view's numbering, as FBGMM.predict reports it: an
        active component its index, K for "would found a new component".

        One deliberate difference from a serial Viterbi visit (gibbs_sample_i with fb_type "viterbi"): every segment is
        labelled independently against the same frozen statistics -- nothing is added to the bank between segments, and the
        model is not changed at all.  No uniform is consumed (`random` and `np.random` stay where they are); fb_type and the
        temperatures play no part.  A chosen segment whose span has no embedding (only after the DP stepped back from a dead
        end) is kept with embedding -1, label -1 and log density -inf.

        Returns a `Decoded`; with device_out=True its arrays are device tensors, enqueued without a synchronisation (the flat
        segment arrays then have n_utt * N_max entries, the first seg_offsets[-1] of them segments).
        Raises SegkError before any launch for: beta_sent_boundary != -1, more than one rank, a held-out D other than the
        model's, D > 256, full-covariance components beyond D <= 64 / K_max <= 1024, and a held-out corpus with an
        utterance of more than 64 landmarks without a window of 1..64 slices that holds every embedding and fits LDS."""
        labels, cq = self._heldout_corpus(embedding_mats, vec_ids_dict, durations_dict, landmarks_dict)
        out = self._decode_corpus(labels, cq)
        return out if device_out else out.numpy()

    def _heldout_corpus(self, embedding_mats, vec_ids_dict, durations_dict, landmarks_dict):
        """The checks of decode() and the device image of the held-out utterances: (sorted keys, DeviceCorpus or None for an
        empty set).  Host work and one upload; nothing of the model is read on the device."""
        from ._abi import SegkError
        if self.beta_sent_boundary != -1:
            raise SegkError("decode needs beta_sent_boundary=-1: calc_p_continue supports no other value "
                            "(unigram_acoustic_wordseg.py:513-531)")
        sw = self._get_sweeper()
        if not embedding_mats:
            sw.check_decode(self._corpus.D, 0, 0, self.n_slices_min, self.n_slices_max)
            return [], None
        embeddings, vec_ids, labels = process_embeddings(embedding_mats, vec_ids_dict)
        embeddings = np.asarray(embeddings)
        D = embeddings.shape[1] if embeddings.ndim == 2 else -1
        lengths = [len(landmarks_dict[i]) for i in labels]
        u = Utterances(lengths, vec_ids, [durations_dict[i] for i in labels], [landmarks_dict[i] for i in labels],
                       p_boundary_init=0, n_slices_min=self.n_slices_min, n_slices_max=self.n_slices_max,
                       min_duration=self.min_duration)
        band = u.complete_band_tables(self.n_slices_max)
        sw.check_decode(D, u.N_max, band[0].shape[2] if band is not None else 0, self.n_slices_min, self.n_slices_max)
        if u.vec_ids.max(initial=-1) >= len(embeddings):
            raise SegkError("decode: a span id names row %d of %d held-out embeddings" % (u.vec_ids.max(), len(embeddings)))
        return labels, DeviceCorpus(embeddings.astype(self._corpus.x_np_dtype, copy=False), u.vec_ids, u.durations, u.lengths,
                                    band=band)

    def _decode_corpus(self, labels, cq):
        """decode() on the device image of the held-out utterances: a `Decoded` of device tensors, nothing read back."""
        import torch
        sw = self._get_sweeper()
        if cq is None:
            e_i, e_f = np.zeros(0, np.int64), np.zeros(0)
            return Decoded([], np.zeros((0, 0), bool), e_f, np.zeros(1, np.int64), e_i, e_i, e_i, e_i, e_f,
                           int(sw.totals()[2]) if sw.in_batch_state else int(self.acoustic_model.components.K))
        o = sw.decode(cq, self._dev_bounds, self.n_slices_min, self.n_slices_max, self.wip, self.time_power_term)
        # segment j of utterance i ends behind its j-th set flag and starts where segment j - 1 ends; the flat arrays are the
        # rows' first n_seg entries in utterance order (stable sorts: nothing is read back)
        n_utt, NM = o["boundaries"].shape
        flags = o["boundaries"] != 0
        end = torch.sort((~flags).to(torch.int8), dim=1, stable=True).indices + 1
        start = torch.cat([torch.zeros_like(end[:, :1]), end[:, :-1]], dim=1)
        valid = torch.arange(NM, device=end.device)[None, :] < o["n_seg"][:, None]
        order = torch.sort((~valid).flatten().to(torch.int8), stable=True).indices
        flat = [t.flatten().index_select(0, order) for t in (start, end, o["seg_embed"].long(), o["seg_label"].long(),
                                                              o["seg_density"])]
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=end.device), torch.cumsum(o["n_seg"].long(), 0)])
        return Decoded(labels, flags, o["log_prob"], offsets, *flat, K=o["K"])

    # ------------------------------------------------------------------ one utterance
    def _gibbs_i_async(self, i, anneal_temp, anneal_gibbs_am):
        viterbi = self.fb_type == "viterbi"
        log_p_continue = math.log(self.calc_p_continue())
        self._df.gibbs_utt(self._dev_bounds, i, viterbi, self.n_slices_min, self.n_slices_max, self.wip,
                           self.time_power_term, log_p_continue, anneal_temp,
                           anneal_temp if anneal_gibbs_am else 1.0)
        self.utterances.mark_device_dirty()

    def gibbs_sample_i(self, i, anneal_temp=1, anneal_gibbs_am=False):
        """unigram_acoustic_wordseg.py:252-360."""
        self._leave_batch()
        self._open_stream([i])
        self._gibbs_i_async(i, anneal_temp, anneal_gibbs_am)
        self._close_stream()
        self._df.check_status()
        return float(self._df.out_logprob[i].item())

    # ------------------------------------------------------------------ sweeps
    def gibbs_sample(self, n_iter, am_n_iter=0, anneal_schedule=None, anneal_start_temp_inv=0.1,
                     anneal_end_temp_inv=1, n_anneal_steps=-1, anneal_gibbs_am=False, sync=None, am_sync=None,
                     am_score_precision=None):
        """unigram_acoustic_wordseg.py:362-472; same record keys.  sync: None = the mode the object was built with; "batch" /
        "sequential" = the sweeps of this call in that mode (the two modes mix freely: every switch rebuilds the state the
        other one reads).  am_sync: how the `am_n_iter` inner sweeps of the acoustic model run -- None / "sequential": the
        reference's serial chain over the assigned tokens (batch mode is left for it); "batch" (with sync "batch" only):
        `am_n_iter` acoustic-model batch sweeps at temperature 1 (the reference's inner sweeps are not annealed) without
        leaving batch mode; they always sample, whatever the fb_type.  am_score_precision (with am_sync "batch" only): the
        precision of the inner sweeps' token likelihoods, passed to every one of them (am_batch_sweep_async)."""
        import torch
        assert sync in (None, "sequential", "batch")
        sync = self.sync if sync is None else sync
        assert am_sync in (None, "sequential", "batch")
        assert am_sync != "batch" or sync == "batch", "am_sync=\"batch\" runs inside batch mode: it needs sync=\"batch\""
        assert am_score_precision is None or am_sync == "batch", \
            "am_score_precision is the precision of the batch inner sweeps: it needs am_sync=\"batch\""
        if anneal_schedule is None:
            get_anneal_temp = iter([])
        elif anneal_schedule == "linear":
            if n_anneal_steps == -1:
                n_anneal_steps = n_iter
            get_anneal_temp = iter(1. / np.linspace(anneal_start_temp_inv, anneal_end_temp_inv, n_anneal_steps))
        elif anneal_schedule == "step":
            assert not n_anneal_steps == -1, "`n_anneal_steps` of -1 not allowed for step annealing schedule"
            n_iter_per_step = int(round(float(n_iter) / n_anneal_steps))
            anneal_list = 1. / np.linspace(anneal_start_temp_inv, anneal_end_temp_inv, n_anneal_steps)
            get_anneal_temp = iter(np.repeat(anneal_list, n_iter_per_step))
        else:
            assert False, "invalid anneal_schedule"

        record_dict = {k: [] for k in ["sample_time", "log_marg", "log_marg*length", "log_prob_z",
                                       "log_prob_X_given_z", "anneal_temp", "components", "n_tokens"]}
        am = self.acoustic_model
        for i_iter in range(n_iter):
            start_time = time.time()
            if am_n_iter > 0 and am_sync == "batch":
                for _ in range(am_n_iter):
                    self.am_batch_sweep_async(score_precision=am_score_precision)
            elif am_n_iter > 0:                                   # unigram_acoustic_wordseg.py:440-443
                self._leave_batch()
                self.acoustic_model.gibbs_sample(am_n_iter, consider_unassigned=False)
            anneal_temp = next(get_anneal_temp, anneal_end_temp_inv)
            if sync == "batch":
                self.batch_sweep_async(anneal_temp, anneal_gibbs_am)
                torch.cuda.synchronize()
                self._df.check_status()
                log_prob = float(np.sum(self._get_sweeper().utt_values(self._df.out_logprob)))
                self.materialise()                                # the record metrics read the reference's view
            else:
                self._leave_batch()
                utt_order = list(range(self.utterances.D))
                rng.shuffle(utt_order)
                if debug_gibbs_only:
                    utt_order = [i_debug_monitor]
                self._open_stream(utt_order)
                # the whole chain of the sweep by one library call (a persistent kernel per stretch of utterances between two
                # emptied components) where it applies; SEGK_SEQ_PER_UTT=1 / SEGK_FB_CHAIN=0 keep the four launches per utterance
                whole = os.environ.get("SEGK_SEQ_PER_UTT", "0") != "1" and not debug_gibbs_only and self._df.sequential_sweep(
                    self._dev_bounds, utt_order, self._row_start, self.fb_type == "viterbi", self.n_slices_min, self.n_slices_max,
                    self.wip, self.time_power_term, math.log(self.calc_p_continue()), anneal_temp,
                    anneal_temp if anneal_gibbs_am else 1.0)
                if whole:
                    self.utterances.mark_device_dirty()
                else:
                    for i_utt in utt_order:
                        self._gibbs_i_async(i_utt, anneal_temp, anneal_gibbs_am)
                torch.cuda.synchronize()
                self._close_stream()
                self._df.check_status()
                lps = self._df.out_logprob.cpu().numpy()
                log_prob = 0
                for i_utt in utt_order:
                    log_prob += lps[i_utt]

            record_dict["sample_time"].append(time.time() - start_time)
            # the record metrics (fbgmm.py:208-225, components.log_marg) in one device call instead of numpy on host
            # snapshots of the assignments; SEGK_HOST_METRICS=1 keeps the host expressions (tests compare the two)
            if os.environ.get("SEGK_HOST_METRICS", "0") == "1":
                lpz, lpx, n_comp, n_tok = am.log_prob_z(), am.log_prob_X_given_z(), am.components.K, am.get_n_assigned()
            else:
                lpz, lpx, n_comp, n_tok = self._df.record_metrics()
            record_dict["log_marg"].append(lpz + lpx)
            record_dict["log_marg*length"].append(log_prob)
            record_dict["log_prob_z"].append(lpz)
            record_dict["log_prob_X_given_z"].append(lpx)
            record_dict["anneal_temp"].append(anneal_temp)
            record_dict["components"].append(n_comp)
            record_dict["n_tokens"].append(n_tok)
            info = "iteration: " + str(i_iter)
            for key in sorted(record_dict):
                info += ", " + key + ": " + str(record_dict[key][-1])
            logger.info(info)
        return record_dict

    # ------------------------------------------------------------------ helpers of the reference API
    def get_vec_embed_log_probs(self, vec_ids, durations):
        """unigram_acoustic_wordseg.py:474-511."""
        vec_ids = np.asarray(vec_ids)
        out = -np.inf * np.ones(len(vec_ids))
        valid = np.where(vec_ids != -1)[0]
        if len(valid):
            lm = self._df.log_marg_rows(vec_ids[valid])
            d = np.asarray(durations, dtype=np.float64)[valid]
            with np.errstate(invalid="ignore"):
                out[valid] = np.where(np.isnan(d), -np.inf, lm * d ** self.time_power_term)
        return out + self.wip

    def calc_p_continue(self):
        """unigram_acoustic_wordseg.py:513-531 (only beta_sent_boundary == -1 works in the reference)."""
        if self.beta_sent_boundary != -1:
            assert False, "to check"
        return 1.0

    def get_unsup_transcript_i(self, i):
        return list(self.acoustic_model.components.get_assignments(self.utterances.get_segmented_embeds_i(i)))

    def get_log_margs_i(self, i):
        """unigram_acoustic_wordseg.py:539-564."""
        comps = self.acoustic_model.components
        segmented_embeds = self.utterances.get_segmented_embeds_i(i)
        assignments = comps.get_assignments(segmented_embeds)
        for e in segmented_embeds:
            if e == -1:
                continue
            comps.del_item(e)
        log_margs = [self.acoustic_model.log_marg_i(j) for j in segmented_embeds if j != -1]
        for e, k in zip(segmented_embeds, assignments):
            comps.add_item(e, k)
        return log_margs


class Decoded(object):
    """What UnigramAcousticWordseg.decode returns.  utterance_labels: the sorted keys; boundaries bool [n_utt, N_max];
    log_prob [n_utt]: the DP totals; segments i: the flat entries seg_offsets[i] .. seg_offsets[i + 1] - 1 of seg_start /
    seg_end (landmark indices: the segment spans the slices [start, end)), seg_embed (row of the stacked held-out matrix,
    utterances in sorted-key order; -1: no embedding), seg_label (the reference view's numbering; K: "would found a new
    component"; -1: no embedding) and seg_log_marg (the held-out log density of the embedding; -inf: none); K: the active
    components at the time of the call."""

    _fields = ("boundaries", "log_prob", "seg_offsets", "seg_start", "seg_end", "seg_embed", "seg_label", "seg_log_marg", "K")

    def __init__(self, utterance_labels, boundaries, log_prob, seg_offsets, seg_start, seg_end, seg_embed, seg_label,
                 seg_log_marg, K):
        self.utterance_labels = list(utterance_labels)
        self.boundaries, self.log_prob, self.seg_offsets = boundaries, log_prob, seg_offsets
        self.seg_start, self.seg_end, self.seg_embed = seg_start, seg_end, seg_embed
        self.seg_label, self.seg_log_marg, self.K = seg_label, seg_log_marg, K

    def numpy(self):
        """The host form (waits for the device): NumPy arrays, the flat arrays cut to the segments, K an int."""
        if isinstance(self.K, int):
            return self
        h = {k: getattr(self, k).cpu().numpy() for k in self._fields}
        n = int(h["seg_offsets"][-1])
        for k in ("seg_start", "seg_end", "seg_embed", "seg_label", "seg_log_marg"):
            h[k] = h[k][:n]
        h["K"] = int(h["K"])
        return Decoded(self.utterance_labels, **h)

    def transcript(self, i):
        """The labels of utterance i's segments, in order (a list of ints; reads the device arrays back if need be)."""
        r = self.numpy()
        return [int(k) for k in r.seg_label[r.seg_offsets[i]:r.seg_offsets[i + 1]]]


def _with_rng_stream(N, run):
    """Pre-draw N+1 uniforms, run, rewind and advance by the number consumed."""
    state = random.getstate()
    u = [random.random() for _ in range(N + 1)]
    result, used = run(u)
    random.setstate(state)
    for _ in range(used):
        random.random()
    return result


def forward_backward(vec_embed_log_probs, log_p_continue, N, n_slices_min=0, n_slices_max=0, i_utt=None,
                     anneal_temp=1):
    """unigram_acoustic_wordseg.py:653-756 on the device (consumes `random` like the reference)."""
    def run(u):
        tot, bounds, nd, st = _dp_tri(2, vec_embed_log_probs, N, n_slices_min, n_slices_max, log_p_continue,
                                      anneal_temp, u)
        if st:
            raise AssertionError("log_prob == -inf")
        return (np.float64(tot), bounds), nd
    return _with_rng_stream(N, run)


def forward_backward_viterbi(vec_embed_log_probs, log_p_continue, N, n_slices_min=0, n_slices_max=0, i_utt=None,
                             anneal_temp=None):
    """unigram_acoustic_wordseg.py:759-864 on the device."""
    tot, bounds, _, _ = _dp_tri(1, vec_embed_log_probs, N, n_slices_min, n_slices_max)
    return tot, bounds

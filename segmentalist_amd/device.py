"""
Device-resident state of the hot path and thin wrappers over the C ABI (include/segk.h).

PyTorch is used for exactly three things here: allocating device buffers, host<->device
copies, and the stream handle.  All arithmetic of the hot path runs in libsegk.so.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import SEGK_F32, SEGK_F64, SegkError, check, ptr
from .comm import SingleComm, get_comm

# FbgmmBatchSweeper.am_sweep(..., score_precision="f32"): the token bound of a block (the landmarks of its utterances over the
# local slices) from which the tile kernel (segk_fbt_assign_diag32) takes the step; below it segk_fbb_assign_diag32 on the
# unchanged token lists does.  Measured, not guessed (profiles/README.md "Acoustic-model batch sweeps in float32", DESIGN.md
# 4.17.1): at D 39, K_max 100 the other route wins up to a bound of 10 080 landmarks per block (by 0.07 ms a sweep, the larger
# range 0.05) and the tiles win from 20 000 on (by 0.22 ms); the constant is the middle of the two.  SEGK_AM32_TILE_MIN
# overrides it per sweep.
AM32_TILE_MIN = 15000


def _torch():
    import torch
    return torch


def _dev():
    torch = _torch()
    if not torch.cuda.is_available():
        raise SegkError("segmentalist_amd needs an MI355X: no ROCm device is visible and there is no "
                        "CPU fallback for the hot path")
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(a, dtype=None):
    torch = _torch()
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))
    return torch.from_numpy(a).to(_dev())


def _host_init_stats(X, assignments, K_max, random_means):
    """KMeansComponents.__init__'s statistics (kmeans_components.py:79-81: add_item for k ascending, i ascending within k) on
    the host, exactly as k_kmeans_init_stats computes them on the device -- float64 sums of a component's rows in ascending row
    order, means = the float64 quotient rounded to the dtype of X, empty slots = the random means --, for the ranks of a
    sharded corpus, none of which holds every row on its device."""
    X = np.asarray(X)
    a = np.asarray(assignments, dtype=np.int64)
    D = X.shape[1]
    numer = np.zeros((K_max, D), dtype=np.float64)
    counts = np.zeros(K_max, dtype=np.int64)
    means = np.array(random_means, dtype=X.dtype, copy=True)
    rows = np.flatnonzero((a >= 0) & (a < K_max))
    order = rows[np.argsort(a[rows], kind="stable")]          # by component, ascending rows inside a component
    ks, starts = np.unique(a[order], return_index=True)
    ends = np.append(starts[1:], len(order))
    for k, s, e in zip(ks, starts, ends):
        numer[k] = np.cumsum(X[order[s:e]].astype(np.float64), axis=0)[-1]      # cumsum: strictly sequential additions
        counts[k] = e - s
        means[k] = (numer[k] / float(e - s)).astype(X.dtype)
    K = int(ks.max()) + 1 if len(ks) else 0
    return means, numer, counts, K


class DeviceCorpus(object):
    """Device image of the embedding matrix and (optionally) of `Utterances`
    (utterances.py:74-105): vec_ids int32 [n_utt, tri], durations f64, lengths int32."""

    def __init__(self, X, vec_ids=None, durations=None, lengths=None, band=None):
        torch = _torch()
        X = np.asarray(X)
        if X.dtype not in (np.float32, np.float64):
            X = X.astype(np.float64)
        assert X.ndim == 2
        self.x_np_dtype = X.dtype
        self.x_dtype = SEGK_F32 if X.dtype == np.float32 else SEGK_F64
        self.n_emb, self.D = X.shape
        if self.n_emb >= 2 ** 31:
            raise SegkError("more than 2^31 embeddings are not supported (int32 row ids)")
        self.ld32 = (self.D + 3) // 4 * 4
        dev = _dev()
        if self.x_dtype == SEGK_F32 and self.ld32 == self.D:
            self.X = to_dev(X)
            self.X32 = self.X
            self.ldx = self.D
            x32_out = None
        else:
            self.X = to_dev(X)
            self.ldx = self.D
            self.X32 = torch.empty((self.n_emb, self.ld32), dtype=torch.float32, device=dev)
            x32_out = self.X32
        self.xnorm = torch.empty(self.n_emb, dtype=torch.float32, device=dev)
        if vec_ids is not None:
            vec_ids = np.asarray(vec_ids)
            self.n_utt = vec_ids.shape[0]
            self.lengths_np = np.asarray(lengths, dtype=np.int32)
            self.N_max = int(self.lengths_np.max())
            tri = self.N_max * (self.N_max + 1) // 2
            assert vec_ids.shape[1] == tri
            self.vec_ids = to_dev(vec_ids, np.int32)
            self.durations = to_dev(durations, np.float64)
            self.lengths = to_dev(self.lengths_np)
        else:
            self.n_utt, self.N_max = 0, 0
            self.vec_ids = self.durations = self.lengths = None
            self.lengths_np = None
        self.tri = self.N_max * (self.N_max + 1) // 2
        # banded span tables (ids int32 [n_utt, N_max, W], durations f64): what the per-utterance kernels read
        self.band_ids = self.band_dur = None
        self.band_W = 0
        if band is not None and vec_ids is not None:
            bi, bd = band
            assert bi.shape == bd.shape == (self.n_utt, self.N_max, bi.shape[2])
            self.band_ids, self.band_dur, self.band_W = to_dev(bi, np.int32), to_dev(bd, np.float64), int(bi.shape[2])
        # fp16x2 image of the rows for the k-means filter (float32 data, 8 <= D <= 128); built on demand
        self.Xb3 = None
        self.c = _abi.Corpus(
            X=self.X.data_ptr(), X32=self.X32.data_ptr(), x_dtype=self.x_dtype, D=self.D,
            n_emb=self.n_emb, ldx=self.ldx, ld32=self.ld32, xnorm=self.xnorm.data_ptr(),
            vec_ids=self.vec_ids.data_ptr() if self.vec_ids is not None else None,
            durations=self.durations.data_ptr() if self.durations is not None else None,
            lengths=self.lengths.data_ptr() if self.lengths is not None else None,
            n_utt=self.n_utt, N_max=self.N_max, band_W=self.band_W,
            band_ids=self.band_ids.data_ptr() if self.band_ids is not None else None,
            band_dur=self.band_dur.data_ptr() if self.band_dur is not None else None)
        check(_abi.lib().segk_corpus_prepare(_abi.ctx(), C.byref(self.c), ptr(x32_out), ptr(self.xnorm),
                                             _abi.stream()))

    def ensure_b3(self):
        """The rows split into two fp16 pieces (segk_corpus_prepare_b3) for the split-precision k-means
        filter: SEGK_SCORE_B3=2 (default) builds them; 0 (or any other value) keeps the fp32 MFMA filter."""
        import os
        pieces = int(os.environ.get("SEGK_SCORE_B3", "2") or 2)
        if pieces != 2:
            return False
        if self.Xb3 is None and self.x_dtype == SEGK_F32 and 8 <= self.D <= 128:
            torch = _torch()
            nbytes = int(_abi.lib().segk_corpus_b3_bytes(self.n_emb, self.D))
            self.Xb3 = torch.empty(nbytes, dtype=torch.uint8, device=self.X.device)
            check(_abi.lib().segk_corpus_prepare_b3(_abi.ctx(), C.byref(self.c), ptr(self.Xb3), pieces, _abi.stream()))
            self.c.Xb3 = self.Xb3.data_ptr()
            self.c.sp_pieces = pieces
        return self.Xb3 is not None

    @property
    def torch_xdtype(self):
        torch = _torch()
        return torch.float32 if self.x_dtype == SEGK_F32 else torch.float64


class DeviceKMeans(object):
    """Device image of `KMeansComponents` (kmeans_components.py:18-91) plus the derived MFMA
    operands and the per-sweep work buffers."""

    def __init__(self, corpus, K_max, assignments, random_means, shard=None):
        torch = _torch()
        dev = _dev()
        self.corpus = corpus
        c = corpus
        self.K_max = int(K_max)
        # shard = (row_lo, row_hi, X_host): `corpus` holds the rows [row_lo, row_hi) of the embedding matrix, numbered from 0
        # (multi-rank batch mode, SURVEY 8(e): "each GPU keeps its shard's X rows").  Everything row-indexed on the device --
        # the span tables' ids, token lists, candidates, `assignments` -- is then in that LOCAL numbering; the host-facing
        # views (components.assignments, checkpoints) are assembled from all ranks.  Component statistics are replicated.
        self.row_base, self.n_rows_global, self.shard = 0, c.n_emb, None
        assignments = np.asarray(assignments)
        init = None
        if shard is not None:
            lo, hi, X_host = shard
            assert hi - lo == c.n_emb and len(assignments) == X_host.shape[0]
            self.row_base, self.n_rows_global, self.shard = lo, len(assignments), (lo, hi)
            init = _host_init_stats(X_host, assignments, self.K_max, np.asarray(random_means, dtype=c.x_np_dtype))
            assignments = assignments[lo:hi]
        xd = c.torch_xdtype
        self.means = torch.empty((self.K_max, c.D), dtype=xd, device=dev)
        self.mean_numerators = torch.zeros((self.K_max, c.D), dtype=torch.float64, device=dev)
        self.counts = torch.zeros(self.K_max, dtype=torch.int64, device=dev)
        self.random_means = to_dev(np.asarray(random_means, dtype=c.x_np_dtype))
        self.assignments = to_dev(assignments, np.int32)
        self.K = torch.zeros(1, dtype=torch.int32, device=dev)
        n_tiles_f = _abi.lib().segk_kmeans_tiles_floats(self.K_max, c.D)
        self.tiles = torch.zeros(int(n_tiles_f), dtype=torch.float32, device=dev)
        self.mnorm_max = torch.zeros(1, dtype=torch.float64, device=dev)
        self.tiles_b3 = None
        if c.ensure_b3():
            self.tiles_b3 = torch.zeros(int(_abi.lib().segk_kmeans_tiles_b3_floats(self.K_max, c.D)), dtype=torch.float32,
                                        device=dev)
        self.m = _abi.KMeansDev(
            tiles_b3=self.tiles_b3.data_ptr() if self.tiles_b3 is not None else None,
            means=self.means.data_ptr(), mean_numerators=self.mean_numerators.data_ptr(),
            counts=self.counts.data_ptr(), random_means=self.random_means.data_ptr(),
            assignments=self.assignments.data_ptr(), K=self.K.data_ptr(), K_max=self.K_max,
            tiles=self.tiles.data_ptr(), mnorm_max=self.mnorm_max.data_ptr())
        # candidates of the filter stage, indexed by embedding row
        self.cand_k = torch.zeros(c.n_emb, dtype=torch.int32, device=dev)
        self.cand_f = torch.zeros((c.n_emb, 2), dtype=torch.float32, device=dev)
        self.cand_s = torch.zeros(c.n_emb, dtype=torch.float64, device=dev)
        self.cand_queue = torch.zeros(c.n_emb, dtype=torch.int32, device=dev)
        self.cand_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.cand = _abi.CandDev(k=self.cand_k.data_ptr(), f=self.cand_f.data_ptr(), s=self.cand_s.data_ptr(),
                                 queue=self.cand_queue.data_ptr(), count=self.cand_count.data_ptr())
        self.status = torch.zeros(8, dtype=torch.int32, device=dev)
        self.assign_stale = None
        # multi-rank batch sweeps: the communicator of the sweeper (ensure_assignments / ensure_boundaries are
        # collectives on it) and the boundary buffer whose rows of other ranks' utterances are out of date
        self.batch_comm = SingleComm()
        self.bounds_stale = None
        self._L = _abi.lib()
        self._ctx = _abi.ctx()
        self._ctx_q = None           # the context held-out rows are scored on (_heldout_ctx), created at the first such call
        if init is None:
            check(self._L.segk_kmeans_init_stats(self._ctx, C.byref(c.c), C.byref(self.m), _abi.stream()))
        else:
            means, numer, counts, K = init
            self.means.copy_(torch.from_numpy(means))
            self.mean_numerators.copy_(torch.from_numpy(numer))
            self.counts.copy_(torch.from_numpy(counts))
            self.K.fill_(int(K))
            self.prepare()
        if c.n_utt:
            self._alloc_utt_buffers()

    # ------------------------------------------------------------------ buffers for segmentation
    def _alloc_utt_buffers(self):
        torch = _torch()
        dev = _dev()
        c = self.corpus
        nu, nm = c.n_utt, c.N_max
        self.old_tok = torch.zeros((nu, nm), dtype=torch.int32, device=dev)
        self.new_tok = torch.zeros((nu, nm), dtype=torch.int32, device=dev)
        self.new_k = torch.zeros((nu, nm), dtype=torch.int32, device=dev)
        self.n_old = torch.zeros(nu, dtype=torch.int32, device=dev)
        self.n_new = torch.zeros(nu, dtype=torch.int32, device=dev)
        self.n_flag = torch.zeros(nu, dtype=torch.int32, device=dev)
        self.out_total = torch.zeros(nu, dtype=torch.float64, device=dev)
        self.utt_arange = torch.arange(nu, dtype=torch.int32, device=dev)
        self.remap = torch.zeros(self.K_max, dtype=torch.int32, device=dev)
        self.out_scalars = torch.zeros(8, dtype=torch.float64, device=dev)
        self.refit_moved = torch.zeros(1, dtype=torch.int32, device=dev)      # tokens a batch refit relabelled (this rank's)
        # batch sweeps leave `assignments` untouched: `assign_stale` = (lo, hi, world) of the token
        # lists it must be rebuilt from, or None when it is current

    # ------------------------------------------------------------------ single calls
    def _cp(self):
        return C.byref(self.corpus.c)

    def require_whole_corpus(self, what):
        if self.shard is not None:
            raise SegkError("%s needs every row of the embedding matrix on this device, but the segmenter holds a shard (rows "
                            "%d..%d of %d): construct it with shard_corpus=False" % (what, self.shard[0], self.shard[1],
                                                                                     self.n_rows_global))

    def global_assignments(self):
        """`assignments` of ALL rows as a numpy array (a collective on the sweeper's communicator when anything is stale or
        the corpus is sharded: every rank contributes the labels of its own rows)."""
        self.ensure_assignments()
        a = self.assignments.cpu().numpy()
        if self.shard is None:
            return a
        out = np.full(self.n_rows_global, -1, dtype=a.dtype)
        for lo, hi, part in self.batch_comm.all_gather_object((self.shard[0], self.shard[1], a)):
            out[lo:hi] = part
        return out

    def set_global_assignments(self, a):
        """Upload `assignments` given for all rows (checkpoint resume)."""
        torch = _torch()
        a = np.asarray(a)
        if self.shard is not None:
            a = a[self.shard[0]:self.shard[1]]
        self.assignments.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(self.assignments.dtype))

    def ensure_assignments(self, group=None):
        """Materialise `assignments` after batch sweeps (they only maintain the token lists).  With more than
        one rank this is a COLLECTIVE on the sweeper's communicator (every rank holds the tokens of its own
        utterances only): all ranks must call it -- directly or through `components.assignments`,
        `sum_neg_sqrd_norm()`, `state_dict()` ... -- together."""
        if self.assign_stale is None:
            return
        lo, hi, world = self.assign_stale
        check(self._L.segk_kmeans_assignments_from_tokens(self._ctx, self._cp(), C.byref(self.m), lo, hi,
                                                          ptr(self.new_tok), ptr(self.new_k), ptr(self.n_new),
                                                          _abi.stream()))
        if world > 1 and self.shard is None:
            (self.batch_comm if group is None else get_comm(group)).all_reduce_max(self.assignments)
        self.assign_stale = None

    def ensure_boundaries(self):
        """After multi-rank batch sweeps every rank has resegmented its own utterances only: fetch the rows of
        the others (COLLECTIVE on the sweeper's communicator, like ensure_assignments), so that
        `utterances.boundaries`, transcripts and checkpoints are the same, complete state on every rank."""
        if self.bounds_stale is None:
            return
        bounds, pt = self.bounds_stale
        torch = _torch()
        mine = torch.zeros_like(bounds)
        mine[pt.utt_lo:pt.utt_hi] = bounds[pt.utt_lo:pt.utt_hi]
        self.batch_comm.all_reduce_max(mine)
        bounds.copy_(mine)
        self.bounds_stale = None

    def ensure_state(self):
        """Both of the above: what the sequential-mode entry points need after multi-rank batch sweeps (they read the
        old boundaries and labels of utterances other ranks own).  A collective when anything is stale."""
        self.ensure_assignments()
        self.ensure_boundaries()

    def prepare(self):
        check(self._L.segk_kmeans_prepare(self._ctx, self._cp(), C.byref(self.m), _abi.stream()))

    def score_rows(self, ids=None, row0=0, n=None, hint_remap=None, hint_identity=False):
        """A1 over rows (device int32 tensor `ids`, or the range row0..row0+n): afterwards
        cand_k / cand_s hold np.argmax / np.max of neg_sqrd_norm for those rows.
        hint_remap (device int32 [K_max]): cand_k of these rows holds what the previous call left there, in the labelling
        that table translates into the current one -- the library then verifies those hints against the dense filter values
        instead of tracking the winner's index (segk_kmeans_score_hinted); the results are the same bits either way.
        hint_identity: the same with cand_k already in the current labelling (no table)."""
        if ids is not None:
            n = ids.numel()
            p = ptr(ids)
        else:
            p = None
            n = self.corpus.n_emb - row0 if n is None else n
        if hint_remap is not None or hint_identity:
            check(self._L.segk_kmeans_score_hinted(self._ctx, self._cp(), C.byref(self.m), p, int(row0), int(n),
                                                   C.byref(self.cand), ptr(hint_remap), ptr(self.status), _abi.stream()))
            return
        check(self._L.segk_kmeans_score(self._ctx, self._cp(), C.byref(self.m), p, int(row0), int(n),
                                        C.byref(self.cand), ptr(self.status), _abi.stream()))

    # ------------------------------------------------------------------ held-out rows
    def check_heldout(self, D, what):
        """What scoring rows that are not in the model refuses, from host values alone (nothing is launched)."""
        if self.batch_comm.world > 1:
            raise SegkError("%s runs in one process only (%d ranks): held-out rows are not sharded" % (what, self.batch_comm.world))
        if self.shard is not None:
            raise SegkError("%s needs a model whose corpus is not sharded (this device holds rows %d..%d of %d)"
                            % (what, self.shard[0], self.shard[1], self.n_rows_global))
        if D != self.corpus.D:
            raise SegkError("%s: the held-out embeddings have D = %d, the model's have D = %d" % (what, D, self.corpus.D))

    def _heldout_ctx(self):
        """A second segk_ctx, this model's own: the score path's workspaces, the per-XCD shares, the hint feedback and the
        delta pass's base state belong to a context (include/segk.h, segk_kmeans_score_hinted), and every un-hinted score
        call drops the delta state of the context it runs on.  Held-out rows are scored here, so the context the sweeps run
        on never sees them."""
        if self._ctx_q is None:
            h = C.c_void_p()
            check(self._L.segk_create(int(_torch().cuda.current_device()), C.byref(h)))
            self._ctx_q = h
        return self._ctx_q

    def __del__(self):
        try:
            if self._ctx_q is not None:
                self._L.segk_destroy(self._ctx_q)
                self._ctx_q = None
        except Exception:
            pass

    def score_heldout(self, cq):
        """segk_kmeans_score, un-hinted, over all rows of `cq` -- a DeviceCorpus that is in no model, of the model's D and
        dtype -- against the means as they stand, on the model's second context and into candidate buffers of the call's
        own: returns (CandDev, its tensors k int32 [M], f, s float64 [M], queue, count, status): k / s = np.argmax / np.max
        of neg_sqrd_norm over all K_max rows.  Reads means, tiles and mnorm_max; writes nothing of the model: not cand_k
        (the next sweep's hints), not `status`.  Enqueued on the current stream, nothing read back."""
        torch = _torch()
        dev = _dev()
        self.check_heldout(cq.D, "scoring held-out rows")
        if cq.x_dtype != self.corpus.x_dtype:
            raise SegkError("scoring held-out rows: the held-out embeddings must have the dtype of the model's")
        if self.tiles_b3 is not None:
            cq.ensure_b3()
        M = cq.n_emb
        t = (torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros((M, 2), dtype=torch.float32, device=dev),
             torch.zeros(M, dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.int32, device=dev),
             torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev))
        cand = _abi.CandDev(k=t[0].data_ptr(), f=t[1].data_ptr(), s=t[2].data_ptr(), queue=t[3].data_ptr(), count=t[4].data_ptr())
        check(self._L.segk_kmeans_score(self._heldout_ctx(), C.byref(cq.c), C.byref(self.m), None, 0, int(M), C.byref(cand),
                                        ptr(t[5]), _abi.stream()))
        return cand, t

    @staticmethod
    def decode_lds_bytes(N_max, n_slices_max):
        """The LDS of one wave of k_kmd_decode (segk_kmdecode.hip kmd_lds)."""
        Wc = n_slices_max if 0 < n_slices_max < N_max else N_max
        cells = N_max * Wc
        if 1 <= n_slices_max <= 8 and N_max <= 64:
            b = (9 * N_max + 12) * 8 + (2 * cells + 2 * N_max + 8) * 4
        else:
            b = (cells + N_max + 1) * 8 + cells * 4 + N_max
        return (b + 15) // 16 * 16

    def check_decode(self, D, N_max, n_slices_min, n_slices_max):
        """What decode() refuses, from host values alone (nothing is launched): the limits of segk_kmd_decode, each named."""
        self.check_heldout(D, "decode")
        if n_slices_min not in (0, 1):
            raise SegkError("decode: n_slices_min must be 0 or 1, got %r" % (n_slices_min,))
        if n_slices_max < 0:
            raise SegkError("decode: n_slices_max must be >= 0, got %r" % (n_slices_max,))
        lds = self.decode_lds_bytes(N_max, n_slices_max)
        if lds > 160 * 1024:
            raise SegkError("decode: the band of spans of the longest held-out utterance does not fit in the LDS of a workgroup: "
                            "N_max = %d landmarks, n_slices_max = %d: %d bytes needed, %d available"
                            % (N_max, n_slices_max, lds, 160 * 1024))

    def decode(self, cq, n_slices_min, n_slices_max, wip):
        """Boundaries, objective and transcript of the HELD-OUT utterances of `cq` against the means as they stand --
        SegmentalKMeansWordseg.decode; specification tests/kmeans_decode.py; DESIGN.md 4.24: score_heldout, then
        segk_kmd_decode.  Returns a dict of device tensors, enqueued on the current stream, nothing read back: boundaries
        uint8 [n_utt, N_max], objective [n_utt], n_seg int32 [n_utt], seg_embed / seg_row / seg_label int32 and seg_score
        float64 [n_utt, N_max], row int32 / score float64 [M] (every candidate row), K (a copy of the model's).  Read-only:
        whatever ensure_state() has pending stays pending."""
        torch = _torch()
        dev = _dev()
        self.check_decode(cq.D, cq.N_max, int(n_slices_min), int(n_slices_max))
        n_utt, NM = cq.n_utt, cq.N_max
        cand, t = self.score_heldout(cq)
        i32 = torch.int32
        out = dict(boundaries=torch.zeros((n_utt, NM), dtype=torch.uint8, device=dev),
                   objective=torch.zeros(n_utt, dtype=torch.float64, device=dev), n_seg=torch.zeros(n_utt, dtype=i32, device=dev),
                   seg_embed=torch.full((n_utt, NM), -1, dtype=i32, device=dev),
                   seg_row=torch.full((n_utt, NM), -1, dtype=i32, device=dev),
                   seg_label=torch.full((n_utt, NM), -1, dtype=i32, device=dev),
                   seg_score=torch.full((n_utt, NM), -np.inf, dtype=torch.float64, device=dev), row=t[0], score=t[2])
        # (the model's own context: the kernel uses none of a context's state)
        check(self._L.segk_kmd_decode(self._ctx, C.byref(cq.c), C.byref(self.m), C.byref(cand), int(n_slices_min), int(n_slices_max),
                                      float(wip), ptr(out["boundaries"]), ptr(out["seg_embed"]), ptr(out["seg_row"]),
                                      ptr(out["seg_label"]), ptr(out["seg_score"]), ptr(out["n_seg"]), ptr(out["objective"]),
                                      _abi.stream()))
        out["K"] = self.K.clone()
        return out

    def delta_stats(self):
        """What the delta score pass did in the latest hinted call whose figures have arrived (segk_kmeans_delta_stats, no
        synchronisation): (mode: 1 delta, 0 full, -1 no delta state; changed image columns; packed tiles multiplied;
        positions whose hinted score was taken over from the previous call)."""
        out = (C.c_int32 * 4)()
        check(self._L.segk_kmeans_delta_stats(self._ctx, out))
        return tuple(int(v) for v in out)

    def score_ptr(self, ids_ptr, n):
        check(self._L.segk_kmeans_score(self._ctx, self._cp(), C.byref(self.m), C.c_void_p(ids_ptr), 0, int(n),
                                        C.byref(self.cand), ptr(self.status), _abi.stream()))

    def exact_max(self, ids):
        """np.max / np.argmax of neg_sqrd_norm for rows `ids` (host ints) ->
        (float64[n], int32[n], number of rows that needed the full scan)."""
        torch = _torch()
        ids_t = to_dev(self._local_rows(ids), np.int32)
        n = ids_t.numel()
        out_max = torch.empty(n, dtype=torch.float64, device=ids_t.device)
        out_arg = torch.empty(n, dtype=torch.int32, device=ids_t.device)
        self.score_rows(ids_t)
        check(self._L.segk_kmeans_exact_max(self._ctx, self._cp(), C.byref(self.m), ptr(ids_t), n,
                                            C.byref(self.cand), ptr(out_max), ptr(out_arg), _abi.stream()))
        return out_max.cpu().numpy(), out_arg.cpu().numpy(), int(self.cand_count.item())

    def _local_rows(self, ids):
        """Global row ids -> the device's numbering (identity unless the corpus is sharded: then they must lie in the shard)."""
        if self.shard is None:
            return ids
        a = np.asarray(ids, dtype=np.int64)
        if a.size and (a.min() < self.shard[0] or a.max() >= self.shard[1]):
            self.require_whole_corpus("scoring rows outside this rank's shard")
        return a - self.shard[0]

    def neg_sqrd_norm(self, row):
        torch = _torch()
        row = int(self._local_rows([row])[0])
        out = torch.empty(self.K_max, dtype=self.corpus.torch_xdtype, device=self.means.device)
        check(self._L.segk_kmeans_neg_sqrd_norm(self._ctx, self._cp(), C.byref(self.m), int(row), ptr(out),
                                                _abi.stream()))
        return out.cpu().numpy()

    def add_item(self, i, k):
        self.require_whole_corpus("add_item")
        self.ensure_assignments()
        check(self._L.segk_kmeans_add_item(self._ctx, self._cp(), C.byref(self.m), int(i), int(k),
                                           ptr(self.status), _abi.stream()))

    def del_item(self, i):
        self.require_whole_corpus("del_item")
        self.ensure_assignments()
        check(self._L.segk_kmeans_del_item(self._ctx, self._cp(), C.byref(self.m), int(i), ptr(self.status),
                                           _abi.stream()))

    def del_component(self, k):
        self.require_whole_corpus("del_component")
        self.ensure_assignments()
        check(self._L.segk_kmeans_del_component(self._ctx, self._cp(), C.byref(self.m), int(k),
                                                ptr(self.status), _abi.stream()))

    def clean_components(self):
        self.require_whole_corpus("clean_components")
        self.ensure_assignments()
        check(self._L.segk_kmeans_clean_components(self._ctx, self._cp(), C.byref(self.m), ptr(self.status),
                                                   _abi.stream()))

    def sum_neg_sqrd_norm(self):
        self.ensure_assignments()
        torch = _torch()
        out = torch.zeros(1, dtype=torch.float64, device=self.means.device)
        check(self._L.segk_kmeans_sum_neg_sqrd_norm(self._ctx, self._cp(), C.byref(self.m), ptr(out),
                                                    _abi.stream()))
        if self.shard is not None:      # every rank's rows, added in rank order (a record metric: tolerance-level parity)
            return float(sum(self.batch_comm.all_gather_object(float(out.item()))))
        return float(out.item())

    # ------------------------------------------------------------------ segmentation
    def segment(self, boundaries, n_slices_min, n_slices_max, wip, utt=None, utt0=0, n_utts=None):
        """A5+A8+argmax for one utterance (`utt`) or the range utt0..utt0+n_utts."""
        c = self.corpus
        if utt is not None:
            up = C.c_void_p(self.utt_arange.data_ptr() + 4 * int(utt))
            utt0, n = 0, 1
        else:
            up = None
            n = c.n_utt - utt0 if n_utts is None else n_utts
        check(self._L.segk_kmeans_segment(
            self._ctx, self._cp(), C.byref(self.m), up, int(utt0), int(n), int(n_slices_min), int(n_slices_max),
            float(wip), C.byref(self.cand), ptr(boundaries), ptr(self.old_tok),
            ptr(self.new_tok), ptr(self.new_k), ptr(self.n_old), ptr(self.n_new), ptr(self.n_flag),
            ptr(self.out_total), ptr(self.status), _abi.stream()))

    def segment_utt_sequential(self, boundaries, i, n_slices_min, n_slices_max, wip):
        """The whole of segment_i (kmeans_acoustic_wordseg.py:225-332) for utterance i, enqueued
        asynchronously: score its spans, DP, del/add/clean in the reference's order."""
        c = self.corpus
        self.require_whole_corpus("the sequential chain (segment_i)")
        self.ensure_state()
        N = int(c.lengths_np[i])
        tri_i = N * (N + 1) // 2
        self.score_ptr(c.vec_ids.data_ptr() + 4 * i * c.tri, tri_i)
        self.segment(boundaries, n_slices_min, n_slices_max, wip, utt=i)
        check(self._L.segk_kmeans_update_utt(self._ctx, self._cp(), C.byref(self.m), int(i), ptr(self.old_tok),
                                             ptr(self.new_tok), ptr(self.new_k), ptr(self.n_old),
                                             ptr(self.n_new), ptr(self.status), _abi.stream()))

    def sequential_sweep(self, boundaries, order, n_slices_min, n_slices_max, wip):
        """segment_i for every utterance of `order` in turn by ONE library call (segk_kmeans_sequential_sweep): where the
        configuration allows, one persistent kernel per stretch of utterances between two emptied components -- the call
        then SYNCHRONISES the stream after every such launch --, otherwise three launches per utterance (direct exact score,
        DP, update), all enqueued.  Returns False when the library does not support the data (float64): the caller then
        walks the utterances itself."""
        if self.corpus.x_dtype != SEGK_F32 or self.corpus.N_max > 63:
            return False
        torch = _torch()
        self.require_whole_corpus("the sequential chain (segment)")
        self.ensure_state()
        if getattr(self, "_seq_keys", None) is None:
            self._seq_keys = torch.zeros(self.corpus.tri + 2, dtype=torch.int64, device=self.means.device)
        arr = np.ascontiguousarray(order, dtype=np.int32)       # (a ctypes array built element by element: 2 ms of a 135 ms sweep)
        check(self._L.segk_kmeans_sequential_sweep(
            self._ctx, self._cp(), C.byref(self.m), arr.ctypes.data, len(order), int(n_slices_min), int(n_slices_max), float(wip),
            C.byref(self.cand), ptr(self._seq_keys), ptr(boundaries), ptr(self.old_tok), ptr(self.new_tok), ptr(self.new_k),
            ptr(self.n_old), ptr(self.n_new), ptr(self.n_flag), ptr(self.out_total), ptr(self.status), _abi.stream()))
        return True

    def batch_record(self, lo, hi):
        """The record values of the batch sweep just enqueued, in ONE device-to-host copy (segk_kmeans_batch_record):
        (sum_neg_len_sqrd_norm, K, n_tokens, sum_neg_sqrd_norm); raises like check_status."""
        check(self._L.segk_kmeans_batch_record(self._ctx, self._cp(), C.byref(self.m), int(lo), int(hi), ptr(self.new_tok),
                                               ptr(self.new_k), ptr(self.status), ptr(self.out_scalars), _abi.stream()))
        o = self.out_scalars.cpu().numpy()
        self._raise_status(int(o[5]))
        return float(o[0]), int(o[1]), int(o[2]), float(o[4])

    def refit_record(self, lo, hi, moved):
        """The record values of the batch refit just enqueued, in ONE device-to-host copy (segk_kmeans_refit_record):
        (n_mean_updates of this rank's tokens, K, n_tokens, sum_neg_sqrd_norm of this rank's tokens); raises like
        check_status."""
        check(self._L.segk_kmeans_refit_record(self._ctx, self._cp(), C.byref(self.m), int(lo), int(hi), ptr(self.new_tok),
                                               ptr(self.new_k), ptr(self.status), ptr(moved), ptr(self.out_scalars),
                                               _abi.stream()))
        o = self.out_scalars.cpu().numpy()
        self._raise_status(int(o[5]))
        return int(o[7]), int(o[1]), int(o[2]), float(o[4])

    def fit_step(self, consider_unassigned, n_items_max=None):
        """One Lloyd iteration of KMeans.fit enqueued by ONE library call (segk_kmeans_fit_step) and its record
        in ONE device-to-host copy -> (n_mean_updates, K, items, sum_neg_sqrd_norm); raises like check_status.  The state
        afterwards is that of the item-by-item route (exact_max, del_item + add_item per moved item, clean_components), bit
        for bit.  n_items_max (consider_unassigned=False): a bound of the number of rows with a label, n_emb when None."""
        torch = _torch()
        self.require_whole_corpus("KMeans.fit")
        self.ensure_assignments()
        c = self.corpus
        n_max = c.n_emb if consider_unassigned or n_items_max is None else max(1, min(int(n_items_max), c.n_emb))
        words = int(self._L.segk_kmeans_fit_scratch_words(c.n_emb, n_max, self.K_max))
        if getattr(self, "_fit_scratch", None) is None or self._fit_scratch.numel() < words:
            self._fit_scratch = torch.zeros(words, dtype=torch.int32, device=self.means.device)
            self._fit_record = torch.zeros(8, dtype=torch.float64, device=self.means.device)
        check(self._L.segk_kmeans_fit_step(self._ctx, self._cp(), C.byref(self.m), C.byref(self.cand), 1 if consider_unassigned else 0,
                                           n_max, ptr(self._fit_scratch), ptr(self._fit_record), ptr(self.status), _abi.stream()))
        o = self._fit_record.cpu().numpy()
        if int(o[5]) & 8:
            raise SegkError("KMeans.fit on the device: more rows carry a label than the item list was sized for, or a row holds a "
                            "label outside [-1, K_max): the statistics of this iteration are not usable")
        self._raise_status(int(o[5]))
        return int(o[0]), int(o[1]), int(o[2]), float(o[4])

    def _raise_status(self, bits):
        if bits & 8:
            raise SegkError("batch refit: a token's row was not scored (more tokens than the id list was sized for, or a row "
                            "without a result): the labels of this refit are not usable")
        if bits & 1:
            raise AssertionError("a new segment has no embedding (vec_id == -1): the reference asserts in "
                                 "KMeansComponents.add_item (kmeans_components.py:100)")
        if bits & 2:
            raise AssertionError("add_item on an item that is already assigned (kmeans_components.py:101)")
        if bits & 4:
            raise SegkError("batch sweep: in one statistics block more new tokens chose an inactive component than "
                            "`flag_cap`; the tokens beyond were dropped, so the statistics of this sweep are not usable: "
                            "rebuild the segmenter (or load a checkpoint) with a larger flag_cap")

    def check_status(self):
        st = self.status.cpu().numpy()
        self._raise_status(int(st[0]))
        return int(st[1])


class Partition(object):
    """Static split of the utterances into `n_blocks` statistics blocks (the fixed summation
    tree of the batch mode) and of the blocks over `world` ranks (rank r owns a contiguous
    run of blocks, hence of utterances and of embedding rows)."""

    def __init__(self, n_utt, utt_row_start, n_blocks=8, rank=0, world=1):
        if n_blocks % world != 0:
            raise SegkError("the number of statistics blocks (%d) must be a multiple of the number of "
                            "ranks (%d)" % (n_blocks, world))
        self.n_blocks, self.rank, self.world = n_blocks, rank, world
        self.nbl = n_blocks // world
        self.bounds = np.array([(b * n_utt) // n_blocks for b in range(n_blocks + 1)], dtype=np.int32)
        self.utt_lo = int(self.bounds[rank * self.nbl])
        self.utt_hi = int(self.bounds[(rank + 1) * self.nbl])
        self.row_lo = int(utt_row_start[self.utt_lo])
        self.row_hi = int(utt_row_start[self.utt_hi])
        self.local_bounds = self.bounds[rank * self.nbl:(rank + 1) * self.nbl + 1].copy()
        self._row_start = utt_row_start

    def minibatch(self, n_batches):
        """Step j of a mini-batch sweep resegments run j of EVERY statistics block (oracle/np_oracle.py minibatch_ranges):
        for this rank's blocks -> per step (utterance ids int32, embedding rows int32, contiguous?) as numpy arrays."""
        steps = []
        for j in range(n_batches):
            utts, rows = [], []
            for b in range(self.rank * self.nbl, (self.rank + 1) * self.nbl):
                lo_b, hi_b = int(self.bounds[b]), int(self.bounds[b + 1])
                lo = lo_b + (j * (hi_b - lo_b)) // n_batches
                hi = lo_b + ((j + 1) * (hi_b - lo_b)) // n_batches
                utts.append(np.arange(lo, hi, dtype=np.int32))
                rows.append(np.arange(int(self._row_start[lo]), int(self._row_start[hi]), dtype=np.int32))
            u, r = np.concatenate(utts), np.concatenate(rows)
            contiguous = self.nbl == 1 or (len(u) and u[-1] - u[0] + 1 == len(u))
            steps.append((u, r, bool(contiguous)))
        return steps


class KMeansBatchSweeper(object):
    """One batch-synchronous sweep = score -> segment -> partials -> [ONE all-gather] -> finalize, all enqueued
    on the current stream.  With world == 1 there is no collective; with world > 1 every rank contributes one
    packed record -- the partial sums, totals and counts of its statistics blocks and, per block, the (normally
    empty) list of tokens that found new components -- of segk_kmeans_batch_record_words() 8-byte words
    (nbl * (K_max * (D + 1) + 1 + flag words): 0.8 MB per rank at 8 GPUs on the headline corpus) over RCCL."""

    def __init__(self, dk, part, flag_cap=4096, group=None):
        torch = _torch()
        dev = _dev()
        self.dk, self.part, self.cap, self.comm = dk, part, int(flag_cap), get_comm(group)
        assert self.comm.world == part.world and self.comm.rank == part.rank
        c = dk.corpus
        W = part.world
        # a sharded corpus: the embedding rows of the tokens that found new components travel in the record (the other ranks
        # cannot read them from their own X)
        self.flag_rows = 1 if dk.shard is not None else 0
        self.rank_stride = int(dk._L.segk_kmeans_batch_record_words(
            dk.K_max, c.D, part.nbl, self.cap, c.D * (4 if c.x_dtype == SEGK_F32 else 8) if self.flag_rows else 0))
        self.pack_all = torch.zeros((W, self.rank_stride), dtype=torch.float64, device=dev)
        self.pack = self.pack_all[part.rank]
        self.blk_lo = to_dev(part.local_bounds, np.int32)
        # sort scratch: one region per (local block, component range), addressed by the kernels as sorted + p0 * NR with p0 the
        # block's first GLOBAL token slot (utterance * N_max): only this rank's slots are backed by memory -- the pointer
        # handed to the library is the address slot 0 would have (the kernels touch the regions of the local blocks only)
        ws, wk = C.c_int64(), C.c_int64()
        n_loc = (part.utt_hi - part.utt_lo) * c.N_max
        check(dk._L.segk_kmeans_batch_scratch_words(dk.K_max, n_loc, part.nbl, C.byref(ws), C.byref(wk)))
        self.sorted = torch.zeros(ws.value, dtype=torch.int32, device=dev)
        nr = ws.value // max(n_loc, 1)
        self._sorted_ptr = C.c_void_p(self.sorted.data_ptr() - 4 * part.utt_lo * c.N_max * nr)
        self.koff = torch.zeros(wk.value, dtype=torch.int32, device=dev)
        # the sums of token lists that stand from call to call stay in `pack` (segk_kmeans_batch_partials_keep): the kernel's
        # own record of what `sorted`, `koff` and `pack` hold, zeroed with them; no state on the host
        self.keep = torch.zeros(int(dk._L.segk_kmeans_batch_keep_words(dk.K_max, part.nbl)), dtype=torch.int32, device=dev)
        # SEGK_SWEEP_GRAPH=1: the sweep replayed as a hipGraph from its second run on.  Default 0: measured on MI355X
        # the replay is SLOWER than the plain launches it replaces (full corpus 0.661 vs 0.634 ms per sweep, a
        # 1 250-utterance shard 0.258 vs 0.216 ms: the launches of sweep i + 1 are enqueued while sweep i runs, so
        # their host cost is already hidden, and a replay adds ~10 us of its own -- profiles/README.md r02_b)
        import os
        self.use_graph = os.environ.get("SEGK_SWEEP_GRAPH", "0") == "1"
        self._graph, self._graph_args, self._side, self._warm = None, None, None, 0
        # Hints for the score stage (segk_kmeans_score_hinted): every row's argmax of the previous sweep + the relabelling of that
        # sweep's finalize.  They are passed from the THIRD sweep of a chain on (the first sweep has none; the second would hint
        # with labels found against the initial means -- on a fresh chain more than half of them are wrong, and verifying a wrong
        # hint costs more than not hinting), and left out for one sweep whenever the library reports that the certificate of a
        # recent hinted sweep failed on more than HINT_MISS_PERMILLE of the rows (segk_kmeans_hint_feedback: no synchronisation).
        # Results are identical either way.
        self._sweeps_done = 0
        _l, _s, _p = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        check(dk._L.segk_kmeans_hint_feedback(dk._ctx, C.byref(_l), C.byref(_s), C.byref(_p)))
        self._fb_seen = _l.value     # figures of hinted calls enqueued before this sweeper existed are not its business
        self._mb = None              # (n_batches, per-step launch tables) of sweep_minibatch
        # batch refits (refit): after one, cand_k of every row has been translated through each finalize's relabel table as it
        # happened, so the next hinted call takes the identity; a sweep's finalize leaves its table to the next call again
        self._hints_current = False
        self._refits_done = 0
        self._refit = None           # refit's buffers: (id list, chunk scratch, token count [dev], host bound of the token count)
        self._n_tok = None           # this rank's token count where the host knows it (note_token_count), else None
        dk.batch_comm = self.comm

    HINT_MISS_PERMILLE = 450

    def _use_hints(self):
        if self._sweeps_done < 2:
            return False
        launched, seen, permille = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        check(self.dk._L.segk_kmeans_hint_feedback(self.dk._ctx, C.byref(launched), C.byref(seen), C.byref(permille)))
        if seen.value > self._fb_seen:
            self._fb_seen = seen.value
            if permille.value > self.HINT_MISS_PERMILLE:
                return False
        return True

    # ------------------------------------------------------------------ mini-batch sweeps
    def _minibatch_tables(self, n_batches):
        if self._mb is None or self._mb[0] != n_batches:
            steps = []
            for u, r, contiguous in self.part.minibatch(n_batches):
                r = r - self.dk.row_base                 # rows in the device's numbering (a shard starts at 0)
                if contiguous:
                    steps.append((int(u[0]) if len(u) else 0, len(u), int(r[0]) if len(r) else 0, len(r), None, None))
                else:
                    steps.append((0, len(u), 0, len(r), to_dev(u, np.int32), to_dev(r, np.int32)))
            self._mb = (n_batches, steps)
        return self._mb[1]

    def _tokens_from_state(self, boundaries):
        """Token lists of ALL utterances from the boundaries and `assignments` (the state a fresh segmenter or the
        sequential mode leaves): what a mini-batch step needs for the utterances it does not resegment."""
        torch = _torch()
        dk, c = self.dk, self.dk.corpus
        check(dk._L.segk_fbb_collect(dk._ctx, dk._cp(), ptr(boundaries), ptr(dk.new_tok), ptr(dk.n_new), _abi.stream()))
        live = torch.arange(c.N_max, device=dk.n_new.device, dtype=torch.int32)[None, :] < dk.n_new[:, None]
        lab = dk.assignments[dk.new_tok.clamp(min=0).long()]
        dk.new_k.copy_(torch.where(live, lab, torch.full_like(lab, -1)))
        dk.n_flag.zero_()

    def sweep_minibatch(self, boundaries, n_slices_min, n_slices_max, wip, n_batches):
        """One sweep as n_batches steps (specification: oracle/np_oracle.py kmeans_minibatch_sweep): step j scores and
        resegments run j of every local statistics block against the current means, then the statistics are rebuilt from the
        current tokens of ALL utterances exactly as in a whole-sweep batch step (sort, partial sums, ONE all-gather,
        finalize) -- n_batches all-gathers per sweep, n_batches times fresher statistics."""
        dk, pt = self.dk, self.part
        L, ctx, cp, mp, st = dk._L, dk._ctx, dk._cp(), C.byref(dk.m), _abi.stream()
        if dk.assign_stale is None:
            dk.ensure_boundaries()
            self._tokens_from_state(boundaries)
        # (the rows of step j carry the labels of step j of the PREVIOUS sweep, n_batches finalizes old, of which only the last
        # one's relabelling is in dk.remap: while components are still being removed some hints are stale -- they are verified
        # like any other and cost one pass of the band stage, never a wrong result)
        hints = self._use_hints()
        self._n_tok = None
        for (utt0, n_utts, row0, n_rows, utts, rows) in self._minibatch_tables(n_batches):
            # (after a refit the first step's hints are in the current labelling; every step's finalize relabels again)
            hint = {} if not hints else {"hint_identity": True} if self._hints_current else {"hint_remap": dk.remap}
            self._hints_current = False
            if rows is None:
                dk.score_rows(row0=row0, n=n_rows, **hint)
                dk.segment(boundaries, n_slices_min, n_slices_max, wip, utt0=utt0, n_utts=n_utts)
            else:
                dk.score_rows(ids=rows, **hint)
                check(L.segk_kmeans_segment(ctx, cp, mp, ptr(utts), 0, n_utts, int(n_slices_min), int(n_slices_max), float(wip),
                                            C.byref(dk.cand), ptr(boundaries), ptr(dk.old_tok), ptr(dk.new_tok), ptr(dk.new_k),
                                            ptr(dk.n_old), ptr(dk.n_new), ptr(dk.n_flag), ptr(dk.out_total), ptr(dk.status), st))
            check(L.segk_kmeans_batch_partials_keep(ctx, cp, mp, ptr(self.blk_lo), pt.nbl, ptr(dk.new_tok), ptr(dk.new_k),
                                                    ptr(dk.n_flag), ptr(dk.out_total), self._sorted_ptr, ptr(self.koff),
                                                    ptr(self.pack), self.cap, self.flag_rows, ptr(dk.out_scalars), st,
                                                    ptr(self.keep), self.keep.numel()))
            if pt.world > 1:
                self.comm.all_gather_rows(self.pack_all, self.pack)
            self._enqueue_back()
        self._sweeps_done += 1
        dk.assign_stale = (pt.utt_lo, pt.utt_hi, pt.world)
        dk.bounds_stale = (boundaries, pt) if pt.world > 1 else None

    def _enqueue_front(self, boundaries, n_slices_min, n_slices_max, wip):
        dk, pt = self.dk, self.part
        L, ctx, cp, mp, st = dk._L, dk._ctx, dk._cp(), C.byref(dk.m), _abi.stream()
        # from the second sweep on cand_k holds every row's argmax of the previous sweep and dk.remap the relabelling of
        # that sweep's finalize: hints for the score stage (same results)
        # (after a refit the hints are in the current labelling already: refit)
        hint = {} if not self._use_hints() else {"hint_identity": True} if self._hints_current else {"hint_remap": dk.remap}
        dk.score_rows(row0=pt.row_lo - dk.row_base, n=pt.row_hi - pt.row_lo, **hint)
        dk.segment(boundaries, n_slices_min, n_slices_max, wip, utt0=pt.utt_lo, n_utts=pt.utt_hi - pt.utt_lo)
        check(L.segk_kmeans_batch_partials_keep(ctx, cp, mp, ptr(self.blk_lo), pt.nbl, ptr(dk.new_tok), ptr(dk.new_k),
                                                ptr(dk.n_flag), ptr(dk.out_total), self._sorted_ptr, ptr(self.koff),
                                                ptr(self.pack), self.cap, self.flag_rows, ptr(dk.out_scalars), st,
                                                ptr(self.keep), self.keep.numel()))

    def _enqueue_back(self):
        dk, pt = self.dk, self.part
        L, ctx, cp, mp, st = dk._L, dk._ctx, dk._cp(), C.byref(dk.m), _abi.stream()
        check(L.segk_kmeans_batch_finalize(ctx, cp, mp, pt.utt_lo, pt.utt_hi, ptr(self.pack_all), pt.n_blocks, pt.nbl,
                                           self.rank_stride, self.cap, self.flag_rows, pt.rank, ptr(dk.new_k), ptr(dk.remap),
                                           ptr(dk.out_scalars), ptr(dk.status), st))

    def sweep(self, boundaries, n_slices_min, n_slices_max, wip):
        dk, pt = self.dk, self.part
        if self.use_graph:
            self._sweep_graph(boundaries, n_slices_min, n_slices_max, wip)
        else:
            self._enqueue_front(boundaries, n_slices_min, n_slices_max, wip)
            if pt.world > 1:
                self.comm.all_gather_rows(self.pack_all, self.pack)
            self._enqueue_back()
        dk.assign_stale = (pt.utt_lo, pt.utt_hi, pt.world)
        dk.bounds_stale = (boundaries, pt) if pt.world > 1 else None
        self._sweeps_done += 1
        self._hints_current = False
        self._n_tok = None

    # ------------------------------------------------------------------ batch refit between sweeps
    def note_token_count(self, n):
        """This rank's number of tokens, where the caller has it on the host (one rank: the record of the sweep or refit just
        run): the refit then scores exactly that many rows instead of the bound the host can know without it."""
        self._n_tok = int(n)

    def _relabel_hints(self):
        dk = self.dk
        check(dk._L.segk_kmeans_hint_relabel(dk._ctx, dk._cp(), C.byref(dk.m), C.byref(dk.cand), ptr(dk.remap), _abi.stream()))

    def refit(self, boundaries):
        """Enqueue one batch refit (specification: tests/kmeans_refit.py kmeans_batch_refit): every current token of this rank's
        utterances gets the argmax against the means as they stand, then the statistics are rebuilt from the relabelled token
        lists exactly as after a sweep -- partial sums, ONE all-gather, finalize.  The segmentation, `out_total` and the
        communication pattern of a sweep stay; `dk.refit_moved` holds the number of this rank's tokens whose label changed."""
        torch = _torch()
        dk, pt, c = self.dk, self.part, self.dk.corpus
        L, ctx, cp, mp, st = dk._L, dk._ctx, dk._cp(), C.byref(dk.m), _abi.stream()
        if dk.assign_stale is None:
            dk.ensure_boundaries()
            self._tokens_from_state(boundaries)
            self._n_tok = None
        if self.use_graph:
            # a captured sweep holds the addresses of the score path's workspaces, which scoring an id list of another length
            # may reallocate: the next sweep runs eagerly and is captured again
            self._drop_graph()
            self._warm = 0
        n_slots = (pt.utt_hi - pt.utt_lo) * c.N_max
        if self._refit is None:
            # a token spans at least one landmark: the landmarks of the local utterances bound the tokens
            bound = min(int(c.lengths_np[pt.utt_lo:pt.utt_hi].sum()), n_slots, c.n_emb)
            dev = dk.new_k.device
            self._refit = (torch.zeros(max(bound, 1), dtype=torch.int32, device=dev),
                           torch.zeros(int(L.segk_kmeans_refit_scratch_words(n_slots)), dtype=torch.int32, device=dev),
                           torch.zeros(1, dtype=torch.int32, device=dev), bound)
        ids, chunks, count, bound = self._refit
        n_list = bound if self._n_tok is None else min(self._n_tok, bound)
        hints = self._use_hints()
        # the hints of ALL rows into the current labelling, here and after the finalize below (two relabellings lie between
        # a span row's hint and the next sweep, and dk.remap holds only the latest): the hinted calls then take the identity
        if not self._hints_current and self._sweeps_done + self._refits_done > 0:
            self._relabel_hints()
        check(L.segk_kmeans_refit_collect(ctx, cp, pt.utt_lo, pt.utt_hi, ptr(dk.new_tok), ptr(dk.new_k), ptr(chunks), ptr(ids),
                                          None, n_list, ptr(count), ptr(dk.status), st))
        dk.score_rows(ids=ids[:n_list], hint_identity=hints)
        check(L.segk_kmeans_refit_apply(ctx, cp, mp, C.byref(dk.cand), pt.utt_lo, pt.utt_hi, ptr(dk.new_tok), ptr(dk.new_k),
                                        ptr(dk.n_flag), ptr(dk.refit_moved), ptr(dk.status), st))
        check(L.segk_kmeans_batch_partials_keep(ctx, cp, mp, ptr(self.blk_lo), pt.nbl, ptr(dk.new_tok), ptr(dk.new_k),
                                                ptr(dk.n_flag), ptr(dk.out_total), self._sorted_ptr, ptr(self.koff),
                                                ptr(self.pack), self.cap, self.flag_rows, ptr(dk.out_scalars), st,
                                                ptr(self.keep), self.keep.numel()))
        if pt.world > 1:
            self.comm.all_gather_rows(self.pack_all, self.pack)
        self._enqueue_back()
        self._relabel_hints()
        self._hints_current = True
        self._refits_done += 1
        dk.assign_stale = (pt.utt_lo, pt.utt_hi, pt.world)

    # ------------------------------------------------------------------ hipGraph replay
    def _capture(self, fn):
        """Run `fn` (library launches only) under stream capture on the sweeper's side stream -> executable graph."""
        dk = self.dk
        st = _abi.stream()
        check(dk._L.segk_graph_begin(dk._ctx, st))
        try:
            fn()
        finally:
            ex = C.c_void_p()
            rc = dk._L.segk_graph_end(dk._ctx, st, C.byref(ex))
        check(rc)
        return ex

    def _sweep_graph(self, boundaries, n_slices_min, n_slices_max, wip):
        """The sweep as one hipGraph (two around the all-gather with more than one rank), replayed on a stream of
        the sweeper's own (a capture cannot run on the legacy default stream); the caller's current stream is
        ordered before and after it.  The first sweep runs eagerly: it creates what a capture cannot contain
        (workspaces, kernel attributes)."""
        torch = _torch()
        dk, pt = self.dk, self.part
        args = (boundaries.data_ptr(), int(n_slices_min), int(n_slices_max), float(wip))
        cur = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream()
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            if self._warm < 1 or (self._graph is not None and self._graph_args != args):
                self._drop_graph()
            if self._warm < 1:
                self._enqueue_front(boundaries, n_slices_min, n_slices_max, wip)
                if pt.world > 1:
                    self.comm.all_gather_rows(self.pack_all, self.pack)
                self._enqueue_back()
                self._warm += 1
            else:
                if self._graph is None:
                    if pt.world > 1:
                        front = self._capture(lambda: self._enqueue_front(boundaries, n_slices_min, n_slices_max, wip))
                        back = self._capture(self._enqueue_back)
                        self._graph = (front, back)
                    else:
                        def whole():
                            self._enqueue_front(boundaries, n_slices_min, n_slices_max, wip)
                            self._enqueue_back()
                        self._graph = (self._capture(whole),)
                    self._graph_args = args
                st = _abi.stream()
                check(dk._L.segk_graph_launch(dk._ctx, self._graph[0], st))
                if pt.world > 1:
                    self.comm.all_gather_rows(self.pack_all, self.pack)
                    check(dk._L.segk_graph_launch(dk._ctx, self._graph[1], st))
        cur.wait_stream(self._side)

    def _drop_graph(self):
        if self._graph is not None:
            for ex in self._graph:
                self.dk._L.segk_graph_destroy(self.dk._ctx, ex)
        self._graph = None

    def __del__(self):
        try:
            self._drop_graph()
        except Exception:
            pass


class DeviceFbgmm(object):
    """Device image of FBGMM + its Gaussian components (fixed-variance, diagonal or full covariance), see
    include/segk.h `segk_fbgmm`."""

    def __init__(self, corpus, cov_type, K_max, alpha, lms, prior_a, prior_b, prior_c, k_0, v_0, assignments,
                 lm=None):
        torch = _torch()
        dev = _dev()
        self.corpus = corpus
        c = corpus
        self.K_max = int(K_max)
        self.cov_type = int(cov_type)
        f64 = torch.float64
        self.prior_a = to_dev(prior_a, np.float64)
        self.prior_b = to_dev(prior_b, np.float64)
        if self.cov_type == 2:
            # full covariance: D x D statistics and factors per component; prior_c is derived by the library (the prior's
            # factor, the prior predictive of every row, one status word)
            assert lm is None and tuple(self.prior_a.shape) == (c.D, c.D)
            self.prior_c = torch.zeros(c.D * c.D + c.n_emb + 1, dtype=f64, device=dev)
            mat = (self.K_max, c.D, c.D)
        else:
            self.prior_c = to_dev(prior_c if prior_c is not None else np.zeros(c.D), np.float64)
            mat = (self.K_max, c.D)
        self.stat_a = torch.zeros((self.K_max, c.D), dtype=f64, device=dev)
        self.stat_b = torch.zeros(mat, dtype=f64, device=dev)
        self.log_prod = torch.zeros(self.K_max, dtype=f64, device=dev)
        self.pred = torch.zeros(mat, dtype=f64, device=dev)
        self.kconst = torch.zeros(self.K_max + 1, dtype=f64, device=dev)
        self.counts = torch.zeros(self.K_max, dtype=torch.int64, device=dev)
        self.assignments = to_dev(assignments, np.int32)
        self.K = torch.zeros(1, dtype=torch.int32, device=dev)
        self.f = _abi.FbgmmDev(
            cov_type=self.cov_type, K_max=self.K_max, alpha=float(alpha), lms=float(lms), k_0=float(k_0),
            v_0=float(v_0), prior_a=self.prior_a.data_ptr(), prior_b=self.prior_b.data_ptr(),
            prior_c=self.prior_c.data_ptr(), stat_a=self.stat_a.data_ptr(), stat_b=self.stat_b.data_ptr(),
            log_prod=self.log_prod.data_ptr(), pred=self.pred.data_ptr(), counts=self.counts.data_ptr(),
            assignments=self.assignments.data_ptr(), K=self.K.data_ptr(), kconst=self.kconst.data_ptr())
        self.lm = lm
        if lm is not None:        # bigram_lms.BigramSmoothLM: its count tensors are tied to the components
            assert lm.K == self.K_max and self.cov_type == 0
            self.f.lm_unigram = lm._unigram.data_ptr()
            self.f.lm_bigram = lm._bigram.data_ptr()
            self.f.lm_lambda, self.f.lm_a, self.f.lm_b = float(lm.intrp_lambda), float(lm.a), float(lm.b)
        self.score = torch.zeros(c.n_emb, dtype=f64, device=dev)
        self.status = torch.zeros(8, dtype=torch.int32, device=dev)
        self._L = _abi.lib()
        self._ctx = _abi.ctx()
        # scratch for single-item calls
        self._tok1 = torch.zeros(max(c.N_max, 1), dtype=torch.int32, device=dev)
        self._n1 = torch.ones(1, dtype=torch.int32, device=dev)
        self._u1 = torch.zeros(1, dtype=f64, device=dev)
        self._cur1 = torch.zeros(1, dtype=torch.int64, device=dev)
        check(self._L.segk_fbgmm_init_stats(self._ctx, self._cp(), C.byref(self.f), _abi.stream()))
        if c.n_utt:
            nu, nm = c.n_utt, c.N_max
            self.new_tok = torch.zeros((nu, nm), dtype=torch.int32, device=dev)
            self.n_new = torch.zeros(nu, dtype=torch.int32, device=dev)
            self.out_logprob = torch.zeros(nu, dtype=f64, device=dev)
            self.ucursor = torch.zeros(1, dtype=torch.int64, device=dev)
            self.ustream = torch.zeros(1, dtype=f64, device=dev)

    def _cp(self):
        return C.byref(self.corpus.c)

    def set_lms_alpha(self, alpha, lms):
        self.f.alpha, self.f.lms = float(alpha), float(lms)

    def update(self, op, utt=0, item=0, k=0, boundaries=None):
        check(self._L.segk_fbgmm_update(self._ctx, self._cp(), C.byref(self.f), int(op), int(utt), int(item),
                                        int(k), ptr(boundaries), _abi.stream()))

    def score_rows(self, ids_ptr=None, row0=0, n=None):
        n = self.corpus.n_emb - row0 if n is None else n
        p = C.c_void_p(ids_ptr) if ids_ptr is not None else None
        check(self._L.segk_fbgmm_score(self._ctx, self._cp(), C.byref(self.f), p, int(row0), int(n),
                                       ptr(self.score), _abi.stream()))

    def log_marg_rows(self, ids):
        """log_marg_i for a list of rows -> numpy float64."""
        ids_t = to_dev(ids, np.int32)
        check(self._L.segk_fbgmm_score(self._ctx, self._cp(), C.byref(self.f), ptr(ids_t), 0, ids_t.numel(),
                                       ptr(self.score), _abi.stream()))
        return self.score[ids_t.long()].cpu().numpy()

    def pred_vector(self, row):
        """(log_post_pred(row)[:K], log_prior(row)) evaluated on the device."""
        torch = _torch()
        out = torch.zeros(self.K_max + 1, dtype=torch.float64, device=self.stat_a.device)
        check(self._L.segk_fbgmm_pred_vector(self._ctx, self._cp(), C.byref(self.f), int(row), ptr(out),
                                             _abi.stream()))
        o = out.cpu().numpy()
        return o[:int(self.K.item())].copy(), float(o[self.K_max])

    def assign_item(self, i, u, anneal_temp=1.0, map_assign=False, j_prev=None):
        """gibbs_sample_inside_loop_i / map_assign_i for one row with the uniform `u`; with an LM
        attached gibbs_sample_inside_loop_i_embed given the previous component `j_prev`.
        Returns the component the row went to."""
        self._tok1[0] = int(i)
        self._u1[0] = float(u)
        self._cur1.zero_()
        check(self._L.segk_fbgmm_assign(self._ctx, self._cp(), C.byref(self.f), 0, 1 if map_assign else 0,
                                        -1 if j_prev is None else int(j_prev), float(anneal_temp),
                                        ptr(self._tok1), ptr(self._n1), ptr(self._u1), ptr(self._cur1), 1,
                                        ptr(self.status), _abi.stream()))
        return int(self.assignments[int(i)].item())

    def gibbs_items(self, uniforms, consider_unassigned=True, anneal_temp=1.0, ids=None):
        """One pass of FBGMM.gibbs_sample's inner loop (fbgmm.py:352-405) over `ids` (default: all
        rows, in index order) consuming `uniforms` in order."""
        torch = _torch()
        u = to_dev(np.asarray(uniforms, dtype=np.float64)) if len(uniforms) else torch.zeros(1, dtype=torch.float64,
                                                                                             device=self.K.device)
        cur = torch.zeros(1, dtype=torch.int64, device=self.K.device)
        ids_t = None if ids is None else to_dev(ids, np.int32)
        n = self.corpus.n_emb if ids is None else ids_t.numel()
        check(self._L.segk_fbgmm_gibbs_items(self._ctx, self._cp(), C.byref(self.f), ptr(ids_t), int(n),
                                             1 if consider_unassigned else 0, float(anneal_temp), ptr(u), ptr(cur),
                                             len(uniforms), ptr(self.status), _abi.stream()))
        return int(cur.item())

    def map_items(self, consider_unassigned=True):
        """One MAP sweep of the serial chain over all rows in index order (fbgmm.py:352-405 with map_assign_i's choice in
        place of the draw; segk_fbgmm_map_items).  Returns the number of items that moved."""
        torch = _torch()
        moved = torch.zeros(1, dtype=torch.int32, device=self.K.device)
        check(self._L.segk_fbgmm_map_items(self._ctx, self._cp(), C.byref(self.f), None, int(self.corpus.n_emb),
                                           1 if consider_unassigned else 0, ptr(self.status), ptr(moved), _abi.stream()))
        return int(moved.item())

    def set_uniform_stream(self, u):
        self.ustream = to_dev(u, np.float64)
        self.ucursor.zero_()

    def gibbs_utt(self, boundaries, i, viterbi, n_slices_min, n_slices_max, wip, time_power_term,
                  log_p_continue, anneal_temp_fb, anneal_temp_am, assignments_only=False, map_assign=None):
        """gibbs_sample_i (unigram_acoustic_wordseg.py:252-360; with an LM attached
        bigram_acoustic_wordseg.py:386-551) for utterance i, enqueued asynchronously: [remove its
        LM counts,] remove its segments, score its spans, sample boundaries, assign[, add its LM
        counts]."""
        c = self.corpus
        L, ctx, cp, fp, st = self._L, self._ctx, self._cp(), C.byref(self.f), _abi.stream()
        N = int(c.lengths_np[i])
        tri_i = N * (N + 1) // 2
        if map_assign is None:
            map_assign = viterbi
        if self.lm is not None:
            check(L.segk_fbgmm_update(ctx, cp, fp, 5, int(i), 0, 0, ptr(boundaries), st))
        check(L.segk_fbgmm_update(ctx, cp, fp, 0, int(i), 0, 0, ptr(boundaries), st))
        if not assignments_only:
            check(L.segk_fbgmm_score(ctx, cp, fp, C.c_void_p(c.vec_ids.data_ptr() + 4 * i * c.tri), 0, tri_i,
                                     ptr(self.score), st))
        mode = 2 if assignments_only else (1 if viterbi else 0)
        check(L.segk_unigram_segment(ctx, cp, int(i), mode, int(n_slices_min), int(n_slices_max),
                                     float(wip), float(time_power_term), float(log_p_continue),
                                     float(anneal_temp_fb), ptr(self.score), ptr(self.ustream), ptr(self.ucursor),
                                     self.ustream.numel(), ptr(boundaries), ptr(self.new_tok), ptr(self.n_new),
                                     ptr(self.out_logprob), ptr(self.status), st))
        check(L.segk_fbgmm_assign(ctx, cp, fp, int(i), 1 if map_assign else 0, -1, float(anneal_temp_am),
                                  ptr(self.new_tok), ptr(self.n_new), ptr(self.ustream), ptr(self.ucursor),
                                  self.ustream.numel(), ptr(self.status), st))
        if self.lm is not None:
            check(L.segk_fbgmm_update(ctx, cp, fp, 6, int(i), 0, 0, ptr(boundaries), st))

    def sequential_sweep(self, boundaries, order, row_start, viterbi, n_slices_min, n_slices_max, wip, time_power_term,
                         log_p_continue, anneal_temp_fb, anneal_temp_am, map_assign=None):
        """gibbs_utt for every utterance of `order` in turn by ONE library call (segk_fbgmm_sequential_sweep: a persistent
        kernel per stretch of utterances between two emptied components; the call synchronises the stream; with a language
        model attached the bigram sampler's gibbs_sample_i, bigram_acoustic_wordseg.py:386-551).  Returns False, with nothing
        enqueued, where the kernel does not apply (a model too large for a workgroup's LDS, ...): the caller then walks the
        utterances itself."""
        if self.corpus.N_max > 64:
            return False
        if getattr(self, "_row_start_dev", None) is None:
            self._row_start_dev = to_dev(np.asarray(row_start, dtype=np.int32))
        arr = np.ascontiguousarray(order, dtype=np.int32)
        if map_assign is None:
            map_assign = viterbi
        rc = self._L.segk_fbgmm_sequential_sweep(
            self._ctx, self._cp(), C.byref(self.f), arr.ctypes.data, len(arr), ptr(self._row_start_dev), 1 if viterbi else 0,
            1 if map_assign else 0, int(n_slices_min), int(n_slices_max), float(wip), float(time_power_term),
            float(log_p_continue), float(anneal_temp_fb), float(anneal_temp_am), ptr(self.score), ptr(self.ustream),
            ptr(self.ucursor), self.ustream.numel(), ptr(boundaries), ptr(self.new_tok), ptr(self.n_new),
            ptr(self.out_logprob), ptr(self.status), _abi.stream())
        if rc == _abi.SEGK_ERR_UNSUPPORTED:
            return False
        check(rc)
        return True

    def record_metrics(self, urn=False, urn_a=0.0):
        """(log_prob_z, log_prob_X_given_z, K, n_assigned) of the sequential-mode state, computed on the device (segk_fbgmm_record_metrics): fbgmm.py:208-225 or, with urn=True,
        bigram_acoustic_wordseg.py:287-305; gaussian_components_{fixedvar,diag}.py log_marg."""
        torch = _torch()
        if getattr(self, "_metric_out", None) is None:
            self._metric_out = torch.zeros(4, dtype=torch.float64, device=self.K.device)
        check(self._L.segk_fbgmm_record_metrics(self._ctx, self._cp(), C.byref(self.f), 1 if urn else 0, float(urn_a),
                                                ptr(self._metric_out), _abi.stream()))
        o = self._metric_out.cpu().numpy()
        lpx = float(o[1])
        if self.cov_type == 0 and self.corpus.D == 1:
            # numpy reduces an (n, 1) matrix along axis 0 as a contiguous vector, pairwise, where the kernel adds row after
            # row (8e-7 apart in float32, against 1e-8 for record values): D = 1 is no workload, the host expression answers
            comp = self._components() if getattr(self, "_components", None) is not None else None
            if comp is None:
                raise SegkError("record_metrics at D = 1 evaluates the components' host expression: build the model through "
                                "GaussianComponentsFixedVar")
            lpx = float(comp.log_marg())
        return float(o[0]), lpx, int(o[2]), int(o[3])

    def check_status(self):
        st = int(self.status[0].item())
        if self.cov_type == 2:      # the calls without a status argument (init_stats, update) report in prior_c's last word
            st |= int(self.prior_c[-1:].view(_torch().int32)[0].item())
        if st & 8:
            raise SegkError("uniform stream exhausted")
        if st & 16:
            raise AssertionError("forward_backward: log_prob == -inf (unigram_acoustic_wordseg.py:753)")
        if st & 32:
            raise SegkError("full-covariance component: the covariance matrix of a component is not positive definite "
                            "(a non-positive or non-finite Cholesky pivot); the component kept its previous factor")
        if st & 64:
            raise SegkError("full-covariance component: add_item / del_component named a component beyond K")


class FbgmmBatchSweeper(object):
    """Batch-synchronous ("blocked parallel Gibbs") sweeps of the FBGMM / bigram samplers --
    specification oracle/np_fbgmm_batch.py, C ABI `segk_fbb_*` (include/segk.h).

    The utterances are cut into `n_stat_blocks` slices (rank r owns a contiguous run of them) x
    `n_gibbs_blocks` blocks.  Per Gibbs step b every rank resamples block b of its slices against
    the statistics of all other blocks, recomputes the block's partial sums and all-gathers them
    (one RCCL all-gather of S/P * K_max*(2D+1) doubles per rank and step; with a language model a
    second one of the block's transcripts).  All partial sums are replicated, so every rank derives
    the same statistics in the same fixed order: results do not depend on the number of ranks."""

    def __init__(self, df, row_start, n_gibbs_blocks=8, n_stat_blocks=8, seed=0, group=None, score_precision="f64"):
        torch = _torch()
        dev = _dev()
        self.df, self.comm = df, get_comm(group)
        assert score_precision in ("f64", "f32", "f16")
        self.fullcov = df.cov_type == 2
        if self.fullcov:
            # full-covariance components: fp64 scores, no language model, one process
            if score_precision != "f64":
                raise SegkError("the batch sampler takes full-covariance components with score_precision='f64' only "
                                "(got %r): there is no reduced-precision form of the triangular solves" % (score_precision,))
            if df.lm is not None:
                raise SegkError("the batch sampler takes full-covariance components without a language model only")
            if self.comm.world > 1:
                raise SegkError("the batch sampler takes full-covariance components in one process only (%d ranks): the "
                                "exchange of their partial sums between ranks is not covered by any test" % self.comm.world)
            if df.corpus.D > 64:
                raise SegkError("full-covariance components (cov_type 2) support D <= 64, got %d" % df.corpus.D)
        if score_precision == "f16" and df.cov_type != 0:
            raise SegkError("score_precision='f16' (matrix-core span score) exists for fixed-variance components only")
        if score_precision == "f16" and 2 * df.corpus.D > 208:
            raise SegkError("score_precision='f16' supports D <= 104")
        # fixed variance: the span score as a matrix-core contraction (f32 / f16); diagonal: the Student-t terms in
        # float32 with the hardware logarithm (f32)
        self.score_f32 = score_precision in ("f32", "f16") and df.cov_type == 0
        self.score_f16 = score_precision == "f16"
        self.score_diag32 = score_precision == "f32" and df.cov_type == 1
        self._fused = None             # segk_fbb_step_diag32: None = not tried yet, False = the library refused (unsupported shape)
        c = df.corpus
        self.S, self.B = int(n_stat_blocks), int(n_gibbs_blocks)
        rank, world = self.comm.rank, self.comm.world
        if self.S % world != 0:
            raise SegkError("the number of statistics slices (%d) must be a multiple of the number of ranks (%d)"
                            % (self.S, world))
        self.rank, self.world = rank, world
        self.s_n = self.S // world
        self.s_lo = rank * self.s_n
        n_utt = c.n_utt
        sb = [(s * n_utt) // self.S for s in range(self.S + 1)]
        ur = np.zeros((self.S, self.B, 2), np.int32)
        rr = np.zeros((self.S, self.B, 2), np.int32)
        row_start = np.asarray(row_start, dtype=np.int64)
        for s in range(self.S):
            n_s = sb[s + 1] - sb[s]
            for b in range(self.B):
                lo, hi = sb[s] + (b * n_s) // self.B, sb[s] + ((b + 1) * n_s) // self.B
                ur[s, b] = (lo, hi)
                rr[s, b] = (row_start[lo], row_start[hi])
        self.utt_range_np, self.row_range_np = ur, rr
        self.utt_range, self.row_range = to_dev(ur), to_dev(rr)
        K, D = df.K_max, c.D
        # doubles of a (block, slice) cell's record: counts, sum x, then sum x^2 or the packed triangle of sum outer(x, x)
        self.rec = K * (1 + D + D * (D + 1) // 2) if self.fullcov else K * (2 * D + 1)
        f64 = torch.float64
        self.partials = torch.zeros((self.B, self.S, self.rec), dtype=f64, device=dev)
        self.cnt = torch.zeros(K, dtype=f64, device=dev)
        # (full covariance: the mean of every slot, slot-major, and the Cholesky factor of its covar as DeviceFbgmm.pred
        # stores it -- include/segk.h, segk_fbatch)
        self.mean_t = torch.zeros((K, D) if self.fullcov else (D, K), dtype=f64, device=dev)
        self.q_t = torch.zeros((K, D, D) if self.fullcov else (D, K), dtype=f64, device=dev)
        self.lconst = torch.zeros(K, dtype=f64, device=dev)
        self.zconst = torch.zeros(K, dtype=f64, device=dev)
        self.half = torch.zeros(K, dtype=f64, device=dev)
        self.scal = torch.zeros(2, dtype=f64, device=dev)
        self.slot = torch.zeros(c.n_emb, dtype=torch.int32, device=dev)
        self.remap = torch.zeros(K, dtype=torch.int32, device=dev)
        self.u_max = int((ur[:, :, 1] - ur[:, :, 0]).max())
        if self.u_max * max(c.N_max, 1) >= 2 ** 31:
            raise SegkError("a block of %d utterances x %d landmarks has more token positions than the kernels' int32 "
                            "counters hold: use more blocks or slices" % (self.u_max, c.N_max))
        self.lm_tok = None
        # the batch state keeps its own bigram table (indexed by slots); the sequential-mode tables of
        # the LM object are only written by materialise()
        self.f = _abi.FbgmmDev.from_buffer_copy(df.f)
        if df.lm is not None:
            self.lm_tok = torch.full((self.B, self.S, self.u_max, c.N_max), -1, dtype=torch.int32, device=dev)
            self.lm_big = torch.zeros((K, K), dtype=torch.int64, device=dev)
            self.f.lm_bigram = self.lm_big.data_ptr()
        self.y = self.tiles32 = None
        ldy = (2 * D + 3) // 4 * 4
        if self.score_f32:
            self.y = torch.zeros((c.n_emb, ldy), dtype=torch.float32, device=dev)
            self.tiles32 = torch.zeros(int(_abi.lib().segk_kmeans_tiles_floats(K + 1, 2 * D)), dtype=torch.float32,
                                       device=dev)
        self.y16 = self.tiles16 = self.rows32 = self.consts16 = None
        if self.score_f16:
            L = _abi.lib()
            self.y16 = torch.zeros(int(L.segk_corpus_b3_bytes(c.n_emb, 2 * D)), dtype=torch.uint8, device=dev)
            self.tiles16 = torch.zeros(int(L.segk_kmeans_tiles_b3_floats(K + 1, 2 * D)), dtype=torch.float32, device=dev)
            self.rows32 = torch.zeros((K + 1, 2 * D), dtype=torch.float32, device=dev)
            self.consts16 = torch.zeros(2 * (K + 2) + 32, dtype=f64, device=dev)
        # the prior predictive of every row (an empty slot's likelihood): a constant of corpus and prior, evaluated once
        # instead of in the score and assignment kernels of every Gibbs step (same values)
        self.prior_rows = torch.zeros(c.n_emb, dtype=f64, device=dev)
        check(df._L.segk_fbb_prior_rows(df._ctx, df._cp(), C.byref(self.f), self.prior_rows.data_ptr(), _abi.stream()))
        # the reduced-precision kernels work in coordinates centred on the corpus column mean (segk_fbatch.centre): the
        # rounding of their float32 / fp16x2 operands then follows the data's spread, not its distance from the origin.  One
        # pass over X per sampler, in fp64 and in row order on the host, so every rank (each holds the whole corpus) gets the
        # same bits
        self.centre = self._corpus_centre() if score_precision != "f64" else None
        # diagonal float32 mode: segk_fbb_prepare writes the float32 slot tables the score / step kernels stage
        self.tab32 = torch.zeros(2 * D * K, dtype=torch.float32, device=dev) if self.score_diag32 else None
        self.bt = _abi.FbatchDev(
            centre=self.centre.data_ptr() if self.centre is not None else None,
            tab32=self.tab32.data_ptr() if self.tab32 is not None else None,
            prior_rows=self.prior_rows.data_ptr(),
            y16=self.y16.data_ptr() if self.y16 is not None else None,
            tiles16=self.tiles16.data_ptr() if self.tiles16 is not None else None,
            rows32=self.rows32.data_ptr() if self.rows32 is not None else None,
            consts16=self.consts16.data_ptr() if self.consts16 is not None else None,
            y=self.y.data_ptr() if self.y is not None else None, ldy=ldy,
            tiles32=self.tiles32.data_ptr() if self.tiles32 is not None else None,
            n_slices=self.S, n_blocks=self.B, u_max=self.u_max if df.lm is not None else 0, fast_dp=1 if score_precision != "f64" else 0,
            utt_range=self.utt_range.data_ptr(), row_range=self.row_range.data_ptr(),
            partials=self.partials.data_ptr(), cnt=self.cnt.data_ptr(), mean_t=self.mean_t.data_ptr(),
            q_t=self.q_t.data_ptr(), lconst=self.lconst.data_ptr(), zconst=self.zconst.data_ptr(),
            half=self.half.data_ptr(), scal=self.scal.data_ptr(), slot=self.slot.data_ptr(),
            lm_tok=self.lm_tok.data_ptr() if self.lm_tok is not None else None, seed=int(seed) & (2 ** 64 - 1))
        # host-side per-step launch tables
        I32 = C.c_int32 * self.s_n
        self._n_rows = [I32(*[int(rr[self.s_lo + i, b, 1] - rr[self.s_lo + i, b, 0]) for i in range(self.s_n)])
                        for b in range(self.B)]
        self._n_utts = [I32(*[int(ur[self.s_lo + i, b, 1] - ur[self.s_lo + i, b, 0]) for i in range(self.s_n)])
                        for b in range(self.B)]
        # acoustic-model batch sweeps (am_sweep): the landmarks of every cell's utterances, the host's bound on its tokens
        self._tok_cap = None
        if c.lengths_np is not None:
            lens = c.lengths_np.astype(np.int64)
            self._tok_cap = [I32(*[int(lens[ur[self.s_lo + i, b, 0]:ur[self.s_lo + i, b, 1]].sum()) for i in range(self.s_n)])
                             for b in range(self.B)]
        self.score_precision = score_precision
        self.probe_ll = None             # am_sweep: a [n_utt * N_max, >= K_max] float64 device tensor, the likelihoods (tests)
        self._bt32 = None                # am_sweep(score_precision="f32") on an fp64 sweeper: the copy of `bt` (_bt_am32)
        self.ll_mat = None
        if self.score_f16:
            # token likelihoods of the assignment step from the matrix cores: per block, the positions of its
            # utterances' token slots in the flat new_tok array (slice order) and the matrix they fill
            nm = c.N_max
            self._tok_map = [to_dev(np.concatenate([np.arange(ur[self.s_lo + i, b, 0] * nm, ur[self.s_lo + i, b, 1] * nm)
                                                    for i in range(self.s_n)]).astype(np.int64))
                             for b in range(self.B)]
            self._tok_rows = torch.zeros(max(t.numel() for t in self._tok_map), dtype=torch.int32, device=dev)
            self.ll_ld = (K + 1 + 31) // 32 * 32
            self.ll_mat = torch.zeros((self._tok_rows.numel(), self.ll_ld), dtype=torch.float32, device=dev)
        if self.score_f32:
            # the rows of block b over the local slices, one launch per step
            self._block_rows = [to_dev(np.concatenate([np.arange(rr[self.s_lo + i, b, 0], rr[self.s_lo + i, b, 1])
                                                       for i in range(self.s_n)]).astype(np.int32))
                                for b in range(self.B)]
            check(df._L.segk_fbb_make_y(df._ctx, df._cp(), C.byref(self.bt), _abi.stream()))
        self.in_batch_state = False
        self.sweep_index = 0

    # ------------------------------------------------------------------ plumbing
    def _args(self):
        df = self.df
        self.f.alpha, self.f.lms = df.f.alpha, df.f.lms
        return df._L, df._ctx, df._cp(), C.byref(self.f), C.byref(self.bt), _abi.stream()

    def _gather(self, full, b):
        """in-place all-gather of full[b] ([S, ...]): every rank contributes its slices."""
        if self.world == 1:
            return
        out = full[b].view(self.world, -1)
        self.comm.all_gather_rows(out, out[self.rank])

    def enter(self, boundaries):
        """Build the batch state (slots, token lists, all partial sums, transcripts) from the
        sequential-mode state of the components."""
        df = self.df
        L, ctx, cp, fp, bp, st = self._args()
        self.slot.copy_(df.assignments)
        if df.lm is not None:
            self.lm_big.copy_(df.lm._bigram)
        check(L.segk_fbb_collect(ctx, cp, ptr(boundaries), ptr(df.new_tok), ptr(df.n_new), st))
        for b in range(self.B):
            check(L.segk_fbb_partials(ctx, cp, fp, bp, self.s_lo, self.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
            self._gather(self.partials, b)
            if self.lm_tok is not None:
                check(L.segk_fbb_lm_fill(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], ptr(df.new_tok),
                                         ptr(df.n_new), st))
                self._gather(self.lm_tok, b)
        self.in_batch_state = True

    def rebuild_from_slots(self, boundaries):
        """Partial sums and transcripts from the current `slot` labels (checkpoint resume)."""
        df = self.df
        L, ctx, cp, fp, bp, st = self._args()
        check(L.segk_fbb_collect(ctx, cp, ptr(boundaries), ptr(df.new_tok), ptr(df.n_new), st))
        for b in range(self.B):
            check(L.segk_fbb_partials(ctx, cp, fp, bp, self.s_lo, self.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
            self._gather(self.partials, b)
            if self.lm_tok is not None:
                check(L.segk_fbb_lm_fill(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], ptr(df.new_tok),
                                         ptr(df.n_new), st))
                self._gather(self.lm_tok, b)
        self.in_batch_state = True

    def sweep(self, boundaries, n_slices_min, n_slices_max, wip, time_power_term, anneal_temp_fb=1.0,
              anneal_temp_am=1.0, viterbi=False):
        """One sweep = n_gibbs_blocks steps, all enqueued on the current stream.

        viterbi: the sweep of fb_type "viterbi" (specification tests/map_batch.py) -- per step the same span scores, then
        the MAP boundaries (segk_fbb_segment_map) and the MAP slot of every new segment (segk_fbb_assign_map) in place of the
        draws: no uniform is consumed and the temperatures have no effect.  Always the three calls, never the fused step."""
        torch = _torch()
        df = self.df
        if viterbi and df.lm is not None:
            raise SegkError("batch sweeps with fb_type=\"viterbi\" exist without a language model only: the reference's "
                            "bigram segmenter has no Viterbi mode (fb_type is \"bigram\" or \"unigram\")")
        if not self.in_batch_state:
            self.enter(boundaries)
        L, ctx, cp, fp, bp, st = self._args()
        sw = self.sweep_index
        for b in range(self.B):
            if self.lm_tok is not None:
                check(L.segk_fbb_lm_apply(ctx, cp, fp, bp, b, -1, st))
            check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
            if self.score_diag32 and self.lm_tok is None and self._fused is not False and not viterbi:
                # span scores, boundaries and slots of the block by ONE launch where the library can (segk_fbb_step_diag32)
                rc = L.segk_fbb_step_diag32(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], sw, int(n_slices_min),
                                            int(n_slices_max), float(wip), float(time_power_term), float(anneal_temp_fb),
                                            float(anneal_temp_am), ptr(df.score), ptr(boundaries), ptr(df.new_tok),
                                            ptr(df.n_new), ptr(df.out_logprob), ptr(df.status), st)
                if rc == _abi.SEGK_ERR_UNSUPPORTED:
                    self._fused = False
                else:
                    check(rc)
                    self._fused = True
                    check(L.segk_fbb_partials(ctx, cp, fp, bp, self.s_lo, self.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
                    self._gather(self.partials, b)
                    continue
            if self.score_f32:
                check(L.segk_fbb_score_f32(ctx, cp, fp, bp, ptr(self._block_rows[b]), self._block_rows[b].numel(),
                                           ptr(df.score), st))
            elif self.score_diag32:
                check(L.segk_fbb_score_diag32(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_rows[b], ptr(df.score), st))
            else:
                check(L.segk_fbb_score(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_rows[b], ptr(df.score), st))
            if viterbi:
                check(L.segk_fbb_segment_map(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], sw, int(n_slices_min),
                                             int(n_slices_max), float(wip), float(time_power_term), ptr(df.score),
                                             ptr(boundaries), ptr(df.new_tok), ptr(df.n_new), ptr(df.out_logprob),
                                             ptr(df.status), st))
                # (the fixed-variance tolerance modes take the fp64 quadratic here: the token-likelihood matrix is not formed)
                check(L.segk_fbb_assign_map(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], sw, ptr(df.new_tok),
                                            ptr(df.n_new), 1 if self.score_diag32 else 0, st))
                check(L.segk_fbb_partials(ctx, cp, fp, bp, self.s_lo, self.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
                self._gather(self.partials, b)
                continue
            check(L.segk_fbb_segment(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], sw, int(n_slices_min),
                                     int(n_slices_max), float(wip), float(time_power_term), float(anneal_temp_fb),
                                     ptr(df.score), ptr(boundaries), ptr(df.new_tok), ptr(df.n_new),
                                     ptr(df.out_logprob), ptr(df.status), st))
            if self.ll_mat is not None:
                tm = self._tok_map[b]
                rows = self._tok_rows[:tm.numel()]
                torch.index_select(df.new_tok.view(-1), 0, tm, out=rows)
                check(L.segk_fbb_token_scores(ctx, cp, fp, bp, ptr(rows), tm.numel(), ptr(self.ll_mat), self.ll_ld, st))
                check(L.segk_fbb_assign(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], sw, float(anneal_temp_am),
                                        ptr(df.new_tok), ptr(df.n_new), ptr(self.ll_mat), self.ll_ld, st))
            elif self.score_diag32:
                check(L.segk_fbb_assign_diag32(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], sw,
                                               float(anneal_temp_am), ptr(df.new_tok), ptr(df.n_new), st))
            else:
                check(L.segk_fbb_assign(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], sw, float(anneal_temp_am),
                                        ptr(df.new_tok), ptr(df.n_new), None, 0, st))
            if self.lm_tok is not None:
                check(L.segk_fbb_lm_fill(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], ptr(df.new_tok),
                                         ptr(df.n_new), st))
                self._gather(self.lm_tok, b)
                check(L.segk_fbb_lm_apply(ctx, cp, fp, bp, b, 1, st))
            check(L.segk_fbb_partials(ctx, cp, fp, bp, self.s_lo, self.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
            self._gather(self.partials, b)
        self.sweep_index += 1

    def _corpus_centre(self):
        """the corpus column mean the reduced-precision kernels centre their operands on (segk_fbatch.centre), as a device
        tensor: one pass over X in fp64 and in row order on the host, so every rank (each holds the whole corpus) gets the
        same bits"""
        c = self.df.corpus
        xh = c.X.cpu().numpy()
        mean = np.add.reduce(xh, axis=0, dtype=np.float64) / max(c.n_emb, 1)
        return _torch().from_numpy(np.ascontiguousarray(mean[:c.D])).to(_dev())

    def _bt_am32(self):
        """The batch state the float32 inner sweeps pass to the library.  A sweeper built with score_precision="f32" (diagonal)
        has `centre` and `tab32` in `bt`.  An fp64 sweeper has neither, and setting them there would change the bits of its
        outer sweeps (fbb_centre): it gets, once, a COPY of `bt` -- the same buffers -- with a centre and a table of its own."""
        if self.score_diag32:
            return self.bt
        if self._bt32 is None:
            K, D = self.df.K_max, self.df.corpus.D
            self._centre32 = self._corpus_centre()
            self._tab32_am = _torch().zeros(2 * D * K, dtype=_torch().float32, device=_dev())
            bt = _abi.FbatchDev.from_buffer_copy(self.bt)
            bt.centre, bt.tab32 = self._centre32.data_ptr(), self._tab32_am.data_ptr()
            self._bt32 = bt
        return self._bt32

    def _am_sweep_f32(self, boundaries, anneal_temp):
        """am_sweep(..., score_precision="f32") once its refusals have passed: per block prepare (which writes tab32), the token
        step in float32 by one of two routes, partials.  The route is chosen on the host from the block's token bound: the tile
        kernel (segk_fbt_assign_diag32) from AM32_TILE_MIN tokens on, segk_fbb_assign_diag32 on the unchanged token lists
        below it -- the same uniforms and the same draw (fbb_draw_row) on likelihoods of the same float32 terms.
        SEGK_AM32_TILE_MIN overrides the constant (read per sweep; 0 = always tiles): a launch-plan switch like SEGK_FBI_Z_MIB."""
        df = self.df
        bt32 = self._bt_am32()
        if not self.in_batch_state:
            self.enter(boundaries)
        L, ctx, cp, fp, _, st = self._args()
        bp = C.byref(bt32)
        try:
            tile_min = int(os.environ.get("SEGK_AM32_TILE_MIN", AM32_TILE_MIN))
        except ValueError:
            raise SegkError("SEGK_AM32_TILE_MIN must be an integer, got %r" % (os.environ.get("SEGK_AM32_TILE_MIN"),))
        pl = self.probe_ll
        ld = pl.shape[1] if pl is not None else 0
        for b in range(self.B):
            check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
            if sum(self._tok_cap[b]) >= tile_min:
                check(L.segk_fbt_assign_diag32(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], self._tok_cap[b],
                                               self.sweep_index, float(anneal_temp), ptr(df.new_tok), ptr(df.n_new), ptr(pl), ld, st))
            else:
                if pl is not None:
                    check(L.segk_fbb_set_probe(ctx, None, ptr(pl), ld))
                try:
                    check(L.segk_fbb_assign_diag32(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], self.sweep_index,
                                                   float(anneal_temp), ptr(df.new_tok), ptr(df.n_new), st))
                finally:
                    if pl is not None:
                        check(L.segk_fbb_set_probe(ctx, None, None, 0))
            check(L.segk_fbb_partials(ctx, cp, fp, bp, self.s_lo, self.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
        self.sweep_index += 1

    def am_sweep(self, boundaries, anneal_temp=1.0, score_precision=None):
        """One ACOUSTIC-MODEL batch sweep (specification tests/am_batch.py): the boundaries stay, every current
        token of block b is resampled against the statistics of all other blocks -- per block segk_fbb_prepare(b),
        segk_fbt_assign, segk_fbb_partials(b), all enqueued on the current stream.  Consumes one sweep index, the counter of
        `sweep`.  One process, no language model.
        score_precision: the precision of THIS sweep's token likelihoods, whatever the sweeper was built with.  None / "f64":
        the fp64 step (a sweeper built with reduced-precision scores refuses it, as before); "f32" (diagonal components;
        DESIGN.md 4.17.1): the Student-t terms in float32 on the hardware logarithm, on a sweeper of either precision --
        statistics, logits and draws stay fp64."""
        df = self.df
        if score_precision not in (None, "f64", "f32"):
            raise SegkError("acoustic-model batch sweeps (am_sweep) take score_precision None, 'f64' or 'f32', got %r"
                            % (score_precision,))
        if df.lm is not None:
            raise SegkError("acoustic-model batch sweeps (am_sweep) exist without a language model only: the bigram segmenter "
                            "has no inner sweeps (its reference asserts at am_n_iter > 0)")
        if self.world > 1:
            raise SegkError("acoustic-model batch sweeps (am_sweep) run in one process only (%d ranks)" % self.world)
        if score_precision == "f32":
            if df.cov_type != 1:
                raise SegkError("acoustic-model batch sweeps (am_sweep) with score_precision='f32' exist for diagonal components "
                                "only (covariance_type=\"diag\"): fixed-variance and full-covariance components take the fp64 "
                                "inner sweeps")
            if self._tok_cap is None:
                raise SegkError("acoustic-model batch sweeps (am_sweep) need a segmenter's corpus (utterances with span tables)")
            return self._am_sweep_f32(boundaries, anneal_temp)
        if self.score_precision != "f64":
            raise SegkError("acoustic-model batch sweeps (am_sweep) take score_precision='f64' only (got %r): the "
                            "reduced-precision sweepers keep their state in other coordinates" % (self.score_precision,))
        if self.fullcov and df.K_max > 1024:
            raise SegkError("the batch sampler takes full-covariance components (cov_type 2) with K_max <= 1024, got %d"
                            % df.K_max)
        if self._tok_cap is None:
            raise SegkError("acoustic-model batch sweeps (am_sweep) need a segmenter's corpus (utterances with span tables)")
        if not self.in_batch_state:
            self.enter(boundaries)
        L, ctx, cp, fp, bp, st = self._args()
        pl = self.probe_ll
        for b in range(self.B):
            check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
            check(L.segk_fbt_assign(ctx, cp, fp, bp, self.s_lo, self.s_n, b, self._n_utts[b], self._tok_cap[b], self.sweep_index,
                                    float(anneal_temp), ptr(df.new_tok), ptr(df.n_new), ptr(pl),
                                    pl.shape[1] if pl is not None else 0, st))
            check(L.segk_fbb_partials(ctx, cp, fp, bp, self.s_lo, self.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
        self.sweep_index += 1

    def cell_partials(self, b, s):
        """(counts [K], sum x [K, D], sum x^2 [K, D] -- full covariance: sum outer(x, x) [K, D, D], the packed triangle
        unfolded --) of the (block b, slice s) cell, as numpy float64."""
        K, D = self.df.K_max, self.df.corpus.D
        r = self.partials[b, s].cpu().numpy()
        cnt, sx = r[:K].copy(), r[K:K + K * D].reshape(K, D).copy()
        if not self.fullcov:
            return cnt, sx, r[K + K * D:].reshape(K, D).copy()
        tri = r[K + K * D:].reshape(K, D * (D + 1) // 2)
        sxx = np.zeros((K, D, D))
        cols, rows = np.triu_indices(D)                      # column-major lower triangle: (b, a), a >= b, b ascending
        sxx[:, rows, cols] = tri
        sxx[:, cols, rows] = tri
        return cnt, sx, sxx

    def utt_values(self, t):
        """numpy copy of a per-utterance device vector with every rank's own utterances filled in."""
        v = t.cpu().numpy().copy()
        if self.world > 1:
            lo = int(self.utt_range_np[self.s_lo, 0, 0])
            hi = int(self.utt_range_np[self.s_lo + self.s_n - 1, -1, 1])
            for plo, phi, x in self.comm.all_gather_object((lo, hi, v[lo:hi])):
                v[plo:phi] = x
        return v

    def totals(self):
        """(counts per slot as float64 numpy, total, occupied) of the current state."""
        L, ctx, cp, fp, bp, st = self._args()
        check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
        sc = self.scal.cpu().numpy()
        return self.cnt.cpu().numpy(), float(sc[0]), int(sc[1])

    def check_decode(self, D, N_max, band_W, n_slices_min, n_slices_max):
        """What decode() refuses, from host values alone (nothing is launched): the limits of segk_fbi_predict and
        segk_fbd_decode (include/segk.h), each named."""
        df = self.df
        if self.world > 1:
            raise SegkError("decode runs in one process only (%d ranks): held-out utterances are not sharded" % self.world)
        if df.lm is not None:
            raise SegkError("decode exists without a language model only: the reference has no Viterbi mode with one")
        if D != df.corpus.D:
            raise SegkError("decode: the held-out embeddings have D = %d, the model's have D = %d" % (D, df.corpus.D))
        if D > 256:
            raise SegkError("decode supports D <= 256, got %d" % D)
        if self.fullcov and D > 64:
            raise SegkError("full-covariance components (cov_type 2) support D <= 64, got %d" % D)
        if self.fullcov and df.K_max > 1024:
            raise SegkError("decode takes full-covariance components (cov_type 2) with K_max <= 1024, got %d" % df.K_max)
        if n_slices_min not in (0, 1):
            raise SegkError("decode: n_slices_min must be 0 or 1, got %r" % (n_slices_min,))
        if N_max > 64:
            if not 1 <= n_slices_max <= 64:
                raise SegkError("decode takes held-out utterances of more than 64 landmarks (N_max = %d) with a window of 1..64 "
                                "slices only (n_slices_max = %d)" % (N_max, n_slices_max))
            if band_W != n_slices_max:
                raise SegkError("decode takes held-out utterances of more than 64 landmarks (N_max = %d) only when no span longer "
                                "than the window has an embedding (no complete band for n_slices_max = %d)" % (N_max, n_slices_max))
            lds = 12 * N_max * band_W + 24 * N_max + 16 + (N_max + 15) // 16 * 16
            if lds > 160 * 1024:
                raise SegkError("decode: the banded span table of the longest held-out utterance does not fit in LDS: N_max = %d "
                                "landmarks, window W = %d: %d bytes needed, %d available" % (N_max, band_W, lds, 160 * 1024))

    def _canonical_tables(self):
        """The slot tables segk_fbb_prepare(-1) left, COPIED into the reference view's slot order -- the occupied slots in
        increasing slot order, then the empty ones, the numbering materialise() gives a serial state -- as (a reference to a
        copy of `bt` that points at the copies, the copies).  A held-out row's density is a sum over the slots in slot order:
        on these tables a live batch state gives the bits the serial state of the same model gives.  The batch state itself is
        not touched; nothing is read back."""
        torch = _torch()
        order = torch.sort((self.cnt <= 0).to(torch.int8), stable=True).indices
        ax = 0 if self.fullcov else 1                         # (full covariance: slot-major tables)
        t = dict(cnt=self.cnt.index_select(0, order), lconst=self.lconst.index_select(0, order),
                 zconst=self.zconst.index_select(0, order), half=self.half.index_select(0, order),
                 mean_t=self.mean_t.index_select(ax, order), q_t=self.q_t.index_select(ax, order))
        if self.tab32 is not None:
            t["tab32"] = self.tab32.view(-1, self.df.K_max).index_select(1, order).contiguous()
        bt = _abi.FbatchDev.from_buffer_copy(self.bt)
        for k, v in t.items():
            setattr(bt, k, v.data_ptr())
        return C.byref(bt), (bt, t)

    def decode(self, cq, boundaries, n_slices_min, n_slices_max, wip, time_power_term):
        """MAP boundaries and transcript of the HELD-OUT utterances of `cq` (a DeviceCorpus that is in no model: its rows are
        their candidate embeddings) against the frozen statistics -- UnigramAcousticWordseg.decode; specification
        tests/wordseg_decode.py; DESIGN.md 4.23.  segk_fbb_prepare(-1), one segk_fbi_predict (_diag32 on a sweeper of float32
        diagonal scores; fp64 everywhere else) over all rows of `cq`, segk_fbd_decode.  Returns a dict of device tensors,
        enqueued on the current stream, nothing read back: boundaries uint8 [n_utt, N_max], log_prob [n_utt], n_seg int32
        [n_utt], seg_embed / seg_label int32 and seg_density float64 [n_utt, N_max], label int32 / density float64 [M] (every
        candidate row), K (int64 scalar: the occupied slots).

        Read-only.  On a batch state slots, partial sums and sweep_index stay; the rows are scored on copies of the slot tables
        in the reference view's slot order (_canonical_tables), so that the densities are the bits a serial state gives.  On a serial state the tables are built from the
        current assignments and `boundaries` (the model's own; enter() -- df.new_tok / df.n_new are its workspaces) and dropped
        again (invalidate(), no materialise()).  No uniform is consumed."""
        torch = _torch()
        dev = _dev()
        self.check_decode(cq.D, cq.N_max, cq.band_W, int(n_slices_min), int(n_slices_max))
        if cq.x_dtype != self.df.corpus.x_dtype:
            raise SegkError("decode: the held-out embeddings must have the dtype of the model's")
        M, n_utt, NM = cq.n_emb, cq.n_utt, cq.N_max
        f64, i32 = torch.float64, torch.int32
        label = torch.zeros(max(M, 1), dtype=i32, device=dev)
        dens = torch.zeros(max(M, 1), dtype=f64, device=dev)
        prior_q = torch.empty(max(M, 1), dtype=f64, device=dev)
        out = dict(boundaries=torch.zeros((n_utt, NM), dtype=torch.uint8, device=dev),
                   log_prob=torch.zeros(n_utt, dtype=f64, device=dev), n_seg=torch.zeros(n_utt, dtype=i32, device=dev),
                   seg_embed=torch.full((n_utt, NM), -1, dtype=i32, device=dev),
                   seg_label=torch.full((n_utt, NM), -1, dtype=i32, device=dev),
                   seg_density=torch.full((n_utt, NM), -np.inf, dtype=f64, device=dev), label=label[:M], density=dens[:M])
        # the model's corpus as segk_fbi_predict reads it (x_dtype and D): a corpus of items, no span tables
        cv = _abi.Corpus.from_buffer_copy(self.df.corpus.c)
        cv.vec_ids = cv.durations = cv.band_ids = cv.band_dur = None
        entered = not self.in_batch_state
        if entered:
            self.enter(boundaries)
        try:
            L, ctx, cp, fp, bp, st = self._args()
            check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
            call = L.segk_fbi_predict_diag32 if self.score_diag32 else L.segk_fbi_predict
            if not entered:
                bp, canon = self._canonical_tables()          # (kept alive until the calls are enqueued)
            check(call(ctx, C.byref(cv), fp, bp, ptr(cq.X), cq.ldx, M, ptr(prior_q), ptr(label), ptr(dens), None, 0, None, 0, st))
            check(L.segk_fbd_decode(ctx, C.byref(cq.c), int(n_slices_min), int(n_slices_max), float(wip), float(time_power_term),
                                    ptr(dens), ptr(label), ptr(out["boundaries"]), ptr(out["seg_embed"]), ptr(out["seg_label"]),
                                    ptr(out["seg_density"]), ptr(out["n_seg"]), ptr(out["log_prob"]), st))
            out["K"] = (self.cnt > 0).sum()
        finally:
            if entered:
                self.invalidate()
        return out

    def invalidate(self):
        """The sequential-mode state was mutated: rebuild the batch state before the next sweep."""
        self.in_batch_state = False

    def materialise(self, boundaries=None):
        """The reference's view of the current batch state, without touching it: contiguous
        component labels in `assignments` / K, the LM tables of the LM object, and the
        sequential-mode statistics rebuilt from the assignments (Components.__init__ order)."""
        if not self.in_batch_state:
            return
        torch = _torch()
        df = self.df
        L, ctx, cp, fp, bp, st = self._args()
        check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
        check(L.segk_fbb_canonical(ctx, cp, C.byref(df.f), bp, ptr(self.remap), st))
        if self.world > 1:
            # every rank holds the slots of its own rows only
            lo, hi = int(self.row_range_np[self.s_lo, 0, 0]), int(self.row_range_np[self.s_lo + self.s_n - 1, -1, 1])
            for plo, phi, t in self.comm.all_gather_object((lo, hi, df.assignments[lo:hi].cpu())):
                df.assignments[plo:phi] = t.to(df.assignments.device)
            if boundaries is not None:          # the boundaries of the other ranks' utterances
                ulo = int(self.utt_range_np[self.s_lo, 0, 0])
                uhi = int(self.utt_range_np[self.s_lo + self.s_n - 1, -1, 1])
                for plo, phi, t in self.comm.all_gather_object((ulo, uhi, boundaries[ulo:uhi].cpu())):
                    boundaries[plo:phi] = t.to(boundaries.device)
        if df.lm is not None:
            occ = torch.nonzero(self.remap >= 0).flatten()
            K = occ.numel()
            big = df.lm._bigram
            big.zero_()
            big[:K, :K] = self.lm_big[occ][:, occ]
            df.lm._unigram.zero_()
            df.lm._unigram[:K] = self.cnt[occ].round().long()
        check(L.segk_fbgmm_init_stats(ctx, cp, C.byref(df.f), st))


class FbgmmItemSweeper(object):
    """Batch-synchronous sweeps of the STAND-ALONE mixture model (FBGMM.gibbs_sample(sync="batch")): FbgmmBatchSweeper with
    "utterance" read as "item" -- specification tests/fbgmm_items.py, C ABI `segk_fbi_assign` (include/segk.h).

    The items 0..N-1 are cut into `n_stat_blocks` slices x `n_gibbs_blocks` blocks.  Step b: segk_fbb_prepare(b) (the
    statistics of all other blocks), segk_fbi_assign (logits and draw of every considered item of block b),
    segk_fbb_partials(b).  The statistics kernels see the items as a corpus of one-landmark utterances: new_tok[i] = i,
    n_new[i] = does item i hold a slot.  One process, no language model.
    score_precision: "f64", or "f32" for diagonal components -- the Student-t terms of the item likelihoods in float32 on
    the hardware logarithm (segk_fbi_assign_diag32); statistics, logits and draws stay fp64.
    sweep(map_assign=True) is a MAP sweep (segk_fbi_assign_map / _map_diag32 in the item half).
    predict() labels and scores rows that are not in the model, read-only (segk_fbi_predict / _predict_diag32)."""

    def __init__(self, df, n_gibbs_blocks=8, n_stat_blocks=8, seed=0, group=None, score_precision="f64"):
        torch = _torch()
        c = df.corpus
        if score_precision not in ("f64", "f32"):
            raise SegkError("the stand-alone mixture model's batch sweeps take score_precision 'f64' or 'f32', got %r"
                            % (score_precision,))
        if score_precision == "f32" and df.cov_type != 1:
            raise SegkError("score_precision='f32' of the stand-alone mixture model's batch sweeps exists for diagonal components "
                            "only (covariance_type=\"diag\"; this model has %s components)"
                            % ("fixed-variance" if df.cov_type == 0 else "full-covariance"))
        self.score_precision = score_precision
        self.score_diag32 = score_precision == "f32"
        if c.n_utt:
            raise SegkError("this mixture model is the acoustic model of a segmenter (its corpus carries utterances): batch "
                            "sweeps of its tokens are the segmenter's gibbs_sample(sync=\"batch\")")
        world = get_comm(group).world
        if world > 1:
            raise SegkError("the stand-alone mixture model's batch sweeps run in one process only (%d ranks)" % world)
        if df.lm is not None:
            raise SegkError("the stand-alone mixture model's batch sweeps take no language model")
        self.fullcov = df.cov_type == 2
        if self.fullcov and c.D > 64:
            raise SegkError("full-covariance components (cov_type 2) support D <= 64, got %d" % c.D)
        if self.fullcov and df.K_max > 1024:
            raise SegkError("the batch sampler takes full-covariance components (cov_type 2) with K_max <= 1024, got %d"
                            % df.K_max)
        self.S, self.B = int(n_stat_blocks), int(n_gibbs_blocks)
        if not (1 <= self.S <= 16 and self.B >= 1):
            raise SegkError("n_stat_blocks must be in 1..16 and n_gibbs_blocks >= 1 (got %d, %d)" % (self.S, self.B))
        dev = _dev()
        self.df = df
        N, K, D = c.n_emb, df.K_max, c.D
        self.N = N
        # the items as one-landmark utterances: the corpus structure with n_utt = N, N_max = 1 and no span tables
        self.c = _abi.Corpus.from_buffer_copy(c.c)
        self.c.n_utt, self.c.N_max = N, 1
        sb = [(s * N) // self.S for s in range(self.S + 1)]
        ur = np.zeros((self.S, self.B, 2), np.int32)
        for s in range(self.S):
            n_s = sb[s + 1] - sb[s]
            for b in range(self.B):
                ur[s, b] = (sb[s] + (b * n_s) // self.B, sb[s] + ((b + 1) * n_s) // self.B)
        self.utt_range_np = ur
        self.utt_range = to_dev(ur)
        self.rec = K * (1 + D + D * (D + 1) // 2) if self.fullcov else K * (2 * D + 1)
        f64 = torch.float64
        self.partials = torch.zeros((self.B, self.S, self.rec), dtype=f64, device=dev)
        self.cnt = torch.zeros(K, dtype=f64, device=dev)
        self.mean_t = torch.zeros((K, D) if self.fullcov else (D, K), dtype=f64, device=dev)
        self.q_t = torch.zeros((K, D, D) if self.fullcov else (D, K), dtype=f64, device=dev)
        self.lconst = torch.zeros(K, dtype=f64, device=dev)
        self.zconst = torch.zeros(K, dtype=f64, device=dev)
        self.half = torch.zeros(K, dtype=f64, device=dev)
        self.scal = torch.zeros(2, dtype=f64, device=dev)
        self.slot = torch.zeros(N, dtype=torch.int32, device=dev)
        self.remap = torch.zeros(K, dtype=torch.int32, device=dev)
        self.new_tok = torch.arange(N, dtype=torch.int32, device=dev)
        self.n_new = torch.zeros(N, dtype=torch.int32, device=dev)
        self.f = _abi.FbgmmDev.from_buffer_copy(df.f)
        self.prior_rows = torch.zeros(N, dtype=f64, device=dev)
        check(df._L.segk_fbb_prior_rows(df._ctx, C.byref(self.c), C.byref(self.f), self.prior_rows.data_ptr(), _abi.stream()))
        # float32 likelihoods: the coordinates centred on the corpus column mean as in FbgmmBatchSweeper (fp64, row order, on
        # the host), and the float32 slot tables segk_fbb_prepare writes for the item kernel
        self.centre = self.tab32 = None
        if self.score_diag32:
            xh = c.X.cpu().numpy()
            mean = np.add.reduce(xh, axis=0, dtype=np.float64) / max(N, 1)
            self.centre = torch.from_numpy(np.ascontiguousarray(mean[:D])).to(dev)
            self.tab32 = torch.zeros(2 * D * K, dtype=torch.float32, device=dev)
        self.bt = _abi.FbatchDev(
            centre=self.centre.data_ptr() if self.centre is not None else None,
            tab32=self.tab32.data_ptr() if self.tab32 is not None else None,
            prior_rows=self.prior_rows.data_ptr(), n_slices=self.S, n_blocks=self.B, u_max=0, fast_dp=0,
            utt_range=self.utt_range.data_ptr(), row_range=self.utt_range.data_ptr(), partials=self.partials.data_ptr(),
            cnt=self.cnt.data_ptr(), mean_t=self.mean_t.data_ptr(), q_t=self.q_t.data_ptr(), lconst=self.lconst.data_ptr(),
            zconst=self.zconst.data_ptr(), half=self.half.data_ptr(), scal=self.scal.data_ptr(), slot=self.slot.data_ptr(),
            seed=int(seed) & (2 ** 64 - 1))
        I32 = C.c_int32 * self.S
        self._n_items = [I32(*[int(ur[s, b, 1] - ur[s, b, 0]) for s in range(self.S)]) for b in range(self.B)]
        self.probe_ll = None             # a [N, K_max] float64 device tensor: the likelihood part of the logits (tests)
        self.n_moved = torch.zeros(1, dtype=torch.int32, device=dev)     # the moved items of the last MAP sweep
        self.in_batch_state = False
        self.sweep_index = 0

    def _args(self):
        df = self.df
        self.f.alpha, self.f.lms = df.f.alpha, df.f.lms
        return df._L, df._ctx, C.byref(self.c), C.byref(self.f), C.byref(self.bt), _abi.stream()

    def enter(self):
        """Build the batch state (slots, all partial sums) from the sequential-mode assignments."""
        torch = _torch()
        L, ctx, cp, fp, bp, st = self._args()
        self.slot.copy_(self.df.assignments)
        self.n_new.copy_((self.slot >= 0).to(torch.int32))
        for b in range(self.B):
            check(L.segk_fbb_partials(ctx, cp, fp, bp, 0, self.S, b, ptr(self.new_tok), ptr(self.n_new), st))
        self.in_batch_state = True

    def sweep(self, anneal_temp=1.0, consider_unassigned=True, map_assign=False):
        """One sweep = n_gibbs_blocks steps, all enqueued on the current stream.
        map_assign: a MAP sweep (specification tests/fbgmm_items_map.py) -- every considered item takes the first slot of
        the largest log(alpha / K_max + n_k) + loglik_k (segk_fbi_assign_map / _map_diag32: no temperature, no uniform);
        the device counter behind `moved()` is zeroed on the stream first and counts the items whose slot changed.  The
        sweep takes one value of sweep_index like any other."""
        if not self.in_batch_state:
            self.enter()
        L, ctx, cp, fp, bp, st = self._args()
        pl = self.probe_ll
        if map_assign:
            self.n_moved.zero_()
            assign = L.segk_fbi_assign_map_diag32 if self.score_diag32 else L.segk_fbi_assign_map
        else:
            assign = L.segk_fbi_assign_diag32 if self.score_diag32 else L.segk_fbi_assign
        for b in range(self.B):
            check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
            if map_assign:
                check(assign(ctx, cp, fp, bp, 0, self.S, b, self._n_items[b], self.sweep_index,
                             1 if consider_unassigned else 0, ptr(self.new_tok), ptr(self.n_new), ptr(pl),
                             pl.shape[1] if pl is not None else 0, ptr(self.n_moved), st))
            else:
                check(assign(ctx, cp, fp, bp, 0, self.S, b, self._n_items[b], self.sweep_index, float(anneal_temp),
                             1 if consider_unassigned else 0, ptr(self.new_tok), ptr(self.n_new), ptr(pl),
                             pl.shape[1] if pl is not None else 0, st))
            check(L.segk_fbb_partials(ctx, cp, fp, bp, 0, self.S, b, ptr(self.new_tok), ptr(self.n_new), st))
        self.sweep_index += 1

    def moved(self):
        """Items whose slot the last MAP sweep changed (reads the device counter back: waits for the sweep)."""
        return int(self.n_moved.item())

    def reassign_orphans(self, was_assigned):
        """The orphan pass of FBGMM.set_K(..., sync="batch") (specification tests/fbgmm_set_k.py), enqueued on the current
        stream: per block b the statistics of every item that holds a slot (segk_fbb_prepare(-1)), a draw at temperature 1 for
        every item of the block that holds none but did before the cut (`was_assigned`: the old assignments, >= 0 where the
        item was assigned), segk_fbb_partials(b) -- the orphans of later blocks see those placed in earlier ones.  Always the
        fp64 likelihoods.  The pass takes one value of the sweep counter."""
        if not self.in_batch_state:
            self.enter()
        was = to_dev(np.asarray(was_assigned), np.int32)
        assert was.numel() == self.N
        L, ctx, cp, fp, bp, st = self._args()
        pl = self.probe_ll
        for b in range(self.B):
            check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
            check(L.segk_fbi_assign_orphans(ctx, cp, fp, bp, 0, self.S, b, self._n_items[b], self.sweep_index, ptr(was),
                                            ptr(self.new_tok), ptr(self.n_new), ptr(pl), pl.shape[1] if pl is not None else 0,
                                            st))
            check(L.segk_fbb_partials(ctx, cp, fp, bp, 0, self.S, b, ptr(self.new_tok), ptr(self.n_new), st))
        self._was = was                                   # (kept alive: the pass is only enqueued)
        self.sweep_index += 1

    def predict(self, Xq, want_label=True, want_density=True, want_resp=False, device_out=False, probe_ll=None):
        """Held-out rows against the fitted bank (FBGMM.predict / score_samples / predict_log_proba; specification
        tests/fbgmm_predict.py; segk_fbi_predict / _predict_diag32): every row of `Xq` [M, D] (a NumPy array or
        a device tensor, converted to the model's dtype) as an unassigned item appended to X, against the statistics of all
        items that hold a component.  Returns (labels int64 [M], log densities float64 [M], log responsibilities float64
        [M, K_max]) in the reference view's numbering -- the K active components in increasing slot order, then the empty
        ones; a label K means "would found a new component" --, None where not wanted; NumPy, or with device_out device
        tensors without a synchronisation.  probe_ll: a [M, >= K_max] float64 device tensor that receives the likelihoods in
        slot order (tests).

        Read-only.  On a batch state: segk_fbb_prepare(-1), then the call -- slots, partial sums and sweep_index stay.  On a
        serial state: the tables are built from the current assignments (enter()) and dropped again (invalidate(), no
        materialise()): assignments, K, counts and the serial statistics are not touched.  No uniform is consumed."""
        torch = _torch()
        dev = _dev()
        c = self.df.corpus
        D, K = c.D, self.df.K_max
        if isinstance(Xq, torch.Tensor):
            xq = Xq.detach().to(device=dev, dtype=c.torch_xdtype)
        else:
            xq = np.asarray(Xq)
            xq = to_dev(xq, c.x_np_dtype) if xq.ndim == 2 else xq
        if xq.ndim != 2 or xq.shape[1] != D:
            raise SegkError("predict: the query rows must be [M, %d] like the model's X, got shape %s" % (D, tuple(xq.shape)))
        xq = xq.contiguous()
        M = int(xq.shape[0])
        f64 = torch.float64
        label = torch.zeros(M, dtype=torch.int32, device=dev) if want_label else None
        dens = torch.zeros(M, dtype=f64, device=dev) if want_density else None
        resp = torch.zeros((M, K), dtype=f64, device=dev) if want_resp else None
        if M:
            prior_q = torch.empty(M, dtype=f64, device=dev)
            entered = not self.in_batch_state
            if entered:
                self.enter()
            try:
                L, ctx, cp, fp, bp, st = self._args()
                check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
                call = L.segk_fbi_predict_diag32 if self.score_diag32 else L.segk_fbi_predict
                check(call(ctx, cp, fp, bp, ptr(xq), D, M, ptr(prior_q), ptr(label), ptr(dens), ptr(resp), K, ptr(probe_ll),
                           probe_ll.shape[1] if probe_ll is not None else 0, st))
            finally:
                if entered:
                    self.invalidate()
            if resp is not None:
                # the reference view's column order: the occupied slots in increasing slot order, then the empty ones
                order = torch.sort((self.cnt <= 0).to(torch.int8), stable=True).indices
                resp = resp.index_select(1, order)
        if label is not None:
            label = label.to(torch.int64)
        out = (label, dens, resp)
        if device_out:
            return out
        return tuple(None if t is None else t.cpu().numpy() for t in out)

    cell_partials = FbgmmBatchSweeper.cell_partials

    def totals(self):
        """(counts per slot as float64 numpy, total, occupied) of the current state."""
        L, ctx, cp, fp, bp, st = self._args()
        check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
        sc = self.scal.cpu().numpy()
        return self.cnt.cpu().numpy(), float(sc[0]), int(sc[1])

    def invalidate(self):
        """The sequential-mode state was mutated: rebuild the batch state before the next sweep."""
        self.in_batch_state = False

    def materialise(self):
        """The reference's view of the current batch state, without touching it: contiguous component labels in
        `assignments` / K and the sequential-mode statistics rebuilt from them (Components.__init__ order)."""
        if not self.in_batch_state:
            return
        df = self.df
        L, ctx, cp, fp, bp, st = self._args()
        check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
        check(L.segk_fbb_canonical(ctx, cp, C.byref(df.f), bp, ptr(self.remap), st))
        check(L.segk_fbgmm_init_stats(ctx, df._cp(), C.byref(df.f), st))

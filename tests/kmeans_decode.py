"""
Executable SPECIFICATION of `SegmentalKMeansWordseg.decode` and `KMeans.predict` (`segk_kmd_decode`): boundaries
and transcript of utterances that are NOT in the model, read-only.  Test infrastructure only, like tests/wordseg_decode.py.

K-means is the clean case: segment_i (kmeans_acoustic_wordseg.py:225-332) scores an utterance's spans against the current means
WITHOUT removing the utterance's own items and takes boundaries and labels (:288, :313) before its update (:314-320), so decoding
a held-out utterance is segment_i minus its last seven lines -- nothing differs from the reference and everything is compared
bit for bit.  For an utterance of N landmarks, with the model's n_slices_min, n_slices_max, min_duration and wip:

  rows, scores   per candidate embedding x the first index and the value of max_k -sum_d (means[k, d] - x[d])^2 over ALL K_max
                 rows of `means`, inactive rows (the random means) included, in the dtype of the data
                 (argmax_neg_sqrd_norm_i / max_neg_sqrd_norm_i, kmeans_components.py:225-232); vectorised here
  span scores    vec[j] = double(score[id_j]) * dur_j + wip, -inf where vec_ids[j] == -1 or the duration is NaN
                 (get_vec_embed_neg_len_sqrd_norms, :334-351)
  boundaries,    forward_backward_kmeans_viterbi (:449-555) from cleared flags; among equal maxima the shortest span; the
  objective      reference's stepping back from a dead end (:521-533); the objective summed in the backward walk's order
  labels         per chosen segment the raw argmax row and min(row, K), the component add_item would give it
                 (kmeans_components.py:103-106; K: "would found a new component"); seg_score the UNSCALED max, as a double
  no embedding   a chosen segment whose span has no embedding (only after stepping back from a dead end) is kept: embedding -1,
                 row -1, label -1, score -inf, so that segments and boundaries stay aligned

`witness` runs the same over the building blocks of an implementation (the oracle's classes, or the reference's for the golden
vectors): its KMeansComponents over [X_train; X_held] with the held-out rows at -1 and the fitted model's arrays copied in
(re-summing would change the bits), per utterance its get_vec_embed_neg_len_sqrd_norms, forward_backward_kmeans_viterbi,
argmax_neg_sqrd_norm_i and max_neg_sqrd_norm_i; and, as a second witness of boundaries and objective, its segment_i on a deep
copy of that segmenter per utterance (segment_i asserts on a chosen segment without an embedding: those utterances are
reported, not compared).

Cases: the model of a case is trained on the first n_utt utterances of make_corpus(n_utt + HELD, ...) and the last HELD are held
out (the first n_utt of that call ARE the corpus of make_corpus(n_utt, ...): the held-out rows share the cluster centres).  Every
case is fitted twice from `random.seed(5); np.random.seed(5)`: "serial" -- two sweeps of segment_i over the utterances in index
order --, and "batch" -- two kmeans_batch_sweep --.

LDS of one wave of k_kmd_decode (restated from segmentalist_amd/csrc/segk_kmdecode.hip; tests/test_kmeans_decode_cpu.py holds it
against the source): Wc = n_slices_max when 0 < n_slices_max < N_max else N_max, cells = N_max Wc;
  register DP (N_max <= 64, windows 1..8)   8 (9 N_max + 12) + 4 (2 cells + 2 N_max + 8)
  generic walk                              8 (cells + N_max + 1) + 4 cells + N_max
each rounded up to 16 bytes.
"""
import copy
import random

import numpy as np

from oracle import np_oracle as no

HELD = 6
LDS_MAX = 160 * 1024
MODES = ("serial", "batch")

# name -> (n_utt, D, K, corpus seed, N_range, the corpus's longest span with an embedding, dtype, constructor keywords)
# n_slices_max (a keyword) is the MODEL's window where it differs from the corpus's
CASES = {
    # tests/golden/cases.KMEANS_CHAINS
    "km_tiny": (4, 3, 3, 11, (3, 9), 4, "float32", {}),
    "km_small": (12, 8, 6, 12, (3, 9), 6, "float32", {}),
    "km_mid": (40, 16, 12, 13, (3, 9), 6, "float32", {}),
    "km_f64": (8, 5, 4, 14, (3, 9), 5, "float64", {}),
    # tests/golden/cases.EDGE_CHAINS: one landmark; NaN durations and dead ends; a single initial span
    "e_km_short": (14, 6, 7, 61, (1, 5), 4, "float32", dict(p_boundary_init=0.5)),
    "e_km_mindur": (12, 6, 6, 62, (2, 8), 4, "float32", dict(p_boundary_init=0.5, min_duration=9)),
    "e_km_onespan": (10, 5, 5, 63, (3, 6), 6, "float32", dict(p_boundary_init=0.0)),
    # the D = 39 and K = 30 shapes of tests/kmeans_refit.SHAPES
    "refit_D39": (64, 39, 40, 1064, (3, 9), 6, "float32", {}),
    "refit_K30_f64": (25, 5, 30, 1025, (3, 9), 4, "float64", {}),
    "refit_K30": (33, 12, 30, 1033, (3, 9), 4, "float32", {}),
    # a held-out corpus of N_max 92 (three utterances of 92 landmarks, three short ones) on a model trained on 3..9 landmarks
    "long92_w6": (40, 16, 12, 13, (3, 9), 6, "float32", {}),
    # no window at decode (the fitted model's n_slices_max attribute set to 0: no initial segmentation exists without a
    # window) and a word insertion penalty
    "w0": (12, 8, 6, 12, (3, 9), 6, "float32", dict(decode_n_slices_max=0, wip=-0.3)),
    # a window of 12 slices
    "w12": (16, 8, 6, 77, (8, 20), 12, "float32", {}),
    # dead ends on held-out utterances only (a serial sweep asserts on one): the fitted model's min_duration attribute set to
    # 36 for decode, which cuts most spans of utterances of 5..12 landmarks (gaps of 3..11 frames, four slices at most)
    "dead_end": (12, 6, 6, 62, (5, 12), 4, "float32", dict(p_boundary_init=0.5, decode_min_duration=36)),
}
LONG = {"long92_w6": 92}


def lds_bytes(N_max, n_slices_max):
    Wc = n_slices_max if 0 < n_slices_max < N_max else N_max
    cells = N_max * Wc
    if 1 <= n_slices_max <= 8 and N_max <= 64:
        b = 8 * (9 * N_max + 12) + 4 * (2 * cells + 2 * N_max + 8)
    else:
        b = 8 * (cells + N_max + 1) + 4 * cells + N_max
    return (b + 15) // 16 * 16


def seg_kwargs(name):
    """keyword arguments of the segmenter's constructor (oracle and product alike)"""
    n_utt, D, K, seed, N_range, nmax, dtype, kw = CASES[name]
    return dict(n_slices_min=0, n_slices_max=kw.get("n_slices_max", nmax), min_duration=kw.get("min_duration", 0),
                p_boundary_init=kw.get("p_boundary_init", 0.5), init_am_assignments="rand", wip=kw.get("wip", 0))


def decode_window(name):
    """the n_slices_max decode runs with: the constructor's unless the case sets the attribute afterwards"""
    return CASES[name][7].get("decode_n_slices_max", seg_kwargs(name)["n_slices_max"])


def decode_min_duration(name):
    return CASES[name][7].get("decode_min_duration", seg_kwargs(name)["min_duration"])


def _take(corpus, keys, rename=None):
    return tuple({(rename or {}).get(k, k): d[k] for k in keys} for d in corpus)


_corpora = {}


def corpora(name):
    """(training dictionaries, held-out dictionaries) of a case; every held-out key sorts after every training key"""
    if name not in _corpora:
        from segmentalist_amd.synth import make_corpus
        n_utt, D, K, seed, N_range, nmax, dtype, kw = CASES[name]
        c = make_corpus(n_utt + HELD, D, K, seed=seed, ragged=True, n_slices_max=nmax, dtype=np.dtype(dtype).type, N_range=N_range)
        keys = sorted(c[0])
        train = _take(c, keys[:n_utt])
        if name in LONG:
            # the same seed: the same cluster centres
            lg = make_corpus(3, D, K, seed=seed, N=LONG[name], ragged=False, n_slices_max=nmax, dtype=np.dtype(dtype).type)
            held = _take(c, keys[-3:], {k: "x" + k for k in keys})
            for d, e in zip(held, _take(lg, sorted(lg[0]), {k: "y" + k for k in lg[0]})):
                d.update(e)
        else:
            held = _take(c, keys[-HELD:])
        _corpora[name] = (train, held)
    return _corpora[name]


_fitted = {}


def fitted(name, mode):
    """the oracle's segmenter of a case after its two sweeps (shared: do not modify).  `random` / `np.random` are left where
    they were."""
    if (name, mode) not in _fitted:
        n_utt, D, K = CASES[name][:3]
        st, nst = random.getstate(), np.random.get_state()
        try:
            random.seed(5); np.random.seed(5)
            ref = no.SegmentalKMeansWordseg(K, *corpora(name)[0], **seg_kwargs(name))
            for _ in range(2):
                if mode == "serial":
                    for i in range(ref.utterances.D):
                        ref.segment_i(i)
                else:
                    no.kmeans_batch_sweep(ref, n_blocks=n_blocks(name))
        finally:
            random.setstate(st); np.random.set_state(nst)
        _fitted[(name, mode)] = ref
    return _fitted[(name, mode)]


def n_blocks(name):
    return min(8, CASES[name][0])


def product_fitted(name, mode, **kw):
    """the product's segmenter of a case brought to the same state: sync="sequential" after two sweeps of segment_i in index
    order, or sync="batch" with its batch state live after two batch sweeps"""
    import torch
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    K = CASES[name][2]
    st, nst = random.getstate(), np.random.get_state()
    try:
        random.seed(5); np.random.seed(5)
        seg = kaw.SegmentalKMeansWordseg(K, *corpora(name)[0], sync="sequential" if mode == "serial" else "batch",
                                         n_stat_blocks=n_blocks(name), **dict(seg_kwargs(name), **kw))
    finally:
        random.setstate(st); np.random.set_state(nst)
    for _ in range(2):
        if mode == "serial":
            for i in range(seg.utterances.D):
                seg._segment_i_async(i)
        else:
            seg.batch_sweep_async()
    torch.cuda.synchronize()
    seg._dk.check_status()
    seg.n_slices_max = decode_window(name)
    seg.min_duration = decode_min_duration(name)
    return seg


class Tables(object):
    """the held-out utterances as an implementation's containers: stacked rows, Utterances with p_boundary_init = 0 (no
    np.random draw) and the model's n_slices_min / n_slices_max / min_duration"""

    def __init__(self, held, n_slices_min, n_slices_max, min_duration, impl=no):
        rows, vec_ids, self.labels = impl.process_embeddings(held[0], held[1])
        self.Xq = np.asarray(rows)
        self.u = impl.Utterances([len(held[3][k]) for k in self.labels], vec_ids, [held[2][k] for k in self.labels],
                                 [held[3][k] for k in self.labels], p_boundary_init=0, n_slices_min=n_slices_min,
                                 n_slices_max=n_slices_max, min_duration=min_duration)


class Census(object):
    def __init__(self):
        self.dead_end_starts = self.dead_windows = self.hit_zero = 0


def rows_and_scores(means, Xq, chunk=2048):
    """per row of Xq the first index and the value of the maximum of neg_sqrd_norm over all rows of `means`, in the dtype of
    the data"""
    means = np.asarray(means)
    Xq = np.asarray(Xq, dtype=means.dtype)
    rows = np.zeros(len(Xq), np.int64)
    score = np.zeros(len(Xq), means.dtype)
    for lo in range(0, len(Xq), chunk):
        d = means[None, :, :] - Xq[lo:lo + chunk, None, :]
        nsn = -(d * d).sum(axis=2)
        rows[lo:lo + chunk] = np.argmax(nsn, axis=1)
        score[lo:lo + chunk] = np.max(nsn, axis=1)
    return rows, score


def viterbi(vec, N, n_slices_max, census):
    """forward_backward_kmeans_viterbi (kmeans_acoustic_wordseg.py:449-555), n_slices_min in {0, 1}: (objective, flags)"""
    W = n_slices_max if n_slices_max else N
    g = np.zeros(N)

    def q_of(t):
        lo, i = max(0, t - W), t * (t - 1) // 2
        return i, vec[i + lo:i + t] + g[lo:t]

    for t in range(1, N):
        q = q_of(t)[1]
        g[t] = np.max(q)
        census.dead_windows += int(g[t] == -np.inf)
    b = np.zeros(N, bool)
    b[N - 1] = True
    t, total = N, 0.0
    while True:
        i, q = q_of(t)
        if np.all(q == -np.inf):
            census.dead_end_starts += 1
            while np.all(q == -np.inf):
                t -= 1
                if t == 0:
                    census.hit_zero += 1
                    break
                i, q = q_of(t)
            b[t - 1] = True
        k = int(np.argmax(q[::-1])) + 1
        total += vec[i + t - k]
        if t - k - 1 < 0:
            break
        b[t - k - 1] = True
        t -= k
    return total, b


class Dec(object):
    FIELDS = ("boundaries", "objective", "seg_offsets", "seg_start", "seg_end", "seg_embed", "seg_row", "seg_label", "seg_score",
              "K")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])
        self.rows, self.score, self.tables = kw.get("rows"), kw.get("score"), kw.get("tables")

    def as_dict(self):
        return {k: np.asarray(getattr(self, k)) for k in self.FIELDS}


def _pack(u, bounds, totals, segs, K, **kw):
    b = np.zeros((u.D, u.N_max), bool)
    for i, f in enumerate(bounds):
        b[i, :len(f)] = f
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    flat = [x for s in segs for x in s]
    col = lambda j, dt: np.array([x[j] for x in flat], dtype=dt)
    return Dec(boundaries=b, objective=np.array(totals, np.float64), seg_offsets=offs, seg_start=col(0, np.int64),
               seg_end=col(1, np.int64), seg_embed=col(2, np.int64), seg_row=col(3, np.int64), seg_label=col(4, np.int64),
               seg_score=col(5, np.float64), K=int(K), **kw)


def _segments(flags):
    ends = np.flatnonzero(flags) + 1
    return list(zip(np.concatenate([[0], ends[:-1]]), ends))


def decode_spec(means, K, tables, n_slices_max, wip, census=None):
    """The specification over a model's `means` [K_max, D] (the dtype of the data) and K."""
    census = census if census is not None else Census()
    u = tables.u
    rows, score = rows_and_scores(means, tables.Xq)
    wide = score.astype(np.float64)
    bounds, totals, segs = [], [], []
    for i in range(u.D):
        N = u.lengths[i]
        tri = N * (N + 1) // 2
        ids, dur = np.asarray(u.vec_ids[i, :tri]), np.asarray(u.durations[i, :tri], np.float64)
        ok = (ids != -1) & ~np.isnan(dur)
        with np.errstate(invalid="ignore"):
            vec = np.where(ok, wide[np.where(ok, ids, 0)] * np.where(ok, dur, 1.0), -np.inf) + wip
        total, b = viterbi(vec, N, n_slices_max, census)
        out = []
        for s, e in _segments(b):
            x = int(u.vec_ids[i, e * (e - 1) // 2 + s])
            out.append((s, e, x, rows[x], min(rows[x], K), wide[x]) if x != -1 else (s, e, -1, -1, -1, -np.inf))
        bounds.append(b); totals.append(total); segs.append(out)
    return _pack(u, bounds, totals, segs, K, rows=rows, score=score, tables=tables)


_decoded = {}


def decoded(name, mode):
    """(specification of a case on the oracle's fitted model, census); shared: do not modify"""
    if (name, mode) not in _decoded:
        ref = fitted(name, mode)
        kw = seg_kwargs(name)
        c = ref.acoustic_model.components
        census = Census()
        t = Tables(corpora(name)[1], kw["n_slices_min"], decode_window(name), decode_min_duration(name))
        _decoded[(name, mode)] = (decode_spec(c.means, c.K, t, decode_window(name), kw["wip"], census), census)
    return _decoded[(name, mode)]


class OracleImpl(object):
    process_embeddings = staticmethod(no.process_embeddings)
    Utterances = no.Utterances
    KMeansComponents = no.KMeansComponents
    Segmenter = no.SegmentalKMeansWordseg
    viterbi = staticmethod(no.forward_backward_kmeans_viterbi)


class _Model(object):
    def __init__(self, components):
        self.components = components


def witness(name, mode, impl):
    """The serial witness over an implementation's classes -> (Dec, the objectives of segment_i on a deep copy per utterance
    (NaN where it asserted), the flags it left).  The model's arrays come from the oracle's fitted segmenter."""
    ref = fitted(name, mode)
    kw = dict(seg_kwargs(name), n_slices_max=decode_window(name), min_duration=decode_min_duration(name))
    train, held = corpora(name)
    both = tuple(dict(a, **b) for a, b in zip(train, held))
    rows, vec_ids, labels = impl.process_embeddings(both[0], both[1])
    X = np.asarray(rows)
    n_train = ref.utterances.D
    assert labels[:n_train] == sorted(train[0]) and labels[n_train:] == sorted(held[0])
    rc = ref.acoustic_model.components
    n_rows = rc.N
    assert np.array_equal(X[:n_rows], rc.X) and X.dtype == rc.X.dtype
    st = np.random.get_state()
    try:
        c = impl.KMeansComponents(X, -1 * np.ones(len(X), dtype=np.int64), rc.K_max)
    finally:
        np.random.set_state(st)
    c.means, c.mean_numerators, c.counts = rc.means.copy(), rc.mean_numerators.copy(), rc.counts.copy()
    c.random_means, c.K = rc.random_means.copy(), rc.K
    c.assignments[:n_rows] = rc.assignments
    u = impl.Utterances([len(both[3][k]) for k in labels], vec_ids, [both[2][k] for k in labels], [both[3][k] for k in labels],
                        p_boundary_init=0, n_slices_min=kw["n_slices_min"], n_slices_max=kw["n_slices_max"],
                        min_duration=kw["min_duration"])
    for i in range(n_train):
        u.boundaries[i, :] = False
        u.boundaries[i, :ref.utterances.N_max] = ref.utterances.boundaries[i][:u.N_max]
    seg = object.__new__(impl.Segmenter)
    seg.acoustic_model, seg.utterances = _Model(c), u
    seg.n_slices_min, seg.n_slices_max, seg.wip = kw["n_slices_min"], kw["n_slices_max"], kw["wip"]
    bounds, totals, segs, totals2, bounds2 = [], [], [], [], []
    for i in range(n_train, u.D):
        N = u.lengths[i]
        tri = N * (N + 1) // 2
        vec = seg.get_vec_embed_neg_len_sqrd_norms(u.vec_ids[i, :tri], u.durations[i, :tri])
        total, b = impl.viterbi(vec, N, kw["n_slices_min"], kw["n_slices_max"])
        out = []
        for s, e in _segments(b):
            x = int(u.vec_ids[i, e * (e - 1) // 2 + s])
            if x == -1:
                out.append((s, e, -1, -1, -1, -np.inf))
            else:
                r = int(c.argmax_neg_sqrd_norm_i(x))
                out.append((s, e, x - n_rows, r, min(r, c.K), np.float64(c.max_neg_sqrd_norm_i(x))))
        bounds.append(np.array(b, bool)); totals.append(total); segs.append(out)
        twin = copy.deepcopy(seg)
        try:
            totals2.append(twin.segment_i(i))
        except AssertionError:
            totals2.append(np.nan)
        bounds2.append(np.array(twin.utterances.boundaries[i, :N], bool))
    held_u = Tables(held, kw["n_slices_min"], kw["n_slices_max"], kw["min_duration"]).u
    return _pack(held_u, bounds, totals, segs, c.K), np.array(totals2, np.float64), bounds2


def assert_same(got, want, what=""):
    """every field of two results (Dec, dict or the product's KMeansDecoded), bit for bit"""
    g = got.as_dict() if isinstance(got, Dec) else got if isinstance(got, dict) else {k: np.asarray(getattr(got, k)) for k in Dec.FIELDS}
    w = want.as_dict() if isinstance(want, Dec) else want
    for k in Dec.FIELDS:
        a, b = np.asarray(g[k]), np.asarray(w[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        assert np.array_equal(a, b), (what, k, a, b)

"""
The carry-over of the delta score pass (segk_score_hint.hip, k_hint_merge): a row whose winner of the previous hinted call is an
unchanged mean keeps (label, score) when every changed mean's current filter value lies below its hinted score by the
certificate's slack -- whatever the base pass holds.  That decides the near-tie rows the certificate must queue sweep after
sweep.  The near-ties are made on purpose: several large clusters get a TWIN, another row of `means` equal to theirs up to a
relative perturbation of 1e-4 -- far inside the filter's margin, not an exact duplicate --, so that every row of those clusters
fails the certificate and reaches the band stage (checked on the CPU below, against the margin's own formula).

Every direct call is compared with the C oracle, every sequence is repeated under SEGK_SCORE_DELTA=0 and SEGK_SCORE_HINT=0 with
equal bits, and segk_kmeans_stage_counts says how many rows a call queued for the band stage ([0]) and for the full scan ([1]).
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests.test_filter_bounds_cpu import _resid_norms
from tests.test_gpu_kmeans_delta import MODES, _problem, _Scorer, _setenv, _snapshot, gpu  # noqa: F401

SHAPES = {"three_tiles": (3000, 20, 70, 21, 4), "two_lds_ranges": (6000, 20, 1100, 22, 40), "headline_instantiation": (8192, 100, 1000, 23, 40)}


class _Twins(object):
    """A _problem with `pairs` twin pairs (i, j): i one of the largest clusters, j one of the smallest, means[j] = means[i] up to
    1e-4 relative; `rows` = the rows whose two best components are such a pair."""

    def __init__(self, n, D, K, seed, pairs):
        self.X, means, self.rs = _problem(n, D, K, seed)
        lab = np.argmax(self.X.astype(np.float64) @ means.T.astype(np.float64) - 0.5 * (means.astype(np.float64) ** 2).sum(1), axis=1)
        order = np.bincount(lab, minlength=K).argsort(kind="stable")[::-1]
        self.big = [int(k) for k in order[:pairs]]
        self.small = [int(k) for k in order[::-1][:pairs]]
        assert not set(self.big) & set(self.small)
        for i, j in zip(self.big, self.small):
            means[j] = means[i] * (np.float32(1.0) + np.float32(1e-4) * self.rs.choice([-1.0, 1.0], D).astype(np.float32))
        assert len(np.unique(means, axis=0)) == K
        self.means = means
        self.rows = np.flatnonzero(np.isin(lab, self.big))
        self.lab = lab
        # components that are neither: free to be moved by a test
        self.free = [int(k) for k in order[pairs:K - pairs]]


def _twins(shape):
    n, D, K, seed, pairs = SHAPES[shape]
    return _Twins(n, D, K, seed, pairs)


def _tau_slack(X, means):
    """Per row: tau - 2 E of k_hint_merge / filter_tau_h1 in numpy (float64), the largest gap of two TRUE filter-domain scores
    at which their computed filter values are certainly within tau: such a pair is never certified."""
    D = X.shape[1]
    u = 2.0 ** -24
    KP = (D + 15) & ~15
    xn = np.linalg.norm(X.astype(np.float64), axis=1)
    M = np.linalg.norm(means.astype(np.float64), axis=1).max()
    ex = _resid_norms(X)[0]
    Em = _resid_norms(means)[0].max()
    e1 = (1.02 * (KP + 16) + 16.0) * u * (xn * M + 0.5 * M * M)
    e2 = (D // 8 + 13) * u * (xn + M) ** 2
    rnd = np.minimum((xn + ex) * Em + ex * M, 1.01 * 2.0 ** -10 * xn * M)
    tau = 1.25 * (2.0 * e1 + e2) + 2.5 * rnd
    return tau - 2.0 * (e1 + rnd)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_twin_rows_are_near_ties_cpu(shape):
    """The construction, with the oracle alone: for every row of a twin cluster the pair (i, j) holds the two best reference
    scores, and their gap in the filter's domain (half the score) is inside tau - 2 E: the certificate cannot pass."""
    from oracle import c_oracle as co
    t = _twins(shape)
    assert t.rows.size >= 100, t.rows.size
    others = np.delete(t.means, t.big + t.small, axis=0)
    s_other = co.kmeans_max_argmax(others, t.X, t.rows)[0]
    slack = _tau_slack(t.X, t.means)[t.rows]
    s_i = np.empty(t.rows.size)
    s_j = np.empty(t.rows.size)
    for i, j in zip(t.big, t.small):
        sel = t.lab[t.rows] == i
        s_i[sel] = co.kmeans_max_argmax(t.means[i:i + 1], t.X, t.rows[sel])[0]
        s_j[sel] = co.kmeans_max_argmax(t.means[j:j + 1], t.X, t.rows[sel])[0]
    assert (np.minimum(s_i, s_j) > s_other).all()
    gap = 0.5 * np.abs(s_i - s_j)
    print("twin rows %d, largest gap / (tau - 2E): %.3f" % (t.rows.size, (gap / slack).max()))
    assert (gap < slack).all()


_ORACLE = {}


class _CScorer(_Scorer):
    """_Scorer whose oracle results are computed once per (rows, means) and shared by the three modes."""

    def score(self, remap=None, **kw):
        import torch
        from oracle import c_oracle as co
        d = self.c.dev
        d.score_rows(hint_remap=self.ident if remap is None else remap, **kw)
        torch.cuda.synchronize()
        k, s = d.cand_k.cpu().numpy().copy(), d.cand_s.cpu().numpy().copy()
        if not kw:
            key = (self.X.shape, hash(self.X.tobytes()), hash(self.means.tobytes()))
            if key not in _ORACLE:
                want_s, want_k = co.kmeans_max_argmax(self.means, self.X)
                _ORACLE[key] = (want_s.astype(np.float64), want_k)
            want_s, want_k = _ORACLE[key]
            assert np.array_equal(k, want_k)
            assert np.array_equal(s, want_s)
        return k, s, d.delta_stats()


def _counts(sc):
    from segmentalist_amd import _abi
    d = sc.c.dev
    out = (C.c_int32 * 2)()
    _abi.check(_abi.lib().segk_kmeans_stage_counts(d._ctx, C.byref(d.cand), out, _abi.stream()))
    return int(out[0]), int(out[1])


def _call(sc, **kw):
    """One hinted call -> (cand_k, cand_s, delta statistics, (band-stage rows, full-scan rows))."""
    k, s, st = sc.score(**kw)
    return k, s, st, _counts(sc)


def _prelude(sc):
    """-> [the base call, the settled call].  The base call starts from the true winners but has nothing to carry: the
    constructor's labels are no hints, so a first call finds the winners, and an un-hinted call then drops the state."""
    _call(sc)
    sc.c.dev.score_rows()
    return [_call(sc), _call(sc)]


def _run(monkeypatch, make, steps):
    """The base call, the settled call, then (edit, call) per step, in the three modes: equal bits; -> the delta mode's
    (cand_k, cand_s, delta statistics, stage counts) per call."""
    res = {}
    for name, env in MODES:
        _setenv(monkeypatch, env)
        sc = make()
        out = _prelude(sc)
        for step in steps:
            step(sc)
            out.append(_call(sc))
        res[name] = out
    for name in ("full", "nohint"):
        for i, (a, b) in enumerate(zip(res["delta"], res[name])):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, i)
    return res["delta"]


def _edit(fn):
    def step(sc):
        m = sc.means.copy()
        fn(m)
        sc.write(m)
    return step


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_carry_fires(gpu, monkeypatch, shape):
    """The base call queues the twin clusters' rows; the same call again queues at most the rows the full scan decided (they have
    no recorded label); with one distant mean edited in between -- a delta call with one packed tile -- the twin clusters' rows
    are still carried."""
    t = _twins(shape)
    k_far = t.free[-1]

    def far(m):
        m[k_far] = m[k_far] * np.float32(1.01)

    out = _run(monkeypatch, lambda: _CScorer(t.X, t.means), [lambda sc: None, _edit(far)])
    cnt = [o[3] for o in out]
    st = [o[2] for o in out]
    print("stage counts per call:", cnt, "delta stats:", st, "twin rows:", t.rows.size)
    assert st[0][0] == 0 and st[1][0] == 1, st
    assert t.X.shape[0] // 2 > cnt[0][0] >= t.rows.size > 0, (cnt, t.rows.size)     # the near-ties, not every row
    for i in (1, 2):
        assert cnt[i][0] <= cnt[i - 1][1], (i, cnt)                       # at most the rows without a recorded label
        assert cnt[i][0] <= cnt[0][0] // 8, (i, cnt)
    assert st[3][:3] == (1, 1, 1), st
    assert cnt[3][0] <= t.rows.size // 8, (cnt, t.rows.size)


@pytest.mark.gpu
def test_a_changed_column_takes_rows_over(gpu, monkeypatch):
    """Rows that were carried must follow a changed mean that beats their winner: another component moved onto a twin cluster's
    centroid, to within 1e-4 of the winner, bit-identical to the winner with a lower index (the first maximum moves to it) and
    with a higher index (it does not)."""
    t = _twins("three_tiles")
    by_index = sorted(t.big)
    i_hi, i_onto, i_near, i_lo = by_index             # i_hi duplicated at a higher index, i_lo at a lower one
    free = sorted(t.free)
    k_onto, k_near = free[1], free[2]
    k_lo = [k for k in free if k < i_lo and k not in (k_onto, k_near)][0]
    k_hi = [k for k in free if k > i_hi and k not in (k_onto, k_near, k_lo)][-1]

    def onto(m):
        m[k_onto] = t.X[t.lab == i_onto].mean(0)

    signs = t.rs.choice([-1.0, 1.0], t.means.shape[1]).astype(np.float32)      # (drawn once: the three modes get the same edit)

    def near(m):
        m[k_near] = m[i_near] * (np.float32(1.0) + np.float32(1e-4) * signs)

    def lower(m):
        m[k_lo] = m[i_lo]

    def higher(m):
        m[k_hi] = m[i_hi]

    out = _run(monkeypatch, lambda: _CScorer(t.X, t.means), [_edit(onto), _edit(near), _edit(lower), _edit(higher)])
    cnt = [o[3] for o in out]
    print("stage counts per call:", cnt, "delta stats:", [o[2] for o in out])
    assert cnt[1][0] <= cnt[0][0] // 8, cnt                               # the settled call carried the twin rows
    k1 = out[1][0]
    assert (out[2][0][k1 == i_onto] == k_onto).any()
    assert (out[3][0] == k_near).any()
    had = np.flatnonzero(out[3][0] == i_lo)
    assert had.size > 0 and (out[4][0][had] == k_lo).all()
    had = np.flatnonzero(out[4][0] == i_hi)
    assert had.size > 0 and (out[5][0][had] == i_hi).all()


@pytest.mark.gpu
def test_a_mean_changes_below_the_images_resolution(gpu, monkeypatch):
    """One more twin, equal to its original but for two ulps in one coordinate, nudged by one to three ulps at a time in both
    directions: the exact argmax of some rows flips between the two while no image column changes.  While a mean has changed
    that the packed image does not hold, nothing may be carried."""
    t = _twins("three_tiles")
    i2, j2 = t.big[0], t.free[0]
    m0 = t.means.copy()
    m0[j2] = m0[i2]
    m0[j2, 3] = np.nextafter(np.nextafter(m0[i2, 3], np.float32(9.0)), np.float32(9.0))

    def nudge(ulps):
        def fn(m):
            for _ in range(abs(ulps)):
                m[j2, 3] = np.nextafter(m[j2, 3], np.float32(9.0 if ulps > 0 else -9.0))
        return _edit(fn)

    # offsets from the original's coordinate: 2 -> 3 -> 1 -> -2 -> -1 -> 2 (never 0: that would be an exact duplicate)
    out = _run(monkeypatch, lambda: _CScorer(t.X, m0), [nudge(1), nudge(-2), nudge(-3), nudge(1), nudge(3)])
    cnt = [o[3] for o in out]
    st = [o[2] for o in out]
    print("stage counts per call:", cnt, "delta stats:", st)
    assert cnt[1][0] <= cnt[0][0] // 8, cnt
    flips = 0
    for c in range(2, len(out)):
        flips += int((out[c][0] != out[c - 1][0]).sum())
        if st[c][0] == 1 and st[c][1] == 0:                               # a delta call, and no image column has changed
            assert cnt[c][0] >= t.rows.size, (c, cnt)
    assert flips > 0


@pytest.mark.gpu
def test_the_callers_hints_are_not_trusted(gpu, monkeypatch):
    """cand_k overwritten in place between calls -- garbage, -1, the twin's label, a constant: a wrong hint costs only time."""
    import torch
    t = _twins("three_tiles")
    n, K = t.X.shape[0], t.means.shape[0]
    twin_of = np.arange(K)
    for i, j in zip(t.big, t.small):
        twin_of[i], twin_of[j] = j, i
    rs = np.random.RandomState(3)
    junk = rs.choice(np.array([-1, -7, K, K + 5, 2 ** 30, 2 ** 29 | 3, 2 ** 31 - 1] + list(range(K)), dtype=np.int64), n)

    def hints(fn):
        def step(sc):
            d = sc.c.dev
            torch.cuda.synchronize()
            cur = d.cand_k.cpu().numpy()
            d.cand_k.copy_(torch.from_numpy(np.ascontiguousarray(fn(cur)).astype(np.int32)).to(d.cand_k.device))
        return step

    steps = [hints(lambda k: junk), lambda sc: None, hints(lambda k: np.full(n, -1)), lambda sc: None,
             hints(lambda k: twin_of[k]), lambda sc: None, hints(lambda k: np.full(n, t.big[0])), lambda sc: None]
    out = _run(monkeypatch, lambda: _CScorer(t.X, t.means), steps)
    cnt = [o[3] for o in out]
    print("stage counts per call:", cnt)
    for c in range(3, len(out), 2):                                       # the call after each overwritten one carries again
        assert cnt[c][0] <= cnt[0][0] // 8, (c, cnt)


@pytest.mark.gpu
def test_state_hygiene(gpu, monkeypatch):
    """An un-hinted call, an id list, a sub-range, a second table on the same context, a relabelling that is not the identity:
    the next call carries nothing (the queue is back at the base call's level), the one after it does again."""
    import torch
    t = _twins("three_tiles")
    t2 = _Twins(3000, 20, 70, 24, 4)
    K = t.means.shape[0]
    for name, env in MODES[:2]:
        _setenv(monkeypatch, env)
        a, b = _CScorer(t.X, t.means), _CScorer(t2.X, t2.means)
        pre = _prelude(a)
        base, low = pre[0][3][0], pre[1][3][0]
        assert base >= t.rows.size
        if name == "delta":
            assert low <= base // 8, (base, low)
        ids = torch.arange(100, 900, dtype=torch.int32, device="cuda")
        between = [lambda: a.c.dev.score_rows(), lambda: a.score(ids=ids), lambda: a.score(row0=64, n=1000), lambda: b.score()]
        for i, fn in enumerate(between):
            fn()
            c1, c2 = _call(a)[3][0], _call(a)[3][0]
            print(name, "disturbance", i, "queue then:", c1, c2)
            if name == "delta":
                assert c1 >= t.rows.size and c2 <= base // 8, (i, base, c1, c2)
        perm = np.arange(K)
        perm[[0, 1]] = perm[[1, 0]]
        a.write(t.means[perm])
        c1 = _call(a, remap=torch.from_numpy(perm.astype(np.int32)).cuda())
        want_s, want_k = _oracle(a)
        assert np.array_equal(c1[0], want_k) and np.array_equal(c1[1], want_s)
        c2 = _call(a)
        if name == "delta":
            assert c1[2][0] == 0 and c1[3][0] >= t.rows.size, c1[2:]
            assert c2[3][0] <= base // 8, (base, c2[3])


def _oracle(sc):
    from oracle import c_oracle as co
    want_s, want_k = co.kmeans_max_argmax(sc.means, sc.X)
    return want_s.astype(np.float64), want_k


@pytest.mark.gpu
def test_chain(gpu, monkeypatch):
    """400 utterances x 12 landmarks, D = 20, K = 70, 30 sweeps, one mean nudged before every fourth sweep from sweep 18 on: the
    states are equal in the three modes, and delta sweeps queue fewer than half the rows the last full sweep queued."""
    from segmentalist_amd import _abi
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(400, 20, 70, seed=0, N=12, n_slices_max=6)
    res = {}
    for name, env in MODES:
        _setenv(monkeypatch, env)
        random.seed(0); np.random.seed(0)
        seg = kaw.SegmentalKMeansWordseg(70, *corpus, n_slices_max=6, init_am_assignments="spread", sync="batch")
        states, stats, queue = [], [], []
        for it in range(30):
            if it >= 18 and it % 4 == 2:
                seg._dk.means[it % 7] *= 1.0 + 1e-3
                seg._dk.prepare()
            seg.batch_sweep_async()
            gpu.cuda.synchronize()
            out = (C.c_int32 * 2)()
            _abi.check(_abi.lib().segk_kmeans_stage_counts(_abi.ctx(), C.byref(seg._dk.cand), out, _abi.stream()))
            states.append(_snapshot(seg))
            stats.append(seg._dk.delta_stats())
            queue.append(int(out[0]))
        seg._dk.check_status()
        res[name] = (states, stats, queue)
    for name in ("full", "nohint"):
        for it, (x, y) in enumerate(zip(res["delta"][0], res[name][0])):
            for i, (p, q) in enumerate(zip(x, y)):
                assert np.array_equal(p, q, equal_nan=True), (name, it, i)
    stats, queue = res["delta"][1], res["delta"][2]
    print("delta stats per sweep:", stats)
    print("band-stage rows per sweep:", queue, "every pass full:", res["full"][2])
    below, last_full = 0, None
    for s, q in zip(stats, queue):
        if s[0] == 0:
            last_full = q
        elif s[0] == 1 and last_full is not None and 2 * q < last_full:
            below += 1
    assert below >= 3, (stats, queue)

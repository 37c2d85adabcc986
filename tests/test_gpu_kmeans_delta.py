"""
The delta score pass of the hinted k-means path (segk_score_hint.hip): while a score call repeats on the same rows, K1 multiplies
only the component columns whose fp16x2 image changed since the last full ("base") pass, and the hint waves take a row's hinted
score over from the previous call when that mean's bits have not changed.  Results never depend on it: everything here is
compared bit for bit with the same calls under SEGK_SCORE_DELTA=0 (every pass full) and SEGK_SCORE_HINT=0 (no hints at all),
and the direct score calls with the C oracle as well.  segk_kmeans_delta_stats says which mode a call took, so that a test that
never left full mode cannot pass.
"""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = (("delta", {"SEGK_SCORE_HINT": "1"}), ("full", {"SEGK_SCORE_HINT": "1", "SEGK_SCORE_DELTA": "0"}),
         ("nohint", {"SEGK_SCORE_HINT": "0"}))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _setenv(monkeypatch, env):
    for k in ("SEGK_SCORE_HINT", "SEGK_SCORE_DELTA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _snapshot(seg):
    dk = seg._dk
    return [t.cpu().numpy().copy() for t in (seg._dev_bounds, dk.cand_k, dk.cand_s, dk.new_tok, dk.new_k, dk.n_new, dk.means,
                                              dk.counts, dk.K)]


def _chain(torch, monkeypatch, corpus, K, sweeps, env, n_batches=1, between=None):
    """`sweeps` batch sweeps -> (state after every sweep, delta statistics after every sweep)."""
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    _setenv(monkeypatch, env)
    random.seed(0); np.random.seed(0)
    seg = kaw.SegmentalKMeansWordseg(K, *corpus, n_slices_max=6, init_am_assignments="spread", sync="batch", n_batches=n_batches)
    states, stats = [], []
    for it in range(sweeps):
        if between is not None:
            between(seg, it)
        seg.batch_sweep_async()
        torch.cuda.synchronize()
        states.append(_snapshot(seg))
        stats.append(seg._dk.delta_stats())
    seg._dk.check_status()
    return states, stats


def _same_chains(torch, monkeypatch, corpus, K, sweeps, **kw):
    out = {}
    for name, env in MODES:
        out[name] = _chain(torch, monkeypatch, corpus, K, sweeps, env, **kw)
    for name in ("full", "nohint"):
        for it, (a, b) in enumerate(zip(out["delta"][0], out[name][0])):
            for i, (x, y) in enumerate(zip(a, b)):
                assert np.array_equal(x, y, equal_nan=True), (name, it, i)
    return out["delta"][1]


def test_base_shape_chain_reaches_every_mode(gpu, monkeypatch):
    """400 utterances x 12 landmarks, D = 20, K = 70: three tiles, the last one partly filled, 22 800 rows (no multiple of 64);
    30 sweeps.  From sweep 18 on one mean is nudged before every fourth sweep (the chain has stopped moving by then), so that
    delta sweeps with packed tiles, the full pass that makes a new base once the table rests, and delta sweeps without any tile
    follow one another."""
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(400, 20, 70, seed=0, N=12, n_slices_max=6)

    def between(seg, it):
        if it >= 18 and it % 4 == 2:
            dk = seg._dk
            dk.means[it % 7] *= 1.0 + 1e-3
            dk.prepare()

    stats = _same_chains(gpu, monkeypatch, corpus, 70, 30, between=between)
    print("delta stats per sweep (mode, changed columns, packed tiles, skipped positions):", stats)
    delta = [s for s in stats if s[0] == 1]
    assert len(delta) >= 10, stats
    assert sum(1 for s in delta if s[2] == 0) >= 3, stats
    assert sum(1 for s in delta if s[2] >= 1) >= 3, stats
    assert sum(s[3] for s in delta) > 0, stats


def _problem(n, D, K, seed):
    rs = np.random.RandomState(seed)
    mu = rs.randn(K, D)
    lab = rs.randint(0, K, n)
    X = mu[lab] + 0.3 * rs.randn(n, D)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    means = mu + 0.05 * rs.randn(K, D)
    means /= np.linalg.norm(means, axis=1, keepdims=True)
    return X.astype(np.float32), means.astype(np.float32), rs


class _Scorer(object):
    """Direct hinted score calls on one component table; every call checked against the C oracle."""

    def __init__(self, X, means, K_max=None):
        import torch
        from segmentalist_amd.kmeans_components import KMeansComponents
        np.random.seed(0)
        self.X = X
        self.means = means.copy()
        self.c = KMeansComponents(X, np.zeros(X.shape[0], dtype=int), means.shape[0] if K_max is None else K_max)
        self.ident = torch.arange(self.c.dev.K_max, dtype=torch.int32, device="cuda")
        self.write(self.means)

    def write(self, means):
        import ctypes as C
        import torch
        from segmentalist_amd import _abi
        self.means = np.ascontiguousarray(means, dtype=np.float32)
        d = self.c.dev
        d.means[:self.means.shape[0]].copy_(torch.from_numpy(self.means).to(d.means.device))
        d.prepare()
        _abi.check(_abi.lib().segk_kmeans_mark_duplicates(d._ctx, d._cp(), C.byref(d.m), None, _abi.stream()))

    def score(self, remap=None, **kw):
        """-> (cand_k, cand_s, delta statistics) of one hinted call over all rows (or ids= / row0=, n=)."""
        import torch
        from oracle import c_oracle as co
        d = self.c.dev
        d.score_rows(hint_remap=self.ident if remap is None else remap, **kw)
        torch.cuda.synchronize()
        k, s = d.cand_k.cpu().numpy().copy(), d.cand_s.cpu().numpy().copy()
        if not kw:
            want_s, want_k = co.kmeans_max_argmax(self.means, self.X)
            assert np.array_equal(k, want_k)
            assert np.array_equal(s, want_s.astype(np.float64))
        return k, s, d.delta_stats()


def _run_steps(monkeypatch, make, steps):
    """The same sequence of (means edit, hinted call) in the three modes -> the delta mode's statistics per call; results equal."""
    res = {}
    for name, env in MODES:
        _setenv(monkeypatch, env)
        sc = make()
        out = [sc.score(), sc.score()]
        for step in steps:
            step(sc)
            out.append(sc.score())
        res[name] = out
    for name in ("full", "nohint"):
        for i, (a, b) in enumerate(zip(res["delta"], res[name])):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, i)
    return [o[2] for o in res["delta"]]


def test_forced_column_changes_between_calls(gpu, monkeypatch):
    """A settled table (two calls: full, then delta with nothing changed), then edits of the means between calls."""
    n, D, K = 3000, 20, 70
    X, means0, rs = _problem(n, D, K, 11)
    lab = np.argmax(X @ means0.T - 0.5 * (means0 ** 2).sum(1), axis=1)
    big = np.bincount(lab, minlength=K).argsort()[::-1]
    h_far, h_near, k_other = int(big[0]), int(big[1]), int(big[2])

    def edit(fn):
        def step(sc):
            m = sc.means.copy()
            fn(m)
            sc.write(m)
        return step

    def move_cols(cnt):
        def fn(m):
            m[:cnt] = m[:cnt] * np.float32(1.01)
        return fn

    def far(m):
        m[h_far] = -m[h_far]                          # the hinted component leaves its rows by much more than tau

    def near(m):
        m[h_near] = X[lab == h_near].mean(0)          # ... moves towards them

    def onto(m):
        m[k_other] = X[lab == h_far].mean(0)          # another component lands on a cluster and becomes its argmax

    def tiny(m):
        m[5, 0] = np.nextafter(m[5, 0], np.float32(2.0))    # far below the resolution of the image K1 multiplies: mean bits only

    def dup(m):
        m[40] = m[3]                                  # an exact duplicate of a lower row: absent in the images

    def undup(m):
        m[40] = means0[40]

    def scale(m):
        m *= np.float32(4.0)                          # the image exponent changes

    steps = [edit(move_cols(1)), edit(move_cols(32)), edit(move_cols(33)), edit(far), edit(near), edit(onto), edit(tiny),
             edit(dup), edit(undup), edit(scale)]
    stats = _run_steps(monkeypatch, lambda: _Scorer(X, means0), steps)
    print("delta stats per call:", stats)
    assert stats[0][0] == 0 and stats[1][:3] == (1, 0, 0), stats            # base pass, then nothing to multiply
    assert stats[1][3] > 0, stats                                            # ... and the hint waves skipped rows
    assert stats[2][:3] == (1, 1, 1), stats                                  # exactly one column
    assert stats[3][0] == 1 and stats[3][1] == 32 and stats[3][2] == 1, stats
    # 33 columns are two packed tiles: with the two tiles multiplied since the base that is more than the table's three -> the
    # next base
    assert stats[4][0] == 0 and stats[4][1] == 33, stats
    for i in (5, 6, 7):
        assert stats[i][0] == 1 and stats[i][1] == i - 4 and stats[i][2] == 1, (i, stats)
    # the tiny change left the image's bits alone; by now the delta passes since the base have multiplied a whole table's
    # tiles, so this call is the next base
    assert stats[8][0] == 0 and stats[8][1] == stats[7][1], stats
    # column 40 turns absent: one changed column; distinct again it is what the base pass multiplied: none
    assert stats[9][:3] == (1, 1, 1) and stats[10][:3] == (1, 0, 0), stats
    assert stats[11][0] == 0, stats                                          # exponent change -> every column -> full


def test_two_lds_ranges(gpu, monkeypatch):
    n, D, K = 6000, 20, 1100
    X, means0, rs = _problem(n, D, K, 12)

    def some(cnt, f):
        def step(sc):
            m = sc.means.copy()
            idx = np.arange(0, K, K // cnt)[:cnt]
            m[idx] = m[idx] * np.float32(f)
            sc.write(m)
        return step

    stats = _run_steps(monkeypatch, lambda: _Scorer(X, means0), [some(3, 1.01), some(40, 0.99), some(3, 1.5)])
    print("delta stats per call:", stats)
    assert stats[1][:3] == (1, 0, 0) and stats[2][0] == 1 and stats[2][2] == 1 and stats[3][0] == 1 and stats[3][2] >= 2, stats


def test_state_hygiene_between_calls(gpu, monkeypatch):
    """Calls that must drop or bypass the state: a relabelling that is not the identity, an id list, a sub-range, an un-hinted
    call, and a second table scored on the same context in between."""
    import torch
    n, D, K = 3000, 20, 70
    X, means0, rs = _problem(n, D, K, 13)
    X2, means2, _ = _problem(n, D, K, 14)
    for name, env in MODES[:2]:
        _setenv(monkeypatch, env)
        a, b = _Scorer(X, means0), _Scorer(X2, means2)
        want_a, want_b = a.score()[:2], b.score()[:2]
        for i in range(3):                                   # two tables alternating on one context
            ka, sa, st = a.score()
            kb, sb, _ = b.score()
            assert np.array_equal(ka, want_a[0]) and np.array_equal(kb, want_b[0])
            if name == "delta":
                assert st[0] == 0, st                        # the other table's call took the state
        st = [a.score()[2] for _ in range(2)]
        if name == "delta":
            assert st[1][0] == 1, st
        # a relabelling: labels 0 and 1 swapped
        perm = np.arange(K)
        perm[[0, 1]] = perm[[1, 0]]
        a.write(means0[perm])                                # new row j = old row perm[j]: old label k is now perm[k]
        k, s, st = a.score(remap=torch.from_numpy(perm.astype(np.int32)).cuda())
        if name == "delta":
            assert st[0] == 0, st
        assert a.score()[2][0] == (1 if name == "delta" else -1)
        # an id list and a sub-range in between, then an un-hinted call
        ids = torch.arange(100, 900, dtype=torch.int32, device="cuda")
        a.score(ids=ids)
        st1 = a.score()[2]
        a.score(row0=64, n=1000)
        st2 = a.score()[2]
        a.c.dev.score_rows()
        st3 = a.score()[2]
        st4 = a.score()[2]
        if name == "delta":
            assert st1[0] == 0 and st2[0] == 0 and st3[0] == 0 and st4[0] == 1, (st1, st2, st3, st4)


def test_minibatch_sweeps(gpu, monkeypatch):
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(400, 20, 70, seed=1, N=12, n_slices_max=6)
    _same_chains(gpu, monkeypatch, corpus, 70, 6, n_batches=4)


def test_headline_instantiation_small_corpus(gpu, monkeypatch):
    """D = 100, K = 1 000 (the headline's template instantiation, two LDS ranges of 16 tiles), 600 utterances, 12 sweeps."""
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(600, 100, 1000, seed=0, N=20, n_slices_max=6)
    stats = _same_chains(gpu, monkeypatch, corpus, 1000, 12)
    print("delta stats per sweep:", stats)

"""
The delta score pass's single K1 launch (segk_score_hint.hip): one launch that takes the full or the delta parameter set from the
mode word, and the hint waves' chunked skip.  As in test_gpu_kmeans_delta.py every call is compared bit for bit with the same
sequence under SEGK_SCORE_DELTA=0 and SEGK_SCORE_HINT=0, direct calls with the C oracle as well, and segk_kmeans_delta_stats is
asserted (mode, packed tiles, skipped positions) so that a case that never took the intended path cannot pass.
"""
import numpy as np
import pytest

from tests.test_gpu_kmeans_delta import MODES, _problem, _same_chains, _Scorer, _setenv, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

class _RangeScorer(_Scorer):
    """_Scorer whose calls cover row0 .. row0 + n; the C oracle checks that range in every call."""

    def __init__(self, X, means, row0=0, n=None):
        self.row0, self.n = row0, X.shape[0] - row0 if n is None else n
        _Scorer.__init__(self, X, means)

    def score(self, remap=None):
        import torch
        from oracle import c_oracle as co
        d = self.c.dev
        d.score_rows(hint_remap=self.ident if remap is None else remap, row0=self.row0, n=self.n)
        torch.cuda.synchronize()
        sl = slice(self.row0, self.row0 + self.n)
        k, s = d.cand_k.cpu().numpy()[sl].copy(), d.cand_s.cpu().numpy()[sl].copy()
        want_s, want_k = co.kmeans_max_argmax(self.means, self.X[sl])
        assert np.array_equal(k, want_k)
        assert np.array_equal(s, want_s.astype(np.float64))
        return k, s, d.delta_stats()


def _run(monkeypatch, make, steps, env=None, settle=2):
    """`settle` calls, then (edit, call) per step, in the three modes -> the delta mode's statistics per call; results equal."""
    res = {}
    for name, e in MODES:
        _setenv(monkeypatch, e)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        sc = make()
        out = [sc.score() for _ in range(settle)]
        for step in steps:
            step(sc)
            out.append(sc.score())
        res[name] = out
    for name in ("full", "nohint"):
        for i, (a, b) in enumerate(zip(res["delta"], res[name])):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, i)
    return [o[2] for o in res["delta"]]


def _edit(fn):
    def step(sc):
        m = sc.means.copy()
        fn(m)
        sc.write(m)
    return step


def _move(cnt, f=1.01):
    return _edit(lambda m: m.__setitem__(slice(0, cnt), m[:cnt] * np.float32(f)))


def _tiles_after_base(monkeypatch, make, t, env=None):
    """A settled pair of calls (full, delta without tiles), then the first 32 (t - 1) + 1 means move: a delta launch of t tiles."""
    cols = 32 * (t - 1) + 1
    stats = _run(monkeypatch, make, [_move(cols)], env=env)
    print("%d tiles; delta stats per call:" % t, stats)
    assert stats[0][0] == 0 and stats[1][:3] == (1, 0, 0) and stats[1][3] > 0, stats
    assert stats[2][:3] == (1, cols, t), stats


def test_tile_counts(gpu, monkeypatch):
    """22 801 rows (no multiple of 32), D = 20, K = 70: three tiles, the last partly filled; delta launches of 0, 1, 2 and 3
    packed tiles, each right after a base."""
    n, D, K = 22801, 20, 70
    X, means0, _ = _problem(n, D, K, 21)
    for t in (1, 2, 3):
        _tiles_after_base(monkeypatch, lambda: _Scorer(X, means0), t)


def test_more_tiles_than_a_small_table(gpu, monkeypatch):
    """K = 230 (eight tiles): delta launches of 1, 4 and 5 packed tiles."""
    n, D, K = 3001, 20, 230
    X, means0, _ = _problem(n, D, K, 22)
    for t in (1, 4, 5):
        _tiles_after_base(monkeypatch, lambda: _Scorer(X, means0), t)


@pytest.mark.parametrize("row0,n", [(0, 50), (12345, 22801 - 12345)])
def test_row_ranges(gpu, monkeypatch, row0, n):
    """A call of fewer than 64 rows; a sub-range with row0 > 0 whose length is no multiple of 64 and whose last row is the
    corpus's last row."""
    N, D, K = 22801, 20, 70
    X, means0, _ = _problem(N, D, K, 23)
    assert n % 64 != 0 and row0 + n <= N
    stats = _run(monkeypatch, lambda: _RangeScorer(X, means0, row0, n), [_move(1), _move(33)])
    print("delta stats per call:", stats)
    assert stats[1][:3] == (1, 0, 0) and 0 < stats[1][3] <= n, stats
    assert stats[2][0] == 1 and stats[2][2] == 1 and stats[3][0] == 1 and stats[3][2] == 2, stats
    assert 0 < stats[2][3] <= n and 0 < stats[3][3] < n, stats           # the moved means' rows lose the skip, others keep it


@pytest.mark.parametrize("D", [8, 20, 64, 100, 128])
def test_operand_widths(gpu, monkeypatch, D):
    """KS = 1, 2 (V != 0), 4, 7, 8: one and two packed tiles, rows no multiple of 32."""
    n, K = 2801, 70
    X, means0, _ = _problem(n, D, K, 24 + D)
    stats = _run(monkeypatch, lambda: _Scorer(X, means0), [_move(1), _move(33)])
    print("delta stats per call:", stats)
    assert stats[1][:3] == (1, 0, 0) and 0 < stats[1][3] <= n, stats
    assert stats[2][0] == 1 and stats[2][2] == 1 and stats[3][0] == 1 and stats[3][2] == 2, stats
    assert 0 < stats[2][3] < n and 0 < stats[3][3] < n, stats


def test_headline_instantiation_chain(gpu, monkeypatch):
    """D = 100, K = 1 000 (two LDS ranges in full mode, one in delta mode), 600 utterances, 12 sweeps; one mean is nudged before
    the last sweeps so that delta sweeps of few packed tiles follow those of many."""
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(600, 100, 1000, seed=0, N=20, n_slices_max=6)

    def between(seg, it):
        if it >= 9:
            dk = seg._dk
            dk.means[it] *= 1.0 + 1e-3
            dk.prepare()

    stats = _same_chains(gpu, monkeypatch, corpus, 1000, 12, between=between)
    print("delta stats per sweep:", stats)
    assert any(s[0] == 1 and s[2] >= 1 for s in stats), stats
    assert any(s[0] == 0 for s in stats[2:]), stats


def test_chunked_hint_skip(gpu, monkeypatch):
    """Enough rows for whole chunks of eight steps per hint wave and a partial last one.  After three calls every position is
    skipped; then cand_k of a handful of rows is overwritten with wrong but valid labels and with garbage -- in the first and the
    last position of a chunk and in the last, partial chunk -- and one mean moves, so that its rows lose the skip too."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n, D, K = 8 * 4 * n_cu * 32 + 9 * 4 * 32 * 7 + 17, 8, 70
    X, means0, _ = _problem(n, D, K, 29)
    n_w = 4 * min(n_cu, -(-n // 256))                       # hint waves of the delta launch; wave w: steps w, w + n_w, ...
    n_steps = -(-n // 32)
    assert n_steps > 8 * n_w and n_steps < 16 * n_w         # every wave: one whole chunk, then a partial one
    first = [32 * w for w in (0, 5)]                                        # step 0 of a chunk, its first row
    last = [32 * (w + 7 * n_w) + 31 for w in (1, n_w - 1)]                  # step 7 of a chunk, its last row
    part = [32 * (w + 8 * n_w) + r for w, r in ((0, 0), (3, 31), (6, 7))]   # the second, partial chunk
    rows = np.array(first + last + part + [n - 1])
    assert rows.max() < n and len(set(rows.tolist())) == len(rows)
    moved = {}

    def spoil(sc):
        d = sc.c.dev
        lab = d.cand_k.cpu().numpy().copy()
        new = lab[rows].copy()
        new[0::3] = (new[0::3] + 1) % K                     # wrong but valid
        new[1::3] = -7                                      # garbage
        new[2::3] = d.K_max + 12345
        d.cand_k[torch.from_numpy(rows).to(d.cand_k.device).long()] = torch.from_numpy(new).to(d.cand_k.device)
        lab[rows] = new
        k_mv = int(np.bincount(lab[(lab >= 0) & (lab < K)], minlength=K).argmax())
        moved["touched"] = int(np.count_nonzero(lab == k_mv) + np.count_nonzero(lab[rows] != k_mv))
        m = sc.means.copy()
        m[k_mv] = m[k_mv] * np.float32(1.0 + 1e-2)
        sc.write(m)

    stats = _run(monkeypatch, lambda: _Scorer(X, means0), [spoil], settle=3)
    print("delta stats per call:", stats, "rows touched:", moved)
    assert stats[2][:3] == (1, 0, 0) and stats[2][3] == n, stats
    assert stats[3][0] == 1 and stats[3][2] == 1, stats
    assert stats[3][3] == n - moved["touched"], (stats, moved)


def test_full_mode_before_and_after(gpu, monkeypatch):
    """The single launch takes the full parameter set whenever the mode word says so: state dropped by another table's call on
    the context, a relabelling that is not the identity; delta launches in between."""
    import torch
    n, D, K = 3000, 20, 70
    X, means0, _ = _problem(n, D, K, 30)
    X2, means2, _ = _problem(n, D, K, 31)
    for name, env in MODES[:2]:
        _setenv(monkeypatch, env)
        a, b = _Scorer(X, means0), _Scorer(X2, means2)
        a.score(); b.score()
        st = [a.score()[2], b.score()[2]]                    # each took the other's state: full
        if name == "delta":
            assert st[0][0] == 0 and st[1][0] == 0, st
        a.score()
        _move(1)(a)
        st = a.score()[2]
        if name == "delta":
            assert st[0] == 1 and st[2] == 1, st             # a delta launch
        perm = np.arange(K)
        perm[[0, 1]] = perm[[1, 0]]
        a.write(a.means[perm])
        st = a.score(remap=torch.from_numpy(perm.astype(np.int32)).cuda())[2]
        if name == "delta":
            assert st[0] == 0, st                            # not the identity: full
        _move(33)(a)
        st = a.score()[2]
        if name == "delta":
            assert st[0] == 1 and st[2] == 2, st

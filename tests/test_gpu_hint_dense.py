"""
The hint waves' dense bodies in a delta score pass (hint_wave_rows, segk_score_hint.hip): the positions of a chunk that lose the
skip go onto a pending list, and a body runs over 32 list entries whenever 32 are pending and once more at the end of the wave's
steps.  As in test_gpu_kmeans_delta_stream.py every call is compared bit for bit with the same sequence under SEGK_SCORE_DELTA=0
and SEGK_SCORE_HINT=0 and with the C oracle, and the skipped positions of segk_kmeans_delta_stats must be the rows minus the live
positions, which the tests choose exactly: after three settling calls (every position skipped) cand_k of chosen rows is
overwritten with a wrong but valid label, or a mean moves.

Shape of the large cases, as in test_chunked_hint_skip: wave w of the n_w hint waves owns the steps w, w + n_w, ... of 32 rows;
every wave has one whole chunk of eight steps, the first 253 a second chunk of one step, and the last step has 17 rows.
"""
import numpy as np
import pytest

from tests.test_gpu_kmeans_delta import MODES, _problem, _Scorer, gpu  # noqa: F401
from tests.test_gpu_kmeans_delta_stream import _RangeScorer, _run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big(gpu):
    n_cu = gpu.cuda.get_device_properties(0).multi_processor_count
    n, D, K = 8 * 4 * n_cu * 32 + 9 * 4 * 32 * 7 + 17, 8, 70
    X, means0, _ = _problem(n, D, K, 29)
    n_w = 4 * min(n_cu, -(-n // 256))                       # hint waves of the delta launch
    n_steps = -(-n // 32)
    assert 8 * n_w < n_steps < 9 * n_w and n % 32 == 17
    return {"n": n, "K": K, "X": X, "means": means0, "n_w": n_w, "n_steps": n_steps}


def _pos(big, w, i, r):
    """Position r of step i (0 .. 7: the first chunk, 8: the second) of wave w."""
    s = w + i * big["n_w"]
    assert s < big["n_steps"] and 32 * s + r < big["n"]
    return 32 * s + r


def _spoil(pos, row0=0, garbage=()):
    """cand_k at the positions `pos` of a call that starts at row0 := a wrong but valid label; at `garbage`: -7 and K_max + 12345."""
    def step(sc):
        import torch
        d = sc.c.dev
        K = sc.means.shape[0]
        for p, kind in ((pos, 0), (garbage, 1)):
            if len(p) == 0:
                continue
            idx = torch.from_numpy(np.asarray(p, dtype=np.int64) + row0).to(d.cand_k.device)
            lab = d.cand_k[idx].cpu().numpy()
            assert ((lab >= 0) & (lab < K)).all()
            new = (lab + 1) % K
            if kind:
                new[0::2] = -7
                new[1::2] = d.K_max + 12345
            d.cand_k[idx] = torch.from_numpy(new.astype(lab.dtype)).to(d.cand_k.device)
    return step


def _live_case(monkeypatch, make, n, steps, live, tiles=(0,)):
    """Three settling calls, then `steps`; the last call: a delta launch with n - live positions skipped."""
    stats = _run(monkeypatch, make, steps, settle=3)
    print("delta stats per call:", stats, "live:", live)
    assert stats[2][:3] == (1, 0, 0) and stats[2][3] == n, stats
    assert stats[-1][0] == 1 and stats[-1][2] in tiles, stats
    assert stats[-1][3] == n - live, (stats, live)
    return stats


def _chunk0(big, w, cnt, seed):
    """cnt positions of wave w's first chunk, spread over its eight steps (fixed seed)."""
    rs = np.random.RandomState(seed)
    c = np.sort(rs.permutation(256)[:cnt])
    return [_pos(big, w, int(v) // 32, int(v) % 32) for v in c]


def test_no_live_position(big, monkeypatch):
    _live_case(monkeypatch, lambda: _Scorer(big["X"], big["means"]), big["n"], [lambda sc: None], 0)


@pytest.mark.parametrize("cnt", [31, 32, 33])
def test_one_chunk(big, monkeypatch, cnt):
    """31, 32, 33 live positions in one wave's first chunk: one partly filled body; one full body; a full body and one entry."""
    pos = _chunk0(big, 5, cnt, 100 + cnt)
    assert len(set(pos)) == cnt
    _live_case(monkeypatch, lambda: _Scorer(big["X"], big["means"]), big["n"], [_spoil(pos)], cnt)


def test_entries_carried_over_the_chunk_boundary(big, monkeypatch):
    """20 live positions in a wave's first chunk and 20 in its second, partial one: a body of 32 and a body of 8."""
    w = 3
    pos = _chunk0(big, w, 20, 7) + [_pos(big, w, 8, r) for r in range(3, 23)]
    assert len(set(pos)) == 40
    _live_case(monkeypatch, lambda: _Scorer(big["X"], big["means"]), big["n"], [_spoil(pos)], 40)


def test_whole_step_and_one_more(big, monkeypatch):
    """All 32 positions of one step and one position of another step of the same chunk."""
    w = big["n_w"] - 1
    pos = [_pos(big, w, 2, r) for r in range(32)] + [_pos(big, w, 5, 7)]
    _live_case(monkeypatch, lambda: _Scorer(big["X"], big["means"]), big["n"], [_spoil(pos)], 33)


def test_last_chunk_only(big, monkeypatch):
    """Live positions only in second, partial chunks, among them the call's last position (in the step of 17 rows)."""
    n, w_last = big["n"], big["n_steps"] - 1 - 8 * big["n_w"]
    assert w_last == 252
    pos = [n - 1, n - 17, n - 9, _pos(big, 0, 8, 0), _pos(big, 0, 8, 31), _pos(big, 100, 8, 13)]
    assert n - 17 == _pos(big, w_last, 8, 0) and len(set(pos)) == 6
    _live_case(monkeypatch, lambda: _Scorer(big["X"], big["means"]), n, [_spoil(pos)], 6)


def test_every_hint_wrong(big, monkeypatch):
    """Every position live with the means unchanged: as many dense bodies as there are steps, in a delta launch without tiles."""
    n = big["n"]
    _live_case(monkeypatch, lambda: _Scorer(big["X"], big["means"]), n, [_spoil(np.arange(n))], n)


def test_all_means_move(big, monkeypatch):
    """Every position live because every mean moved (every column changes with them: the launch takes the full parameter set,
    and the hint waves still go through the skip test of the previous call's entries)."""
    n = big["n"]

    def move(sc):
        sc.write(sc.means * np.float32(1.01))

    stats = _run(monkeypatch, lambda: _Scorer(big["X"], big["means"]), [move], settle=3)
    print("delta stats per call:", stats)
    assert stats[2][:3] == (1, 0, 0) and stats[2][3] == n, stats
    assert stats[3][1] == big["K"] and stats[3][3] == 0, stats


def test_garbage_and_absent_hints(big, monkeypatch):
    """Among the live entries: garbage hints (-7, K_max + 12345), wrong but valid ones, and hints the image marks absent (mean 40
    becomes an exact duplicate of mean 3: its rows' hints name an absent component)."""
    n, K = big["n"], big["K"]
    w = 9
    bad = _chunk0(big, w, 12, 1) + [_pos(big, w, 8, 4), _pos(big, w, 8, 5)]
    wrong = _chunk0(big, w + 1, 9, 2) + [n - 1]
    assert len(set(bad + wrong)) == len(bad) + len(wrong)
    seen = {}

    def plant(sc):
        _spoil(wrong, garbage=bad)(sc)
        lab = sc.c.dev.cand_k.cpu().numpy()
        seen["live"] = int(np.count_nonzero(lab == 40)) + int(np.count_nonzero(lab[np.array(bad + wrong)] != 40))
        seen["absent"] = int(np.count_nonzero(lab == 40))
        m = sc.means.copy()
        m[40] = m[3]
        sc.write(m)

    stats = _run(monkeypatch, lambda: _Scorer(big["X"], big["means"]), [plant], settle=3)
    print("delta stats per call:", stats, seen)
    assert seen["absent"] > 32 and seen["live"] > seen["absent"], seen
    assert stats[2][:3] == (1, 0, 0) and stats[2][3] == n, stats
    assert stats[3][:3] == (1, 1, 1), stats
    assert stats[3][3] == n - seen["live"], (stats, seen)


@pytest.mark.parametrize("D", [20, 100, 128])
def test_five_percent_live(gpu, monkeypatch, D):
    """About 5 % of the positions live at random: the body with a remainder block (D = 20, 100), the headline width, the widest."""
    n, K = 22801, 70
    X, means0, _ = _problem(n, D, K, 40 + D)
    pos = np.sort(np.random.RandomState(D).permutation(n)[:n // 20])
    _live_case(monkeypatch, lambda: _Scorer(X, means0), n, [_spoil(pos)], len(pos))


def test_sub_range(gpu, monkeypatch):
    """A call over row0 .. row0 + n with row0 > 0 and n no multiple of 64: a few live positions in its last step (24 rows)."""
    N, D, K = 22801, 20, 70
    row0, n = 12345, 22801 - 12345
    assert n % 64 != 0 and n % 32 == 24
    X, means0, _ = _problem(N, D, K, 23)
    pos = [n - 1, n - 24, n - 10, 0]
    _live_case(monkeypatch, lambda: _RangeScorer(X, means0, row0, n), n, [_spoil(pos, row0=row0)], len(pos))

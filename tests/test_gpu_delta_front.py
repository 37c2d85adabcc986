"""
The front of a hinted score call after a batch finalize: k_batch_post runs the delta prep of the call that follows (the tile image
and `means` against their snapshots, the mode word), and that call skips its k_delta_prep launch when the context's pending prep
is its own (segk_score_hint.hip launch_delta_prep, segk_stats.hip k_batch_post).  Nothing may change by it: not the results, not
what segk_kmeans_delta_stats reports.

Batch chains are compared bit for bit, after every sweep, with the same chain under SEGK_DELTA_PREP_FOLD=0 (every prep a launch
of its own), under SEGK_SCORE_DELTA=0 (every pass full) and with oracle/np_oracle.py kmeans_batch_sweep; direct score calls with
the C oracle and with SEGK_SCORE_DELTA=0 / SEGK_SCORE_HINT=0, and segk_kmeans_stage_counts says how many rows a call queued for
the band stage ([0]) and for the full scan ([1]).  segk_kmeans_delta_stats says which mode a call took, so that a chain that never
reached a delta call with skipped positions cannot pass.  There are no tolerances.
"""
import random

import numpy as np
import pytest

from tests.test_gpu_kmeans_carry import _CScorer, _call, _edit, _run, _twins  # noqa: F401
from tests.test_gpu_kmeans_delta import _snapshot, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

DELTA = {"SEGK_SCORE_HINT": "1"}
NOFOLD = {"SEGK_SCORE_HINT": "1", "SEGK_DELTA_PREP_FOLD": "0"}
FULL = {"SEGK_SCORE_HINT": "1", "SEGK_SCORE_DELTA": "0"}


def _setenv(monkeypatch, env):
    for k in ("SEGK_SCORE_HINT", "SEGK_SCORE_DELTA", "SEGK_DELTA_PREP_FOLD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _chain(torch, monkeypatch, corpus, K, sweeps, env, n_batches=1, between=None):
    """`sweeps` batch sweeps -> (state after every sweep, delta statistics after every sweep)."""
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    _setenv(monkeypatch, env)
    random.seed(0); np.random.seed(0)
    seg = kaw.SegmentalKMeansWordseg(K, *corpus, n_slices_max=5, init_am_assignments="spread", sync="batch", n_batches=n_batches)
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


def _oracle_chain(torch, monkeypatch, corpus, K, nsm, sweeps, env, between=None):
    """`sweeps` batch sweeps beside the numpy specification: boundaries, means, counts and K equal after every sweep, the
    assignments after the last -> (device state after every sweep, delta statistics after every sweep, K after every sweep)."""
    from oracle import np_oracle as no
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    _setenv(monkeypatch, env)
    random.seed(0); np.random.seed(0)
    ref = no.SegmentalKMeansWordseg(K, *corpus, n_slices_max=nsm, init_am_assignments="spread")
    random.seed(0); np.random.seed(0)
    seg = kaw.SegmentalKMeansWordseg(K, *corpus, n_slices_max=nsm, init_am_assignments="spread", sync="batch")
    cr, cd = ref.acoustic_model.components, seg.acoustic_model.components
    states, stats, ks = [], [], []
    for it in range(sweeps):
        if between is not None:
            between(seg, ref, it)
        random.seed(100 + it)
        no.kmeans_batch_sweep(ref, n_blocks=8)
        random.seed(100 + it)
        seg.batch_sweep_async()
        torch.cuda.synchronize()
        states.append(_snapshot(seg))
        stats.append(seg._dk.delta_stats())
        ks.append(int(cr.K))
        assert np.array_equal(seg.utterances.boundaries, ref.utterances.boundaries), it
        assert cd.K == cr.K, it
        assert np.array_equal(cd.counts, cr.counts), it
        assert np.array_equal(cd.means, cr.means), it
    assert np.array_equal(cd.assignments, cr.assignments)
    seg._dk.check_status()
    return states, stats, ks


def _equal_states(a, b, what):
    for it, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x, y)):
            assert np.array_equal(p, q, equal_nan=True), (what, it, i)


@pytest.mark.parametrize("n_utt,D,N,nsm", [(120, 16, 10, 5), (100, 100, 8, 4)])
def test_chain_of_14_sweeps(gpu, monkeypatch, n_utt, D, N, nsm):
    """K_max = 70 (three tiles, the last one part empty), D = 16 (one k-step) and D = 100 (the headline's <7, 3>): un-hinted
    sweeps, full and delta calls, delta calls without a packed tile.  Components empty during the first sweeps (K falls from
    one sweep to the next), so clean_components moves rows and the relabelling is not the identity: the call after such a
    sweep has no SKIP -- it skips no position."""
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(n_utt, D, 70, seed=0, N=N, n_slices_max=nsm)
    states, stats, ks = _oracle_chain(gpu, monkeypatch, corpus, 70, nsm, 14, DELTA)
    nofold = _oracle_chain(gpu, monkeypatch, corpus, 70, nsm, 14, NOFOLD)
    full = _oracle_chain(gpu, monkeypatch, corpus, 70, nsm, 14, FULL)
    _equal_states(states, nofold[0], "SEGK_DELTA_PREP_FOLD=0")
    _equal_states(states, full[0], "SEGK_SCORE_DELTA=0")
    assert stats[2:] == nofold[1][2:], (stats, nofold[1])        # (the first two sweeps are un-hinted: no figures of their own)
    print("K per sweep:", ks)
    print("delta stats per sweep (mode, changed columns, packed tiles, skipped positions):", stats)
    delta = [s for s in stats if s[0] == 1]
    assert len(delta) >= 3, stats
    assert any(s[2] == 0 for s in delta), stats
    assert sum(s[3] for s in delta) > 0, stats
    shrank = [it for it in range(1, 14) if ks[it] < ks[it - 1]]
    assert shrank, ks                                                        # a component emptied: rows of `means` moved
    for it in shrank:
        # the hinted call of sweep it + 1 sees the relabelling of sweep it: FULL, and without SKIP no position is skipped
        # (an un-hinted sweep leaves the figures of the sweep before)
        if it + 1 < 14 and stats[it + 1] != stats[it]:
            assert stats[it + 1][0] <= 0 and stats[it + 1][3] == 0, (it, stats)


def test_edits_between_sweeps(gpu, monkeypatch):
    """means[k] *= 1 + 1e-3, a change below the image's resolution (* (1 + 2**-20)), and mark_duplicates, each through the
    supported route (prepare()) in a settled chain and followed by three sweeps; the specification gets the same edit.  Each
    comes between a batch finalize and the hinted call: the pending prep has compared the table as it was BEFORE the edit and
    must have been dropped -- taken over, the hint waves would keep the edited component's scores of the previous sweep."""
    import ctypes as C
    from segmentalist_amd import _abi
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(120, 16, 70, seed=0, N=10, n_slices_max=5)

    def between(seg, ref, it):
        dk = seg._dk
        rm = ref.acoustic_model.components.means
        if it == 9:
            dk.means[3] *= 1.0 + 1e-3
            rm[3] *= np.float32(1.0 + 1e-3)
        elif it == 12:
            dk.means[5] *= 1.0 + 2.0 ** -20
            rm[5] *= np.float32(1.0 + 2.0 ** -20)
        if it in (9, 12):
            assert np.array_equal(dk.means.cpu().numpy(), rm)
            dk.prepare()
        if it == 15:
            _abi.check(_abi.lib().segk_kmeans_mark_duplicates(dk._ctx, dk._cp(), C.byref(dk.m), None, _abi.stream()))

    states, stats, _ = _oracle_chain(gpu, monkeypatch, corpus, 70, 5, 18, DELTA, between=between)
    nofold = _oracle_chain(gpu, monkeypatch, corpus, 70, 5, 18, NOFOLD, between=between)
    full = _oracle_chain(gpu, monkeypatch, corpus, 70, 5, 18, FULL, between=between)
    _equal_states(states, nofold[0], "SEGK_DELTA_PREP_FOLD=0")
    _equal_states(states, full[0], "SEGK_SCORE_DELTA=0")
    print("delta stats per sweep:", stats)
    assert stats[2:] == nofold[1][2:], (stats, nofold[1])        # (the first two sweeps are un-hinted: no figures of their own)
    assert sum(1 for s in stats if s[0] == 1 and s[3] > 0) >= 3, stats
    # the sweeps behind the two edits of `means` are delta calls (the state survives prepare()), and each has recomputed the
    # rows of the edited component: not every position skipped, as in the settled sweeps at the end
    n_rows = states[0][1].shape[0]
    for it in (9, 12):
        assert stats[it][0] == 1 and 0 < stats[it][3] < n_rows, (it, stats)
    assert stats[-1][3] == n_rows, stats


def test_two_models_on_one_context(gpu, monkeypatch):
    """Two segmenters sweeping alternately on the one context, and a third created in the middle of the chain: each equals
    its own chain run alone under SEGK_SCORE_DELTA=0.  Every hinted call follows the other model's batch finalize: neither
    may take the other's pending prep for its own."""
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    corpora = [make_corpus(80, 16, 36, seed=s, N=8, n_slices_max=4) for s in (1, 2, 3)]

    def make(i):
        random.seed(i); np.random.seed(i)
        return kaw.SegmentalKMeansWordseg(36, *corpora[i], n_slices_max=4, init_am_assignments="spread", sync="batch")

    def alone(i, sweeps):
        seg = make(i)
        out = []
        for _ in range(sweeps):
            seg.batch_sweep_async()
            gpu.cuda.synchronize()
            out.append(_snapshot(seg))
        return out

    _setenv(monkeypatch, FULL)
    want = [alone(0, 10), alone(1, 10), alone(2, 5)]
    _setenv(monkeypatch, DELTA)
    segs, got = [make(0), make(1)], [[], [], []]
    for it in range(10):
        if it == 5:
            segs.append(make(2))
        for i, seg in enumerate(segs):
            seg.batch_sweep_async()
            gpu.cuda.synchronize()
            got[i].append(_snapshot(seg))
    for i in range(3):
        _equal_states(got[i], want[i], "model %d" % i)
    for env in (DELTA, NOFOLD):
        _setenv(monkeypatch, env)
        _equal_states(alone(0, 10), want[0], "model 0 alone")


def test_minibatch_and_an_unhinted_sweep_in_between(gpu, monkeypatch):
    """n_batches = 2: sub-range calls, which have no delta state; and a chain in which one sweep runs un-hinted
    (SEGK_SCORE_HINT=0 for that sweep): the state it drops is rebuilt, the results are those of the chain without the delta pass."""
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(120, 16, 70, seed=1, N=10, n_slices_max=5)
    a = _chain(gpu, monkeypatch, corpus, 70, 6, DELTA, n_batches=2)
    for env in (NOFOLD, FULL):
        b = _chain(gpu, monkeypatch, corpus, 70, 6, env, n_batches=2)
        _equal_states(a[0], b[0], "n_batches=2 %r" % (env,))

    def between(seg, it):
        monkeypatch.setenv("SEGK_SCORE_HINT", "0" if it == 9 else "1")

    a = _chain(gpu, monkeypatch, corpus, 70, 14, DELTA, between=between)
    for env in (NOFOLD, FULL):
        b = _chain(gpu, monkeypatch, corpus, 70, 14, env, between=between)
        _equal_states(a[0], b[0], "un-hinted sweep 9 %r" % (env,))
        if env is NOFOLD:
            assert a[1][2:] == b[1][2:], (a[1], b[1])
    print("delta stats per sweep:", a[1])
    assert a[1][8][0] == 1 and a[1][10][0] == 0 and a[1][-1][0] == 1, a[1]


# ---- the merge behind a prep (its own launch here: direct calls): planted twin means, tests/test_gpu_kmeans_carry.py ------------

def _near_tie_rows(X, means, i, j, rows):
    """Of `rows`, those whose reference scores against i and j are closer (in the filter's domain: half the score) than
    tau - 2 E: the certificate cannot pass on them whichever of the two wins."""
    from tests.test_gpu_kmeans_carry import _tau_slack
    x = X[rows].astype(np.float64)
    s_i = -((x - means[i].astype(np.float64)) ** 2).sum(1)
    s_j = -((x - means[j].astype(np.float64)) ** 2).sum(1)
    return rows[0.5 * np.abs(s_i - s_j) < 0.9 * _tau_slack(X, means)[rows]]


@pytest.mark.parametrize("shape", ["three_tiles", "two_lds_ranges", "headline_instantiation"])
def test_settled_call_carries_and_a_changed_twin_takes_its_rows(gpu, monkeypatch, shape):
    """The settled delta calls with nothing changed queue nothing but rows without a recorded label -- those the full scan
    decided in the call before; with one distant mean changed (a packed tile) the twin rows are still carried.  Then one
    twin's mean moves (still 1e-4 from its original): that pair's rows go to the band stage, every other twin row is still
    carried.  Bounds of that call's queue: at least the pair's rows that the certificate cannot pass (a near-tie, from the
    margin's own formula) and the carry-over cannot decide either -- the moved twin was or becomes their winner --, at most
    the pair's rows beside what the call before could not decide."""
    t = _twins(shape)
    i, j = t.big[0], t.small[0]
    k_far = t.free[-1]
    signs = t.rs.choice([-1.0, 1.0], t.means.shape[1]).astype(np.float32)

    def far(m):
        m[k_far] = m[k_far] * np.float32(1.01)

    def twin(m):
        m[j] = m[i] * (np.float32(1.0) + np.float32(1e-4) * signs)

    out = _run(monkeypatch, lambda: _CScorer(t.X, t.means), [lambda sc: None, _edit(far), _edit(twin), lambda sc: None])
    cnt = [o[3] for o in out]
    st = [o[2] for o in out]
    print("stage counts per call:", cnt, "delta stats:", st, "twin rows:", t.rows.size)
    assert cnt[0][0] >= t.rows.size > 0, cnt
    assert st[1][:3] == (1, 0, 0) and st[2][:3] == (1, 0, 0) and st[3][:3] == (1, 1, 1) and st[4][:3] == (1, 2, 1), st
    for c in (1, 2):
        assert cnt[c][0] <= cnt[c - 1][1], (c, cnt)
    assert cnt[3][0] <= t.rows.size // 8, (cnt, t.rows.size)
    m4 = t.means.copy()
    far(m4)
    twin(m4)
    pair_rows = np.flatnonzero(t.lab == i)
    must = _near_tie_rows(t.X, m4, i, j, pair_rows)
    must = must[(out[3][0][must] == j) | (out[4][0][must] == j)]
    assert must.size > 0, pair_rows.size
    assert must.size <= cnt[4][0] <= pair_rows.size + cnt[3][0] + cnt[3][1], (cnt, must.size, pair_rows.size)
    assert st[5][0] == 1, st
    # (the moved twin's column stays in the packed image: its pair's rows keep failing condition 5 while it is there)
    assert cnt[5][0] <= cnt[4][0] + cnt[4][1], cnt


def test_hint_is_the_base_certified_label_of_a_changed_column(gpu, monkeypatch):
    """The largest cluster without a twin moves a little: its rows' hint is the label the base pass certified and that column
    has changed -- the stale base value is dropped (the lab_base repair) and the certificate
    passes on the fresh one.  Without the repair every row of the cluster that the base pass certified would be queued: the
    stale and the fresh value of its own column lie far inside tau of each other."""
    t = _twins("three_tiles")
    h = t.free[0]
    n_h = int((t.lab == h).sum())
    assert n_h >= 30

    def move(m):
        m[h] = m[h] * np.float32(1.0 + 1e-3)

    out = _run(monkeypatch, lambda: _CScorer(t.X, t.means), [lambda sc: None, _edit(move), lambda sc: None])
    cnt = [o[3] for o in out]
    st = [o[2] for o in out]
    print("stage counts per call:", cnt, "delta stats:", st, "rows of the moved cluster:", n_h)
    assert st[3][:3] == (1, 1, 1), st
    assert (out[3][0] == h).sum() >= n_h // 2
    assert cnt[0][0] + cnt[0][1] <= t.rows.size + n_h // 4, (cnt, t.rows.size, n_h)     # the base certified most of the cluster
    assert cnt[3][0] <= cnt[2][1] + n_h // 2, (cnt, n_h)
    assert cnt[4][0] <= cnt[3][1] + n_h // 2, cnt


def test_sub_resolution_change_switches_the_carry_over_off(gpu, monkeypatch):
    """A distant mean moves by one ulp in one coordinate: no image column changes, nothing is packed, and condition 4 must
    switch the carry-over off for that call -- every twin row takes the normal route again -- and only for that call."""
    t = _twins("three_tiles")
    k_far = t.free[-1]

    def ulp(m):
        m[k_far, 2] = np.nextafter(m[k_far, 2], np.float32(9.0))

    out = _run(monkeypatch, lambda: _CScorer(t.X, t.means), [lambda sc: None, _edit(ulp), lambda sc: None])
    cnt = [o[3] for o in out]
    st = [o[2] for o in out]
    print("stage counts per call:", cnt, "delta stats:", st)
    assert cnt[2][0] <= cnt[1][1], cnt
    assert st[3][:3] == (1, 0, 0), st
    assert cnt[3][0] >= t.rows.size, (cnt, t.rows.size)
    assert cnt[4][0] <= cnt[3][1], cnt


def test_foreign_hints_cost_only_time(gpu, monkeypatch):
    """cand_k overwritten with garbage between two settled calls: exact results (the C oracle, in _CScorer), and the call after
    carries again."""
    import torch
    t = _twins("three_tiles")
    n = t.X.shape[0]
    K = t.means.shape[0]
    rs = np.random.RandomState(5)
    junk = rs.choice(np.array([-1, -9, K, K + 3, 2 ** 30, 2 ** 30 | 5, 2 ** 31 - 1] + list(range(K)), dtype=np.int64), n)

    def garbage(sc):
        d = sc.c.dev
        torch.cuda.synchronize()
        d.cand_k.copy_(torch.from_numpy(junk.astype(np.int32)).to(d.cand_k.device))

    out = _run(monkeypatch, lambda: _CScorer(t.X, t.means), [garbage, lambda sc: None, lambda sc: None])
    cnt = [o[3] for o in out]
    print("stage counts per call:", cnt)
    assert cnt[3][0] <= cnt[2][1] and cnt[4][0] <= cnt[3][1], cnt

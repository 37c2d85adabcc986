"""GPU parity of the batch sweep with fb_type="viterbi" (segk_fbb_segment_map, segk_fbb_assign_map) against its executable
specification tests/map_batch.py.  tests/test_map_batch_cpu.py is the precondition of the exact tests here: on every case,
over the sweeps run here, every argmax is decided by at least 1e-6 relative (ties among empty slots aside, where the first
wins on both sides), so boundaries and slots must coincide; log-probabilities to 1e-9 relative.

In the tolerance modes (score_precision "f32" / "f16") the chain may leave the specification's, so every step is checked
against the device's own numbers: the boundaries must be optimal for the span scores the step used, the slots for the token
likelihoods it used -- a failure cannot hide behind a near-tie in this form, and no margin precondition is needed."""
import random

import numpy as np
import numpy.testing as npt
import pytest

from oracle import np_oracle as no
from tests import fbgmm_long
from tests import map_batch as mb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _sweep_matches(gpu, ref, spec, seg, sw, viterbi=True):
    """One sweep of the product (its own fb_type) against the specification's sweep `sw` from identical states: boundaries
    and slots equal, log-probabilities to 1e-9 relative, the reference's view (canonical assignments, counts) equal."""
    lp = spec.sweep(sw, viterbi=viterbi)
    seg.batch_sweep_async()
    gpu.cuda.synchronize()
    seg._df.check_status()
    assert seg._get_sweeper().sweep_index == sw + 1
    assert np.array_equal(seg.utterances.boundaries, ref.utterances.boundaries), sw
    assert np.array_equal(seg._get_sweeper().slot.cpu().numpy(), spec.slot), sw
    npt.assert_allclose(seg._df.out_logprob.cpu().numpy(), lp, rtol=1e-9)
    seg.materialise()
    a, Kc = spec.canonical()
    c = seg.acoustic_model.components
    assert c.K == Kc
    assert np.array_equal(c.assignments, a)
    cnt = spec.stats_excluding(-1)[0]
    assert np.array_equal(c.counts[:Kc], cnt[cnt > 0])


@pytest.mark.parametrize("name", mb.EXACT)
def test_viterbi_sweeps_match_specification(gpu, name):
    ref, spec, seg = mb.pair(name)
    seg.set_fb_type("viterbi")
    for sw in range(mb.n_sweeps(name)):
        _sweep_matches(gpu, ref, spec, seg, sw)


@pytest.mark.parametrize("name", mb.MIXED)
def test_sampled_sweeps_then_viterbi_sweeps_on_a_live_sweeper(gpu, name):
    """The use pattern: sample, then set_fb_type("viterbi") and sweep on; sweep_index goes on counting."""
    ref, spec, seg = mb.pair(name)
    for sw in range(2):
        _sweep_matches(gpu, ref, spec, seg, sw, viterbi=False)
    sweeper = seg._get_sweeper()
    seg.set_fb_type("viterbi")
    for sw in range(2, 4):
        _sweep_matches(gpu, ref, spec, seg, sw)
    assert seg._get_sweeper() is sweeper


def test_gibbs_sample_in_viterbi_mode_returns_the_record(gpu):
    ref, spec, seg = mb.pair("fixed_small")
    seg.set_fb_type("viterbi")
    state = random.getstate()
    rec = seg.gibbs_sample(2)
    assert random.getstate() == state          # no uniform of Python's `random` consumed
    assert sorted(rec) == sorted(["sample_time", "log_marg", "log_marg*length", "log_prob_z", "log_prob_X_given_z", "anneal_temp",
                                  "components", "n_tokens"])
    for sw in range(2):
        lp = spec.sweep(sw)
        npt.assert_allclose(rec["log_marg*length"][sw], np.sum(lp), rtol=1e-9)
        assert rec["components"][sw] == spec.canonical()[1]
        assert rec["n_tokens"][sw] == int(np.count_nonzero(spec.slot >= 0))
    assert np.array_equal(seg.utterances.boundaries, ref.utterances.boundaries)


def test_refusal_with_a_language_model(gpu):
    from segmentalist_amd._abi import SegkError
    seg = fbgmm_long.product_of("short_bigram")
    with pytest.raises(SegkError, match="language model"):
        seg._get_sweeper().sweep(seg._dev_bounds, seg.n_slices_min, seg.n_slices_max, seg.wip, seg.time_power_term, viterbi=True)


def test_viterbi_sweeps_on_two_ranks_equal_the_specification(gpu):
    """`ragged_fixed` (S = 4) on two virtual ranks (tests/virtual_ranks.py): the specification's bits on every rank."""
    from tests.virtual_ranks import VirtualWorld
    name = "ragged_fixed"
    ref, spec, _ = mb.pair(name, product=False)
    want = []
    for sw in range(2):
        lp = spec.sweep(sw)
        want.append((ref.utterances.boundaries.copy(), lp))
    corpus = fbgmm_long.corpus_of(mb.LONG_CASES[name])

    def run(comm):
        seg = fbgmm_long.product_of(mb.LONG_CASES[name], corpus=corpus, process_group=comm)
        seg.set_fb_type("viterbi")
        states = []
        for sw in range(len(want)):
            seg.batch_sweep_async()
            gpu.cuda.synchronize()
            seg._df.check_status()
            lp = seg._get_sweeper().utt_values(seg._df.out_logprob)
            seg.materialise()
            states.append((seg.utterances.boundaries.copy(), lp))
        c = seg.acoustic_model.components
        return states, c.assignments.copy(), c.K, c.counts.copy()

    for states, assignments, K, counts in VirtualWorld(2).run(run):
        for (bnd, lp), (wb, wlp) in zip(states, want):
            assert np.array_equal(bnd, wb)
            npt.assert_allclose(lp, wlp, rtol=1e-9)
        a, Kc = spec.canonical()
        assert K == Kc and np.array_equal(assignments, a)
        cnt = spec.stats_excluding(-1)[0]
        assert np.array_equal(counts[:Kc], cnt[cnt > 0])


def test_sampled_sweeps_still_take_the_fused_step(gpu):
    ref, spec, seg = mb.pair("diag_K65", prec="f32")
    seg.batch_sweep_async()
    gpu.cuda.synchronize()
    seg._df.check_status()
    sweeper = seg._get_sweeper()
    assert sweeper._fused is True
    seg.set_fb_type("viterbi")
    seg.batch_sweep_async()
    gpu.cuda.synchronize()
    seg._df.check_status()
    assert sweeper._fused is True
    seg.set_fb_type("standard")
    seg.batch_sweep_async()
    gpu.cuda.synchronize()
    seg._df.check_status()
    assert sweeper._fused is True and sweeper.sweep_index == 3


# ------------------------------------------------------------------ tolerance modes
def _one_map_step(sw, seg, b):
    """Step b of a Viterbi sweep as FbgmmBatchSweeper.sweep enqueues it (score, segment_map, assign_map), without the
    partial-sum refresh, the way tests/test_gpu_tolerance_modes.py::_one_step drives a sampled step."""
    import torch
    from segmentalist_amd._abi import check, ptr
    df = seg._df
    L, ctx, cp, fp, bp, st = sw._args()
    check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
    if sw.score_f32:
        check(L.segk_fbb_score_f32(ctx, cp, fp, bp, ptr(sw._block_rows[b]), sw._block_rows[b].numel(), ptr(df.score), st))
    elif sw.score_diag32:
        check(L.segk_fbb_score_diag32(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_rows[b], ptr(df.score), st))
    else:
        check(L.segk_fbb_score(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_rows[b], ptr(df.score), st))
    check(L.segk_fbb_segment_map(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], 0, int(seg.n_slices_min),
                                 int(seg.n_slices_max), float(seg.wip), float(seg.time_power_term), ptr(df.score),
                                 ptr(seg._dev_bounds), ptr(df.new_tok), ptr(df.n_new), ptr(df.out_logprob), ptr(df.status), st))
    check(L.segk_fbb_assign_map(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], 0, ptr(df.new_tok), ptr(df.n_new),
                                1 if sw.score_diag32 else 0, st))
    torch.cuda.synchronize()
    df.check_status()


TOLERANCE = [("diag_K65", "f32", None), ("diag_K130", "f32", None), ("ragged_diag", "f32", None), ("fixed_small", "f32", None), ("fixed_small", "f16", 12)]


@pytest.mark.parametrize("name,prec,D", TOLERANCE, ids=["%s_%s" % (c[0], c[1]) for c in TOLERANCE])
def test_tolerance_modes_decide_optimally_on_their_own_numbers(gpu, name, prec, D):
    torch = gpu
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import check, ptr
    ref, spec, seg = mb.pair(name, prec=prec, D=D)
    sw = seg._get_sweeper()
    assert sw.bt.fast_dp == 1
    sw.enter(seg._dev_bounds)
    u = ref.utterances
    n_utt, N_max, K = u.D, seg._corpus.N_max, spec.K_max
    tpt, wip, n_max = float(seg.time_power_term), float(seg.wip), int(seg.n_slices_max)
    alpha = torch.full((n_utt, N_max), float("nan"), dtype=torch.float64, device="cuda")
    ll = torch.full((n_utt * N_max, K), float("nan"), dtype=torch.float64, device="cuda")
    L, ctx = _abi.lib(), _abi.ctx()
    check(L.segk_fbb_set_probe(ctx, ptr(alpha), ptr(ll), K))
    worst_path = worst_slot = 0.0
    try:
        for b in range(sw.B):
            _one_map_step(sw, seg, b)
            score = seg._df.score.cpu().numpy()
            bnd = seg._dev_bounds.cpu().numpy().astype(bool)
            lp = seg._df.out_logprob.cpu().numpy()
            cnt = sw.cnt.cpu().numpy()
            new_tok, n_new = seg._df.new_tok.cpu().numpy().reshape(n_utt, N_max), seg._df.n_new.cpu().numpy()
            slot = sw.slot.cpu().numpy()
            llh = ll.cpu().numpy().reshape(n_utt, N_max, K)
            prior = np.log(float(spec.alpha) / K + cnt)
            for s in range(sw.S):
                for i in range(*sw.utt_range_np[s, b]):
                    # 1. boundaries: optimal for vec rebuilt from the step's own span scores (score * dur ** tpt + wip in fp64;
                    #    1e-9 covers the one multiply-add per span that host and device may round differently)
                    N = u.lengths[i]
                    tri = (N * N + N) // 2
                    vec = -np.inf * np.ones(tri)
                    for j in range(tri):
                        e = u.vec_ids[i, j]
                        if e != -1 and not np.isnan(u.durations[i, j]):
                            vec[j] = score[e] * u.durations[i, j] ** tpt
                    vec = vec + wip
                    opt, _ = no.forward_backward_viterbi(vec, 0.0, N, seg.n_slices_min, n_max, i)
                    got = mb.path_total(vec, bnd[i], N)
                    tol = 1e-9 * max(1.0, abs(opt))
                    worst_path = max(worst_path, (opt - got) / max(1.0, abs(opt)))
                    assert got >= opt - tol, (b, i, got, opt)
                    assert abs(got - lp[i]) <= tol, (b, i, got, lp[i])
                    # 2. slots: maximal for the token likelihoods the step used
                    assert n_new[i] > 0
                    for t in range(n_new[i]):
                        z = prior + llh[i, t]
                        assert not np.any(np.isnan(z))
                        k = slot[new_tok[i, t]]
                        worst_slot = max(worst_slot, (z.max() - z[k]) / max(1.0, abs(z.max())))
                        assert z[k] >= z.max() - 1e-9 * max(1.0, abs(z.max())), (b, i, t, k, int(np.argmax(z)))
    finally:
        check(L.segk_fbb_set_probe(ctx, None, None, 0))
    print("%s %s: worst shortfall of the path total %.3g, of the slot logit %.3g (relative)" % (name, prec, worst_path, worst_slot))

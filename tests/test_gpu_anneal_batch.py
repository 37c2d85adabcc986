"""The batch-synchronous FBGMM / bigram sampler (sync="batch") at temperatures other than 1, which no other GPU test passes:

  * score_precision="f64": the specification's chain (oracle/np_fbgmm_batch.py::FbgmmBatch.sweep(sweep, T, am)) bit for bit,
    per kernel form -- k_fbb_segment on triangles and on the band (fb_dp_sample_on leaves its register path for the LDS path
    whenever T != 1), the wave-per-token draws of k_fbb_slots and the block-wide draws of k_fbb_assign_lm at every chunk
    size --, through gibbs_sample's schedule and on two ranks;
  * score_precision "f32" / "f16": every boundary draw and every slot draw of one sweep, value by value, against the fp64
    probabilities of the device's own span scores, alphas and token likelihoods (segk_fbb_set_probe) -- fb_dp_sample_fast32's
    float32 re-normalisation, k_fbb_assign_lm_wave's two forms, k_fbb_step_diag32's float32 inverse temperature on base-2
    logits, and the fp64 recurrence with hardware exp / log above 64 landmarks.

The cases, their segmenter keywords and the checkers: tests/anneal.py.  That every case's draws do depend on the temperature,
and that the checkers tell the case's temperature from 1, is verified without a GPU in tests/test_anneal_batch_cpu.py."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import anneal as an
from tests import fbgmm_long as fl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


# ------------------------------------------------------------------ exact mode
def _assign_form(c):
    """(threads of k_fbb_slots / k_fbb_assign_lm, tokens per chunk) as fbb_assign_plan picks them: 512 threads and sixteen
    tokens where the bank has at most 128 slots, no language model and the rows fit; else 256 threads and _fbb_rcap tokens."""
    from tests.test_gpu_large_banks import _fbb_rcap
    K, D = c["K"], c["D"]
    rcap = _fbb_rcap(K, D)
    if K <= 128 and c["kind"] != "bigram" and rcap == 8:
        return 512, (16 if (K + 16 * D + 16 + 16) * 8 + 16 * K * 8 <= 80 * 1024 else rcap)
    return 256, rcap


# what the named cases are there for: (N_max > 64, window class, threads, tokens per chunk)
FORMS = {
    "fixed_w5_fb": (False, "<=16", 512, 16), "fixed_w5_am": (False, "<=16", 512, 16), "diag_w5_am": (False, "<=16", 512, 16),
    "bigram_w5_am": (False, "<=16", 256, 8), "wide_fixed_w20": (False, "17..64", 512, 16), "wide_diag_w20": (False, "17..64", 512, 16),
    "wide_fixed_w30_n64": (False, "17..64", 512, 16), "long_ragged_fixed": (True, "<=16", 512, 16),
    "long_ragged_diag": (True, "<=16", 512, 16), "long_ragged_bigram": (True, "<=16", 256, 8),
    "long_diag_100_w20": (True, "17..64", 512, 16), "K300_am": (False, "<=16", 256, 8),
    "bank_rcap4_fixed": (False, "<=16", 256, 4), "bank_rcap1_diag": (False, "<=16", 256, 1),
}


@pytest.mark.parametrize("name", list(an.EXACT))
def test_annealed_sweeps_match_specification(gpu, name):
    """tests/test_gpu_fbgmm_batch.py's check (boundaries, slots, bigram table, canonical assignments and counts equal;
    log-probabilities to 1e-9 relative) over two sweeps at the case's temperature."""
    from tests.test_gpu_fbgmm_batch import _chains_match
    c = an.EXACT[name]
    ref, spec, seg = an.build(c, product=True)
    N_max = seg._corpus.N_max
    assert N_max == int(np.max(ref.utterances.lengths))
    if c["src"] == "chain" and c["n_landmarks"]:
        assert N_max == c["n_landmarks"]
    form = (N_max > 64, "<=16" if c["nmax"] <= 16 else "17..64") + _assign_form(c)
    assert 1 <= c["nmax"] <= 64
    if name in FORMS:
        assert form == FORMS[name], (name, form)
    assert seg.n_slices_min == c["kw"].get("n_slices_min", 0)
    _chains_match(gpu, ref, spec, seg, 2, c["T"], c["am"])
    assert seg._get_sweeper()._fused is None          # (f64: the fused step is never tried)


@pytest.mark.parametrize("driver", list(an.DRIVER))
def test_annealing_schedule_of_gibbs_sample_in_batch_mode(gpu, driver):
    """gibbs_sample with the reference's default schedule (linear in 1 / T from 0.1) and anneal_gibbs_am on a sync="batch"
    segmenter: the specification stepped with the same temperatures."""
    name = an.DRIVER[driver]
    c = an.EXACT[name]
    ref, spec, seg = an.build(c, product=True)
    assert type(seg).__name__ == ("BigramAcousticWordseg" if driver == "bigram" else "UnigramAcousticWordseg")
    n = 3
    temps = 1. / np.linspace(0.1, 1, n)
    lps = [spec.sweep(sw, float(temps[sw]), True) for sw in range(n)]
    rec = seg.gibbs_sample(n, anneal_schedule="linear", anneal_start_temp_inv=0.1, anneal_gibbs_am=True)
    assert np.array_equal(np.array(rec["anneal_temp"]), temps)
    assert temps[0] == 10.0 and temps[-1] == 1.0
    npt.assert_allclose(rec["log_marg*length"], [lp.sum() for lp in lps], rtol=1e-9)
    assert np.array_equal(seg.utterances.boundaries, ref.utterances.boundaries)
    assert np.array_equal(seg._get_sweeper().slot.cpu().numpy(), spec.slot)
    a, Kc = spec.canonical()
    comp = seg.acoustic_model.components
    assert comp.K == Kc and np.array_equal(comp.assignments, a)
    assert list(rec["components"])[-1] == Kc


def test_annealed_sweeps_on_two_ranks_equal_one_rank_and_the_specification(gpu):
    """Two virtual ranks (tests/virtual_ranks.py) under annealing: the specification's bits on every rank -- and so one
    rank's, which test_annealed_sweeps_match_specification holds to the same chain."""
    from tests.virtual_ranks import VirtualWorld
    c = an.EXACT[an.RANKS]
    T, am = c["T"], c["am"]
    corpus = fl.corpus_of(c)
    ref, spec = fl.oracle_of(c, corpus=corpus)
    want = []
    for sw in range(2):
        lp = spec.sweep(sw, T, am)
        want.append((ref.utterances.boundaries.copy(), lp.copy()))

    def run(comm):
        seg = fl.product_of(c, corpus=corpus, process_group=comm)
        states = []
        for sw in range(len(want)):
            seg.batch_sweep_async(T, am)
            gpu.cuda.synchronize()
            seg._df.check_status()
            lp = seg._get_sweeper().utt_values(seg._df.out_logprob)
            seg.materialise()
            states.append((seg.utterances.boundaries.copy(), lp))
        comp = seg.acoustic_model.components
        return states, comp.assignments.copy(), comp.K, comp.counts.copy()

    for states, assignments, K, counts in VirtualWorld(2).run(run):
        for (bnd, lp), (wb, wlp) in zip(states, want):
            assert np.array_equal(bnd, wb)
            npt.assert_allclose(lp, wlp, rtol=1e-9)
        a, Kc = spec.canonical()
        assert K == Kc and np.array_equal(assignments, a)
        cnt = spec.stats_excluding(-1)[0]
        assert np.array_equal(counts[:Kc], cnt[cnt > 0])


# ------------------------------------------------------------------ tolerance modes
@pytest.mark.parametrize("annealed", [False, True], ids=["T1", "annealed"])
@pytest.mark.parametrize("name", list(an.TOLERANCE))
def test_draws_of_the_tolerance_modes_under_annealing(gpu, monkeypatch, name, annealed):
    """One sweep's Gibbs steps (tests/test_gpu_tolerance_modes.py::_one_step: every block against the initial state) at T = 1
    and at the case's temperature, boundaries and slots annealed.

    Slots: every token's uniform against the interval of the slot it drew -- fp64 softmax((prior + ll) / T) of the
    specification's prior and the device's own probed token log-likelihoods; bound 1e-4 max(1, 1 / T).

    Boundaries: every backward step's uniform against the interval of the segment it chose -- fp64 softmax(w / T) of the
    device's own span scores and probed alphas; bound 2 delta / T + 1e-5, delta = 4 ulp of float32 at the step's largest
    operand (tests/anneal.py::boundary_bound: derived from the float32 DP's roundings, not measured).

    Measured on an MI355X: in all eighteen runs every uniform lies inside its interval (worst slot distance 0, worst
    boundary distance 0, i.e. 0 of the bound, over 170 to 330 draws of each kind per run), while intervals computed at the
    wrong temperature put 0.20 to 0.38 of the boundary draws and 0.27 to 0.75 of the slot draws outside the bounds
    (tests/test_anneal_batch_cpu.py).  The worst distances are printed."""
    torch = gpu
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import check, ptr
    from tests.test_gpu_tolerance_modes import _one_step
    c = an.TOLERANCE[name]
    T = c["T"] if annealed else 1.0
    fused = c.get("form") == "fused"
    if c.get("form") == "0":
        monkeypatch.setenv("SEGK_FBB_ASSIGN_WAVE", "0")
    ref, spec, seg = an.build(c, product=True)
    kind, K, W = c["kind"], c["K"], c["nmax"]
    u = ref.utterances
    n_utt, N_max = u.D, seg._corpus.N_max
    sw = seg._get_sweeper()
    assert sw.bt.fast_dp == 1
    if name.startswith("long_"):
        assert N_max > 64
    else:
        assert N_max <= 64 and W <= 16          # fb_dp_sample_fast32
    if kind == "bigram":
        assert sw.ll_mat is not None and (K > 1024) == name.endswith("K1100")
    sw.enter(seg._dev_bounds)
    alpha = torch.full((n_utt, N_max), float("nan"), dtype=torch.float64, device="cuda")
    ll = torch.full((n_utt * N_max, K), float("nan"), dtype=torch.float64, device="cuda")
    L, ctx = _abi.lib(), _abi.ctx()
    check(L.segk_fbb_set_probe(ctx, ptr(alpha), ptr(ll), K))
    try:
        for b in range(sw.B):
            _one_step(sw, seg, b, fused=fused, anneal_temp_fb=T, anneal_temp_am=T)
    finally:
        check(L.segk_fbb_set_probe(ctx, None, None, 0))
    alpha, ll = alpha.cpu().numpy(), ll.cpu().numpy().reshape(n_utt, N_max, K)
    score = seg._df.score.cpu().numpy()          # every row as its block's step scored it
    new_tok, n_new = seg._df.new_tok.cpu().numpy(), seg._df.n_new.cpu().numpy()
    bounds = seg._dev_bounds.cpu().numpy().astype(bool)
    slots = sw.slot.cpu().numpy()
    tpt, wip = float(ref.time_power_term), float(ref.wip)
    worst_slot = worst_fb = worst_fb_abs = 0.0
    n_tok = n_steps = n_moved = n_drawn_empty = 0
    for b in range(sw.B):
        d = spec.derive(*spec.stats_excluding(b))
        if kind == "bigram":           # (the one-wave kernel's register form takes the empty slots as one annealed term)
            assert not d["active"].all()
        uni = big = None
        if kind == "bigram":           # LM counts of all other blocks
            uni, big = spec.uni.copy(), spec.big.copy()
            for s in range(spec.S):
                for i in range(*spec.ranges[s][b]):
                    spec._lm_count(uni, big, spec.tr[i], -1)
        for s in range(spec.S):
            for i in range(*spec.ranges[s][b]):
                N = u.lengths[i]
                tri = N * (N + 1) // 2
                ids, dur = u.vec_ids[i, :tri], u.durations[i, :tri]
                assert not np.isnan(dur[ids >= 0]).any()
                vec = np.full(tri, -np.inf)
                vec[ids >= 0] = score[ids[ids >= 0]] * dur[ids >= 0] ** tpt
                vec = vec + wip
                assert np.all(np.isfinite(alpha[i, :N])), i
                assert bounds[i, N - 1]
                n_moved += not np.array_equal(bounds[i, :N], u.boundaries[i, :N])
                for dist, M in an.boundary_draw_distance(vec, alpha[i, :N], N, W, T, bounds[i, :N], spec.seed, 0, i):
                    bound = an.boundary_bound(M, T)
                    worst_fb, worst_fb_abs = max(worst_fb, dist / bound), max(worst_fb_abs, dist)
                    n_steps += 1
                # the tokens the device lists are the segments of the boundaries it sampled
                assert n_new[i] == int(np.count_nonzero(np.asarray(_segment_rows(u, bounds[i, :N], i)) != -1))
                j_prev = None
                for t in range(n_new[i]):
                    assert np.all(np.isfinite(ll[i, t])), (i, t)
                    k = int(slots[new_tok[i, t]])
                    assert 0 <= k < K
                    dist = an.slot_draw_distance(spec.prior_z(d, j_prev, uni, big), ll[i, t], T, k,
                                                 an.token_uniform(spec.seed, 0, i, N_max, t))
                    worst_slot = max(worst_slot, dist)
                    n_tok += 1
                    n_drawn_empty += int(not d["active"][k])
                    j_prev = k if kind == "bigram" else None
    print("%s T = %g: worst slot distance %.3g (bound %.3g) over %d tokens; worst boundary distance %.3g, %.3g of its bound, "
          "over %d backward steps; %d tokens drew an empty slot; %d of %d utterances left their initial boundaries"
          % (name, T, worst_slot, an.slot_bound(T), n_tok, worst_fb_abs, worst_fb, n_steps, n_drawn_empty, n_moved, n_utt))
    assert n_tok >= 2 * n_utt and n_steps >= n_tok
    assert worst_slot <= an.slot_bound(T), worst_slot
    assert worst_fb <= 1.0, (worst_fb, worst_fb_abs)


def _segment_rows(u, bnd, i):
    out, j_prev = [], 0
    for j in range(len(bnd)):
        if bnd[j]:
            out.append(u.vec_ids[i, (j + 1) * j // 2 + j_prev])
            j_prev = j + 1
    return out


def test_fused_gibbs_step_against_the_three_launches_under_annealing(gpu):
    """tests/test_gpu_tolerance_modes.py::_fused_against_three_launches at T = 10 with the keywords of the fused cases: span
    scores, boundaries, log-probabilities and token counts bit-identical, slots equal on more than 0.98 of the tokens -- and
    the boundaries are not those of T = 1 (the comparison would otherwise hold for a kernel pair that both ignored T)."""
    from tests.test_gpu_tolerance_modes import _fused_against_three_launches
    kw = an.TOLERANCE["diag_f32_fused_K100"]["kw"]
    hot = _fused_against_three_launches(None, 10.0, **kw)
    cold = _fused_against_three_launches(None, 1.0, **kw)
    assert np.array_equal(hot[0], cold[0])            # the span scores do not depend on the temperature
    assert np.mean(np.any(hot[1] != cold[1], axis=1)) >= 0.10

"""The batch-synchronous FBGMM / bigram sampler on corpora whose longest utterance has more than 64 landmarks (up to 256):
bit for bit the specification oracle/np_fbgmm_batch.py with score_precision="f64" -- boundaries, slots, bigram table;
log-probabilities to 1e-9 relative --, the 1e-4 contract in the tolerance modes, the same bits on two ranks, and the
refusals that remain.  Such corpora run the banded boundary kernel (k_fbb_segment<BAND>) and the chunked partial sums;
corpora of at most 64 landmarks keep the triangular kernel.  The corpora and what each is there for: tests/fbgmm_long.py;
that they do exercise it is checked with the oracle in tests/test_fbgmm_batch_long_cpu.py and again here, before the device
runs."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import np_oracle as no
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


def _specification(name, sweeps=2):
    """The oracle's side first: per sweep (boundaries, slots, bigram table, log-probabilities), the canonical view after the
    last one, and the conditions that keep the case from passing vacuously."""
    ref, spec = fl.oracle_of(name)
    want = []
    with fl.DpCensus() as census:
        for sw in range(sweeps):
            lp = spec.sweep(sw)
            assert np.all(np.isfinite(lp)), (name, sw)
            want.append((ref.utterances.boundaries.copy(), spec.slot.copy(),
                         spec.big.copy() if fl.CASES[name]["kind"] == "bigram" else None, lp.copy()))
    if name.startswith("short_"):
        assert fl.longest(ref) <= 64
    else:
        assert fl.longest(ref) > 64
    if name == "diag_65":
        assert fl.longest(ref) == 65 and min(ref.utterances.lengths) < fl.CASES[name]["nmax"]
    if name == "fixed_150_w1":
        assert max(fl.tokens_per_utterance(ref)) > 64
    if name == "diag_mindur":
        assert census.dead_windows > 0
    if name == "diag_mindur_backtrack":
        assert census.backtracks > 0
    return ref, spec, want


def _sweeps_match(gpu, name, seg, ref, spec, want):
    kind = fl.CASES[name]["kind"]
    for sw, (bnd, slot, big, lp) in enumerate(want):
        seg.batch_sweep_async()
        gpu.cuda.synchronize()
        seg._df.check_status()
        assert np.array_equal(seg.utterances.boundaries, bnd), (name, sw)
        assert np.array_equal(seg._get_sweeper().slot.cpu().numpy(), slot), (name, sw)
        if kind == "bigram":
            assert np.array_equal(seg._get_sweeper().lm_big.cpu().numpy(), big), (name, sw)
        npt.assert_allclose(seg._df.out_logprob.cpu().numpy(), lp, rtol=1e-9)
    seg.materialise()
    a, Kc = spec.canonical()
    c = seg.acoustic_model.components
    assert c.K == Kc
    assert np.array_equal(c.assignments, a)
    cnt = spec.stats_excluding(-1)[0]
    assert np.array_equal(c.counts[:Kc], cnt[cnt > 0])
    if kind == "bigram":
        occ = np.where(cnt > 0)[0]
        assert np.array_equal(seg.lm.unigram_counts[:Kc], cnt[occ])
        assert np.array_equal(seg.lm.bigram_counts[:Kc, :Kc], spec.big[np.ix_(occ, occ)])


F64 = [n for n in fl.CASES if "prec" not in fl.CASES[n]]


@pytest.mark.parametrize("name", F64)
def test_long_utterance_sweeps_match_specification(gpu, name):
    ref, spec, want = _specification(name)
    seg = fl.product_of(name)
    assert seg._corpus.N_max == fl.longest(ref)
    _sweeps_match(gpu, name, seg, ref, spec, want)
    assert seg._get_sweeper()._fused is None          # (f64: the fused step is never tried)


@pytest.mark.parametrize("name", ["fixed_f32", "diag_f32", "fixed_f16", "bigram_f16"])
def test_long_utterance_tolerance_modes(gpu, name):
    """score_precision="f32" / "f16" above 64 landmarks: the span scores within the path's 1e-4 of the specification's log_marg_i (as
    tests/test_gpu_fbgmm_batch.py::_diag_float32_span_scores measures them), the fused Gibbs step refused and replaced by the
    score / segment / assign launches, and the banded DP's forward filter (fp64 recurrence with the hardware exponential
    and logarithm; read through segk_fbb_set_probe) within 1e-4 of the fp64 recurrence on the device's own span scores."""
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import check, ptr
    torch = gpu
    c = fl.CASES[name]
    ref, spec = fl.oracle_of(name)
    assert fl.longest(ref) > 64
    seg = fl.product_of(name)
    sw = seg._get_sweeper()
    assert sw.bt.fast_dp == 1 and (sw.score_diag32 if c["kind"] == "diag" else sw.score_f32)
    sw.enter(seg._dev_bounds)
    L, ctx, cp, fp, bp, st = sw._args()
    worst = 0.0
    for b in range(sw.B):
        check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
        if c["kind"] == "diag":
            check(L.segk_fbb_score_diag32(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_rows[b], ptr(seg._df.score), st))
        else:
            check(L.segk_fbb_score_f32(ctx, cp, fp, bp, ptr(sw._block_rows[b]), sw._block_rows[b].numel(), ptr(seg._df.score), st))
        d = spec.derive(*spec.stats_excluding(b))
        # with a language model the unigram counts of "all other blocks" are the slot counts
        uni, big = (d["cnt"], spec.big) if c["kind"] == "bigram" else (None, None)
        score = seg._df.score.cpu().numpy()
        for s_ in range(sw.S):
            lo, hi = sw.row_range_np[s_, b]
            for row in range(lo, hi):
                want = spec.log_marg(d, spec.X[row], uni, big)
                worst = max(worst, abs(score[row] - want) / max(abs(want), 1.0))
    print("%s: worst span-score error relative to max(|log_marg_i|, 1) = %.3g" % (name, worst))
    assert worst < 1e-4, worst
    # one sweep with the forward filter probed
    n_utt, N_max, W = c["n_utt"], seg._corpus.N_max, c["nmax"]
    alpha = torch.full((n_utt, N_max), float("nan"), dtype=torch.float64, device="cuda")
    check(L.segk_fbb_set_probe(ctx, ptr(alpha), None, 0))
    try:
        seg.batch_sweep_async()
        gpu.cuda.synchronize()
    finally:
        check(L.segk_fbb_set_probe(ctx, None, None, 0))
    seg._df.check_status()
    if c["kind"] == "diag":
        assert sw._fused is False          # refused for N_max > 64: the launches took over
    alpha = alpha.cpu().numpy()
    score = seg._df.score.cpu().numpy()    # every row as its block's step scored it
    u = ref.utterances
    worst_a = 0.0
    for i in range(n_utt):
        N = u.lengths[i]
        tri = N * (N + 1) // 2
        vec = -np.inf * np.ones(tri)
        for j in range(tri):
            e = u.vec_ids[i, j]
            if e != -1 and not np.isnan(u.durations[i, j]):
                vec[j] = score[e] * u.durations[i, j]
        a_own = no.forward_alphas(vec, 0.0, N, W)
        got = alpha[i, :N]
        assert np.all(np.isfinite(got)), (i, got)
        worst_a = max(worst_a, float(np.max(np.abs(got - a_own) / np.maximum(np.abs(a_own), 1.0))))
    print("%s: worst forward-filter error relative to max(|alpha|, 1) = %.3g" % (name, worst_a))
    assert worst_a < 1e-4, worst_a
    # the chain is a valid one
    seg.batch_sweep_async()
    gpu.cuda.synchronize()
    seg._df.check_status()
    seg.materialise()
    comp = seg.acoustic_model.components
    assert comp.counts[:comp.K].sum() == seg.acoustic_model.get_n_assigned()
    if c["kind"] == "bigram":
        assert seg.lm.unigram_counts.sum() == seg.acoustic_model.get_n_assigned()


def test_long_utterances_on_two_ranks_equal_one_rank_and_the_specification(gpu):
    """`ragged_fixed` (S = 4) on two virtual ranks (tests/virtual_ranks.py): the specification's bits on every rank."""
    from tests.virtual_ranks import VirtualWorld
    name = "ragged_fixed"
    ref, spec, want = _specification(name)
    corpus = fl.corpus_of(name)

    def run(comm):
        seg = fl.product_of(name, corpus=corpus, process_group=comm)
        states = []
        for sw in range(len(want)):
            seg.batch_sweep_async()
            gpu.cuda.synchronize()
            seg._df.check_status()
            # (collectives, in the same order on every rank; materialise() fetches the other rank's boundaries, as
            # gibbs_sample does after every sweep, and leaves the batch state alone)
            lp = seg._get_sweeper().utt_values(seg._df.out_logprob)
            seg.materialise()
            states.append((seg.utterances.boundaries.copy(), lp))
        c = seg.acoustic_model.components
        return states, c.assignments.copy(), c.K, c.counts.copy()

    for states, assignments, K, counts in VirtualWorld(2).run(run):
        for (bnd, lp), (wb, _, _, wlp) in zip(states, want):
            assert np.array_equal(bnd, wb)
            npt.assert_allclose(lp, wlp, rtol=1e-9)
        a, Kc = spec.canonical()
        assert K == Kc and np.array_equal(assignments, a)
        cnt = spec.stats_excluding(-1)[0]
        assert np.array_equal(counts[:Kc], cnt[cnt > 0])


def _refusal_segmenter(N, corpus_window, window, n_utt=4, **over):
    case = dict(kind="fixed", n_utt=n_utt, D=4, K=6, cseed=120, N=N, nmax=corpus_window, B=2, S=2)
    corpus = fl.corpus_of(case)
    case["nmax"] = window
    case.update(over)
    return fl.product_of(case, corpus=corpus)


def test_refusal_unbounded_window(gpu):
    from segmentalist_amd._abi import SegkError
    seg = _refusal_segmenter(70, 6, 6)
    seg.n_slices_max = 0               # the unbounded window: the band would be the triangle
    with pytest.raises(SegkError, match="window of 1..64 slices"):
        seg.batch_sweep_async()


def test_refusal_embeddings_outside_the_window(gpu):
    from segmentalist_amd._abi import SegkError
    seg = _refusal_segmenter(70, 9, 7)          # embeddings for spans of up to nine slices, a window of seven
    assert seg._corpus.band_ids is None
    with pytest.raises(SegkError, match="no complete band"):
        seg.batch_sweep_async()


def test_refusal_band_beyond_lds(gpu):
    from segmentalist_amd._abi import SegkError
    seg = _refusal_segmenter(300, 50, 50)       # 12 * 300 * 50 bytes of band alone: more than a workgroup's 160 KB
    assert seg._corpus.band_W == 50
    with pytest.raises(SegkError, match=r"does not fit in LDS: N_max = 300 landmarks, window W = 50"):
        seg.batch_sweep_async()

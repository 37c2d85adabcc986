"""
Direct tolerance tests of the modes `bench.py --workload fbgmm_diag_c2 / bigram_c5` time (score_precision "f32" / "f16").
north_star: "log-likelihoods within 1e-4 rel for FBGMM".  The span scores of these modes are held to that bound in
tests/test_gpu_fbgmm_batch.py; here the OTHER places where reduced-precision arithmetic enters the sampler are measured
value by value against the fp64 specification (oracle/np_fbgmm_batch.py, built from the reference's densities:
gaussian_components_diag.py:237-259, gaussian_components_fixedvar.py:242-253, unigram_acoustic_wordseg.py:684-703), at
configs[1] (D = 39, K = 100) and configs[4] (D = 100, K = 1000) shapes, through the library's probes
(segk_fbb_set_probe):

  * the token log-likelihoods the assignment draws are made from -- float32 Student-t terms with v_log_f32
    (segk_fbb_assign_diag32), the fp16x2 matrix-core contraction (segk_fbb_token_scores -> segk_fbb_assign, with and
    without a language model: the block-wide form and the one-wave-per-utterance form);
  * the forward filter's alphas of the boundary sampler with hardware exp / log (segk_fbatch.fast_dp = 1).

Bound: |got - want| <= 1e-4 * max(|want|, 1).
"""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import affine

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _pair(kind, n_utt, D, K, prec, B=3, S=2, seed=5, transform=None, product=True, **kw):
    """transform: a name of tests/affine.py -- the corpus and the prior moved to new coordinates together.  product=False: the
    oracle's side alone (no device), None in the product's place.  kw: segmenter keywords over the defaults below."""
    if product:
        from segmentalist_amd import bigram_acoustic_wordseg as baw, fbgmm, unigram_acoustic_wordseg as uaw
        from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
        from segmentalist_amd.niw import NIW
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(n_utt, D, K, seed=17, N=20, n_slices_max=6)          # the bench generator: 105 spans per utterance
    args = dict(n_slices_min=0, n_slices_max=6, p_boundary_init=0.5, beta_sent_boundary=-1, lms=1.0, wip=0.0,
                init_am_assignments="rand", time_power_term=1.0)
    args.update(kw)
    bargs = dict(sync="batch", n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=11, score_precision=prec)
    fixed = (0.002 * np.ones(D), np.zeros(D), 0.002 / 0.05 * np.ones(D))
    niw = (np.zeros(D), 0.05, D + 3, 0.002 * (D + 3) * np.ones(D))
    lm = {"type": "smooth", "intrp_lambda": 0.1, "a": 0.5, "b": 0.5}
    if transform is not None:
        s, c = affine.params(transform, D)
        corpus = affine.corpus(corpus, s, c)
        fixed, niw = affine.fixed_prior(*fixed, s, c), affine.niw_prior(*niw, s, c)
    out = []
    for side in ("oracle", "product"):
        if side == "product" and not product:
            out.append(None)
            continue
        random.seed(seed)
        np.random.seed(seed)
        if kind == "bigram":
            seg = (no.BigramAcousticWordseg(K, no.FixedVarPrior(*fixed), dict(lm), *corpus, covariance_type="fixed",
                                            fb_type="unigram", **args) if side == "oracle" else
                   baw.BigramAcousticWordseg(K, FixedVarPrior(*fixed), dict(lm), *corpus, covariance_type="fixed",
                                             fb_type="unigram", **args, **bargs))
        elif side == "oracle":
            prior = no.FixedVarPrior(*fixed) if kind == "fixed" else no.NIW(*niw)
            seg = no.UnigramAcousticWordseg(no.FBGMM, 1.0, K, prior, *corpus, covariance_type=kind, fb_type="standard", **args)
        else:
            prior = FixedVarPrior(*fixed) if kind == "fixed" else NIW(*niw)
            seg = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, prior, *corpus, covariance_type=kind, fb_type="standard",
                                             **args, **bargs)
        out.append(seg)
    ref, seg = out
    return ref, nb.FbgmmBatch(ref, n_gibbs_blocks=B, n_stat_blocks=S, seed=11), seg


def _one_step(sw, seg, b, sweep=0, fused=False, anneal_temp_fb=1.0, anneal_temp_am=1.0):
    """Gibbs step b of the sampler as FbgmmBatchSweeper.sweep enqueues it, without the partial-sum refresh (so that every
    step of this test conditions on the INITIAL state of the other blocks, which is what the specification object holds).
    The segmenter's own window, word insertion penalty and time power term; the temperatures of the boundary draws and of the
    slot draws as given."""
    n_min, n_max, wip, tpt = int(seg.n_slices_min), int(seg.n_slices_max), float(seg.wip), float(seg.time_power_term)
    T_fb, T_am = float(anneal_temp_fb), float(anneal_temp_am)
    import torch
    from segmentalist_amd._abi import check, ptr
    df = seg._df
    L, ctx, cp, fp, bp, st = sw._args()
    if sw.lm_tok is not None:
        check(L.segk_fbb_lm_apply(ctx, cp, fp, bp, b, -1, st))
    check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
    if fused:                  # the three calls below as one launch (diagonal components, float32 terms)
        check(L.segk_fbb_step_diag32(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], sweep, n_min, n_max, wip, tpt, T_fb, T_am,
                                     ptr(df.score), ptr(seg._dev_bounds), ptr(df.new_tok), ptr(df.n_new), ptr(df.out_logprob),
                                     ptr(df.status), st))
        torch.cuda.synchronize()
        df.check_status()
        return
    if sw.score_f32:
        check(L.segk_fbb_score_f32(ctx, cp, fp, bp, ptr(sw._block_rows[b]), sw._block_rows[b].numel(), ptr(df.score), st))
    elif sw.score_diag32:
        check(L.segk_fbb_score_diag32(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_rows[b], ptr(df.score), st))
    else:
        check(L.segk_fbb_score(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_rows[b], ptr(df.score), st))
    check(L.segk_fbb_segment(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], sweep, n_min, n_max, wip, tpt, T_fb, ptr(df.score),
                             ptr(seg._dev_bounds), ptr(df.new_tok), ptr(df.n_new), ptr(df.out_logprob), ptr(df.status), st))
    if sw.ll_mat is not None:
        tm = sw._tok_map[b]
        rows = sw._tok_rows[:tm.numel()]
        torch.index_select(df.new_tok.view(-1), 0, tm, out=rows)
        check(L.segk_fbb_token_scores(ctx, cp, fp, bp, ptr(rows), tm.numel(), ptr(sw.ll_mat), sw.ll_ld, st))
        check(L.segk_fbb_assign(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], sweep, T_am, ptr(df.new_tok), ptr(df.n_new),
                                ptr(sw.ll_mat), sw.ll_ld, st))
    elif sw.score_diag32:
        check(L.segk_fbb_assign_diag32(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], sweep, T_am, ptr(df.new_tok),
                                       ptr(df.n_new), st))
    else:
        check(L.segk_fbb_assign(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], sweep, T_am, ptr(df.new_tok), ptr(df.n_new),
                                None, 0, st))
    if sw.lm_tok is not None:          # put the block's old transcripts back: the next step starts from the initial tables
        check(L.segk_fbb_lm_apply(ctx, cp, fp, bp, b, 1, st))
    torch.cuda.synchronize()
    df.check_status()


CASES = [
    ("diag", "f32", 48, 39, 100, None),            # configs[1] shape: float32 Student-t token likelihoods, fast_dp
    ("diag", "f32", 48, 39, 100, "fused"),         # ... the Gibbs step as one launch (segk_fbb_step_diag32)
    ("diag", "f32", 40, 20, 160, "fused"),         # ... with three chunks of 64 slots
    ("diag", "f32", 48, 39, 130, None),            # the first row beyond 128 slots: segk_fbb_assign_diag32 with one thread per slot
    ("fixed", "f16", 48, 39, 100, None),           # fp16x2 token likelihoods, block-wide draw kernel, fast_dp
    ("fixed", "f32", 48, 39, 100, None),           # fp32 MFMA span scores, fp64 token likelihoods, fast_dp
    ("bigram", "f16", 48, 100, 1000, None),        # configs[4] shape: one wave per utterance, hardware log / exp
    ("bigram", "f16", 48, 100, 1000, "0"),         # ... and the block-wide form it replaced (SEGK_FBB_ASSIGN_WAVE=0)
    ("fixed", "f16", 36, 100, 1000, None),
    ("bigram", "f16", 40, 60, 1100, None),         # more than 1 024 slots: the wave kernel's per-slot loops behind the column table
]


@pytest.mark.parametrize("kind,prec,n_utt,D,K,wave", CASES,
                         ids=["%s_%s_D%d_K%d%s" % (c[0], c[1], c[3], c[4], "" if c[5] is None else "_fused" if c[5] == "fused" else "_blockwide")
                              for c in CASES])
def test_token_likelihoods_and_forward_filter_within_the_contract(gpu, monkeypatch, kind, prec, n_utt, D, K, wave):
    _token_likelihoods_and_forward_filter(gpu, monkeypatch, kind, prec, n_utt, D, K, wave)


# the same measurements on corpora moved away from the origin and rescaled (tests/affine.py): the configs[1] shape (D = 39 is
# odd: 2D = 78, ldy = 80, the zero tail of the operand rows), the three forms of the fp16x2 token likelihoods (block-wide, one
# wave per utterance with a language model, the bigram model at the configs[4] shape).  (A small odd D -- 13, 21 -- has span
# scores of both signs: some alphas pass within 1 of zero, where max(|alpha|, 1) no longer scales with the sum of the span
# errors times their durations, and the comparison fails at the identity transform in every mode.  Its span scores are
# measured in test_gpu_fbgmm_batch.py.)
AFFINE_CASES = [
    ("diag", "f32", 30, 39, 100, None),
    ("diag", "f32", 30, 39, 100, "fused"),
    ("fixed", "f32", 30, 39, 100, None),
    ("fixed", "f16", 30, 39, 100, None),
    ("bigram", "f16", 30, 39, 100, None),
    ("bigram", "f16", 25, 100, 1000, None),
]


@pytest.mark.parametrize("transform", affine.NAMES)
@pytest.mark.parametrize("kind,prec,n_utt,D,K,wave", AFFINE_CASES,
                         ids=["%s_%s_D%d_K%d%s" % (c[0], c[1], c[3], c[4], "" if c[5] is None else "_fused") for c in AFFINE_CASES])
def test_token_likelihoods_and_forward_filter_on_transformed_corpora(gpu, monkeypatch, kind, prec, n_utt, D, K, wave,
                                                                     transform):
    _token_likelihoods_and_forward_filter(gpu, monkeypatch, kind, prec, n_utt, D, K, wave, transform)


def _token_likelihoods_and_forward_filter(gpu, monkeypatch, kind, prec, n_utt, D, K, wave, transform=None):
    torch = gpu
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import check, ptr
    fused = wave == "fused"
    if wave is not None and not fused:
        monkeypatch.setenv("SEGK_FBB_ASSIGN_WAVE", wave)
    ref, spec, seg = _pair(kind, n_utt, D, K, prec, transform=transform)
    sw = seg._get_sweeper()
    assert sw.bt.fast_dp == 1
    sw.enter(seg._dev_bounds)
    u = ref.utterances
    N_max = seg._corpus.N_max
    alpha = torch.full((n_utt, N_max), float("nan"), dtype=torch.float64, device="cuda")
    ll = torch.full((n_utt * N_max, K), float("nan"), dtype=torch.float64, device="cuda")
    L, ctx = _abi.lib(), _abi.ctx()
    check(L.segk_fbb_set_probe(ctx, ptr(alpha), ptr(ll), K))
    try:
        for b in range(sw.B):
            _one_step(sw, seg, b, fused=fused)
    finally:
        check(L.segk_fbb_set_probe(ctx, None, None, 0))
    alpha, ll = alpha.cpu().numpy(), ll.cpu().numpy().reshape(n_utt, N_max, K)
    score = seg._df.score.cpu().numpy()
    new_tok, n_new = seg._df.new_tok.cpu().numpy(), seg._df.n_new.cpu().numpy()
    worst_ll = worst_a_own = worst_a_spec = worst_draw = 0.0
    at_a_spec = (0.0, 0.0)             # (|got - want|, |want|) where worst_a_spec was found
    n_tok = n_occ = n_drawn_empty = 0
    slots = sw.slot.cpu().numpy()
    for b in range(sw.B):
        d = spec.derive(*spec.stats_excluding(b))
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
                # --- forward filter: (i) against the fp64 recurrence on the device's own span scores, (ii) against the
                # specification end to end (fp64 scores, library exp / log)
                vec_own = -np.inf * np.ones(tri)
                vec_spec = -np.inf * np.ones(tri)
                for j in range(tri):
                    e = u.vec_ids[i, j]
                    if e == -1 or np.isnan(u.durations[i, j]):
                        continue
                    vec_own[j] = score[e] * u.durations[i, j]
                    vec_spec[j] = spec.log_marg(d, spec.X[e], uni, big) * u.durations[i, j]
                a_own = no.forward_alphas(vec_own, 0.0, N, 6)
                a_spec = no.forward_alphas(vec_spec, 0.0, N, 6)
                got = alpha[i, :N]
                assert np.all(np.isfinite(got)), (i, got)
                worst_a_own = max(worst_a_own, float(np.max(np.abs(got - a_own) / np.maximum(np.abs(a_own), 1.0))))
                rel = np.abs(got - a_spec) / np.maximum(np.abs(a_spec), 1.0)
                if float(np.max(rel)) > worst_a_spec:
                    worst_a_spec = float(np.max(rel))
                    at_a_spec = (float(np.abs(got - a_spec)[np.argmax(rel)]), float(np.abs(a_spec)[np.argmax(rel)]))
                # --- token log-likelihoods, every slot
                assert n_new[i] > 0
                for t in range(n_new[i]):
                    want = spec.loglik(d, spec.X[new_tok[i, t]])
                    g = ll[i, t]
                    assert np.all(np.isfinite(g)), (i, t)
                    worst_ll = max(worst_ll, float(np.max(np.abs(g - want) / np.maximum(np.abs(want), 1.0))))
                    n_tok += 1
                    n_occ += int(d["active"].sum())
                # --- the draws: slot k was drawn with the token's uniform u iff cum(k - 1) <= u < cum(k), cum the running sum
                # of the probabilities in slot order (utils.draw).  Probabilities out of the device's own fp64 token
                # log-likelihoods and the specification's prior (the device: v_log_f32 / v_exp_f32, ~3e-6 relative; the
                # one-wave kernel sums the occupied slots and the block of equal empty ones separately)
                if kind == "bigram" or fused:
                    j_prev = None
                    for t in range(n_new[i]):
                        z = spec.prior_z(d, j_prev, uni, big) + ll[i, t]
                        pr = np.exp(z - z.max())
                        cum = np.cumsum(pr / pr.sum())
                        k = int(slots[new_tok[i, t]])
                        assert 0 <= k < K
                        uu = nb.u01(spec.seed, 0, i, N_max + t)
                        below = cum[k - 1] if k > 0 else 0.0
                        worst_draw = max(worst_draw, below - uu, uu - cum[k])
                        n_drawn_empty += int(not d["active"][k])
                        j_prev = k if kind == "bigram" else None
    print("%s %s D=%d K=%d%s%s: token log-likelihoods worst %.3g (over %d tokens x %d slots, %.0f occupied per token); "
          "alphas worst %.3g against fp64 on the device's scores, %.3g against the specification (%.3g at |alpha| %.3g)"
          % (kind, prec, D, K, " fused" if fused else "", "" if transform is None else " " + transform, worst_ll, n_tok, K,
             n_occ / max(n_tok, 1), worst_a_own, worst_a_spec, *at_a_spec))
    if kind == "bigram" or fused:
        print("draws: worst distance of a token's uniform from its slot's interval %.3g; %d of %d tokens drew an empty slot"
              % (worst_draw, n_drawn_empty, n_tok))
        assert worst_draw < 1e-4, worst_draw
    assert n_tok >= 4 * n_utt
    assert worst_ll < TOL, worst_ll
    assert worst_a_own < TOL, worst_a_own
    assert worst_a_spec < TOL, worst_a_spec


def test_fused_gibbs_step_gives_the_span_scores_and_boundaries_of_the_three_launches(gpu):
    _fused_against_three_launches(None)


@pytest.mark.parametrize("transform", ["shift16", "mfcc"])
def test_fused_gibbs_step_gives_the_span_scores_and_boundaries_of_the_three_launches_on_transformed_corpora(gpu, transform):
    _fused_against_three_launches(transform)


def _fused_against_three_launches(transform, anneal_temp=1.0, **kw):
    """segk_fbb_step_diag32 against segk_fbb_score_diag32 + segk_fbb_segment + segk_fbb_assign_diag32 from identical states,
    every block of a sweep: the span scores and the boundaries bit for bit (the same arithmetic and the same uniforms); the
    slots agree wherever the token's uniform does not fall within the last bits of a cumulative boundary (the token
    likelihoods of the two forms differ in their last float32 bits).  anneal_temp: the temperature of the boundary draws
    and of the slot draws; kw: segmenter keywords."""
    out = []
    for fused in (False, True):
        ref, spec, seg = _pair("diag", 64, 39, 100, "f32", transform=transform, **kw)
        sw = seg._get_sweeper()
        sw.enter(seg._dev_bounds)
        for b in range(sw.B):
            _one_step(sw, seg, b, fused=fused, anneal_temp_fb=anneal_temp, anneal_temp_am=anneal_temp)
        out.append((seg._df.score.cpu().numpy().copy(), seg._dev_bounds.cpu().numpy().copy(), sw.slot.cpu().numpy().copy(),
                    seg._df.out_logprob.cpu().numpy().copy(), seg._df.n_new.cpu().numpy().copy()))
    a, b_ = out
    assert np.array_equal(a[0], b_[0])
    assert np.array_equal(a[1], b_[1])
    assert np.array_equal(a[3], b_[3]) and np.array_equal(a[4], b_[4])
    both = (a[2] >= 0) | (b_[2] >= 0)
    assert np.mean(a[2][both] == b_[2][both]) > 0.98, np.mean(a[2][both] == b_[2][both])
    return a


@pytest.mark.parametrize("fused", [False, True], ids=["three_launches", "fused"])
def test_span_scores_and_token_likelihoods_on_settled_slots_of_thousands_of_items(gpu, fused):
    """The float32 Student-t term where its rounding is multiplied by a slot's count: the rows of the settled
    case st_D39_K8_n4096 of tests/fbgmm_items_f32.py -- two slots of 2 000 items each -- as utterances of one landmark through
    the unigram segmenter with score_precision="f32".  The span score of an utterance is then the log marginal of its row
    (segk_fbb_score_diag32, or the fused segk_fbb_step_diag32: the packed form of the term), its one token's likelihoods the
    row's (segk_fbb_assign_diag32 / the fused step).  Every Gibbs step on the settled start, f32.PROBES rows a step against
    the specification (tests/fbgmm_items.py: FbgmmItems.log_marg, loglik) on the statistics without the step's block.
    First the rows must show that they can tell the compensated term from the plain one: the emulation without the
    compensation misses the contract by 2 x or more on them, on the span scores and on the likelihoods."""
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import check, ptr
    from tests import fbgmm_items_f32 as f32
    torch = gpu
    name = "st_D39_K8_n4096"
    case = f32.SETTLED[name]
    K, N = case[3], case[6]
    spec = f32.spec_of(case)
    centre = f32.centre_of(spec.X)
    # first, before the device is asked anything: the specification on the rows every step will sample, and the inputs' condition
    steps = []
    plain_ll = plain_score = 0.0
    for b in range(spec.B):
        d = spec.derive(*spec.stats_excluding(b))
        rows = f32.probe_rows(f32.considered(spec, b, True))
        want, _, _, e_plain = f32.compare(spec, d, spec.X[rows], None, centre)
        want_score = np.array([spec.log_marg(d, spec.X[i]) for i in rows])
        assert f32.rel(f32.marginals(spec, d, want), want_score) <= 1e-12
        plain = f32.emulate_uncompensated(f32._Rows(spec, spec.X[rows]), d, range(len(rows)), centre)
        plain_ll = max(plain_ll, e_plain)
        plain_score = max(plain_score, f32.rel(f32.marginals(spec, d, plain), want_score))
        steps.append((d, rows, want, want_score))
    assert plain_score >= f32.DISCRIMINATES * f32.CONTRACT and plain_ll >= f32.DISCRIMINATES * f32.CONTRACT, (plain_score, plain_ll)
    seg = f32.segmenter_of(case)
    sw = seg._get_sweeper()
    assert sw.score_diag32 and seg._corpus.N_max == 1
    sw.enter(seg._dev_bounds)
    alpha = torch.full((N, 1), float("nan"), dtype=torch.float64, device="cuda")
    ll = torch.full((N, K), float("nan"), dtype=torch.float64, device="cuda")
    L, ctx = _abi.lib(), _abi.ctx()
    check(L.segk_fbb_set_probe(ctx, ptr(alpha), ptr(ll), K))
    try:
        for b in range(sw.B):
            _one_step(sw, seg, b, fused=fused)          # (no partial-sum refresh: every step on the settled start)
    finally:
        check(L.segk_fbb_set_probe(ctx, None, None, 0))
    ll, score, slots = ll.cpu().numpy(), seg._df.score.cpu().numpy(), sw.slot.cpu().numpy()
    assert np.array_equal(seg._df.new_tok.cpu().numpy().reshape(-1), np.arange(N))      # utterance i: row i, its one token
    worst_ll = worst_score = worst_empty = worst_draw = 0.0
    draws = skipped = 0
    for d, rows, want, want_score in steps:
        occ = d["active"]
        worst_ll = max(worst_ll, f32.rel(ll[rows][:, occ], want[:, occ]))
        worst_empty = max(worst_empty, f32.rel(ll[rows][:, ~occ], want[:, ~occ]))
        worst_score = max(worst_score, f32.rel(score[rows], want_score))
        # the slots: the fp64 function of the device's OWN likelihoods.  segk_fbb_assign_diag32 draws in fp64 (fbb_draw_row): the
        # slot is draw_chunked's wherever the uniform lies 1e-6 clear of an edge; the fused step forms its probabilities with
        # v_exp_f32 / v_log_f32: the uniform within 1e-4 of its slot's interval, as for the cases above
        pz = spec.prior_z(d, None, None, None)
        for i in rows:
            p, u = spec._probabilities(pz + ll[i], 1.0), nb.u01(spec.seed, 0, int(i), 1 + 0)
            k = int(slots[i])
            assert 0 <= k < K
            draws += 1
            if fused:
                cum = np.cumsum(p)
                worst_draw = max(worst_draw, (cum[k - 1] if k > 0 else 0.0) - u, u - cum[k])
            elif f32.margin(p, u) < f32.fi.DRAW_MARGIN:
                skipped += 1
            else:
                assert k == nb.draw_chunked(p, u), i
    print("%s as one-landmark utterances%s: span scores worst %.3g, token likelihoods %.3g (occupied), %.3g (empty) on %d "
          "probes a step; the emulation without the compensation: %.3g, %.3g; %d draws, %d skipped near an edge, worst distance "
          "from the slot's interval %.3g"
          % (name, " fused" if fused else "", worst_score, worst_ll, worst_empty, f32.PROBES, plain_score, plain_ll, draws, skipped,
             worst_draw))
    assert worst_score <= f32.CONTRACT and worst_ll <= f32.CONTRACT
    # (an empty slot: the row's prior predictive, fp64 in segk_fbb_assign_diag32; the fused step keeps every logit of a token as
    # a float32 in base 2 and its probe gives that back -- the contract there, as for the cases above)
    assert worst_empty <= (f32.CONTRACT if fused else 1e-9)
    assert skipped <= f32.NEAR_EDGE * draws and worst_draw < 1e-4


@pytest.mark.parametrize("fused", [False, True], ids=["three_launches", "fused"])
def test_span_scores_and_token_likelihoods_on_a_settled_multi_landmark_corpus(gpu, fused):
    """The same term at large counts on UTTERANCES OF EIGHT LANDMARKS (tests/am_batch_f32.py SETTLED_SEG: 800 utterances, a
    window of three, two slots of about 2 000 tokens): span rows of every duration in one score tile, three to eight tokens an
    utterance in the token kernels.  Every Gibbs step on the settled start (no partial-sum refresh), with
    segk_fbb_score_diag32 + segk_fbb_segment + segk_fbb_assign_diag32 or the fused segk_fbb_step_diag32:
      * first, before the device is asked anything, the probed span rows must tell the compensated term from the plain one;
      * the span scores of f32.PROBES span rows a block within the contract of nb.FbgmmBatch.log_marg;
      * the likelihoods of EVERY new token within the contract of loglik (empty slots at 1e-9; the fused step's float32
        logits: the contract), on tokens that can tell the two terms apart too;
      * every new token's slot the fp64 function of the device's own likelihoods: draw_chunked's wherever the uniform lies
        1e-6 clear of an edge (fbb_draw_row), the uniform within 1e-4 of the slot's interval for the fused step."""
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import check, ptr
    from tests import am_batch_f32 as a32
    f32 = a32.f32
    torch = gpu
    case = a32.SETTLED_SEG
    K = case[3]
    corpus, bounds, spec = a32.settled_seg_spec(case)
    centre = f32.centre_of(spec.X)
    steps = [a32.settled_seg_figures(spec, b, centre) for b in range(spec.B)]
    plain_score = min(st[5] for st in steps)
    assert plain_score >= f32.DISCRIMINATES * f32.CONTRACT, plain_score             # (the inputs: or the rows prove nothing)
    seg = a32.settled_seg_product(case, corpus, bounds, spec)
    assert np.array_equal(seg.acoustic_model.components.assignments, spec.slot)
    assert np.array_equal(seg.utterances.boundaries, spec.seg.utterances.boundaries)
    sw = seg._get_sweeper()
    n_utt, N_max = seg._corpus.n_utt, seg._corpus.N_max
    assert sw.score_diag32 and N_max == case[7]
    sw.enter(seg._dev_bounds)
    alpha = torch.full((n_utt, N_max), float("nan"), dtype=torch.float64, device="cuda")
    ll = torch.full((n_utt * N_max, K), float("nan"), dtype=torch.float64, device="cuda")
    L, ctx = _abi.lib(), _abi.ctx()
    check(L.segk_fbb_set_probe(ctx, ptr(alpha), ptr(ll), K))
    try:
        for b in range(sw.B):
            _one_step(sw, seg, b, fused=fused)
    finally:
        check(L.segk_fbb_set_probe(ctx, None, None, 0))
    ll, score, slots = ll.cpu().numpy().reshape(n_utt, N_max, K), seg._df.score.cpu().numpy(), sw.slot.cpu().numpy()
    new_tok, n_new = seg._df.new_tok.cpu().numpy(), seg._df.n_new.cpu().numpy()
    worst_score = worst_ll = worst_empty = worst_draw = plain_ll = 0.0
    n_tok = skipped = 0
    per_utt = set()
    for b, (d, rows, want, want_score, _, _) in enumerate(steps):
        occ = d["active"]
        worst_score = max(worst_score, f32.rel(score[rows], want_score))
        pz = spec.prior_z(d, None, None, None)
        toks = [(i, t) for s in range(spec.S) for i in range(*spec.ranges[s][b]) for t in range(n_new[i])]
        got = np.array([ll[i, t] for i, t in toks])
        assert np.isfinite(got).all()
        tok_rows = np.array([new_tok[i, t] for i, t in toks], np.int64)
        want_tok, e, _, e_plain = f32.compare(spec, d, spec.X[tok_rows], got, centre)
        worst_ll, plain_ll = max(worst_ll, e), max(plain_ll, e_plain)
        worst_empty = max(worst_empty, f32.rel(got[:, ~occ], want_tok[:, ~occ]))
        per_utt |= {int(n_new[i]) for s in range(spec.S) for i in range(*spec.ranges[s][b])}
        for j, (i, t) in enumerate(toks):
            p, u = spec._probabilities(pz + got[j], 1.0), nb.u01(spec.seed, 0, i, N_max + t)
            k = int(slots[tok_rows[j]])
            assert 0 <= k < K
            n_tok += 1
            if fused:
                cum = np.cumsum(p)
                worst_draw = max(worst_draw, (cum[k - 1] if k > 0 else 0.0) - u, u - cum[k])
            elif f32.margin(p, u) < f32.fi.DRAW_MARGIN:
                skipped += 1
            else:
                assert k == nb.draw_chunked(p, u), (b, i, t)
    print("settled multi-landmark corpus%s: span scores worst %.3g on %d probes a block (without the compensation %.3g); token "
          "likelihoods %.3g (occupied), %.3g (empty) over %d tokens, %s an utterance (without the compensation %.3g); %d draws "
          "skipped near an edge, worst distance from the slot's interval %.3g"
          % (" fused" if fused else "", worst_score, f32.PROBES, plain_score, worst_ll, worst_empty, n_tok, sorted(per_utt), plain_ll,
             skipped, worst_draw))
    assert plain_ll >= f32.DISCRIMINATES * f32.CONTRACT
    assert len(per_utt) >= 3 and max(per_utt) >= 4
    assert worst_score <= f32.CONTRACT and worst_ll <= f32.CONTRACT
    assert worst_empty <= (f32.CONTRACT if fused else 1e-9)
    assert skipped <= f32.NEAR_EDGE * n_tok and worst_draw < 1e-4

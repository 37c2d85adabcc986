"""
GPU tests of the batch sampler with full-covariance components (`UnigramAcousticWordseg(..., covariance_type="full")`
built with sync="sequential" and the batch arguments; batch sweeps through batch_sweep_async / gibbs_sample(sync="batch"))
against the NumPy specification tests/fullcov_batch.py.  tests/test_fullcov_batch_cpu.py shows that on these corpora every
draw is at least 1e-6 in probability clear of the cumulative edges and every Viterbi / MAP maximum 1e-6 clear of its
runner-up, so slots and boundaries must coincide; values are held to the 1e-9 of the fp64 path, statistics to 1e-13.
"""
import ctypes as C
import random

import numpy as np
import numpy.testing as npt
import pytest

from tests import fullcov_batch as fb
from tests import fullcov_wordseg as fw

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def pair(ci, K, B, S, map_batch=False, **kw):
    seg_spec, spec = fb.spec_of(ci, K, B, S, map_batch=map_batch)
    seg = fb.product_of(ci, K, B, S, **kw)
    assert np.array_equal(seg.acoustic_model.components.assignments, spec.slot)
    assert np.array_equal(seg.utterances.boundaries, seg_spec.utterances.boundaries)
    return spec, seg


def sweep_both(gpu, spec, seg, index, temp=1.0, anneal_am=False, what="", **spec_kw):
    """One sweep of both; everything the issue holds equal after a sweep."""
    spec.marg_log = []
    lp = spec.sweep(index, temp, anneal_am, **spec_kw)
    seg.batch_sweep_async(temp, anneal_am)
    gpu.cuda.synchronize()
    seg._df.check_status()
    sw = seg._get_sweeper()
    assert sw.sweep_index == index + 1
    u = spec.seg.utterances
    assert np.array_equal(sw.slot.cpu().numpy(), spec.slot), what
    assert np.array_equal(seg.utterances.boundaries, u.boundaries), what
    got_lp = seg._df.out_logprob.cpu().numpy()
    print("%s out_logprob %.3g" % (what, rel(got_lp, lp)))
    assert rel(got_lp, lp) <= RTOL, what
    rows = spec.scored_rows()
    assert len(rows) == len(spec.marg_log)
    got = seg._df.score.cpu().numpy()[rows]
    print("%s score %.3g over %d rows" % (what, rel(got, spec.marg_log), len(rows)))
    assert rel(got, spec.marg_log) <= RTOL, what
    worst = 0.0
    for s in range(spec.S):
        for b in range(spec.B):
            cnt, sx, sxx = sw.cell_partials(b, s)
            rc, rx, rxx = spec._partial(s, b)
            assert np.array_equal(cnt, rc), what
            worst = max(worst, rel(sx, rx), rel(sxx, rxx))
    print("%s partials %.3g" % (what, worst))
    assert worst <= 1e-13, what
    spec.marg_log = None
    return lp


@pytest.fixture(scope="module")
def finished(gpu):
    """name -> (spec, seg) after the sampled sweeps of test_sampled_sweeps (later tests go on from there)."""
    return {}


@pytest.mark.parametrize("name", list(fb.SAMPLED))
def test_sampled_sweeps(gpu, finished, name):
    ci, K, B, S, n, annealed = fb.SAMPLED[name]
    spec, seg = pair(ci, K, B, S)
    temps = fb.anneal_temps(n) if annealed else [1.0] * n
    probe = name in ("w4_D33", "w5_D64")
    if probe:
        from segmentalist_amd import _abi
        c = seg._df.corpus
        ll = gpu.zeros((c.n_utt * c.N_max, K), dtype=gpu.float64, device="cuda")
        _abi.check(_abi.lib().segk_fbb_set_probe(_abi.ctx(), None, _abi.ptr(ll), K))
    try:
        for s in range(n):
            spec.tok_log = [] if probe else None
            sweep_both(gpu, spec, seg, s, temps[s], annealed, "%s sweep %d" % (name, s))
            if probe:                   # the token likelihoods as the draws used them
                toks = spec.new_tokens()
                assert len(toks) == len(spec.tok_log)
                got = ll.cpu().numpy().reshape(c.n_utt, c.N_max, K)
                worst = max(rel(got[i, t], v) for (i, t, e), v in zip(toks, spec.tok_log))
                print("%s sweep %d token likelihoods %.3g over %d tokens" % (name, s, worst, len(toks)))
                assert worst <= RTOL
    finally:
        if probe:
            _abi.check(_abi.lib().segk_fbb_set_probe(_abi.ctx(), None, None, 0))
            spec.tok_log = None
    assert np.count_nonzero(spec.stats_excluding(-1)[0] == 0) >= 1
    finished[name] = (spec, seg)


@pytest.mark.parametrize("name", list(fb.MAP))
def test_map_sweeps(gpu, name):
    ci, K, B, S, n = fb.MAP[name]
    spec, seg = pair(ci, K, B, S, map_batch=True)
    seg.set_fb_type("viterbi")
    for s in range(n):
        sweep_both(gpu, spec, seg, s, what="%s MAP sweep %d" % (name, s))


def test_sampled_then_map_on_a_live_sweeper(gpu):
    ci, K, B, S, n_sampled, n_map = fb.MIXED["w1_mixed"]
    spec, seg = pair(ci, K, B, S, map_batch=True)
    for s in range(n_sampled):
        sweep_both(gpu, spec, seg, s, what="mixed sampled %d" % s, viterbi=False)
    seg.set_fb_type("viterbi")
    for s in range(n_sampled, n_sampled + n_map):
        sweep_both(gpu, spec, seg, s, what="mixed MAP %d" % s)


def spec_model(spec):
    """The serial specification's FBGMM of the canonical view of `spec` (fresh SpecComponents of those assignments)."""
    canon, K = spec.canonical()
    p = spec.seg.acoustic_model.components.prior
    am = fw.SpecWordsegFBGMM(spec.X, fw.SpecPrior(p.m_0, p.k_0, p.v_0, p.S_0), fw.ALPHA, spec.K_max, canon, lms=fw.LMS)
    assert am.components.K == K
    return canon, am


def same_view(seg, spec):
    canon, am = spec_model(spec)
    cd, cs = seg.acoustic_model.components, am.components
    assert cd.K == cs.K and np.array_equal(cd.assignments, canon)
    assert np.array_equal(cd.counts[:cs.K], cs.counts[:cs.K])
    for nm in ("m_N_numerators", "S_N_partials"):
        npt.assert_allclose(getattr(cd, nm)[:cs.K], getattr(cs, nm)[:cs.K], rtol=1e-13, atol=1e-300, err_msg=nm)
    npt.assert_allclose(cd.logdet_covars[:cs.K], cs.logdet_covars[:cs.K], rtol=RTOL, atol=1e-9)
    return am


def test_materialise_and_record(gpu, finished):
    if "w1" not in finished:
        test_sampled_sweeps(gpu, finished, "w1")
    spec, seg = finished["w1"]
    seg.materialise()
    same_view(seg, spec)
    n = seg._get_sweeper().sweep_index
    rec = seg.gibbs_sample(1, sync="batch")
    lp = spec.sweep(n)
    am = same_view(seg, spec)
    want = {"log_marg": am.log_marg(), "log_marg*length": float(np.sum(lp)), "log_prob_z": am.log_prob_z(),
            "log_prob_X_given_z": am.log_prob_X_given_z(), "anneal_temp": 1}
    for k, v in want.items():
        print("record %s: %.17g against %.17g" % (k, rec[k][0], v))
        assert abs(rec[k][0] - v) <= 1e-8 * max(1.0, abs(v)), k
    assert rec["components"][0] == am.components.K and rec["n_tokens"][0] == am.get_n_assigned()
    assert np.array_equal(seg._get_sweeper().slot.cpu().numpy(), spec.slot)


def test_serial_sweep_between_batch_sweeps(gpu):
    ci, K, B, S = 0, 8, 2, 2
    spec, seg = pair(ci, K, B, S)
    for s in range(2):
        sweep_both(gpu, spec, seg, s, what="before the serial sweep %d" % s)
    random.seed(5)
    seg.gibbs_sample(1)                                     # the serial chain from the materialised state; checks the status
    sw = seg._get_sweeper()
    assert not sw.in_batch_state
    # the specification rebuilt from that state
    u = spec.seg.utterances
    u.boundaries[:] = seg.utterances.boundaries
    spec.slot = np.array(seg.acoustic_model.components.assignments, dtype=spec.slot.dtype)
    spec.P = [[spec._partial(s, b) for b in range(spec.B)] for s in range(spec.S)]
    sweep_both(gpu, spec, seg, sw.sweep_index, what="after the serial sweep")
    assert sw.in_batch_state


def test_checkpoint_resumes_bit_for_bit(gpu):
    ci, K, B, S = 1, 10, 3, 4
    spec, seg = pair(ci, K, B, S)
    sweep_both(gpu, spec, seg, 0, what="checkpoint sweep 0")
    sd = seg.state_dict()
    sweep_both(gpu, spec, seg, 1, what="checkpoint sweep 1")
    fresh = fb.product_of(ci, K, B, S)
    fresh.load_state_dict(sd)
    fresh.batch_sweep_async()
    gpu.cuda.synchronize()
    fresh._df.check_status()
    assert np.array_equal(fresh._get_sweeper().slot.cpu().numpy(), seg._get_sweeper().slot.cpu().numpy())
    assert np.array_equal(fresh.utterances.boundaries, seg.utterances.boundaries)
    assert np.array_equal(fresh._df.out_logprob.cpu().numpy(), seg._df.out_logprob.cpu().numpy())


def test_refusals(gpu):
    from segmentalist_amd import _abi, bigram_acoustic_wordseg as baw, fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.niw import NIW
    ci, K, B, S = 0, 8, 2, 2
    seg = fb.product_of(ci, K, B, S, score_precision="f32")
    with pytest.raises(SegkError, match="f64"):
        seg.batch_sweep_async()
    prior, corpus = NIW(*fw.prior_params(ci)), fw.case_corpus(ci)
    with pytest.raises(NotImplementedError):
        baw.BigramAcousticWordseg(K, prior, (0.5, 1.0, 1.0), *corpus, covariance_type="full", n_slices_max=4)
    with pytest.raises(NotImplementedError, match="batch sampler"):
        uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, prior, *corpus, sync="batch", **fw.seg_kwargs(ci))
    # the library's entry points without a full-covariance form
    seg = fb.product_of(ci, K, B, S)
    seg.batch_sweep_async()
    gpu.cuda.synchronize()
    sw, df = seg._get_sweeper(), seg._df
    L, ctx, cp, fp, bp, st = sw._args()
    p = _abi.ptr
    nu, nr = sw._n_utts[0], sw._n_rows[0]
    calls = {
        "segk_fbb_score_diag32": lambda: L.segk_fbb_score_diag32(ctx, cp, fp, bp, 0, sw.s_n, 0, nr, p(df.score), st),
        "segk_fbb_score_f32": lambda: L.segk_fbb_score_f32(ctx, cp, fp, bp, p(df.new_tok), 1, p(df.score), st),
        "segk_fbb_assign_diag32": lambda: L.segk_fbb_assign_diag32(ctx, cp, fp, bp, 0, sw.s_n, 0, nu, 0, 1.0, p(df.new_tok),
                                                                   p(df.n_new), st),
        "segk_fbb_assign_map f32": lambda: L.segk_fbb_assign_map(ctx, cp, fp, bp, 0, sw.s_n, 0, nu, 0, p(df.new_tok),
                                                                 p(df.n_new), 1, st),
        "segk_fbb_step_diag32": lambda: L.segk_fbb_step_diag32(ctx, cp, fp, bp, 0, sw.s_n, 0, nu, 0, 0, 4, 0.0, 1.0, 1.0, 1.0,
                                                               p(df.score), p(seg._dev_bounds), p(df.new_tok), p(df.n_new),
                                                               p(df.out_logprob), p(df.status), st),
        "segk_fbb_token_scores": lambda: L.segk_fbb_token_scores(ctx, cp, fp, bp, p(df.new_tok), 1, None, 32, st),
        "segk_fbb_lm_apply": lambda: L.segk_fbb_lm_apply(ctx, cp, fp, bp, 0, 1, st),
        "segk_fbb_lm_fill": lambda: L.segk_fbb_lm_fill(ctx, cp, fp, bp, 0, sw.s_n, 0, nu, p(df.new_tok), p(df.n_new), st),
    }
    for name, call in calls.items():
        assert call() == _abi.SEGK_ERR_UNSUPPORTED, name
        assert "cov_type 2" in L.segk_last_error().decode(), name
    # a language model attached to the batch's copy of the model: refused by name, nothing launched
    f_lm = _abi.FbgmmDev.from_buffer_copy(sw.f)
    f_lm.lm_unigram = df.counts.data_ptr()
    assert L.segk_fbb_prepare(ctx, cp, C.byref(f_lm), bp, 0, st) == _abi.SEGK_ERR_UNSUPPORTED
    assert "cov_type 2" in L.segk_last_error().decode()
    gpu.cuda.synchronize()
    df.check_status()

"""
GPU tests of full-covariance components in the unigram segmenter's serial chain (`UnigramAcousticWordseg(...,
covariance_type="full")`, sync="sequential": segk_fullcov.hip behind the launches per utterance) against vectors
recorded from the reference (tests/golden/fullcov_wordseg.npz) and against the NumPy specification
(tests/fullcov_wordseg.py).  Values are held to the 1e-9 of the fp64 path; tests/test_fullcov_wordseg_cpu.py shows that
every stored draw is at least 1e-6 in probability clear of the cumulative edges and every Viterbi / MAP maximum 1e-6
clear of its runner-up, so the chains must coincide with the reference's draw for draw.
"""
import random

import numpy as np
import numpy.testing as npt
import pytest

from tests import fullcov_wordseg as fw

pytestmark = pytest.mark.gpu
RTOL = 1e-9
N_CASES = len(fw.CASES)
CASE_IDS = [fw.case_tag(ci) for ci in range(N_CASES)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def make_dev(ci, **over):
    from segmentalist_amd import fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd.niw import NIW
    kw = dict(fw.seg_kwargs(ci))
    kw.update(over)
    return uaw.UnigramAcousticWordseg(fbgmm.FBGMM, fw.ALPHA, fw.CASES[ci][2], NIW(*fw.prior_params(ci)), *fw.case_corpus(ci), **kw)


def make_spec(ci, **over):
    kw = dict(fw.seg_kwargs(ci))
    kw.update(over)
    return fw.SpecWordseg(fw.ALPHA, fw.CASES[ci][2], fw.SpecPrior(*fw.prior_params(ci)), *fw.case_corpus(ci), **kw)


def seeded(ci, n_labels):
    """Seed dictionaries for case ci: a boundary at every second landmark and at the last one, integer labels below
    `n_labels` -- a state with K = n_labels < K_max without a sweep."""
    landmarks = fw.case_corpus(ci)[3]
    rs = np.random.RandomState(7)
    sb = {u: sorted(set(lm[1::2] + [lm[-1]])) for u, lm in landmarks.items()}
    sa = {u: [int(k) for k in rs.randint(0, n_labels, len(sb[u]))] for u in sorted(sb)}
    return dict(seed_boundaries_dict=sb, seed_assignments_dict=sa)


def pair(ci, **over):
    """The specification's and the device's segmenter of case ci from the same seeds."""
    random.seed(1)
    np.random.seed(1)
    spec = make_spec(ci, **over)
    random.seed(1)
    np.random.seed(1)
    dev = make_dev(ci, **over)
    return spec, dev


def same_state(dev, spec, what=""):
    cd, cs = dev.acoustic_model.components, spec.acoustic_model.components
    assert np.array_equal(dev.utterances.boundaries, spec.utterances.boundaries), what
    assert np.array_equal(cd.assignments, cs.assignments), what
    assert cd.K == cs.K and np.array_equal(cd.counts, cs.counts), what
    for nm in ("m_N_numerators", "S_N_partials"):
        npt.assert_allclose(getattr(cd, nm), getattr(cs, nm), rtol=1e-13, atol=1e-300, err_msg=what + nm)
    npt.assert_allclose(cd.logdet_covars, cs.logdet_covars, rtol=RTOL, atol=1e-9, err_msg=what)


def same_as_golden(got, g, tag, sweeps):
    for s in sweeps:
        pre = "sweep%d_" % s
        for k in ("bounds", "assign", "counts", "K", "rec_components", "rec_n_tokens"):
            assert np.array_equal(got[pre + k], g[tag + pre + k]), pre + k
        for nm in ("m_N_numerators", "S_N_partials"):
            if pre + nm in got:
                npt.assert_allclose(got[pre + nm], g[tag + pre + nm], rtol=1e-13, atol=1e-300, err_msg=pre + nm)
        if pre + "logdet_covars" in got:
            npt.assert_allclose(got[pre + "logdet_covars"], g[tag + pre + "logdet_covars"], rtol=RTOL, atol=1e-9, err_msg=pre)
        for k in ("log_marg*length", "log_marg", "log_prob_z", "log_prob_X_given_z", "anneal_temp"):
            npt.assert_allclose(got[pre + "rec_" + k], g[tag + pre + "rec_" + k], rtol=1e-8, err_msg=pre + k)


@pytest.mark.parametrize("ci", range(N_CASES), ids=CASE_IDS)
def test_chain_vs_reference(gpu, golden, ci):
    """Four sweeps of gibbs_sample(1) through segmentalist_amd: boundaries and assignments draw for draw, counts equal,
    statistics at 1e-13, the record values at 1e-8, and the `random` stream left where the reference left it."""
    g, tag = golden("fullcov_wordseg"), fw.case_tag(ci) + "_"
    got = fw.run_case(ci, make_dev)
    assert np.array_equal(got["init_bounds"], g[tag + "init_bounds"])
    assert np.array_equal(got["init_assign"], g[tag + "init_assign"])
    same_as_golden(got, g, tag, range(fw.N_SWEEPS))
    assert float(got["random_after"]) == float(g[tag + "random_after"])


@pytest.mark.parametrize("ci", [0, 3, 4, 5, fw.LONG_CASE], ids=[CASE_IDS[i] for i in [0, 3, 4, 5, fw.LONG_CASE]])
def test_span_scores_vs_specification(gpu, ci):
    """get_vec_embed_log_probs of whole triangles (the lane-per-row kernel: every D bucket, both dtypes, chunks beyond 64
    rows with a ragged last one) on a state with K < K_max, with -1 ids and NaN durations, against the specification at
    1e-9; the same rows one at a time through log_marg_rows (the workgroup-per-row kernel) agree at 1e-9."""
    K_max = fw.CASES[ci][2]
    spec, dev = pair(ci, **seeded(ci, K_max - 2))
    assert dev.acoustic_model.components.K == K_max - 2
    same_state(dev, spec)
    u = spec.utterances
    lens = np.asarray(u.lengths)
    for i in sorted(set([int(np.argmax(lens)), int(np.argmin(lens)), 1])):
        N = u.lengths[i]
        tri = N * (N + 1) // 2
        ids = u.vec_ids[i, :tri]
        dur = np.array(u.durations[i, :tri], np.float64)
        dur[::5] = np.nan
        want = spec.get_vec_embed_log_probs(ids, dur)
        got = dev.get_vec_embed_log_probs(ids, dur)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        assert np.isneginf(got[ids == -1]).all() and np.isneginf(got[np.isnan(dur)]).all()
        fin = np.isfinite(want)
        npt.assert_allclose(got[fin], want[fin], rtol=RTOL)
    # the longest utterance's rows: the batched kernel against one row at a time
    i = int(np.argmax(lens))
    rows = u.vec_ids[i, :lens[i] * (lens[i] + 1) // 2]
    rows = rows[rows != -1]
    assert len(rows) >= 16
    df = dev._df
    step = max(1, len(rows) // 24)
    batched = df.log_marg_rows(rows)[::step]
    single = np.array([df.log_marg_rows([int(e)])[0] for e in rows[::step]])
    npt.assert_allclose(batched, single, rtol=RTOL)
    df.check_status()


def test_device_record_metrics_vs_host_expressions(gpu, monkeypatch):
    """segk_fbgmm_record_metrics for cov_type 2 against the host expressions the segmenter uses under
    SEGK_HOST_METRICS=1, at 1e-8: on the initial state and after a sweep that deletes components."""
    ci = 4
    random.seed(1)
    np.random.seed(1)
    seg = make_dev(ci)
    am = seg.acoustic_model
    for step in range(2):
        lpz, lpx, n_comp, n_tok = seg._df.record_metrics()
        npt.assert_allclose(lpz, am.log_prob_z(), rtol=1e-8)
        npt.assert_allclose(lpx, am.log_prob_X_given_z(), rtol=1e-8)
        assert n_comp == am.components.K and n_tok == am.get_n_assigned()
        if step == 0:
            monkeypatch.setenv("SEGK_HOST_METRICS", "1")
            rec = seg.gibbs_sample(2)
            monkeypatch.delenv("SEGK_HOST_METRICS")
            lpz, lpx, n_comp, n_tok = seg._df.record_metrics()
            npt.assert_allclose(rec["log_prob_z"][-1], lpz, rtol=1e-8)
            npt.assert_allclose(rec["log_prob_X_given_z"][-1], lpx, rtol=1e-8)
            npt.assert_allclose(rec["log_marg"][-1], lpz + lpx, rtol=1e-8)
            assert rec["components"][-1] == n_comp < fw.CASES[ci][2] and rec["n_tokens"][-1] == n_tok


def test_single_utterances_and_helpers_vs_specification(gpu):
    """gibbs_sample_i on single utterances (sampled, annealed with the components' draws annealed, then Viterbi after
    set_fb_type), get_log_margs_i and get_unsup_transcript_i, against the specification."""
    ci = 7
    spec, dev = pair(ci)
    same_state(dev, spec, "init")
    random.seed(11)
    for n, i in enumerate([3, 0, 17, 3, 9, 12]):
        if n == 4:
            spec.fb_type = "viterbi"
            dev.set_fb_type("viterbi")
        kw = dict(anneal_temp=1.5, anneal_gibbs_am=True) if n in (2, 3) else {}
        state = random.getstate()
        want = spec.gibbs_sample_i(i, **kw)
        after = random.getstate()
        random.setstate(state)
        got = dev.gibbs_sample_i(i, **kw)
        assert random.getstate() == after                   # the same uniforms, the stream left at the same place
        npt.assert_allclose(got, want, rtol=RTOL)
        same_state(dev, spec, "utterance %d" % i)
        assert [int(k) for k in dev.get_unsup_transcript_i(i)] == [int(k) for k in spec.get_unsup_transcript_i(i)]
    npt.assert_allclose(dev.get_log_margs_i(5), spec.get_log_margs_i(5), rtol=RTOL)
    same_state(dev, spec, "after get_log_margs_i")
    dev._df.check_status()


@pytest.mark.parametrize("init", ["one-by-one", "seeds"])
def test_initialisations_vs_specification(gpu, init):
    """The "one-by-one" initialisation (gibbs_sample_inside_loop_i per initial segment) and a seed-dictionary
    initialisation, then one sweep, against the specification."""
    ci = 0
    over = dict(init_am_assignments="one-by-one") if init == "one-by-one" else seeded(ci, 5)
    spec, dev = pair(ci, **over)
    same_state(dev, spec, "init")
    random.seed(5)
    want = spec.gibbs_sample(1)
    after = random.random()
    random.seed(5)
    got = dev.gibbs_sample(1)
    assert random.random() == after
    same_state(dev, spec, "sweep")
    for k in ("log_marg*length", "log_marg", "log_prob_z", "log_prob_X_given_z"):
        npt.assert_allclose(got[k][0], want[k][0], rtol=1e-8, err_msg=k)
    dev._df.check_status()


def test_am_iterations_and_step_schedule_vs_specification(gpu):
    """gibbs_sample with am_n_iter = 1 (FBGMM.gibbs_sample over the assigned rows between the sweeps) under a "step"
    schedule, against the specification."""
    ci = 0
    spec, dev = pair(ci)
    kw = dict(am_n_iter=1, anneal_schedule="step", anneal_start_temp_inv=0.5, anneal_end_temp_inv=1.0, n_anneal_steps=2)
    random.seed(9)
    want = spec.gibbs_sample(2, **kw)
    after = random.random()
    random.seed(9)
    got = dev.gibbs_sample(2, **kw)
    assert random.random() == after
    same_state(dev, spec)
    assert got["anneal_temp"] == want["anneal_temp"] and got["components"] == want["components"]
    for k in ("log_marg*length", "log_marg", "log_prob_z", "log_prob_X_given_z"):
        npt.assert_allclose(got[k], want[k], rtol=1e-8, err_msg=k)


def test_checkpoint_round_trip_in_mid_chain(gpu, golden):
    """state_dict after two sweeps, loaded into a fresh segmenter built from other seeds: sweeps three and four end in the
    golden state."""
    ci = 1
    g, tag = golden("fullcov_wordseg"), fw.case_tag(ci) + "_"
    random.seed(1)
    np.random.seed(1)
    seg = make_dev(ci)
    for kw in fw.sweep_kwargs(ci)[:2]:
        seg.gibbs_sample(1, **kw)
    sd = seg.state_dict()
    del seg
    random.seed(99)
    np.random.seed(99)
    seg = make_dev(ci)
    seg.load_state_dict(sd)
    c = seg.acoustic_model.components
    got = {}
    for s in (2, 3):
        rec = seg.gibbs_sample(1, **fw.sweep_kwargs(ci)[s])
        pre = "sweep%d_" % s
        got.update({pre + "bounds": seg.utterances.boundaries.copy(), pre + "assign": c.assignments, pre + "counts": c.counts,
                    pre + "K": np.array(c.K)})
        for nm in fw.STAT_NAMES:
            got[pre + nm] = getattr(c, nm)
        for k in fw.REC_KEYS:
            got[pre + "rec_" + k] = np.array(rec[k][0])
    same_as_golden(got, g, tag, (2, 3))
    assert random.random() == float(g[tag + "random_after"])


def test_what_still_refuses(gpu):
    """sync="batch" names the batch sampler; the bigram classes keep refusing; so do the library's entry points without a
    full-covariance form."""
    import ctypes as C
    from segmentalist_amd import _abi, bigram_acoustic_wordseg as baw, fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.bigram_fbgmm import BigramFBGMM
    from segmentalist_amd.niw import NIW
    ci = 0
    K, prior, corpus = fw.CASES[ci][2], NIW(*fw.prior_params(ci)), fw.case_corpus(ci)
    with pytest.raises(NotImplementedError, match="batch sampler"):
        uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, prior, *corpus, sync="batch", **fw.seg_kwargs(ci))
    kw = dict(fw.seg_kwargs(ci))
    del kw["beta_sent_boundary"]                            # the default, 2.0: calc_p_continue supports -1 only
    with pytest.raises(NotImplementedError, match="beta_sent_boundary"):
        uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, prior, *corpus, **kw)
    with pytest.raises(NotImplementedError):
        baw.BigramAcousticWordseg(K, prior, (0.5, 1.0, 1.0), *corpus, covariance_type="full", n_slices_max=4)
    X = np.random.RandomState(0).randn(20, 5).astype(np.float32)
    with pytest.raises(NotImplementedError):
        BigramFBGMM(X, prior, 3, covariance_type="full")
    # a stand-alone FBGMM has no utterances: op 0 and the device record stay the segmenter's
    alone = fbgmm.FBGMM(X, prior, 1.0, 3).components.dev
    with pytest.raises(SegkError, match="cov_type 2"):
        alone.update(0, utt=0)
    with pytest.raises(SegkError, match="cov_type 2"):
        alone.record_metrics()
    random.seed(1)
    np.random.seed(1)
    seg = make_dev(ci)
    df = seg._df
    L, ctx = _abi.lib(), _abi.ctx()
    for op in (5, 6):
        assert L.segk_fbgmm_update(ctx, df._cp(), C.byref(df.f), op, 0, 0, 0, _abi.ptr(seg._dev_bounds), _abi.stream()) == \
            _abi.SEGK_ERR_UNSUPPORTED
    with pytest.raises(SegkError, match="cov_type 2"):
        df.record_metrics(urn=True, urn_a=1.0)
    assert df.sequential_sweep(seg._dev_bounds, [0, 1], seg._row_start, False, 0, 4, 0.0, 1.0, 0.0, 1.0, 1.0) is False
    assert "cov_type 2" in L.segk_last_error().decode()

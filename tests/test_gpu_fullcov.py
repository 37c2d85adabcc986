"""
GPU tests of the full-covariance FBGMM (covariance_type="full": segmentalist_amd.gaussian_components on
segk_fullcov.hip) against vectors recorded from the reference (tests/golden/fullcov.npz) and against the NumPy
specification (tests/fullcov.py).  Values are held to the 1e-9 of the fp64 path (tests/test_gpu_fbgmm.py);
tests/test_fullcov_cpu.py shows that every stored draw is at least 1e-6 in probability clear of the cumulative
edges, so the sampled components must coincide with the reference's draw for draw.
"""
import numpy as np
import numpy.testing as npt
import pytest

from tests import fullcov

pytestmark = pytest.mark.gpu
RTOL = 1e-9
CASE_IDS = [fullcov.case_tag(ci) for ci in range(len(fullcov.CASES))]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


@pytest.fixture(scope="module")
def device_runs(gpu):
    """Every case walked once through the device classes (tests/fullcov.py run_case), on demand; shared by the tests."""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.niw import NIW
    runs = {}

    def get(ci):
        if ci not in runs:
            runs[ci] = fullcov.run_case(ci, FBGMM, NIW, covariance_type="full")
        return runs[ci]
    return get


def _stats_equal(got, g, tag, pre):
    assert int(got[pre + "_K"]) == int(g[tag + pre + "_K"]), pre
    assert np.array_equal(got[pre + "_counts"], g[tag + pre + "_counts"]), pre
    assert np.array_equal(got[pre + "_assign"], g[tag + pre + "_assign"]), pre
    for nm in ("m_N_numerators", "S_N_partials"):
        npt.assert_allclose(got[pre + "_" + nm], g[tag + pre + "_" + nm], rtol=1e-13, atol=1e-300, err_msg=pre + nm)
    npt.assert_allclose(got[pre + "_logdet_covars"], g[tag + pre + "_logdet_covars"], rtol=RTOL, atol=1e-9, err_msg=pre)


@pytest.mark.parametrize("ci", range(len(fullcov.CASES)), ids=CASE_IDS)
def test_construction_vs_reference(device_runs, golden, ci):
    """K, counts, statistics at 1e-13 (the float32 rounding of the cached outer products included), logdet_covars and
    inv_covars at the value tolerance."""
    g, tag, got = golden("fullcov"), fullcov.case_tag(ci) + "_", device_runs(ci)
    _stats_equal(got, g, tag, "init")
    if fullcov.CASES[ci][0] <= fullcov.INV_D_MAX:
        want = g[tag + "init_inv_covars"]
        npt.assert_allclose(got["init_inv_covars"], want, rtol=RTOL, atol=RTOL * np.abs(want).max())


@pytest.mark.parametrize("ci", range(len(fullcov.CASES)), ids=CASE_IDS)
def test_predictive_values_vs_reference(device_runs, golden, ci):
    g, tag, got = golden("fullcov"), fullcov.case_tag(ci) + "_", device_runs(ci)
    for k in ("log_post_pred", "log_prior", "log_marg_i"):
        npt.assert_allclose(got[k], g[tag + k], rtol=RTOL, err_msg=k)
    npt.assert_allclose(got["log_marg"], g[tag + "log_marg"], rtol=1e-10)
    npt.assert_allclose(got["components_log_marg"], g[tag + "components_log_marg"], rtol=1e-10)


@pytest.mark.parametrize("ci", range(len(fullcov.CASES)), ids=CASE_IDS)
def test_single_item_draws_and_map_vs_reference(device_runs, golden, ci):
    """gibbs_sample_inside_loop_i with the reference's uniforms (the same `random` stream) and map_assign_i: the same
    components, then the same statistics."""
    g, tag, got = golden("fullcov"), fullcov.case_tag(ci) + "_", device_runs(ci)
    assert np.array_equal(got["draw_k"], g[tag + "draw_k"])
    _stats_equal(got, g, tag, "draw")
    assert np.array_equal(got["map_k"], g[tag + "map_k"])
    _stats_equal(got, g, tag, "map")


@pytest.mark.parametrize("ci", range(len(fullcov.CASES)), ids=CASE_IDS)
def test_gibbs_sample_vs_reference(device_runs, golden, ci):
    """fbgmm.py:288-420 through segk_fbgmm_gibbs_items: assignments, K, counts and statistics after every sweep, the
    record values at 1e-8, and the `random` stream left where the reference left it."""
    g, tag, got = golden("fullcov"), fullcov.case_tag(ci) + "_", device_runs(ci)
    for s in range(fullcov.N_SWEEPS[ci]):
        pre = "sweep%d" % s
        _stats_equal(got, g, tag, pre)
        assert int(got[pre + "_rec_components"]) == int(g[tag + pre + "_rec_components"])
        for k in ("log_marg", "log_prob_z", "log_prob_X_given_z", "anneal_temp"):
            npt.assert_allclose(got[pre + "_rec_" + k], g[tag + pre + "_rec_" + k], rtol=1e-8, err_msg=pre + k)
    assert float(got["random_after"]) == float(g[tag + "random_after"])


def test_cached_log_prior_and_map(gpu):
    """cached_log_prior is log_prior of every row; map(k) against the specification."""
    from segmentalist_amd.gaussian_components import GaussianComponents
    from segmentalist_amd.niw import NIW
    ci = 1
    X, a = fullcov.case_data(ci), fullcov.initial_assignments(ci)
    dev = GaussianComponents(X, NIW(*fullcov.prior_params(ci)), a.copy(), K_max=fullcov.CASES[ci][1])
    ref = fullcov.SpecComponents(X, fullcov.SpecPrior(*fullcov.prior_params(ci)), a.copy(), K_max=fullcov.CASES[ci][1])
    npt.assert_allclose(dev.cached_log_prior, ref.cached_log_prior, rtol=RTOL)
    npt.assert_allclose(dev.log_prior(3), dev.cached_log_prior[3], rtol=1e-14)
    npt.assert_allclose(dev.log_post_pred_k(3, 1), ref.log_post_pred_k(3, 1), rtol=RTOL)
    k_N = ref.prior.k_0 + ref.counts[1]
    m_N = ref.m_N_numerators[1] / k_N
    sigma = (ref.S_N_partials[1] - k_N * np.outer(m_N, m_N)) / (ref.prior.v_0 + ref.counts[1] + ref.D + 2)
    got_m, got_s = dev.map(1)
    npt.assert_allclose(got_m, m_N, rtol=1e-12)
    npt.assert_allclose(got_s, sigma, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_component_mutators_vs_specification(gpu, dtype):
    """60 random add_item / del_item steps (components opened and, by swap-last compaction, deleted) and a
    del_component against the specification."""
    from segmentalist_amd.gaussian_components import GaussianComponents
    from segmentalist_amd.niw import NIW
    rs = np.random.RandomState(3)
    D, K_max = 6, 7
    X = (rs.randn(50, D) + 1.0).astype(dtype)
    assign = rs.randint(0, 4, 50)
    assign[rs.rand(50) < 0.5] = -1
    assign = np.array([{k: j for j, k in enumerate(sorted(set(assign) - {-1}))}.get(a, -1) for a in assign])
    pp = (0.5 * np.ones(D), 0.05, D + 3, 0.1 * (D + 3) * np.eye(D))
    ref = fullcov.SpecComponents(X, fullcov.SpecPrior(*pp), assign.copy(), K_max=K_max)
    dev = GaussianComponents(X, NIW(*pp), assign.copy(), K_max=K_max)

    def same():
        assert dev.K == ref.K
        assert np.array_equal(dev.counts, ref.counts)
        assert np.array_equal(dev.assignments, ref.assignments)
        for nm in ("m_N_numerators", "S_N_partials"):
            npt.assert_allclose(getattr(dev, nm), getattr(ref, nm), rtol=1e-12, atol=1e-300, err_msg=nm)
        npt.assert_allclose(dev.logdet_covars, ref.logdet_covars, rtol=RTOL, atol=1e-9)
        npt.assert_allclose(dev.chol_covars, ref.chol, rtol=RTOL, atol=1e-9)
        npt.assert_allclose(dev.inv_covars, ref.inv_covars, rtol=RTOL, atol=RTOL * np.abs(ref.inv_covars).max())
    same()
    free = list(np.where(ref.assignments == -1)[0])
    used = list(np.where(ref.assignments != -1)[0])
    for step in range(60):
        if rs.rand() < 0.5 and free:
            i = free.pop(rs.randint(len(free)))
            k = int(rs.randint(0, ref.K + 1)) if ref.K < K_max else int(rs.randint(0, ref.K))
            ref.add_item(i, k)
            dev.add_item(i, k)
            used.append(i)
        elif used:
            i = used.pop(rs.randint(len(used)))
            ref.del_item(i)
            dev.del_item(i)
            free.append(i)
        same()
    k = ref.K - 2
    ref.assignments[ref.assignments == k] = -1        # (del_component leaves the rows of k to the caller)
    ref.del_component(k)
    for i in np.where(dev.assignments == k)[0]:
        dev.dev.assignments[int(i)] = -1
    dev.del_component(k)
    same()
    dev.dev.check_status()


def test_refusals(gpu):
    """D = 65, a NIW prior with a vector S_0, the segmenters and BigramFBGMM with "full", rand_k, and the library's
    entry points that have no full-covariance form."""
    import ctypes as C
    from segmentalist_amd import _abi, bigram_acoustic_wordseg as baw, fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.bigram_fbgmm import BigramFBGMM
    from segmentalist_amd.gaussian_components import GaussianComponents
    from segmentalist_amd.niw import NIW
    from tests.golden import cases
    rs = np.random.RandomState(0)
    X65 = rs.randn(20, 65).astype(np.float32)
    with pytest.raises(SegkError, match="D <= 64"):
        fbgmm.FBGMM(X65, NIW(np.zeros(65), 0.05, 68, np.eye(65)), 1.0, 3)
    X = rs.randn(20, 4).astype(np.float32)
    vec_prior = NIW(np.zeros(4), 0.05, 7, np.ones(4))
    with pytest.raises(NotImplementedError, match="S_0"):
        fbgmm.FBGMM(X, vec_prior, 1.0, 3)
    with pytest.raises(AssertionError):
        GaussianComponents(X, vec_prior, np.zeros(20, np.int64), K_max=3)
    full_prior = NIW(np.zeros(4), 0.05, 7, np.eye(4))
    with pytest.raises(NotImplementedError):
        BigramFBGMM(X, full_prior, 3, covariance_type="full")
    corpus = cases.chain_corpus(6, 6, 5, 12, True, 0, 4, "float32")
    p6 = NIW(np.zeros(6), 0.05, 9, np.eye(6))
    with pytest.raises(NotImplementedError):
        uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, 5, p6, *corpus, covariance_type="full", n_slices_max=4)
    with pytest.raises(NotImplementedError):
        baw.BigramAcousticWordseg(5, p6, (0.5, 1.0, 1.0), *corpus, covariance_type="full", n_slices_max=4)
    fm = fbgmm.FBGMM(X, full_prior, 1.0, 3)
    with pytest.raises(NotImplementedError):
        fm.components.rand_k(0)
    df = fm.components.dev
    L, ctx = _abi.lib(), _abi.ctx()
    with pytest.raises(SegkError, match="cov_type 2"):
        df.record_metrics()
    with pytest.raises(SegkError, match="cov_type 2"):
        df.update(0, utt=0)
    rc = L.segk_fbgmm_update(ctx, df._cp(), C.byref(df.f), 5, 0, 0, 0, None, _abi.stream())
    assert rc == _abi.SEGK_ERR_UNSUPPORTED
    with pytest.raises(SegkError, match="component out of range"):
        fm.components.add_item(0, 3)

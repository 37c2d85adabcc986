"""
The NumPy specification of the full-covariance FBGMM (tests/fullcov.py) against the vectors recorded
from the reference (tests/golden/fullcov.npz, made by tests/golden/make_golden_fullcov.py), and the
conditions on those vectors that the GPU test (tests/test_gpu_fullcov.py) relies on.  No GPU.
"""
import os

import numpy as np
import numpy.testing as npt
import pytest

from tests import fullcov

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullcov.npz")
CASE_IDS = [fullcov.case_tag(ci) for ci in range(len(fullcov.CASES))]

EXACT = ("_K", "_counts", "_assign", "draw_k", "map_k", "_rec_components")
STATS = ("_m_N_numerators", "_S_N_partials")


@pytest.fixture(scope="module")
def spec_runs():
    """Every case walked once through the specification; shared by the tests below."""
    runs = {}
    for ci in range(len(fullcov.CASES)):
        fms = []

        def make(*a, **k):
            fms.append(fullcov.SpecFBGMM(*a, **k))
            return fms[0]

        def take():
            got = list(fms[0].margins)
            del fms[0].margins[:]
            return got
        runs[ci] = fullcov.run_case(ci, make, fullcov.SpecPrior, take)
    return runs


@pytest.mark.parametrize("ci", range(len(fullcov.CASES)), ids=CASE_IDS)
def test_specification_reproduces_the_reference(golden, spec_runs, ci):
    """Statistics at 1e-13, predictive values at 1e-12, assignments and K equal, over the whole walk: construction,
    single-item draws, MAP assignments, sweeps with components emptying (swap-last compaction)."""
    g = golden("fullcov")
    tag = fullcov.case_tag(ci) + "_"
    got = spec_runs[ci]
    keys = [k[len(tag):] for k in g.files if k.startswith(tag)]
    assert sorted(keys) == sorted(got.keys())
    for k in keys:
        want = g[tag + k]
        if k.endswith(EXACT):
            assert np.array_equal(got[k], want), k
        elif k.endswith(STATS):
            npt.assert_allclose(got[k], want, rtol=1e-13, atol=1e-300, err_msg=k)
        elif k.endswith("_margin"):
            # the same draws: the margins are differences of the probabilities themselves
            npt.assert_allclose(got[k], want, rtol=1e-6, atol=1e-10, err_msg=k)
        elif k == "random_after":
            assert got[k] == want
        elif k.endswith("_inv_covars"):
            npt.assert_allclose(got[k], want, rtol=1e-9, atol=1e-9, err_msg=k)
        elif "_rec_" in k:
            npt.assert_allclose(got[k], want, rtol=1e-10, err_msg=k)
        else:           # logdet_covars, log_post_pred, log_prior, log_marg_i, log_marg
            npt.assert_allclose(got[k], want, rtol=1e-12, atol=1e-12, err_msg=k)


@pytest.mark.parametrize("ci", range(len(fullcov.CASES)), ids=CASE_IDS)
def test_every_stored_draw_is_clear_of_the_cumulative_edges(golden, ci):
    """A condition on the inputs: every uniform of every stored draw lies at least 1e-6 in probability from the nearest
    edge of the cumulative distribution.  It is what entitles the GPU test to demand identical assignments of a path whose
    values are held to 1e-9."""
    g = golden("fullcov")
    tag = fullcov.case_tag(ci) + "_"
    keys = [k for k in g.files if k.startswith(tag) and k.endswith("_margin")]
    assert len(keys) == 1 + fullcov.N_SWEEPS[ci]
    for k in keys:
        assert g[k].size > 0 and g[k].min() >= 1e-6, (k, g[k].min())


@pytest.mark.parametrize("ci", range(len(fullcov.CASES)), ids=CASE_IDS)
def test_cases_cover_compaction_and_do_not_collapse(golden, ci):
    """Each chain deletes at least one component (swap-last compaction runs) and never falls below two."""
    g = golden("fullcov")
    tag = fullcov.case_tag(ci) + "_"
    comps = [int(g[tag + "sweep%d_rec_components" % s]) for s in range(fullcov.N_SWEEPS[ci])]
    assert min(comps) >= 2
    assert min(comps) < int(g[tag + "init_K"])


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 1000 * 1000

"""
The NumPy specification of the full-covariance unigram segmenter (tests/fullcov_wordseg.py) against the vectors
recorded from the reference (tests/golden/fullcov_wordseg.npz, made by tests/golden/make_golden_fullcov_wordseg.py),
and the conditions on those vectors that the GPU test (tests/test_gpu_fullcov_wordseg.py) relies on.  No GPU.
"""
import os

import numpy as np
import numpy.testing as npt
import pytest

from tests import fullcov_wordseg as fw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullcov_wordseg.npz")
N_CASES = len(fw.CASES)
CASE_IDS = [fw.case_tag(ci) for ci in range(N_CASES)]

EXACT = ("_bounds", "_assign", "_counts", "_K", "_rec_components", "_rec_n_tokens", "_uniforms", "random_after")
STATS = ("_m_N_numerators", "_S_N_partials")


@pytest.fixture(scope="module")
def spec_runs():
    """Every case walked once through the specification, with its margins and gaps; shared by the tests below."""
    runs = {}
    for ci in range(N_CASES):
        segs = []

        def make(ci):
            segs.append(fw.make_spec(ci))
            return segs[0]

        def take():
            am = segs[0].acoustic_model
            got = list(am.margins), list(segs[0].boundary_margins)
            del am.margins[:], segs[0].boundary_margins[:]
            return got
        res = fw.run_case(ci, make, take, log_uniforms=True)
        runs[ci] = (res, np.array(segs[0].dp_gaps), np.array(segs[0].acoustic_model.map_gaps))
    return runs


@pytest.mark.parametrize("ci", range(N_CASES), ids=CASE_IDS)
def test_specification_reproduces_the_reference(golden, spec_runs, ci):
    """Boundaries, assignments, counts and the uniforms consumed equal; statistics at 1e-13; values and records at 1e-12."""
    g = golden("fullcov_wordseg")
    tag = fw.case_tag(ci) + "_"
    got = spec_runs[ci][0]
    keys = [k[len(tag):] for k in g.files if k.startswith(tag)]
    assert sorted(keys) == sorted(got.keys())
    for k in keys:
        want = g[tag + k]
        if k.endswith(EXACT):
            assert np.array_equal(got[k], want), k
        elif k.endswith(STATS):
            npt.assert_allclose(got[k], want, rtol=1e-13, atol=1e-300, err_msg=k)
        elif "_margin_" in k:
            # the same draws: the margins are differences of the probabilities themselves
            npt.assert_allclose(got[k], want, rtol=1e-6, atol=1e-10, err_msg=k)
        else:           # logdet_covars and the record values
            npt.assert_allclose(got[k], want, rtol=1e-12, atol=1e-12, err_msg=k)


@pytest.mark.parametrize("ci", range(N_CASES), ids=CASE_IDS)
def test_every_stored_draw_is_clear_of_the_cumulative_edges(golden, ci):
    """A condition on the inputs: every uniform of every stored boundary and component draw lies at least 1e-6 in
    probability from the nearest edge of its cumulative distribution.  It is what entitles the GPU test to demand the
    reference's chain draw for draw of a path whose values are held to 1e-9."""
    g = golden("fullcov_wordseg")
    tag = fw.case_tag(ci) + "_"
    keys = [k for k in g.files if k.startswith(tag) and "_margin_" in k]
    assert len(keys) == 2 * fw.N_SWEEPS
    n = 0
    for k in keys:
        n += g[k].size
        if g[k].size:
            assert g[k].min() >= 1e-6, (k, g[k].min())
    assert (n == 0) == (fw.CASES[ci][6] == "viterbi")


@pytest.mark.parametrize("ci", range(N_CASES), ids=CASE_IDS)
def test_cases_cover_compaction_and_do_not_collapse(golden, ci):
    """Each chain deletes at least one component (swap-last compaction runs, inside an utterance's delete or inside its
    assignment) and never falls below two."""
    g = golden("fullcov_wordseg")
    tag = fw.case_tag(ci) + "_"
    comps = [int(g[tag + "sweep%d_rec_components" % s]) for s in range(fw.N_SWEEPS)]
    assert min(comps) >= 2
    assert min(comps) < int(g[tag + "init_K"])


@pytest.mark.parametrize("ci", [ci for ci in range(N_CASES) if fw.CASES[ci][6] == "viterbi"],
                         ids=[t for ci, t in enumerate(CASE_IDS) if fw.CASES[ci][6] == "viterbi"])
def test_viterbi_and_map_gaps_are_clear(spec_runs, ci):
    """Every DP maximum (forward pass and backtrack) and every MAP slot of the Viterbi chains has its best alternative at
    least 1e-6 (log domain) above the second best."""
    _, dp, mp = spec_runs[ci]
    assert dp.size > 0 and mp.size > 0
    print("least DP gap %.3e over %d maxima, least MAP gap %.3e over %d slots" % (dp.min(), dp.size, mp.min(), mp.size))
    assert dp.min() >= 1e-6
    assert mp.min() >= 1e-6


def test_cases_cover_the_kernel_paths():
    """Every D bucket of the span-score kernel with its padding, both dtypes, triangles of more than 64 rows."""
    Ds = set(c[1] for c in fw.CASES)
    assert {5, 16, 33, 64} <= Ds
    assert {np.float32, np.float64} == set(c[5] for c in fw.CASES)
    assert fw.CASES[fw.LONG_CASE][7][0] > 12 and fw.CASES[fw.LONG_CASE][7][1] > 64


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 1000 * 1000

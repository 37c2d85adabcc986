"""
tests/label_blocks.py (the reference of tests/test_gpu_label_blocks.py) held against the oracle on small cases, and the
cases of the GPU test held to what they are named for: every label vector is generated here and must have the blocks,
the straddling / absent components, the list lengths and the holes of its row of the table; every fixed-variance float32
case must be sensitive, by more than ten times the GPU test's tolerance, to the order in which a component's rows are
taken.  The diagonal and full-covariance metrics are functions of the fp64 statistics alone -- an order error there moves
the last bits only and is caught by the bit-for-bit comparison of the statistics, not by the record value.
"""
import numpy as np
import numpy.testing as npt
import pytest

from oracle import np_oracle as no
from tests import fullcov
from tests import label_blocks as lb

RTOL_RECORD = 1e-8          # the GPU test's tolerance for record values
F32, F64 = np.float32, np.float64


def _small(cov, dtype, holes, seed=5):
    """300 rows, D = 4, a bank of 7 with 6 active components, through the mfcc transform."""
    from tests import affine
    n, D, K_max = 300, 4, 7
    rs = np.random.RandomState(seed)
    X = (lb.SPREAD * (1.5 * rs.randn(5, D)[rs.randint(0, 5, n)] + 0.3 * rs.randn(n, D))).astype(dtype)
    s, c = affine.params("mfcc", D)
    X = affine.rows(X, s, c)
    labels = rs.randint(0, 6, n).astype(np.int64)
    labels[:6] = np.arange(6)
    if holes:
        labels[6:][rs.rand(n - 6) < 1. / 3.] = -1
    return X, labels, K_max, lb.case_prior(cov, D, s, c)


@pytest.mark.parametrize("holes", [False, True], ids=["all_assigned", "holes"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("cov", ["fixed", "diag", "full"])
def test_reference_equals_the_oracle_on_small_cases(cov, dtype, holes):
    """Statistics bit for bit (np.cumsum performs the additions of the oracle's add_item loop), derived arrays at 1e-13,
    log_marg() and log_prob_z() at 1e-12."""
    X, labels, K_max, prior = _small(cov, dtype, holes)
    st = lb.init_stats(X, labels, K_max, cov, prior)
    if cov == "full":
        fm = fullcov.SpecFBGMM(X, fullcov.SpecPrior(*prior), lb.ALPHA, K_max, labels.copy())
        names = ("m_N_numerators", "S_N_partials", None, "logdet_covars")
    else:
        pr = no.FixedVarPrior(*prior) if cov == "fixed" else no.NIW(*prior)
        fm = no.FBGMM(X, pr, lb.ALPHA, K_max, labels.copy(), covariance_type=cov)
        names = (("mu_N_numerators", "precision_Ns", "precision_preds", "log_prod_precision_preds") if cov == "fixed" else
                 ("m_N_numerators", "S_N_partials", "inv_vars", "log_prod_vars"))
    c = fm.components
    assert st["K"] == c.K == 6
    assert np.array_equal(st["counts"], c.counts) and np.array_equal(st["assignments"], c.assignments)
    assert np.array_equal(st["a"], getattr(c, names[0])), names[0]
    assert np.array_equal(st["b"], getattr(c, names[1])), names[1]
    if names[2]:
        npt.assert_allclose(st["derived"], getattr(c, names[2]), rtol=1e-13, atol=0)
    npt.assert_allclose(st["log_prod"], getattr(c, names[3]), rtol=1e-13 if cov != "full" else 1e-12, atol=0)
    npt.assert_allclose(lb.log_prob_X_given_z(X, cov, prior, st), c.log_marg(), rtol=1e-12)
    npt.assert_allclose(lb.log_prob_z_fbgmm(st["counts"], lb.ALPHA, K_max), fm.log_prob_z(), rtol=1e-12)
    hz, hx = lb.metrics_hi(X, labels, K_max, cov, prior, lb.ALPHA)
    # the longdouble evaluation is the same function (float32 data: the reference's float32 squares and sums stand between)
    if dtype is F64:
        npt.assert_allclose(float(hx), c.log_marg(), rtol=1e-9)
    npt.assert_allclose(float(hz), fm.log_prob_z(), rtol=1e-12)


def test_urn_form_equals_the_loop_and_the_closed_form():
    """bigram_acoustic_wordseg.py:287-305 over the assigned rows in row order (the loop, as the oracle runs it over its
    transcripts) against the vectorised urn, which takes the rows component by component, and against the form the
    kernel evaluates: sum_k [lgamma(n_k + a/K) - lgamma(a/K)] - [lgamma(T + a) - lgamma(a)]."""
    from scipy.special import gammaln
    _, labels, K_max, _ = _small("fixed", F32, True)
    for a in lb.URN_A:
        lm = no.BigramSmoothLM(0.1, a, 1.0, K_max)
        lp = 0.
        for k in labels[labels >= 0]:
            lp += np.log(lm.prob_i(k))
            lm.unigram_counts[k] += 1
        cnt = np.bincount(labels[labels >= 0], minlength=K_max).astype(F64)
        closed = np.sum((gammaln(cnt + a / K_max) - gammaln(a / K_max))[cnt > 0]) - (gammaln(cnt.sum() + a) - gammaln(a))
        npt.assert_allclose(lb.log_prob_z_urn(labels, a, K_max), lp, rtol=1e-12)
        npt.assert_allclose(lb.log_prob_z_urn(labels, a, K_max), closed, rtol=1e-12)


@pytest.mark.parametrize("name", list(lb.CASES))
def test_every_gpu_case_has_the_properties_it_is_named_for(name):
    c = lb.CASES[name]
    assert lb.block_plan(c["n"])[0] == lb.EXPECT[name]["n_blocks"]
    for K_max in sorted(set(m[1] for m in c["models"])):
        labels = lb.case_labels(name, K_max)
        assert labels.shape == (c["n"],)
        got = lb.assert_case_properties(name, labels, K_max)
        assert got["holes"] == bool(c.get("holes"))
        if got["holes"]:
            assert 0.25 < np.mean(labels < 0) < 0.4
        # rows_of: every component's rows ascending, together every assigned row once
        rows = lb.component_rows(labels)
        assert all(np.all(np.diff(r) > 0) and np.all(labels[r] == k) for k, r in enumerate(rows))
        assert sum(len(r) for r in rows) == np.count_nonzero(labels >= 0)


NOT_FULL = [m for m in lb.models() if m[3] != "full"]


@pytest.mark.parametrize("name,D,K_max,cov,dtype", NOT_FULL, ids=[i for i, m in zip(lb.model_ids(), lb.models()) if m[3] != "full"])
def test_log_prod_is_a_sum_of_terms_of_one_sign(name, D, K_max, cov, dtype):
    """The GPU test holds log_prod_precision_preds / log_prod_vars to rtol = 1e-13 against a sum taken in another order:
    that bound needs a sum without cancellation (tests/label_blocks.py SPREAD)."""
    assert lb.derived_terms_have_one_sign(lb.case(name, D, K_max, cov, dtype)["stats"])


def test_block_plan_formulas():
    for n, nb in [(1, 1), (16384, 1), (16385, 2), (32768, 2), (32769, 3), (40001, 3), (1048576, 64), (1048577, 64), (2097153, 64)]:
        n_blocks, lo = lb.block_plan(n)
        assert n_blocks == nb and lo[0] == 0 and lo[-1] == n and np.all(np.diff(lo) > 0)
        assert [int(v) for v in lo] == [b * n // nb for b in range(nb + 1)]
    assert list(lb.block_plan(40001)[1]) == [0, 13333, 26667, 40001]
    sizes = np.diff(lb.block_plan(2097153)[1])
    assert sizes.max() == 32769 > lb.STAGED_ROWS and np.count_nonzero(sizes == 32768) == 63


FIXED_F32 = [m for m in lb.models() if m[3] == "fixed" and m[4] is F32]


@pytest.mark.parametrize("name,D,K_max,cov,dtype", FIXED_F32, ids=["%s-D%d" % (m[0], m[1]) for m in FIXED_F32])
def test_fixed_variance_metric_is_sensitive_to_the_row_order(name, D, K_max, cov, dtype):
    """A component's rows reversed, and the rows of block 1 taken before those of block 0, move log_prob_X_given_z by more
    than ten times the GPU test's tolerance: a kernel that walks the lists in a wrong order cannot pass."""
    c = lb.case(name, D, K_max, cov, dtype)
    rows = lb.component_rows(c["labels"])
    n_blocks = lb.block_plan(len(c["labels"]))[0]
    for how in ("reversed", "swap01")[:2 if n_blocks > 1 else 1]:
        v = lb.log_marg_fixed(c["X"], lb.reordered(rows, how, len(c["labels"])), c["prior"])
        moved = abs(v - c["lpx"]) / abs(c["lpx"])
        print("%s D=%d %s: log_prob_X_given_z moves by %.3g relative" % (name, D, how, moved))
        assert moved > 10 * RTOL_RECORD, (how, moved)


def test_numpy_sums_a_float32_column_pairwise_and_wider_matrices_row_after_row():
    """Which order the reference is.  D >= 2: `X.sum(axis=0)` adds row after row and equals np.cumsum(X, axis=0)[-1] bit
    for bit, in both dtypes.  D == 1: the (n, 1) array reduces as a contiguous vector, pairwise -- on the d1 case's
    float32 data the value differs from the sequential sum and equals the pairwise sum of the flat column."""
    for name, D, dt in [("two_blocks", 5, F32), ("three_uneven", 7, F64), ("unstaged", 2, F32)]:
        X = lb.case_data(name, D, dt)[0][:50000]
        assert np.array_equal(X.sum(axis=0), np.cumsum(X, axis=0)[-1])
    c = lb.case("d1", 1, 6, "fixed", F32)
    differ = 0
    for r in lb.component_rows(c["labels"]):
        Xk = c["X"][r]
        assert Xk.shape[1] == 1
        assert Xk.sum(axis=0)[0] == np.add.reduce(np.ascontiguousarray(Xk[:, 0]))
        differ += Xk.sum(axis=0)[0] != np.cumsum(Xk, axis=0)[-1, 0]
    assert differ > 0
    # and the record value built on the sequential sums is off by far more than the record tolerance
    seq = 0.
    var, mu_0, var_0 = c["prior"]
    p, p0, m0 = 1. / var, 1. / var_0, mu_0
    for r in lb.component_rows(c["labels"]):
        Xk, N = c["X"][r], len(r)
        Sx, Sxx = np.cumsum(Xk, axis=0)[-1], np.cumsum(np.square(Xk), axis=0)[-1]
        seq += np.sum((N - 1) / 2. * np.log(p) - 0.5 * N * np.log(2 * np.pi) - 0.5 * np.log(N / p0 + 1. / p) - 0.5 * p * Sxx
                      - 0.5 * p0 * np.square(m0) + 0.5 * (np.square(Sx) * p / p0 + np.square(m0) * p0 / p + 2 * Sx * m0)
                      / (N / p0 + 1. / p))
    assert abs(seq - c["lpx"]) / abs(c["lpx"]) > 10 * RTOL_RECORD

"""
The affine transforms of tests/affine.py on the fp64 specification (oracle/np_fbgmm_batch.py): a transformed corpus with
its transformed prior is the same model in new coordinates, so every log-marginal (log_marg, the span score) and every
token log-likelihood (loglik, all slots) equals the original one plus the Jacobian term -sum_d log s_d.  The GPU tests
that measure the reduced-precision paths on these corpora (test_gpu_tolerance_modes.py, test_gpu_fbgmm_batch.py) are
meaningful only if this holds.
"""
import random

import numpy as np
import pytest

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import affine
from tests.golden import cases


def _spec(kind, corpus, prior, K):
    args = dict(n_slices_min=0, n_slices_max=6, p_boundary_init=0.5, beta_sent_boundary=-1, lms=1.0, wip=0.0,
                init_am_assignments="rand", time_power_term=1.0)
    random.seed(5)
    np.random.seed(5)
    p = no.FixedVarPrior(*prior) if kind == "fixed" else no.NIW(*prior)
    ref = no.UnigramAcousticWordseg(no.FBGMM, 1.0, K, p, *corpus, covariance_type=kind, fb_type="standard", **args)
    return nb.FbgmmBatch(ref, n_gibbs_blocks=3, n_stat_blocks=2, seed=11)


@pytest.mark.parametrize("kind", ["fixed", "diag"])
@pytest.mark.parametrize("name", [n for n in affine.NAMES if n != "identity"])
def test_affine_transform_is_the_same_model_in_new_coordinates(kind, name):
    D, K = 39, 100
    corpus = cases.chain_corpus(25, D, K, 321, True, 0, 6, "float64")
    prior = cases.fixed_prior_params(D) if kind == "fixed" else cases.diag_prior_params(D)
    s, c = affine.params(name, D)
    tprior = affine.fixed_prior(*prior, s, c) if kind == "fixed" else affine.niw_prior(*prior, s, c)
    a = _spec(kind, corpus, prior, K)
    t = _spec(kind, affine.corpus(corpus, s, c), tprior, K)
    assert np.array_equal(a.slot, t.slot)                  # the same initial state
    jac = affine.log_jacobian(s)
    shift_only = np.all(s == 1.0)
    assert (jac == 0.0) == shift_only
    worst_lm = worst_ll = 0.0
    n = 0
    for b in range(a.B):
        da, dt = a.derive(*a.stats_excluding(b)), t.derive(*t.stats_excluding(b))
        assert 0 < da["active"].sum() < K                  # occupied slots and empty ones (the prior predictive)
        for row in range(0, a.X.shape[0], 3):
            want = a.log_marg(da, a.X[row]) + jac
            got = t.log_marg(dt, t.X[row])
            worst_lm = max(worst_lm, abs(got - want) / max(abs(want), 1.0))
            want = a.loglik(da, a.X[row]) + jac
            got = t.loglik(dt, t.X[row])
            worst_ll = max(worst_ll, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))))
            n += 1
    print("%s %s: log_marg worst %.3g, loglik worst %.3g relative (%d rows, Jacobian %.4g)"
          % (kind, name, worst_lm, worst_ll, n, jac))
    # the NIW posterior scale, S_0 + k_0 m_0^2 + sum x^2 - k_N m_N^2 (gaussian_components_diag.py:162-177), cancels terms of
    # size |x|^2 down to a variance of size s^2: the specification's own fp64 rounding grows with (c/s)^2
    tol = 1e-12 if kind == "fixed" else 1e-12 * (1.0 + float(np.max(np.square(c / s))))
    assert worst_lm < tol, (worst_lm, tol)
    assert worst_ll < tol, (worst_ll, tol)


def test_affine_transforms_are_as_named():
    D = 39
    s, c = affine.params("mfcc", D)
    assert 55.0 < c[0] < 65.0 and np.all(np.abs(c[1:]) <= 15.0)
    assert s.min() == 0.3 and s.max() == 8.0
    assert np.array_equal(affine.params("mfcc", D)[0], s)        # fixed seed
    x = np.arange(2 * D, dtype=np.float32).reshape(2, D)
    assert affine.rows(x, s, c).dtype == np.float32
    for name in affine.NAMES:
        s, c = affine.params(name, 7)
        assert s.shape == c.shape == (7,)

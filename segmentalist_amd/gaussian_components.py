"""
Drop-in for segmentalist/gaussian_components.py: full-covariance (normal-inverse-Wishart)
components, statistics resident in HBM (`segk_fbgmm`, cov_type 2).

Where the reference keeps `inv_covars`, the device keeps the lower Cholesky factor of each
component's Student-t covariance matrix (include/segk.h); `inv_covars` is formed from a snapshot of
the factors on request.  Supported by the stand-alone `FBGMM` and by `UnigramAcousticWordseg` with
sync="sequential": D <= 64, no language model; the batch sampler and the bigram classes refuse
covariance_type="full".
"""
import math

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import gammaln

from ._gauss_base import _DeviceGaussianComponents


class GaussianComponents(_DeviceGaussianComponents):
    _cov_type = 2

    def __init__(self, X, prior, assignments=None, K_max=None, _corpus=None, _alpha=1.0, _lms=1.0):
        self.prior = prior
        if K_max is None:
            K_max = X.shape[0]
        D = X.shape[1]
        assert np.asarray(prior.S_0).shape == (D, D), "For full covariance, S_0 needs to be a D x D matrix."
        self._setup(X, assignments, K_max, np.asarray(prior.S_0, np.float64), np.asarray(prior.m_0, np.float64),
                    None, prior.k_0, prior.v_0, _alpha, _lms, _corpus)
        self.dev.check_status()

    @property
    def m_N_numerators(self):
        return self.dev.stat_a.cpu().numpy()

    @property
    def S_N_partials(self):
        return self.dev.stat_b.cpu().numpy()

    @property
    def logdet_covars(self):
        return self.dev.log_prod.cpu().numpy()

    @property
    def chol_covars(self):
        """The lower Cholesky factors L[k] of the components' covariance matrices (the device stores their transposes:
        column j of L contiguous)."""
        return np.ascontiguousarray(self.dev.pred.cpu().numpy().transpose(0, 2, 1))

    @property
    def inv_covars(self):
        """gaussian_components.py:331, from one snapshot of the factors: (L L')^-1 = L^-T L^-1."""
        L = self.chol_covars
        K = self.K
        out = np.zeros_like(L)
        eye = np.eye(self.D)
        for k in range(K):
            Li = solve_triangular(L[k], eye, lower=True)
            out[k] = Li.T.dot(Li)
        return out

    @property
    def cached_log_prior(self):
        """gaussian_components.py:125-127: log_prior of every row, evaluated once at construction."""
        D2 = self.D * self.D
        return self.dev.prior_c[D2:D2 + self.N].cpu().numpy()

    # A2 (vector API), on the device ---------------------------------------------------------------
    def log_prior(self, i):
        """gaussian_components.py:207-214."""
        return self.dev.pred_vector(i)[1]

    def log_post_pred(self, i):
        """gaussian_components.py:228-251."""
        return self.dev.pred_vector(i)[0]

    def log_post_pred_k(self, i, k):
        """gaussian_components.py:216-226."""
        return self.log_post_pred(i)[k]

    def map(self, k):
        """gaussian_components.py:305-316 (host)."""
        p = self.prior
        cnt = self.counts[k]
        k_N = p.k_0 + cnt
        v_N = p.v_0 + cnt
        m_N = self.m_N_numerators[k] / k_N
        sigma = (self.S_N_partials[k] - k_N * np.outer(m_N, m_N)) / (v_N + self.D + 2)
        return m_N, sigma

    def rand_k(self, k):
        raise NotImplementedError("rand_k needs the reference's wishart.py, which is outside this package")

    def _snapshot(self):
        return dict(assignments=self.assignments, K=self.K, counts=self.counts, a=self.m_N_numerators,
                    b=self.S_N_partials)

    def _log_marg_k(self, k, snap, rows):
        """gaussian_components.py:253-276 (record metric, host)."""
        p, D = self.prior, self.D
        cnt = snap["counts"][k]
        k_N = p.k_0 + cnt
        v_N = p.v_0 + cnt
        m_N = snap["a"][k] / k_N
        S_N = snap["b"][k] - k_N * np.outer(m_N, m_N)
        i = np.arange(1, D + 1)
        return (-cnt * D / 2. * math.log(np.pi) + D / 2. * math.log(p.k_0) - D / 2. * math.log(k_N)
                + p.v_0 / 2. * np.linalg.slogdet(p.S_0)[1] - v_N / 2. * np.linalg.slogdet(S_N)[1]
                + np.sum(gammaln((v_N + 1 - i) / 2.) - gammaln((p.v_0 + 1 - i) / 2.)))

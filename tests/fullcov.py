"""
Full-covariance FBGMM (covariance_type="full"): the test cases and a NumPy restatement of the
reference's `GaussianComponents` (gaussian_components.py) plus the item loop of `FBGMM`
(fbgmm.py:256-285, 352-494), written from the formulas.  Test infrastructure: the CPU test holds it
against vectors recorded from the reference (tests/golden/fullcov.npz), the GPU test walks the
device class against it.

Per component k: m_N_numerators[k] (D), S_N_partials[k] (D x D), counts[k]; after every add and
delete, from scratch,
    covar = (k_N + 1) / (k_N (v_N - D + 1)) (S_N_partial - k_N m_N m_N')
and from it logdet_covars[k] and inv_covars[k].  The predictive is the multivariate Student-t with
v = v_N - D + 1 degrees of freedom; here through the Cholesky factor L of covar (logdet =
2 sum log L_dd, Mahalanobis term |L^-1 delta|^2), where the reference uses inv and slogdet.
"""
import math
import random

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import gammaln, logsumexp

# (D, K_max, n_items, seed, dtype, shift)
CASES = [
    (2, 4, 30, 71, np.float32, 0.0),
    (5, 6, 40, 72, np.float32, 0.0),
    (16, 8, 120, 73, np.float32, 0.0),
    (16, 8, 120, 74, np.float64, 0.0),
    (33, 6, 160, 75, np.float32, 0.0),
    (64, 4, 220, 76, np.float32, 0.0),
    (8, 10, 90, 77, np.float32, 4.0),
]
ALPHA, LMS = 1.7, 0.8
# sweeps of gibbs_sample(1) per case, and the variants (AM_GIBBS has the same for the other types):
N_SWEEPS = [4, 4, 3, 3, 2, 2, 3]
UNASSIGNED_CASE = 1        # consider_unassigned=False, a third of the rows unassigned
LINEAR_CASE = 2            # anneal_schedule="linear" over its sweeps
N_PROBE = 12               # rows at which the predictive values / single-item draws are pinned
INV_D_MAX = 16             # inv_covars is stored for D <= 16 only


def case_tag(ci):
    D, K_max, n, seed, dtype, shift = CASES[ci]
    return "c%d_D%d" % (ci, D)


def case_data(ci):
    D, K_max, n, seed, dtype, shift = CASES[ci]
    rs = np.random.RandomState(seed)
    mu = 1.5 * rs.randn(max(2, K_max // 2), D)
    z = rs.randint(0, len(mu), n)
    X = (mu[z] + 0.3 * rs.randn(n, D) + shift).astype(dtype)
    return X


def prior_params(ci):
    """(m_0, k_0, v_0, S_0) of NIW."""
    D, K_max, n, seed, dtype, shift = CASES[ci]
    v_0 = D + 3
    return shift * np.ones(D), 0.05, v_0, 0.1 * v_0 * np.eye(D)


def probe_rows(ci):
    n = CASES[ci][2]
    return np.unique(np.linspace(0, n - 1, N_PROBE).astype(np.int64))


def sweep_kwargs(ci, n_sweeps):
    """Arguments of the gibbs_sample calls of case ci: a list of one dict per gibbs_sample(1) call."""
    if ci == LINEAR_CASE:
        # one linear schedule spread over the calls (the state is pinned after every sweep): call s is a one-step
        # schedule at inverse temperature linspace(0.5, 1, n)[s]
        return [dict(anneal_schedule="linear", anneal_start_temp_inv=float(a), anneal_end_temp_inv=float(a), n_anneal_steps=1)
                for a in np.linspace(0.5, 1.0, n_sweeps)]
    if ci == UNASSIGNED_CASE:
        return [dict(consider_unassigned=False)] * n_sweeps
    return [{}] * n_sweeps


class SpecPrior(object):
    def __init__(self, m_0, k_0, v_0, S_0):
        self.m_0, self.k_0, self.v_0, self.S_0 = m_0, k_0, v_0, S_0


class SpecComponents(object):
    """gaussian_components.py:75-344."""

    def __init__(self, X, prior, assignments=None, K_max=None):
        self.X, self.prior = X, prior
        self.N, self.D = X.shape
        self.K_max = self.N if K_max is None else K_max
        D, K = self.D, self.K_max
        self.m_N_numerators = np.zeros((K, D))
        self.S_N_partials = np.zeros((K, D, D))
        self.logdet_covars = np.zeros(K)
        self.inv_covars = np.zeros((K, D, D))
        self.chol = np.zeros((K, D, D))
        self.counts = np.zeros(K, np.int64)
        self.K = 0
        # the reference caches np.outer(X[i], X[i]) in the dtype of X (:116-118 assigns it into a float64 array: the
        # products are rounded to X's dtype first)
        self._outer = np.einsum("ni,nj->nij", X, X).astype(np.float64) if X.dtype == np.float64 else None
        covar0 = (prior.k_0 + 1.) / (prior.k_0 * (prior.v_0 - D + 1.)) * np.asarray(prior.S_0, np.float64)
        self._L0 = np.linalg.cholesky(covar0)
        self._logdet0 = 2. * np.log(np.diag(self._L0)).sum()
        self.cached_log_prior = np.array([self.log_prior(i) for i in range(self.N)])
        if assignments is None:
            self.assignments = -1 * np.ones(self.N, np.int64)
        else:
            assignments = np.asarray(assignments, np.int64)
            assert set(assignments).difference([-1]) == set(range(assignments.max() + 1))
            self.assignments = assignments.copy()
            for k in range(self.assignments.max() + 1):
                for i in np.where(self.assignments == k)[0]:
                    self.add_item(i, k)

    def outer(self, i):
        if self._outer is not None:
            return self._outer[i]
        x = self.X[i]
        return np.outer(x, x).astype(np.float64)          # rounded in X's dtype, then widened

    def _refresh(self, k):
        p, D = self.prior, self.D
        k_N = p.k_0 + self.counts[k]
        v_N = p.v_0 + self.counts[k]
        m_N = self.m_N_numerators[k] / k_N
        covar = (k_N + 1.) / (k_N * (v_N - D + 1.)) * (self.S_N_partials[k] - k_N * np.outer(m_N, m_N))
        L = np.linalg.cholesky(covar)
        self.chol[k] = L
        self.logdet_covars[k] = 2. * np.log(np.diag(L)).sum()
        Li = solve_triangular(L, np.eye(D), lower=True)
        self.inv_covars[k] = Li.T.dot(Li)

    def add_item(self, i, k):
        p = self.prior
        if k == self.K:
            self.K += 1
            self.m_N_numerators[k] = p.k_0 * np.asarray(p.m_0, np.float64)
            self.S_N_partials[k] = np.asarray(p.S_0, np.float64) + p.k_0 * np.outer(p.m_0, p.m_0)
        self.m_N_numerators[k] += self.X[i]
        self.S_N_partials[k] += self.outer(i)
        self.counts[k] += 1
        self._refresh(k)
        self.assignments[i] = k

    def del_item(self, i):
        k = self.assignments[i]
        if k != -1:
            self.counts[k] -= 1
            self.assignments[i] = -1
            if self.counts[k] == 0:
                self.del_component(k)
            else:
                self.m_N_numerators[k] -= self.X[i]
                self.S_N_partials[k] -= self.outer(i)
                self._refresh(k)

    def del_component(self, k):
        """Swap-last compaction (:188-205)."""
        self.K -= 1
        K = self.K
        arrays = (self.m_N_numerators, self.S_N_partials, self.logdet_covars, self.inv_covars, self.chol, self.counts)
        if k != K:
            for a in arrays:
                a[k] = a[K]
            self.assignments[self.assignments == K] = k
        for a in arrays:
            a[K] = 0

    def cache(self, k):
        return tuple(np.copy(a[k]) for a in (self.m_N_numerators, self.S_N_partials, self.logdet_covars, self.inv_covars,
                                             self.chol, self.counts))

    def restore(self, k, stats):
        for a, s in zip((self.m_N_numerators, self.S_N_partials, self.logdet_covars, self.inv_covars, self.chol, self.counts),
                        stats):
            a[k] = s

    def _student_t(self, i, mu, logdet, L, v):
        D = self.D
        y = solve_triangular(L, self.X[i].astype(np.float64) - mu, lower=True)
        return (gammaln((v + D) / 2.) - gammaln(v / 2.) - D / 2. * math.log(v) - D / 2. * math.log(np.pi)
                - 0.5 * logdet - (v + D) / 2. * math.log(1. + 1. / v * y.dot(y)))

    def log_prior(self, i):
        p = self.prior
        return self._student_t(i, np.asarray(p.m_0, np.float64), self._logdet0, self._L0, p.v_0 - self.D + 1)

    def log_post_pred_k(self, i, k):
        p = self.prior
        k_N = p.k_0 + self.counts[k]
        v_N = p.v_0 + self.counts[k]
        return self._student_t(i, self.m_N_numerators[k] / k_N, self.logdet_covars[k], self.chol[k], v_N - self.D + 1)

    def log_post_pred(self, i):
        return np.array([self.log_post_pred_k(i, k) for k in range(self.K)])

    def log_marg_k(self, k):
        p, D = self.prior, self.D
        k_N = p.k_0 + self.counts[k]
        v_N = p.v_0 + self.counts[k]
        m_N = self.m_N_numerators[k] / k_N
        S_N = self.S_N_partials[k] - k_N * np.outer(m_N, m_N)
        j = np.arange(1, D + 1)
        return (-self.counts[k] * D / 2. * math.log(np.pi) + D / 2. * math.log(p.k_0) - D / 2. * math.log(k_N)
                + p.v_0 / 2. * np.linalg.slogdet(p.S_0)[1] - v_N / 2. * np.linalg.slogdet(S_N)[1]
                + np.sum(gammaln((v_N + 1 - j) / 2.) - gammaln((p.v_0 + 1 - j) / 2.)))

    def log_marg(self):
        return sum(self.log_marg_k(k) for k in range(self.K))


def draw(p_k, u):
    """utils.draw (utils.py:10-21) with the uniform given; also the distance from u to the nearest cumulative edge."""
    margin = np.inf
    k_out = None
    for i in range(len(p_k)):
        u = u - p_k[i]
        margin = min(margin, abs(u))
        if u < 0 and k_out is None:
            k_out = i
    return (len(p_k) - 1 if k_out is None else k_out), margin


class SpecFBGMM(object):
    """fbgmm.py: the item loop over SpecComponents; uniforms from random.random() like the reference."""

    def __init__(self, X, prior, alpha, K, assignments, lms=1.0):
        self.alpha, self.lms = alpha, lms
        N = X.shape[0]
        if isinstance(assignments, str) and assignments == "rand":
            assignments = np.random.randint(0, K, N)
            # fbgmm.py:118-128: labels made consecutive in order of increasing value
            _, assignments = np.unique(assignments, return_inverse=True)
        self.components = SpecComponents(X, prior, assignments, K_max=K)
        self.margins = []

    def _log_prob_z(self, i, scale, normalise=False):
        c = self.components
        lp = scale * np.log(float(self.alpha) / c.K_max + c.counts)
        if normalise:
            lp = scale * (np.log(float(self.alpha) / c.K_max + c.counts) - np.log(np.sum(c.counts) + self.alpha))
        lp[:c.K] += c.log_post_pred(i)
        lp[c.K:] += c.log_prior(i)
        return lp

    def log_marg_i(self, i):
        return logsumexp(self._log_prob_z(i, self.lms, True))

    def _prob(self, lp, anneal_temp):
        if anneal_temp != 1:
            lp = lp - logsumexp(lp)
            return np.exp(1. / anneal_temp * lp - logsumexp(1. / anneal_temp * lp))
        return np.exp(lp - logsumexp(lp))

    def _draw(self, i, anneal_temp):
        c = self.components
        k, margin = draw(self._prob(self._log_prob_z(i, self.lms), anneal_temp), random.random())
        self.margins.append(margin)
        return min(k, c.K)

    def gibbs_sample_inside_loop_i(self, i, anneal_temp=1):
        self.components.add_item(i, self._draw(i, anneal_temp))

    def map_assign_i(self, i):
        c = self.components
        k = int(np.argmax(self._prob(self._log_prob_z(i, 1.0), 1)))
        c.add_item(i, min(k, c.K))

    def log_prob_z(self):
        c = self.components
        return (gammaln(self.alpha) - gammaln(self.alpha + np.sum(c.counts))
                + np.sum(gammaln(c.counts + float(self.alpha) / c.K_max) - gammaln(self.alpha / c.K_max)))

    def log_marg(self):
        return self.log_prob_z() + self.components.log_marg()

    def gibbs_sample(self, n_iter, consider_unassigned=True, anneal_schedule=None, anneal_start_temp_inv=0.1,
                     anneal_end_temp_inv=1, n_anneal_steps=-1):
        """fbgmm.py:288-420 (schedules None and "linear")."""
        rec = {k: [] for k in ["log_marg", "log_prob_z", "log_prob_X_given_z", "anneal_temp", "components"]}
        temps = iter([])
        if anneal_schedule == "linear":
            temps = iter(1. / np.linspace(anneal_start_temp_inv, anneal_end_temp_inv, n_iter if n_anneal_steps == -1 else n_anneal_steps))
        else:
            assert anneal_schedule is None
        c = self.components
        for _ in range(n_iter):
            anneal_temp = next(temps, anneal_end_temp_inv)
            for i in range(c.N):
                k_old = c.assignments[i]
                if not consider_unassigned and k_old == -1:
                    continue
                K_old = c.K
                stats = c.cache(k_old)
                c.del_item(i)
                k = self._draw(i, anneal_temp)
                if k == k_old and c.K == K_old:
                    c.restore(k_old, stats)
                    c.assignments[i] = k_old
                else:
                    c.add_item(i, k)
            rec["log_marg"].append(self.log_marg())
            rec["log_prob_z"].append(self.log_prob_z())
            rec["log_prob_X_given_z"].append(c.log_marg())
            rec["anneal_temp"].append(anneal_temp)
            rec["components"].append(c.K)
        return rec


def initial_assignments(ci):
    """What FBGMM(..., assignments="rand") draws after np.random.seed(1); the unassigned case then clears every third row."""
    D, K_max, n, seed, dtype, shift = CASES[ci]
    np.random.seed(1)
    a = np.random.randint(0, K_max, n)
    _, a = np.unique(a, return_inverse=True)
    a = a.astype(np.int64)
    if ci == UNASSIGNED_CASE:
        a[::3] = -1
        _, inv = np.unique(a[a != -1], return_inverse=True)
        a[a != -1] = inv
    return a


STAT_NAMES = ["m_N_numerators", "S_N_partials", "logdet_covars"]


def run_case(ci, fbgmm_cls, niw_cls, take_margins=None, **fbgmm_kw):
    """The scripted walk every implementation is put through (the reference when the fixture is made, the specification,
    the device class): construction, predictive values at the probe rows, single-item draws, MAP assignments, sweeps.
    Returns the arrays of tests/golden/fullcov.npz for case ci, keys without the case tag.  `take_margins()`: the draw
    margins recorded since its last call (None: not recorded)."""
    D, K_max, n, seed, dtype, shift = CASES[ci]
    X = case_data(ci)
    out = {}
    random.seed(1)
    np.random.seed(1)
    assign = initial_assignments(ci) if ci == UNASSIGNED_CASE else "rand"
    random.seed(1)
    np.random.seed(1)
    fm = fbgmm_cls(X, niw_cls(*prior_params(ci)), ALPHA, K_max, assign, lms=LMS, **fbgmm_kw)
    c = fm.components

    def stats(tag):
        out[tag + "_K"] = np.array(c.K)
        out[tag + "_counts"] = np.array(c.counts)
        out[tag + "_assign"] = np.array(c.assignments)
        for nm in STAT_NAMES:
            out[tag + "_" + nm] = np.array(getattr(c, nm))

    stats("init")
    if D <= INV_D_MAX:
        out["init_inv_covars"] = np.array(c.inv_covars)
    rows = probe_rows(ci)
    K0 = c.K
    out["log_post_pred"] = np.array([np.asarray(c.log_post_pred(i))[:K0] for i in rows])
    out["log_prior"] = np.array([c.log_prior(i) for i in rows])
    out["log_marg_i"] = np.array([fm.log_marg_i(i) for i in rows])
    out["log_marg"] = np.array(fm.log_marg())
    out["components_log_marg"] = np.array(c.log_marg())
    # single-item draws: the row is taken out first (the state mutates between draws)
    ks = []
    for i in rows:
        c.del_item(i)
        fm.gibbs_sample_inside_loop_i(i)
        ks.append(c.assignments[i])
    out["draw_k"] = np.array(ks)
    if take_margins:
        out["draw_margin"] = np.array(take_margins())
    stats("draw")
    ks = []
    for i in rows[::-1]:
        c.del_item(i)
        fm.map_assign_i(i)
        ks.append(c.assignments[i])
    out["map_k"] = np.array(ks)
    stats("map")
    for s, kw in enumerate(sweep_kwargs(ci, N_SWEEPS[ci])):
        rec = fm.gibbs_sample(1, **kw)
        stats("sweep%d" % s)
        for k in ["log_marg", "log_prob_z", "log_prob_X_given_z", "anneal_temp", "components"]:
            out["sweep%d_rec_%s" % (s, k)] = np.array(rec[k][0])
        if take_margins:
            out["sweep%d_margin" % s] = np.array(take_margins())
    out["random_after"] = np.array(random.random())
    return out

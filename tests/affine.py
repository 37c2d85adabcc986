"""
Affine transforms of a test corpus and of its prior: x' = s*x + c, with s a scalar or a per-dimension vector and c a
per-dimension vector.  The prior moves with the data, so that the transformed pair is the same model in new coordinates:

  fixed variance:  var' = var*s^2, mu_0' = mu_0*s + c, var_0' = var_0*s^2
  NIW diagonal:    m_0' = m_0*s + c, S_0' = S_0*s^2, k_0 and v_0 unchanged

Under such a pair every density of the model (the predictive of an occupied slot, the prior predictive of an empty one,
hence log_marg_i) is the original one times the Jacobian: log p'(x') = log p(x) - sum_d log s_d (exact in real
arithmetic).  Every corpus of the suite is L2-normalised rows next to the origin; these transforms give the reduced-
precision paths the offsets and per-dimension scales of real inputs (MFCC-like embeddings: c0 in the tens, the other
coefficients spread over about +-15, scales differing by more than an order of magnitude between dimensions).
"""
import numpy as np

NAMES = ["identity", "shift1", "shift16", "mfcc", "scale30", "scale1_64"]


def params(name, D):
    """(s, c) of transform `name` at dimension D, both float64 vectors of length D."""
    one = np.ones(D)
    if name == "identity":
        return one, np.zeros(D)
    if name == "shift1":
        return one, one.copy()
    if name == "shift16":
        return one, 16.0 * one
    if name == "scale30":
        return 30.0 * one, np.zeros(D)
    if name == "scale1_64":
        return one / 64.0, np.zeros(D)
    if name == "mfcc":
        rs = np.random.RandomState(1234)
        c = rs.uniform(-15.0, 15.0, D)
        c[0] = 60.0 + rs.uniform(-2.0, 2.0)
        s = np.exp(rs.uniform(np.log(0.3), np.log(8.0), D))
        s[0], s[-1] = 8.0, 0.3                 # both ends of the range present at every D
        return s, c
    raise KeyError(name)


def rows(x, s, c):
    """s*x + c in float64, returned in the dtype of x."""
    return (np.asarray(x, np.float64) * s + c).astype(x.dtype)


def corpus(corp, s, c):
    """(embedding_mats, vec_ids, durations, landmarks) with every embedding row transformed."""
    mats = {k: rows(v, s, c) for k, v in corp[0].items()}
    return (mats,) + tuple(corp[1:])


def fixed_prior(var, mu_0, var_0, s, c):
    s2 = np.square(s)
    return var * s2, mu_0 * s + c, var_0 * s2


def niw_prior(m_0, k_0, v_0, S_0, s, c):
    return m_0 * s + c, k_0, v_0, S_0 * np.square(s)


def log_jacobian(s):
    """log p'(s*x + c) - log p(x) of every density of the transformed model."""
    return -float(np.sum(np.log(s)))

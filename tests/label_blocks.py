"""
A NumPy restatement of what the three consumers of `segk_rows_by_label` (segk_metrics.hip) must produce when the assignment
vector spans more than one block of rows: the statistics of Components.__init__ (k_fbgmm_init_stats, k_fc_init) and the
record metrics (k_metric_log_marg, k_metric_reduce), with the cases of tests/test_gpu_label_blocks.py.

The helper cuts the rows into n_blocks = min(64, ceil(n_emb / 16384)) blocks, blk_lo[b] = b * n_emb // n_blocks, sorts
every block by label (stably) and every consumer then walks a component's rows block after block -- which must be the
component's rows in ascending order.  Nothing below knows about blocks except `block_plan` / `case_properties`, which
say what a case exercises, and `reordered`, which the sensitivity checks use to take the rows in a wrong order.

Order of additions.  The reference classes add a component's rows one at a time, ascending, to fp64 statistics;
np.cumsum([start, terms...], axis=0)[-1] performs the same IEEE additions as that loop, so the statistics below are
comparable bit for bit.  The fixed-variance metric (gaussian_components_fixedvar.py:261-283) sums X and X^2 in the dtype
of X with `X.sum(axis=0)`: for D >= 2 numpy adds row after row (equal to np.cumsum(X, axis=0)[-1] bit for bit), for
D == 1 the (n, 1) array reduces as a contiguous vector, pairwise.  `log_marg_fixed` calls numpy's `sum` itself, so it is
the reference's value in both regimes.
"""
import math

import numpy as np
from scipy.special import gammaln

from tests import affine

ROWS_PER_BLOCK = 16384        # segk_rows_by_label: one block per 16 384 rows ...
MAX_BLOCKS = 64               # ... 64 at most (METRIC_MAX_BLOCKS)
STAGED_ROWS = 32768           # k_batch_sort stages a block's keys in LDS up to this size (SORT_KEYS_LDS)
ALPHA = 1.7
URN_A = (0.5, 3.0)            # the two concentrations of the urn form
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ blocks
def block_plan(n_emb):
    """(n_blocks, blk_lo[n_blocks + 1]) of segk_rows_by_label / k_metric_setup."""
    n_blocks = max(1, min(MAX_BLOCKS, (n_emb + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK))
    blk_lo = (np.arange(n_blocks + 1, dtype=np.int64) * n_emb) // n_blocks
    return n_blocks, blk_lo


def block_counts(labels, K_max):
    """cnt[b, k]: rows of component k in block b."""
    labels = np.asarray(labels)
    n_blocks, blk_lo = block_plan(len(labels))
    blk = np.searchsorted(blk_lo, np.arange(len(labels)), side="right") - 1
    m = labels >= 0
    return np.bincount(blk[m] * K_max + labels[m], minlength=n_blocks * K_max).reshape(n_blocks, K_max)


def case_properties(labels, K_max):
    """What an assignment vector exercises in the walk `for b in blocks: for q in koff[b][k] .. koff[b][k + 1]`."""
    labels = np.asarray(labels)
    n_blocks, blk_lo = block_plan(len(labels))
    sizes = np.diff(blk_lo)
    cnt = block_counts(labels, K_max)
    tot = cnt.sum(axis=0)
    active = tot > 0
    return dict(
        n_blocks=n_blocks, largest_block=int(sizes.max()), smallest_block=int(sizes.min()),
        blocks_staged=int((sizes <= STAGED_ROWS).sum()), blocks_unstaged=int((sizes > STAGED_ROWS).sum()),
        straddles=bool(((cnt > 0).sum(axis=0) >= 2).any()),              # a component with rows in two or more blocks
        absent=bool((active & (cnt == 0).any(axis=0)).any()),            # an active component without a row in some block
        ragged_list=bool((cnt % 8 != 0).any()),                          # a (block, component) list with a clamped tail
        list_of_8=bool((cnt == 8).any()), list_of_9=bool((cnt == 9).any()), list_of_1=bool((cnt == 1).any()),
        holes=bool((labels < 0).any()),
        components_empty=int((tot == 0).sum()), components_single=int((tot == 1).sum()),
        components_many=int((tot >= 1000).sum()))


def rows_of(labels, K):
    """(order, bounds): the rows of component k, ascending, are order[bounds[k]:bounds[k + 1]]."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable")
    bounds = np.searchsorted(labels[order], np.arange(K + 1))
    return order, bounds


def component_rows(labels):
    """List over the active components of their rows in ascending order."""
    K = int(np.max(labels)) + 1
    order, bounds = rows_of(labels, K)
    return [order[bounds[k]:bounds[k + 1]] for k in range(K)]


def reordered(rows, how, n_emb):
    """The rows of every component in a WRONG order, for the sensitivity checks: "reversed", or "swap01" (the rows of
    block 1 before those of block 0, the rest as it was)."""
    if how == "reversed":
        return [r[::-1] for r in rows]
    assert how == "swap01"
    _, blk_lo = block_plan(n_emb)
    out = []
    for r in rows:
        i0, i1 = np.searchsorted(r, [blk_lo[1], blk_lo[2]])
        out.append(np.concatenate([r[i0:i1], r[:i0], r[i1:]]))
    return out


# ------------------------------------------------------------------ initial statistics
def _seq_sum(start, n, terms):
    """start + terms(0, n)[0] + terms(0, n)[1] + ... one row after the other in float64: the additions of a loop (np.cumsum
    is sequential), in chunks to bound the memory."""
    acc = np.array(start, F64)
    chunk = max(1, (1 << 17) // max(1, acc.size))          # a megabyte at a time: the running sums stay in cache
    buf = np.empty((min(n, chunk) + 1,) + acc.shape)
    for lo in range(0, n, chunk):
        m = min(n, lo + chunk) - lo
        buf[0] = acc
        buf[1:m + 1] = terms(lo, lo + m)
        acc = np.cumsum(buf[:m + 1], axis=0, out=buf[:m + 1])[-1].copy()
    return acc


def init_stats(X, labels, K_max, cov, prior, rows=None):
    """The state Components.__init__ leaves for an assignment vector: add_item(i, k) for k ascending and the rows i of k
    ascending.  Returns dict(K, counts, assignments, a, b, derived, log_prod) with the arrays of the reference:
      fixed  a = mu_N_numerators, b = precision_Ns, derived = precision_preds, log_prod = log_prod_precision_preds
      diag   a = m_N_numerators,  b = S_N_partials, derived = inv_vars,        log_prod = log_prod_vars
      full   a = m_N_numerators,  b = S_N_partials [K_max, D, D],              log_prod = logdet_covars (no `derived`)."""
    labels = np.asarray(labels, np.int64)
    n, D = X.shape
    rows = component_rows(labels) if rows is None else rows
    K = len(rows)
    counts = np.zeros(K_max, np.int64)
    counts[:K] = [len(r) for r in rows]
    a = np.zeros((K_max, D))
    b = np.zeros((K_max, D, D) if cov == "full" else (K_max, D))
    derived = None if cov == "full" else np.zeros((K_max, D))
    log_prod = np.zeros(K_max)
    if cov == "fixed":
        var, mu_0, var_0 = prior
        prec, prec_0 = 1. / np.asarray(var, F64), 1. / np.asarray(var_0, F64)
        for k, r in enumerate(rows):
            # add_item: mu_N_numerators += precision * X[i]; precision_Ns += precision (one addition per row)
            a[k] = _seq_sum(prec_0 * mu_0, len(r), lambda lo, hi: prec * X[r[lo:hi]])
            b[k] = _seq_sum(prec_0, len(r), lambda lo, hi: np.broadcast_to(prec, (hi - lo, D)))
        derived[:K] = b[:K] * prec / (b[:K] + prec)
        log_prod[:K] = np.log(derived[:K]).sum(axis=1)
    elif cov == "diag":
        m_0, k_0, v_0, S_0 = prior
        for k, r in enumerate(rows):
            a[k] = _seq_sum(k_0 * m_0, len(r), lambda lo, hi: X[r[lo:hi]])
            # the reference caches np.square(X) in the dtype of X
            b[k] = _seq_sum(S_0 + k_0 * np.square(m_0), len(r), lambda lo, hi: np.square(X[r[lo:hi]]))
        k_N = (k_0 + counts[:K])[:, None]
        v_N = (v_0 + counts[:K])[:, None]
        m_N = a[:K] / k_N
        var = (k_N + 1.) / (k_N * v_N) * (b[:K] - k_N * np.square(m_N))
        derived[:K] = 1. / var
        log_prod[:K] = np.log(var).sum(axis=1)
    else:
        assert cov == "full"
        m_0, k_0, v_0, S_0 = prior
        for k, r in enumerate(rows):
            a[k] = _seq_sum(k_0 * m_0, len(r), lambda lo, hi: X[r[lo:hi]])
            # tests/fullcov.py: np.outer(X[i], X[i]) rounded in the dtype of X, then widened
            b[k] = _seq_sum(S_0 + k_0 * np.outer(m_0, m_0), len(r),
                            lambda lo, hi: np.einsum("ni,nj->nij", X[r[lo:hi]], X[r[lo:hi]]))
            k_N, v_N = k_0 + counts[k], v_0 + counts[k]
            m_N = a[k] / k_N
            covar = (k_N + 1.) / (k_N * (v_N - D + 1.)) * (b[k] - k_N * np.outer(m_N, m_N))
            log_prod[k] = 2. * np.log(np.diag(np.linalg.cholesky(covar))).sum()
    return dict(K=K, counts=counts, assignments=labels, a=a, b=b, derived=derived, log_prod=log_prod)


# ------------------------------------------------------------------ record metrics
def log_marg_fixed(X, rows, prior):
    """Sum over the components of gaussian_components_fixedvar.py:261-283 (`_log_marg_k`), the rows in the order given."""
    var, mu_0, var_0 = prior
    p, p0, m0 = 1. / np.asarray(var, F64), 1. / np.asarray(var_0, F64), np.asarray(mu_0, F64)
    total = 0.
    for r in rows:
        Xk = X[r]
        N = len(r)
        total += np.sum(
            (N - 1) / 2. * np.log(p) - 0.5 * N * math.log(2 * np.pi) - 0.5 * np.log(N / p0 + 1. / p)
            - 0.5 * p * np.square(Xk).sum(axis=0) - 0.5 * p0 * np.square(m0)
            + 0.5 * (np.square(Xk.sum(axis=0)) * p / p0 + np.square(m0) * p0 / p + 2 * Xk.sum(axis=0) * m0)
            / (N / p0 + 1. / p))
    return float(total)


def log_marg_diag(a, b, counts, K, prior):
    """Sum over the components of gaussian_components_diag.py:271-290 from the statistics."""
    m_0, k_0, v_0, S_0 = prior
    D = a.shape[1]
    cnt = counts[:K].astype(F64)
    k_N, v_N = k_0 + cnt, v_0 + cnt
    m_N = a[:K] / k_N[:, None]
    S_N = b[:K] - k_N[:, None] * np.square(m_N)
    terms = (-cnt * D / 2. * math.log(np.pi) + D / 2. * math.log(k_0) - D / 2. * np.log(k_N)
             + v_0 / 2. * np.log(S_0).sum() - v_N / 2. * np.log(S_N).sum(axis=1)
             + D * (gammaln(v_N / 2.) - gammaln(v_0 / 2.)))
    return float(sum(terms, 0.))


def log_marg_full(a, b, counts, K, prior):
    """Sum over the components of gaussian_components.py:253-276 from the statistics."""
    m_0, k_0, v_0, S_0 = prior
    D = a.shape[1]
    j = np.arange(1, D + 1)
    total = 0.
    for k in range(K):
        cnt = counts[k]
        k_N, v_N = k_0 + cnt, v_0 + cnt
        m_N = a[k] / k_N
        S_N = b[k] - k_N * np.outer(m_N, m_N)
        total += (-cnt * D / 2. * math.log(np.pi) + D / 2. * math.log(k_0) - D / 2. * math.log(k_N)
                  + v_0 / 2. * np.linalg.slogdet(S_0)[1] - v_N / 2. * np.linalg.slogdet(S_N)[1]
                  + np.sum(gammaln((v_N + 1 - j) / 2.) - gammaln((v_0 + 1 - j) / 2.)))
    return float(total)


def log_prob_X_given_z(X, cov, prior, stats, rows=None):
    """The record value for the state `stats` (init_stats, or the oracle's arrays after a sweep)."""
    if cov == "fixed":
        return log_marg_fixed(X, component_rows(stats["assignments"]) if rows is None else rows, prior)
    fn = log_marg_diag if cov == "diag" else log_marg_full
    return fn(stats["a"], stats["b"], stats["counts"], stats["K"], prior)


def log_prob_z_fbgmm(counts, alpha, K_max):
    """fbgmm.py:208-225."""
    return float(gammaln(alpha) - gammaln(alpha + np.sum(counts))
                 + np.sum(gammaln(counts + float(alpha) / K_max) - gammaln(alpha / K_max)))


def _urn_ranks(labels):
    """For every assigned row, the number of earlier rows with its label (n_t[k_t] of the sequential urn)."""
    labels = np.asarray(labels)
    lab = labels[labels >= 0]
    order = np.argsort(lab, kind="stable")
    start = np.searchsorted(lab[order], np.arange(int(lab.max()) + 1))
    return np.arange(len(lab)) - start[lab[order]]


def log_prob_z_urn(labels, a, K_max, dtype=F64):
    """bigram_acoustic_wordseg.py:287-305 as the loop computes it: the sequential urn sum_t log((n_t[k_t] + a / K) / (t + a))
    over the assigned rows (taken component by component: only the final counts matter)."""
    ranks = _urn_ranks(labels).astype(dtype)
    a = dtype(a)
    return np.sum(np.log(ranks + a / dtype(K_max))) - np.sum(np.log(np.arange(len(ranks)).astype(dtype) + a))


# ------------------------------------------------------------------ longdouble: where product and reference stand
def _logdet_ld(A):
    """log det of a symmetric positive definite matrix by elimination in longdouble."""
    A = np.array(A, np.longdouble)
    ld = np.longdouble(0)
    for j in range(len(A)):
        ld += np.log(A[j, j])
        col = A[j + 1:, j] / A[j, j]
        A[j + 1:, j + 1:] -= np.outer(col, A[j, j + 1:])
    return ld


def metrics_hi(X, labels, K_max, cov, prior, conc):
    """(log_prob_z, log_prob_X_given_z) with the sums over rows and every expression in np.longdouble (the lgamma terms,
    which depend on the counts alone, stay float64 where no product form is at hand; the full-covariance sums of products
    are one float64 matrix product of the widened rows).  Printed beside the product's and
    the reference's values; nothing is asserted on it.  log_prob_z is the urn product, which equals the FBGMM form."""
    ld = np.longdouble
    rows = component_rows(labels)
    n, D = X.shape
    lpz = log_prob_z_urn(labels, conc, K_max, dtype=ld)
    pi = 4 * np.arctan(ld(1))
    total = ld(0)
    for r in rows:
        N = ld(len(r))
        Xk = X[r].astype(ld)
        if cov == "fixed":
            var, mu_0, var_0 = prior
            p, p0, m0 = 1 / np.asarray(var, ld), 1 / np.asarray(var_0, ld), np.asarray(mu_0, ld)
            Sx, Sxx = Xk.sum(axis=0), np.square(Xk).sum(axis=0)
            den = N / p0 + 1 / p
            total += np.sum((N - 1) / 2 * np.log(p) - N / 2 * np.log(2 * pi) - np.log(den) / 2 - p * Sxx / 2 - p0 * m0 * m0 / 2
                            + (Sx * Sx * p / p0 + m0 * m0 * p0 / p + 2 * Sx * m0) / den / 2)
            continue
        m_0, k_0, v_0, S_0 = prior
        m_0, S_0 = np.asarray(m_0, ld), np.asarray(S_0, ld)
        k_N, v_N = ld(k_0) + N, ld(v_0) + N
        m_N = (ld(k_0) * m_0 + Xk.sum(axis=0)) / k_N
        head = -N * D / 2 * np.log(pi) + ld(D) / 2 * np.log(ld(k_0)) - ld(D) / 2 * np.log(k_N)
        if cov == "diag":
            S_N = S_0 + ld(k_0) * m_0 * m_0 + np.square(Xk).sum(axis=0) - k_N * m_N * m_N
            total += (head + ld(v_0) / 2 * np.log(S_0).sum() - v_N / 2 * np.log(S_N).sum()
                      + D * ld(gammaln(float(v_N) / 2.) - gammaln(v_0 / 2.)))
        else:
            X64 = X[r].astype(F64)                          # (the D x D sums of products in float64: a matrix product)
            S_N = S_0 + ld(k_0) * np.outer(m_0, m_0) + X64.T.dot(X64).astype(ld) - k_N * np.outer(m_N, m_N)
            j = np.arange(1, D + 1)
            total += (head + ld(v_0) / 2 * _logdet_ld(S_0) - v_N / 2 * _logdet_ld(S_N)
                      + ld(np.sum(gammaln((float(v_N) + 1 - j) / 2.) - gammaln((v_0 + 1 - j) / 2.))))
    return lpz, total


def rel(x, hi):
    return float(abs(np.longdouble(x) - hi) / abs(hi))


# ------------------------------------------------------------------ cases
# name -> rows, transform of tests/affine.py, layout of the labels, models (D, K_max, covariance, dtype)
CASES = {
    "one_block_edge": dict(n=16384, tf="mfcc", models=[(5, 12, "fixed", F32), (5, 12, "diag", F64)]),
    "two_blocks": dict(n=16385, tf="shift16", models=[(5, 12, "fixed", F32), (5, 12, "diag", F32), (3, 12, "full", F32)]),
    "three_uneven": dict(n=40001, tf="mfcc", holes=True, front=True,
                         models=[(7, 40, "fixed", F32), (7, 40, "fixed", F64), (7, 40, "diag", F32)]),
    "wide": dict(n=20000, tf="shift16", models=[(65, 6, "fixed", F32), (129, 6, "fixed", F32), (65, 6, "diag", F32),
                                                 (129, 6, "diag", F32)]),
    "full_d64": dict(n=20000, tf="shift16", models=[(64, 4, "full", F64)]),
    "bank_tiers": dict(n=40001, tf="mfcc", bank=True, models=[(4, K, "diag", F32) for K in (1025, 2049, 4097, 8192)]),
    "cap_64": dict(n=1048577, tf="mfcc", models=[(2, 8, "fixed", F32)]),
    "unstaged": dict(n=2097153, tf="shift16", models=[(2, 8, "fixed", F32), (2, 8, "diag", F32)]),
    "d1": dict(n=20000, tf="mfcc", models=[(1, 6, "fixed", F32), (1, 6, "fixed", F64)]),
}
# what case_properties must report for every label vector of the case
EXPECT = {
    "one_block_edge": dict(n_blocks=1, largest_block=16384, list_of_8=True, ragged_list=True, holes=False),
    "two_blocks": dict(n_blocks=2, largest_block=8193, smallest_block=8192, straddles=True, ragged_list=True, list_of_8=True,
                       list_of_9=True),
    "three_uneven": dict(n_blocks=3, largest_block=13334, smallest_block=13333, straddles=True, absent=True, holes=True,
                         ragged_list=True, list_of_8=True, list_of_9=True, list_of_1=True),
    "wide": dict(n_blocks=2, straddles=True, ragged_list=True),
    "full_d64": dict(n_blocks=2, straddles=True, ragged_list=True),
    "bank_tiers": dict(n_blocks=3, straddles=True, absent=True, ragged_list=True, list_of_8=True, list_of_1=True,
                       components_empty=5, min_components_single=1, min_components_many=1),
    "cap_64": dict(n_blocks=64, smallest_block=16384, largest_block=16385, blocks_unstaged=0, straddles=True),
    "unstaged": dict(n_blocks=64, smallest_block=32768, largest_block=32769, straddles=True),
    "d1": dict(n_blocks=2, straddles=True),
}


def assert_case_properties(name, labels, K_max):
    """The label vector has what its case is named for (a key `min_x`: x at least that)."""
    got = case_properties(labels, K_max)
    for key, want in EXPECT[name].items():
        if key.startswith("min_"):
            assert got[key[4:]] >= want, (name, K_max, key, got[key[4:]])
        else:
            assert got[key] == want, (name, K_max, key, got[key])
    if CASES[name].get("front"):
        k = int(np.max(labels)) - 1
        assert np.flatnonzero(labels == k).max() < FIRST_ROWS and block_counts(labels, K_max)[1:, k].sum() == 0
    return got


FIRST_ROWS = 5000           # `front`: one component's rows all lie below this row
TAIL_LISTS = (8, 9, 1)       # the lists of the last active component in blocks 0, 1, 2 (none in the other blocks)


def model_ids():
    return ["%s-D%d-K%d-%s-%s" % (name, D, K, cov, "f32" if dt is F32 else "f64")
            for name, c in CASES.items() for (D, K, cov, dt) in c["models"]]


def models():
    return [(name, D, K, cov, dt) for name, c in CASES.items() for (D, K, cov, dt) in c["models"]]


def _seed(name):
    return 1000 + 17 * sorted(CASES).index(name)


def case_labels(name, K_max):
    """The assignment vector of a case: random labels with every component present; the last active component has lists of
    exactly 8, 9 and 1 rows in blocks 0, 1 and 2; `front`: the component before it lives in the first 5 000 rows only;
    `bank`: five components of the bank stay empty, component 0 has one row, component 1 thousands; `holes`: about a third
    of the other rows unassigned (-1)."""
    c = CASES[name]
    n = c["n"]
    rs = np.random.RandomState(_seed(name) + K_max)
    n_blocks, blk_lo = block_plan(n)
    K_act = K_max - 5 if c.get("bank") else K_max
    k_tail = K_act - 1
    k_front = K_act - 2 if c.get("front") else None
    p0, p1 = (1 if c.get("bank") else 0), K_act - 1 - (1 if c.get("front") else 0)        # the randomly spread components
    labels = rs.randint(p0, p1, n).astype(np.int64)
    if c.get("bank"):
        labels[rs.choice(n, 6000, replace=False)] = p0
    keep = rs.permutation(n)[:p1 - p0]
    labels[keep] = np.arange(p0, p1)                    # every spread component is present
    fixed = np.zeros(n, bool)
    fixed[keep] = True

    def plant(k, lo, hi, count):
        free = lo + np.flatnonzero(~fixed[lo:hi])
        r = rs.choice(free, count, replace=False)
        labels[r] = k
        fixed[r] = True

    if c.get("bank"):
        plant(0, 0, n, 1)
    if k_front is not None:
        plant(k_front, 0, FIRST_ROWS, 300)
    for b in range(min(n_blocks, len(TAIL_LISTS))):
        plant(k_tail, blk_lo[b], blk_lo[b + 1], TAIL_LISTS[b])
    if c.get("holes"):
        labels[~fixed & (rs.rand(n) < 1. / 3.)] = -1
    assert set(np.unique(labels)).difference([-1]) == set(range(K_act))
    return labels


# The clusters before the transform: five centres SPREAD * 1.5 apart per dimension, SPREAD * 0.3 wide.  SPREAD = 1 / 64
# keeps every variance of every component below 1 in the transformed coordinates (the largest scale of "mfcc" is 8: at
# most 64 (0.09 + 5 * 2.25) / 4096), and every predictive precision of the fixed-variance model above 1.  The derived
# scalars log_prod_* are sums over the dimensions of the logarithms of those; with all terms of one sign a sum of D terms
# taken in another order (the kernel adds across lanes, numpy along the vector) differs by at most (D - 1) eps relative,
# 1.4e-14 at D = 129 -- where the terms cancel, no bound relative to the result holds for two orders of the same sum,
# and rtol = 1e-13 would test the luck of the data (`derived_terms_have_one_sign`, asserted for every model on the CPU).
SPREAD = 1. / 64.
VAR = 0.09 * SPREAD * SPREAD


def case_data(name, D, dtype):
    """Seeded Gaussian clusters through the case's transform of tests/affine.py: offsets of 16 to 60 over a spread of a few
    tenths, where float32 sums depend on their order (identity data next to the origin would hide order errors).
    Returns (X, s, c)."""
    c = CASES[name]
    rs = np.random.RandomState(_seed(name) + 7 * D)
    mu = 1.5 * SPREAD * rs.randn(5, D)
    z = rs.randint(0, 5, c["n"])
    X = (mu[z] + 0.3 * SPREAD * rs.randn(c["n"], D)).astype(dtype)
    s, sh = affine.params(c["tf"], D)
    return affine.rows(X, s, sh), s, sh


def case_prior(cov, D, s, c):
    """The prior in the transformed coordinates: fixed (var, mu_0, var_0); diag / full (m_0, k_0, v_0, S_0)."""
    if cov == "fixed":
        var = VAR * np.ones(D)
        return affine.fixed_prior(var, np.zeros(D), var / 0.05, s, c)
    v_0 = D + 3
    m_0, k_0, v_0, S_0 = affine.niw_prior(np.zeros(D), 0.05, v_0, VAR * v_0 * np.ones(D), s, c)
    return m_0, k_0, v_0, (S_0 if cov == "diag" else np.diag(S_0))


def derived_terms_have_one_sign(stats):
    """Every precision_pred / inv_var of the active components lies above 1: the logarithms summed into log_prod_* share
    their sign."""
    return bool(np.all(stats["derived"][:stats["K"]] > 1.))


_cache = {}


def case(name, D, K_max, cov, dtype):
    """Everything a test needs of one model of a case, computed once per process and shared (leave it unchanged):
    dict(X, labels, prior, stats, lpx, lpz, lpz_urn)."""
    key = (name, D, K_max, cov, dtype)
    if key not in _cache:
        X, s, c = case_data(name, D, dtype)
        labels = case_labels(name, K_max)
        prior = case_prior(cov, D, s, c)
        stats = init_stats(X, labels, K_max, cov, prior)
        out = dict(X=X, labels=labels, prior=prior, stats=stats,
                   lpx=log_prob_X_given_z(X, cov, prior, stats),
                   lpz=log_prob_z_fbgmm(stats["counts"], ALPHA, K_max),
                   lpz_urn=[float(log_prob_z_urn(labels, a, K_max)) for a in URN_A])
        for v in (labels,) + tuple(a for a in stats.values() if isinstance(a, np.ndarray)):
            v.setflags(write=False)
        _cache[key] = out
    return _cache[key]

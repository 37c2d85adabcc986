"""
Executable SPECIFICATION of `FBGMM.set_K(K, reassign=True, sync=...)` and the table of its test cases.  Test infrastructure only,
like tests/fullcov.py and tests/fbgmm_items.py.

Serial form.  `set_k(model, K, reassign)` is the reference's method (fbgmm.py:139-180) restated as a function on any object with
the reference's interface -- the oracle's FBGMM, tests/fullcov.py SpecFBGMM, the translated reference, the device class --, with
two stated differences:

  ties     the ranking is np.argsort(counts, kind="stable"); the reference's default sort is not stable, and its order among
           components of equal size depends on the NumPy build.  Every case here has pairwise distinct counts among its active
           components at the call (`distinct_counts`), where the two agree.
  early    components.K <= K: the reference only overwrites the attribute K_max, its arrays keep their old length and its own
           gibbs_sample then fails (tests/golden/make_golden_set_k.py shows it on the translated reference).  Here the bank is
           rebuilt at the new size from the current assignments; no uniform is consumed.

In the main branch the K kept components are all occupied (components.K > K: there are more than K occupied ones), so the new
bank is full from the start: K = K_max = the target, and no orphan can found a component -- there is never room.

Batch form.  `batch_set_k` is the same ranking, relabelling and rebuild (the same `set_k`, reassign=False), the batch
specification of tests/fbgmm_items.py built on the result, and `orphan_pass`: for b in 0..B-1

  d = derive(*stats_excluding(-1))     the statistics of every item that holds a slot now, in all blocks (an orphan holds none)
  every item i of block b of every slice with slot[i] < 0 that was assigned before the call draws
  draw_chunked(p, u01(seed, sweep_index, i, 1)) from z = prior_z + loglik at temperature 1; the block's draws are applied
  together, then P[s][b] = _partial(s, b): orphans of later blocks see those placed in earlier ones.

Items that were -1 before the call stay -1.  The pass takes one value of the sweeper's counter.
"""
import random

import numpy as np

from oracle import np_fbgmm_batch as nb
from tests import fbgmm_items as fi

ALPHA, LMS = fi.ALPHA, fi.LMS
BATCH_SEED = fi.BATCH_SEED
DRAW_MARGIN = fi.DRAW_MARGIN
N_PROBE = 8

# per covariance type: (statistics, held at 1e-13), (derived values)
STATS = {"fixed": (("mu_N_numerators", "precision_Ns"), ("log_prod_precision_preds", "precision_preds")),
         "diag": (("m_N_numerators", "S_N_partials"), ("log_prod_vars", "inv_vars")),
         "full": (("m_N_numerators", "S_N_partials"), ("logdet_covars",))}

# name -> (cov, dtype, D, K_max, N, seed, target K, fraction unassigned, reassign, serial sweeps before the call)
CASES = {
    "fx_D3": ("fixed", "float32", 3, 8, 150, 1, 3, 0.0, True, 0),
    "fx_D39_f64": ("fixed", "float64", 39, 10, 200, 2, 4, 0.0, True, 0),
    "dg_D16": ("diag", "float32", 16, 12, 300, 3, 5, 0.0, True, 0),
    "dg_D39_f64_un": ("diag", "float64", 39, 10, 400, 14, 4, 0.2, True, 0),            # unassigned rows: they stay -1
    "dg_D3_keep": ("diag", "float32", 3, 8, 150, 35, 3, 0.0, False, 0),                # reassign=False
    "dg_D16_swept": ("diag", "float32", 16, 10, 200, 146, 4, 0.0, True, 3),             # components deleted and relabelled first
    "fc_D3": ("full", "float32", 3, 8, 150, 7, 3, 0.0, True, 0),
    "fc_D16_f64": ("full", "float64", 16, 8, 200, 18, 4, 0.0, True, 0),
    "fc_D39": ("full", "float32", 39, 8, 400, 9, 5, 0.1, True, 0),
    "fx_D16_early": ("fixed", "float32", 16, 8, 150, 10, 11, 0.0, True, 0),           # K >= components.K: the early branch
}
EARLY = "fx_D16_early"

# the batch form against its specification: name -> (cov, dtype, D, K_max, N, seed, target K, fraction unassigned, B, S)
BATCH_CASES = {
    "fx_D3_1x1": ("fixed", "float32", 3, 8, 150, 1, 3, 0.0, 1, 1),
    "dg_D16_4x2": ("diag", "float32", 16, 12, 300, 3, 5, 0.0, 4, 2),
    "dg_D39_f64_un_3x4": ("diag", "float64", 39, 10, 400, 14, 4, 0.2, 3, 4),
    "fx_D39_f64_2x2": ("fixed", "float64", 39, 10, 200, 2, 4, 0.0, 2, 2),
    "fc_D16_f64_4x2": ("full", "float64", 16, 8, 200, 18, 4, 0.0, 4, 2),
    "fc_D3_2x2": ("full", "float32", 3, 8, 150, 7, 3, 0.0, 2, 2),
}


def case_inputs(case):
    """(X, assignments): a mixture of fewer clusters than slots; every slot occupied, the sizes spread out by unequal
    weights (the seeds are chosen so that the counts are pairwise distinct), `unassigned` of the rows at -1"""
    cov, dtype, D, K_max, N, seed = case[:6]
    unassigned = case[7]
    X = fi.case_data(D, K_max, N, 7000 + seed, dtype, 1.0 if cov == "full" and D >= 39 else 0.3)
    rs = np.random.RandomState(9000 + seed)
    w = np.arange(1, K_max + 1, dtype=np.float64) ** 1.5
    a = rs.choice(K_max, N, p=w / w.sum())
    a[rs.choice(N, K_max, replace=False)] = np.arange(K_max)          # every slot occupied
    if unassigned:
        a[rs.rand(N) < unassigned] = -1
    assert set(a.tolist()) - {-1} == set(range(K_max))
    return X, a.astype(np.int64)


def distinct_counts(counts):
    """the counts of the active components are pairwise distinct"""
    act = np.asarray(counts)[np.asarray(counts) > 0]
    return len(set(act.tolist())) == len(act)


def probe_rows(N):
    return np.unique(np.linspace(0, N - 1, N_PROBE).astype(np.int64))


def spec_model(case, assignments=None):
    """the serial reference-pinned model of a case (oracle FBGMM; SpecFBGMM for full covariance)"""
    X, a = case_inputs(case)
    return fi.spec_model(case[0], X, case[3], a if assignments is None else assignments)


def product_model(case, assignments=None, B=8, S=8, K_max=None, **kw):
    """the device model of the same initial state (K_max: another bank size over the same rows)"""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    cov, D = case[0], case[2]
    X, a = case_inputs(case)
    prior = FixedVarPrior(*fi.prior_params(cov, D)) if cov == "fixed" else NIW(*fi.prior_params(cov, D))
    args = dict(covariance_type=cov, lms=LMS, sync="sequential", n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=BATCH_SEED)
    args.update(kw)
    return FBGMM(X, prior, ALPHA, case[3] if K_max is None else K_max, a if assignments is None else np.array(assignments), **args)


def rebuild(model, K, assignments):
    """setup_components(K, assignments) (fbgmm.py:93-137); on the specification classes, which have none, the same:
    components of their own class over the same rows and prior, built from the assignments"""
    if hasattr(model, "setup_components"):
        model.setup_components(K, list(assignments))
        return
    c = model.components
    prior = model.prior if hasattr(model, "prior") else c.prior
    model.components = type(c)(c.X, prior, np.array(assignments, np.int64), K_max=K)


def rank_and_relabel(counts, assignments, K):
    """(kept labels in ascending order of size -- the one at rank r becomes label r --, the relabelled assignments)"""
    keep = [int(k) for k in np.argsort(np.asarray(counts), kind="stable")[-K:]]
    table = np.full(len(counts) + 1, -1, dtype=np.int64)       # (the last entry serves the label -1)
    table[keep] = np.arange(K)
    return keep, table[np.asarray(assignments, np.int64)]


def set_k(model, K, reassign=True):
    """fbgmm.py:139-180 on `model`.  Returns (kept labels, assignments after relabelling, orphans); (None, the assignments,
    []) in the early branch."""
    c = model.components
    old = np.array(c.assignments, dtype=np.int64)
    if c.K <= K:
        rebuild(model, K, old.copy())
        return None, old, []
    counts = np.array(c.counts)
    assert distinct_counts(counts), "set_K on components of equal size: the reference's own order is not reproducible"
    keep, new = rank_and_relabel(counts, old, K)
    rebuild(model, K, new.copy())
    orphans = [int(i) for i in np.flatnonzero((old != -1) & (new == -1))]
    if reassign:
        for i in orphans:
            model.gibbs_sample_inside_loop_i(i)
    return keep, new, orphans


def state_of(model, cov, tag, out=None):
    """K, counts, assignments, statistics, log_marg and log_marg_i at the probe rows, as arrays under `tag`_..."""
    out = {} if out is None else out
    c = model.components
    out[tag + "_K"] = np.array(c.K)
    out[tag + "_K_max"] = np.array(c.K_max)
    out[tag + "_counts"] = np.array(c.counts)
    out[tag + "_assign"] = np.array(c.assignments)
    for nm in STATS[cov][0] + STATS[cov][1]:
        out[tag + "_" + nm] = np.array(getattr(c, nm))
    out[tag + "_log_marg"] = np.array(model.log_marg())
    rows = probe_rows(len(out[tag + "_assign"]))
    out[tag + "_log_marg_i"] = np.array([model.log_marg_i(int(i)) for i in rows])
    return out


def run_case(name, make_model, do_set_k, post=True):
    """The scripted walk every implementation of the serial form is put through (the reference when the fixture is made, the
    specification, the device class): construction from the case's assignments, the case's serial sweeps, the state before
    the call, the call, the state after it.  make_model(case, X, assignments) -> model; do_set_k(model, K, reassign) ->
    (kept labels or None, assignments after relabelling).  Returns the arrays of tests/golden/set_k.npz for the case, keys
    without the case's name.  The sweeps of "dg_D16_swept" and the draws of the call come from random.seed(500 + seed)."""
    case = CASES[name]
    cov, K, reassign, sweeps = case[0], case[6], case[8], case[9]
    X, a = case_inputs(case)
    random.seed(500 + case[5])
    model = make_model(case, X, a.copy())
    if sweeps:
        model.gibbs_sample(sweeps)
    out = state_of(model, cov, "pre")
    keep, new = do_set_k(model, K, reassign)
    if keep is not None:
        out["keep"] = np.array(keep)
        out["relabel_assign"] = np.array(new)
    if post:
        state_of(model, cov, "post", out)
    out["random_after"] = np.array(random.random())
    return out


def orphan_pass(spec, old, sweep_index):
    """the blocked pass over the orphans (module docstring) on a batch specification of tests/fbgmm_items.py"""
    old = np.asarray(old)
    if spec.ll_log is not None:
        spec.ll_log = {}
    for b in range(spec.B):
        d = spec.derive(*spec.stats_excluding(-1))
        new = {}
        for s in range(spec.S):
            for i in range(*spec.ranges[s][b]):
                if spec.slot[i] >= 0 or old[i] < 0:
                    continue
                ll = spec.loglik(d, spec.X[i])
                z = spec.prior_z(d, None, None, None) + ll
                p = spec._probabilities(z, 1.0)
                u = nb.u01(spec.seed, sweep_index, i, 1)
                new[i] = nb.draw_chunked(p, u)
                if spec.ll_log is not None:
                    spec.ll_log[i] = ll
                if getattr(spec, "z_log", None) is not None:
                    spec.z_log[i] = z
                if spec.census is not None:
                    spec.census.draw(p, u)
        for i, k in new.items():
            spec.slot[i] = k
        for s in range(spec.S):
            spec.P[s][b] = spec._partial(s, b)


def batch_spec(am, cov, B, S):
    cls = fi.FullcovItems if cov == "full" else fi.FbgmmItems
    spec = cls(am, n_gibbs_blocks=B, n_stat_blocks=S, seed=BATCH_SEED)
    spec.z_log = None
    return spec


def batch_set_k(am, cov, K, reassign, B, S, sweep_index=0, census=False, ll_log=False, z_log=False):
    """set_K(K, reassign, sync="batch") on the serial specification model `am`: returns (kept labels, assignments after
    relabelling, orphans, the batch specification after the pass)"""
    old = np.array(am.components.assignments, dtype=np.int64)
    keep, new, orphans = set_k(am, K, reassign=False)
    spec = batch_spec(am, cov, B, S)
    spec.census = fi.Census() if census else None
    spec.ll_log = {} if ll_log else None
    spec.z_log = {} if z_log else None
    if reassign and keep is not None:
        orphan_pass(spec, old, sweep_index)
    return keep, new, orphans, spec


def layout_assignments(N, K_max, K, B, S, orphans_per_cell, seed):
    """Assignments that put a chosen number of orphans into every (slice, block) cell: labels 0..K_max-K-1 are small components
    (they go), the K labels above them large ones (they stay).  orphans_per_cell[s][b]: how many of the cell's items carry a
    small label, or "all".  The sizes of the small components are consecutive numbers, every large one is larger, and all are
    pairwise distinct (asserted)."""
    rs = np.random.RandomState(seed)
    n_small = K_max - K
    w = np.arange(1, K + 1, dtype=np.float64) ** 1.5
    a = n_small + rs.choice(K, N, p=w / w.sum())
    sb = [(s * N) // S for s in range(S + 1)]
    where = []
    for s in range(S):
        n_s = sb[s + 1] - sb[s]
        for b in range(B):
            lo, hi = sb[s] + (b * n_s) // B, sb[s] + ((b + 1) * n_s) // B
            want = orphans_per_cell[s][b]
            want = hi - lo if want == "all" else want
            assert want <= hi - lo, (s, b, want, hi - lo)
            where.extend(np.sort(rs.choice(np.arange(lo, hi), want, replace=False)).tolist())
    total = len(where)
    sizes = (total - n_small * (n_small - 1) // 2) // n_small + np.arange(n_small)
    assert sizes[0] >= 1
    sizes[-1] += total - sizes.sum()
    a[np.array(where, dtype=np.int64)] = rs.permutation(np.repeat(np.arange(n_small), sizes))
    counts = np.bincount(a, minlength=K_max)
    assert distinct_counts(counts) and counts[:n_small].max() < counts[n_small:].min(), counts
    return a.astype(np.int64)

"""
Executable SPECIFICATION of `FBGMM.predict`, `FBGMM.score_samples` and `FBGMM.predict_log_proba` (`segk_fbi_predict`,
`segk_fbi_predict_diag32`): labels, log densities and log responsibilities of rows that are NOT in the model.  Test
infrastructure only, like tests/fbgmm_items.py (the sampled sweeps) and tests/fbgmm_items_map.py (the MAP sweeps).

A held-out row x is an UNASSIGNED item appended to X.  With the statistics of ALL items that hold a component -- the batch
specification's `derive(*stats_excluding(-1))`: counts n_k, N_a = sum n_k, the predictive parameters of every slot -- and
ll_k(x) = `loglik(d, x)` (an empty slot: the prior predictive of the row):

  label            the first index of max_k log(alpha / K_max + n_k) + ll_k: FBGMM.map_assign_i (fbgmm.py:475-491) -- no lms,
                   no softmax, all empty slots tie and the first wins --, reported in the numbering of the reference's view:
                   an occupied slot its rank among the occupied slots in increasing slot order (what `canonical` assigns), an
                   empty slot K, "would found a new component" (the `k > K -> K` clamp)
  log density      logsumexp_k lms (log(alpha / K_max + n_k) - log(N_a + alpha)) + ll_k: log_marg_i (fbgmm.py:256-285) of the
                   appended item, lms included
  log resp.        lms log(alpha / K_max + n_k) + ll_k - logsumexp(.): the normalised log_prob_z of fbgmm.py:436-451 at
                   temperature 1; [M, K_max] in the reference view's column order, the K active components, then the empty ones

No new statistics: tests/test_fbgmm_predict_cpu.py holds these against the serial oracle over [X; Xq] with the queries at -1.

`query_rows` is the recipe of the query rows of a case, `Census` (tests/fbgmm_items_map.py's) records the decision margins the
label parity rests on, and the byte counts of the kernels' LDS are restated here for the tests that choose K_max on either
side of the placement rule.
"""
import numpy as np
from scipy.special import logsumexp as _sp_logsumexp

from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32
from tests import fbgmm_items_map as fm

MARGIN = fm.MARGIN               # 1e-6 relative: every label decision of every case
M_QUERY = 130                    # two tiles and two rows
QUERY_SEED = 5000                # added to the case's data seed

# the workgroup's bytes (segmentalist_amd/csrc/segk_fbitems.hip; tests/test_fbgmm_predict_cpu.py holds the constants against the
# source).  fp64 form: rows [D][64] and 16 slots' (mean, q) as doubles, the prior terms [K_max] doubles, the rank table
# [K_max + 1] ints rounded up to 8 bytes, then the tile's logits [64][K_max] doubles where all of it fits in LDS_MAX.
# float32 form: f32.stage_bytes(D), the same two tables, logit rows of K_max | 1 doubles.
TILE, KC, LDS_MAX = fi.TILE, 16, 144 * 1024


def rank_bytes(K_max):
    return ((K_max + 1) * 4 + 7) // 8 * 8


def lds_bytes(D, K_max):
    """fp64 form, cov_type 0 / 1, with the tile's logits in LDS"""
    return (TILE * D + 2 * KC * D) * 8 + K_max * 8 + rank_bytes(K_max) + TILE * K_max * 8


def lds_bytes_f32(D, K_max):
    return f32.stage_bytes(D) + K_max * 8 + rank_bytes(K_max) + TILE * (K_max | 1) * 8


def k_max_either_side(D, form=lds_bytes):
    """(the largest K_max whose logits stay in LDS, the first whose logits go to the workspace)"""
    k = 1
    while form(D, k) <= LDS_MAX:
        k += 1
    return k - 1, k


K_LDS, K_WS = k_max_either_side(39)                         # the fp64 form's last K_max in LDS, the first beyond
K32_LDS, K32_WS = k_max_either_side(39, lds_bytes_f32)      # the float32 form's
# shapes of their own, in the layout of fi.CASES: the K_max values on either side of the placement rule at D = 39
EDGE = {
    "fx_D39_Klds": ("fixed", "float32", 39, K_LDS, 2, 2, 300, 405, (1.0,), 0.0),
    "dg_D39_Kws": ("diag", "float64", 39, K_WS, 2, 2, 300, 405, (1.0,), 0.0),
}
EDGE32 = {
    "dg_D39_Klds32": ("diag", "float32", 39, K32_LDS, 2, 2, 300, 405, (1.0,), 0.0),
    "dg_D39_Kws32": ("diag", "float32", 39, K32_WS, 2, 2, 300, 405, (1.0,), 0.0),
}


def case_of(name):
    return fi.CASES[name] if name in fi.CASES else EDGE[name] if name in EDGE else EDGE32[name]


def query_rows(case, M=M_QUERY, query_seed=QUERY_SEED):
    """M rows that are not the case's: its own cluster centres (RandomState(seed), the `mu` expression of fi.case_data), z and
    the noise from RandomState(seed + query_seed), every 7th row scaled by 3 so that some queries choose an empty slot"""
    cov, dtype, D, K_max, B, S, N, seed = case[:8]
    noise = 1.0 if cov == "full" and D >= 39 else 0.3       # (fi.make_inputs)
    mu = 1.5 * np.random.RandomState(seed).randn(max(2, min(N // 8, 12, K_max - 3)), D)
    rs = np.random.RandomState(seed + query_seed)
    z = rs.randint(0, len(mu), M)
    Xq = mu[z] + noise * rs.randn(M, D)
    Xq[::7] *= 3.0
    return Xq.astype(dtype)


class Prediction(object):
    """what the specification says of a query: everything in slot order too, for the checks kept on the device's slots"""

    def __init__(self, M, K_max):
        self.ll = np.zeros((M, K_max))                      # likelihood part of the logits, slot order
        self.label = np.zeros(M, np.int64)                  # reference view's numbering
        self.slot = np.zeros(M, np.int64)                   # the winning slot
        self.density = np.zeros(M)
        self.resp = np.zeros((M, K_max))                    # reference view's column order
        self.resp_slots = np.zeros((M, K_max))              # slot order
        self.K = 0
        self.order = None                                   # column j of `resp` is slot order[j]
        self.cnt = None


def functions_of(ll, cnt, alpha, lms, out=None):
    """label / density / responsibilities of likelihood rows `ll` [M, K_max] (slot order) on counts `cnt`: the three
    definitions above, in fp64.  `census`: see predict."""
    ll = np.asarray(ll, np.float64)
    M, K_max = ll.shape
    out = Prediction(M, K_max) if out is None else out
    cnt = np.asarray(cnt)
    occ = cnt > 0
    pz = np.log(float(alpha) / K_max + cnt)                 # fbgmm.py:475-479 (no lms)
    lt = np.log(int(np.sum(cnt)) + alpha)                   # fbgmm.py:268-272
    rank = np.cumsum(occ) - occ
    out.K, out.cnt = int(occ.sum()), cnt
    out.order = np.argsort(~occ, kind="stable")
    out.ll[:] = ll
    for r in range(M):
        z = pz + ll[r]
        k = int(np.argmax(z))
        out.slot[r] = k
        out.label[r] = rank[k] if occ[k] else out.K
        out.density[r] = _sp_logsumexp(lms * (pz - lt) + ll[r])
        g = lms * pz + ll[r]
        out.resp_slots[r] = g - _sp_logsumexp(g)
        out.resp[r] = out.resp_slots[r][out.order]
    return out


def predict(spec, Xq, census=None):
    """The specification on the state of `spec` (tests/fbgmm_items.py FbgmmItems / FullcovItems, any slots).  census: a
    tests/fbgmm_items_map.py Census that takes every label decision."""
    d = spec.derive(*spec.stats_excluding(-1))
    ll = np.array([spec.loglik(d, x) for x in Xq]).reshape(len(Xq), spec.K_max)
    out = functions_of(ll, d["cnt"], spec.alpha, spec.lms)
    if census is not None:
        pz = np.log(float(spec.alpha) / spec.K_max + d["cnt"])
        for r in range(len(Xq)):
            census.decide(pz + ll[r], d["cnt"])
    return out


def appended_model(case, Xq, assignments):
    """the serial reference-pinned model over [X; Xq] with `assignments` on X and the queries at -1"""
    X, _ = fi.make_inputs(case)
    a = np.concatenate([np.asarray(assignments, np.int64), np.full(len(Xq), -1, np.int64)])
    return fi.spec_model(case[0], np.concatenate([X, Xq.astype(X.dtype)]), case[3], a)


def serial_logits(am, i, scale):
    """scale * log(alpha / K_max + counts) + the log predictive of item i of a serial model (np_oracle FBGMM, or SpecFBGMM)"""
    if hasattr(am, "_log_prob_z"):
        return am._log_prob_z(i, scale)
    return am._logits(i, with_lms=False) if scale == 1.0 else am._logits(i)


def serial_witness(am, i):
    """(map_assign_i's k -- taken without growing the model --, log_marg_i, the normalised log_prob_z of
    gibbs_sample_inside_loop_i at temperature 1) of the unassigned item i of a serial model"""
    c = am.components
    z = serial_logits(am, i, 1.0)
    k = int(np.argmax(np.exp(z - _sp_logsumexp(z))))        # fbgmm.py:485-488
    k = min(k, c.K)                                         # :489-490
    g = serial_logits(am, i, am.lms)
    return k, float(am.log_marg_i(i)), g - _sp_logsumexp(g)


_runs = {}


def swept(name, consider_unassigned=True):
    """the batch specification of a case after its own sweeps (fi.run_spec's walk; shared: do not modify)"""
    key = (name, consider_unassigned)
    if key not in _runs:
        case = case_of(name)
        spec = fi.spec_of(case)[1]
        for s, temp in enumerate(case[8]):
            spec.sweep(s, temp, consider_unassigned)
        _runs[key] = spec
    return _runs[key]

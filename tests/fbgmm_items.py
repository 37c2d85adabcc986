"""
Executable SPECIFICATION of the batch-synchronous sweep of the STAND-ALONE mixture model (`FBGMM.gibbs_sample(sync="batch")`,
`FBGMM.batch_sweep_async`).  Test infrastructure only, like tests/fullcov_batch.py and tests/anneal.py.

The sweep is the segmenter's blocked sampler (oracle/np_fbgmm_batch.py) with "utterance" read as "item".  `FbgmmItems` is
`nb.FbgmmBatch`, `FullcovItems` tests/fullcov_batch.py's `FullcovBatch`, built on a shim that stands for the segmenter: the
slice / block ranges (over items), the partial sums, `stats_excluding`, `derive`, `loglik`, `prior_z` and `canonical` are
inherited untouched.  Only what walks utterances is restated:

  tokens   item i is its own one-token "utterance" while it holds a slot (slot >= 0), and has no token otherwise
  sweep    step b: the statistics of all items outside block b; every CONSIDERED item i of block b (slot >= 0, or every
           item with `consider_unassigned`) forms z = prior_z(d, None) + loglik(d, X[i]) -- no language model --, anneals it
           as FbgmmBatch.sweep does (np_fbgmm_batch.py:286-291) and draws draw_chunked(p, u01(seed, sweep, i, 1)); all items
           of the block against the same statistics; then the block's partial sums are those of the new slots.
           An item that is unassigned and not considered keeps -1 and contributes to nothing.  No renumbering.

The counter j = 1 of u01 is N_max + t of an utterance of one landmark: with every item assigned the sweep is, draw for draw,
FbgmmBatch.sweep on N one-landmark utterances (tests/test_fbgmm_items_cpu.py holds that).

`Census` records what the parity tests rest on: how far every uniform lay from the nearest edge of its cumulative
distribution, how many draws an annealed sweep changed against T = 1 on the same state, and the slots that emptied / were
founded.
"""
import numpy as np
from scipy.special import logsumexp as _sp_logsumexp

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import fullcov_batch as fb
from tests.fullcov import SpecFBGMM, SpecPrior

BATCH_SEED = 11
DRAW_MARGIN = fb.DRAW_MARGIN     # 1e-6: a condition on the inputs, three orders above the 1e-9 of the fp64 path
TILE = 64                        # items per workgroup of k_fbi_assign
ALPHA, LMS = 1.3, 0.9

# name -> (cov, dtype, D, K_max, B, S, N, data seed, temperatures of the sweeps, fraction unassigned at the start)
CASES = {
    "fx_D3_K1_1x1": ("fixed", "float32", 3, 1, 1, 1, 40, 101, (1.0, 1.0), 0.0),                # one slot: runs of 1
    "fx_D39_K7_n255": ("fixed", "float32", 39, 7, 2, 2, 255, 202, (1.0, 1.0, 1.0), 0.0),        # cells of 63 and 64 = TILE - 1, TILE
    "dg_D39_K65_n257": ("diag", "float32", 39, 65, 2, 2, 257, 103, (1.0, 1.0, 1.0), 0.0),       # cells of 64 and 65; runs of 2
    "dg_D100_K130_T10": ("diag", "float64", 100, 130, 3, 4, 300, 104, (10.0, 10.0), 0.0),       # runs of 3; annealed
    "fx_D100_K300_Thalf": ("fixed", "float64", 100, 300, 8, 8, 700, 205, (0.5, 0.5), 0.0),      # runs of 5; logits beyond LDS
    "fx_D39_K1100": ("fixed", "float32", 39, 1100, 2, 2, 600, 3306, (1.0, 1.0), 0.0),            # runs of 18; logits beyond LDS
    "fx_D39_K130_n600": ("fixed", "float32", 39, 130, 2, 2, 600, 107, (1.0, 1.0, 1.0), 0.0),    # three tiles per cell
    "fx_D3_K7_n5_8x8": ("fixed", "float64", 3, 7, 8, 8, 5, 108, (1.0, 1.0, 1.0), 0.0),          # empty cells
    "dg_D3_K7_n1": ("diag", "float32", 3, 7, 2, 2, 1, 109, (1.0, 1.0, 1.0), 0.0),               # one item
    "dg_D39_K7_un": ("diag", "float32", 39, 7, 3, 4, 200, 710, (1.0, 1.0, 1.0), 0.3),           # a third unassigned
    "fx_D39_K65_un": ("fixed", "float64", 39, 65, 2, 2, 200, 111, (1.0, 1.0), 0.3),
    "fc_D3_K7_n5_2x2": ("full", "float32", 3, 7, 2, 2, 5, 112, (1.0, 1.0, 1.0), 0.0),
    "fc_D39_K65": ("full", "float64", 39, 65, 3, 4, 150, 113, (1.0, 1.0), 0.0),
    "fc_D64_K7_un_T10": ("full", "float32", 64, 7, 2, 2, 130, 514, (10.0, 0.5, 1.0), 0.3),      # the limit
}
# every case runs with consider_unassigned=True; these also with False (from the same start)
UNASSIGNED = ["dg_D39_K7_un", "fx_D39_K65_un", "fc_D64_K7_un_T10"]
# N <= B * S with S = 1: at most one item per block -- the statistics an item sees are the serial chain's, everything but
# itself.  (With S > 1 a block is one cell of EVERY slice and holds up to S items, which are all left out together: N <= B * S
# alone does not make the two coincide.)
SERIAL = {"ser_fx": ("fixed", "float32", 5, 6, 12, 1, 12, 121), "ser_dg": ("diag", "float64", 5, 6, 14, 1, 12, 122),
          "ser_fc": ("full", "float32", 5, 6, 12, 1, 12, 123)}


def case_data(D, K_max, N, seed, dtype, noise=0.3):
    """a mixture of fewer clusters than slots"""
    rs = np.random.RandomState(seed)
    mu = 1.5 * rs.randn(max(2, min(N // 8, 12, K_max - 3)), D)
    z = rs.randint(0, len(mu), N)
    return (mu[z] + noise * rs.randn(N, D)).astype(dtype)


def case_assignments(K_max, N, seed, unassigned, cov="fixed"):
    """consecutive labels 0..k-1 of three items each or more (half as many labels as slots; where the slots are few, two of the
    labels on one item each, so that a slot can empty), `unassigned` of the items at -1"""
    rs = np.random.RandomState(seed + 1000)
    k = max(1, min((K_max + 1) // 2, (N + 2) // 3))
    if cov == "full" and N >= 100:
        k = 2            # (two slots that mix all clusters: as wide as the prior predictive, so that slots get founded)
    if k >= 4 and N >= 8 * k:
        a = rs.randint(0, k - 2, N)
        a[rs.choice(N, 2, replace=False)] = (k - 2, k - 1)
    else:
        a = rs.randint(0, k, N)
    if unassigned:
        a[rs.rand(N) < unassigned] = -1
    present = sorted(set(a.tolist()) - {-1})
    remap = {k: j for j, k in enumerate(present)}
    return np.array([remap.get(int(k), -1) for k in a], dtype=np.int64)


def prior_params(cov, D):
    if cov == "fixed":
        return 0.1 * np.ones(D), np.zeros(D), 2.0 * np.ones(D)             # FixedVarPrior(var, mu_0, var_0)
    if cov == "diag":
        return np.zeros(D), 0.05, D + 3, 0.1 * (D + 3) * np.ones(D)        # NIW(m_0, k_0, v_0, S_0)
    return np.zeros(D), 0.05, D + 3, 0.01 * (D + 3) * np.eye(D)       # (a prior predictive as wide as the data: slots get founded)


class _Items(object):
    """what FbgmmBatch asks of a segmenter's `utterances`: their number"""

    def __init__(self, n):
        self.D = n


class _Model(object):
    """what FbgmmBatch asks of a segmenter: the acoustic model, the utterances, no language model"""

    def __init__(self, am, n):
        self.acoustic_model, self.utterances = am, _Items(n)


class Census(object):
    def __init__(self):
        self.margin = np.inf              # least distance of a uniform from an edge of its cumulative distribution
        self.draws = 0
        self.changed_by_T = []            # per sweep: draws that differ from the T = 1 draw on the same state
        self.emptied = self.founded = 0   # slots that went from occupied to empty / from empty to occupied over a sweep

    def draw(self, p, u):
        """distance of u from the nearest edge of cumsum(p) (np.cumsum accumulates left to right like utils.draw; the
        walk of draw_chunked rounds differently by ~1e-16, thirteen orders below the margin asked for)"""
        self.margin = min(self.margin, float(np.min(np.abs(u - np.cumsum(p)))))
        self.draws += 1


class _ItemSweep(object):
    census = None             # a Census
    ll_log = None             # a dict: item -> the likelihood vector its draw of the last sweep used

    def _tokens(self, i):
        return [i] if self.slot[i] >= 0 else []

    @staticmethod
    def _probabilities(z, temp):
        if temp != 1:
            z = z - _sp_logsumexp(z)
            return np.exp(1. / temp * z - _sp_logsumexp(1. / temp * z))
        return np.exp(z - _sp_logsumexp(z))

    def sweep(self, sweep_index, anneal_temp=1.0, consider_unassigned=True):
        before = self.stats_excluding(-1)[0] > 0
        changed = 0
        if self.ll_log is not None:
            self.ll_log = {}
        for b in range(self.B):
            d = self.derive(*self.stats_excluding(b))
            new = {}
            for s in range(self.S):
                for i in range(*self.ranges[s][b]):
                    if self.slot[i] < 0 and not consider_unassigned:
                        continue
                    ll = self.loglik(d, self.X[i])
                    z = self.prior_z(d, None, None, None) + ll
                    p = self._probabilities(z, anneal_temp)
                    u = nb.u01(self.seed, sweep_index, i, 1)
                    new[i] = nb.draw_chunked(p, u)
                    if self.ll_log is not None:
                        self.ll_log[i] = ll
                    if self.census is not None:
                        self.census.draw(p, u)
                        if anneal_temp != 1 and nb.draw_chunked(self._probabilities(z, 1.0), u) != new[i]:
                            changed += 1
            for i, k in new.items():      # all items of the block were sampled from the same statistics: apply
                self.slot[i] = k
            for s in range(self.S):
                self.P[s][b] = self._partial(s, b)
        if self.census is not None:
            after = self.stats_excluding(-1)[0] > 0
            self.census.emptied += int(np.count_nonzero(before & ~after))
            self.census.founded += int(np.count_nonzero(~before & after))
            self.census.changed_by_T.append(changed)


class FbgmmItems(_ItemSweep, nb.FbgmmBatch):
    """fixed-variance and diagonal components, on an oracle FBGMM"""

    def __init__(self, am, n_gibbs_blocks=8, n_stat_blocks=8, seed=0):
        nb.FbgmmBatch.__init__(self, _Model(am, am.components.N), n_gibbs_blocks=n_gibbs_blocks, n_stat_blocks=n_stat_blocks,
                               seed=seed)


class FullcovItems(_ItemSweep, fb.FullcovBatch):
    """full-covariance components, on a tests/fullcov.py SpecFBGMM"""

    def __init__(self, am, n_gibbs_blocks=8, n_stat_blocks=8, seed=0):
        fb.FullcovBatch.__init__(self, _Model(am, am.components.N), n_gibbs_blocks=n_gibbs_blocks, n_stat_blocks=n_stat_blocks,
                                 seed=seed)


def make_inputs(case):
    cov, dtype, D, K, B, S, N, seed = case[:8]
    unassigned = case[9] if len(case) > 9 else 0.0
    # (full covariance in many dimensions: clusters as wide as their distances, or no draw ever leaves the occupied slots)
    return case_data(D, K, N, seed, dtype, 1.0 if cov == "full" and D >= 39 else 0.3), case_assignments(K, N, seed, unassigned, cov)


def spec_model(cov, X, K, assignments):
    """the serial reference-pinned model of these assignments (oracle FBGMM; SpecFBGMM for full covariance)"""
    D = X.shape[1]                        # (a copy of the assignments: the components keep the array and del_item writes it)
    if cov == "full":
        return SpecFBGMM(X, SpecPrior(*prior_params(cov, D)), ALPHA, K, np.array(assignments, np.int64), lms=LMS)
    prior = no.FixedVarPrior(*prior_params(cov, D)) if cov == "fixed" else no.NIW(*prior_params(cov, D))
    return no.FBGMM(X, prior, ALPHA, K, np.array(assignments, np.int64), covariance_type=cov, lms=LMS)


def spec_of(case, assignments=None):
    """(serial model, batch specification) of a case of CASES / SERIAL"""
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, a = make_inputs(case)
    am = spec_model(cov, X, K, a if assignments is None else assignments)
    cls = FullcovItems if cov == "full" else FbgmmItems
    return am, cls(am, n_gibbs_blocks=B, n_stat_blocks=S, seed=BATCH_SEED)


def product_of(case, assignments=None, **kw):
    """The device model of the same initial state: sync="sequential" with the batch arguments (the batch sweeps are reached
    through batch_sweep_async / gibbs_sample(..., sync="batch"))."""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, a = make_inputs(case)
    prior = FixedVarPrior(*prior_params(cov, D)) if cov == "fixed" else NIW(*prior_params(cov, D))
    args = dict(covariance_type=cov, lms=LMS, sync="sequential", n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=BATCH_SEED)
    args.update(kw)
    return FBGMM(X, prior, ALPHA, K, a if assignments is None else assignments, **args)


def run_spec(name, consider_unassigned=True):
    """the specification of CASES[name] after its sweeps, with its census; the slots after every sweep in `.history`"""
    case = CASES[name]
    am, spec = spec_of(case)
    spec.census = Census()
    spec.history = []
    for s, temp in enumerate(case[8]):
        spec.sweep(s, temp, consider_unassigned)
        spec.history.append(spec.slot.copy())
    return spec

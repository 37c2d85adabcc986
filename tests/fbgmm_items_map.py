"""
Executable SPECIFICATION of the MAP sweeps of the STAND-ALONE mixture model (`FBGMM.map_assign`, `FBGMM.batch_sweep_async(...,
map_assign=True)`), batch and serial, with the census of decision margins the parity tests rest on.  Test infrastructure only,
like tests/fbgmm_items.py (the sampled sweeps) and tests/map_batch.py (the segmenter's MAP slots).

Batch MAP sweep.  `MapItems` / `MapFullcovItems` are tests/fbgmm_items.py's `FbgmmItems` / `FullcovItems` with `sweep`
overridden, and the override is `_ItemSweep.sweep` with ONE substitution: for every considered item of block b

    z_k = log(alpha / K_max + n_k) + loglik_k(x_i)        k = the first index of max_k z_k

with n_k and loglik from the statistics of all other blocks: FBGMM.map_assign_i (fbgmm.py:465-494) on slots.  No `lms` on the
prior term (fbgmm.py:475-479 has none), no temperature, no uniform, no softmax, no `k > K` clamp (batch slots are slots): the
rules of tests/map_batch.py.  All empty slots of an item tie exactly and the first one wins.  consider_unassigned, the
application of the block's new slots, the partial sums and `canonical` are inherited.  The sweep takes one value of
`sweep_index` (and reads nothing from it), so sampled sweeps after it use the uniforms they would have used.  It returns
n_moved: the considered items whose slot after the step differs from before (an unassigned item that gets a slot counts).
n_moved == 0 is a fixed point: the partial sums are rebuilt from identical slots, so every later MAP sweep is a no-op.

Serial MAP sweep.  `serial_map_sweep` is the item loop of FBGMM.gibbs_sample (fbgmm.py:352-405) with lines 371-389 replaced by
map_assign_i's 475-491, on the oracle's FBGMM (SpecFBGMM for full covariance).  Per considered item in index order:
cache_component_stats, del_item; the logits of map_assign_i, np.argmax(prob_z) (first maximum), `k > K -> K`;
restore_component_from_stats when k == k_old and K is unchanged, add_item otherwise.  The restore branch is kept on purpose: a
sweep that moves nothing leaves every statistic bit-identical.  No random.random() is consumed.  n_moved counts the items that
took the add_item branch, except a singleton that re-founds its own component (K dropped by one at del_item and the item
chose k == K).

The reference takes np.argmax(np.exp(z - logsumexp(z))); exp is monotone, so wherever the candidates are not within rounding
of each other that is the argmax of z.  `Census` records, for every decision, how far the winner lay from the best competitor
that does not tie with it exactly, whether a tie involved an occupied slot (never allowed), and whether the softmax form
agrees; tests/test_fbgmm_items_map_cpu.py holds every case to MARGIN with the oracle alone.
"""
import numpy as np
from scipy.special import logsumexp as _sp_logsumexp

from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32

MARGIN = 1e-6        # relative gap of every decision: three orders above the 1e-9 the device's fp64 likelihoods are held to
N_SWEEPS = 4         # MAP sweeps of every case

# (name, consider_unassigned) of the batch runs: every case of fbgmm_items.CASES, the UNASSIGNED ones also without
BATCH = [(name, True) for name in fi.CASES] + [(name, False) for name in fi.UNASSIGNED]
# the cases of the serial form: (name, consider_unassigned) over fbgmm_items.CASES, then the names of fbgmm_items.SERIAL
SERIAL_FORM = [("fx_D39_K7_n255", True), ("dg_D39_K65_n257", True), ("fx_D39_K65_un", True), ("fc_D3_K7_n5_2x2", True),
               ("fc_D64_K7_un_T10", True), ("fc_D64_K7_un_T10", False)]
SERIAL = list(fi.SERIAL)
# float32 likelihoods (score_precision="f32"): the cases of tests/fbgmm_items_f32.py, four MAP sweeps each
F32 = list(f32.CASES)
# sampled, sampled, MAP, MAP, sampled on one live sweeper
MIXED = ["dg_D39_K65_n257", "fc_D39_K65"]
MIXED_PLAN = (False, False, True, True, False)
# shapes on which no item can move: one slot (every item is in it or takes it), and the one-item model, whose item re-founds
# the slot it holds
DEGENERATE = ["fx_D3_K1_1x1", "dg_D3_K7_n1", "dg_D3_K1_1x1"]


def case_of(name):
    return fi.CASES[name] if name in fi.CASES else fi.SERIAL[name] if name in fi.SERIAL else f32.CASES[name]


class Census(object):
    def __init__(self):
        self.decisions = 0
        self.gap_abs = self.gap_rel = np.inf    # winner against the largest logit below it, absolute and / max(1, |z|)
        self.empty_ties = 0                     # decisions whose maximum is shared by several (empty) slots
        self.tie_on_occupied = 0                # ... shared by an occupied slot: never allowed
        self.softmax_disagrees = 0              # argmax(z) != argmax(exp(z - logsumexp z))
        self.moved = []                         # per sweep
        self.emptied = self.founded = 0         # batch: slots that went from occupied to empty / empty to occupied over a sweep

    def decide(self, z, cnt):
        self.decisions += 1
        k = int(np.argmax(z))
        at_max = np.where(z == z[k])[0]
        if len(at_max) > 1:
            self.empty_ties += 1
            self.tie_on_occupied += bool(np.any(np.asarray(cnt)[at_max] > 0))
        below = z[z < z[k]]
        if len(below):
            gap = float(z[k] - below.max())
            self.gap_abs = min(self.gap_abs, gap)
            self.gap_rel = min(self.gap_rel, gap / max(1.0, abs(float(z[k]))))
        self.softmax_disagrees += int(np.argmax(np.exp(z - _sp_logsumexp(z)))) != k


class _MapSweep(object):
    census = None             # a Census
    ll_log = None             # a dict: item -> the likelihood vector its decision of the last sweep used
    z_log = None              # a dict: item -> the prior terms pz its decision of the last sweep used (shared per block)

    def sweep(self, sweep_index, anneal_temp=1.0, consider_unassigned=True, map_assign=True):
        """One MAP sweep; returns n_moved.  map_assign=False: the sampled sweep of tests/fbgmm_items.py on the same state."""
        if not map_assign:
            return fi._ItemSweep.sweep(self, sweep_index, anneal_temp, consider_unassigned)
        before = self.stats_excluding(-1)[0] > 0
        moved = 0
        if self.ll_log is not None:
            self.ll_log, self.z_log = {}, {}
        for b in range(self.B):
            d = self.derive(*self.stats_excluding(b))
            pz = np.log(float(self.alpha) / self.K_max + d["cnt"])            # fbgmm.py:475-479: no lms
            new = {}
            for s in range(self.S):
                for i in range(*self.ranges[s][b]):
                    if self.slot[i] < 0 and not consider_unassigned:
                        continue
                    ll = self.loglik(d, self.X[i])
                    z = pz + ll
                    new[i] = int(np.argmax(z))
                    if self.ll_log is not None:
                        self.ll_log[i], self.z_log[i] = ll, pz
                    if self.census is not None:
                        self.census.decide(z, d["cnt"])
            for i, k in new.items():      # all items of the block were decided on the same statistics: apply
                moved += int(self.slot[i] != k)
                self.slot[i] = k
            for s in range(self.S):
                self.P[s][b] = self._partial(s, b)
        if self.census is not None:
            after = self.stats_excluding(-1)[0] > 0
            self.census.emptied += int(np.count_nonzero(before & ~after))
            self.census.founded += int(np.count_nonzero(~before & after))
            self.census.moved.append(moved)
        return moved


class MapItems(_MapSweep, fi.FbgmmItems):
    """fixed-variance and diagonal components"""


class MapFullcovItems(_MapSweep, fi.FullcovItems):
    """full-covariance components"""


def serial_map_sweep(am, consider_unassigned=True, census=None):
    """One serial MAP sweep of `am` (the oracle's FBGMM, or tests/fullcov.py's SpecFBGMM) in place; returns n_moved."""
    c = am.components
    full = hasattr(c, "cache")            # SpecComponents name their cache / restore differently
    moved = 0
    for i in range(c.N):
        k_old = c.assignments[i]
        if not consider_unassigned and k_old == -1:
            continue
        K_old = c.K
        stats = c.cache(k_old) if full else c.cache_component_stats(k_old)
        c.del_item(i)
        K_del = c.K
        z = am._log_prob_z(i, 1.0) if full else am._logits(i, with_lms=False)        # fbgmm.py:475-483
        k = int(np.argmax(np.exp(z - _sp_logsumexp(z))))                             # :485-488
        if census is not None:
            census.decide(z, c.counts)
        if k > K_del:
            k = K_del
        if k == k_old and K_del == K_old:
            if full:
                c.restore(k_old, stats)
            else:
                c.restore_component_from_stats(k_old, *stats)
            c.assignments[i] = k_old
        else:
            c.add_item(i, k)
            moved += not (K_del == K_old - 1 and k == K_del)
    if census is not None:
        census.moved.append(moved)
    return int(moved)


def spec_of(case, assignments=None):
    """(serial model, batch MAP specification) of a case, as fbgmm_items.spec_of builds them"""
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, a = fi.make_inputs(case)
    am = fi.spec_model(cov, X, K, a if assignments is None else assignments)
    cls = MapFullcovItems if cov == "full" else MapItems
    return am, cls(am, n_gibbs_blocks=B, n_stat_blocks=S, seed=fi.BATCH_SEED)


def partition(a):
    """labels renumbered by first occurrence (-1 stays): two labellings of one partition give the same array"""
    first = {}
    return np.array([-1 if k < 0 else first.setdefault(int(k), len(first)) for k in a], dtype=np.int64)


_runs = {}


def run_batch(name, consider_unassigned=True, n_sweeps=N_SWEEPS):
    """the batch specification of a case after its MAP sweeps, with its census; the slots after every sweep in `.history`,
    the canonical labels and K in `.canon`.  Computed once per (case, flag) and shared: do not modify."""
    key = ("batch", name, consider_unassigned, n_sweeps)
    if key not in _runs:
        am, spec = spec_of(case_of(name))
        spec.census = Census()
        spec.history, spec.canon = [], []
        for s in range(n_sweeps):
            spec.sweep(s, 1.0, consider_unassigned)
            spec.history.append(spec.slot.copy())
            spec.canon.append(spec.canonical())
        _runs[key] = spec
    return _runs[key]


class SerialRun(object):
    """a serial model after its MAP sweeps: per sweep the assignments, K, n_moved, log_marg / log_prob_z /
    log_prob_X_given_z and the number of assigned items"""

    def __init__(self, name, consider_unassigned=True, n_sweeps=N_SWEEPS):
        case = case_of(name)
        X, a = fi.make_inputs(case)
        self.am = am = fi.spec_model(case[0], X, case[3], a)
        self.census = Census()
        self.assignments, self.K, self.record, self.assigned = [], [], [], []
        for s in range(n_sweeps):
            serial_map_sweep(am, consider_unassigned, self.census)
            c = am.components
            self.assignments.append(np.array(c.assignments))
            self.K.append(int(c.K))
            self.assigned.append(int(np.count_nonzero(c.assignments != -1)))
            lz, lx = am.log_prob_z(), c.log_marg()
            self.record.append({"log_marg": lz + lx, "log_prob_z": lz, "log_prob_X_given_z": lx})
        self.moved = self.census.moved


def run_serial(name, consider_unassigned=True, n_sweeps=N_SWEEPS):
    key = ("serial", name, consider_unassigned, n_sweeps)
    if key not in _runs:
        _runs[key] = SerialRun(name, consider_unassigned, n_sweeps)
    return _runs[key]

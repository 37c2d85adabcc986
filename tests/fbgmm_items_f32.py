"""
Test infrastructure of `FBGMM(..., covariance_type="diag", sync="batch", score_precision="f32")`: the batch sweeps of the
stand-alone mixture model with the Student-t terms of the item likelihoods in float32 on the hardware logarithm
(`segk_fbi_assign_diag32`).  The specification stays tests/fbgmm_items.py (`FbgmmItems`, fp64); this module
adds

  CASES        the shapes that walk every place the kernel can go wrong, and the affine transforms (tests/affine.py) each runs
               under
  SETTLED      shapes with slots of thousands of items, where the rounding of a float32 term shows in the likelihood; compared
               on PROBES rows (`compare`, `settled_figures`), also as utterances of one landmark through the segmenter
               (`segmenter_of`)
  emulate      a NumPy emulation of the kernel's float32 terms on the specification's `derive` output: float32 subtract /
               multiply / add / log2 with the compensation of what 1 + e rounds away, a sequential float32 sum over the
               dimensions, fp64 constants -- what the contract can be checked against before a device is asked anything;
               `emulate_uncompensated`: the term as it stood before
  step / run   the specification walked one Gibbs step at a time with a hook per step (the device test keeps the specification
               on the device's own slots; the CPU test measures the emulation and the draws' margins)

The contract is the project's tolerance contract (tests/test_gpu_tolerance_modes.py): every likelihood that enters a logit
within 1e-4 max(|want|, 1) of the fp64 specification on the same statistics; statistics and draws stay fp64.
"""
import numpy as np
from scipy.special import logsumexp as _sp_logsumexp

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import affine
from tests import fbgmm_items as fi

CONTRACT = 1e-4                  # |got - want| <= CONTRACT * max(|want|, 1)
EMULATION = 5e-5                 # half of it for the float32 arithmetic itself; the other half is the hardware logarithm's
#                                  last bit and another grouping of the sum
NEAR_EDGE = 0.01                 # at most this fraction of the draws may lie within fi.DRAW_MARGIN of an edge

# the byte count of k_fbi_assign_diag32 (segmentalist_amd/csrc/segk_fbitems.hip; tests/test_fbgmm_items_f32_cpu.py holds the
# constants against the source): the (mean, q) pairs of KC slots, the tile's rows at a stride of XS floats, rounded up to 16;
# then TILE rows of K_max | 1 doubles of logits where both fit in LDS_MAX
TILE, KC, XS, LDS_MAX = fi.TILE, 32, 65, 144 * 1024


def stage_bytes(D):
    return ((2 * KC * D + XS * D) * 4 + 15) // 16 * 16


def lds_bytes(D, K_max):
    """LDS of a workgroup with the tile's logits in it"""
    return stage_bytes(D) + TILE * (K_max | 1) * 8


def k_max_either_side(D):
    """(the largest K_max whose logits stay in LDS below the first that does not, that first one)"""
    k = 1
    while lds_bytes(D, k) <= LDS_MAX:
        k += 1
    return k - 1, k


K_LDS, K_WS = k_max_either_side(39)

# name -> (cov, dtype, D, K_max, B, S, N, data seed, temperatures of the sweeps, fraction unassigned at the start): the layout
# of fi.CASES (the entries shared with it are the same inputs)
CASES = {
    "dg_D39_K65_n257": fi.CASES["dg_D39_K65_n257"],                                              # cells of 64 and 65 items
    "dg_D39_K7_n255": ("diag", "float32", 39, 7, 2, 2, 255, 417, (1.0, 1.0), 0.0),               # one cell short of a tile
    "dg_D100_K130_T10_Thalf": ("diag", "float64", 100, 130, 3, 4, 300, 104, (10.0, 0.5), 0.0),   # float64 rows, hot and cold
    "dg_D21_K9": ("diag", "float32", 21, 9, 2, 2, 150, 321, (1.0, 1.0), 0.0),                    # D = 16 + 4 + 1
    "dg_D16_K9": ("diag", "float32", 16, 9, 2, 2, 150, 316, (1.0, 1.0), 0.0),                    # D = 16 exactly
    "dg_D256_K20": ("diag", "float32", 256, 20, 2, 2, 130, 356, (1.0, 1.0, 1.0, 1.0), 0.0),      # the D limit
    "dg_D3_K1_1x1": ("diag", "float32", 3, 1, 1, 1, 40, 101, (1.0, 1.0), 0.0),                   # one slot, one block
    "dg_D3_K7_n1": fi.CASES["dg_D3_K7_n1"],                                                      # one item
    "dg_D3_K7_n5_8x8": ("diag", "float32", 3, 7, 8, 8, 5, 108, (1.0, 1.0, 1.0), 0.0),            # empty cells
    "dg_D3_K7_n40": ("diag", "float32", 3, 7, 2, 2, 40, 340, (1.0, 1.0), 0.0),                   # D = 3 with occupied slots in play
    "dg_D39_K7_un": fi.CASES["dg_D39_K7_un"],                                                    # a third unassigned
    "dg_D39_Klds": ("diag", "float32", 39, K_LDS, 2, 2, 300, 405, (1.0, 1.0), 0.0),              # the last K_max with logits in LDS
    "dg_D39_Kws": ("diag", "float32", 39, K_WS, 2, 2, 300, 405, (1.0, 1.0), 0.0),                # the first in the workspace
    "dg_D39_K300_8x8": ("diag", "float32", 39, 300, 8, 8, 700, 405, (1.0, 1.0), 0.0),            # eight tiles a block (two launches)
    "dg_D39_K1100": ("diag", "float32", 39, 1100, 2, 2, 600, 3306, (4.0, 1.0), 0.0),             # more than 1 024 slots
}
UNASSIGNED = ["dg_D39_K7_un"]            # also with consider_unassigned=False
FIVE = ["identity", "shift1", "shift16", "mfcc", "scale30"]
# scale1_64 adds D log 64 to every log-density: the values pass near zero, where the floor max(|want|, 1) of the bound makes it
# an absolute bound on half x a sum of D float32 terms, which no float32 sum meets at D >= 100 (at D = 39 the margin is 2 x).
# A property of the bound's shape (the comment above AFFINE_CASES of tests/test_gpu_tolerance_modes.py records the same), so
# scale1_64 runs at D = 3 only.
TRANSFORMS = {name: ["identity"] for name in CASES}
TRANSFORMS["dg_D39_K65_n257"] = FIVE
TRANSFORMS["dg_D100_K130_T10_Thalf"] = FIVE
TRANSFORMS["dg_D3_K7_n5_8x8"] = ["identity", "scale1_64"]        # (its five items share a block: every one against the prior)
TRANSFORMS["dg_D3_K7_n40"] = ["identity", "scale1_64"]
RUNS = [(name, t) for name in CASES for t in TRANSFORMS[name]]


# SETTLED cases: few clusters, every item in the slot of the cluster that generated it, so that a slot holds THOUSANDS of items
# -- where a float32 term's rounding, multiplied by the slot's factor (v_N + 1) / 2 ~ n_k / 2, shows in the likelihood (DESIGN.md
# 4.16.1).  fi.case_assignments mixes the clusters, and CASES holds 700 items over 300 slots at the most: neither reaches it.
# The layout of CASES with the number of clusters appended; the smallest shapes at which the term without its compensation
# (emulate_uncompensated) misses the contract by more than 3 x over all rows; eight Gibbs blocks, so that a step's statistics
# keep seven eighths of the items.  Their specification is evaluated on PROBES rows a step, never walked item by item, and they
# are held to the contract only: CASES keeps the draws' margins and the census of founded / emptied slots.
# Under `mfcc` the log-densities are larger (|ll| >= 11 against >= 0.1), the same absolute error is a smaller relative one, and
# N = 4 096 gives 3.7e-5 without the compensation -- inside the contract, so that shape could not tell the two terms apart
# there; `mfcc` runs at N = 65 536 (4.2e-4 or more on every step's probes).
SETTLED = {
    "st_D39_K8_n4096": ("diag", "float32", 39, 8, 8, 2, 4096, 7, (1.0,), 0.0, 2),
    "st_D39_K8_n65536": ("diag", "float32", 39, 8, 8, 2, 65536, 7, (1.0,), 0.0, 2),
    "st_D100_K8_n16384": ("diag", "float64", 100, 8, 8, 2, 16384, 7, (1.0,), 0.0, 3),                # float64 rows
}
SETTLED_RUNS = [("st_D39_K8_n4096", "identity"), ("st_D39_K8_n4096", "shift16"), ("st_D39_K8_n65536", "mfcc"),
                ("st_D100_K8_n16384", "identity")]
SETTLED_IDS = ["%s-%s" % r for r in SETTLED_RUNS]
PROBES = 256                     # rows a settled case is compared on
DISCRIMINATES = 2.0              # the term without its compensation misses the contract by at least this factor there


def settled_data(case, M=None, query_seed=0):
    """(rows, generating cluster) of a SETTLED case: the recipe of fi.case_data (centres 1.5 randn, noise 0.3) with the number
    of clusters the case names.  M, query_seed: M held-out rows of the same centres, z and noise from RandomState(seed +
    query_seed)."""
    cov, dtype, D, K, B, S, N, seed = case[:8]
    rs = np.random.RandomState(seed)
    mu = 1.5 * rs.randn(case[10], D)
    if M is not None:
        rs, N = np.random.RandomState(seed + query_seed), M
    z = rs.randint(0, len(mu), N)
    return (mu[z] + 0.3 * rs.randn(N, D)).astype(dtype), z.astype(np.int64)


def settled_queries(case, transform="identity", M=PROBES, query_seed=5000):
    """M held-out rows of the case's own clusters, under the transform"""
    Xq = settled_data(case, M, query_seed)[0]
    return Xq if transform == "identity" else affine.rows(Xq, *affine.params(transform, case[2]))


def probe_rows(items, m=PROBES):
    """m of the items (a number: of range(items)), evenly"""
    items = np.arange(items) if np.isscalar(items) else np.asarray(items, np.int64)
    return items[::max(1, len(items) // m)][:m]


def inputs(case, transform="identity"):
    """(X, assignments, NIW parameters) of a case under a transform: prior and data are moved together"""
    D = case[2]
    X, a = settled_data(case) if len(case) > 10 else fi.make_inputs(case)
    s, c = affine.params(transform, D)
    if transform == "identity":
        return X, a, fi.prior_params("diag", D)
    return affine.rows(X, s, c), a, affine.niw_prior(*fi.prior_params("diag", D), s, c)


def spec_of(case, transform="identity"):
    """the batch specification (fp64) of a case under a transform"""
    cov, dtype, D, K, B, S, N, seed = case[:8]
    assert cov == "diag"
    X, a, pp = inputs(case, transform)
    am = no.FBGMM(X, no.NIW(*pp), fi.ALPHA, K, np.array(a, np.int64), covariance_type="diag", lms=fi.LMS)
    return fi.FbgmmItems(am, n_gibbs_blocks=B, n_stat_blocks=S, seed=fi.BATCH_SEED)


def product_of(case, transform="identity", assignments=None, **kw):
    """the device model of the same initial state (score_precision="f32" unless `kw` says otherwise)"""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.niw import NIW
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, a, pp = inputs(case, transform)
    args = dict(covariance_type="diag", lms=fi.LMS, sync="sequential", n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=fi.BATCH_SEED,
                score_precision="f32")
    args.update(kw)
    return FBGMM(X, NIW(*pp), fi.ALPHA, K, a if assignments is None else assignments, **args)


def one_landmark_corpus(X):
    """the rows as utterances of one landmark, one span of duration 1 each, in row order: (corpus, keys)"""
    keys = ["u%07d" % i for i in range(len(X))]
    return ({k: X[i:i + 1] for i, k in enumerate(keys)}, {k: np.array([0]) for k in keys}, {k: [1] for k in keys},
            {k: [1] for k in keys}), keys


def segmenter_of(case, transform="identity", **kw):
    """The device's UNIGRAM SEGMENTER over the case's rows as utterances of one landmark (score_precision="f32", sync="batch"
    unless `kw` says otherwise), in the case's initial state: the span score of utterance i is the log marginal of row i, its
    one token row i, and the blocks are the stand-alone model's -- spec_of(case) is its specification."""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    K, B, S = case[3], case[4], case[5]
    X, a, pp = inputs(case, transform)
    corpus, keys = one_landmark_corpus(X)
    args = dict(covariance_type="diag", n_slices_min=0, n_slices_max=1, beta_sent_boundary=-1, lms=fi.LMS, sync="batch",
                n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=fi.BATCH_SEED, score_precision="f32")
    args.update(kw)
    np.random.seed(1)
    seg = UnigramAcousticWordseg(FBGMM, fi.ALPHA, K, NIW(*pp), *corpus, seed_boundaries_dict={k: [1] for k in keys},
                                 seed_assignments_dict={k: [int(a[i])] for i, k in enumerate(keys)}, **args)
    assert np.array_equal(seg.acoustic_model.components.assignments, a)
    return seg


def marginals(spec, d, ll):
    """log marginals [n] of likelihood rows ll [n, K_max] on the parameters d: nb.FbgmmBatch.log_marg without a language model
    (fbgmm.py:256-285), which is also the held-out log density of tests/fbgmm_predict.py"""
    z = spec.lms * (np.log(float(spec.alpha) / spec.K_max + d["cnt"]) - np.log(int(np.sum(d["cnt"])) + spec.alpha))
    return _sp_logsumexp(z[None, :] + np.asarray(ll, np.float64), axis=1)


def rel(got, want):
    """the contract's measure: max |got - want| / max(|want|, 1)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))) if got.size else 0.0


def centre_of(X):
    """the fp64 column mean in row order, as FbgmmItemSweeper forms it"""
    return np.add.reduce(X, axis=0, dtype=np.float64) / max(len(X), 1)


LOG2E_F = np.float32(1.4426950408889634)


def _term(e, compensated):
    """log2(1 + e) of the float32 route on float32 e >= 0 (fbb_term32 of segk_fbb_dev.h): u = 1 + e; c = e - (u - 1), the
    part of e the addition dropped (exact), taken where u < 2 and 0 beyond (there c / u is below the logarithm's own last bit
    and c alone would overstate it); term = c * LOG2E_F + log2(u), rounded once (an fma: formed in fp64 here).
    compensated=False: log2(u) alone, the arithmetic before the compensation."""
    f32 = np.float32
    u = f32(1.0) + e
    if not compensated:
        return np.log2(u)
    c = np.where(u < f32(2.0), e - (u - f32(1.0)), f32(0.0))
    return (c.astype(np.float64) * np.float64(LOG2E_F) + np.log2(u).astype(np.float64)).astype(f32)


def emulate(spec, d, rows, centre, compensated=True):
    """The likelihoods [len(rows), K_max] of the float32 route on the parameters `d` (spec.derive): per (item, slot)
    m = float32(mean - centre), q = float32(q), x = float32(X[i] - centre) (the differences in fp64), delta = m - x,
    acc += _term((delta * delta) * q) in float32, dimensions ascending, then const - half * (ln 2 * acc) in fp64; an
    empty slot: the prior predictive (fp64)."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        m = (d["mean"] - centre).astype(f32)                                   # [K, D]
        q = d["q"].astype(f32)
        x = (spec.X[rows].astype(np.float64) - centre).astype(f32)             # [n, D]
        acc = np.zeros((len(rows), spec.K_max), f32)
        for j in range(spec.D):
            delta = m[None, :, j] - x[:, None, j]
            acc = acc + _term((delta * delta) * q[None, :, j], compensated)
        ll = d["const"][None, :] - d["half"][None, :] * (0.6931471805599453 * acc.astype(np.float64))
    prior = np.array([spec.log_prior_pred(spec.X[i]) for i in rows])
    return np.where(d["active"][None, :], ll, prior[:, None])


def emulate_uncompensated(spec, d, rows, centre):
    """`emulate` with the term as it stood before the compensation, log2(1 + e): its error grows with a slot's count (1 + e
    rounds away up to 6e-8 of an e of the order of 1 / n_k, and half = (v_N + 1) / 2 multiplies that back up).  Kept to show
    that a case's inputs can tell the two apart: a condition on the inputs of the SETTLED cases."""
    return emulate(spec, d, rows, centre, compensated=False)


def set_slots(spec, slots):
    """the specification on these slots (the device's own), its partial sums rebuilt"""
    spec.slot[:] = np.asarray(slots, np.int64)
    for s in range(spec.S):
        for b in range(spec.B):
            spec.P[s][b] = spec._partial(s, b)
    return spec


def compare(spec, d, X, got=None, centre=None):
    """The fp64 specification's likelihoods [len(X), K_max] of the rows X on the parameters d, and, by the contract's measure
    over the occupied slots: (want, error of `got` or None, error of the emulation, error of the emulation without the
    compensation).  The last is the condition on the inputs of a SETTLED test: at or beyond DISCRIMINATES x CONTRACT, or the
    rows could not tell the two terms apart."""
    occ = d["active"]
    centre = centre_of(spec.X) if centre is None else centre
    want = np.array([spec.loglik(d, x) for x in X]).reshape(len(X), spec.K_max)
    rows = _Rows(spec, X)
    new, old = (rel(emulate(rows, d, range(len(X)), centre, c)[:, occ], want[:, occ]) for c in (True, False))
    return want, None if got is None else rel(np.asarray(got)[:, occ], want[:, occ]), new, old


def settled_figures(name, transform="identity"):
    """A SETTLED case at its start, before a device is asked anything: {"steps": over the probes of every Gibbs step, on the
    statistics without the step's block; "queries": the held-out rows on all statistics} -> (the emulation's error, the
    emulation's without the compensation), and the largest count"""
    case = SETTLED[name]
    spec = spec_of(case, transform)
    centre = centre_of(spec.X)
    new = old = 0.0
    for b in range(spec.B):
        d = spec.derive(*spec.stats_excluding(b))
        rows = probe_rows(considered(spec, b, True))
        _, _, e_new, e_old = compare(spec, d, spec.X[rows], centre=centre)
        new, old = max(new, e_new), max(old, e_old)
    d = spec.derive(*spec.stats_excluding(-1))
    _, _, q_new, q_old = compare(spec, d, settled_queries(case, transform), centre=centre)
    return {"steps": (new, old), "queries": (q_new, q_old)}, int(d["cnt"].max())


def discriminates(spec, what, queries=None):
    """The FIRST thing a device test of a SETTLED case does, before the device is asked anything: on the state `spec` holds,
    the emulation without the compensation over the rows the test will sample -- the probes of every Gibbs step on the
    statistics without the step's block, or `queries` on all statistics -- must miss the contract by DISCRIMINATES x or more;
    otherwise the rows could not show the defect and the case has to be chosen again.  Returns that figure."""
    centre = centre_of(spec.X)
    if queries is not None:
        plain = compare(spec, spec.derive(*spec.stats_excluding(-1)), queries, centre=centre)[3]
    else:
        plain = max(compare(spec, spec.derive(*spec.stats_excluding(b)), spec.X[probe_rows(considered(spec, b, True))],
                            centre=centre)[3] for b in range(spec.B))
    assert plain >= DISCRIMINATES * CONTRACT, "%s: the plain term gives %.3g on the sampled rows: they prove nothing" % (what, plain)
    return plain


class _Rows(object):
    """what `emulate` asks of a specification, on rows that need not be the model's"""

    def __init__(self, spec, X):
        self.X, self.K_max, self.D, self.log_prior_pred = X, spec.K_max, spec.D, spec.log_prior_pred


def considered(spec, b, consider_unassigned):
    """the items of block b the step resamples, in item order"""
    return [i for s in range(spec.S) for i in range(*spec.ranges[s][b]) if consider_unassigned or spec.slot[i] >= 0]


def margin(p, u):
    """distance of u from the nearest edge of the cumulative distribution (fi.Census.draw)"""
    return float(np.min(np.abs(u - np.cumsum(p))))


def step(spec, sweep_index, b, temp, consider_unassigned=True, likelihoods=None):
    """Gibbs step b of the specification (fi._ItemSweep.sweep, one block of it): returns (d, items, ll [n, K_max], p [n,
    K_max], u [n], new slots [n]) and applies the slots.  likelihoods(d, items) -> [n, K_max] replaces spec.loglik in the
    logits (the device's own probe rows)."""
    d = spec.derive(*spec.stats_excluding(b))
    items = considered(spec, b, consider_unassigned)
    ll = np.array([spec.loglik(d, spec.X[i]) for i in items]).reshape(len(items), spec.K_max)
    used = ll if likelihoods is None else likelihoods(d, items)
    pz = spec.prior_z(d, None, None, None)
    p = np.array([spec._probabilities(pz + used[j], temp) for j in range(len(items))]).reshape(len(items), spec.K_max)
    u = np.array([nb.u01(spec.seed, sweep_index, i, 1) for i in items])
    new = np.array([nb.draw_chunked(p[j], u[j]) for j in range(len(items))], dtype=np.int64)
    apply_slots(spec, b, items, new)
    return d, items, ll, p, u, new


def apply_slots(spec, b, items, slots):
    """the block's new slots and the partial sums they give"""
    for i, k in zip(items, slots):
        spec.slot[i] = k
    for s in range(spec.S):
        spec.P[s][b] = spec._partial(s, b)


class Run(object):
    """what the CPU test asks of a (case, transform): the emulation's worst error by the contract's measure, the draws and how
    many lay within fi.DRAW_MARGIN of an edge, slots emptied / founded, draws changed against T = 1 per sweep, the slots after
    every sweep"""

    def __init__(self):
        self.worst = 0.0
        self.draws = self.near = self.emptied = self.founded = 0
        self.changed_by_T = []
        self.history = []


def run(name, transform="identity", consider_unassigned=True):
    case = CASES[name]
    spec = spec_of(case, transform)
    centre = centre_of(spec.X)
    out = Run()
    for sweep_index, temp in enumerate(case[8]):
        before = spec.stats_excluding(-1)[0] > 0
        changed = 0
        for b in range(spec.B):
            d, items, ll, p, u, new = step(spec, sweep_index, b, temp, consider_unassigned)
            if not items:
                continue
            out.worst = max(out.worst, rel(emulate(spec, d, items, centre), ll))
            out.draws += len(items)
            out.near += sum(1 for j in range(len(items)) if margin(p[j], u[j]) < fi.DRAW_MARGIN)
            if temp != 1:
                pz = spec.prior_z(d, None, None, None)
                changed += sum(1 for j in range(len(items))
                               if nb.draw_chunked(spec._probabilities(pz + ll[j], 1.0), u[j]) != new[j])
        after = spec.stats_excluding(-1)[0] > 0
        out.emptied += int(np.count_nonzero(before & ~after))
        out.founded += int(np.count_nonzero(~before & after))
        out.changed_by_T.append(changed)
        out.history.append(spec.slot.copy())
    return out

"""
Test infrastructure of the FLOAT32 acoustic-model batch sweeps of the unigram segmenter (`FbgmmBatchSweeper.am_sweep(...,
score_precision="f32")`, `UnigramAcousticWordseg.am_batch_sweep_async(score_precision="f32")`, `gibbs_sample(...,
am_sync="batch", am_score_precision="f32")`; C entry points `segk_fbt_assign_diag32` and, for blocks of few tokens,
`segk_fbb_assign_diag32`).  The specification stays tests/am_batch.py (`AmBatch`, fp64); the emulation of the
float32 terms is tests/fbgmm_items_f32.py's `emulate`, applied to token rows with `centre_of(X)` over the whole corpus.  This
module adds

  CASES        the shapes (layout of am_batch.CASES) that walk every place the token axis of the tile kernel can go wrong, and
               the affine transforms (tests/affine.py) each runs under
  spec_of / product_of   am_batch's, with prior and data moved together under a transform
  step         one block of the specification's inner sweep with a hook for the likelihoods (the device test keeps the
               specification on the device's own probe rows and slots; the CPU test walks the emulated trajectory)

The contract is the project's tolerance contract: every likelihood that enters a logit within 1e-4 max(|want|, 1) of the fp64
specification on the same statistics; statistics and draws stay fp64.
"""
import numpy as np

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import affine
from tests import am_batch as ab
from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32

CONTRACT, EMULATION, NEAR_EDGE = f32.CONTRACT, f32.EMULATION, f32.NEAR_EDGE
DRAW_MARGIN = ab.DRAW_MARGIN
TILE, LDS_MAX = f32.TILE, f32.LDS_MAX
lds_bytes, stage_bytes, rel, centre_of, emulate, margin = (f32.lds_bytes, f32.stage_bytes, f32.rel, f32.centre_of, f32.emulate,
                                                           f32.margin)
_tiles, _ragged = ab._tiles_layout, ab._ragged_layout

# name -> cov, dtype, D, K_max, B, S, tokens of every utterance, landmarks N, window, corpus seed, temperatures of the sweeps
CASES = {
    "dg_D39_K65_tiles": ab.CASES["dg_D39_K65_tiles"],               # cells of 63, 64, 65 and 150 tokens
    "dg_D100_K7_3x4": ab.CASES["dg_D100_K7_3x4"],                   # float64 rows, T = 10
    "dg_D3_K7_1x1": ab.CASES["dg_D3_K7_1x1"],                       # one block: every token against the prior
    "dg_band_N80": ab.CASES["dg_band_N80"],                         # a band corpus, positions beyond 64, T = 0.5
    "il_dg": ab.INTERLEAVED["il_dg"],                               # (no temperatures of its own: temps_of)
    "dg_D39_K247_tiles": ("diag", "float32", 39, 247, 2, 2, _tiles(), 10, 10, 371, (1.0, 1.0)),   # last K_max with logits in LDS
    "dg_D39_K248_tiles": ("diag", "float32", 39, 248, 2, 2, _tiles(), 10, 10, 371, (1.0, 1.0)),   # first in the workspace
    # eight tiles a block: two launches at SEGK_FBI_Z_MIB=1
    "dg_D39_K300_tiles": ("diag", "float32", 39, 300, 2, 2, _tiles(), 10, 10, 373, (0.5, 1.0)),
    "dg_D256_K20_f64": ("diag", "float64", 256, 20, 2, 2, _ragged(16, 14), 10, 10, 372, (1.0, 1.0)),   # the D limit, float64 rows
    "dg_D16_K9": ("diag", "float32", 16, 9, 2, 2, _ragged(16, 15), 10, 10, 374, (1.0, 1.0)),
    "dg_D21_K9": ("diag", "float32", 21, 9, 2, 2, _ragged(16, 16), 10, 10, 375, (1.0, 1.0)),      # D = 16 + 4 + 1
    "dg_D3_K7_8x8": ("diag", "float64", 3, 7, 8, 8, _ragged(11, 7, 3), 10, 10, 376, (1.0, 1.0, 1.0)),   # empty cells
}
NO_SLOT_EMPTIED = ["dg_D256_K20_f64"]          # founds ten slots and empties none (tests/test_am_batch_f32_cpu.py prints the census)
ANNEALED = ["dg_D100_K7_3x4", "dg_band_N80", "dg_D39_K300_tiles"]
FIVE = f32.FIVE
# scale1_64 at D = 3 only: the reason stands above AFFINE_CASES of tests/test_gpu_tolerance_modes.py and above TRANSFORMS of
# tests/fbgmm_items_f32.py (near-zero log-densities make the bound absolute, which no float32 sum over many dimensions meets)
TRANSFORMS = {name: ["identity"] for name in CASES}
TRANSFORMS["dg_D39_K65_tiles"] = list(FIVE)
TRANSFORMS["dg_D100_K7_3x4"] = list(FIVE)
TRANSFORMS["dg_D3_K7_1x1"] = ["identity", "scale1_64"]
TRANSFORMS["dg_D3_K7_8x8"] = ["identity", "scale1_64"]
RUNS = [(name, t) for name in CASES for t in TRANSFORMS[name]]
# both sweeper precisions ("f64" and "f32" construction) / both routes (forced with SEGK_AM32_TILE_MIN)
BOTH_PRECISIONS = ["dg_D39_K65_tiles", "dg_band_N80", "dg_D3_K7_8x8"]
BOTH_ROUTES = ["dg_D39_K65_tiles", "dg_band_N80", "dg_D39_K300_tiles"]
TILES, SLOTS = "0", str(1 << 30)               # SEGK_AM32_TILE_MIN: always the tile kernel / never
# slots of thousands of tokens, where a float32 term's rounding is multiplied by the slot's count: the
# settled case of tests/fbgmm_items_f32.py as utterances of one landmark (f32.segmenter_of; its specification f32.spec_of --
# tests/test_fbgmm_items_cpu.py holds the item sweep to be FbgmmBatch.sweep on such utterances, draw for draw).  The cases
# above hold about five tokens a slot and cannot show it.
SETTLED = "st_D39_K8_n4096"


def temps_of(case):
    """the temperatures of a case's inner sweeps (the interleaved case brings none: two sweeps at T = 1)"""
    return tuple(case[10]) or (1.0, 1.0)


def _prior(case, transform):
    D = case[2]
    pp = fi.prior_params("diag", D)
    if transform == "identity":
        return pp
    return affine.niw_prior(*pp, *affine.params(transform, D))


def _corpus(case, transform):
    corpus = ab.case_corpus(case)
    if transform == "identity":
        return corpus
    return affine.corpus(corpus, *affine.params(transform, case[2]))


def spec_of(case, transform="identity"):
    """(specification's segmenter, AmBatch) of a case under a transform: ab.spec_of's diagonal branch, prior and data moved
    together"""
    cov, dtype, D, K, B, S = case[:6]
    assert cov == "diag"
    if transform == "identity":
        return ab.spec_of(case)
    corpus = _corpus(case, transform)
    bounds = ab.case_boundaries(case, corpus)
    np.random.seed(1)
    prior = no.NIW(*_prior(case, transform))
    seg = no.UnigramAcousticWordseg(no.FBGMM, ab.ALPHA, K, prior, *corpus, seed_boundaries_dict=bounds, **ab.seg_kwargs(case))
    u = seg.utterances
    a = -np.ones(len(seg.acoustic_model.components.X), np.int64)
    rows = [e for i in range(u.D) for e in u.get_segmented_embeds_i(i)]
    assert -1 not in rows
    a[np.array(rows, np.int64)] = ab.case_assignments(case)
    seg.acoustic_model = no.FBGMM(seg.acoustic_model.components.X, prior, ab.ALPHA, K, a, covariance_type=cov, lms=ab.LMS)
    spec = ab.AmBatch(seg, n_gibbs_blocks=B, n_stat_blocks=S, seed=ab.BATCH_SEED)
    assert [len(spec._tokens(i)) for i in range(u.D)] == list(case[6])
    return seg, spec


def product_of(case, transform="identity", seeds=None, **kw):
    """the device segmenter of the same initial state (ab.product_of under a transform); score_precision is the caller's"""
    if transform == "identity":
        return ab.product_of(case, seeds=seeds, **kw)
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    K, B, S = case[3], case[4], case[5]
    corpus = _corpus(case, transform)
    args = dict(ab.seg_kwargs(case), sync="sequential", n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=ab.BATCH_SEED)
    args.update(kw)
    np.random.seed(1)
    return UnigramAcousticWordseg(FBGMM, ab.ALPHA, K, NIW(*_prior(case, transform)), *corpus,
                                  seed_boundaries_dict=ab.case_boundaries(case, corpus),
                                  seed_assignments_dict=ab.seed_assignments(case, corpus) if seeds is None else seeds, **args)


def block_tokens(spec, b):
    """the tokens (utterance, position, row) of block b in the order of the partial sums: slice, utterance, position"""
    return [(i, t, e) for s in range(spec.S) for i in range(*spec.ranges[s][b]) for t, e in enumerate(spec._tokens(i))]


def step(spec, sweep_index, b, temp, likelihoods=None):
    """Block b of the specification's inner sweep (ab.AmSweep.am_sweep, one block of it): returns (d, tokens, ll [n, K_max]
    of the fp64 specification, p [n, K_max], u [n], new slots [n]) and applies nothing -- apply_slots does.
    likelihoods(d, tokens) -> [n, K_max] replaces spec.loglik in the logits."""
    d = spec.derive(*spec.stats_excluding(b))
    toks = block_tokens(spec, b)
    n, K = len(toks), spec.K_max
    ll = np.array([spec.loglik(d, spec.X[e]) for _, _, e in toks]).reshape(n, K)
    used = ll if likelihoods is None else np.asarray(likelihoods(d, toks)).reshape(n, K)
    pz = spec.prior_z(d, None, None, None)
    p = np.array([spec._probabilities(pz + used[j], temp) for j in range(n)]).reshape(n, K)
    N_max = spec.seg.utterances.N_max
    u = np.array([nb.u01(spec.seed, sweep_index, i, N_max + t) for i, t, _ in toks])
    new = np.array([nb.draw_chunked(p[j], u[j]) for j in range(n)], dtype=np.int64)
    return d, toks, ll, p, u, new


def apply_slots(spec, b, toks, slots):
    """the block's new slots and the partial sums they give"""
    for (_, _, e), k in zip(toks, slots):
        spec.slot[e] = k
    for s in range(spec.S):
        spec.P[s][b] = spec._partial(s, b)


class Run(object):
    """what the CPU test asks of a (case, transform), along the EMULATED trajectory (the draws use the emulation's
    likelihoods): the emulation's worst error by the contract's measure, the draws and how many lay within DRAW_MARGIN of an
    edge and the least margin, slots emptied / founded, draws changed against T = 1 per sweep, the slots after every sweep"""

    def __init__(self):
        self.worst = 0.0
        self.least = np.inf
        self.draws = self.near = self.emptied = self.founded = 0
        self.changed_by_T = []
        self.history = []


def run(name, transform="identity"):
    case = CASES[name]
    _, spec = spec_of(case, transform)
    centre = centre_of(spec.X)
    out = Run()
    for sweep_index, temp in enumerate(temps_of(case)):
        before = spec.stats_excluding(-1)[0] > 0
        changed = 0
        for b in range(spec.B):
            em = {}

            def emulated(d, toks):
                em["ll"] = emulate(spec, d, [e for _, _, e in toks], centre) if toks else np.zeros((0, spec.K_max))
                return em["ll"]
            d, toks, ll, p, u, new = step(spec, sweep_index, b, temp, emulated)
            if toks:
                out.worst = max(out.worst, rel(em["ll"], ll))
                out.draws += len(toks)
                ms = [margin(p[j], u[j]) for j in range(len(toks))]
                out.least = min(out.least, min(ms))
                out.near += sum(1 for m in ms if m < DRAW_MARGIN)
                if temp != 1:
                    pz = spec.prior_z(d, None, None, None)
                    changed += sum(1 for j in range(len(toks))
                                   if nb.draw_chunked(spec._probabilities(pz + em["ll"][j], 1.0), u[j]) != new[j])
            apply_slots(spec, b, toks, new)
        after = spec.stats_excluding(-1)[0] > 0
        out.emptied += int(np.count_nonzero(before & ~after))
        out.founded += int(np.count_nonzero(~before & after))
        out.changed_by_T.append(changed)
        out.history.append(spec.slot.copy())
    return out


# ---- a settled MULTI-LANDMARK corpus: SETTLED above reaches every float32 kernel at large counts, but with one token and one span
# an utterance.  Here 800 utterances of eight landmarks and a window of three (21 spans each: rows of three durations in one
# score tile, three to eight tokens an utterance in the token kernels), the rows from TWO cluster centres, every token in the slot of its row's centre: two slots of about 2 000 tokens.
# cov, dtype, D, K_max, B, S, tokens of every utterance, landmarks N, window, corpus seed, temperatures (the layout of CASES)
SETTLED_SEG = ("diag", "float32", 39, 6, 4, 2, [8, 4, 5, 3, 6] * 160, 8, 3, 377, (1.0,))
N_CENTRES = 2
# rows: unit vectors times ROW_SCALE sqrt(D).  The contract's measure is relative to max(|want|, 1): at ab.SCALE = 1.5 the span
# scores lie near -18 and the plain term's error (the same absolute size) is 4e-5 of them, inside the contract -- such a corpus
# could not show the defect; at 0.8 they lie near -3 and the plain term misses by 3.3e-4 or more on every block's probes
# (tests/test_am_batch_f32_cpu.py holds that)
ROW_SCALE = 0.8


def settled_seg_corpus(case=SETTLED_SEG):
    """ab.case_corpus with N_CENTRES cluster centres, at ROW_SCALE"""
    cov, dtype, D, K, B, S, tokens, N, nmax, cseed = case[:10]
    corpus = ab.fl.corpus_of(dict(n_utt=len(tokens), D=D, K=2 * N_CENTRES, cseed=cseed, N=N, nmax=nmax))
    mats = {k: (ROW_SCALE * np.sqrt(D) * np.asarray(v, np.float64)).astype(dtype) for k, v in corpus[0].items()}
    return (mats,) + tuple(corpus[1:])


def settled_seg_spec(case=SETTLED_SEG):
    """(corpus, boundaries, AmBatch) of the settled start: a32.spec_of's construction with every token labelled by the centre
    its row lies nearest to (the centres: the first draw of synth.make_corpus' generator, as directions)"""
    cov, dtype, D, K, B, S, tokens, N, nmax, cseed = case[:10]
    corpus = settled_seg_corpus(case)
    bounds = ab.case_boundaries(case, corpus)
    np.random.seed(1)
    prior = no.NIW(*fi.prior_params("diag", D))
    seg = no.UnigramAcousticWordseg(no.FBGMM, ab.ALPHA, K, prior, *corpus, seed_boundaries_dict=bounds, **ab.seg_kwargs(case))
    u = seg.utterances
    X = seg.acoustic_model.components.X
    mu = np.random.RandomState(cseed).randn(N_CENTRES, D)
    rows = np.array([e for i in range(u.D) for e in u.get_segmented_embeds_i(i)], np.int64)
    assert -1 not in rows
    a = -np.ones(len(X), np.int64)
    a[rows] = np.argmax(X[rows].astype(np.float64) @ mu.T, axis=1)
    seg.acoustic_model = no.FBGMM(X, prior, ab.ALPHA, K, a, covariance_type=cov, lms=ab.LMS)
    spec = ab.AmBatch(seg, n_gibbs_blocks=B, n_stat_blocks=S, seed=ab.BATCH_SEED)
    assert [len(spec._tokens(i)) for i in range(u.D)] == list(tokens)
    return corpus, bounds, spec


def settled_seg_product(case, corpus, bounds, spec, **kw):
    """the device segmenter of the same start (score_precision="f32", sync="batch" unless `kw` says otherwise)"""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    D, K, B, S = case[2], case[3], case[4], case[5]
    args = dict(ab.seg_kwargs(case), sync="batch", n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=ab.BATCH_SEED, score_precision="f32")
    args.update(kw)
    np.random.seed(1)
    return UnigramAcousticWordseg(FBGMM, ab.ALPHA, K, NIW(*fi.prior_params("diag", D)), *corpus, seed_boundaries_dict=bounds,
                                  seed_assignments_dict=ab.seeds_from(spec, spec.slot), **args)


def block_span_rows(spec, b):
    """the embedding rows of every span of the utterances of block b (slice order), with the span's duration"""
    u = spec.seg.utterances
    out = []
    for s in range(spec.S):
        for i in range(*spec.ranges[s][b]):
            n = u.lengths[i]
            for j in range(n * (n + 1) // 2):
                if u.vec_ids[i, j] != -1 and not np.isnan(u.durations[i, j]):
                    out.append((int(u.vec_ids[i, j]), float(u.durations[i, j])))
    return out


def settled_seg_figures(spec, b, centre, rows=None):
    """block b of the settled start: the probed span rows, the fp64 span scores (log marginals) and likelihoods of those rows on
    the statistics without the block, and the error of the emulation / of the emulation without the compensation on the span
    scores, by the contract's measure: (d, rows, want_ll, want_score, emulated, plain)"""
    d = spec.derive(*spec.stats_excluding(b))
    if rows is None:
        rows = f32.probe_rows(np.array([e for e, _ in block_span_rows(spec, b)], np.int64))
    want, _, _, _ = f32.compare(spec, d, spec.X[rows], None, centre)
    want_score = np.array([spec.log_marg(d, spec.X[e]) for e in rows])
    view = f32._Rows(spec, spec.X[rows])
    new, old = (rel(f32.marginals(spec, d, emulate(view, d, range(len(rows)), centre, c)), want_score) for c in (True, False))
    return d, rows, want, want_score, new, old

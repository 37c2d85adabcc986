"""
Executable SPECIFICATION of the ACOUSTIC-MODEL batch sweep of the unigram segmenter (`FbgmmBatchSweeper.am_sweep`,
`UnigramAcousticWordseg.am_batch_sweep_async`, `gibbs_sample(..., am_n_iter=m, sync="batch", am_sync="batch")`): the batch
form of the inner sweeps `FBGMM.gibbs_sample(m, consider_unassigned=False)` the reference runs over the currently assigned
tokens before every segmentation sweep (unigram_acoustic_wordseg.py:440-443).  Test infrastructure only, like
tests/fbgmm_items.py and tests/fullcov_batch.py.

The sweep is `nb.FbgmmBatch.sweep` with its steps 2-3 (span scores, boundaries) left out and the boundaries untouched.  The
slice / block ranges, the partial sums, `stats_excluding`, `derive`, `loglik`, `prior_z`, `_tokens` and `canonical` are
inherited; `AmSweep` is a mix-in over `nb.FbgmmBatch` (fixed, diag) and tests/fullcov_batch.py's `FullcovBatch` (full):

  am_sweep  step b: d = derive(stats_excluding(b)); every token (i, t) of the block's utterances -- the utterance's current
            tokens `_tokens(i)` in order, t their position -- forms z = prior_z(d, None, None, None) + loglik(d, X[e]), is
            annealed exactly as np_fbgmm_batch.py:286-291 when T != 1, and draws draw_chunked(p, u01(seed, sweep, i, N_max + t));
            all tokens of the block against the same statistics; then P[s][b] = _partial(s, b).
            No token is added or removed, log_probs and boundaries are not written, there is no language model.

The sweep index is the caller's: the device keeps ONE counter for outer and inner sweeps, so the uniform streams never repeat.

`Census` (tests/fbgmm_items.py's) records what the parity tests rest on: the least distance of a uniform from an edge of its
cumulative distribution, the draws an annealed sweep changed against T = 1 on the same state, the slots emptied / founded.

The CASES are corpora of segmentalist_amd.synth.make_corpus through tests/fbgmm_long.corpus_of (N landmarks per utterance,
a window as long as the utterance: every segmentation has an embedding per segment; the band case: a window of six) whose
`seed_boundaries_dict` fixes the token count of every (slice, block) cell exactly, and whose assignments are chosen like
tests/fbgmm_items.case_assignments (half as many labels as slots, two of them on one token each: slots empty and are founded).
"""
import numpy as np
from scipy.special import logsumexp as _sp_logsumexp

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import fbgmm_items as fi
from tests import fbgmm_long as fl
from tests import fullcov_batch as fb
from tests import fullcov_wordseg as fw
from tests.fullcov import SpecPrior

BATCH_SEED = fi.BATCH_SEED
DRAW_MARGIN = fb.DRAW_MARGIN     # 1e-6, the project's constant
TILE = fi.TILE                   # tokens per workgroup of the tile kernel
ALPHA, LMS = fi.ALPHA, fi.LMS
Census = fi.Census
SCALE = 1.5                      # rows of the corpora: unit vectors times SCALE sqrt(D)


class AmSweep(object):
    census = None             # a Census
    ll_log = None             # a dict: (utterance, position) -> the likelihood vector the token's draw of the last sweep used

    @staticmethod
    def _probabilities(z, temp):
        if temp != 1:         # np_fbgmm_batch.py:286-291
            z = z - _sp_logsumexp(z)
            return np.exp(1. / temp * z - _sp_logsumexp(1. / temp * z))
        return np.exp(z - _sp_logsumexp(z))

    def am_sweep(self, sweep_index, anneal_temp=1.0):
        assert self.lm is None and self.world == 1
        u = self.seg.utterances
        before = self.stats_excluding(-1)[0] > 0
        changed = 0
        if self.ll_log is not None:
            self.ll_log = {}
        for b in range(self.B):
            d = self.derive(*self.stats_excluding(b))
            new = {}
            for s in range(self.S):
                for i in range(*self.ranges[s][b]):
                    for t, e in enumerate(self._tokens(i)):
                        ll = self.loglik(d, self.X[e])
                        z = self.prior_z(d, None, None, None) + ll
                        p = self._probabilities(z, anneal_temp)
                        uu = nb.u01(self.seed, sweep_index, i, u.N_max + t)
                        new[e] = nb.draw_chunked(p, uu)
                        if self.ll_log is not None:
                            self.ll_log[(i, t)] = ll
                        if self.census is not None:
                            self.census.draw(p, uu)
                            if anneal_temp != 1 and nb.draw_chunked(self._probabilities(z, 1.0), uu) != new[e]:
                                changed += 1
            for e, k in new.items():      # all tokens of the block were sampled from the same statistics: apply
                self.slot[e] = k
            for s in range(self.S):
                self.P[s][b] = self._partial(s, b)
        if self.census is not None:
            after = self.stats_excluding(-1)[0] > 0
            self.census.emptied += int(np.count_nonzero(before & ~after))
            self.census.founded += int(np.count_nonzero(~before & after))
            self.census.changed_by_T.append(changed)


class AmBatch(AmSweep, nb.FbgmmBatch):
    """fixed-variance and diagonal components, on an oracle UnigramAcousticWordseg"""


class AmFullcovBatch(AmSweep, fb.FullcovBatch):
    """full-covariance components, on a tests/fullcov_wordseg.py SpecWordseg"""


# ------------------------------------------------------------------------------------------------------------------ cases
def _spread(total, n, most):
    """n token counts in 1..most that sum to `total`, as even as they come"""
    assert n <= total <= n * most
    base, extra = divmod(total, n)
    return [base + 1] * extra + [base] * (n - extra)


def _tiles_layout():
    """2 x 2 cells of 20 utterances of ten landmarks: 63, 64, 65 and 150 tokens (TILE - 1, TILE, TILE + 1, three tiles).  The
    first cell holds an utterance that is all one segment, the last one ten with a boundary at every landmark."""
    first = [1] + _spread(62, 19, 10)
    return first + _spread(64, 20, 10) + _spread(65, 20, 10) + [10] * 10 + [5] * 10


def _ragged_layout(n, seed, most=10):
    return [int(v) for v in np.random.RandomState(seed).randint(1, most + 1, n)]


# name -> cov, dtype, D, K_max, B, S, tokens of every utterance, landmarks N, window, corpus seed, temperatures of the sweeps
CASES = {
    "fx_D3_K1_1x1": ("fixed", "float32", 3, 1, 1, 1, [1, 3, 10, 2], 10, 10, 301, (1.0, 1.0)),
    "fx_D39_K7_tiles": ("fixed", "float32", 39, 7, 2, 2, _tiles_layout(), 10, 10, 302, (1.0, 1.0, 1.0)),
    "dg_D39_K65_tiles": ("diag", "float32", 39, 65, 2, 2, _tiles_layout(), 10, 10, 303, (1.0, 1.0)),
    "dg_D100_K7_3x4": ("diag", "float64", 100, 7, 3, 4, _ragged_layout(30, 4), 10, 10, 304, (10.0, 1.0)),
    "fx_D100_K65_3x4": ("fixed", "float64", 100, 65, 3, 4, _ragged_layout(30, 5), 10, 10, 305, (10.0, 1.0)),
    "fx_D39_K300_tiles": ("fixed", "float32", 39, 300, 2, 2, _tiles_layout(), 10, 10, 306, (0.5, 1.0)),      # logits beyond LDS
    "fx_D3_K7_8x8": ("fixed", "float64", 3, 7, 8, 8, _ragged_layout(11, 7, 3), 10, 10, 307, (1.0, 1.0, 1.0)),  # empty cells
    "dg_D3_K7_1x1": ("diag", "float32", 3, 7, 1, 1, [2, 5, 1], 10, 10, 308, (1.0, 1.0, 1.0)),                # one block: the prior
    "fc_D39_K7_2x2": ("full", "float32", 39, 7, 2, 2, _ragged_layout(16, 9), 10, 10, 354, (1.0, 1.0, 1.0)),
    "fc_D64_K65_3x4": ("full", "float64", 64, 65, 3, 4, _ragged_layout(30, 10), 10, 10, 310, (10.0, 1.0)),   # the limit
    # a band corpus: 80 landmarks, a window of six; utterances with a boundary at every landmark hold positions t beyond 64
    "dg_band_N80": ("diag", "float32", 8, 10, 2, 2, [80, 14, 40, 80, 20, 80, 27, 16], 80, 6, 360, (1.0, 0.5, 1.0)),
}
# one utterance per block (S = 1, B = utterances): the statistics a token sees are everything but its own utterance
SERIAL = {
    "ser_fx": ("fixed", "float32", 5, 6, 6, 1, [3, 1, 4, 2, 5, 2], 6, 6, 321, ()),
    "ser_dg": ("diag", "float64", 5, 6, 6, 1, [2, 3, 1, 6, 2, 4], 6, 6, 322, ()),
    "ser_fc": ("full", "float32", 5, 6, 5, 1, [3, 2, 4, 1, 5], 6, 6, 323, ()),
}
# the interleaving / re-entry / checkpoint tests run outer sweeps too
INTERLEAVED = {
    "il_dg": ("diag", "float32", 8, 10, 2, 2, _ragged_layout(12, 12, 8), 8, 8, 331, ()),
    "il_fc": ("full", "float32", 8, 10, 2, 3, _ragged_layout(12, 13, 8), 8, 8, 332, ()),
}


def case_corpus(case):
    """(embedding_mats, vec_ids_dict, durations_dict, landmarks_dict) of tests/fbgmm_long.corpus_of, the rows in the case's dtype"""
    cov, dtype, D, K, B, S, tokens, N, nmax, cseed = case[:10]
    corpus = fl.corpus_of(dict(n_utt=len(tokens), D=D, K=max(K, 8), cseed=cseed, N=N, nmax=nmax))
    # (make_corpus normalises its rows; spread like tests/fbgmm_items.case_data -- centres 1.5 apart per dimension -- a slot
    # that mixes clusters is wider than the prior predictive, and slots get founded)
    mats = {k: (SCALE * np.sqrt(D) * np.asarray(v, np.float64)).astype(dtype) for k, v in corpus[0].items()}
    return (mats,) + tuple(corpus[1:])


def case_boundaries(case, corpus):
    """seed_boundaries_dict: utterance j gets tokens[j] segments -- boundaries at evenly spread landmarks, the last one among
    them -- none longer than the window"""
    tokens, N, nmax = case[6], case[7], case[8]
    out = {}
    for j, key in enumerate(sorted(corpus[0])):
        n = tokens[j]
        idx = sorted({((q + 1) * N) // n - 1 for q in range(n)})
        assert len(idx) == n and idx[-1] == N - 1 and max(np.diff([-1] + idx)) <= nmax
        lm = corpus[3][key]
        out[key] = [lm[q] for q in idx]
    return out


def case_assignments(case):
    """one label per token in token order (tests/fbgmm_items.case_assignments on the number of tokens)"""
    cov, K, tokens, cseed = case[0], case[3], case[6], case[9]
    return fi.case_assignments(K, int(sum(tokens)), cseed, 0.0, cov)


def seed_assignments(case, corpus):
    a = case_assignments(case)
    out, at = {}, 0
    for j, key in enumerate(sorted(corpus[0])):
        out[key] = [int(k) for k in a[at:at + case[6][j]]]
        at += case[6][j]
    return out


def seg_kwargs(case):
    return dict(covariance_type=case[0], n_slices_min=0, n_slices_max=case[8], beta_sent_boundary=-1, lms=LMS, wip=0.0,
                fb_type="standard", time_power_term=1.0)


def spec_of(case, B=None, S=None):
    """(specification's segmenter, AmBatch / AmFullcovBatch) of a case"""
    cov, dtype, D, K = case[:4]
    B, S = case[4] if B is None else B, case[5] if S is None else S
    corpus = case_corpus(case)
    bounds, seeds = case_boundaries(case, corpus), seed_assignments(case, corpus)
    np.random.seed(1)
    if cov == "full":
        seg = fw.SpecWordseg(ALPHA, K, SpecPrior(*fi.prior_params(cov, D)), *corpus, seed_boundaries_dict=bounds,
                             seed_assignments_dict=seeds, **seg_kwargs(case))
        spec = AmFullcovBatch(seg, n_gibbs_blocks=B, n_stat_blocks=S, seed=BATCH_SEED)
    else:
        prior = no.FixedVarPrior(*fi.prior_params(cov, D)) if cov == "fixed" else no.NIW(*fi.prior_params(cov, D))
        seg = no.UnigramAcousticWordseg(no.FBGMM, ALPHA, K, prior, *corpus, seed_boundaries_dict=bounds, **seg_kwargs(case))
        # (its constructor draws the assignments: the case's take their place)
        u = seg.utterances
        a = -np.ones(len(seg.acoustic_model.components.X), np.int64)
        rows = [e for i in range(u.D) for e in u.get_segmented_embeds_i(i)]
        assert -1 not in rows
        a[np.array(rows, np.int64)] = case_assignments(case)
        seg.acoustic_model = no.FBGMM(seg.acoustic_model.components.X, prior, ALPHA, K, a, covariance_type=cov, lms=LMS)
        spec = AmBatch(seg, n_gibbs_blocks=B, n_stat_blocks=S, seed=BATCH_SEED)
    assert [len(spec._tokens(i)) for i in range(seg.utterances.D)] == list(case[6])
    return seg, spec


def seeds_from(spec, assignments):
    """seed_assignments_dict of the specification's current tokens labelled by `assignments` (an array over the rows)"""
    keys = spec.seg.ids_to_utterance_labels
    return {key: [int(assignments[e]) for e in spec._tokens(i)] for i, key in enumerate(keys)}


def product_of(case, B=None, S=None, seeds=None, bounds=None, **kw):
    """The device segmenter of the same initial state: sync="sequential" with the batch arguments.  seeds / bounds: other
    assignments (seeds_from) / boundaries (seed_boundaries_dict) than the case's."""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    cov, dtype, D, K = case[:4]
    B, S = case[4] if B is None else B, case[5] if S is None else S
    corpus = case_corpus(case)
    prior = FixedVarPrior(*fi.prior_params(cov, D)) if cov == "fixed" else NIW(*fi.prior_params(cov, D))
    args = dict(seg_kwargs(case), sync="sequential", n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=BATCH_SEED)
    args.update(kw)
    np.random.seed(1)
    return UnigramAcousticWordseg(FBGMM, ALPHA, K, prior, *corpus,
                                  seed_boundaries_dict=case_boundaries(case, corpus) if bounds is None else bounds,
                                  seed_assignments_dict=seed_assignments(case, corpus) if seeds is None else seeds, **args)


def cell_tokens(spec):
    """tokens of every (slice, block) cell"""
    return [[sum(len(spec._tokens(i)) for i in range(*spec.ranges[s][b])) for b in range(spec.B)] for s in range(spec.S)]


def run_spec(name):
    """the specification of CASES[name] after its inner sweeps, with its census; the slots after every sweep in `.history`"""
    case = CASES[name]
    seg, spec = spec_of(case)
    spec.census = Census()
    spec.history = []
    spec.bounds0 = seg.utterances.boundaries.copy()
    spec.tokens0 = [list(spec._tokens(i)) for i in range(seg.utterances.D)]
    for s, temp in enumerate(case[10]):
        spec.am_sweep(s, temp)
        spec.history.append(spec.slot.copy())
    return spec

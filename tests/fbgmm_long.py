"""Corpora and segmenter pairs of the batch sampler's long-utterance tests (more than 64 landmarks per utterance):
tests/test_fbgmm_batch_long_cpu.py checks, with the oracle alone, that every corpus exercises what it is there for;
tests/test_gpu_fbgmm_batch_long.py runs the device against the specification on the same corpora.

The pairs are built as tests/test_gpu_fbgmm_batch.py::_pair builds them, from segmentalist_amd.synth.make_corpus directly
(tests/golden/cases.chain_corpus fixes ragged lengths at 3..9 landmarks)."""
import random

import numpy as np

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests.golden import cases

# name -> kind, corpus (n_utt, D, K, cseed, N or N_range), window, blocks B x slices S, segmenter keywords
CASES = {
    # short and long utterances in one block (corpus seeds with an utterance no longer than the window among them)
    "ragged_fixed": dict(kind="fixed", n_utt=16, D=8, K=10, cseed=110, N_range=(3, 150), nmax=6, B=3, S=4),
    "ragged_diag": dict(kind="diag", n_utt=16, D=8, K=10, cseed=102, N_range=(3, 150), nmax=6, B=3, S=4),
    "ragged_bigram": dict(kind="bigram", n_utt=16, D=8, K=10, cseed=109, N_range=(3, 150), nmax=5, B=3, S=4),
    # the kernels are chosen per corpus (N_max > 64): the same builders at N_max <= 64 take the triangular kernel as before
    "short_fixed": dict(kind="fixed", n_utt=16, D=8, K=10, cseed=101, N_range=(3, 64), nmax=6, B=3, S=4),
    "short_diag": dict(kind="diag", n_utt=16, D=8, K=10, cseed=102, N_range=(3, 64), nmax=6, B=3, S=4),
    "short_bigram": dict(kind="bigram", n_utt=16, D=8, K=10, cseed=103, N_range=(3, 64), nmax=5, B=3, S=4),
    # the smallest band corpus, N_max = 65: the token lists' second chunk of 64 flags holds a single landmark, and an utterance
    # of two landmarks, shorter than the window, reads only the band's -1 padded rows
    "diag_65": dict(kind="diag", n_utt=12, D=8, K=10, cseed=168, N_range=(2, 65), nmax=6, B=2, S=2),
    # the stated upper end
    "fixed_256": dict(kind="fixed", n_utt=6, D=8, K=10, cseed=104, N=256, nmax=6, B=2, S=2),
    # windows beyond one DPP row of sixteen lanes and beyond 32 lanes
    "diag_100_w20": dict(kind="diag", n_utt=8, D=8, K=10, cseed=105, N=100, nmax=20, B=2, S=2),
    "fixed_100_w40": dict(kind="fixed", n_utt=8, D=8, K=10, cseed=106, N=100, nmax=40, B=2, S=2),
    # 150 tokens per utterance (p_boundary_init < 1: the initial-boundary rejection loop does not end for a window of one)
    "fixed_150_w1": dict(kind="fixed", n_utt=8, D=8, K=10, cseed=107, N=150, nmax=1, B=2, S=2, kw=dict(p_boundary_init=1.0)),
    # NaN durations: windows whose every candidate is -inf
    "diag_mindur": dict(kind="diag", n_utt=8, D=8, K=10, cseed=108, N_range=(60, 200), nmax=6, B=2, S=2,
                        kw=dict(min_duration=9)),
    # ... and the back-tracking branch of the backward pass, which min_duration = 9 cannot reach on these corpora (see
    # test_fbgmm_batch_long_cpu.py).  With a floor of 30 frames an utterance whose last six slices are shorter than that
    # has a dead end at its last landmark; corpus seed 110 was picked on the CPU: it has such utterances and none whose
    # FIRST six slices are that short (those have no valid segmentation at all: the oracle's assertion, status bit 16).
    "diag_mindur_backtrack": dict(kind="diag", n_utt=8, D=8, K=10, cseed=110, N_range=(60, 200), nmax=6, B=2, S=2,
                                  kw=dict(min_duration=30)),
    # tolerance modes
    "fixed_f32": dict(kind="fixed", n_utt=16, D=8, K=10, cseed=110, N_range=(3, 150), nmax=6, B=3, S=4, prec="f32"),
    "diag_f32": dict(kind="diag", n_utt=16, D=8, K=10, cseed=102, N_range=(3, 150), nmax=6, B=3, S=4, prec="f32"),
    # ... with the matrix-core token likelihoods of the assignment step (rows utterance * N_max + position) and, with a
    # language model, the one-wave-per-utterance assignment kernel
    "fixed_f16": dict(kind="fixed", n_utt=16, D=12, K=10, cseed=110, N_range=(3, 150), nmax=6, B=3, S=4, prec="f16"),
    "bigram_f16": dict(kind="bigram", n_utt=16, D=12, K=10, cseed=109, N_range=(3, 150), nmax=5, B=3, S=4, prec="f16"),
    # a bank of 300 slots: the partial sums through the counting sort (k_fbb_sort walks token positions utterance * N_max + j)
    "fixed_K300": dict(kind="fixed", n_utt=16, D=8, K=300, cseed=110, N_range=(3, 150), nmax=6, B=3, S=4),
}


def corpus_of(case):
    from segmentalist_amd.synth import make_corpus
    c = CASES[case] if isinstance(case, str) else case
    if "N_range" in c:
        return make_corpus(c["n_utt"], c["D"], c["K"], seed=c["cseed"], ragged=True, n_slices_max=c["nmax"],
                           N_range=c["N_range"])
    return make_corpus(c["n_utt"], c["D"], c["K"], seed=c["cseed"], N=c["N"], n_slices_max=c["nmax"])


def seg_args(c):
    args = dict(n_slices_min=0, n_slices_max=c["nmax"], p_boundary_init=0.5, beta_sent_boundary=-1, lms=1.0, wip=0.0,
                init_am_assignments="rand", time_power_term=1.0)
    args.update(c.get("kw", {}))
    return args


def oracle_of(case, corpus=None, seed=5):
    """(oracle segmenter, batch specification) of a case."""
    c = CASES[case] if isinstance(case, str) else case
    corpus = corpus_of(c) if corpus is None else corpus
    D, K = c["D"], c["K"]
    fixed, niw = cases.fixed_prior_params(D), cases.diag_prior_params(D)
    random.seed(seed)
    np.random.seed(seed)
    if c["kind"] == "bigram":
        ref = no.BigramAcousticWordseg(K, no.FixedVarPrior(*fixed), dict(cases.BIGRAM_LM), *corpus, covariance_type="fixed",
                                       fb_type="unigram", **seg_args(c))
    else:
        prior = no.FixedVarPrior(*fixed) if c["kind"] == "fixed" else no.NIW(*niw)
        ref = no.UnigramAcousticWordseg(no.FBGMM, 1.0, K, prior, *corpus, covariance_type=c["kind"], fb_type="standard",
                                        **seg_args(c))
    return ref, nb.FbgmmBatch(ref, n_gibbs_blocks=c["B"], n_stat_blocks=c["S"], seed=11)


def product_of(case, corpus=None, seed=5, process_group=None):
    """The product's segmenter of a case, from the same initial state as oracle_of's."""
    from segmentalist_amd import bigram_acoustic_wordseg as baw, fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    c = CASES[case] if isinstance(case, str) else case
    corpus = corpus_of(c) if corpus is None else corpus
    D, K = c["D"], c["K"]
    fixed, niw = cases.fixed_prior_params(D), cases.diag_prior_params(D)
    bargs = dict(sync="batch", n_gibbs_blocks=c["B"], n_stat_blocks=c["S"], batch_seed=11, score_precision=c.get("prec", "f64"))
    if process_group is not None:
        bargs["process_group"] = process_group
    random.seed(seed)
    np.random.seed(seed)
    if c["kind"] == "bigram":
        return baw.BigramAcousticWordseg(K, FixedVarPrior(*fixed), dict(cases.BIGRAM_LM), *corpus, covariance_type="fixed",
                                         fb_type="unigram", **seg_args(c), **bargs)
    prior = FixedVarPrior(*fixed) if c["kind"] == "fixed" else NIW(*niw)
    return uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, prior, *corpus, covariance_type=c["kind"], fb_type="standard",
                                      **seg_args(c), **bargs)


class DpCensus(object):
    """Counts, inside the oracle's forward_backward, the forward steps whose every candidate is -inf and the calls whose
    backward pass steps back from a dead end (unigram_acoustic_wordseg.py:718-730); use as a context manager."""

    def __enter__(self):
        self.dead_windows = self.backtracks = self.calls = 0
        self._orig = no.forward_backward
        census = self

        def counted(vec, log_p_continue, N, n_slices_min=0, n_slices_max=0, *a, **kw):
            census.calls += 1
            alpha = np.ones(N)
            alpha[0] = 0.0
            i = 0
            for t in range(1, N):
                q = no._win(vec, t, i, n_slices_max) + (alpha[:t][-n_slices_max:] if n_slices_max else alpha[:t])
                dead = bool(np.all(q == -np.inf))
                census.dead_windows += dead
                alpha[t] = -np.inf if dead else no.logsumexp(q) + log_p_continue
                i += t
            lp, bnd = census._orig(vec, log_p_continue, N, n_slices_min, n_slices_max, *a, **kw)
            # a dead end leaves a boundary that no chosen segment accounts for: the chosen segments' windows, walked from
            # the end, hit an all -inf one exactly when the reference steps back
            t = N
            while t > 0:
                i = (t - 1) * t // 2
                q = no._win(vec, t, i, n_slices_max) + (alpha[:t][-n_slices_max:] if n_slices_max else alpha[:t])
                if np.all(q == -np.inf):
                    census.backtracks += 1
                    break
                s = t - 1
                while s > 0 and not bnd[s - 1]:
                    s -= 1
                t = s
            return lp, bnd

        no.forward_backward = counted
        return self

    def __exit__(self, *exc):
        no.forward_backward = self._orig
        return False


def longest(ref):
    return int(np.max(ref.utterances.lengths))


def tokens_per_utterance(ref):
    u = ref.utterances
    return [int(np.count_nonzero(np.asarray(u.get_segmented_embeds_i(i)) != -1)) for i in range(u.D)]

"""
The oracle side of the relabel-heavy chains of tests/test_gpu_large_banks.py.

The persistent FBGMM chain (k_fb_chain) logs every component that empties within one utterance and stops the launch after
it; the launcher relabels the other utterances' rows from that log.  The log held 16 pairs, and an utterance can empty one
component per old segment: up to N_max = 64.  The GPU test runs chains in which some utterance empties more than 16
components and others empty 13 to 16.  These checks keep that precondition true on every CPU run, so a change of seeds,
corpus builder or oracle cannot leave the GPU test without an overflowing utterance.
"""
import random

import numpy as np
import pytest

from oracle import np_oracle as no
from tests.golden import cases

# (kind, n_utt, D, K, N_range, n_slices_max): make_corpus(n_utt, D, K, seed=4, ragged=True, ...) with the priors of
# tests/golden/cases.py, init_am_assignments="rand", random / np.random seeded with 3 before the build, two sweeps
RELABEL_SHAPES = [
    ("diag", 8, 13, 300, (30, 40), 2),
    ("diag", 12, 4, 600, (40, 64), 6),
    ("fixed", 8, 13, 300, (30, 40), 2),
    ("bigram", 8, 13, 300, (30, 40), 2),
    ("bigram", 12, 4, 600, (40, 64), 6),
]
RELABEL_IDS = ["%s_D%d_K%d_u%d" % (s[0], s[2], s[3], s[1]) for s in RELABEL_SHAPES]


def relabel_corpus(n_utt, D, K, N_range, nmax):
    from segmentalist_amd.synth import make_corpus
    return make_corpus(n_utt, D, K, seed=4, ragged=True, n_slices_max=nmax, N_range=N_range)


def build_segmenter(mods, kind, corpus, D, K, nmax, seed=3, fb_type="standard"):
    """An oracle (mods from oracle/np_oracle.py) or product segmenter with the priors of tests/golden/cases.py, random and
    np.random seeded with `seed` first (init_am_assignments="rand" draws from np.random)."""
    random.seed(seed)
    np.random.seed(seed)
    args = dict(n_slices_min=0, n_slices_max=nmax, p_boundary_init=0.5, beta_sent_boundary=-1, lms=1.0, wip=0.0,
                init_am_assignments="rand", time_power_term=1.0)
    fixed = mods["FixedVarPrior"](*cases.fixed_prior_params(D))
    if kind == "bigram":
        return mods["BigramAcousticWordseg"](K, fixed, dict(cases.BIGRAM_LM), *corpus, covariance_type="fixed",
                                             fb_type="unigram", **args)
    prior = fixed if kind == "fixed" else mods["NIW"](*cases.diag_prior_params(D))
    return mods["UnigramAcousticWordseg"](mods["FBGMM"], 1.0, K, prior, *corpus, covariance_type=kind, fb_type=fb_type, **args)


ORACLE_MODS = dict(FixedVarPrior=no.FixedVarPrior, NIW=no.NIW, FBGMM=no.FBGMM, UnigramAcousticWordseg=no.UnigramAcousticWordseg,
                   BigramAcousticWordseg=no.BigramAcousticWordseg)


def count_deletions(ref):
    """Wrap the oracle segmenter `ref` so that every gibbs_sample_i appends to the returned list the number of components
    del_component removed during it."""
    comp = ref.acoustic_model.components
    per, n = [], [0]
    real_del, real_utt = comp.del_component, ref.gibbs_sample_i

    def del_component(k):
        n[0] += 1
        return real_del(k)

    def gibbs_sample_i(i, *a, **kw):
        n[0] = 0
        out = real_utt(i, *a, **kw)
        per.append(n[0])
        return out

    comp.del_component = del_component
    ref.gibbs_sample_i = gibbs_sample_i
    return per


def assert_relabel_heavy(per):
    """Some utterance empties more than the old log held, another one 13 to 16 components."""
    assert max(per) > 16, "no utterance empties more than 16 components: %s" % sorted(per)[-5:]
    assert any(13 <= p <= 16 for p in per), "no utterance empties 13 to 16 components: %s" % sorted(per)[-5:]
    assert max(per) <= 64


@pytest.mark.parametrize("kind,n_utt,D,K,N_range,nmax", RELABEL_SHAPES, ids=RELABEL_IDS)
def test_relabel_heavy_shapes_empty_more_components_than_the_old_log_held(kind, n_utt, D, K, N_range, nmax):
    corpus = relabel_corpus(n_utt, D, K, N_range, nmax)
    no.set_shuffle("py3")
    ref = build_segmenter(ORACLE_MODS, kind, corpus, D, K, nmax)
    per = count_deletions(ref)
    for _ in range(2):
        ref.gibbs_sample(1)
    assert len(per) == 2 * n_utt
    assert_relabel_heavy(per)
    # never more than one per old segment: the bound the log is sized by
    assert max(per) <= N_range[1]

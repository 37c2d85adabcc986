"""The corpora of tests/test_gpu_fbgmm_batch_long.py do what they are there for -- checked with the oracle and the batch
specification alone, so that it is verified on a machine without a GPU: the longest utterance exceeds 64 landmarks, the
window-of-one case holds more than 64 tokens in an utterance, the duration-floor cases reach the all -inf windows and the
back-tracking branch, and every log-probability is finite."""
import numpy as np
import pytest

from tests import fbgmm_long as fl

LONG = [n for n in fl.CASES if not n.startswith("short_")]


def _two_sweeps(name):
    ref, spec = fl.oracle_of(name)
    with fl.DpCensus() as census:
        lps = [spec.sweep(sw) for sw in range(2)]
    return ref, spec, census, lps


@pytest.mark.parametrize("name", LONG)
def test_long_corpora_exceed_64_landmarks_and_have_finite_logprobs(name):
    ref, spec, census, lps = _two_sweeps(name)
    assert fl.longest(ref) > 64
    c = fl.CASES[name]
    if "N" in c:
        assert fl.longest(ref) == c["N"]
    if name == "diag_65":
        assert fl.longest(ref) == 65, "one landmark in the token lists' second chunk of 64 flags"
        assert min(ref.utterances.lengths) < c["nmax"], "an utterance shorter than the window reads the band's padded rows"
    if name.startswith("ragged_") or name.endswith("_f32"):
        assert min(ref.utterances.lengths) <= c["nmax"], "an utterance no longer than the window rides along"
    for lp in lps:
        assert np.all(np.isfinite(lp))
    assert census.calls == 2 * c["n_utt"]


@pytest.mark.parametrize("name", ["short_fixed", "short_diag", "short_bigram"])
def test_short_twins_stay_within_64_landmarks(name):
    ref, spec = fl.oracle_of(name)
    assert 32 < fl.longest(ref) <= 64
    assert np.all(np.isfinite(spec.sweep(0)))


def test_upper_end_is_256_landmarks():
    ref, _ = fl.oracle_of("fixed_256")
    assert set(ref.utterances.lengths) == {256}


def test_window_of_one_holds_more_than_64_tokens_per_utterance():
    ref, spec, census, lps = _two_sweeps("fixed_150_w1")
    assert max(fl.tokens_per_utterance(ref)) > 64
    assert min(fl.tokens_per_utterance(ref)) == 150


def test_duration_floor_reaches_dead_windows_and_back_tracking():
    """min_duration = 9, the case as it was asked for: spans shorter than nine frames have NaN durations, and forward steps
    whose every candidate is -inf occur.  Its backward pass can NOT reach a dead end on these corpora, whatever the seed:
    make_corpus draws every slice 3..11 frames long, so every span of three slices has at least nine frames; alpha[3] and
    every later alpha are therefore finite, and so is a candidate of every window the backward pass visits.  The count is
    asserted to be zero here so that this stays a stated fact.  The back-tracking branch is covered by the twin case with a
    floor of 30 frames (corpus seed picked on the CPU, tests/fbgmm_long.py), where the count is positive."""
    ref, spec, census, lps = _two_sweeps("diag_mindur")
    assert np.isnan(ref.utterances.durations[ref.utterances.vec_ids >= 0]).any()
    assert census.dead_windows > 0
    assert census.backtracks == 0
    ref, spec, census, lps = _two_sweeps("diag_mindur_backtrack")
    assert census.dead_windows > 0
    assert census.backtracks > 0
    for lp in lps:
        assert np.all(np.isfinite(lp))


@pytest.mark.parametrize("name", ["ragged_fixed", "diag_100_w20", "diag_mindur_backtrack"])
def test_complete_band_exists_for_the_window(name):
    """What the banded kernel reads: Utterances.complete_band_tables(W) of the product's Utterances (host only)."""
    import random
    from segmentalist_amd.utterances import Utterances, process_embeddings
    c = fl.CASES[name]
    emb, vec_ids_dict, dur, lms = fl.corpus_of(name)
    _, vec_ids, labels = process_embeddings(emb, vec_ids_dict)
    random.seed(5)
    np.random.seed(5)
    u = Utterances([len(lms[k]) for k in labels], vec_ids, [dur[k] for k in labels], [lms[k] for k in labels],
                   n_slices_max=c["nmax"], **{k: v for k, v in c.get("kw", {}).items() if k in ("min_duration", "p_boundary_init")})
    band = u.complete_band_tables(c["nmax"])
    assert band is not None
    ids, d = band
    assert ids.shape == (c["n_utt"], u.N_max, c["nmax"])
    assert u.complete_band_tables(c["nmax"] - 1) is None if c["nmax"] > 1 else True

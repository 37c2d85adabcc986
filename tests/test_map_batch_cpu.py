"""The precondition of tests/test_gpu_map_batch.py, checked with the oracle alone (no device): on every exact case, over
the sweeps the GPU test runs, every decision of the Viterbi / MAP sweep (tests/map_batch.py) is far from a tie.

  * DP margin: at every step t = 1..N the gap between the largest and the second largest finite candidate vec + alpha,
    relative to max(1, |largest|), is >= 1e-6;
  * slot margin: the gap between the maximal logit and the largest strictly smaller one, same scaling, is >= 1e-6; exact
    ties at the maximum are allowed among empty slots only (they carry one value; the first wins).

Where the 1e-6 comes from: the suite holds the device's fp64 log-probabilities to 1e-9 relative of the specification
(tests/test_gpu_fbgmm_batch.py); this is three orders above that.  It is a condition on the INPUTS, not a tolerance of the
device: if a seed fails it after some later change to the corpus generator, change the seed, never the threshold.

Measured (smallest DP margin / smallest slot margin, corpus seed 200): fixed_small 3.6e-3 / 1.0e-2, diag_K65 1.1e-2 / 2.7e-1,
diag_K130 3.0e-4 / 8.9e-3 (no tie on an occupied slot, 29 ties among empty slots, 16 occupied slots, 115 tokens in two sweeps),
fixed_K300 3.2e-3 / 6.1e-2, fixed_K1025 2.3e-2 / 4.7e-2, fixed_w20 3.8e-4 / 5.0e-2, diag_w20 5.2e-4 / 3.2e-2, fixed_64_w30
3.6e-5 / 2.6e-3, ragged_fixed 2.9e-6 / 4.3e-5, ragged_diag 2.7e-5 / 4.2e-4, diag_65 (corpus seed 168) 3.6e-5 / 1.1e-2,
diag_100_w20 3.2e-6 / 2.1e-2, fixed_100_w40 1.7e-5 / 5.1e-2, diag_mindur_backtrack 3.4e-5 / 1.1e-3, chain_diag_D70
7.7e-5 / 1.8e-2, chain_diag_D256 4.5e-5 / 6.0e-4, fixed_small_f64 (seed 200, the first tried) 3.6e-3 / 1.0e-2."""
import numpy as np
import pytest

from tests import fbgmm_long
from tests import map_batch as mb

_RUNS = {}


def _run(name):
    """Census of the Viterbi sweeps of a case, and what changed in every sweep (computed once per session)."""
    if name not in _RUNS:
        ref, spec, _ = mb.pair(name, product=False)
        spec.census = mb.Census()
        u = ref.utterances
        changes = []
        for sw in range(mb.n_sweeps(name)):
            b0, s0 = u.boundaries.copy(), spec.slot.copy()
            spec.sweep(sw)
            changes.append((int(np.count_nonzero(b0 != u.boundaries)), int(np.count_nonzero(s0 != spec.slot))))
        _RUNS[name] = (spec.census, changes, fbgmm_long.longest(ref))
    return _RUNS[name]


def _assert_far_from_ties(c):
    assert c.dp_steps > 0 and c.tokens > 0
    assert c.dp_margin >= mb.MARGIN, c.dp_margin
    assert c.slot_margin >= mb.MARGIN, c.slot_margin
    assert c.tie_on_occupied == 0
    # the reference's argmax(exp(z - logsumexp z)) (slots) and argmax(exp(q[::-1] - logsumexp q)) (DP) are the argmax of z and
    # of q[::-1] on every token and at every step: the device may skip the softmax
    assert c.softmax_disagrees == 0


@pytest.mark.parametrize("name", mb.EXACT)
def test_every_decision_is_far_from_a_tie(name):
    census, changes, _ = _run(name)
    _assert_far_from_ties(census)


@pytest.mark.parametrize("name", mb.MIXED)
def test_every_decision_of_the_mixed_chain_is_far_from_a_tie(name):
    """two sampled sweeps, then two Viterbi sweeps on the same state (the use pattern)"""
    ref, spec, _ = mb.pair(name, product=False)
    for sw in range(2):
        spec.sweep(sw, viterbi=False)
    spec.census = mb.Census()
    for sw in range(2, 4):
        spec.sweep(sw)
    _assert_far_from_ties(spec.census)


@pytest.mark.parametrize("name", ["fixed_small", "ragged_diag", "diag_mindur_backtrack"])
def test_the_viterbi_chain_moves_and_is_not_the_sampled_chain(name):
    """Boundaries and slots change in sweep 0 and still change in sweep 1 (not a fixed point at once), and sweep 0 does not
    reproduce the sampled sweep from the same state."""
    census, changes, _ = _run(name)
    for sw in (0, 1):
        assert changes[sw][0] > 0 and changes[sw][1] > 0, (sw, changes)
    ref_v, spec_v, _ = mb.pair(name, product=False)
    ref_s, spec_s, _ = mb.pair(name, product=False)
    assert np.array_equal(ref_v.utterances.boundaries, ref_s.utterances.boundaries) and np.array_equal(spec_v.slot, spec_s.slot)
    spec_v.sweep(0)
    spec_s.sweep(0, viterbi=False)
    # (the fixed-variance cases' keywords make the boundary posteriors so peaked that the draws may all land on the maximum:
    # the chains then part in the slots)
    assert not (np.array_equal(ref_v.utterances.boundaries, ref_s.utterances.boundaries) and np.array_equal(spec_v.slot, spec_s.slot))
    if name != "fixed_small":
        assert not np.array_equal(ref_v.utterances.boundaries, ref_s.utterances.boundaries)


def test_the_corpora_exercise_what_they_are_there_for():
    # exact ties among empty slots occur, and tokens are won by the first empty slot
    assert any(_run(n)[0].empty_ties > 0 for n in mb.EXACT)
    assert _run("fixed_K300")[0].empty_winners >= 32 and _run("fixed_K1025")[0].empty_winners >= 64
    assert _run("diag_K65")[0].empty_ties > 0
    # all -inf windows in the forward pass, and decodes that start from a dead end at t = N
    c = _run("diag_mindur_backtrack")[0]
    assert c.dead_windows > 0 and c.dead_end_starts >= 1, (c.dead_windows, c.dead_end_starts)
    assert c.dead_end_starts < c.decodes
    # more tokens in an utterance than one row of sixteen lanes, short and long utterances in one corpus
    for n in ("ragged_fixed", "ragged_diag"):
        assert _run(n)[0].max_tokens_per_utt > 16
        assert _run(n)[2] > 64
    # the kernel choice (N_max > 64: band) and the window paths
    assert _run("fixed_64_w30")[2] == 64 and _run("fixed_w20")[2] == 24
    assert _run("diag_100_w20")[2] == 100 and _run("fixed_100_w40")[2] == 100
    assert _run("diag_65")[2] == 65


def test_no_uniform_is_consumed_and_the_temperature_is_ignored():
    import random
    ref_a, spec_a, _ = mb.pair("fixed_small", product=False)
    ref_b, spec_b, _ = mb.pair("fixed_small", product=False)
    state = random.getstate()
    lp_a = spec_a.sweep(0)
    assert random.getstate() == state
    lp_b = spec_b.sweep(0, anneal_temp=3.0, anneal_gibbs_am=True)
    assert np.array_equal(lp_a, lp_b) and np.array_equal(spec_a.slot, spec_b.slot)
    assert np.array_equal(ref_a.utterances.boundaries, ref_b.utterances.boundaries)


@pytest.mark.parametrize("cseed", [200, 201, 202])
def test_one_utterance_per_block_is_the_serial_viterbi_step(cseed):
    """With one slice and one utterance per block, step b conditions utterance b on everything but itself: the statistics of
    the oracle's serial fb_type="viterbi" gibbs_sample_i.  With lms = 1 (the serial span scores carry lms on the prior term
    like the batch's; map_assign_i carries none in either) the boundaries are the serial ones, and so is the component of the
    utterance's first new token, up to the batch's missing `k > K` clamp: compared through the reference's view, as the set of
    rows outside the utterance that share the token's component.  (Later tokens of the utterance see the earlier ones in the
    serial chain and not in the batch: np_fbgmm_batch.py, step 4.)"""
    c = dict(mb.LONG_CASES["diag_K65"], cseed=cseed, K=10, n_utt=6, B=6, S=1)
    corpus = fbgmm_long.corpus_of(c)
    ref_b, _ = fbgmm_long.oracle_of(c, corpus)
    spec = mb.MapBatch(ref_b, n_gibbs_blocks=c["B"], n_stat_blocks=1, seed=11)
    ref_s, _ = fbgmm_long.oracle_of(c, corpus)
    ref_s.fb_type = "viterbi"
    assert all(hi - lo == 1 for lo, hi in spec.ranges[0])
    for i in range(2):          # utterance 0, then utterance 1 on the state step 0 left where both sides agree on it
        mine = set(int(e) for e in ref_s.utterances.vec_ids[i] if e != -1)
        lp_b = np.zeros(ref_b.utterances.D)
        spec.step(i, lp_b)
        lp_s = ref_s.gibbs_sample_i(i)
        N = ref_b.utterances.lengths[i]
        assert np.array_equal(ref_b.utterances.boundaries[i, :N], ref_s.utterances.boundaries[i, :N])
        assert abs(lp_b[i] - lp_s) <= 1e-9 * max(1.0, abs(lp_s))
        toks = spec._tokens(i)
        assert toks == [e for e in ref_s.utterances.get_segmented_embeds_i(i) if e != -1]
        e0 = toks[0]
        a_b, _K = spec.canonical()
        a_s = ref_s.acoustic_model.components.assignments
        mates_b = set(int(r) for r in np.where(a_b == a_b[e0])[0]) - mine
        mates_s = set(int(r) for r in np.where(a_s == a_s[e0])[0]) - mine
        assert mates_b == mates_s
        if len(toks) > 1:       # the sides may part on the later tokens: stop where they do
            if not all(set(np.where(a_b == a_b[e])[0]) == set(np.where(a_s == a_s[e])[0]) for e in toks):
                break

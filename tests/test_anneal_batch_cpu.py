"""The cases of tests/test_gpu_anneal_batch.py are worth running -- checked with the oracle and the batch specification alone
(oracle/np_fbgmm_batch.py), on a machine without a GPU:

  * every case's first sweep depends on the temperature: at least one utterance in ten takes other boundaries than at T = 1,
    and where the case anneals the assignments at least one token in ten differs from the run that does not (on the corpora
    of the existing tests with their default keywords most of these shares are 0: a kernel that ignored anneal_temp would
    give the specification's chain bit for bit);
  * the host-side checkers of the tolerance-mode tests (tests/anneal.py) return exactly 0 on the specification's own draws,
    and tell the case's temperature from 1: with intervals computed at T = 1 at least one draw in ten lies further outside
    than the bound the device is held to;
  * what n_slices_min = 1 (accepted by the batch entry points, passed by no other test) changes.

The shares are printed (pytest -s)."""
import numpy as np
import pytest

from oracle import np_oracle as no
from tests import anneal as an

ALL = list(an.EXACT) + list(an.TOLERANCE)


def test_tables_hold_what_the_device_tests_need():
    for name in ALL:
        c = an.case_of(name)
        assert c["T"] in an.TEMPS and c["T"] != 1.0, name
    ex = an.EXACT.values()
    for kind in ("fixed", "diag", "bigram"):
        mine = [c for c in ex if c["kind"] == kind]
        assert any(not c["am"] for c in mine), kind + ": boundary-only annealing"
        assert any(c["am"] for c in mine), kind + ": assignment annealing on top"
        assert any(c["T"] < 1 for c in mine), kind + ": T < 1"
    for form in an.DRIVER.values():
        assert an.EXACT[form]["am"]
    assert an.EXACT[an.RANKS]["S"] % 2 == 0


@pytest.mark.parametrize("name", ALL)
def test_case_depends_on_the_temperature(name):
    c = an.case_of(name)
    fb, am = an.sensitivity(name)
    print("%s (T = %g, %s): boundaries of %.2f of the utterances differ from T = 1; %.2f of the tokens differ with "
          "anneal_gibbs_am%s" % (name, c["T"], c["kw"], fb, am, "" if c["am"] else " (not annealed in this case)"))
    assert fb >= 0.10, fb
    if c["am"]:
        assert am >= 0.10, am


def _draws(name):
    """The specification's run the case stands for: (run, temperature of its slot draws)."""
    c = an.case_of(name)
    run = an.first_sweeps(name)[2 if c["am"] else 1]
    return run, (c["T"] if c["am"] else 1.0)


def _boundary_distances(run, T):
    out = []
    for d in run["trace"].dp:
        alpha = no.forward_alphas(d["vec"], 0.0, d["N"], d["window"])
        out += an.boundary_draw_distance(d["vec"], alpha, d["N"], d["window"], T, d["bounds"], run["seed"], 0, d["utt"])
    return out


def _slot_distances(run, T):
    return [an.slot_draw_distance(t["prior"], t["ll"], T, t["k"], an.token_uniform(run["seed"], 0, t["utt"], run["N_max"], t["t"]))
            for t in run["trace"].tok]


@pytest.mark.parametrize("name", ALL)
def test_checkers_on_the_specification_s_own_draws(name):
    """Exactly 0 at the temperature the draws were made at; and with intervals computed at T = 1 instead, beyond the device's
    bound for at least one draw in ten (a checker that cannot tell T from 1 proves nothing).  The second condition is held
    for the tolerance-mode cases, where the checkers are what the device is measured with; for the exact-mode cases, which
    are held to equality with the specification, the share is printed (at T = 0.5 a sharpened draw mostly keeps the
    candidate that already dominated: few intervals move, while one utterance in four still takes other boundaries)."""
    c = an.case_of(name)
    run, T_am = _draws(name)
    assert all(d["T"] == c["T"] for d in run["trace"].dp)
    right = _boundary_distances(run, c["T"])
    assert len(right) >= len(run["trace"].dp) and all(dist == 0.0 for dist, _ in right), max(d for d, _ in right)
    wrong = _boundary_distances(run, 1.0)
    share_fb = float(np.mean([dist > an.boundary_bound(M, c["T"]) for dist, M in wrong]))
    share_am = None
    slots = _slot_distances(run, T_am)
    assert slots and all(dist == 0.0 for dist in slots), max(slots)
    if c["am"]:
        share_am = float(np.mean([dist > an.slot_bound(c["T"]) for dist in _slot_distances(run, 1.0)]))
    print("%s (T = %g): intervals computed at T = 1 reject %.2f of %d boundary draws%s"
          % (name, c["T"], share_fb, len(wrong), "" if share_am is None else " and %.2f of %d slot draws" % (share_am, len(slots))))
    if name in an.TOLERANCE:
        assert share_fb >= 0.10, share_fb
        assert share_am >= 0.10, share_am


def test_minimum_of_one_slice_changes_nothing_in_the_specification():
    """n_slices_min = 1, the other value the batch entry points accept: every segment spans at least one slice, so the
    initial boundaries' rejection loop (utterances.py:141-157) accepts what it accepts at 0, and forward_backward takes the
    argument without reading it (unigram_acoustic_wordseg.py:653-756).  The specification's chain is therefore the same,
    stated here as a fact; the case that carries n_slices_min = 1 holds the device to it (segk_fbb_segment and
    segk_fbb_step_diag32 validate the argument and must not act on it either)."""
    c = an.EXACT["diag_w5_am"]
    assert c["kw"]["n_slices_min"] == 1
    chains = []
    for n_min in (1, 0):
        ref, spec, _ = an.build(dict(c, kw=dict(c["kw"], n_slices_min=n_min)))
        assert ref.n_slices_min == n_min
        lps = [spec.sweep(sw, c["T"], c["am"]) for sw in range(2)]
        chains.append((ref.utterances.boundaries.copy(), spec.slot.copy(), np.array(lps)))
    for a, b in zip(*chains):
        assert np.array_equal(a, b)

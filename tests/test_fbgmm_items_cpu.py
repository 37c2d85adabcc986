"""The stand-alone batch specification (tests/fbgmm_items.py) on the CPU: that it is the segmenter's blocked sampler on
one-landmark utterances, that with one item per block it sees the serial chain's statistics, the conditions on the inputs
the device parity tests rest on, and the ABI the feature adds."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import fbgmm_items as fi
from tests import fullcov_batch as fb
from tests import fullcov_wordseg as fw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ASSIGNED = [n for n, c in fi.CASES.items() if c[9] == 0.0]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


@pytest.fixture(scope="module")
def runs():
    """name -> the specification after the case's sweeps (consider_unassigned=True), computed once"""
    return {name: fi.run_spec(name) for name in fi.CASES}


@pytest.fixture(scope="module")
def runs_assigned_only():
    return {name: fi.run_spec(name, consider_unassigned=False) for name in fi.UNASSIGNED}


def one_landmark_corpus(X):
    """the rows as utterances of one landmark, one span of duration 1 each, in row order"""
    keys = ["u%07d" % i for i in range(len(X))]
    mats = {k: X[i:i + 1] for i, k in enumerate(keys)}
    vec_ids = {k: np.array([0]) for k in keys}
    durations = {k: [1] for k in keys}
    landmarks = {k: [1] for k in keys}
    return mats, vec_ids, durations, landmarks


def segmenter_route(case):
    """nb.FbgmmBatch (FullcovBatch) on the oracle's UnigramAcousticWordseg (tests/fullcov_wordseg.py SpecWordseg) over the
    case's rows as one-landmark utterances, from the case's assignments"""
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, a = fi.make_inputs(case)
    corpus = one_landmark_corpus(X)
    np.random.seed(1)
    if cov == "full":
        seeds = {k: [int(a[i])] for i, k in enumerate(sorted(corpus[0]))}
        seg = fw.SpecWordseg(fi.ALPHA, K, fi.SpecPrior(*fi.prior_params(cov, D)), *corpus, seed_assignments_dict=seeds,
                             seed_boundaries_dict={k: [1] for k in corpus[0]}, n_slices_max=1, lms=fi.LMS)
        cls = fb.FullcovBatch
    else:
        prior = no.FixedVarPrior(*fi.prior_params(cov, D)) if cov == "fixed" else no.NIW(*fi.prior_params(cov, D))
        seg = no.UnigramAcousticWordseg(no.FBGMM, fi.ALPHA, K, prior, *corpus, covariance_type=cov, n_slices_max=1, lms=fi.LMS)
        # (its constructor draws the assignments: the case's take their place)
        seg.acoustic_model = no.FBGMM(seg.acoustic_model.components.X, prior, fi.ALPHA, K, a, covariance_type=cov, lms=fi.LMS)
        cls = nb.FbgmmBatch
    assert np.array_equal(seg.acoustic_model.components.X, X) and np.array_equal(seg.acoustic_model.components.assignments, a)
    assert seg.utterances.N_max == 1 and seg.utterances.boundaries.all()
    return cls(seg, n_gibbs_blocks=B, n_stat_blocks=S, seed=fi.BATCH_SEED)


@pytest.mark.parametrize("name", ALL_ASSIGNED)
def test_sweep_is_the_segmenters_on_one_landmark_utterances(runs, name):
    """(a) With every item assigned the slots after every sweep are those of nb.FbgmmBatch (FullcovBatch for full
    covariance) run on the oracle's segmenter over the same rows as N one-landmark utterances of duration 1 (n_slices_max 1,
    the same B, S and seed, the components' draws at the sweep's temperature): the oracle's constructors take such a corpus."""
    case = fi.CASES[name]
    route = segmenter_route(case)
    for s, temp in enumerate(case[8]):
        route.sweep(s, temp, anneal_gibbs_am=True)
        assert np.array_equal(route.slot, runs[name].history[s]), (name, s)
        assert route.seg.utterances.boundaries.all()


@pytest.mark.parametrize("name", list(fi.SERIAL))
def test_one_item_per_block_sees_the_serial_statistics(name):
    """(b) N <= B * S: the log-probability vector of every item equals, at 1e-12, the one the oracle's FBGMM (SpecFBGMM over
    SpecComponents for full covariance) forms for it after del_item -- up to the labelling: occupied slots in slot order
    are the serial components, every empty slot carries the prior's term.  The cases have S = 1: a block is one cell of every
    slice, so with S > 1 it holds up to S items that are left out together, and N <= B * S alone does not give the serial
    statistics (at B x S = 4 x 3, N = 12 the vectors differ in the first digit)."""
    case = fi.SERIAL[name]
    cov, dtype, D, K, B, S, N, seed = case
    assert N <= B * S and S == 1
    am, spec = fi.spec_of(case)
    X, a = fi.make_inputs(case)
    for b in range(B):
        d = spec.derive(*spec.stats_excluding(b))
        for s in range(S):
            lo, hi = spec.ranges[s][b]
            assert hi - lo <= 1
            for i in range(lo, hi):
                z = spec.prior_z(d, None, None, None) + spec.loglik(d, spec.X[i])
                serial = fi.spec_model(cov, X, K, a)
                c = serial.components
                c.del_item(i)
                want = serial._log_prob_z(i, serial.lms) if cov == "full" else serial._logits(i)
                occ = np.where(d["active"])[0]
                assert len(occ) == c.K
                # the serial labels of the occupied slots: an item outside the block names them
                order = [int(c.assignments[np.where((spec.slot == k) & (np.arange(N) != i))[0][0]]) for k in occ]
                assert _rel(z[occ], want[order]) <= 1e-12, (name, i)
                empty = np.where(~d["active"])[0]
                assert _rel(z[empty], np.full(len(empty), want[c.K])) <= 1e-12, (name, i)


@pytest.mark.parametrize("name", list(fi.CASES))
def test_conditions_on_the_inputs(runs, name):
    """(c) on the specification alone: every draw at least DRAW_MARGIN clear of the edges of its cumulative distribution;
    with more than one slot, a slot empties and a slot is founded within the sweeps; every annealed sweep changes a draw
    against T = 1 on the same state."""
    case, spec = fi.CASES[name], runs[name]
    cen = spec.census
    print("%s: %d draws, least margin %.3g, emptied %d, founded %d, changed by T %s" % (name, cen.draws, cen.margin, cen.emptied,
                                                                                      cen.founded, cen.changed_by_T))
    assert cen.draws >= 1 and cen.margin >= fi.DRAW_MARGIN
    if case[3] > 1:
        assert cen.emptied >= 1 and cen.founded >= 1
    for temp, changed in zip(case[8], cen.changed_by_T):
        assert temp == 1 or changed >= 1


@pytest.mark.parametrize("name", fi.UNASSIGNED)
def test_consider_unassigned_is_not_vacuous(runs, runs_assigned_only, name):
    """(c) the runs with and without consider_unassigned end in different slots; the second one's draws keep the margin and
    its annealed sweeps change draws too; the items it never considered are still unassigned."""
    case = fi.CASES[name]
    a, b = runs[name], runs_assigned_only[name]
    X, start = fi.make_inputs(case)
    assert np.count_nonzero(start < 0) >= 0.2 * len(start)
    assert np.all(a.slot >= 0)
    assert np.array_equal(b.slot < 0, start < 0)
    assert np.count_nonzero(a.slot != b.slot) >= 1
    assert b.census.margin >= fi.DRAW_MARGIN
    for temp, changed in zip(case[8], b.census.changed_by_T):
        assert temp == 1 or changed >= 1


@pytest.mark.parametrize("name", ["fx_D39_K7_n255", "dg_D39_K7_un", "fc_D3_K7_n5_2x2"])
def test_record_cases_keep_the_margin(name):
    """the two sweeps of gibbs_sample(2, sync="batch", anneal_schedule="linear") -- T = 10, then 1 -- that the device test
    of the record runs on these cases: their draws keep the margin too"""
    am, spec = fi.spec_of(fi.CASES[name])
    spec.census = fi.Census()
    for s, temp in enumerate(1. / np.linspace(0.1, 1, 2)):
        spec.sweep(s, float(temp), True)
    assert spec.census.margin >= fi.DRAW_MARGIN
    assert spec.census.changed_by_T[0] >= 1


def test_cases_cover_the_kernel_paths():
    """the shapes the issue asks for, between the cases"""
    cases = list(fi.CASES.values())
    assert {c[0] for c in cases} == {"fixed", "diag", "full"} and {c[1] for c in cases} == {"float32", "float64"}
    assert {c[2] for c in cases if c[0] != "full"} == {3, 39, 100} and {c[2] for c in cases if c[0] == "full"} == {3, 39, 64}
    assert {c[3] for c in cases} == {1, 7, 65, 130, 300, 1100}
    assert {(c[3] + 63) // 64 for c in cases} == {1, 2, 3, 5, 18}                     # entries per run of draw_chunked
    assert {(1, 1), (2, 2), (3, 4), (8, 8)} <= {(c[4], c[5]) for c in cases}
    assert {1, 5} <= {c[6] for c in cases}
    cells = set()
    for c in cases:
        sb = no.block_bounds(c[6], c[5])
        for s in range(c[5]):
            bb = no.block_bounds(sb[s + 1] - sb[s], c[4])
            cells |= {bb[b + 1] - bb[b] for b in range(c[4])}
    assert {0, fi.TILE - 1, fi.TILE, fi.TILE + 1} <= cells and max(cells) > 2 * fi.TILE
    assert {10.0, 0.5, 1.0} <= {t for c in cases for t in c[8]}


def test_abi_15_and_the_new_entry_point():
    """(d) header, library and binding report 15 and the new symbol resolves (the built library, no GPU)."""
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION
    assert hasattr(lib, "segk_fbi_assign") and "segk_fbi_assign" in _abi.SIGNATURES
    assert re.search(r"\bsegk_fbi_assign\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "fbgmm.py:288-463" in hdr

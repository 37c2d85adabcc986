"""The specification of the acoustic-model batch sweep (tests/am_batch.py) on the CPU: that on one-landmark utterances it is
the stand-alone model's item sweep, that with one utterance per block a token sees the serial chain's statistics, the
conditions on the inputs the device parity tests rest on, and the entry point the feature adds."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as no
from tests import am_batch as ab
from tests import fbgmm_items as fi
from tests import fullcov_wordseg as fw
from tests.test_fbgmm_items_cpu import one_landmark_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


@pytest.fixture(scope="module")
def runs():
    """name -> the specification after the case's inner sweeps, computed once"""
    return {name: ab.run_spec(name) for name in ab.CASES}


def one_landmark_route(case):
    """AmBatch (AmFullcovBatch) on the oracle's segmenter over the rows of a tests/fbgmm_items.py case as one-landmark
    utterances, from the case's assignments"""
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, a = fi.make_inputs(case)
    corpus = one_landmark_corpus(X)
    np.random.seed(1)
    if cov == "full":
        seeds = {k: [int(a[i])] for i, k in enumerate(sorted(corpus[0]))}
        seg = fw.SpecWordseg(fi.ALPHA, K, fi.SpecPrior(*fi.prior_params(cov, D)), *corpus, seed_assignments_dict=seeds,
                             seed_boundaries_dict={k: [1] for k in corpus[0]}, n_slices_max=1, lms=fi.LMS)
        cls = ab.AmFullcovBatch
    else:
        prior = no.FixedVarPrior(*fi.prior_params(cov, D)) if cov == "fixed" else no.NIW(*fi.prior_params(cov, D))
        seg = no.UnigramAcousticWordseg(no.FBGMM, fi.ALPHA, K, prior, *corpus, covariance_type=cov, n_slices_max=1, lms=fi.LMS)
        seg.acoustic_model = no.FBGMM(seg.acoustic_model.components.X, prior, fi.ALPHA, K, a, covariance_type=cov, lms=fi.LMS)
        cls = ab.AmBatch
    assert seg.utterances.N_max == 1 and seg.utterances.boundaries.all()
    return cls(seg, n_gibbs_blocks=B, n_stat_blocks=S, seed=fi.BATCH_SEED)


@pytest.mark.parametrize("name", ["fx_D39_K7_n255", "dg_D100_K130_T10", "fx_D3_K7_n5_8x8", "fc_D3_K7_n5_2x2", "fc_D64_K7_un_T10"])
def test_one_token_per_utterance_is_the_item_sweep(name):
    """1. One-landmark corpus, every item assigned: the slots after every sweep are those of tests/fbgmm_items.py's item
    sweep with consider_unassigned=False, draw for draw (annealed sweeps included)."""
    case = list(fi.CASES[name])
    case[9] = 0.0                                            # every item assigned
    am, items = fi.spec_of(case)
    route = one_landmark_route(case)
    assert np.all(items.slot >= 0) and np.array_equal(items.slot, route.slot)
    for s, temp in enumerate(case[8]):
        items.sweep(s, temp, consider_unassigned=False)
        route.am_sweep(s, temp)
        assert np.array_equal(route.slot, items.slot), (name, s)
        for sl in range(items.S):
            for b in range(items.B):
                for x, y in zip(route.P[sl][b], items.P[sl][b]):
                    assert np.array_equal(x, y)


@pytest.mark.parametrize("name", list(ab.SERIAL))
def test_one_utterance_per_block_sees_the_serial_statistics(name):
    """2. S = 1, B = number of utterances: the logits of every token equal, at 1e-12, those the serial oracle model (SpecFBGMM
    for full covariance) forms for it after del_item of all tokens of its utterance -- up to the labelling: occupied slots in
    slot order are the serial components, every empty slot carries the prior's term."""
    case = ab.SERIAL[name]
    cov, K, B, S = case[0], case[3], case[4], case[5]
    seg, spec = ab.spec_of(case)
    u = seg.utterances
    assert S == 1 and B == u.D
    seen = 0
    for b in range(B):
        d = spec.derive(*spec.stats_excluding(b))
        lo, hi = spec.ranges[0][b]
        assert hi - lo == 1
        toks = spec._tokens(lo)
        serial = fi.spec_model(cov, spec.X, K, spec.slot)
        c = serial.components
        for e in toks:
            c.del_item(e)
        occ = np.where(d["active"])[0]
        assert len(occ) == c.K
        mine = set(toks)
        # the serial labels of the occupied slots: a token outside the utterance names them
        order = [int(c.assignments[[r for r in np.where(spec.slot == k)[0] if r not in mine][0]]) for k in occ]
        empty = np.where(~d["active"])[0]
        for e in toks:
            z = spec.prior_z(d, None, None, None) + spec.loglik(d, spec.X[e])
            want = serial._log_prob_z(e, serial.lms) if cov == "full" else serial._logits(e)
            assert _rel(z[occ], want[order]) <= 1e-12, (name, e)
            assert _rel(z[empty], np.full(len(empty), want[c.K])) <= 1e-12, (name, e)
            seen += 1
    assert seen == sum(case[6])


@pytest.mark.parametrize("name", list(ab.CASES))
def test_conditions_on_the_inputs(runs, name):
    """3. On the specification alone, for every case of the device tests: every uniform at least DRAW_MARGIN clear of the
    edges of its cumulative distribution; with more than one slot a slot empties and a slot is founded within the sweeps; every
    annealed sweep changes a draw against T = 1 on the same state; tokens and boundaries are those from before the sweeps."""
    case, spec = ab.CASES[name], runs[name]
    cen = spec.census
    print("%s: %d draws, least margin %.3g, emptied %d, founded %d, changed by T %s, cells %s"
          % (name, cen.draws, cen.margin, cen.emptied, cen.founded, cen.changed_by_T, ab.cell_tokens(spec)))
    assert cen.draws == len(case[10]) * sum(case[6]) and cen.margin >= ab.DRAW_MARGIN
    if case[3] > 1:
        assert cen.emptied >= 1 and cen.founded >= 1
    for temp, changed in zip(case[10], cen.changed_by_T):
        assert temp == 1 or changed >= 1
    u = spec.seg.utterances
    assert np.array_equal(u.boundaries, spec.bounds0)
    assert [list(spec._tokens(i)) for i in range(u.D)] == spec.tokens0
    assert np.array_equal(np.where(spec.slot >= 0)[0], np.sort(np.concatenate([np.array(t, np.int64) for t in spec.tokens0])))


@pytest.mark.parametrize("name", list(ab.INTERLEAVED))
def test_interleaved_cases_keep_the_margin(name):
    """3. the sweeps of gibbs_sample(3, am_n_iter=2, sync="batch", am_sync="batch") that the device tests run on these cases
    -- two inner sweeps, one outer sweep, one shared counter -- keep the margin for the slot draws, inner and outer"""
    from tests import fullcov_batch as fb
    seg, spec = ab.spec_of(ab.INTERLEAVED[name])
    spec.census = ab.Census()
    index = 0
    for _ in range(3):
        for _ in range(2):
            spec.am_sweep(index, 1.0)
            index += 1
        margins = fb.Margins()
        record_outer(spec, index, margins)
        index += 1
        assert margins.slot >= ab.DRAW_MARGIN and margins.boundary >= ab.DRAW_MARGIN
    assert spec.census.margin >= ab.DRAW_MARGIN and spec.census.draws >= 1


def record_outer(spec, index, margins):
    """one outer sweep of the specification with the distances of its draws from the edges recorded (the way
    tests/fullcov_batch.FullcovBatch.sweep records them, for both classes)"""
    from oracle import np_fbgmm_batch as nb
    orig_draw, orig_chunked = no.draw, nb.draw_chunked

    def draw(p, u=None, *a, **k):
        if u is not None:
            margins.draw(p, u, "boundary")
        return orig_draw(p, u, *a, **k)

    def chunked(p, u):
        margins.draw(p, u, "slot")
        return orig_chunked(p, u)
    no.draw, nb.draw_chunked = draw, chunked
    try:
        return nb.FbgmmBatch.sweep(spec, index, 1.0, False)
    finally:
        no.draw, nb.draw_chunked = orig_draw, orig_chunked


def test_cases_cover_the_kernel_paths(runs):
    """the shapes the issue asks for, between the cases"""
    cases = list(ab.CASES.values())
    assert {c[0] for c in cases} == {"fixed", "diag", "full"} and {c[1] for c in cases} == {"float32", "float64"}
    assert {3, 39, 100} <= {c[2] for c in cases if c[0] != "full"} and {c[2] for c in cases if c[0] == "full"} == {39, 64}
    assert {1, 7, 65, 300} <= {c[3] for c in cases}
    assert {(1, 1), (2, 2), (3, 4), (8, 8)} <= {(c[4], c[5]) for c in cases}
    cells = {n for spec in runs.values() for row in ab.cell_tokens(spec) for n in row}
    assert {0, 1, ab.TILE - 1, ab.TILE, ab.TILE + 1, 150} <= cells
    per_utt = {(c[7], n) for c in cases for n in c[6]}
    assert (10, 1) in per_utt and (10, 10) in per_utt        # all one segment; a boundary at every landmark
    assert {10.0, 0.5, 1.0} <= {t for c in cases for t in c[10]}
    # logits beyond LDS: 768 D + 512 K_max > 147 456
    assert any(768 * c[2] + 512 * c[3] > 147456 for c in cases if c[0] != "full")
    band = ab.CASES["dg_band_N80"]
    assert band[7] == 80 and band[8] < band[7] and max(band[6]) > 64


def test_entry_point_declared_bound_and_abi_still_15():
    """4. the header declares segk_fbt_assign, the binding binds it, the library exports it, and the version is still 15."""
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    assert re.search(r"\bsegk_fbt_assign\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "segk_fbt_assign" in _abi.SIGNATURES and len(_abi.SIGNATURES["segk_fbt_assign"][1]) == 16
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION
    assert hasattr(lib, "segk_fbt_assign")
    assert re.search(r"15 \(no bump\) segk_fbt_assign", hdr)

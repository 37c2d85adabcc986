"""
GPU tests of the MAP sweeps of the stand-alone mixture model (`FBGMM.map_assign`, `batch_sweep_async(map_assign=True)`;
`segk_fbi_assign_map`, `segk_fbi_assign_map_diag32`, `segk_fbgmm_map_items`) against the NumPy specification
tests/fbgmm_items_map.py.  tests/test_fbgmm_items_map_cpu.py shows that on these cases every decision lies at least 1e-6
(relative) clear of its best competitor, so with likelihoods held to 1e-9 the slots and the moved counts must coincide.
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32
from tests import fbgmm_items_map as fm
from tests.test_gpu_fbgmm_items import one_landmark_corpus, rel, same_view

pytestmark = pytest.mark.gpu
RTOL = 1e-9
RECORD = ["components", "log_marg", "log_prob_X_given_z", "log_prob_z", "n_moved", "sample_time"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _ids(pairs):
    return ["%s%s" % (n, "" if cu else "/assigned") for n, cu in pairs]


def pair(case, probe=None):
    am, spec = fm.spec_of(case)
    m = fi.product_of(case)
    assert np.array_equal(m.components.assignments, spec.slot)
    if probe is not None:
        m._get_sweeper().probe_ll = probe.zeros((len(spec.slot), spec.K_max), dtype=probe.float64, device="cuda")
    return spec, m


def sweep_both(gpu, spec, m, index, consider_unassigned=True, map_assign=True, what=""):
    """One sweep of both (MAP, or sampled at temperature 1); everything held equal after it."""
    sw = m._get_sweeper()
    spec.ll_log = {} if sw.probe_ll is not None else None
    moved = spec.sweep(index, 1.0, consider_unassigned, map_assign=map_assign)
    m.batch_sweep_async(1, consider_unassigned, map_assign=map_assign)
    gpu.cuda.synchronize()
    m.components.dev.check_status()
    assert sw.sweep_index == index + 1
    got_slots = sw.slot.cpu().numpy()
    print("%s: moved %s (device %s)" % (what, moved, sw.moved() if map_assign else "-"))
    assert np.array_equal(got_slots, spec.slot), what
    if map_assign:
        assert sw.moved() == moved, what
    if sw.probe_ll is not None:
        got = sw.probe_ll.cpu().numpy()
        worst = max([rel(got[i], ll) for i, ll in spec.ll_log.items()] or [0.0])
        print("%s likelihoods %.3g over %d items" % (what, worst, len(spec.ll_log)))
        assert worst <= RTOL, what
    worst = 0.0
    for s in range(spec.S):
        for b in range(spec.B):
            cnt, sx, sxx = sw.cell_partials(b, s)
            rc, rx, rxx = spec._partial(s, b)
            assert np.array_equal(cnt, rc), what
            worst = max(worst, rel(sx, rx), rel(sxx, rxx))
    print("%s partials %.3g" % (what, worst))
    assert worst <= 1e-13, what
    return moved


@pytest.mark.parametrize("name,cu", fm.BATCH, ids=_ids(fm.BATCH))
def test_map_sweeps(gpu, name, cu):
    """slots, n_moved, probed likelihoods and partial sums after every MAP sweep of every case"""
    spec, m = pair(fi.CASES[name], probe=gpu)
    moved = [sweep_both(gpu, spec, m, s, cu, True, "%s MAP sweep %d" % (name, s)) for s in range(fm.N_SWEEPS)]
    assert moved == fm.run_batch(name, cu).census.moved
    if not cu:
        assert np.count_nonzero(spec.slot < 0) >= 1


def test_counter_accumulates_over_the_launches_of_a_block(gpu, monkeypatch):
    """K_max = 300, D = 100: the 65 rows of a tile (logits and prior terms) do not fit in LDS.  With the workspace bound at
    1 MiB a launch holds six tiles and the block's eight are walked in two launches: the same slots, and one count."""
    monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")
    name = "fx_D100_K300_Thalf"
    case = fi.CASES[name]
    spec, m = pair(case, probe=gpu)
    tiles = sum((hi - lo + fi.TILE - 1) // fi.TILE for row in spec.ranges for (lo, hi) in row[:1])
    per_launch = (1 << 20) // ((fi.TILE + 1) * case[3] * 8)
    assert 1 <= per_launch < tiles
    moved = [sweep_both(gpu, spec, m, s, True, True, "bounded workspace, MAP sweep %d" % s) for s in range(2)]
    assert moved == fm.run_batch(name, True).census.moved[:2]


@pytest.mark.parametrize("name", fm.MIXED)
def test_sampled_and_map_sweeps_mix_on_one_sweeper(gpu, name):
    """two sampled sweeps, two MAP sweeps, one sampled sweep: every sweep against the specification, sweep_index counting on"""
    spec, m = pair(fi.CASES[name], probe=gpu)
    for s, is_map in enumerate(fm.MIXED_PLAN):
        sweep_both(gpu, spec, m, s, True, is_map, "%s mixed sweep %d (%s)" % (name, s, "MAP" if is_map else "sampled"))
    m.materialise()
    same_view(m, spec, fi.CASES[name])


@pytest.mark.parametrize("name", fm.F32)
def test_float32_map_steps(gpu, monkeypatch, name):
    """score_precision="f32", one Gibbs step at a time through the C ABI (prepare, segk_fbi_assign_map_diag32, partials), the
    specification kept on the device's own slots.  Per step: finite probe rows for exactly the considered items, within the
    1e-4 contract of the fp64 likelihoods (empty slots: the prior predictive at 1e-9); every slot the fp64 first argmax of
    pz + the device's OWN probed likelihoods wherever the top two of that vector are 1e-9 max(1, |z|) apart (closer items
    are skipped, at most 1 %); the counter equals the slots that changed.  Then the same sweeps through FBGMM.map_assign on a
    second model: the same slots and counts."""
    from segmentalist_amd import _abi
    if name == "dg_D39_K300_8x8":
        monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")           # (the block's eight tiles in two launches)
    case = f32.CASES[name]
    spec = f32.spec_of(case)
    m = f32.product_of(case)
    sw = m._get_sweeper()
    assert sw.score_diag32
    N, K = len(spec.slot), spec.K_max
    probe = gpu.empty((N, K), dtype=gpu.float64, device="cuda")
    sw.enter()
    L, ctx, cp, fp, bp, st = sw._args()
    worst = worst_empty = 0.0
    decisions = skipped = 0
    moved_per_sweep = []
    for sweep_index in range(fm.N_SWEEPS):
        sw.n_moved.zero_()
        moved = 0
        for b in range(spec.B):
            probe.fill_(float("nan"))
            _abi.check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
            _abi.check(L.segk_fbi_assign_map_diag32(ctx, cp, fp, bp, 0, sw.S, b, sw._n_items[b], sweep_index, 1,
                                                    _abi.ptr(sw.new_tok), _abi.ptr(sw.n_new), _abi.ptr(probe), K,
                                                    _abi.ptr(sw.n_moved), st))
            _abi.check(L.segk_fbb_partials(ctx, cp, fp, bp, 0, sw.S, b, _abi.ptr(sw.new_tok), _abi.ptr(sw.n_new), st))
            gpu.cuda.synchronize()
            m.components.dev.check_status()
            got, slots = probe.cpu().numpy(), sw.slot.cpu().numpy()
            where = "%s sweep %d step %d" % (name, sweep_index, b)
            items = f32.considered(spec, b, True)
            others = np.setdiff1d(np.arange(N), items)
            assert np.isfinite(got[items]).all() and np.isnan(got[others]).all(), where
            assert np.array_equal(slots[others], spec.slot[others]), where
            d = spec.derive(*spec.stats_excluding(b))
            pz = np.log(float(spec.alpha) / K + d["cnt"])
            occ = d["active"]
            for i in items:
                want = spec.loglik(d, spec.X[i])
                worst = max(worst, f32.rel(got[i][occ], want[occ]))
                worst_empty = max(worst_empty, f32.rel(got[i][~occ], want[~occ]))
                z = pz + got[i]
                k = int(np.argmax(z))
                below = z[z < z[k]]
                decisions += 1
                if len(below) and z[k] - below.max() < 1e-9 * max(1.0, abs(z[k])):
                    skipped += 1
                else:
                    assert slots[i] == k, (where, i)
                assert 0 <= slots[i] < K, (where, i)
                moved += int(slots[i] != spec.slot[i])
            f32.apply_slots(spec, b, items, slots[items])          # the specification goes on from the device's slots
        assert sw.moved() == moved, (name, sweep_index)
        moved_per_sweep.append(moved)
    print("%s: worst likelihood error %.3g (occupied), %.3g (empty); %d decisions, %d skipped; moved %s"
          % (name, worst, worst_empty, decisions, skipped, moved_per_sweep))
    assert worst <= f32.CONTRACT and worst_empty <= 1e-9
    assert skipped <= 0.01 * decisions
    other = f32.product_of(case)
    rec = other.map_assign(fm.N_SWEEPS, sync="batch")
    assert rec["n_moved"] == moved_per_sweep
    assert np.array_equal(other._get_sweeper().slot.cpu().numpy(), spec.slot)


@pytest.mark.parametrize("name,transform", f32.SETTLED_RUNS, ids=f32.SETTLED_IDS)
def test_float32_map_steps_on_settled_slots_of_thousands_of_items(gpu, name, transform):
    """segk_fbi_assign_map_diag32 where a float32 term's rounding is multiplied by a slot's count (f32.SETTLED): the contract on
    f32.PROBES rows of every step, the slots of those rows the fp64 first argmax on the device's own likelihoods, the counter
    the slots that changed -- after the rows have shown that they can tell the compensated term from the plain one"""
    from tests.test_gpu_fbgmm_items_f32 import walk_settled
    walk_settled(gpu, name, transform, map_assign=True)


@pytest.mark.parametrize("name,cu", fm.SERIAL_FORM + [(n, True) for n in fm.SERIAL],
                         ids=_ids(fm.SERIAL_FORM + [(n, True) for n in fm.SERIAL]))
def test_serial_map_sweeps(gpu, name, cu):
    """FBGMM.map_assign(n, sync="sequential") against serial_map_sweep: assignments, K and n_moved exactly, the record at
    1e-9; no random.random() is consumed"""
    want = fm.run_serial(name, cu)
    m = fi.product_of(fm.case_of(name))
    state = random.getstate()
    for s in range(fm.N_SWEEPS):                          # (one sweep per call: the assignments after every sweep)
        rec = m.map_assign(1, consider_unassigned=cu, sync="sequential")
        where = "%s serial MAP sweep %d" % (name, s)
        assert sorted(rec) == RECORD and all(len(v) == 1 for v in rec.values()), where
        print("%s: moved %d, K %d, log_marg %.17g against %.17g" % (where, rec["n_moved"][0], rec["components"][0],
                                                                    rec["log_marg"][0], want.record[s]["log_marg"]))
        assert np.array_equal(m.components.assignments, want.assignments[s]), where
        assert m.components.K == want.K[s] == rec["components"][0], where
        assert rec["n_moved"][0] == want.moved[s], where
        for k, v in want.record[s].items():
            assert abs(rec[k][0] - v) <= RTOL * max(1.0, abs(v)), (where, k)
    assert random.getstate() == state


def test_until_converged_and_the_record(gpu):
    name = "dg_D39_K65_n257"
    case = fi.CASES[name]
    want = fm.run_batch(name, True)
    n = want.census.moved.index(0) + 1                    # the specification's sweep count
    spec, m = pair(case)
    state = random.getstate()
    rec = m.map_assign(10, sync="batch", until_converged=True)
    assert random.getstate() == state
    assert sorted(rec) == RECORD and all(len(v) == n for v in rec.values())
    assert rec["n_moved"] == want.census.moved[:n] and rec["n_moved"][-1] == 0
    sw = m._get_sweeper()
    assert sw.sweep_index == n
    assert np.array_equal(sw.slot.cpu().numpy(), want.history[n - 1])
    for s in range(n):
        canon, K = want.canon[s]
        assert rec["components"][s] == K
        fresh = fi.product_of(case, assignments=canon)
        for k, v in (("log_marg", fresh.log_marg()), ("log_prob_z", fresh.log_prob_z()),
                     ("log_prob_X_given_z", fresh.log_prob_X_given_z())):
            assert abs(rec[k][s] - v) <= RTOL * max(1.0, abs(v)), (k, s)
    # a further sweep changes nothing
    slots, partials = sw.slot.clone(), sw.partials.clone()
    more = m.map_assign(1, sync="batch")
    assert more["n_moved"] == [0]
    assert gpu.equal(sw.slot, slots) and gpu.equal(sw.partials, partials)
    # without until_converged the cap is the count
    assert len(fi.product_of(case).map_assign(2, sync="batch")["n_moved"]) == 2
    # the serial form stops at its own fixed point
    serial = fm.run_serial("fx_D39_K7_n255", True)
    ms = fi.product_of(fi.CASES["fx_D39_K7_n255"])
    rec = ms.map_assign(10, sync="sequential", until_converged=True)
    assert rec["n_moved"] == serial.moved[:serial.moved.index(0) + 1]


@pytest.mark.parametrize("name", ["fx_D39_K130_n600", "fc_D39_K65"])
def test_materialise_after_async_map_sweeps(gpu, name):
    case = fi.CASES[name]
    want = fm.run_batch(name, True)
    spec, m = pair(case)
    for _ in range(2):
        m.batch_sweep_async(map_assign=True)
    m.materialise()
    canon, K = want.canon[1]
    c = m.components
    assert c.K == K and np.array_equal(c.assignments, canon)
    fresh = fi.product_of(case, assignments=canon)          # the serial statistics are those of a model built from the labels
    for nm in ("counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "K", "assignments"):
        assert gpu.equal(getattr(c.dev, nm), getattr(fresh.components.dev, nm)), nm
    assert m._get_sweeper().moved() == want.census.moved[1]
    assert np.array_equal(m._get_sweeper().slot.cpu().numpy(), want.history[1])


def test_object_in_batch_mode(gpu):
    """FBGMM(..., sync="batch").map_assign(2) runs batch MAP sweeps"""
    name = "dg_D39_K65_n257"
    m = fi.product_of(fi.CASES[name], sync="batch")
    rec = m.map_assign(2)
    want = fm.run_batch(name, True)
    assert rec["n_moved"] == want.census.moved[:2]
    assert np.array_equal(m._get_sweeper().slot.cpu().numpy(), want.history[1])
    assert np.array_equal(m.components.assignments, want.canon[1][0])


def test_refusals(gpu, monkeypatch):
    from segmentalist_amd import _abi, device
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    # a model that belongs to a segmenter
    case = fi.CASES["fx_D3_K7_n5_8x8"]
    X, a = fi.make_inputs(case)
    corpus, keys = one_landmark_corpus(X)
    seg = UnigramAcousticWordseg(FBGMM, fi.ALPHA, 7, FixedVarPrior(*fi.prior_params("fixed", 3)), *corpus,
                                 covariance_type="fixed", n_slices_max=1, beta_sent_boundary=-1)
    with pytest.raises(SegkError, match="segmenter"):
        seg.acoustic_model.map_assign(1, sync="batch")
    with pytest.raises(SegkError, match="segmenter"):
        seg.acoustic_model.batch_sweep_async(map_assign=True)
    # more than one rank
    m = fi.product_of(case)

    class TwoRanks(object):
        rank, world = 0, 2
    monkeypatch.setattr(device, "get_comm", lambda group=None: TwoRanks())
    with pytest.raises(SegkError, match="one process"):
        m.map_assign(1, sync="batch")
    monkeypatch.undo()
    # through the C ABI: a language model, a corpus with span tables, the float32 form on components that are not diagonal
    m.batch_sweep_async(map_assign=True)
    gpu.cuda.synchronize()
    sw = m._get_sweeper()
    before = sw.slot.clone()
    L, ctx, cp, fp, bp, st = sw._args()
    tail = (_abi.ptr(sw.new_tok), _abi.ptr(sw.n_new), None, 0, _abi.ptr(sw.n_moved), st)
    f_lm = _abi.FbgmmDev.from_buffer_copy(sw.f)
    f_lm.lm_unigram = m.components.dev.counts.data_ptr()
    rc = L.segk_fbi_assign_map(ctx, cp, C.byref(f_lm), bp, 0, sw.S, 0, sw._n_items[0], 0, 1, *tail)
    assert rc == _abi.SEGK_ERR_UNSUPPORTED and "language model" in L.segk_last_error().decode()
    rc = L.segk_fbi_assign_map(ctx, seg._df._cp(), fp, bp, 0, sw.S, 0, sw._n_items[0], 0, 1, *tail)
    assert rc != 0 and "corpus of items" in L.segk_last_error().decode()
    rc = L.segk_fbi_assign_map_diag32(ctx, cp, fp, bp, 0, sw.S, 0, sw._n_items[0], 0, 1, *tail)
    assert rc == _abi.SEGK_ERR_UNSUPPORTED and "diagonal components" in L.segk_last_error().decode()
    rc = L.segk_fbgmm_map_items(ctx, m.components.dev._cp(), C.byref(f_lm), None, len(X), 1,
                                _abi.ptr(m.components.dev.status), _abi.ptr(sw.n_moved), st)
    assert rc != 0 and "language-model" in L.segk_last_error().decode()
    gpu.cuda.synchronize()
    assert gpu.equal(sw.slot, before)
    m.components.dev.check_status()

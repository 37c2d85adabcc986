"""
GPU tests of `FBGMM(..., covariance_type="diag", sync="batch", score_precision="f32")`: the batch sweeps of the stand-alone
mixture model with float32 item likelihoods (`segk_fbi_assign_diag32`), against the fp64 specification tests/fbgmm_items.py
under the project's tolerance contract.  tests/test_fbgmm_items_f32_cpu.py checks the inputs first (cases, emulation, margins).

The cases are walked one Gibbs step at a time -- segk_fbb_prepare, segk_fbi_assign_diag32, segk_fbb_partials, as
FbgmmItemSweeper.sweep enqueues them -- with the specification kept on the device's own state: after step b it takes the
device's slots and recomputes its partial sums of block b.  Per step:

  * the probe (prefilled with NaN) holds finite rows for exactly the considered items of the block;
  * occupied slots: |got - want| <= 1e-4 max(|want|, 1) against FbgmmItems.loglik on the same statistics;
  * empty slots: the row's prior predictive at 1e-9 (the fp64 path);
  * every item's slot is draw_chunked of the specification's prior term, annealing and u01(seed, sweep, i, 1) applied to the
    device's OWN probe likelihoods -- for every item whose uniform lies 1e-6 or more from an edge; items nearer are skipped and
    may not exceed 1 % of the draws;
  * the cell's partial sums equal the specification's from the same slots at 1e-13.

The SETTLED cases of tests/fbgmm_items_f32.py -- slots of thousands of items, where the rounding of a float32 term is multiplied
by the slot's count -- are walked in the same way on f32.PROBES rows a step (`walk_settled`), after those rows have shown that
the term without its compensation would miss the contract on them by 2 x or more.

Measured worst likelihood error per case (MI355X; printed by every run): see the table of DESIGN.md 4.16.1.
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def walk(gpu, case, transform="identity", consider_unassigned=True, what=""):
    """The case's sweeps step by step (module docstring); returns (specification, model) with both in the state after them."""
    from segmentalist_amd import _abi
    spec = f32.spec_of(case, transform)
    m = f32.product_of(case, transform)
    assert np.array_equal(m.components.assignments, spec.slot)
    sw = m._get_sweeper()
    assert sw.score_precision == "f32" and sw.tab32 is not None and sw.centre is not None
    assert np.array_equal(sw.centre.cpu().numpy(), f32.centre_of(spec.X))
    N, K = len(spec.slot), spec.K_max
    probe = gpu.empty((N, K), dtype=gpu.float64, device="cuda")
    sw.enter()
    L, ctx, cp, fp, bp, st = sw._args()
    cu = 1 if consider_unassigned else 0
    worst = worst_empty = worst_partials = 0.0
    draws = skipped = 0
    for sweep_index, temp in enumerate(case[8]):
        for b in range(spec.B):
            probe.fill_(float("nan"))
            _abi.check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
            _abi.check(L.segk_fbi_assign_diag32(ctx, cp, fp, bp, 0, sw.S, b, sw._n_items[b], sweep_index, float(temp), cu,
                                                _abi.ptr(sw.new_tok), _abi.ptr(sw.n_new), _abi.ptr(probe), K, st))
            _abi.check(L.segk_fbb_partials(ctx, cp, fp, bp, 0, sw.S, b, _abi.ptr(sw.new_tok), _abi.ptr(sw.n_new), st))
            gpu.cuda.synchronize()
            m.components.dev.check_status()
            got, slots = probe.cpu().numpy(), sw.slot.cpu().numpy()
            where = "%s sweep %d step %d" % (what, sweep_index, b)
            items = f32.considered(spec, b, consider_unassigned)
            others = np.setdiff1d(np.arange(N), items)
            assert np.isfinite(got[items]).all(), where
            assert np.isnan(got[others]).all(), where
            before = spec.slot.copy()
            d, items, want, p, u, new = f32.step(spec, sweep_index, b, temp, consider_unassigned,
                                                 likelihoods=lambda d, items: got[items])
            assert np.array_equal(slots[others], before[others]), where
            if items:
                occ = d["active"]
                worst = max(worst, f32.rel(got[items][:, occ], want[:, occ]))
                worst_empty = max(worst_empty, f32.rel(got[items][:, ~occ], want[:, ~occ]))
                for j, i in enumerate(items):
                    draws += 1
                    if f32.margin(p[j], u[j]) < fi.DRAW_MARGIN:
                        skipped += 1
                    else:
                        assert slots[i] == new[j], (where, i)
                assert np.all((slots[items] >= 0) & (slots[items] < K)), where
            f32.apply_slots(spec, b, items, slots[items])           # the specification goes on from the device's slots
            assert np.array_equal(slots, spec.slot), where
            for s in range(spec.S):
                cnt, sx, sxx = sw.cell_partials(b, s)
                rc, rx, rxx = spec.P[s][b]
                assert np.array_equal(cnt, rc), where
                worst_partials = max(worst_partials, f32.rel(sx, rx), f32.rel(sxx, rxx))
    sw.sweep_index = len(case[8])
    print("%s: worst likelihood error %.3g (occupied), %.3g (empty); partials %.3g; %d draws, %d skipped near an edge"
          % (what, worst, worst_empty, worst_partials, draws, skipped))
    assert worst <= f32.CONTRACT, what
    assert worst_empty <= 1e-9, what
    assert worst_partials <= 1e-13, what
    assert skipped <= f32.NEAR_EDGE * draws, what
    return spec, m


def walk_settled(gpu, name, transform="identity", map_assign=False):
    """A case of f32.SETTLED (slots of thousands of items) one Gibbs step at a time, sampled (segk_fbi_assign_diag32) or MAP
    (segk_fbi_assign_map_diag32; tests/test_gpu_fbgmm_items_map.py): the specification is evaluated on f32.PROBES rows of
    every step, on the device's own slots; the rest of the walk's checks on those rows.  First of all the rows must be able to
    tell the compensated term from the plain one: the emulation without the compensation misses the contract by 2 x or more
    on them.  Returns the worst likelihood error over the occupied slots."""
    from segmentalist_amd import _abi
    case = f32.SETTLED[name]
    what = "%s %s%s" % (name, transform, " MAP" if map_assign else "")
    spec = f32.spec_of(case, transform)
    f32.discriminates(spec, what)                  # (first, on the settled start; once more below on the state the walk saw)
    m = f32.product_of(case, transform)
    sw = m._get_sweeper()
    assert sw.score_diag32 and np.array_equal(sw.centre.cpu().numpy(), f32.centre_of(spec.X))
    centre = f32.centre_of(spec.X)
    N, K = len(spec.slot), spec.K_max
    probe = gpu.empty((N, K), dtype=gpu.float64, device="cuda")
    sw.enter()
    L, ctx, cp, fp, bp, st = sw._args()
    worst = worst_empty = worst_partials = emulated = plain = 0.0
    draws = skipped = 0
    for sweep_index, temp in enumerate(case[8]):
        sw.n_moved.zero_()
        moved = 0
        for b in range(spec.B):
            probe.fill_(float("nan"))
            _abi.check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
            if map_assign:
                _abi.check(L.segk_fbi_assign_map_diag32(ctx, cp, fp, bp, 0, sw.S, b, sw._n_items[b], sweep_index, 1, _abi.ptr(sw.new_tok),
                                                        _abi.ptr(sw.n_new), _abi.ptr(probe), K, _abi.ptr(sw.n_moved), st))
            else:
                _abi.check(L.segk_fbi_assign_diag32(ctx, cp, fp, bp, 0, sw.S, b, sw._n_items[b], sweep_index, float(temp), 1,
                                                    _abi.ptr(sw.new_tok), _abi.ptr(sw.n_new), _abi.ptr(probe), K, st))
            _abi.check(L.segk_fbb_partials(ctx, cp, fp, bp, 0, sw.S, b, _abi.ptr(sw.new_tok), _abi.ptr(sw.n_new), st))
            gpu.cuda.synchronize()
            m.components.dev.check_status()
            where = "%s sweep %d step %d" % (what, sweep_index, b)
            items = np.array(f32.considered(spec, b, True))
            rows = f32.probe_rows(items)
            got, slots = probe[gpu.from_numpy(rows).cuda()].cpu().numpy(), sw.slot.cpu().numpy()
            assert np.isfinite(got).all(), where
            d = spec.derive(*spec.stats_excluding(b))
            occ = d["active"]
            want, e, e_new, e_old = f32.compare(spec, d, spec.X[rows], got, centre)
            worst, emulated, plain = max(worst, e), max(emulated, e_new), max(plain, e_old)
            worst_empty = max(worst_empty, f32.rel(got[:, ~occ], want[:, ~occ]))
            # the slots of the probed items: the fp64 functions of the device's OWN likelihoods
            if map_assign:
                pz = np.log(float(spec.alpha) / K + d["cnt"])
                for j, i in enumerate(rows):
                    z = pz + got[j]
                    k = int(np.argmax(z))
                    below = z[z < z[k]]
                    draws += 1
                    if len(below) and z[k] - below.max() < 1e-9 * max(1.0, abs(z[k])):
                        skipped += 1
                    else:
                        assert slots[i] == k, (where, i)
            else:
                pz = spec.prior_z(d, None, None, None)
                for j, i in enumerate(rows):
                    p, u = spec._probabilities(pz + got[j], temp), f32.nb.u01(spec.seed, sweep_index, int(i), 1)
                    draws += 1
                    if f32.margin(p, u) < fi.DRAW_MARGIN:
                        skipped += 1
                    else:
                        assert slots[i] == f32.nb.draw_chunked(p, u), (where, i)
            others = np.setdiff1d(np.arange(N), items)
            assert np.array_equal(slots[others], spec.slot[others]), where
            assert np.all((slots >= 0) & (slots < K)), where
            moved += int(np.count_nonzero(slots[items] != spec.slot[items]))
            f32.apply_slots(spec, b, items, slots[items])           # the specification goes on from the device's slots
            for s in range(spec.S):
                cnt, sx, sxx = sw.cell_partials(b, s)
                rc, rx, rxx = spec.P[s][b]
                assert np.array_equal(cnt, rc), where
                worst_partials = max(worst_partials, f32.rel(sx, rx), f32.rel(sxx, rxx))
        assert not map_assign or sw.moved() == moved, what
    n_k = int(spec.stats_excluding(-1)[0].max())
    print("%s: largest slot %d items; worst likelihood error %.3g (occupied), %.3g (empty) on %d probes a step; the emulation %.3g, "
          "without the compensation %.3g; partials %.3g; %d slots compared, %d skipped near an edge"
          % (what, n_k, worst, worst_empty, f32.PROBES, emulated, plain, worst_partials, draws, skipped))
    assert plain >= f32.DISCRIMINATES * f32.CONTRACT, what             # (the inputs: or the rows prove nothing)
    assert worst <= f32.CONTRACT, what
    assert worst_empty <= 1e-9, what
    assert worst_partials <= 1e-13, what
    assert skipped <= f32.NEAR_EDGE * draws, what
    return worst


@pytest.mark.parametrize("name,transform", f32.SETTLED_RUNS, ids=f32.SETTLED_IDS)
def test_steps_on_settled_slots_of_thousands_of_items(gpu, name, transform):
    """the contract where a float32 term's rounding is multiplied by a slot's count: DESIGN.md 4.16.1 holds the figures"""
    walk_settled(gpu, name, transform)


@pytest.fixture(scope="module")
def finished(gpu):
    """name -> (specification, model) after the walk of test_steps (later tests go on from there)"""
    return {}


@pytest.mark.parametrize("name", list(f32.CASES))
def test_steps(gpu, finished, monkeypatch, name):
    if name == "dg_D39_K300_8x8":
        # the workspace bound at 1 MiB holds six tiles of K_max | 1 = 301 doubles x 64: the block's eight take two launches
        monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")
    finished[name] = walk(gpu, f32.CASES[name], what=name)


@pytest.mark.parametrize("name", f32.UNASSIGNED)
def test_steps_without_the_unassigned(gpu, name):
    spec, m = walk(gpu, f32.CASES[name], consider_unassigned=False, what=name + " assigned only")
    assert np.count_nonzero(spec.slot < 0) >= 1


def test_logits_in_lds_and_in_the_workspace():
    """the two K_max of the cases dg_D39_Klds / dg_D39_Kws lie on either side of the kernel's byte count (the constants are
    held against the source by tests/test_fbgmm_items_f32_cpu.py); test_steps walks both"""
    lo, hi = f32.CASES["dg_D39_Klds"][3], f32.CASES["dg_D39_Kws"][3]
    assert hi == lo + 1 and f32.lds_bytes(39, lo) <= f32.LDS_MAX < f32.lds_bytes(39, hi)


TRANSFORMED = [(n, t) for n, t in f32.RUNS if t != "identity"]


@pytest.mark.parametrize("name,transform", TRANSFORMED, ids=["%s-%s" % r for r in TRANSFORMED])
def test_steps_on_transformed_corpora(gpu, name, transform):
    """prior and data moved together (tests/affine.py): the same contract in the new coordinates"""
    walk(gpu, f32.CASES[name], transform, what="%s %s" % (name, transform))


def test_f64_passed_explicitly(gpu):
    """score_precision="f64": the fp64 path, the slots of fi.run_spec sweep for sweep"""
    name = "dg_D39_K65_n257"
    case = f32.CASES[name]
    want = fi.run_spec(name)
    m = f32.product_of(case, score_precision="f64")
    sw = m._get_sweeper()
    assert sw.score_precision == "f64" and sw.tab32 is None and sw.centre is None
    for s, temp in enumerate(case[8]):
        m.batch_sweep_async(temp, True)
        gpu.cuda.synchronize()
        assert np.array_equal(sw.slot.cpu().numpy(), want.history[s]), s
    m.components.dev.check_status()


def same_view(gpu, m, spec, case):
    """materialise(): assignments and K are canonical() of the slots; the serial statistics are, bit for bit, those of a fresh
    model constructed from those assignments"""
    canon, K = spec.canonical()
    c = m.components
    assert c.K == K and np.array_equal(c.assignments, canon)
    fresh = f32.product_of(case, assignments=canon)
    a, b = c.dev, fresh.components.dev
    for nm in ("counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "K", "assignments"):
        assert gpu.equal(getattr(a, nm), getattr(b, nm)), nm


@pytest.mark.parametrize("name", ["dg_D39_K65_n257", "dg_D39_K7_un"])
def test_materialise_after_f32_sweeps(gpu, finished, monkeypatch, name):
    if name not in finished:
        test_steps(gpu, finished, monkeypatch, name)
    spec, m = finished[name]
    m.materialise()
    same_view(gpu, m, spec, f32.CASES[name])
    assert m._get_sweeper().in_batch_state
    assert np.array_equal(m._get_sweeper().slot.cpu().numpy(), spec.slot)          # (the batch state is not touched)


def test_serial_sweep_between_f32_batch_sweeps(gpu):
    """batch_sweep_async (f32), a serial gibbs_sample(1), batch again: the serial call leaves batch mode, the next batch sweep
    re-enters it from the serial result"""
    case = f32.CASES["dg_D39_K65_n257"]
    m = f32.product_of(case)
    sw = m._get_sweeper()
    m.batch_sweep_async()
    gpu.cuda.synchronize()
    assert sw.in_batch_state and sw.sweep_index == 1
    first = sw.slot.cpu().numpy().copy()
    random.seed(5)
    m.gibbs_sample(1)
    assert not sw.in_batch_state
    serial = np.array(m.components.assignments)
    assert serial.min() >= 0 and np.count_nonzero(first >= 0) == len(serial)
    m.batch_sweep_async()
    gpu.cuda.synchronize()
    m.components.dev.check_status()
    assert sw.in_batch_state and sw.sweep_index == 2 and m._get_sweeper() is sw
    # the batch state was rebuilt from the serial result: all items hold a slot, the counts add up
    cnt, total, occupied = sw.totals()
    assert total == len(serial) and occupied == len(set(sw.slot.cpu().numpy().tolist()))
    m.materialise()
    assert m.components.K == occupied


def test_record_of_gibbs_sample_batch_f32(gpu):
    case = f32.CASES["dg_D39_K7_un"]
    m = f32.product_of(case)
    state = random.getstate()
    rec = m.gibbs_sample(2, sync="batch")
    assert random.getstate() == state                         # no random.random() is consumed
    assert sorted(rec) == ["anneal_temp", "components", "log_marg", "log_prob_X_given_z", "log_prob_z", "sample_time"]
    for k, v in rec.items():
        assert len(v) == 2 and np.all(np.isfinite(np.asarray(v, np.float64))), k
    assert m._get_sweeper().score_precision == "f32" and m._get_sweeper().sweep_index == 2


def test_object_in_batch_mode_f32(gpu):
    """FBGMM(..., sync="batch", score_precision="f32"): gibbs_sample without a sync argument runs the float32 batch sweeps"""
    case = f32.CASES["dg_D39_K7_n255"]
    m = f32.product_of(case, sync="batch")
    m.gibbs_sample(1)
    sw = m._get_sweeper()
    assert sw.score_diag32 and sw.sweep_index == 1 and sw.in_batch_state


def test_refusals(gpu):
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    rs = np.random.RandomState(3)
    X = rs.randn(12, 3).astype(np.float32)
    a = np.arange(12) % 3
    with pytest.raises(SegkError, match="diagonal components"):
        FBGMM(X, FixedVarPrior(*fi.prior_params("fixed", 3)), fi.ALPHA, 4, a, covariance_type="fixed", score_precision="f32")
    with pytest.raises(SegkError, match="diagonal components"):
        FBGMM(X, NIW(*fi.prior_params("full", 3)), fi.ALPHA, 4, a, covariance_type="full", score_precision="f32")
    with pytest.raises(SegkError, match="f16"):
        FBGMM(X, NIW(*fi.prior_params("diag", 3)), fi.ALPHA, 4, a, covariance_type="diag", score_precision="f16")
    # the sweeper itself refuses too (a model built before the keyword was set)
    from segmentalist_amd.device import FbgmmItemSweeper
    fx = FBGMM(X, FixedVarPrior(*fi.prior_params("fixed", 3)), fi.ALPHA, 4, a, covariance_type="fixed")
    with pytest.raises(SegkError, match="diagonal components"):
        FbgmmItemSweeper(fx.components.dev, 2, 2, 0, score_precision="f32")
    with pytest.raises(SegkError, match="f16"):
        FbgmmItemSweeper(fx.components.dev, 2, 2, 0, score_precision="f16")
    # the entry point: refused before anything is launched, the reason in segk_last_error
    m = f32.product_of(f32.CASES["dg_D3_K7_n40"])
    m.batch_sweep_async()
    gpu.cuda.synchronize()
    sw = m._get_sweeper()
    L, ctx, cp, fp, bp, st = sw._args()
    slots = sw.slot.clone()

    def call(f=fp, bt=bp):
        return L.segk_fbi_assign_diag32(ctx, cp, f, bt, 0, sw.S, 0, sw._n_items[0], 7, 1.0, 1, _abi.ptr(sw.new_tok),
                                        _abi.ptr(sw.n_new), None, 0, st)
    for cov in (0, 2):
        f_cov = _abi.FbgmmDev.from_buffer_copy(sw.f)
        f_cov.cov_type = cov
        assert call(f=C.byref(f_cov)) == _abi.SEGK_ERR_UNSUPPORTED
        assert "cov_type %d" % cov in L.segk_last_error().decode()
    f_lm = _abi.FbgmmDev.from_buffer_copy(sw.f)
    f_lm.lm_unigram = m.components.dev.counts.data_ptr()
    assert call(f=C.byref(f_lm)) == _abi.SEGK_ERR_UNSUPPORTED and "language model" in L.segk_last_error().decode()
    for field in ("tab32", "centre", "prior_rows"):
        bt = _abi.FbatchDev.from_buffer_copy(sw.bt)
        setattr(bt, field, None)
        rc = call(bt=C.byref(bt))
        assert rc == -1 and "tab32" in L.segk_last_error().decode(), field              # SEGK_ERR_ARG
    gpu.cuda.synchronize()
    assert gpu.equal(sw.slot, slots)                           # nothing was launched
    m.components.dev.check_status()

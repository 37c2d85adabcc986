"""
The specification of the MAP sweeps of the stand-alone mixture model (tests/fbgmm_items_map.py), checked with the oracle alone:
every case is one on which exact parity of an argmax is defined, and the sweeps have the properties the device tests
(tests/test_gpu_fbgmm_items_map.py) and FBGMM.map_assign's documentation rest on.

The margins are conditions on the INPUTS.  Should a later change of a case break one, drop that case by name from the lists of
tests/fbgmm_items_map.py -- keeping every covariance type and both dtypes -- rather than lowering MARGIN.
"""
import copy
import ctypes
import os
import random
import re

import numpy as np
import pytest

from tests import fbgmm_items as fi
from tests import fbgmm_items_map as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(pairs):
    return ["%s%s" % (n, "" if cu else "/assigned") for n, cu in pairs]


def _report(what, cen):
    print("%s: %d decisions, least gap %.3g absolute, %.3g relative; %d ties among empty slots; moved %s; emptied %d, founded %d"
          % (what, cen.decisions, cen.gap_abs, cen.gap_rel, cen.empty_ties, cen.moved, cen.emptied, cen.founded))


def _holds_margin(cen):
    assert cen.decisions >= 1
    assert cen.gap_rel >= fm.MARGIN
    assert cen.tie_on_occupied == 0
    assert cen.softmax_disagrees == 0


@pytest.mark.parametrize("name,cu", fm.BATCH, ids=_ids(fm.BATCH))
def test_batch_decisions_keep_the_margin(name, cu):
    """every decision of the four MAP sweeps lies MARGIN clear of its best competitor, ties are among empty slots only, and
    the reference's argmax(exp(z - logsumexp z)) is the argmax of z; the first sweep moves an item unless the shape is one of
    the named degenerate ones"""
    state = random.getstate()
    spec = fm.run_batch(name, cu)
    assert random.getstate() == state
    _report(name, spec.census)
    _holds_margin(spec.census)
    assert len(spec.census.moved) == fm.N_SWEEPS
    if name in fm.DEGENERATE:
        assert spec.census.moved == [0] * fm.N_SWEEPS
    else:
        assert spec.census.moved[0] >= 1


@pytest.mark.parametrize("name", fm.F32)
def test_float32_cases_keep_the_margin_in_fp64(name):
    """the cases of the float32 device test: their fp64 decisions keep the margin too (the device test skips an item only
    where the top two of ITS logits are within 1e-9, and expects to skip none)"""
    spec = fm.run_batch(name, True)
    _report(name, spec.census)
    _holds_margin(spec.census)
    assert name in fm.DEGENERATE or spec.census.moved[0] >= 1


def test_cases_keep_every_covariance_type_and_dtype():
    cases = [fi.CASES[n] for n, _ in fm.BATCH]
    assert {c[0] for c in cases} == {"fixed", "diag", "full"} and {c[1] for c in cases} == {"float32", "float64"}
    assert {c[3] for c in cases} >= {1, 7, 65, 130, 300, 1100}
    serial = [fm.case_of(n) for n, _ in fm.SERIAL_FORM] + [fm.case_of(n) for n in fm.SERIAL]
    assert {c[0] for c in serial} == {"fixed", "diag", "full"} and {c[1] for c in serial} == {"float32", "float64"}
    assert {fm.case_of(n)[0] for n in fm.F32} == {"diag"}


@pytest.mark.parametrize("name,cu", fm.SERIAL_FORM + [(n, True) for n in fm.SERIAL],
                         ids=_ids(fm.SERIAL_FORM + [(n, True) for n in fm.SERIAL]))
def test_serial_decisions_keep_the_margin(name, cu):
    """the serial form on its cases: the margin at every decision, no uniform consumed, and log_marg() non-decreasing from
    one sweep to the next wherever the sweep assigned no new item"""
    state = random.getstate()
    run = fm.run_serial(name, cu)
    assert random.getstate() == state
    _report(name, run.census)
    _holds_margin(run.census)
    lm = [r["log_marg"] for r in run.record]
    print("%s: log_marg %s, assigned %s" % (name, lm, run.assigned))
    for s in range(1, fm.N_SWEEPS):
        if run.assigned[s] == run.assigned[s - 1]:
            assert lm[s] >= lm[s - 1] - 1e-9 * abs(lm[s - 1]), (name, s)
    if not cu:
        start = fi.make_inputs(fm.case_of(name))[1]
        assert np.array_equal(run.assignments[-1] < 0, start < 0)


@pytest.mark.parametrize("name", fm.SERIAL)
def test_one_item_per_block_is_the_serial_sweep(name):
    """at most one item per block and S = 1: every item is decided against everything but itself, in index order -- the
    batch sweep's canonical labels name the partition the serial sweep reaches, sweep for sweep, with the same n_moved"""
    case = fi.SERIAL[name]
    assert case[6] <= case[4] * case[5] and case[5] == 1
    batch, serial = fm.run_batch(name, True), fm.run_serial(name, True)
    for s in range(fm.N_SWEEPS):
        canon, K = batch.canon[s]
        assert K == serial.K[s]
        assert np.array_equal(fm.partition(canon), fm.partition(serial.assignments[s])), (name, s)
    assert batch.census.moved == serial.moved


@pytest.mark.parametrize("name,within", [("dg_D39_K65_n257", 4), ("fx_D39_K7_n255", 3)])
def test_fixed_point(name, within):
    """n_moved == 0 within the stated number of sweeps, and a sweep that moves nothing changes neither the slots nor the
    partial sums (bit for bit); the serial form leaves every statistic bit-identical"""
    spec = fm.run_batch(name, True)
    assert 0 in spec.census.moved[:within]
    am, live = fm.spec_of(fi.CASES[name])
    n = 0
    while live.sweep(n) != 0:
        n += 1
        assert n < within
    slots = live.slot.copy()
    P = [[tuple(np.copy(a) for a in live.P[s][b]) for b in range(live.B)] for s in range(live.S)]
    assert live.sweep(n + 1) == 0
    assert np.array_equal(live.slot, slots)
    for s in range(live.S):
        for b in range(live.B):
            for got, want in zip(live.P[s][b], P[s][b]):
                assert np.array_equal(got, want)
    # serial
    run = fm.run_serial(name, True)
    assert run.moved[-1] == 0
    am = copy.deepcopy(run.am)                    # (the run is shared)
    c = am.components
    names = [k for k, v in vars(c).items() if isinstance(v, np.ndarray) and k != "X"]
    kept = {k: np.copy(getattr(c, k)) for k in names}
    K = c.K
    assert fm.serial_map_sweep(am, True) == 0
    assert c.K == K and len(names) >= 4
    for k in names:
        assert np.array_equal(getattr(c, k), kept[k]), k


def test_sampled_sweeps_after_a_map_sweep_use_their_own_uniforms():
    """a MAP sweep takes one value of sweep_index and reads no uniform: the mixed plan on the MAP specification is the plain
    specification's sampled sweep at the same index from the same state"""
    for name in fm.MIXED:
        case = fi.CASES[name]
        am, spec = fm.spec_of(case)
        for s, is_map in enumerate(fm.MIXED_PLAN):
            if not is_map:
                _, plain = fi.spec_of(case, assignments=None)
                plain.slot = spec.slot.copy()
                plain.P = [[plain._partial(ss, b) for b in range(plain.B)] for ss in range(plain.S)]
                plain.sweep(s, 1.0, True)
            spec.sweep(s, 1.0, True, map_assign=is_map)
            if not is_map:
                assert np.array_equal(spec.slot, plain.slot), (name, s)


def test_abi_and_the_new_entry_points():
    """header, library and binding: ABI 15 without a bump, the three symbols exported, bound, declared with the reference
    lines they replace"""
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("segk_fbi_assign_map", "segk_fbi_assign_map_diag32", "segk_fbgmm_map_items"):
        assert hasattr(lib, sym) and sym in _abi.SIGNATURES, sym
        assert re.search(r"\b%s\s*\(" % sym, code), sym
    assert "fbgmm.py:465-494" in hdr and "475-491" in hdr

"""`FBGMM(..., sync="batch", score_precision="f32")` on the CPU: the inputs of tests/test_gpu_fbgmm_items_f32.py checked before
the device is asked anything (as tests/test_anneal_batch_cpu.py does for the annealing cases), and the ABI the feature adds.

1. the NumPy emulation of the float32 terms (tests/fbgmm_items_f32.py `emulate`) stays within 5e-5 -- half the contract -- of the
   fp64 specification on every (case, transform) the GPU file runs;
2. in every case at least 99 % of the specification's draws lie fi.DRAW_MARGIN or more from every edge of their cumulative
   distribution (a uniform puts about K_max * 2e-6 of them nearer);
3. every case with more than one slot founds and empties a slot over its sweeps, every annealed sweep changes draws against
   T = 1;
4. header, binding and library carry segk_fbi_assign_diag32 at ABI 15;
5. on the SETTLED cases (slots of thousands of items) the emulation stays within 5e-5 while the emulation of the term WITHOUT
   its compensation (`emulate_uncompensated`) misses the contract by 2 x or more: the inputs can show the defect.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs():
    """(name, transform) -> the specification's run with the emulation beside it, computed once"""
    return {}


def _run(runs, name, transform):
    if (name, transform) not in runs:
        runs[(name, transform)] = f32.run(name, transform)
    return runs[(name, transform)]


@pytest.mark.parametrize("name,transform", f32.RUNS, ids=["%s-%s" % r for r in f32.RUNS])
def test_emulation_within_half_the_contract(runs, name, transform):
    r = _run(runs, name, transform)
    print("%s %s: emulation worst %.3g over %d draws" % (name, transform, r.worst, r.draws))
    assert r.draws >= 1 and r.worst <= f32.EMULATION


@pytest.mark.parametrize("name,transform", f32.SETTLED_RUNS, ids=f32.SETTLED_IDS)
def test_settled_cases_tell_the_compensated_term_from_the_plain_one(name, transform):
    """slots of thousands of items (f32.SETTLED): the emulation stays within half the contract, and the emulation WITHOUT the
    compensation misses the contract by 2 x or more -- on the probes of the Gibbs steps and on the held-out rows alike.  The
    second is a condition on the inputs: a case that does not meet it could not show the defect and must be chosen again."""
    figures, n_k = f32.settled_figures(name, transform)
    for what, (new, old) in sorted(figures.items()):
        print("%s %s, largest slot %d items, %s: emulation %.3g, without the compensation %.3g" % (name, transform, n_k, what, new, old))
    assert n_k >= 2000
    for new, old in figures.values():
        assert new <= f32.EMULATION
        assert old >= f32.DISCRIMINATES * f32.CONTRACT


def test_the_plain_term_misses_nothing_on_the_small_cases():
    """why CASES alone never saw it: with a handful of items a slot the term without the compensation is as good"""
    case = f32.CASES["dg_D39_K300_8x8"]
    spec = f32.spec_of(case)
    d = spec.derive(*spec.stats_excluding(-1))
    rows = f32.probe_rows(case[6])
    _, _, new, old = f32.compare(spec, d, spec.X[rows])
    print("dg_D39_K300_8x8, largest slot %d items: emulation %.3g, without the compensation %.3g" % (d["cnt"].max(), new, old))
    assert new <= f32.EMULATION and old <= f32.EMULATION


@pytest.mark.parametrize("name,transform", f32.RUNS, ids=["%s-%s" % r for r in f32.RUNS])
def test_draws_keep_clear_of_the_edges(runs, name, transform):
    r = _run(runs, name, transform)
    print("%s %s: %d of %d draws within %.0e of an edge" % (name, transform, r.near, r.draws, fi.DRAW_MARGIN))
    assert r.near <= f32.NEAR_EDGE * r.draws


@pytest.mark.parametrize("name", list(f32.CASES))
def test_slots_are_founded_and_emptied_and_annealing_changes_draws(runs, name):
    case, r = f32.CASES[name], _run(runs, name, "identity")
    print("%s: emptied %d, founded %d, changed by T %s" % (name, r.emptied, r.founded, r.changed_by_T))
    if case[3] > 1:
        assert r.emptied >= 1 and r.founded >= 1
    for temp, changed in zip(case[8], r.changed_by_T):
        assert temp == 1 or changed >= 1


@pytest.mark.parametrize("name", f32.UNASSIGNED)
def test_without_the_unassigned(name):
    """consider_unassigned=False from the same start: the emulation and the margins hold there too, the items never
    considered stay unassigned, and the run ends elsewhere than the one that considers them"""
    case = f32.CASES[name]
    r = f32.run(name, consider_unassigned=False)
    start = fi.make_inputs(case)[1]
    assert np.count_nonzero(start < 0) >= 0.2 * len(start)
    assert r.worst <= f32.EMULATION and r.near <= f32.NEAR_EDGE * r.draws
    assert np.array_equal(r.history[-1] < 0, start < 0)
    assert np.count_nonzero(f32.run(name).history[-1] != r.history[-1]) >= 1


@pytest.mark.parametrize("name", ["dg_D39_K65_n257", "dg_D3_K7_n1", "dg_D39_K7_un"])
def test_stepwise_walk_is_the_specifications_sweep(runs, name):
    """f32.step block by block is fi's sweep: on the cases shared with fi.CASES the slots after every sweep coincide"""
    want = fi.run_spec(name)
    got = _run(runs, name, "identity")
    for a, b in zip(got.history, want.history):
        assert np.array_equal(a, b)


def test_cases_walk_the_kernels_paths():
    cases = f32.CASES
    assert all(c[0] == "diag" for c in cases.values())
    assert {c[1] for c in cases.values()} == {"float32", "float64"}
    # the three loops of fbb_accumulate_rows32 (16 + 4 + 1), 16 exactly, the limit
    assert {3, 16, 21, 39, 100, 256} == {c[2] for c in cases.values()}
    assert {1, 7, 1100} <= {c[3] for c in cases.values()} and max(c[3] for c in cases.values()) > 1024
    cells = set()
    for c in cases.values():
        spec_ranges = f32.spec_of(c).ranges if c[6] <= 300 else []
        cells |= {hi - lo for row in spec_ranges for lo, hi in row}
    assert {0, 1, f32.TILE - 1, f32.TILE, f32.TILE + 1} <= cells
    # the two K_max on either side of the LDS formula at D = 39
    assert cases["dg_D39_Klds"][3] + 1 == cases["dg_D39_Kws"][3]
    assert f32.lds_bytes(39, cases["dg_D39_Klds"][3]) <= f32.LDS_MAX < f32.lds_bytes(39, cases["dg_D39_Kws"][3])
    assert f32.stage_bytes(256) <= f32.LDS_MAX                     # the D limit stages
    # eight tiles a block, and a workspace bound of 1 MiB holds fewer
    c = cases["dg_D39_K300_8x8"]
    spec = f32.spec_of(c)
    tiles = sum((hi - lo + f32.TILE - 1) // f32.TILE for row in spec.ranges for (lo, hi) in row[:1])
    assert f32.lds_bytes(39, c[3]) > f32.LDS_MAX and tiles == 8 > (1 << 20) // (f32.TILE * (c[3] | 1) * 8) >= 4


def test_byte_count_is_the_kernels():
    """the constants of f32.lds_bytes against the kernel's source"""
    src = open(os.path.join(ROOT, "segmentalist_amd", "csrc", "segk_fbitems.hip")).read()

    def define(name):
        return re.search(r"#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, src, flags=re.M).group(1)
    assert int(define("FBI_T")) == f32.TILE
    assert int(define("FBI32_KW")) * int(define("FBI32_NT")) // 64 == f32.KC and define("FBI32_KC") == "(FBI32_KW * (FBI32_NT / 64))"
    assert define("FBI32_XS") == "(FBI_T + 1)" and f32.XS == f32.TILE + 1
    assert define("FBI_LDS_MAX") == "(144 * 1024)" and f32.LDS_MAX == 144 * 1024
    assert "return ((2 * (size_t)FBI32_KC * D + (size_t)FBI32_XS * D) * sizeof(float) + 15) & ~(size_t)15;" in src
    assert "fbi32_ldl(int KM) { return KM | 1; }" in src


def test_abi_15_and_the_float32_entry_point():
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    assert re.search(r"\bsegk_fbi_assign_diag32\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    sig = _abi.SIGNATURES
    assert "segk_fbi_assign_diag32" in sig
    assert sig["segk_fbi_assign_diag32"][0] is sig["segk_fbi_assign"][0]
    assert len(sig["segk_fbi_assign_diag32"][1]) == len(sig["segk_fbi_assign"][1]) == 16
    assert sig["segk_fbi_assign_diag32"][1] == sig["segk_fbi_assign"][1]
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "segk_fbi_assign_diag32")
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION

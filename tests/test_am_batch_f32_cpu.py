"""The float32 acoustic-model batch sweeps (`am_sweep(..., score_precision="f32")`) on the CPU: the inputs of
tests/test_gpu_am_batch_f32.py checked before the device is asked anything, and the ABI the feature adds.

1. the NumPy emulation of the float32 terms (tests/fbgmm_items_f32.py `emulate` on token rows) stays within 5e-5 -- half the
   contract -- of the fp64 specification on every (case, transform) the GPU file runs, along the emulated trajectory;
2. at most 1 % of the draws lie within 1e-6 of an edge of their cumulative distribution;
3. every case founds a slot, every case but NO_SLOT_EMPTIED empties one;
4. the annealed sweeps change a draw against T = 1;
5. the cases walk the kernel's paths, the byte-count constants are the source's;
6. header, binding and library carry segk_fbt_assign_diag32 at ABI 15; the Python surface has the new keywords.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import am_batch as ab
from tests import am_batch_f32 as a32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["%s-%s" % r for r in a32.RUNS]


@pytest.fixture(scope="module")
def runs():
    """(name, transform) -> the run along the emulated trajectory, computed once"""
    return {}


def _run(runs, name, transform="identity"):
    if (name, transform) not in runs:
        runs[(name, transform)] = a32.run(name, transform)
    return runs[(name, transform)]


@pytest.mark.parametrize("name,transform", a32.RUNS, ids=IDS)
def test_emulation_within_half_the_contract(runs, name, transform):
    r = _run(runs, name, transform)
    print("%s %s: emulation worst %.3g over %d draws" % (name, transform, r.worst, r.draws))
    assert r.draws >= 1 and r.worst <= a32.EMULATION


def test_settled_case_tells_the_compensated_term_from_the_plain_one():
    """a32.SETTLED, slots of thousands of tokens: the emulation stays within half the contract and the emulation WITHOUT the
    compensation misses the contract by 2 x or more on the probes of every Gibbs step -- a condition on the inputs of the
    device test; about five tokens a slot (every case of CASES) cannot tell the two apart"""
    figures, n_k = a32.f32.settled_figures(a32.SETTLED)
    new, old = figures["steps"]
    print("%s, largest slot %d tokens: emulation %.3g, without the compensation %.3g" % (a32.SETTLED, n_k, new, old))
    assert n_k >= 2000 and new <= a32.EMULATION and old >= a32.f32.DISCRIMINATES * a32.CONTRACT
    case = a32.CASES["dg_D39_K65_tiles"]
    _, spec = a32.spec_of(case)
    d = spec.derive(*spec.stats_excluding(-1))
    rows = [e for i in range(spec.seg.utterances.D) for e in spec._tokens(i)]
    _, _, new, old = a32.f32.compare(spec, d, spec.X[rows])
    print("dg_D39_K65_tiles, largest slot %d tokens: emulation %.3g, without the compensation %.3g" % (d["cnt"].max(), new, old))
    assert new <= a32.EMULATION and old <= a32.EMULATION


def test_settled_multi_landmark_corpus_tells_the_compensated_term_from_the_plain_one():
    """a32.SETTLED_SEG: two slots of about 2 000 tokens, utterances of three to eight tokens, span rows of every duration in a
    block.  On the probes of every block the span scores of the emulation stay within half the contract and those of the
    emulation WITHOUT the compensation miss the contract by 2 x or more: a condition on the inputs of the device test."""
    corpus, bounds, spec = a32.settled_seg_spec()
    cnt = spec.stats_excluding(-1)[0]
    assert sorted(cnt[cnt > 0].tolist())[0] >= 2000 and np.count_nonzero(cnt) == a32.N_CENTRES
    assert {len(spec._tokens(i)) for i in range(spec.seg.utterances.D)} == {3, 4, 5, 6, 8}
    centre = a32.centre_of(spec.X)
    for b in range(spec.B):
        assert len({dur for _, dur in a32.block_span_rows(spec, b)}) >= 3
        d, rows, want, want_score, new, old = a32.settled_seg_figures(spec, b, centre)
        print("settled multi-landmark corpus, block %d: span scores of the emulation %.3g, without the compensation %.3g" % (b, new, old))
        assert new <= a32.EMULATION and old >= a32.f32.DISCRIMINATES * a32.CONTRACT


@pytest.mark.parametrize("name,transform", a32.RUNS, ids=IDS)
def test_draws_keep_clear_of_the_edges(runs, name, transform):
    r = _run(runs, name, transform)
    print("%s %s: %d of %d draws within %.0e of an edge, least margin %.3g" % (name, transform, r.near, r.draws, a32.DRAW_MARGIN,
                                                                              r.least))
    assert r.near <= a32.NEAR_EDGE * r.draws


@pytest.mark.parametrize("name", list(a32.CASES))
def test_slots_are_founded_and_emptied(runs, name):
    r = _run(runs, name)
    print("%s: emptied %d, founded %d" % (name, r.emptied, r.founded))
    assert r.founded >= 1
    if name not in a32.NO_SLOT_EMPTIED:
        assert r.emptied >= 1


@pytest.mark.parametrize("name", a32.ANNEALED)
def test_annealing_changes_draws(runs, name):
    case, r = a32.CASES[name], _run(runs, name)
    temps = a32.temps_of(case)
    print("%s: changed by T %s at %s" % (name, r.changed_by_T, temps))
    assert any(t != 1 for t in temps)
    for temp, changed in zip(temps, r.changed_by_T):
        assert temp == 1 or changed >= 1


def test_cases_walk_the_kernels_paths():
    cases = a32.CASES
    assert len(cases) == 12 and all(c[0] == "diag" for c in cases.values())
    assert {c[1] for c in cases.values()} == {"float32", "float64"}
    for name in ("dg_D39_K65_tiles", "dg_D100_K7_3x4", "dg_D3_K7_1x1", "dg_band_N80"):
        assert cases[name] is ab.CASES[name]
    assert cases["il_dg"] is ab.INTERLEAVED["il_dg"]
    # the three loops of fbb_accumulate_rows32 on the other route (16 + 4 + 1), 16 exactly, the limit
    assert {3, 16, 21, 39, 100, 256} <= {c[2] for c in cases.values()}
    # cells of TILE - 1, TILE, TILE + 1 tokens, of three tiles, and empty ones
    cells = {n for row in ab.cell_tokens(ab.spec_of(cases["dg_D39_K65_tiles"])[1]) for n in row}
    assert cells == {a32.TILE - 1, a32.TILE, a32.TILE + 1, 150}
    assert 0 in {n for row in ab.cell_tokens(a32.spec_of(cases["dg_D3_K7_8x8"])[1]) for n in row}
    # positions beyond 64
    assert max(cases["dg_band_N80"][6]) > 64
    # the two K_max on either side of the LDS formula at D = 39
    lo, hi = cases["dg_D39_K247_tiles"][3], cases["dg_D39_K248_tiles"][3]
    assert hi == lo + 1 and a32.lds_bytes(39, lo) <= a32.LDS_MAX < a32.lds_bytes(39, hi)
    assert a32.stage_bytes(256) <= a32.LDS_MAX                     # the D limit stages
    # eight tiles a block by the host's bound (the landmarks), and a workspace bound of 1 MiB holds fewer
    c = cases["dg_D39_K300_tiles"]
    n_utt, N, B, S = len(c[6]), c[7], c[4], c[5]
    tiles = S * ((n_utt // (B * S) * N + a32.TILE - 1) // a32.TILE)
    assert a32.lds_bytes(39, c[3]) > a32.LDS_MAX and tiles == 8 > (1 << 20) // (a32.TILE * (c[3] | 1) * 8) >= 4


def test_byte_count_is_the_kernels():
    """the constants of lds_bytes against the kernel's source; the token axis shares them"""
    src = open(os.path.join(ROOT, "segmentalist_amd", "csrc", "segk_fbitems.hip")).read()

    def define(name):
        return re.search(r"#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, src, flags=re.M).group(1)
    assert int(define("FBI_T")) == a32.TILE
    assert int(define("FBI32_KW")) * int(define("FBI32_NT")) // 64 == a32.f32.KC
    assert define("FBI32_XS") == "(FBI_T + 1)" and a32.f32.XS == a32.TILE + 1
    assert define("FBI_LDS_MAX") == "(144 * 1024)" and a32.LDS_MAX == 144 * 1024 == 147456
    assert "return ((2 * (size_t)FBI32_KC * D + (size_t)FBI32_XS * D) * sizeof(float) + 15) & ~(size_t)15;" in src
    assert "fbi32_ldl(int KM) { return KM | 1; }" in src
    # one kernel with a token axis, one placement rule for both float32 entry points
    assert re.search(r"template <typename XT, bool TOK = false>\s*__global__ __launch_bounds__\(FBI32_NT\) void k_fbi_assign_diag32", src)
    assert len(re.findall(r"\bfbi32_launch\(ctx", src)) == 2 and src.count('segk_env_int("SEGK_FBI_Z_MIB"') == 2


def test_abi_15_and_the_float32_token_entry_point():
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    assert re.search(r"\bsegk_fbt_assign_diag32\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert re.search(r"15 \(no bump\) segk_fbt_assign_diag32", hdr)
    sig = _abi.SIGNATURES
    assert "segk_fbt_assign_diag32" in sig
    assert sig["segk_fbt_assign_diag32"][0] is sig["segk_fbt_assign"][0]
    assert sig["segk_fbt_assign_diag32"][1] == sig["segk_fbt_assign"][1] and len(sig["segk_fbt_assign"][1]) == 16
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "segk_fbt_assign_diag32")
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION


def test_python_surface():
    from segmentalist_amd import device
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    p = inspect.signature(device.FbgmmBatchSweeper.am_sweep).parameters
    assert list(p) == ["self", "boundaries", "anneal_temp", "score_precision"] and p["score_precision"].default is None
    p = inspect.signature(UnigramAcousticWordseg.am_batch_sweep_async).parameters
    assert list(p) == ["self", "anneal_temp", "score_precision"] and p["score_precision"].default is None
    p = inspect.signature(UnigramAcousticWordseg.gibbs_sample).parameters
    assert list(p)[-2:] == ["am_sync", "am_score_precision"] and p["am_score_precision"].default is None
    assert isinstance(device.AM32_TILE_MIN, int) and device.AM32_TILE_MIN >= 0

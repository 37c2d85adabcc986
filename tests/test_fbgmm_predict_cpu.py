"""
What the GPU tests of `FBGMM.predict` / `score_samples` / `predict_log_proba` (tests/test_gpu_fbgmm_predict.py) rest on, held
with NumPy alone before the device is asked anything:

1. the specification tests/fbgmm_predict.py against the SERIAL oracle (oracle/np_oracle.py FBGMM; tests/fullcov.py SpecFBGMM
   for full covariance) over [X; Xq] with the queries appended unassigned -- log_marg_i, the normalised log_prob_z, map_assign_i's
   choice -- at 1e-12, and against the recorded values of the reference itself (tests/golden/predict.npz) at 1e-12;
2. the census of label decisions: every decision of every case at least MARGIN = 1e-6 (relative) clear of its best
   competitor, no tie that involves an occupied slot; per case at least one query labelled K and two distinct components;
3. the renumbering is `canonical`'s on states whose slots are not canonical; lms != 1 separates the prior terms of density
   and label;
4. the float32 emulation of the query likelihoods within 5e-5 of the fp64 ones;
5. the LDS byte counts against the source, both symbols at ABI 15.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32
from tests import fbgmm_items_map as fm
from tests import fbgmm_predict as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
# the states after the cases' own sweeps (non-canonical slots); the two shapes of 1 100 and 300 slots are left to their initial
# states: their sweeps alone take longer than every other test of this file together
SWEPT = ["fx_D39_K7_n255", "dg_D39_K65_n257", "dg_D100_K130_T10", "fx_D39_K130_n600", "dg_D39_K7_un", "fx_D39_K65_un",
         "fc_D39_K65", "fc_D64_K7_un_T10"]
SWEPT += list(fp.EDGE)
STATES = [(n, "initial") for n in list(fi.CASES) + list(fp.EDGE)] + [(n, "swept") for n in SWEPT]
GOLDEN = os.path.join(ROOT, "tests", "golden", "predict.npz")


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


_states = {}


def state(name, which):
    """(case, batch specification, Xq, its prediction, its census); shared: do not modify"""
    key = (name, which)
    if key not in _states:
        case = fp.case_of(name)
        spec = fi.spec_of(case)[1] if which == "initial" else fp.swept(name)
        Xq = fp.query_rows(case)
        census = fm.Census()
        _states[key] = (case, spec, Xq, fp.predict(spec, Xq, census), census)
    return _states[key]


def _ids(states):
    return ["%s/%s" % s for s in states]


@pytest.mark.parametrize("name,which", STATES, ids=_ids(STATES))
def test_specification_is_the_serial_oracle_on_appended_unassigned_rows(name, which):
    case, spec, Xq, got, _ = state(name, which)
    labels, K = spec.canonical()
    am = fp.appended_model(case, Xq, labels)
    N = len(labels)
    assert am.components.K == K == got.K
    worst = {"density": 0.0, "resp": 0.0}
    step = 1 if which == "initial" and case[0] != "full" else 5       # (every query on the cheap models, every fifth elsewhere)
    for r in range(0, len(Xq), step):
        k, dens, resp = fp.serial_witness(am, N + r)
        assert k == got.label[r], (name, which, r)
        worst["density"] = max(worst["density"], rel(got.density[r], dens))
        worst["resp"] = max(worst["resp"], rel(got.resp[r], resp))
    print("%s %s: density %.3g, responsibilities %.3g against the serial oracle" % (name, which, worst["density"], worst["resp"]))
    assert worst["density"] <= TOL and worst["resp"] <= TOL
    assert np.array_equal(am.components.assignments[N:], np.full(len(Xq), -1))         # (the witness grew nothing)


@pytest.mark.parametrize("name,which", STATES, ids=_ids(STATES))
def test_label_decisions_keep_the_margin(name, which):
    case, spec, Xq, got, census = state(name, which)
    n_new = int(np.count_nonzero(got.label == got.K))
    chosen = len(set(got.label.tolist()))
    print("%s %s: %d decisions, least gap %.3g relative, %d empty ties; %d of %d queries to an empty slot, %d labels chosen, K %d"
          % (name, which, census.decisions, census.gap_rel, census.empty_ties, n_new, len(Xq), chosen, got.K))
    assert census.decisions == len(Xq) == fp.M_QUERY
    assert census.gap_rel >= fp.MARGIN
    assert census.tie_on_occupied == 0 and census.softmax_disagrees == 0
    if case[3] > 1:
        # (a label K needs an empty slot: after its sweeps fc_D64_K7_un_T10 holds all seven, and its initial state sends
        # queries to an empty slot)
        assert n_new >= 1 or (got.K == case[3] and which == "swept")
        assert chosen >= 2 and np.count_nonzero(got.label < got.K) >= 1
    else:
        assert set(got.label.tolist()) <= {0}


def test_renumbering_is_canonicals_on_slots_that_are_not_canonical():
    seen = 0
    for name in SWEPT:
        case, spec, Xq, got, _ = state(name, "swept")
        labels, K = spec.canonical()
        held = spec.slot >= 0
        table = np.full(spec.K_max, -1, np.int64)
        table[spec.slot[held]] = labels[held]               # canonical's label of every occupied slot
        occupied = np.flatnonzero(got.cnt > 0)
        if not np.array_equal(occupied, np.arange(K)):
            seen += 1
        for r in range(len(Xq)):
            k = got.slot[r]
            assert got.label[r] == (table[k] if got.cnt[k] > 0 else K), (name, r)
        assert np.array_equal(got.order[:K], occupied) and np.array_equal(table[got.order[:K]], np.arange(K)), name
        assert np.all(got.cnt[got.order[K:]] == 0)
    print("%d of %d swept states hold slots that are not canonical" % (seen, len(SWEPT)))
    assert seen >= len(SWEPT) // 2


def test_lms_separates_the_prior_terms_of_density_and_label():
    """LMS = 0.9: the density's and the responsibilities' prior term carries lms, the label's does not -- on the same
    likelihoods, lms = 1 gives other densities and the same labels"""
    assert fi.LMS != 1.0
    case, spec, Xq, got, _ = state("dg_D39_K65_n257", "swept")
    one = fp.functions_of(got.ll, got.cnt, spec.alpha, 1.0)
    assert np.array_equal(one.label, got.label)
    assert np.min(np.abs(one.density - got.density)) > 1e-6
    assert rel(one.resp, got.resp) > 1e-6
    # the density is not the label's logits summed: it carries lms and the normaliser log(N_a + alpha)
    pz = np.log(spec.alpha / spec.K_max + got.cnt)
    r = 0
    naive = np.log(np.sum(np.exp(pz + got.ll[r] - np.max(pz + got.ll[r])))) + np.max(pz + got.ll[r])
    assert abs(naive - got.density[r]) > 1e-6


F32_CASES = [n for n in f32.CASES if n not in ("dg_D39_K1100", "dg_D39_K300_8x8")]


@pytest.mark.parametrize("name", F32_CASES)
def test_float32_emulation_of_the_query_likelihoods(name):
    case = f32.CASES[name]
    spec = f32.spec_of(case)
    Xq = fp.query_rows(case)
    d = spec.derive(*spec.stats_excluding(-1))

    class QueryView(object):                                # what f32.emulate asks of a specification, with the queries as rows
        X, K_max, D, log_prior_pred = Xq, spec.K_max, spec.D, staticmethod(spec.log_prior_pred)
    rows = list(range(len(Xq)))
    got = f32.emulate(QueryView, d, rows, f32.centre_of(spec.X))
    want = np.array([spec.loglik(d, x) for x in Xq])
    worst = f32.rel(got, want)
    print("%s: float32 emulation of %d query rows, worst %.3g" % (name, len(Xq), worst))
    assert worst <= f32.EMULATION
    assert np.array_equal(got[:, ~d["active"]], want[:, ~d["active"]])


def test_byte_counts_are_the_kernels():
    src = open(os.path.join(ROOT, "segmentalist_amd", "csrc", "segk_fbitems.hip")).read()

    def define(name):
        return re.search(r"#define\s+%s\s+(.+?)\s*(?://.*)?$" % name, src, flags=re.M).group(1)
    assert int(define("FBI_T")) == fp.TILE == 64
    assert define("FBI_KW") == "2" and define("FBI_NT") == "512" and fp.KC == 2 * (512 // 64)
    assert define("FBI_LDS_MAX") == "(144 * 1024)" and fp.LDS_MAX == 144 * 1024
    assert "return (size_t)FBI_T * D + 2 * (size_t)FBI_KC * D;" in src
    assert "return (((size_t)KM + 1) * sizeof(int32_t) + 7) & ~(size_t)7;" in src
    assert ("return (fullcov ? 0 : fbi_stage_doubles(D) * sizeof(double)) + (size_t)KM * sizeof(double) + "
            "fbi_predict_rank_bytes(KM);") in src
    assert "return fbi32_stage_bytes(D) + (size_t)KM * sizeof(double) + fbi_predict_rank_bytes(KM);" in src
    assert "(size_t)FBI_T * KM * sizeof(double)" in src and "(size_t)FBI_T * fbi32_ldl(KM) * sizeof(double)" in src
    # the K_max values on either side of the rule, as DESIGN.md 4.22 states them
    assert fp.k_max_either_side(39) == (224, 225) and fp.k_max_either_side(100) == (134, 135)
    assert fp.lds_bytes(39, 224) <= fp.LDS_MAX < fp.lds_bytes(39, 225)
    lo, hi = fp.k_max_either_side(39, fp.lds_bytes_f32)
    assert fp.lds_bytes_f32(39, lo) <= fp.LDS_MAX < fp.lds_bytes_f32(39, hi) and hi == lo + 1


def test_abi_15_and_the_two_entry_points():
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("segk_fbi_predict", "segk_fbi_predict_diag32"):
        assert hasattr(lib, sym) and sym in _abi.SIGNATURES, sym
        assert re.search(r"\b%s\s*\(" % sym, code), sym
        assert len(_abi.SIGNATURES[sym][1]) == 15
    assert "fbgmm.py:256-285" in hdr and "fbgmm.py:436-451" in hdr and "fbgmm.py:475-488" in hdr


def test_golden_vectors_of_the_reference():
    """tests/golden/predict.npz (tests/golden/make_golden_predict.py, recorded from the reference's own FBGMM over [X; Xq]
    with the queries at -1): log_marg_i, the log_prob_z vector of fbgmm.py:436-445 and map_assign_i's k of every query"""
    g = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in g.files})
    assert len(names) >= 3
    for name in names:
        case = fi.CASES[name]
        spec = fi.spec_of(case)[1]
        Xq = fp.query_rows(case, M=int(g[name + "/M"]))
        assert np.array_equal(Xq, g[name + "/Xq"]), name
        got = fp.predict(spec, Xq)
        assert np.array_equal(got.label, g[name + "/k"]), name
        d, z = rel(got.density, g[name + "/log_marg_i"]), g[name + "/log_prob_z"]
        # the recorded vector is unnormalised: normalise it as fbgmm.py:450-451 does
        zn = z - (np.log(np.sum(np.exp(z - z.max(axis=1, keepdims=True)), axis=1)) + z.max(axis=1))[:, None]
        r = rel(got.resp, zn)
        print("%s: density %.3g, responsibilities %.3g against the reference's recorded values" % (name, d, r))
        assert d <= TOL and r <= TOL

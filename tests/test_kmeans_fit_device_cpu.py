"""
CPU tests of the specification of KMeans.fit on the device (tests/kmeans_fit_device.py): the decomposition the
kernels implement -- move list, clamp replay, ordered operation lists per component, apply, clean -- must leave what the
reference's item-by-item fit (oracle/np_oracle.py KMeans.fit) leaves, after every iteration of every case: equal, not close
(sum_neg_sqrd_norm alone keeps the project's rtol=1e-10).  The case list must contain the situations that can break the kernels.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as no
from tests import kmeans_fit_device as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_infos = {}


def run_spec(case, dtype, consider_unassigned=True):
    """The specification against the oracle's trace, iteration by iteration -> the per-iteration info dicts (cached)."""
    key = (case[0], dtype, consider_unassigned)
    if key in _infos:
        return _infos[key]
    trace = kf.oracle_trace(case, dtype, consider_unassigned)
    spec = kf.new_model(no.KMeans, case, dtype).components
    infos = []
    for it, want in enumerate(trace):
        info = {}
        moved, K, obj = kf.fit_step(spec, consider_unassigned, info)
        got = kf.snapshot(spec)
        for f in kf.FIELDS:
            assert np.array_equal(got[f], want[f]), (case[0], dtype, it, f)
        assert got["means"].dtype == want["means"].dtype
        assert moved == want["n_mean_updates"] and K == want["components"], (case[0], it)
        assert np.isclose(obj, want["sum_neg_sqrd_norm"], rtol=1e-10)
        infos.append(info)
    _infos[key] = infos
    return infos


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", kf.CASES, ids=kf.CASE_IDS)
def test_decomposition_equals_the_reference_fit(case, dtype):
    infos = run_spec(case, dtype)
    assert len(infos) >= 1


@pytest.mark.parametrize("flag", [True, False])
def test_unassigned_rows_both_ways(flag):
    case = kf.CASES[kf.CASE_IDS.index("holes")]
    X, a = kf.case_data(case, "float32")
    assert (a == -1).sum() > 50
    infos = run_spec(case, "float32", flag)
    trace = kf.oracle_trace(case, "float32", flag)
    if flag:
        assert (trace[0]["assignments"] != -1).all()           # every row got a label in the first iteration
        assert infos[0]["n_items"] == case[1]
    else:
        assert ((trace[-1]["assignments"] == -1) == (a == -1)).all()      # the unassigned rows stay out
        assert all(i["n_items"] == (a != -1).sum() for i in infos)


def all_infos():
    out = []
    for case in kf.CASES:
        for dtype in ("float32", "float64"):
            out += [(case[0], dtype, it, i) for it, i in enumerate(run_spec(case, dtype))]
    case = kf.CASES[kf.CASE_IDS.index("holes")]
    out += [(case[0], "float32-assigned", it, i) for it, i in enumerate(run_spec(case, "float32", False))]
    return out


def test_case_list_contains_what_can_break_the_kernels():
    infos = all_infos()
    # at least three foundings in one iteration, one of them a true clamp (k_requested > K at that moment)
    assert any(i["founded"] >= 3 and i["clamped"] >= 1 for _, _, _, i in infos)
    # a component reaches count 0 and is refilled later in the same iteration
    assert any(i["refilled"] >= 1 for _, _, _, i in infos)
    # an iteration ends with at least two empty components, one of them not the last active one
    assert any(i["n_empty"] >= 2 and i["empty_inside"] for _, _, _, i in infos)
    # an iteration without a move
    assert any(i["moved"] == 0 for _, _, _, i in infos)
    # more moves naming a row >= K than one round of the clamp replay holds, and a founding that is not the first of its round
    assert any(i["n_hi"] > kf.WAVE for _, _, _, i in infos)
    # more operations than one chunk of the counting sort, with K_max beyond one workgroup's threads
    assert any(2 * i["moved"] > kf.OPS_CHUNK for n, _, _, i in infos if n == "big_bank")
    # the per-case figures the issue names
    by = {(n, d, it): i for n, d, it, i in infos}
    assert by[("one_start", "float32", 0)]["founded"] >= 3 and by[("one_start", "float32", 0)]["clamped"] >= 1
    assert max(i["n_empty"] for (n, d, it), i in by.items() if n == "empties") >= 10
    assert max(i["founded"] for (n, d, it), i in by.items() if n == "big_bank") >= 100
    assert max(i["n_empty"] for (n, d, it), i in by.items() if n == "big_bank") >= 100


def test_argmax_ties_exist_in_the_ties_case():
    case = kf.CASES[kf.CASE_IDS.index("ties")]
    m = kf.new_model(no.KMeans, case, "float32")
    c = m.components
    tied = 0
    for i in range(c.N):
        s = c.neg_sqrd_norm(i)
        tied += int(np.count_nonzero(s == s.max()) > 1)
    assert tied > 0


def test_clamp_rounds_equal_the_serial_clamp():
    rs = np.random.RandomState(0)
    for trial in range(200):
        K_max = int(rs.randint(1, 40))
        K0 = int(rs.randint(0, K_max + 1))
        n = int(rs.randint(0, 400))
        if K0 == K_max:
            n = 0
        req = rs.randint(K0, K_max, size=n) if n else np.zeros(0, np.int64)
        fin, K, _, _ = kf.clamp_serial(req, K0, K_max)
        fin2, K2 = kf.clamp_rounds(req, K0, K_max)
        assert K == K2 and np.array_equal(fin, fin2), trial


def test_ordered_lists_are_a_stable_sort():
    rs = np.random.RandomState(1)
    for n, K_max in ((0, 3), (1, 1), (300, 4), (700, 50), (1500, 700)):
        old = rs.randint(-1, K_max, size=n)
        fin = rs.randint(0, K_max, size=n)
        ops, off = kf.ordered_lists(old, fin, K_max)
        keys = np.empty(2 * n, np.int64)
        keys[0::2], keys[1::2] = old, fin
        want = np.argsort(keys, kind="stable")
        want = want[keys[want] >= 0]
        assert np.array_equal(ops, want)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(keys[keys >= 0], minlength=K_max))]))


def test_header_binding_and_makefile_list_the_entry_points():
    from segmentalist_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    for name in ("segk_kmeans_fit_scratch_words", "segk_kmeans_fit_step"):
        assert name in _abi.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr)
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15 == _abi.ABI_VERSION
    assert "segk_fit.hip" in open(os.path.join(ROOT, "segmentalist_amd", "csrc", "Makefile")).read()
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    lib.segk_kmeans_fit_scratch_words.restype = ctypes.c_int64
    lib.segk_kmeans_fit_scratch_words.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
    small, large = lib.segk_kmeans_fit_scratch_words(1000, 10, 8), lib.segk_kmeans_fit_scratch_words(1000, 1000, 8)
    assert 0 < small < large
    assert lib.segk_kmeans_fit_scratch_words(0, 1, 8) == 0
    # the operands are refused on the host before anything touches a device
    assert lib.segk_kmeans_fit_step(None, None, None, None, 1, 1, None, None, None, None) != 0


def test_fit_signature_keeps_the_defaults():
    import inspect
    from segmentalist_amd.kmeans import KMeans
    sig = inspect.signature(KMeans.fit)
    assert sig.parameters["on_device"].default is False
    assert list(sig.parameters)[:5] == ["self", "n_iter", "consider_unassigned", "no_empty", "on_device"]

"""
What the GPU tests of `SegmentalKMeansWordseg.decode` (tests/test_gpu_kmeans_decode.py) rest on, held with NumPy and the oracle
alone before the device is asked anything:

1. specification = serial witness (the oracle's classes over training plus held-out rows, the held-out rows at -1), bit for bit
   on every integer field and on seg_score; the objective equal as the chain tests hold segment_i's return value (==); the
   second witness, segment_i on a deep copy, gives the same flags and objective wherever it does not assert;
2. the recorded values of the reference itself (tests/golden/kmeans_decode.npz), the same way;
3. the census: which case carries what it is listed for;
4. the LDS byte count against the source, the symbol in header, binding and library at ABI 15; the Python surface exists.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import kmeans_decode as kd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kmeans_decode.npz")
PAIRS = [(n, m) for n in kd.CASES for m in kd.MODES]


@pytest.mark.parametrize("name,mode", PAIRS)
def test_specification_is_the_serial_witness(name, mode):
    dec, _ = kd.decoded(name, mode)
    w, totals2, bounds2 = kd.witness(name, mode, kd.OracleImpl())
    kd.assert_same(dec, w, (name, mode))
    u = dec.tables.u
    for i in range(u.D):
        N = u.lengths[i]
        assert np.array_equal(bounds2[i], dec.boundaries[i, :N]), (name, mode, i)
        no_emb = np.any(dec.seg_embed[dec.seg_offsets[i]:dec.seg_offsets[i + 1]] < 0)
        # segment_i asserts in add_item exactly where a chosen segment has no embedding (kmeans_components.py:100)
        assert np.isnan(totals2[i]) == bool(no_emb), (name, mode, i)
        if not no_emb:
            assert totals2[i] == dec.objective[i], (name, mode, i)


def test_golden_vectors_of_the_reference():
    g = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in g.files})
    assert names == sorted(["km_mid", "km_f64", "dead_end", "long92_w6"])
    assert kd.CASES["km_mid"][6] == "float32" and kd.CASES["km_f64"][6] == "float64"
    assert g["long92_w6/boundaries"].shape[1] == 92 and np.any(g["dead_end/seg_embed"] < 0)
    for name in names:
        dec, _ = kd.decoded(name, "serial")
        kd.assert_same(dec, {k.split("/")[1]: g[k] for k in g.files if k.startswith(name + "/")}, name)
        t2 = g[name + "/segment_i_objective"]
        ok = ~np.isnan(t2)
        assert np.array_equal(t2[ok], dec.objective[ok])


def test_census_every_case_exercises_what_it_is_listed_for():
    # a segment whose raw row is an inactive one (label K): the batch-fitted km_mid, e_km_short and long92_w6
    for name in ("km_mid", "e_km_short", "long92_w6"):
        dec, _ = kd.decoded(name, "batch")
        hit = dec.seg_row >= dec.K
        assert hit.any() and np.all(dec.seg_label[hit] == dec.K) and dec.K < kd.CASES[name][2]
    # stepping back from a dead end, down to t == 0, and segments without an embedding: dead_end, both fits
    for mode in kd.MODES:
        dec, c = kd.decoded("dead_end", mode)
        assert c.dead_end_starts >= 1 and c.hit_zero >= 1 and c.dead_windows >= 1
        no_emb = dec.seg_embed < 0
        assert no_emb.any() and not no_emb.all()
        assert np.all(dec.seg_row[no_emb] == -1) and np.all(dec.seg_label[no_emb] == -1) and np.all(dec.seg_score[no_emb] == -np.inf)
    # NaN durations inside the window without a dead end at the start: e_km_mindur
    dec, c = kd.decoded("e_km_mindur", "serial")
    assert c.dead_windows >= 1 and c.dead_end_starts == 0
    # more than 64 landmarks beside utterances shorter than the window: the generic walk over band and triangle
    dec, _ = kd.decoded("long92_w6", "serial")
    assert dec.tables.u.N_max == 92 and min(dec.tables.u.lengths) < kd.decode_window("long92_w6") == 6
    assert max(kd.fitted("long92_w6", "serial").utterances.lengths) <= 9
    # the wide window, and spans longer than 8 chosen under it or not, utterances longer than it
    dec, _ = kd.decoded("w12", "serial")
    assert kd.decode_window("w12") == 12 and max(dec.tables.u.lengths) > 12
    # no window
    assert kd.decode_window("w0") == 0 and kd.seg_kwargs("w0")["wip"] != 0
    # a one-landmark utterance
    dec, _ = kd.decoded("e_km_short", "serial")
    assert min(dec.tables.u.lengths) == 1
    # float64 data
    assert kd.decoded("km_f64", "serial")[0].score.dtype == np.float64 == kd.decoded("refit_K30_f64", "batch")[0].score.dtype
    for name, mode in PAIRS:
        dec, _ = kd.decoded(name, mode)
        u = dec.tables.u
        assert u.D == kd.HELD and kd.lds_bytes(u.N_max, kd.decode_window(name)) <= kd.LDS_MAX
        for i in range(u.D):                          # segment j of utterance i ends behind its j-th set flag
            ends = np.flatnonzero(dec.boundaries[i]) + 1
            lo, hi = dec.seg_offsets[i], dec.seg_offsets[i + 1]
            assert np.array_equal(dec.seg_end[lo:hi], ends) and ends[-1] == u.lengths[i]
            assert np.array_equal(dec.seg_start[lo:hi], np.concatenate([[0], ends[:-1]]))


def test_lds_bytes_are_the_kernels():
    from segmentalist_amd.device import DeviceKMeans
    src = open(os.path.join(ROOT, "segmentalist_amd", "csrc", "segk_kmdecode.hip")).read()
    assert "#define KMD_LDS_MAX (160 * 1024)" in src and kd.LDS_MAX == 160 * 1024
    assert "const int64_t cells = NM * Wc;" in src
    assert ("fast ? (size_t)(9 * NM + 12) * sizeof(double) + (size_t)(2 * cells + 2 * NM + 8) * sizeof(int32_t)") in src
    assert ": (size_t)(cells + NM + 1) * sizeof(double) + (size_t)cells * sizeof(int32_t) + (size_t)NM;" in src
    assert "return (b + 15) & ~(size_t)15;" in src
    for NM, W in ((92, 6), (9, 6), (64, 8), (64, 0), (65, 8), (20, 12), (1, 4), (200, 0)):
        assert kd.lds_bytes(NM, W) == DeviceKMeans.decode_lds_bytes(NM, W)
    assert kd.lds_bytes(92, 6) == (8 * (552 + 93) + 4 * 552 + 92 + 15) // 16 * 16
    assert kd.lds_bytes(200, 0) > kd.LDS_MAX >= kd.lds_bytes(100, 0)
    assert not re.search(r"atomic(Add|Or|CAS|Max|Min|Exch)|__syncthreads|cooperative", src)      # a plain grid, one wave each


def test_abi_15_entry_point_and_python_surface():
    from segmentalist_amd import _abi, kmeans, kmeans_acoustic_wordseg as kaw
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert hasattr(lib, "segk_kmd_decode") and "segk_kmd_decode" in _abi.SIGNATURES
    assert re.search(r"\bsegk_kmd_decode\s*\(", code)
    assert len(_abi.SIGNATURES["segk_kmd_decode"][1]) == 15
    assert "kmeans_acoustic_wordseg.py:225-332" in hdr and ":449-555" in hdr and "kmeans_components.py:103-106" in hdr
    assert "segk_kmdecode.hip" in open(os.path.join(ROOT, "segmentalist_amd", "csrc", "Makefile")).read()
    assert callable(kaw.SegmentalKMeansWordseg.decode) and callable(kmeans.KMeans.predict)
    assert set(kd.Dec.FIELDS) == set(kaw.KMeansDecoded._fields)

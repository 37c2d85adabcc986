"""
What the GPU tests of `UnigramAcousticWordseg.decode` (tests/test_gpu_wordseg_decode.py) rest on, held with NumPy and the oracle
alone before the device is asked anything:

1. the census of decisions of the specification tests/wordseg_decode.py: on every case every DP step and the label of every
   chosen segment at least MARGIN = 1e-6 (relative) clear of its best competitor -- three orders above the 1e-9 the device's
   fp64 log-probabilities are held to; a condition on the inputs --, no tie that involves an occupied slot, the reference's
   softmax form agreeing with the argmax; and every case exercises what it is listed for;
2. the serial witness: the specification equals the oracle's segmenter classes over training plus held-out utterances with the
   held-out tokens deleted -- get_vec_embed_log_probs, forward_backward_viterbi, map_assign_i on a deep copy per segment --,
   log-probabilities at 1e-12, boundaries and labels equal;
3. the recorded values of the reference itself (tests/golden/decode.npz, tests/golden/make_golden_decode.py) at 1e-12;
4. the LDS byte count against the source, the symbol in header, binding and library at ABI 15.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import wordseg_decode as wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
ALL = wd.CASES + wd.FULL
GOLDEN = os.path.join(ROOT, "tests", "golden", "decode.npz")
# what a case is in the list for: (held-out N_max over 64: the band, the least window, segments labelled K at least,
# distinct occupied labels at least)
BAND = {"ragged_fixed": 138, "ragged_diag": 138, "diag_100_w20": 100, "fixed_100_w40": 100, "diag_mindur_backtrack": None,
        "diag_K65_x_ragged": 92, "fixed_small_x_ragged": 92, "w6_long": None}
LABELLED_K = {"diag_K65": 3, "diag_K65_x_ragged": 1, "fixed_small_x_ragged": 1, "fixed_K300": 1, "diag_K130": 1}
ONLY_K = ["fixed_K1025"]


@pytest.mark.parametrize("name", ALL)
def test_every_decision_keeps_the_margin(name):
    dec, c = wd.decoded(name)
    u = dec.tables.u
    print("%s: N_max %d, %d rows, K %d, %d segments (%d labelled K, %d without an embedding); %d DP steps, least gap %.3g; "
          "least label gap %.3g; %d dead windows, %d dead-end starts"
          % (name, u.N_max, len(dec.tables.Xq), dec.K, len(dec.seg_label), int(np.count_nonzero(dec.seg_label == dec.K)),
             int(np.count_nonzero(dec.seg_embed < 0)), c.dp_steps, c.dp_margin, c.slot_margin, c.dead_windows, c.dead_end_starts))
    assert c.decodes == u.D == wd.HELD
    assert c.dp_margin >= wd.MARGIN and c.slot_margin >= wd.MARGIN
    assert c.tie_on_occupied == 0 and c.softmax_disagrees == 0
    assert c.tokens == int(np.count_nonzero(dec.seg_embed >= 0))


@pytest.mark.parametrize("name", ALL)
def test_every_case_exercises_what_it_is_listed_for(name):
    dec, c = wd.decoded(name)
    u = dec.tables.u
    n_max = wd.swept(name)[1].seg.n_slices_max
    if name in BAND:
        assert u.N_max > 64 and 1 <= n_max <= 64
        assert BAND[name] is None or u.N_max == BAND[name]
        assert wd.lds_bytes(u.N_max, n_max) <= wd.BAND_LDS_MAX
    else:
        assert u.N_max <= 64
    if name == "diag_65":
        # a triangular held-out corpus on a model trained on a band corpus
        assert u.N_max == 54 and max(wd.swept(name)[0].utterances.lengths) == 65
    if name in wd.CROSS:
        assert max(wd.swept(name)[0].utterances.lengths) <= 64
    if name in ("fixed_w20", "diag_w20", "diag_100_w20"):
        assert n_max > 16 and max(u.lengths) > 16
    if name in ("fixed_100_w40",):
        assert n_max > 32
    if name == "fixed_64_w30":
        assert u.N_max == 64
    if name == "diag_mindur_backtrack":
        assert c.dead_windows == 109 and c.dead_end_starts == 1
        no_emb = np.flatnonzero(dec.seg_embed < 0)
        assert len(no_emb) == 1
        assert dec.seg_label[no_emb[0]] == -1 and dec.seg_log_marg[no_emb[0]] == -np.inf
    else:
        assert c.dead_end_starts == 0 and np.all(dec.seg_embed >= 0)
    occupied = dec.seg_label[(dec.seg_label >= 0) & (dec.seg_label < dec.K)]
    n_K = int(np.count_nonzero(dec.seg_label == dec.K))
    if name in ONLY_K:
        assert n_K == len(dec.seg_label) > 0
    else:
        assert len(set(occupied.tolist())) >= 2
        assert n_K >= LABELLED_K.get(name, 0)
    # segments and boundaries are aligned: segment j of utterance i ends behind its j-th set flag
    for i in range(u.D):
        ends = np.flatnonzero(dec.boundaries[i]) + 1
        lo, hi = dec.seg_offsets[i], dec.seg_offsets[i + 1]
        assert np.array_equal(dec.seg_end[lo:hi], ends)
        assert np.array_equal(dec.seg_start[lo:hi], np.concatenate([[0], ends[:-1]]))
        assert ends[-1] == u.lengths[i]


@pytest.mark.parametrize("name", ALL)
def test_specification_is_the_serial_oracle_with_the_held_out_tokens_deleted(name):
    dec, _ = wd.decoded(name)
    worst = wd.assert_equals_witness(dec, wd.witness(name, wd.OracleImpl()), TOL)
    print("%s: log-probabilities and densities %.3g against the serial witness" % (name, worst))


def test_golden_vectors_of_the_reference():
    g = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in g.files})
    assert len(names) == 4 and any(n in wd.FULL for n in names) and any(g[n + "/boundaries"].shape[1] > 64 for n in names)
    kinds = {wd.model_case(n)["kind"] for n in names if n not in wd.FULL}
    assert kinds == {"fixed", "diag"}
    for name in names:
        dec, _ = wd.decoded(name)
        worst = wd.assert_equals_witness(dec, {k.split("/")[1]: g[k] for k in g.files if k.startswith(name + "/")}, TOL)
        print("%s: %.3g against the reference's recorded values" % (name, worst))


def test_lds_bytes_are_the_kernels():
    src = open(os.path.join(ROOT, "segmentalist_amd", "csrc", "segk_fbdecode.hip")).read()
    assert "#define FBD_BAND_LDS_MAX (160 * 1024)" in src and wd.BAND_LDS_MAX == 160 * 1024
    assert "const int64_t cells = band ? NM * W : NM * (NM + 1) / 2;" in src
    assert ("return (size_t)(cells + 3 * NM + 2) * sizeof(double) + (size_t)cells * sizeof(int32_t) + (size_t)((NM + 15) & ~15);"
            in src)
    # k_fbb_segment's bytes without the old token list [N_max] int32
    batch = open(os.path.join(ROOT, "segmentalist_amd", "csrc", "segk_fbbatch.hip")).read()
    assert ("return (size_t)(cells + 3 * NM + 2) * sizeof(double) + (size_t)(NM + cells) * sizeof(int32_t) + "
            "(size_t)((NM + 15) & ~15);") in batch
    for NM, W in ((138, 6), (100, 40), (194, 6), (65, 64)):
        assert wd.lds_bytes(NM, W) == 12 * NM * W + 24 * NM + 16 + (NM + 15) // 16 * 16
    assert wd.lds_bytes(64) == 8 * (2080 + 194) + 4 * 2080 + 64
    assert "__launch_bounds__(128)" in src
    assert not re.search(r"atomic(Add|Or|CAS|Max|Min|Exch)|__syncthreads_count|cooperative", src)      # a plain grid


def test_abi_15_and_the_entry_point():
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert lib.segk_abi_version() == 15 == _abi.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert hasattr(lib, "segk_fbd_decode") and "segk_fbd_decode" in _abi.SIGNATURES
    assert re.search(r"\bsegk_fbd_decode\s*\(", code)
    assert len(_abi.SIGNATURES["segk_fbd_decode"][1]) == 15
    assert "unigram_acoustic_wordseg.py:474-511" in hdr and ":759-864" in hdr and "fbgmm.py:475-490" in hdr
    mk = open(os.path.join(ROOT, "segmentalist_amd", "csrc", "Makefile")).read()
    assert "segk_fbdecode.hip" in mk

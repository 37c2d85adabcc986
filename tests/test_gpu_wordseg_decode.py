"""GPU parity of `UnigramAcousticWordseg.decode` (segk_fbd_decode behind segk_fbi_predict) against its executable
specification tests/wordseg_decode.py.  tests/test_wordseg_decode_cpu.py is the precondition of the exact tests here: on every
case every DP step and every label is decided by at least 1e-6 relative, so boundaries, segment rows and labels must coincide;
log-probabilities and log densities to 1e-9 relative, -inf matched exactly.

In the tolerance mode (score_precision "f32", diagonal components) the densities may leave the specification's within the
project's 1e-4 contract, so the decisions are checked against the device's own numbers: the path total of the device's
boundaries reaches the host optimum for the device's span scores, and every label is the argmax of the device's own logits."""
import random

import numpy as np
import pytest

from oracle import np_oracle as no
from tests import map_batch as mbm
from tests import wordseg_decode as wd

pytestmark = pytest.mark.gpu
RTOL = 1e-9
FIELDS = ("boundaries", "log_prob", "seg_offsets", "seg_start", "seg_end", "seg_embed", "seg_label", "seg_log_marg")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def assert_matches(res, dec, what):
    """a product result against the specification's"""
    assert res.utterance_labels == dec.utterance_labels, what
    assert res.K == dec.K, what
    assert res.boundaries.dtype == bool and np.array_equal(res.boundaries, dec.boundaries), what
    for k in ("seg_offsets", "seg_start", "seg_end", "seg_embed", "seg_label"):
        assert np.array_equal(getattr(res, k), getattr(dec, k)), (what, k)
    worst = max(wd.rel(res.log_prob, dec.log_prob), wd.rel(res.seg_log_marg, dec.seg_log_marg))
    assert worst <= RTOL, (what, worst)
    for i in range(len(dec.utterance_labels)):
        assert res.transcript(i) == dec.transcript(i), (what, i)
    return worst


def same_bits(a, b):
    assert a.utterance_labels == b.utterance_labels and a.K == b.K
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("name", wd.CASES + wd.FULL)
def test_decode_matches_specification(gpu, name):
    dec, _ = wd.decoded(name)
    seg = wd.product_swept(name)
    assert seg._get_sweeper().in_batch_state
    res = seg.decode(*wd.heldout_inputs(name))
    worst = assert_matches(res, dec, name)
    print("%s: %d segments, log-probabilities and densities %.3g against the specification" % (name, len(res.seg_label), worst))


STATE_ENTRY = ["fixed_small", "ragged_diag", "diag_mindur_backtrack", "w0_K8"]


def _both_entries(name):
    """(decode on the live batch state, decode on a serial state: after materialise(), the batch state dropped)"""
    seg = wd.product_swept(name)
    held = wd.heldout_inputs(name)
    live = seg.decode(*held)
    seg.materialise()
    seg._leave_batch()
    sw = seg._get_sweeper()
    assert not sw.in_batch_state
    serial = seg.decode(*held)
    assert not sw.in_batch_state                              # entered, and dropped again
    return live, serial


@pytest.mark.parametrize("name", STATE_ENTRY)
def test_serial_state_matches_specification(gpu, name):
    live, serial = _both_entries(name)
    assert_matches(serial, wd.decoded(name)[0], name)
    for k in ("boundaries", "seg_offsets", "seg_start", "seg_end", "seg_embed", "seg_label"):
        assert np.array_equal(getattr(live, k), getattr(serial, k)), k
    assert live.K == serial.K


@pytest.mark.parametrize("name", STATE_ENTRY)
def test_serial_state_gives_the_bits_of_the_batch_state(gpu, name):
    """Every field, the log-probabilities and log densities included, bit for bit.  A row's density is segk_fbi_predict's
    logsumexp over the slots IN SLOT ORDER, and the two states number the slots differently (the live batch state keeps the
    slots its sweeps left -- fixed_small: 1 2 3 4 5 6 8 9 --, materialise() hands the serial state the canonical labels
    0 .. K - 1): decode on a live batch state therefore scores on a copy of the slot tables in the canonical order
    (FbgmmBatchSweeper._canonical_tables).  Without it 1 of 14 to 19 of 141 densities differed by one unit in the last place."""
    live, serial = _both_entries(name)
    for k in ("log_prob", "seg_log_marg"):
        a, b = getattr(live, k), getattr(serial, k)
        fin = np.isfinite(a) & np.isfinite(b)
        print("%s %s: %d of %d entries differ, worst %.3g relative" % (name, k, int(np.count_nonzero(a != b)), a.size,
                                                                       float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))))))
    same_bits(live, serial)


def _held(name, n):
    """the first n held-out utterances of a case"""
    h = wd.heldout_inputs(name)
    keys = sorted(h[0])[:n]
    return tuple({k: d[k] for k in keys} for d in h)


def test_held_out_sets_of_zero_one_and_two_utterances(gpu):
    name = "diag_K65"
    dec, _ = wd.decoded(name)
    seg = wd.product_swept(name)
    spec = wd.swept(name)[1]
    empty = seg.decode({}, {}, {}, {})
    assert empty.utterance_labels == [] and empty.boundaries.shape == (0, 0) and len(empty.log_prob) == 0
    assert np.array_equal(empty.seg_offsets, [0]) and len(empty.seg_label) == 0 and empty.K == dec.K
    for n in (1, 2):
        h = _held(name, n)
        assert_matches(seg.decode(*h), wd.decode(spec, h), n)


def test_an_utterance_of_one_landmark_and_a_row_count_that_is_no_multiple_of_64(gpu):
    from segmentalist_amd.synth import span_table
    name = "fixed_small"
    seg = wd.product_swept(name)
    spec = wd.swept(name)[1]
    h = tuple(dict(d) for d in _held(name, wd.HELD))
    # one landmark: a single span, its one embedding a copy of a held-out row
    src = sorted(h[0])[0]
    h[0]["one"] = h[0][src][:1].copy()
    h[1]["one"] = span_table(1, seg.n_slices_max)[0]
    h[2]["one"] = np.array([7])
    h[3]["one"] = [7]
    M = sum(len(m) for m in h[0].values())
    assert M % 64 != 0 and M > 64
    want = wd.decode(spec, h)
    res = seg.decode(*h)
    assert_matches(res, want, "one landmark")
    i = res.utterance_labels.index("one")
    assert res.seg_offsets[i + 1] - res.seg_offsets[i] == 1 and res.boundaries[i, 0] and not res.boundaries[i, 1:].any()


def snapshot(seg):
    df, sw = seg._df, seg._get_sweeper()
    dev = {nm: getattr(df, nm).clone() for nm in ("assignments", "K", "counts", "stat_a", "stat_b", "log_prod", "pred", "kconst")}
    dev.update(slot=sw.slot.clone(), partials=sw.partials.clone(), bounds=seg._dev_bounds.clone())
    return dev, (sw.sweep_index, sw.in_batch_state, random.getstate(), np.random.get_state()[1].tobytes(), np.random.get_state()[2])


def same(gpu, a, b, names=None):
    for nm in names or a[0]:
        assert gpu.equal(a[0][nm], b[0][nm]), nm
    assert a[1] == b[1]


@pytest.mark.parametrize("name", ["diag_K65", "ragged_fixed", "w0_K8"])
def test_read_only(gpu, name):
    held = wd.heldout_inputs(name)
    seg, twin = wd.product_swept(name), wd.product_swept(name)
    # batch state: nothing moves, two calls and device_out give the same bits
    before = snapshot(seg)
    first = seg.decode(*held)
    again = seg.decode(*held)
    on_dev = seg.decode(*held, device_out=True)
    assert all(isinstance(getattr(on_dev, k), gpu.Tensor) and getattr(on_dev, k).is_cuda for k in FIELDS + ("K",))
    gpu.cuda.synchronize()
    same(gpu, before, snapshot(seg))
    same_bits(first, again)
    same_bits(first, on_dev.numpy())
    assert on_dev.transcript(0) == first.transcript(0)
    # the next sweep is the sweep of a twin that never decoded
    for s in (seg, twin):
        s.batch_sweep_async()
    gpu.cuda.synchronize()
    a, b = seg._get_sweeper(), twin._get_sweeper()
    assert gpu.equal(a.slot, b.slot) and gpu.equal(a.partials, b.partials) and a.sweep_index == b.sweep_index
    assert gpu.equal(seg._dev_bounds, twin._dev_bounds) and gpu.equal(seg._df.out_logprob, twin._df.out_logprob)
    # serial state: assignments, K, counts, the serial statistics and the boundaries stay (the sweeper's own tables are rebuilt by
    # whoever enters next), and the next serial sweep is the twin's
    for s in (seg, twin):
        s.materialise()
        s._leave_batch()
    before = snapshot(seg)
    seg.decode(*held)
    gpu.cuda.synchronize()
    same(gpu, before, snapshot(seg), ("assignments", "K", "counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "bounds"))
    assert before[1] == snapshot(seg)[1]
    for s in (seg, twin):
        random.seed(9)
        s.gibbs_sample(1, sync="sequential")
    assert np.array_equal(seg.utterances.boundaries, twin.utterances.boundaries)
    assert np.array_equal(seg.acoustic_model.components.assignments, twin.acoustic_model.components.assignments)


@pytest.mark.parametrize("name", ["ragged_diag", "diag_K65"])
def test_float32_scores_decide_optimally_on_their_own_numbers(gpu, name):
    """score_precision="f32" with diagonal components: the densities within 1e-4 of the fp64 specification's on the same state,
    the boundaries optimal for the device's span scores at 1e-9, every label the argmax of the device's own logits"""
    from segmentalist_amd.device import DeviceCorpus
    seg = wd.product_swept(name, prec="f32")
    sw = seg._get_sweeper()
    assert sw.score_diag32
    held = wd.heldout_inputs(name)
    res = seg.decode(*held)
    tables = wd.Tables(held, seg.n_slices_min, seg.n_slices_max, wd.min_duration_of(name))
    u, Xq = tables.u, tables.Xq
    # the device's own numbers for every candidate row: the call decode makes, with the likelihood probe
    cq = DeviceCorpus(Xq.astype(seg._corpus.x_np_dtype), u.vec_ids, u.durations, u.lengths)
    K = sw.df.K_max
    probe = gpu.zeros((len(Xq), K), dtype=gpu.float64, device="cuda")
    from segmentalist_amd import _abi
    import ctypes as C
    cv = _abi.Corpus.from_buffer_copy(sw.df.corpus.c)
    cv.vec_ids = cv.durations = cv.band_ids = cv.band_dur = None
    L, ctx, cp, fp, bp, st = sw._args()
    _abi.check(L.segk_fbb_prepare(ctx, cp, fp, bp, -1, st))
    bp, (bt_canon, tables) = sw._canonical_tables()             # the slot order decode scores in (the reference view's)
    label = gpu.zeros(len(Xq), dtype=gpu.int32, device="cuda")
    dens = gpu.zeros(len(Xq), dtype=gpu.float64, device="cuda")
    prior_q = gpu.zeros(len(Xq), dtype=gpu.float64, device="cuda")
    _abi.check(L.segk_fbi_predict_diag32(ctx, C.byref(cv), fp, bp, _abi.ptr(cq.X), cq.ldx, len(Xq), _abi.ptr(prior_q), _abi.ptr(label),
                                         _abi.ptr(dens), None, 0, _abi.ptr(probe), K, st))
    gpu.cuda.synchronize()
    ll, dens, label, cnt = probe.cpu().numpy(), dens.cpu().numpy(), label.cpu().numpy(), tables["cnt"].cpu().numpy()
    # 1. the densities against the fp64 definition on the DEVICE's state (its counts and fp64 tables are the specification's
    #    only while the chain has not left it: the likelihoods are compared through the definition on the device's own ll)
    from tests import fbgmm_predict as fp_spec
    own = fp_spec.functions_of(ll, cnt, sw.df.f.alpha, sw.df.f.lms)
    assert wd.rel(dens, own.density) <= RTOL and np.array_equal(label, own.label)
    # ... and within the 1e-4 contract of the fp64 likelihoods of the same state
    sw64_ll = gpu.zeros((len(Xq), K), dtype=gpu.float64, device="cuda")
    _abi.check(L.segk_fbi_predict(ctx, C.byref(cv), fp, bp, _abi.ptr(cq.X), cq.ldx, len(Xq), _abi.ptr(prior_q), None, None, None,
                                  0, _abi.ptr(sw64_ll), K, st))
    gpu.cuda.synchronize()
    ll64 = sw64_ll.cpu().numpy()
    worst_ll = float(np.max(np.abs(ll - ll64) / np.maximum(1.0, np.abs(ll64))))
    assert worst_ll <= 1e-4, worst_ll
    worst_dens = wd.rel(dens, fp_spec.functions_of(ll64, cnt, sw.df.f.alpha, sw.df.f.lms).density)
    assert worst_dens <= 1e-4, worst_dens
    # 2. boundaries optimal for the device's span scores, totals at 1e-9; labels the argmax of the device's logits
    pz = np.log(float(sw.df.f.alpha) / K + cnt)
    worst_path = 0.0
    for i in range(u.D):
        N = u.lengths[i]
        vec = wd.span_vec(u, i, dens, seg.time_power_term, seg.wip)
        opt, _ = no.forward_backward_viterbi(vec, 0.0, N, seg.n_slices_min, seg.n_slices_max, i)
        got = mbm.path_total(vec, res.boundaries[i], N)
        tol = RTOL * max(1.0, abs(opt))
        worst_path = max(worst_path, (opt - got) / max(1.0, abs(opt)))
        assert got >= opt - tol and abs(got - res.log_prob[i]) <= tol, (i, got, opt, res.log_prob[i])
        segs = wd.segments_of(u, i, res.boundaries[i])
        lo, hi = res.seg_offsets[i], res.seg_offsets[i + 1]
        assert [e for _, _, e in segs] == res.seg_embed[lo:hi].tolist()
    occ = cnt > 0
    rank = np.cumsum(occ) - occ
    for e, k, d in zip(res.seg_embed, res.seg_label, res.seg_log_marg):
        z = pz + ll[e]
        slot = int(np.argmax(z))
        assert k == (rank[slot] if occ[slot] else res.K) and d == dens[e]
    print("%s f32: likelihoods %.3g, densities %.3g from fp64, worst shortfall of the path total %.3g" % (name, worst_ll, worst_dens, worst_path))


def test_float32_decode_on_settled_slots_of_thousands_of_items(gpu):
    """decode with score_precision="f32" where a float32 term's rounding is multiplied by a slot's count: the
    settled case st_D39_K8_n4096 of tests/fbgmm_items_f32.py -- two slots of 2 000 items each -- as a segmenter over
    utterances of one landmark, and held-out rows of the same clusters as held-out utterances of one landmark.  The one
    segment of such an utterance carries the row's held-out log density, and the utterance's log probability is that number:
    within the 1e-4 contract of the fp64 definition on the same statistics.  First the rows must show that they can tell the
    compensated term from the plain one: the emulation without the compensation misses the contract by 2 x or more on them."""
    from tests import fbgmm_items_f32 as f32
    name = "st_D39_K8_n4096"
    case = f32.SETTLED[name]
    Xq = f32.settled_queries(case)
    f32.discriminates(f32.spec_of(case), name, Xq)                      # (first: likelihoods; the densities below)
    seg = f32.segmenter_of(case)
    assert seg._get_sweeper().score_diag32
    held, keys = f32.one_landmark_corpus(Xq)
    res = seg.decode(*held)
    assert res.utterance_labels == keys and np.array_equal(res.seg_offsets, np.arange(len(Xq) + 1))
    assert np.array_equal(res.seg_embed, np.arange(len(Xq))) and res.boundaries.all()
    spec = f32.spec_of(case)
    d = spec.derive(*spec.stats_excluding(-1))
    want_ll, _, _, _ = f32.compare(spec, d, Xq)
    want = f32.marginals(spec, d, want_ll)
    centre = f32.centre_of(spec.X)
    rows = f32._Rows(spec, Xq)
    emulated, plain = (wd.rel(f32.marginals(spec, d, f32.emulate(rows, d, range(len(Xq)), centre, c)), want) for c in (True, False))
    worst = wd.rel(res.seg_log_marg, want)
    print("%s decode f32: log densities of %d held-out rows worst %.3g; the emulation %.3g, without the compensation %.3g"
          % (name, len(Xq), worst, emulated, plain))
    assert plain >= f32.DISCRIMINATES * f32.CONTRACT                    # (the inputs: or the rows prove nothing)
    assert worst <= f32.CONTRACT
    assert np.array_equal(res.log_prob, res.seg_log_marg)               # (one span of duration 1, no insertion penalty)
    # the labels: the first maximum of the fp64 logits wherever the specification's decision is clear of the contract
    pz = np.log(float(spec.alpha) / spec.K_max + d["cnt"])
    z = pz[None, :] + want_ll
    top = np.sort(z, axis=1)
    clear = top[:, -1] - top[:, -2] > 2 * f32.CONTRACT * np.maximum(1.0, np.abs(top[:, -1]))
    occ = d["cnt"] > 0
    rank = np.cumsum(occ) - occ
    k = np.argmax(z, axis=1)
    assert clear.sum() >= 0.9 * len(Xq)
    assert np.array_equal(res.seg_label[clear], np.where(occ[k], rank[k], res.K)[clear])


def test_fixed_variance_tolerance_sweepers_decode_in_fp64(gpu):
    """a fixed-variance sweeper of float32 span scores has no float32 item form: decode takes the fp64 likelihoods"""
    name = "fixed_small"
    seg = wd.product_swept(name, prec="f32")
    assert seg._get_sweeper().score_f32 and not seg._get_sweeper().score_diag32
    res = seg.decode(*wd.heldout_inputs(name))
    assert len(res.seg_label) > 0 and np.all(np.isfinite(res.log_prob))


# ------------------------------------------------------------------ refusals, each before any launch
def _seg(name="fixed_small"):
    return wd.product_swept(name)


def test_refusals(gpu):
    from segmentalist_amd._abi import SegkError
    name = "fixed_small"
    seg = _seg(name)
    held = wd.heldout_inputs(name)
    # beta_sent_boundary
    seg.beta_sent_boundary = 2.0
    with pytest.raises(SegkError, match="beta_sent_boundary"):
        seg.decode(*held)
    seg.beta_sent_boundary = -1
    # another D
    wide = tuple(dict(d) for d in held)
    for k in wide[0]:
        wide[0][k] = np.concatenate([wide[0][k], wide[0][k][:, :1]], axis=1)
    with pytest.raises(SegkError, match="D = 9"):
        seg.decode(*wide)
    # more than one rank
    sw = seg._get_sweeper()
    sw.world = 2
    with pytest.raises(SegkError, match="one process"):
        seg.decode(*held)
    sw.world = 1
    # n_slices_min
    seg.n_slices_min = 2
    with pytest.raises(SegkError, match="n_slices_min"):
        seg.decode(*held)
    seg.n_slices_min = 0
    # the band conditions: more than 64 landmarks with an unbounded window, a window over 64, an embedding outside the window,
    # a band beyond LDS
    long_held = wd.heldout_inputs("fixed_small_x_ragged")
    seg.n_slices_max = 0
    with pytest.raises(SegkError, match="window of 1..64"):
        seg.decode(*long_held)
    seg.n_slices_max = 65
    with pytest.raises(SegkError, match="window of 1..64"):
        seg.decode(*long_held)
    seg.n_slices_max = 4                                     # (the held-out tables hold spans of five slices)
    with pytest.raises(SegkError, match="no complete band"):
        seg.decode(*long_held)
    seg.n_slices_max = 5
    # the model is as it was: the refused calls launched nothing that moved it
    res = seg.decode(*held)
    assert_matches(res, wd.decoded(name)[0], "after the refusals")


def test_refusal_of_a_band_beyond_lds(gpu):
    from segmentalist_amd._abi import SegkError
    seg = _seg("fixed_small")
    sw = seg._get_sweeper()
    N, W = 260, 64
    assert wd.lds_bytes(N, W) > wd.BAND_LDS_MAX >= wd.lds_bytes(200, W)
    with pytest.raises(SegkError, match="does not fit in LDS"):
        sw.check_decode(seg._corpus.D, N, W, 0, W)
    sw.check_decode(seg._corpus.D, 200, W, 0, W)


def test_refusal_of_wide_and_of_full_covariance_limits(gpu):
    from segmentalist_amd._abi import SegkError
    seg = _seg("fixed_small")
    sw = seg._get_sweeper()
    sw.df.corpus.D, d = 257, sw.df.corpus.D
    try:
        with pytest.raises(SegkError, match="D <= 256"):
            sw.check_decode(257, 10, 0, 0, 5)
    finally:
        sw.df.corpus.D = d
    full = wd.product_swept("w0_K8")
    fsw = full._get_sweeper()
    assert fsw.fullcov
    fsw.df.K_max, k = 1025, fsw.df.K_max
    try:
        with pytest.raises(SegkError, match="K_max <= 1024"):
            fsw.check_decode(full._corpus.D, 10, 0, 0, 4)
    finally:
        fsw.df.K_max = k
    fsw.df.corpus.D, d = 65, fsw.df.corpus.D
    try:
        with pytest.raises(SegkError, match="D <= 64"):
            fsw.check_decode(65, 10, 0, 0, 4)
    finally:
        fsw.df.corpus.D = d


def test_bigram_segmenter_has_no_decode(gpu):
    from segmentalist_amd import bigram_acoustic_wordseg as baw
    assert not hasattr(baw.BigramAcousticWordseg, "decode")


def test_library_refuses_what_the_header_says(gpu):
    """segk_fbd_decode itself: SEGK_ERR_ARG before any launch, n_utt == 0 is SEGK_OK"""
    import ctypes as C
    from segmentalist_amd import _abi
    L, ctx = _abi.lib(), _abi.ctx()
    c = _abi.Corpus(n_utt=0)
    assert L.segk_fbd_decode(ctx, C.byref(c), 0, 5, 0.0, 1.0, None, None, None, None, None, None, None, None, None) == 0
    one = gpu.zeros(64, dtype=gpu.float64, device="cuda")
    c = _abi.Corpus(n_utt=1, N_max=100, lengths=one.data_ptr())
    p = _abi.ptr(one)
    for n_min, n_max, msg in ((2, 5, b"n_slices_min"), (0, 0, b"window of 1..64"), (0, 65, b"window of 1..64"), (0, 6, b"no complete band")):
        assert L.segk_fbd_decode(ctx, C.byref(c), n_min, n_max, 0.0, 1.0, p, p, p, p, p, p, p, p, None) == -1
        assert msg in L.segk_last_error(), msg
    c = _abi.Corpus(n_utt=1, N_max=260, lengths=one.data_ptr(), band_W=64, band_ids=one.data_ptr(), band_dur=one.data_ptr())
    assert L.segk_fbd_decode(ctx, C.byref(c), 0, 64, 0.0, 1.0, p, p, p, p, p, p, p, p, None) == -1
    assert b"does not fit in LDS" in L.segk_last_error()

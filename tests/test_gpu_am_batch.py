"""
GPU tests of the acoustic-model batch sweeps of the unigram segmenter (`FbgmmBatchSweeper.am_sweep`,
`UnigramAcousticWordseg.am_batch_sweep_async`, `gibbs_sample(..., am_n_iter=m, sync="batch", am_sync="batch")`; C entry point
`segk_fbt_assign`) against the NumPy specification tests/am_batch.py.
tests/test_am_batch_cpu.py shows that on these cases every draw is at least 1e-6 in probability clear of the cumulative edges,
so slots must coincide; likelihoods are held to the 1e-9 of the fp64 path, partial sums to 1e-13.
"""
import ctypes as C
import pickle
import random

import numpy as np
import pytest

from oracle import np_fbgmm_batch as nb
from tests import am_batch as ab

pytestmark = pytest.mark.gpu
RTOL = 1e-9
REC_KEYS = ["anneal_temp", "components", "log_marg", "log_marg*length", "log_prob_X_given_z", "log_prob_z", "n_tokens",
            "sample_time"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def pair(case, probe=None, **kw):
    seg_spec, spec = ab.spec_of(case)
    seg = ab.product_of(case, **kw)
    assert np.array_equal(seg.acoustic_model.components.assignments, spec.slot)
    assert np.array_equal(seg.utterances.boundaries, seg_spec.utterances.boundaries)
    if probe is not None:
        c = seg._df.corpus
        seg._get_sweeper().probe_ll = probe.zeros((c.n_utt * c.N_max, spec.K_max), dtype=probe.float64, device="cuda")
    return spec, seg


def frozen(seg):
    """what an inner sweep must leave bit-unchanged, as host copies"""
    df = seg._df
    return [t.cpu().numpy().copy() for t in (seg._dev_bounds, df.new_tok, df.n_new, df.out_logprob)]


def check_state(spec, seg, what=""):
    """slots, boundaries and the partial sums of every cell against the specification"""
    sw = seg._get_sweeper()
    assert np.array_equal(sw.slot.cpu().numpy(), spec.slot), what
    assert np.array_equal(seg.utterances.boundaries, spec.seg.utterances.boundaries), what
    worst = 0.0
    for s in range(spec.S):
        for b in range(spec.B):
            cnt, sx, sxx = sw.cell_partials(b, s)
            rc, rx, rxx = spec._partial(s, b)
            assert np.array_equal(cnt, rc), what
            worst = max(worst, rel(sx, rx), rel(sxx, rxx))
    print("%s partials %.3g" % (what, worst))
    assert worst <= 1e-13, what


def inner_both(gpu, spec, seg, index, temp=1.0, what=""):
    """One inner sweep of both; everything the issue holds equal after it."""
    sw = seg._get_sweeper()
    if not sw.in_batch_state:
        sw.enter(seg._dev_bounds)
    assert sw.sweep_index == index
    before = frozen(seg)
    spec.ll_log = {} if sw.probe_ll is not None else None
    spec.am_sweep(index, temp)
    seg.am_batch_sweep_async(temp)
    gpu.cuda.synchronize()
    seg._df.check_status()
    assert sw.sweep_index == index + 1
    for x, y, nm in zip(before, frozen(seg), ("boundaries", "new_tok", "n_new", "out_logprob")):
        assert x.tobytes() == y.tobytes(), (what, nm)
    if sw.probe_ll is not None:
        c = seg._df.corpus
        got = sw.probe_ll.cpu().numpy().reshape(c.n_utt, c.N_max, -1)
        worst = max([rel(got[i, t, :spec.K_max], ll) for (i, t), ll in spec.ll_log.items()] or [0.0])
        print("%s likelihoods %.3g over %d tokens" % (what, worst, len(spec.ll_log)))
        assert worst <= RTOL, what
    check_state(spec, seg, what)


@pytest.fixture(scope="module")
def finished(gpu):
    """name -> (spec, seg) after the sweeps of test_inner_sweeps (later tests go on from there)"""
    return {}


@pytest.mark.parametrize("name", list(ab.CASES))
def test_inner_sweeps(gpu, finished, name):
    case = ab.CASES[name]
    spec, seg = pair(case, probe=gpu)
    c = seg._df.corpus
    assert c.N_max == case[7] and (c.band_ids is not None) == (name == "dg_band_N80")
    for s, temp in enumerate(case[10]):
        inner_both(gpu, spec, seg, s, temp, "%s sweep %d" % (name, s))
    finished[name] = (spec, seg)


def test_logits_workspace_walked_in_several_launches(gpu, monkeypatch):
    """K_max = 300 at D = 39: a tile's logits do not fit in LDS.  With the workspace bound at 1 MiB a launch holds six tiles
    and the eight the host's token bound asks for per block are walked in two launches: the same slots, likelihoods and sums."""
    monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")
    case = ab.CASES["fx_D39_K300_tiles"]
    spec, seg = pair(case, probe=gpu)
    sw = seg._get_sweeper()
    tiles = min(sum((cap + ab.TILE - 1) // ab.TILE for cap in sw._tok_cap[b]) for b in range(sw.B))
    assert tiles > (1 << 20) // (ab.TILE * case[3] * 8)
    for s, temp in enumerate(case[10]):
        inner_both(gpu, spec, seg, s, temp, "bounded workspace, sweep %d" % s)


@pytest.mark.parametrize("name", ["fx_D39_K7_tiles", "dg_D39_K65_tiles", "dg_band_N80"])
def test_cross_route_on_the_device(gpu, name):
    """From the same state, the new step and segk_fbb_assign on the unchanged token lists (prepare, assign, partials per
    block, the same sweep index and temperature): equal slots and partial sums, bit-equal probe likelihoods."""
    from segmentalist_amd import _abi
    case = ab.CASES[name]
    _, a = pair(case, probe=gpu)
    _, b = pair(case)
    sa, sb = a._get_sweeper(), b._get_sweeper()
    sb.enter(b._dev_bounds)
    c = b._df.corpus
    ll = gpu.zeros((c.n_utt * c.N_max, case[3]), dtype=gpu.float64, device="cuda")
    for index, temp in enumerate(case[10]):
        a.am_batch_sweep_async(temp)
        L, ctx, cp, fp, bp, st = sb._args()
        _abi.check(L.segk_fbb_set_probe(ctx, None, _abi.ptr(ll), case[3]))
        try:
            for blk in range(sb.B):
                _abi.check(L.segk_fbb_prepare(ctx, cp, fp, bp, blk, st))
                _abi.check(L.segk_fbb_assign(ctx, cp, fp, bp, sb.s_lo, sb.s_n, blk, sb._n_utts[blk], index, float(temp),
                                             _abi.ptr(b._df.new_tok), _abi.ptr(b._df.n_new), None, 0, st))
                _abi.check(L.segk_fbb_partials(ctx, cp, fp, bp, sb.s_lo, sb.s_n, blk, _abi.ptr(b._df.new_tok),
                                               _abi.ptr(b._df.n_new), st))
            gpu.cuda.synchronize()
        finally:
            _abi.check(L.segk_fbb_set_probe(ctx, None, None, 0))
        assert gpu.equal(sa.slot, sb.slot), (name, index)
        assert gpu.equal(sa.partials, sb.partials), (name, index)
        assert gpu.equal(sa.probe_ll, ll), (name, index)
        assert float(ll.abs().max()) > 0
    a._df.check_status()


def outer_both(gpu, spec, seg, index, what=""):
    lp = nb.FbgmmBatch.sweep(spec, index, 1.0, False)
    seg.batch_sweep_async()
    gpu.cuda.synchronize()
    seg._df.check_status()
    assert seg._get_sweeper().sweep_index == index + 1
    assert rel(seg._df.out_logprob.cpu().numpy(), lp) <= RTOL, what
    check_state(spec, seg, what)


def spec_record(spec, case):
    """the record entries of the specification's current state: the host expressions on a fresh model of its canonical view"""
    canon, K = spec.canonical()
    am = ab.fi.spec_model(case[0], spec.X, spec.K_max, canon)
    lpz, lpx = am.log_prob_z(), (am.components.log_marg() if case[0] == "full" else am.log_prob_X_given_z())
    return {"log_prob_z": lpz, "log_prob_X_given_z": lpx, "log_marg": lpz + lpx, "components": K,
            "n_tokens": int(np.count_nonzero(canon >= 0))}


@pytest.mark.parametrize("name", list(ab.INTERLEAVED))
def test_interleaved_gibbs_sample(gpu, name):
    """gibbs_sample(3, am_n_iter=2, sync="batch", am_sync="batch"): two inner sweeps before every outer sweep, one shared
    sweep counter, no random.random() consumed, the usual record keys; then a serial sweep, and a second such call re-enters
    from the serial result."""
    case = ab.INTERLEAVED[name]
    spec, seg = pair(case)
    state = random.getstate()
    rec = seg.gibbs_sample(3, am_n_iter=2, sync="batch", am_sync="batch")
    assert random.getstate() == state
    assert sorted(rec) == REC_KEYS and all(len(v) == 3 for v in rec.values())
    index = 0
    for it in range(3):
        for _ in range(2):
            spec.am_sweep(index, 1.0)
            index += 1
        lp = nb.FbgmmBatch.sweep(spec, index, 1.0, False)
        index += 1
        want = dict(spec_record(spec, case), **{"log_marg*length": float(np.sum(lp)), "anneal_temp": 1})
        for k, v in want.items():
            print("%s iteration %d record %s: %.17g against %.17g" % (name, it, k, rec[k][it], v))
            assert abs(rec[k][it] - v) <= RTOL * max(1.0, abs(v)), (k, it)
    sw = seg._get_sweeper()
    assert sw.sweep_index == index == 9 and sw.in_batch_state
    check_state(spec, seg, "after the interleaved call")
    assert np.array_equal(seg.acoustic_model.components.assignments, spec.canonical()[0])
    # a serial sweep, then the specification rebuilt from its result
    random.seed(5)
    seg.gibbs_sample(1, sync="sequential")
    assert not sw.in_batch_state
    spec.seg.utterances.boundaries[:] = seg.utterances.boundaries
    spec.slot = np.array(seg.acoustic_model.components.assignments, dtype=spec.slot.dtype)
    spec.P = [[spec._partial(s, b) for b in range(spec.B)] for s in range(spec.S)]
    seg.gibbs_sample(1, am_n_iter=1, sync="batch", am_sync="batch")
    spec.am_sweep(index, 1.0)
    nb.FbgmmBatch.sweep(spec, index + 1, 1.0, False)
    assert sw.sweep_index == index + 2 and sw.in_batch_state
    check_state(spec, seg, "re-entered after a serial sweep")


def test_interleaved_with_viterbi_outer_sweeps(gpu):
    """fb_type="viterbi": the outer sweeps are the MAP sweeps, the inner sweeps still sample -- the same calls issued by hand."""
    case = ab.INTERLEAVED["il_dg"]
    _, a = pair(case, fb_type="viterbi")
    _, b = pair(case, fb_type="viterbi")
    a.gibbs_sample(2, am_n_iter=1, sync="batch", am_sync="batch")
    for _ in range(2):
        b.am_batch_sweep_async()
        b.batch_sweep_async()
    gpu.cuda.synchronize()
    sa, sb = a._get_sweeper(), b._get_sweeper()
    assert sa.sweep_index == sb.sweep_index == 4
    assert gpu.equal(sa.slot, sb.slot) and gpu.equal(a._dev_bounds, b._dev_bounds) and gpu.equal(sa.partials, sb.partials)
    start = ab.spec_of(case)[1].slot
    assert np.count_nonzero(sa.slot.cpu().numpy() != start) >= 1


@pytest.mark.parametrize("name", ["dg_D39_K65_tiles", "fx_D3_K7_8x8", "fc_D39_K7_2x2"])
def test_materialise_after_an_inner_sweep(gpu, finished, name):
    """materialise(): assignments and K are canonical(); the serial statistics are, bit for bit, those of a fresh model
    constructed from those assignments; the batch state is not touched."""
    if name not in finished:
        test_inner_sweeps(gpu, finished, name)
    spec, seg = finished[name]
    seg.materialise()
    canon, K = spec.canonical()
    c = seg.acoustic_model.components
    assert c.K == K and np.array_equal(c.assignments, canon)
    fresh = ab.product_of(ab.CASES[name], seeds=ab.seeds_from(spec, canon))
    assert np.array_equal(fresh.acoustic_model.components.assignments, canon)
    for nm in ("counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "K", "assignments"):
        assert gpu.equal(getattr(seg._df, nm), getattr(fresh._df, nm)), nm
    sw = seg._get_sweeper()
    assert sw.in_batch_state and np.array_equal(sw.slot.cpu().numpy(), spec.slot)


@pytest.mark.parametrize("name", ["il_dg", "il_fc"])
def test_checkpoint_after_an_inner_sweep(gpu, name):
    """a checkpoint taken after an inner sweep resumes, in a freshly constructed object, to the same next sweeps"""
    case = ab.INTERLEAVED[name]
    _, a = pair(case)
    a.am_batch_sweep_async()
    sd = pickle.loads(pickle.dumps(a.state_dict()))
    assert sd["batch_sweep_index"] == 1
    b = ab.product_of(case)
    b.load_state_dict(sd)
    for seg in (a, b):
        seg.am_batch_sweep_async()
        seg.batch_sweep_async()
    gpu.cuda.synchronize()
    sa, sb = a._get_sweeper(), b._get_sweeper()
    assert sa.sweep_index == sb.sweep_index == 3
    assert gpu.equal(sa.slot, sb.slot) and gpu.equal(a._dev_bounds, b._dev_bounds) and gpu.equal(sa.partials, sb.partials)
    a._df.check_status()
    b._df.check_status()


@pytest.mark.parametrize("name", ["il_dg", "il_fc"])
def test_am_sync_none_keeps_the_serial_inner_sweeps(gpu, name):
    """am_sync=None with am_n_iter=2, sync="batch": leave batch mode, the serial chain over the assigned tokens, one batch
    sweep -- the same record and state as that sequence issued by hand under the same `random` seed."""
    case = ab.INTERLEAVED[name]
    _, a = pair(case)
    _, b = pair(case)
    for seg in (a, b):
        seg.batch_sweep_async()                              # (both in batch mode when the call begins)
    random.seed(7)
    ra = a.gibbs_sample(1, am_n_iter=2, sync="batch")
    after_a = random.getstate()
    random.seed(7)
    b._leave_batch()
    b.acoustic_model.gibbs_sample(2, consider_unassigned=False)
    rb = b.gibbs_sample(1, sync="batch")
    assert random.getstate() == after_a
    for k in REC_KEYS:
        if k != "sample_time":
            assert ra[k] == rb[k], k
    sa, sb = a._get_sweeper(), b._get_sweeper()
    assert sa.sweep_index == sb.sweep_index == 2
    assert gpu.equal(sa.slot, sb.slot) and gpu.equal(a._dev_bounds, b._dev_bounds) and gpu.equal(sa.partials, sb.partials)
    assert np.array_equal(a.acoustic_model.components.assignments, b.acoustic_model.components.assignments)
    # "sequential" is the same route
    _, c = pair(case)
    c.batch_sweep_async()
    random.seed(7)
    rc = c.gibbs_sample(1, am_n_iter=2, sync="batch", am_sync="sequential")
    assert all(ra[k] == rc[k] for k in REC_KEYS if k != "sample_time")


def test_refusals(gpu):
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.niw import NIW
    from tests import fbgmm_items as fi
    from tests import fbgmm_long as fl
    case = ab.INTERLEAVED["il_dg"]
    # the bigram segmenter shares the sweeper: a language model is refused by name, by the method and by the library
    big = fl.product_of("short_bigram")
    sw = big._get_sweeper()
    assert not hasattr(big, "am_batch_sweep_async")
    with pytest.raises(SegkError, match="language model"):
        sw.am_sweep(big._dev_bounds)
    assert not sw.in_batch_state and sw.sweep_index == 0
    L, ctx, cp, fp, bp, st = sw._args()
    df = big._df
    rc = L.segk_fbt_assign(ctx, cp, fp, bp, sw.s_lo, sw.s_n, 0, sw._n_utts[0], sw._tok_cap[0], 0, 1.0, _abi.ptr(df.new_tok),
                           _abi.ptr(df.n_new), None, 0, st)
    assert rc == _abi.SEGK_ERR_UNSUPPORTED and "language model" in L.segk_last_error().decode()
    # reduced-precision scores
    f32 = ab.product_of(case, score_precision="f32")
    with pytest.raises(SegkError, match="score_precision='f64' only"):
        f32.am_batch_sweep_async()
    with pytest.raises(SegkError, match="score_precision='f64' only"):
        f32.gibbs_sample(1, am_n_iter=1, sync="batch", am_sync="batch")
    # inner batch sweeps run inside batch mode
    seg = ab.product_of(case)
    with pytest.raises(AssertionError, match="am_sync"):
        seg.gibbs_sample(1, am_n_iter=1, sync="sequential", am_sync="batch")
    with pytest.raises(AssertionError, match="am_sync"):
        seg.gibbs_sample(1, am_n_iter=1, am_sync="batch")   # (the object was built with sync="sequential")
    # more than one rank
    sws = seg._get_sweeper()
    sws.world = 2
    with pytest.raises(SegkError, match="one process"):
        seg.am_batch_sweep_async()
    sws.world = 1
    # full covariance beyond the batch kernels' limit
    many = list(ab.INTERLEAVED["il_fc"])
    many[3] = 1025
    with pytest.raises(SegkError, match="K_max <= 1024"):
        ab.product_of(many).am_batch_sweep_async()
    # a corpus without span tables is the stand-alone model's: refused by the library before any launch
    seg.am_batch_sweep_async()
    gpu.cuda.synchronize()
    L, ctx, cp, fp, bp, st = sws._args()
    items = fi.product_of(fi.CASES["fx_D3_K7_n5_8x8"])
    items.batch_sweep_async()
    gpu.cuda.synchronize()
    isw = items._get_sweeper()
    rc = L.segk_fbt_assign(ctx, C.byref(isw.c), fp, bp, sws.s_lo, sws.s_n, 0, sws._n_utts[0], sws._tok_cap[0], 0, 1.0,
                           _abi.ptr(seg._df.new_tok), _abi.ptr(seg._df.n_new), None, 0, st)
    assert rc != 0 and "segmenter's corpus" in L.segk_last_error().decode()
    gpu.cuda.synchronize()
    seg._df.check_status()

"""
GPU tests of the FLOAT32 acoustic-model batch sweeps of the unigram segmenter (`FbgmmBatchSweeper.am_sweep(...,
score_precision="f32")`, `UnigramAcousticWordseg.am_batch_sweep_async(score_precision="f32")`, `gibbs_sample(...,
am_sync="batch", am_score_precision="f32")`; C entry points `segk_fbt_assign_diag32` and, below the dispatch constant,
`segk_fbb_assign_diag32`) against the fp64 specification tests/am_batch.py under the project's tolerance contract.
tests/test_am_batch_f32_cpu.py checks the inputs first (cases, emulation, margins).

REPLAY of an inner sweep.  A token is resampled in exactly one step, so one probe tensor (prefilled with NaN) holds, after the
whole sweep, every token's likelihood row.  One inner sweep runs on the device; then the specification is walked block by
block on the device's own rows and slots:

  * d = derive(stats_excluding(b));
  * occupied slots: |got - want| <= 1e-4 max(|want|, 1) against AmBatch.loglik; empty slots: the prior predictive at 1e-9;
  * every token's slot is draw_chunked of the specification's prior term, annealing and u01(seed, sweep, i, N_max + t) applied
    to the device's OWN probe row;
  * the device's slots are applied to the specification and the block's partial sums recomputed.

After the sweep: the partial sums of every cell at 1e-13, boundaries / new_tok / n_new / out_logprob bit-unchanged, the sweep
index advanced by one, the probe rows of non-tokens still NaN.
"""
import ctypes as C
import pickle
import random

import numpy as np
import pytest

from oracle import np_fbgmm_batch as nb
from tests import am_batch as ab
from tests import am_batch_f32 as a32
from tests.test_gpu_am_batch import REC_KEYS, RTOL, check_state, frozen, rel, spec_record

pytestmark = pytest.mark.gpu
ROUTES = ("segk_fbt_assign_diag32", "segk_fbb_assign_diag32", "segk_fbt_assign")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


class Spy(object):
    """the library with the calls of the token-step entry points counted (which route a sweep took)"""

    def __init__(self, lib):
        self._lib = lib
        self.calls = {name: 0 for name in ROUTES}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ROUTES:
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def pair(gpu, case, transform="identity", **kw):
    """(specification, device segmenter with a NaN probe and a spy on its library) of the same initial state"""
    seg_spec, spec = a32.spec_of(case, transform)
    seg = a32.product_of(case, transform, **kw)
    assert np.array_equal(seg.acoustic_model.components.assignments, spec.slot)
    assert np.array_equal(seg.utterances.boundaries, seg_spec.utterances.boundaries)
    c = seg._df.corpus
    seg._get_sweeper().probe_ll = gpu.full((c.n_utt * c.N_max, spec.K_max), float("nan"), dtype=gpu.float64, device="cuda")
    seg._df._L = Spy(seg._df._L)
    return spec, seg


def replay(gpu, spec, seg, index, temp=1.0, what="", launch=None):
    """One float32 inner sweep on the device, replayed on the specification (module docstring)."""
    sw = seg._get_sweeper()
    if not sw.in_batch_state:
        sw.enter(seg._dev_bounds)
    assert sw.sweep_index == index, what
    before = frozen(seg)
    sw.probe_ll.fill_(float("nan"))
    if launch is None:
        seg.am_batch_sweep_async(temp, score_precision="f32")
    else:
        launch()
    gpu.cuda.synchronize()
    seg._df.check_status()
    assert sw.sweep_index == index + 1, what
    for x, y, nm in zip(before, frozen(seg), ("boundaries", "new_tok", "n_new", "out_logprob")):
        assert x.tobytes() == y.tobytes(), (what, nm)
    c = seg._df.corpus
    K = spec.K_max
    got = sw.probe_ll.cpu().numpy().reshape(c.n_utt, c.N_max, -1)[:, :, :K]
    slots = sw.slot.cpu().numpy()
    seen = np.zeros((c.n_utt, c.N_max), bool)
    worst = worst_empty = 0.0
    draws = 0
    for b in range(spec.B):
        d, toks, want, p, u, new = a32.step(spec, index, b, temp, likelihoods=lambda d, toks: [got[i, t] for i, t, _ in toks])
        if toks:
            where = "%s block %d" % (what, b)
            rows = np.array([got[i, t] for i, t, _ in toks])
            assert np.isfinite(rows).all(), where
            occ = d["active"]
            worst = max(worst, rel(rows[:, occ], want[:, occ]))
            worst_empty = max(worst_empty, rel(rows[:, ~occ], want[:, ~occ]))
            for j, (i, t, e) in enumerate(toks):
                assert not seen[i, t]
                seen[i, t] = True
                draws += 1
                assert slots[e] == new[j], (where, i, t, a32.margin(p[j], u[j]))
        a32.apply_slots(spec, b, toks, [slots[e] for _, _, e in toks])      # the specification goes on from the device's slots
    print("%s: worst likelihood error %.3g (occupied), %.3g (empty) over %d tokens" % (what, worst, worst_empty, draws))
    assert draws == int(seen.sum()) >= 1, what
    assert worst <= a32.CONTRACT, what
    assert worst_empty <= 1e-9, what
    assert np.isnan(got[~seen]).all(), what                                  # the probe rows of non-tokens are untouched
    check_state(spec, seg, what)


def taken(seg):
    return dict(seg._df._L.calls)


@pytest.fixture(scope="module")
def finished(gpu):
    """name -> (spec, seg) after the sweeps of test_replay (later tests go on from there)"""
    return {}


@pytest.mark.parametrize("name,transform", a32.RUNS, ids=["%s-%s" % r for r in a32.RUNS])
def test_replay(gpu, finished, monkeypatch, name, transform):
    """every case and every included transform, on an fp64 sweeper, by the tile kernel (the dispatch constant would hand
    these small blocks to the other route: test_replay_on_either_route, test_dispatch_by_the_constant)"""
    monkeypatch.setenv("SEGK_AM32_TILE_MIN", a32.TILES)
    case = a32.CASES[name]
    spec, seg = pair(gpu, case, transform)
    sw = seg._get_sweeper()
    assert sw.score_precision == "f64" and sw.bt.centre is None and sw.bt.tab32 is None
    for s, temp in enumerate(a32.temps_of(case)):
        replay(gpu, spec, seg, s, temp, "%s %s sweep %d" % (name, transform, s))
    # the copy of the batch state: the whole corpus' fp64 column mean in row order, a table of its own; `bt` as it was
    assert sw.bt.centre is None and sw.bt.tab32 is None and sw._bt32.centre and sw._bt32.tab32
    assert np.array_equal(sw._centre32.cpu().numpy(), a32.centre_of(spec.X))
    assert taken(seg) == {"segk_fbt_assign_diag32": sw.B * len(a32.temps_of(case)), "segk_fbb_assign_diag32": 0, "segk_fbt_assign": 0}
    if transform == "identity":
        finished[name] = (spec, seg)


@pytest.mark.parametrize("name", a32.BOTH_PRECISIONS)
def test_replay_on_a_float32_sweeper(gpu, monkeypatch, name):
    """a sweeper built with score_precision="f32" (score_diag32): its own centre and tab32"""
    monkeypatch.setenv("SEGK_AM32_TILE_MIN", a32.TILES)
    case = a32.CASES[name]
    spec, seg = pair(gpu, case, score_precision="f32")
    sw = seg._get_sweeper()
    assert sw.score_diag32 and sw.bt.centre and sw.bt.tab32
    for s, temp in enumerate(a32.temps_of(case)):
        replay(gpu, spec, seg, s, temp, "%s f32 sweeper sweep %d" % (name, s))
    assert sw._bt32 is None and taken(seg)["segk_fbt_assign_diag32"] == sw.B * len(a32.temps_of(case))


def test_dispatch_by_the_constant(gpu, monkeypatch):
    """without SEGK_AM32_TILE_MIN the host's token bound of every block is held against device.AM32_TILE_MIN: blocks of 80, 100
    and 120 landmarks against a constant of 100 take the other route, the tiles, the tiles -- in one sweep, the same replay"""
    from segmentalist_amd import device
    monkeypatch.delenv("SEGK_AM32_TILE_MIN", raising=False)
    monkeypatch.setattr(device, "AM32_TILE_MIN", 100)
    case = a32.CASES["dg_D100_K7_3x4"]
    spec, seg = pair(gpu, case)
    sw = seg._get_sweeper()
    assert [sum(cap) for cap in sw._tok_cap] == [80, 100, 120]
    for s, temp in enumerate(a32.temps_of(case)):
        replay(gpu, spec, seg, s, temp, "mixed routes, sweep %d" % s)
    assert taken(seg) == {"segk_fbt_assign_diag32": 4, "segk_fbb_assign_diag32": 2, "segk_fbt_assign": 0}


@pytest.mark.parametrize("route", ["tiles", "slots"])
@pytest.mark.parametrize("name", a32.BOTH_ROUTES)
def test_replay_on_either_route(gpu, monkeypatch, name, route):
    """SEGK_AM32_TILE_MIN forces the tile kernel (0) or segk_fbb_assign_diag32 on the unchanged token lists (huge)"""
    monkeypatch.setenv("SEGK_AM32_TILE_MIN", a32.TILES if route == "tiles" else a32.SLOTS)
    case = a32.CASES[name]
    spec, seg = pair(gpu, case)
    n = len(a32.temps_of(case))
    for s, temp in enumerate(a32.temps_of(case)):
        replay(gpu, spec, seg, s, temp, "%s %s sweep %d" % (name, route, s))
    B = seg._get_sweeper().B
    want = {"segk_fbt_assign_diag32": n * B if route == "tiles" else 0, "segk_fbb_assign_diag32": 0 if route == "tiles" else n * B,
            "segk_fbt_assign": 0}
    assert taken(seg) == want


def test_logits_workspace_walked_in_two_launches(gpu, monkeypatch):
    """K_max = 300 at D = 39: a tile's logits do not fit in LDS.  With the workspace bound at 1 MiB a launch holds six tiles of
    64 x 301 doubles and the eight the host's token bound asks for per block are walked in two launches."""
    monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")
    monkeypatch.setenv("SEGK_AM32_TILE_MIN", a32.TILES)
    case = a32.CASES["dg_D39_K300_tiles"]
    spec, seg = pair(gpu, case)
    sw = seg._get_sweeper()
    tiles = min(sum((cap + a32.TILE - 1) // a32.TILE for cap in sw._tok_cap[b]) for b in range(sw.B))
    assert tiles == 8 > (1 << 20) // (a32.TILE * (case[3] | 1) * 8)
    for s, temp in enumerate(a32.temps_of(case)):
        replay(gpu, spec, seg, s, temp, "bounded workspace, sweep %d" % s)


def test_interleaved_gibbs_sample(gpu, monkeypatch):
    """gibbs_sample(3, am_n_iter=2, sync="batch", am_sync="batch", am_score_precision="f32") on an fp64 sweeper: every inner
    sweep gets the keyword and is replayed, every outer sweep is the fp64 one of nb.FbgmmBatch.sweep from the same state
    (bit-equal slots and boundaries, log-probabilities at 1e-9), on the one shared counter; then a serial sweep and a
    re-entry."""
    case = a32.CASES["il_dg"]
    from segmentalist_amd import device
    monkeypatch.delenv("SEGK_AM32_TILE_MIN", raising=False)
    spec, seg = pair(gpu, case)
    sw = seg._get_sweeper()
    inner, outer = seg.am_batch_sweep_async, seg.batch_sweep_async
    log = {"index": 0, "lp": [], "kinds": []}

    def inner_checked(anneal_temp=1, score_precision=None):
        assert score_precision == "f32" and anneal_temp == 1
        replay(gpu, spec, seg, log["index"], 1.0, "interleaved inner sweep at index %d" % log["index"],
               launch=lambda: inner(anneal_temp, score_precision))
        log["index"] += 1
        log["kinds"].append("inner")

    def outer_checked(*args, **kw):
        assert sw.sweep_index == log["index"]
        lp = nb.FbgmmBatch.sweep(spec, log["index"], 1.0, False)
        outer(*args, **kw)
        gpu.cuda.synchronize()
        seg._df.check_status()
        what = "interleaved outer sweep at index %d" % log["index"]
        assert sw.sweep_index == log["index"] + 1
        assert rel(seg._df.out_logprob.cpu().numpy(), lp) <= RTOL, what
        check_state(spec, seg, what)
        log["index"] += 1
        log["lp"].append(float(np.sum(lp)))
        log["kinds"].append("outer")

    seg.am_batch_sweep_async, seg.batch_sweep_async = inner_checked, outer_checked
    state = random.getstate()
    rec = seg.gibbs_sample(3, am_n_iter=2, sync="batch", am_sync="batch", am_score_precision="f32")
    assert random.getstate() == state
    assert log["kinds"] == ["inner", "inner", "outer"] * 3 and sw.sweep_index == 9 and sw.in_batch_state
    assert sorted(rec) == REC_KEYS and all(len(v) == 3 for v in rec.values())
    assert rec["log_marg*length"] == pytest.approx(log["lp"], rel=RTOL)
    want = spec_record(spec, case)                       # the last iteration's record: the specification's final state
    for k, v in want.items():
        assert abs(rec[k][2] - v) <= RTOL * max(1.0, abs(v)), k
    assert sw.bt.centre is None and sw.bt.tab32 is None
    assert np.array_equal(seg.acoustic_model.components.assignments, spec.canonical()[0])
    calls = taken(seg)
    # (the route the shipped constant gives these blocks)
    assert calls["segk_fbt_assign_diag32"] == 6 * sum(1 for cap in sw._tok_cap if sum(cap) >= device.AM32_TILE_MIN)
    assert calls["segk_fbt_assign"] == 0 and calls["segk_fbt_assign_diag32"] + calls["segk_fbb_assign_diag32"] == 6 * sw.B
    # a serial sweep, then the specification rebuilt from its result and a re-entry
    random.seed(5)
    seg.gibbs_sample(1, sync="sequential")
    assert not sw.in_batch_state
    spec.seg.utterances.boundaries[:] = seg.utterances.boundaries
    spec.slot = np.array(seg.acoustic_model.components.assignments, dtype=spec.slot.dtype)
    spec.P = [[spec._partial(s, b) for b in range(spec.B)] for s in range(spec.S)]
    seg.gibbs_sample(1, am_n_iter=1, sync="batch", am_sync="batch", am_score_precision="f32")
    assert log["kinds"][-2:] == ["inner", "outer"] and sw.sweep_index == 11 and sw.in_batch_state


@pytest.mark.parametrize("name", ["dg_D39_K65_tiles", "dg_D3_K7_8x8"])
def test_materialise_after_a_float32_inner_sweep(gpu, finished, monkeypatch, name):
    """materialise(): assignments and K are canonical(); the serial statistics are, bit for bit, those of a fresh model
    constructed from those assignments; the batch state is not touched."""
    if name not in finished:
        test_replay(gpu, finished, monkeypatch, name, "identity")
    spec, seg = finished[name]
    seg.materialise()
    canon, K = spec.canonical()
    c = seg.acoustic_model.components
    assert c.K == K and np.array_equal(c.assignments, canon)
    fresh = ab.product_of(a32.CASES[name], seeds=ab.seeds_from(spec, canon))
    assert np.array_equal(fresh.acoustic_model.components.assignments, canon)
    for nm in ("counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "K", "assignments"):
        assert gpu.equal(getattr(seg._df, nm), getattr(fresh._df, nm)), nm
    sw = seg._get_sweeper()
    assert sw.in_batch_state and np.array_equal(sw.slot.cpu().numpy(), spec.slot)


def test_record_keys(gpu):
    case = a32.CASES["il_dg"]
    seg = a32.product_of(case)
    rec = seg.gibbs_sample(2, am_n_iter=1, sync="batch", am_sync="batch", am_score_precision="f32")
    assert sorted(rec) == REC_KEYS
    for k, v in rec.items():
        assert len(v) == 2 and np.all(np.isfinite(np.asarray(v, np.float64))), k
    assert seg._get_sweeper().sweep_index == 4


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_checkpoint_after_a_float32_inner_sweep(gpu, precision):
    """a checkpoint taken after a float32 inner sweep resumes, in a freshly constructed object, to the same next sweeps"""
    case = a32.CASES["il_dg"]
    a = a32.product_of(case, score_precision=precision)
    a.am_batch_sweep_async(score_precision="f32")
    sd = pickle.loads(pickle.dumps(a.state_dict()))
    assert sd["batch_sweep_index"] == 1
    b = a32.product_of(case, score_precision=precision)
    b.load_state_dict(sd)
    for seg in (a, b):
        seg.am_batch_sweep_async(score_precision="f32")
        seg.batch_sweep_async()
    gpu.cuda.synchronize()
    sa, sb = a._get_sweeper(), b._get_sweeper()
    assert sa.sweep_index == sb.sweep_index == 3
    assert gpu.equal(sa.slot, sb.slot) and gpu.equal(a._dev_bounds, b._dev_bounds) and gpu.equal(sa.partials, sb.partials)
    a._df.check_status()
    b._df.check_status()


def test_refusals(gpu):
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import SegkError
    from tests import fbgmm_items as fi
    from tests import fbgmm_long as fl
    case = a32.CASES["il_dg"]

    def untouched(sw):
        return not sw.in_batch_state and sw.sweep_index == 0 and sw._bt32 is None
    # components other than diagonal: the mode exists for diagonal components
    for other in (ab.CASES["fx_D3_K1_1x1"], ab.INTERLEAVED["il_fc"]):
        seg = ab.product_of(other)
        with pytest.raises(SegkError, match="diagonal components"):
            seg.am_batch_sweep_async(score_precision="f32")
        with pytest.raises(SegkError, match="diagonal components"):
            seg.gibbs_sample(1, am_n_iter=1, sync="batch", am_sync="batch", am_score_precision="f32")
        assert untouched(seg._get_sweeper())
    # a language model: by the method and by the library
    big = fl.product_of("short_bigram")
    sw = big._get_sweeper()
    with pytest.raises(SegkError, match="language model"):
        sw.am_sweep(big._dev_bounds, 1.0, "f32")
    assert untouched(sw)
    L, ctx, cp, fp, bp, st = sw._args()
    df = big._df
    rc = L.segk_fbt_assign_diag32(ctx, cp, fp, bp, sw.s_lo, sw.s_n, 0, sw._n_utts[0], sw._tok_cap[0], 0, 1.0, _abi.ptr(df.new_tok),
                                  _abi.ptr(df.n_new), None, 0, st)
    assert rc == _abi.SEGK_ERR_UNSUPPORTED
    assert "language model" in L.segk_last_error().decode() or "cov_type" in L.segk_last_error().decode()
    # more than one rank, an invalid value, the keyword without batch inner sweeps
    seg = a32.product_of(case)
    sws = seg._get_sweeper()
    sws.world = 2
    with pytest.raises(SegkError, match="one process"):
        seg.am_batch_sweep_async(score_precision="f32")
    sws.world = 1
    for bad in ("f16", "float32", 32):
        with pytest.raises(SegkError, match="score_precision"):
            seg.am_batch_sweep_async(score_precision=bad)
    assert untouched(sws)
    with pytest.raises(AssertionError, match="am_score_precision"):
        seg.gibbs_sample(1, am_n_iter=1, sync="batch", am_score_precision="f32")
    with pytest.raises(AssertionError, match="am_score_precision"):
        seg.gibbs_sample(1, am_n_iter=1, sync="batch", am_sync="sequential", am_score_precision="f32")
    assert untouched(sws)
    # the default call on a reduced-precision sweeper keeps its refusal, "f64" passed explicitly too
    f32seg = a32.product_of(case, score_precision="f32")
    for value in (None, "f64"):
        with pytest.raises(SegkError, match="score_precision='f64' only"):
            f32seg.am_batch_sweep_async(score_precision=value)
    with pytest.raises(SegkError, match="score_precision='f64' only"):
        f32seg.gibbs_sample(1, am_n_iter=1, sync="batch", am_sync="batch", am_score_precision="f64")
    # the library's own: return code plus segk_last_error, nothing launched
    seg.am_batch_sweep_async(score_precision="f32")
    gpu.cuda.synchronize()
    L, ctx, cp, fp, _, st = sws._args()
    bt32 = sws._bt32
    slots = sws.slot.clone()

    def call(c=cp, f=fp, bt=C.byref(bt32)):
        return L.segk_fbt_assign_diag32(ctx, c, f, bt, sws.s_lo, sws.s_n, 0, sws._n_utts[0], sws._tok_cap[0], 7, 1.0,
                                        _abi.ptr(seg._df.new_tok), _abi.ptr(seg._df.n_new), None, 0, st)
    for cov in (0, 2):
        f_cov = _abi.FbgmmDev.from_buffer_copy(sws.f)
        f_cov.cov_type = cov
        assert call(f=C.byref(f_cov)) == _abi.SEGK_ERR_UNSUPPORTED
        assert "cov_type %d" % cov in L.segk_last_error().decode()
    f_lm = _abi.FbgmmDev.from_buffer_copy(sws.f)
    f_lm.lm_unigram = seg._df.counts.data_ptr()
    assert call(f=C.byref(f_lm)) == _abi.SEGK_ERR_UNSUPPORTED and "language model" in L.segk_last_error().decode()
    for field in ("tab32", "centre", "prior_rows"):
        bt = _abi.FbatchDev.from_buffer_copy(bt32)
        setattr(bt, field, None)
        assert call(bt=C.byref(bt)) == -1 and "tab32" in L.segk_last_error().decode(), field       # SEGK_ERR_ARG
    assert call(bt=C.byref(sws.bt)) == -1 and "tab32" in L.segk_last_error().decode()               # the fp64 sweeper's own state
    items = fi.product_of(fi.CASES["dg_D3_K7_n1"])
    items.batch_sweep_async()
    gpu.cuda.synchronize()
    isw = items._get_sweeper()
    assert call(c=C.byref(isw.c)) == -1 and "segmenter's corpus" in L.segk_last_error().decode()
    gpu.cuda.synchronize()
    assert gpu.equal(sws.slot, slots)                          # nothing was launched
    seg._df.check_status()


def test_replay_on_settled_slots_of_thousands_of_tokens(gpu, monkeypatch):
    """segk_fbt_assign_diag32 where a float32 term's rounding is multiplied by a slot's count: a32.SETTLED as
    utterances of one landmark, one float32 inner sweep on the device, replayed on the specification block by block on
    f32.PROBES tokens a block: the contract on the occupied slots, the prior predictive at 1e-9 on the empty ones, every probed
    token's slot the draw on the device's OWN row, the device's slots taken over, the partial sums at 1e-13.  First the
    tokens must show that they can tell the compensated term from the plain one: the emulation without the compensation
    misses the contract by 2 x or more on them."""
    f32 = a32.f32
    monkeypatch.setenv("SEGK_AM32_TILE_MIN", a32.TILES)
    case = f32.SETTLED[a32.SETTLED]
    N, K = case[6], case[3]
    spec = f32.spec_of(case)
    f32.discriminates(spec, a32.SETTLED)           # (first, on the settled start; once more below on the replayed state)
    seg = f32.segmenter_of(case, sync="sequential", score_precision="f64")
    sw = seg._get_sweeper()
    assert sw.score_precision == "f64" and seg._df.corpus.N_max == 1
    sw.probe_ll = gpu.full((N, K), float("nan"), dtype=gpu.float64, device="cuda")
    seg._df._L = Spy(seg._df._L)
    sw.enter(seg._dev_bounds)
    before = frozen(seg)
    seg.am_batch_sweep_async(1.0, score_precision="f32")
    gpu.cuda.synchronize()
    seg._df.check_status()
    assert sw.sweep_index == 1
    for x, y, nm in zip(before, frozen(seg), ("boundaries", "new_tok", "n_new", "out_logprob")):
        assert x.tobytes() == y.tobytes(), nm
    assert taken(seg) == {"segk_fbt_assign_diag32": sw.B, "segk_fbb_assign_diag32": 0, "segk_fbt_assign": 0}
    got, slots = sw.probe_ll.cpu().numpy()[:, :K], sw.slot.cpu().numpy()
    assert np.isfinite(got).all()                            # every utterance holds its one token
    centre = f32.centre_of(spec.X)
    assert np.array_equal(sw._centre32.cpu().numpy(), centre)
    worst = worst_empty = emulated = plain = 0.0
    draws = skipped = 0
    for b in range(spec.B):
        d = spec.derive(*spec.stats_excluding(b))
        occ = d["active"]
        items = np.array(f32.considered(spec, b, True))
        rows = f32.probe_rows(items)
        want, e, e_new, e_old = f32.compare(spec, d, spec.X[rows], got[rows], centre)
        worst, emulated, plain = max(worst, e), max(emulated, e_new), max(plain, e_old)
        worst_empty = max(worst_empty, rel(got[rows][:, ~occ], want[:, ~occ]))
        pz = spec.prior_z(d, None, None, None)
        for i in rows:
            p, u = spec._probabilities(pz + got[i], 1.0), nb.u01(spec.seed, 0, int(i), 1 + 0)      # (N_max + t: one landmark, token 0)
            draws += 1
            if a32.margin(p, u) < a32.DRAW_MARGIN:
                skipped += 1
            else:
                assert slots[i] == nb.draw_chunked(p, u), (b, i)
        f32.apply_slots(spec, b, items, slots[items])          # the specification goes on from the device's slots
    print("%s as one-landmark utterances: worst likelihood error %.3g (occupied), %.3g (empty) on %d probes a block; the "
          "emulation %.3g, without the compensation %.3g; %d draws, %d skipped near an edge"
          % (a32.SETTLED, worst, worst_empty, f32.PROBES, emulated, plain, draws, skipped))
    assert plain >= f32.DISCRIMINATES * a32.CONTRACT               # (the inputs: or the tokens prove nothing)
    assert worst <= a32.CONTRACT and worst_empty <= 1e-9
    assert skipped <= a32.NEAR_EDGE * draws
    assert np.array_equal(slots, spec.slot)
    for b in range(spec.B):
        for s in range(spec.S):
            cnt, sx, sxx = sw.cell_partials(b, s)
            rc, rx, rxx = spec.P[s][b]
            assert np.array_equal(cnt, rc) and rel(sx, rx) <= 1e-13 and rel(sxx, rxx) <= 1e-13, (b, s)

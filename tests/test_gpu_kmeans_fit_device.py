"""
GPU tests of KMeans.fit on the device (KMeans.fit(..., on_device=True), segk_kmeans_fit_step,
SegmentalKMeansWordseg.segment(..., kmeans_sync="device")).  After EVERY iteration the state must equal, bit for bit, the old
item-by-item route on a twin object, the oracle's KMeans.fit and -- through them -- the specification
(tests/kmeans_fit_device.py, whose case list tests/test_kmeans_fit_device_cpu.py checks for the situations that can break the
kernels); sum_neg_sqrd_norm alone keeps the project's rtol=1e-10.
"""
import random

import numpy as np
import pytest

from tests import kmeans_fit_device as kf
from tests import kmeans_refit as kr
from tests.golden import cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _state(model):
    c = model.components
    return {"assignments": c.assignments, "K": c.K, "counts": c.counts, "mean_numerators": c.mean_numerators, "means": c.means,
            "random_means": np.asarray(c.random_means)}


def _assert_same(got, want, where, fields=kf.FIELDS):
    for f in fields:
        assert np.array_equal(got[f], want[f]), (where, f)
        if f == "means":
            assert got[f].dtype == want[f].dtype, where


def _run_case(case, dtype, consider_unassigned):
    from segmentalist_amd.kmeans import KMeans
    trace = kf.oracle_trace(case, dtype, consider_unassigned)
    new, old = kf.new_model(KMeans, case, dtype), kf.new_model(KMeans, case, dtype)
    _assert_same(_state(new), _state(old), "start", kf.FIELDS + ("random_means",))
    for it, want in enumerate(trace):
        r_new = new.fit(1, consider_unassigned=consider_unassigned, on_device=True)
        r_old = old.fit(1, consider_unassigned=consider_unassigned)
        print(case[0], dtype, it, "device", r_new["n_mean_updates"], r_new["components"], r_new["sum_neg_sqrd_norm"], "old",
              r_old["n_mean_updates"], r_old["components"], r_old["sum_neg_sqrd_norm"], "oracle", want["n_mean_updates"],
              want["components"], want["sum_neg_sqrd_norm"])
        assert sorted(r_new) == sorted(r_old) == ["components", "n_mean_updates", "sample_time", "sum_neg_sqrd_norm"]
        s_new = _state(new)
        _assert_same(s_new, _state(old), (it, "old route"), kf.FIELDS + ("random_means",))
        _assert_same(s_new, want, (it, "oracle"))
        for key in ("components", "n_mean_updates"):
            assert r_new[key] == r_old[key] == [want[key]], (it, key)
        assert np.isclose(r_new["sum_neg_sqrd_norm"][0], r_old["sum_neg_sqrd_norm"][0], rtol=1e-10, atol=0), it
        assert np.isclose(r_new["sum_neg_sqrd_norm"][0], want["sum_neg_sqrd_norm"], rtol=1e-10, atol=0), it
    return new, old


# ------------------------------------------------------------------ every case, after every iteration
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", kf.CASES, ids=kf.CASE_IDS)
def test_device_fit_equals_old_route_and_oracle(gpu, case, dtype):
    _run_case(case, dtype, True)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_unassigned_rows_are_left_out(gpu, dtype):
    case = kf.CASES[kf.CASE_IDS.index("holes")]
    new, _ = _run_case(case, dtype, False)
    _, a = kf.case_data(case, dtype)
    assert ((new.components.assignments == -1) == (a == -1)).all()


def test_whole_fit_stops_early_like_the_old_route(gpu):
    """fit(n) as one call: the same number of iterations (the early stop after an iteration without a move), the same records."""
    from segmentalist_amd.kmeans import KMeans
    case = kf.CASES[kf.CASE_IDS.index("d5")]
    new, old = kf.new_model(KMeans, case, "float32"), kf.new_model(KMeans, case, "float32")
    r_new, r_old = new.fit(50, on_device=True), old.fit(50)
    assert r_new["n_mean_updates"] == r_old["n_mean_updates"] and r_new["n_mean_updates"][-1] == 0
    assert 1 < len(r_new["n_mean_updates"]) < 50
    assert r_new["components"] == r_old["components"]
    assert len(r_new["sample_time"]) == len(r_new["n_mean_updates"])
    assert np.allclose(r_new["sum_neg_sqrd_norm"], r_old["sum_neg_sqrd_norm"], rtol=1e-10, atol=0)
    _assert_same(_state(new), _state(old), "end")


# ------------------------------------------------------------------ golden chains
@pytest.mark.parametrize("chain", cases.KMEANS_CHAINS, ids=[c[0] for c in cases.KMEANS_CHAINS])
@pytest.mark.parametrize("init", ["spread", "rand"])
def test_fit_after_the_golden_chain(gpu, golden, chain, init):
    """The reference chain of tests/test_gpu_kmeans.py (three sequential sweeps), then fit(3, consider_unassigned=False) on the
    device against the recorded assignments and n_mean_updates."""
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    g = golden("chains")
    name, n_utt, D, K, seed, ragged, N, nmax, dtype = chain
    corpus = cases.chain_corpus(n_utt, D, K, seed, ragged, N, nmax, dtype)
    random.seed(1)
    np.random.seed(1)
    seg = kaw.SegmentalKMeansWordseg(K, *corpus, n_slices_min=0, n_slices_max=nmax, p_boundary_init=0.5,
                                     init_am_assignments=init, wip=0)
    tag = "%s_%s" % (name, init)
    seg.segment(3)
    c = seg.acoustic_model.components
    assert np.array_equal(c.assignments, g[tag + "_assign"][2])
    recf = seg.acoustic_model.fit(3, consider_unassigned=False, on_device=True)
    assert np.array_equal(c.assignments, g[tag + "_fit_assign"])
    assert np.array_equal(recf["n_mean_updates"], g[tag + "_fit_n_mean_updates"])


# ------------------------------------------------------------------ through the segmenter
def _seg(shape, init, sync):
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    K, corpus, ckw = kr.new_pair_args(shape, init)
    random.seed(5); np.random.seed(5)
    kw = dict(sync="batch", n_stat_blocks=shape[5]) if sync == "batch" else {}
    return kaw.SegmentalKMeansWordseg(K, *corpus, **ckw, **kw)


def _seg_state(seg):
    c = seg.acoustic_model.components
    return dict(_state(seg.acoustic_model), boundaries=np.array(seg.utterances.boundaries, copy=True))


def _assert_state_dicts_equal(a, b, where, path=""):
    assert type(a) == type(b), (where, path)
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), (where, path)
        for k in a:
            _assert_state_dicts_equal(a[k], b[k], where, path + "/" + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), (where, path)
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_state_dicts_equal(x, y, where, path + "/" + str(i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), (where, path)
    elif hasattr(a, "cpu"):
        assert bool((a.cpu() == b.cpu()).all()), (where, path)
    else:
        assert a == b, (where, path)


@pytest.mark.parametrize("sync", ["sequential", "batch"])
@pytest.mark.parametrize("shape,init", [(kr.SHAPES[1], "rand"), (kr.SHAPES[2], "spread")], ids=["40x16x12-f32", "25x5x30-f64"])
def test_segment_with_device_fits_equals_the_old_route(gpu, shape, init, sync):
    """segment(2, n_iter_inbetween_kmeans=3, kmeans_sync="device") against kmeans_sync=None on a twin, sweep by sweep: the sweep
    AFTER a fit must agree bit for bit as well (what a fit has to invalidate), then the checkpoints."""
    new, old = _seg(shape, init, sync), _seg(shape, init, sync)
    F = kf.FIELDS + ("random_means", "boundaries")
    for it in range(2):
        random.seed(20 + it); r_new = new.segment(1, n_iter_inbetween_kmeans=3, kmeans_sync="device")
        random.seed(20 + it); r_old = old.segment(1, n_iter_inbetween_kmeans=3, kmeans_sync=None)
        for key in ("sum_neg_len_sqrd_norm", "components", "n_tokens"):
            assert r_new[key] == r_old[key], (it, key)
        assert np.allclose(r_new["sum_neg_sqrd_norm"], r_old["sum_neg_sqrd_norm"], rtol=1e-10, atol=0)
        _assert_same(_seg_state(new), _seg_state(old), it, F)
    # one more sweep without a fit behind it, and the one-call form on fresh twins
    random.seed(30); r_new = new.segment(1)
    random.seed(30); r_old = old.segment(1)
    assert r_new["sum_neg_len_sqrd_norm"] == r_old["sum_neg_len_sqrd_norm"]
    _assert_same(_seg_state(new), _seg_state(old), "sweep after the fits", F)
    _assert_state_dicts_equal(new.state_dict(), old.state_dict(), "state_dict")
    new, old = _seg(shape, init, sync), _seg(shape, init, sync)
    random.seed(40); r_new = new.segment(2, n_iter_inbetween_kmeans=3, kmeans_sync="device")
    random.seed(40); r_old = old.segment(2, n_iter_inbetween_kmeans=3)
    assert r_new["sum_neg_len_sqrd_norm"] == r_old["sum_neg_len_sqrd_norm"] and r_new["components"] == r_old["components"]
    _assert_same(_seg_state(new), _seg_state(old), "segment(2, 3)", F)
    assert new.kmeans_refit_records == []


def test_hinted_and_delta_sweeps_after_a_device_fit(gpu, monkeypatch):
    """Batch sweeps that take the hinted score path and its delta pass (forced at every size), with device fits in between:
    the fit leaves cand.k and the delta state as the old route does -- the sweeps after it agree bit for bit."""
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    monkeypatch.setenv("SEGK_SCORE_HINT", "1")
    corpus = make_corpus(300, 16, 40, seed=77, N=12, n_slices_max=5)
    segs = []
    for _ in range(2):
        random.seed(3); np.random.seed(3)
        segs.append(kaw.SegmentalKMeansWordseg(40, *corpus, n_slices_max=5, init_am_assignments="spread", sync="batch"))
    new, old = segs
    F = kf.FIELDS + ("boundaries",)
    for it, m in enumerate((0, 0, 0, 2, 0, 1, 0)):
        r_new = new.segment(1, n_iter_inbetween_kmeans=m, kmeans_sync="device")
        r_old = old.segment(1, n_iter_inbetween_kmeans=m)
        assert r_new["sum_neg_len_sqrd_norm"] == r_old["sum_neg_len_sqrd_norm"], it
        _assert_same(_seg_state(new), _seg_state(old), it, F)


def test_kmeans_sync_values(gpu):
    seg = _seg(kr.SHAPES[0], "spread", "sequential")
    with pytest.raises(AssertionError):
        seg.segment(1, n_iter_inbetween_kmeans=1, kmeans_sync="gpu")
    with pytest.raises(AssertionError):
        seg.segment(1, n_iter_inbetween_kmeans=1, kmeans_sync="batch")


def test_a_sharded_corpus_is_refused(gpu):
    """The device of a sharded segmenter holds a slice of the rows: fit refuses it with the existing message, on either
    route, before anything is launched."""
    from segmentalist_amd._abi import SegkError
    seg = _seg(kr.SHAPES[0], "spread", "batch")
    dk = seg._dk
    before = _seg_state(seg)
    dk.shard, dk.n_rows_global = (0, dk.corpus.n_emb), dk.corpus.n_emb + 7
    try:
        for kw in (dict(on_device=True), dict()):
            with pytest.raises(SegkError, match="construct it with shard_corpus=False"):
                seg.acoustic_model.fit(1, consider_unassigned=False, **kw)
        with pytest.raises(SegkError, match="construct it with shard_corpus=False"):
            dk.fit_step(False)
    finally:
        dk.shard, dk.n_rows_global = None, dk.corpus.n_emb
    _assert_same(_seg_state(seg), before, "untouched", kf.FIELDS + ("boundaries",))


# ------------------------------------------------------------------ launch discipline, counted
class _Counting(object):
    """The binding's library object with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def test_library_calls_do_not_depend_on_the_moves(gpu, monkeypatch):
    """An iteration on the device is a fixed list of library calls -- none per item, whatever moves -- and ONE device-to-host
    copy; the old route on the same data issues two calls per moved item."""
    from segmentalist_amd.kmeans import KMeans
    case = kf.CASES[kf.CASE_IDS.index("n1025")]
    trace = kf.oracle_trace(case, "float32")
    moved = [s["n_mean_updates"] for s in trace]
    assert moved[0] > 500 and moved[-1] < moved[0] // 4, moved
    model = kf.new_model(KMeans, case, "float32")
    dk = model.components.dev
    lib = _Counting(dk._L)
    monkeypatch.setattr(dk, "_L", lib)
    copies = {"cpu": 0, "item": 0}
    real_cpu, real_item = gpu.Tensor.cpu, gpu.Tensor.item

    def cpu(self, *a, **kw):
        copies["cpu"] += 1
        return real_cpu(self, *a, **kw)

    def item(self):
        copies["item"] += 1
        return real_item(self)

    per_iter = []
    for it in range(len(trace)):
        lib.calls.clear()
        monkeypatch.setattr(gpu.Tensor, "cpu", cpu)
        monkeypatch.setattr(gpu.Tensor, "item", item)
        copies.update(cpu=0, item=0)
        rec = model.fit(1, on_device=True)
        monkeypatch.setattr(gpu.Tensor, "cpu", real_cpu)
        monkeypatch.setattr(gpu.Tensor, "item", real_item)
        assert rec["n_mean_updates"] == [moved[it]]
        assert copies == {"cpu": 1, "item": 0}, (it, copies)
        per_iter.append(dict(lib.calls))
    for calls in per_iter:
        assert calls == per_iter[0], per_iter
        assert "segk_kmeans_add_item" not in calls and "segk_kmeans_del_item" not in calls
        assert calls.get("segk_kmeans_fit_step") == 1 and sum(calls.values()) <= 3, calls
    # the old route, counted the same way
    old = kf.new_model(KMeans, case, "float32")
    lib_old = _Counting(old.components.dev._L)
    monkeypatch.setattr(old.components.dev, "_L", lib_old)
    old.fit(1)
    assert lib_old.calls["segk_kmeans_add_item"] == lib_old.calls["segk_kmeans_del_item"] == moved[0]


def test_fit_step_refuses_bad_operands(gpu):
    import ctypes as C
    from segmentalist_amd import _abi
    from segmentalist_amd.kmeans import KMeans
    case = kf.CASES[kf.CASE_IDS.index("d5")]
    model = kf.new_model(KMeans, case, "float32")
    dk = model.components.dev
    L, ctx = _abi.lib(), _abi.ctx()
    n = dk.corpus.n_emb
    words = int(L.segk_kmeans_fit_scratch_words(n, n, dk.K_max))
    scratch = gpu.zeros(words, dtype=gpu.int32, device="cuda")
    record = gpu.zeros(8, dtype=gpu.float64, device="cuda")
    good = [ctx, dk._cp(), C.byref(dk.m), C.byref(dk.cand), 1, n, _abi.ptr(scratch), _abi.ptr(record), _abi.ptr(dk.status), _abi.stream()]
    before = _state(model)
    for pos, bad in ((5, 0), (5, n + 1), (5, n - 1), (6, None), (7, None), (8, None), (3, None), (0, None)):
        a = list(good)
        a[pos] = bad
        assert L.segk_kmeans_fit_step(*a) != 0, (pos, bad)
    gpu.cuda.synchronize()
    _assert_same(_state(model), before, "refused calls change nothing")
    # a bound below the number of rows with a label: reported, never written out of bounds
    a = list(good)
    a[4], a[5] = 0, 10
    assert L.segk_kmeans_fit_step(*a) == 0
    assert int(record.cpu().numpy()[5]) & 8

"""
SegmentalKMeansWordseg.decode and KMeans.predict on the device against the specification tests/kmeans_decode.py (which
tests/test_kmeans_decode_cpu.py holds against the serial witness and the reference's recorded values): every field bit for bit, on
a sequential model and on a live batch state; small held-out sets; the score path's filter switch; the read-only rule (a twin
that never decoded); the refusals.
"""
import random

import numpy as np
import pytest

from tests import kmeans_decode as kd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _same_model(seg, ref):
    c, r = seg.acoustic_model.components, ref.acoustic_model.components
    assert c.K == r.K and np.array_equal(seg._dk.means.cpu().numpy(), r.means)


@pytest.mark.parametrize("name", list(kd.CASES))
def test_every_field_equals_the_specification_serial_and_live_batch_state(gpu, name):
    held = kd.corpora(name)[1]
    seg = kd.product_fitted(name, "serial")
    _same_model(seg, kd.fitted(name, "serial"))
    got = seg.decode(*held)
    kd.assert_same(got, kd.decoded(name, "serial")[0], (name, "serial"))
    assert got.utterance_labels == sorted(held[0])
    assert got.transcript(0) == [int(k) for k in got.seg_label[got.seg_offsets[0]:got.seg_offsets[1]]]

    seg = kd.product_fitted(name, "batch")
    assert seg._dk.assign_stale is not None                      # the batch state is live: labels pending
    _same_model(seg, kd.fitted(name, "batch"))
    want = kd.decoded(name, "batch")[0]
    live = seg.decode(*held)
    kd.assert_same(live, want, (name, "batch, live"))
    assert seg._dk.assign_stale is not None                      # ... and still pending
    dev = seg.decode(*held, device_out=True)                     # a second call, nothing read back
    assert all(gpu.is_tensor(getattr(dev, k)) for k in dev._fields)
    kd.assert_same(dev.numpy(), want, (name, "batch, device_out"))
    seg._dk.ensure_state()
    assert seg._dk.assign_stale is None
    kd.assert_same(seg.decode(*held), want, (name, "batch, materialised"))


@pytest.mark.parametrize("n_held", [0, 1, 2])
def test_small_held_out_sets(gpu, n_held):
    name = "km_small"
    seg = kd.product_fitted(name, "serial")
    ref = kd.fitted(name, "serial")
    keys = sorted(kd.corpora(name)[1][0])[:n_held]
    held = tuple({k: d[k] for k in keys} for d in kd.corpora(name)[1])
    got = seg.decode(*held)
    if n_held == 0:
        assert got.utterance_labels == [] and got.boundaries.shape == (0, 0) and len(got.objective) == 0
        assert got.seg_offsets.tolist() == [0] and len(got.seg_row) == 0 and got.K == ref.acoustic_model.components.K
        assert seg.decode({}, {}, {}, {}, device_out=True).K == got.K
        return
    kw = kd.seg_kwargs(name)
    t = kd.Tables(held, kw["n_slices_min"], kw["n_slices_max"], kw["min_duration"])
    assert len(t.Xq) % 64 != 0
    c = ref.acoustic_model.components
    kd.assert_same(got, kd.decode_spec(c.means, c.K, t, kw["n_slices_max"], kw["wip"]), n_held)


@pytest.mark.parametrize("name", ["km_mid", "km_f64", "refit_K30"])
def test_predict_is_argmax_neg_sqrd_norm_i_row_by_row(gpu, name):
    seg = kd.product_fitted(name, "batch")
    c = kd.fitted(name, "batch").acoustic_model.components
    Xq = kd.decoded(name, "batch")[0].tables.Xq
    rows, score = seg.acoustic_model.predict(Xq, return_score=True)
    assert rows.dtype == np.int64 and score.dtype == Xq.dtype and len(Xq) % 64 != 0
    for i, x in enumerate(Xq):
        d = c.means - x
        nsn = -(d * d).sum(axis=1)
        assert rows[i] == int(np.argmax(nsn)) and score[i] == np.max(nsn), i
    assert np.array_equal(seg.acoustic_model.predict(Xq), rows)
    assert len(seg.acoustic_model.predict(Xq[:0])) == 0


def test_query_beyond_the_filter_switch(gpu):
    """segk_kmeans_score takes the one-product pre-filter from n > 384 rows per CU on (segk_kmeans_filter, DESIGN.md 4.6;
    float32, D % 4 == 0): the smallest such M, D = 8, K_max = 6, against NumPy bit for bit like the full-size parity tests."""
    seg = kd.product_fitted("km_small", "batch")
    c = kd.fitted("km_small", "batch").acoustic_model.components
    M = 384 * gpu.cuda.get_device_properties(0).multi_processor_count + 1
    rs = np.random.RandomState(3)
    Xq = rs.randn(M, 8)
    Xq = (Xq / np.linalg.norm(Xq, axis=1, keepdims=True)).astype(np.float32)
    Xq[::7] = kd.decoded("km_small", "batch")[0].tables.Xq[0]            # rows from the clusters among the noise
    rows, score = seg.acoustic_model.predict(Xq, return_score=True)
    want_r, want_s = kd.rows_and_scores(c.means, Xq)
    assert np.array_equal(rows, want_r) and np.array_equal(score, want_s)
    assert len(set(rows.tolist())) >= 3


def _snapshot(seg):
    dk = seg._dk
    names = ("means", "mean_numerators", "counts", "K", "tiles", "mnorm_max", "cand_k", "cand_s", "new_tok", "new_k", "n_new",
             "n_flag", "out_total", "status", "remap", "out_scalars")
    s = {k: getattr(dk, k).cpu().numpy().copy() for k in names}
    s["boundaries"] = seg._dev_bounds.cpu().numpy().copy()
    return s


WARM = 10


def _run(gpu, decode):
    """Fit km_mid in batch mode, two sweeps and WARM more (hinted from the third on); then -- with decode and predict calls in
    between when `decode` -- two more sweeps and a serial segment_i: the snapshots after every step, the delta statistics of
    the two sweeps, segment_i's value, the assignments."""
    name = "km_mid"
    held = kd.corpora(name)[1]
    Xq = kd.decoded(name, "batch")[0].tables.Xq
    seg = kd.product_fitted(name, "batch")
    for _ in range(WARM):                                        # hinted from the third sweep on; the chain comes to rest
        seg.batch_sweep_async()
    gpu.cuda.synchronize()
    snaps, stats = [_snapshot(seg)], []
    if decode:
        st, nst = random.getstate(), np.random.get_state()
        got = seg.decode(*held)
        rows = seg.acoustic_model.predict(Xq)
        seg.decode(*held, device_out=True)
        assert random.getstate() == st and all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), nst))
        assert len(rows) == len(Xq) and len(got.seg_row)
    snaps.append(_snapshot(seg))
    for _ in range(2):
        seg.batch_sweep_async()
        gpu.cuda.synchronize()
        snaps.append(_snapshot(seg))
        stats.append(seg._dk.delta_stats())
        if decode:
            seg.decode(*held)
            seg.acoustic_model.predict(Xq[:5])
    total = seg.segment_i(3)
    snaps.append(_snapshot(seg))
    return snaps, stats, total, seg.acoustic_model.components.assignments


@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
def test_a_twin_that_never_decoded(gpu, monkeypatch, graph):
    """The read-only rule: after decode and predict the model, `random` / `np.random` and the next sweeps -- the hinted one, the
    one after it in delta mode, a replayed graph -- and a serial segment_i are those of a twin that never decoded.  (The
    twins run one after the other: the score path's state belongs to the context they share.)"""
    monkeypatch.setenv("SEGK_SCORE_HINT", "1")                  # hints and the delta pass at this size
    monkeypatch.setenv("SEGK_SWEEP_GRAPH", "1" if graph else "0")
    want = _run(gpu, False)
    got = _run(gpu, True)
    steps = ("warm", "after decode", "next sweep", "the sweep after", "segment_i")
    for step, sa, sb in zip(steps, got[0], want[0]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k], equal_nan=True), (step, k)
    assert got[1] == want[1], (got[1], want[1])
    print("delta statistics of the two sweeps (mode, changed columns, packed tiles, skipped positions):", got[1])
    if not graph:
        assert got[1][0][0] == 1 and got[1][1][0] == 1           # the sweeps after a decode ran in delta mode
    assert got[2] == want[2] and np.array_equal(got[3], want[3])


def test_refusals(gpu):
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.synth import make_corpus
    name = "km_small"
    seg = kd.product_fitted(name, "serial")
    held = kd.corpora(name)[1]
    other_d = make_corpus(2, 5, 6, seed=1, ragged=True, n_slices_max=6, N_range=(3, 9))
    with pytest.raises(SegkError, match="D = 5"):
        seg.decode(*other_d)
    with pytest.raises(SegkError, match="D = 5"):
        seg.acoustic_model.predict(np.zeros((3, 5), np.float32))
    bad = tuple(dict(d) for d in held)
    k = sorted(bad[1])[-1]
    bad[1][k] = bad[1][k].copy()
    bad[1][k][0] = 10 ** 6
    with pytest.raises(SegkError, match="span id names row 1000000"):
        seg.decode(*bad)
    seg.n_slices_min = 2
    with pytest.raises(SegkError, match="n_slices_min must be 0 or 1"):
        seg.decode(*held)
    seg.n_slices_min = 0
    long = make_corpus(1, 8, 6, seed=12, N=200, ragged=False, n_slices_max=6)
    seg.n_slices_max = 0
    with pytest.raises(SegkError, match="LDS of a workgroup"):
        seg.decode(*long)
    seg.n_slices_max = 6
    dk = seg._dk
    comm, dk.batch_comm = dk.batch_comm, type("TwoRanks", (), {"world": 2, "rank": 0})()
    try:
        with pytest.raises(SegkError, match="one process only"):
            seg.decode(*held)
        with pytest.raises(SegkError, match="one process only"):
            seg.acoustic_model.predict(np.zeros((3, 8), np.float32))
    finally:
        dk.batch_comm = comm
    dk.shard, dk.n_rows_global = (0, dk.corpus.n_emb), 2 * dk.corpus.n_emb
    try:
        with pytest.raises(SegkError, match="not sharded"):
            seg.decode(*held)
        with pytest.raises(SegkError, match="not sharded"):
            seg.acoustic_model.predict(np.zeros((3, 8), np.float32))
    finally:
        dk.shard, dk.n_rows_global = None, dk.corpus.n_emb
    kd.assert_same(seg.decode(*held), kd.decoded(name, "serial")[0], "after the refusals")

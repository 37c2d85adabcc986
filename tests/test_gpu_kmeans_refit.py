"""
GPU tests of the batch refit of the segmental k-means (KMeansBatchSweeper.refit, kmeans_refit_async,
segment(..., kmeans_sync="batch")) against its executable specification tests/kmeans_refit.py: bit for bit in the
boundaries, assignments, K, counts, numerators and means after every step; the record metric sum_neg_sqrd_norm (another
summation order on the device) at the relative tolerance the other record comparisons of the k-means path use (1e-10).
tests/test_kmeans_refit_cpu.py checks, without a device, that the schedule used here reaches every kind of refit.
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests import kmeans_refit as kr
from tests.virtual_ranks import VirtualWorld

pytestmark = pytest.mark.gpu

FIELDS = ("boundaries", "assignments", "K", "counts", "mean_numerators", "means")
CASES = [(s, i) for s in kr.SHAPES for i in kr.INITS]
IDS = ["%dx%dx%d-%s" % (s[0], s[1], s[2], i) for s, i in CASES]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _device_seg(shape, init, **kw):
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    K, corpus, ckw = kr.new_pair_args(shape, init)
    random.seed(5); np.random.seed(5)
    return kaw.SegmentalKMeansWordseg(K, *corpus, sync="batch", n_stat_blocks=shape[5], **ckw, **kw)


def _oracle_seg(shape, init):
    from oracle import np_oracle as no
    K, corpus, ckw = kr.new_pair_args(shape, init)
    random.seed(5); np.random.seed(5)
    return no.SegmentalKMeansWordseg(K, *corpus, **ckw)


def _assert_state(seg, want, where):
    """`want`: a snapshot of the specification (kr.snapshot) or an oracle segmenter."""
    if not isinstance(want, dict):
        want = kr.snapshot(want)
    c = seg.acoustic_model.components
    got = {"boundaries": seg.utterances.boundaries, "assignments": c.assignments, "K": c.K, "counts": c.counts,
           "mean_numerators": c.mean_numerators, "means": c.means}
    for name in FIELDS:
        assert np.array_equal(got[name], want[name]), (where, name)


def _refit(seg):
    """One refit on the device -> (n_mean_updates, K, n_tokens, sum_neg_sqrd_norm)."""
    seg.kmeans_refit_async()
    return seg._kmeans_refit_record()


# ------------------------------------------------------------------ the specification, step by step
@pytest.mark.parametrize("shape,init", CASES, ids=IDS)
def test_refits_and_sweeps_bit_exact_vs_spec(gpu, shape, init):
    """A refit on the fresh segmenter (its token lists are derived from the initial segmentation), then three rounds of one
    sweep and two refits: components emptied, components founded through tokens that name an inactive row, refits that move
    nothing (tests/test_kmeans_refit_cpu.py asserts that the schedule has them)."""
    steps = kr.schedule_trace(shape, init)
    seg = _device_seg(shape, init)
    for it, s in enumerate(steps):
        if s["op"] == "refit":
            moved, K, n_tok, obj = _refit(seg)
            print(it, "refit", moved, K, n_tok, obj, "spec", s["n_mean_updates"], s["K"], s["n_tokens"], s["sum_neg_sqrd_norm"])
            assert (moved, K, n_tok) == (s["n_mean_updates"], s["K"], s["n_tokens"]), it
            assert np.isclose(obj, s["sum_neg_sqrd_norm"], rtol=1e-10, atol=0), it
        else:
            rec = seg.segment(1)
            assert rec["sum_neg_len_sqrd_norm"][0] == s["total"], it
            assert rec["n_tokens"][0] == s["n_tokens"], it
        _assert_state(seg, s, it)


# ------------------------------------------------------------------ the driver
@pytest.mark.parametrize("shape,init", [(kr.SHAPES[0], "spread"), (kr.SHAPES[1], "rand"), (kr.SHAPES[4], "spread")],
                         ids=["12x8x6", "40x16x12", "33x12x30"])
def test_segment_with_batch_refits_equals_the_specs_loop(gpu, shape, init):
    """segment(3, n_iter_inbetween_kmeans=2, kmeans_sync="batch"): after every sweep up to two refits, stopping after the first
    that moves nothing; the refits' records have KMeans.fit's keys."""
    from oracle import np_oracle as no
    n_blocks = shape[5]
    ref, seg = _oracle_seg(shape, init), _device_seg(shape, init)
    want_tot, want_fit = [], []
    for _ in range(3):
        want_tot.append(no.kmeans_batch_sweep(ref, n_blocks=n_blocks))
        want_fit.append(kr.kmeans_batch_fit(ref, 2, n_blocks))
    rec = seg.segment(3, n_iter_inbetween_kmeans=2, kmeans_sync="batch")
    assert sorted(rec) == ["components", "n_tokens", "sample_time", "sum_neg_len_sqrd_norm", "sum_neg_sqrd_norm"]
    assert rec["sum_neg_len_sqrd_norm"] == want_tot
    assert len(seg.kmeans_refit_records) == 3
    for got, want in zip(seg.kmeans_refit_records, want_fit):
        assert sorted(got) == ["components", "n_mean_updates", "sample_time", "sum_neg_sqrd_norm"]        # KMeans.fit's record
        assert got["n_mean_updates"] == want["n_mean_updates"]                                     # (the early stop included)
        assert got["components"] == want["components"]
        assert len(got["sample_time"]) == len(want["n_mean_updates"])
        assert np.allclose(got["sum_neg_sqrd_norm"], want["sum_neg_sqrd_norm"], rtol=1e-10, atol=0)
    _assert_state(seg, ref, "end")
    if shape == kr.SHAPES[0]:
        assert [len(w["n_mean_updates"]) for w in want_fit][-1] == 1      # this chain has settled: the loop stops after one refit


def test_kmeans_sync_routes(gpu):
    """kmeans_sync="batch" needs a batch object; None on a batch object still takes the serial route (KMeans.fit), whose result
    is the oracle's KMeans.fit after the same sweep, bit for bit."""
    from oracle import np_oracle as no
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    shape = kr.SHAPES[1]
    K, corpus, ckw = kr.new_pair_args(shape, "spread")
    random.seed(5); np.random.seed(5)
    seq = kaw.SegmentalKMeansWordseg(K, *corpus, **ckw)
    with pytest.raises(AssertionError):
        seq.segment(1, n_iter_inbetween_kmeans=1, kmeans_sync="batch")
    with pytest.raises(AssertionError):
        seq.kmeans_refit_async()
    ref, seg = _oracle_seg(shape, "spread"), _device_seg(shape, "spread")
    for it in range(2):
        no.kmeans_batch_sweep(ref, n_blocks=shape[5])
        want = ref.acoustic_model.fit(2, consider_unassigned=False)
        seg.segment(1, n_iter_inbetween_kmeans=2, kmeans_sync=None if it == 0 else "sequential")
        assert seg.kmeans_refit_records == []
        assert want["n_mean_updates"][0] > 0 or it > 0
        _assert_state(seg, ref, it)


# ------------------------------------------------------------------ operand images, hints, delta state
def test_operand_images_after_a_refit_equal_a_fresh_prepare(gpu):
    """As test_operand_images_after_a_batch_sweep_equal_a_fresh_prepare (tests/test_gpu_kmeans.py) at (300, 16, 40): the
    refit's finalize leaves both images as segk_kmeans_prepare + segk_kmeans_mark_duplicates build them from the same means."""
    from segmentalist_amd import _abi, kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    corpus = list(make_corpus(300, 16, 40, seed=77, N=12, n_slices_max=5))
    random.seed(3); np.random.seed(3)
    seg = kaw.SegmentalKMeansWordseg(40, *corpus, n_slices_max=5, init_am_assignments="spread", sync="batch")
    dk = seg._dk
    L, ctx = _abi.lib(), _abi.ctx()
    moved = []
    for it in range(4):
        if it:
            seg.batch_sweep_async()
        seg.kmeans_refit_async()
        gpu.cuda.synchronize()
        dk.check_status()
        moved.append(int(dk.refit_moved.item()))
        got32, got16 = dk.tiles.clone(), dk.tiles_b3.clone()
        dk.prepare()
        _abi.check(L.segk_kmeans_mark_duplicates(ctx, dk._cp(), C.byref(dk.m), None, _abi.stream()))
        gpu.cuda.synchronize()
        assert gpu.equal(got32.view(gpu.int32), dk.tiles.view(gpu.int32)), it
        a, b = got16.view(gpu.int32), dk.tiles_b3.view(gpu.int32)
        assert gpu.equal(a[:2], b[:2]), (it, a[:4].tolist(), b[:4].tolist())          # exponent, E_m
        assert gpu.equal(a[1024:], b[1024:]), it
    assert moved[0] > 0, moved


def _hint_chain(gpu, monkeypatch, hints):
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.device import KMeansBatchSweeper
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(300, 16, 40, seed=77, N=12, n_slices_max=5)
    monkeypatch.setenv("SEGK_SCORE_HINT", "1")          # the hinted path at every size (it starts at 384 rows per CU otherwise)
    if not hints:
        monkeypatch.setattr(KMeansBatchSweeper, "_use_hints", lambda self: False)
    random.seed(3); np.random.seed(3)
    seg = kaw.SegmentalKMeansWordseg(40, *corpus, n_slices_max=5, init_am_assignments="spread", sync="batch")
    states, stats = [], []
    for op in ["sweep"] * 6 + ["refit"] + ["sweep"] * 2:
        if op == "sweep":
            seg.batch_sweep_async()
        else:
            seg.kmeans_refit_async()
        gpu.cuda.synchronize()
        seg._dk.check_status()
        stats.append(seg._dk.delta_stats())
        dk = seg._dk
        states.append([t.cpu().numpy().copy() for t in (seg._dev_bounds, dk.new_k, dk.n_flag, dk.means, dk.mean_numerators,
                                                         dk.counts, dk.K)])
    c = seg.acoustic_model.components
    states.append([c.assignments.copy()])
    monkeypatch.undo()
    return states, stats


def test_hints_and_delta_state_across_a_refit(gpu, monkeypatch):
    """Six sweeps, a refit, two sweeps with the hinted score path forced on: the same bits as the chain without hints; the
    sweep after the refit does not take the delta pass (its state is dropped by the refit: mode 0, a full pass that makes a
    new base, or -1), the one after it may again."""
    with_hints, stats = _hint_chain(gpu, monkeypatch, True)
    without, _ = _hint_chain(gpu, monkeypatch, False)
    for it, (a, b) in enumerate(zip(with_hints, without)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (it, i)
    print("delta stats per step (mode, changed columns, packed tiles, skipped positions):", stats)
    assert any(s[0] == 1 for s in stats[3:6]), stats        # the chain in front of the refit did take delta passes
    assert stats[7][0] in (0, -1), stats
    assert stats[8][0] in (1, 0, -1), stats


# ------------------------------------------------------------------ mini-batches, ranks, larger banks
def test_refit_between_minibatch_sweeps(gpu):
    from oracle import np_oracle as no
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from tests.golden import cases
    n_utt, D, K, nmax, n_blocks, n_batches = 40, 16, 12, 6, 4, 2
    corpus = cases.chain_corpus(n_utt, D, K, 2000 + n_utt, True, 0, nmax, "float32")
    for init in kr.INITS:
        random.seed(5); np.random.seed(5)
        ref = no.SegmentalKMeansWordseg(K, *corpus, n_slices_max=nmax, init_am_assignments=init)
        random.seed(5); np.random.seed(5)
        seg = kaw.SegmentalKMeansWordseg(K, *corpus, n_slices_max=nmax, init_am_assignments=init, sync="batch",
                                         n_stat_blocks=n_blocks, n_batches=n_batches)
        totals = np.zeros(n_utt)
        for it, op in enumerate(["sweep", "refit", "sweep"]):
            if op == "sweep":
                want = no.kmeans_minibatch_sweep(ref, n_blocks, n_batches, totals)
                assert seg.segment(1)["sum_neg_len_sqrd_norm"][0] == want, it
            else:
                info = {}
                moved, K_, obj = kr.kmeans_batch_refit(ref, n_blocks, info)
                got = _refit(seg)
                assert got[:3] == (moved, K_, info["n_tokens"])
                assert np.isclose(got[3], obj, rtol=1e-10, atol=0)
            _assert_state(seg, ref, (init, it))


def _rank_run(shape, init, comm):
    seg = _device_seg(shape, init, process_group=comm)
    rec = seg.segment(3, n_iter_inbetween_kmeans=2, kmeans_sync="batch")
    c = seg.acoustic_model.components
    # every rank reads the collective attributes in the same order
    return dict(assignments=c.assignments.copy(), boundaries=seg.utterances.boundaries.copy(), means=c.means.copy(),
                mean_numerators=c.mean_numerators.copy(), counts=c.counts.copy(), K=c.K, totals=list(rec["sum_neg_len_sqrd_norm"]),
                moved=[r["n_mean_updates"] for r in seg.kmeans_refit_records],
                components=[r["components"] for r in seg.kmeans_refit_records], sharded=seg._dk.shard is not None)


@pytest.mark.parametrize("world", [2, 4])
def test_refits_on_several_ranks_equal_one_rank(gpu, world):
    """(64, 39, 40, 6) sharded over 2 and 4 ranks (threads behind the communicator interface, tests/virtual_ranks.py): every
    rank ends with the one-rank run's means, K and labels, and every rank stops its refits at the same step."""
    from segmentalist_amd.comm import SingleComm
    shape = kr.SHAPES[3]
    one = _rank_run(shape, "spread", SingleComm())
    ranks = VirtualWorld(world).run(lambda comm: _rank_run(shape, "spread", comm))
    assert sum(len(m) for m in one["moved"]) >= 4 and one["moved"][0][0] > 0
    for r in range(world):
        assert ranks[r]["sharded"] and not one["sharded"]
        for k in one:
            if k == "sharded":
                continue
            if isinstance(one[k], np.ndarray):
                assert np.array_equal(one[k], ranks[r][k]), (r, k)
            else:
                assert one[k] == ranks[r][k], (r, k, one[k], ranks[r][k])


@pytest.mark.parametrize("n_utt,D,K,n_blocks", [(150, 16, 2500, 8), (300, 16, 2049, 4)],
                         ids=["ranges_of_128_components", "first_bank_beyond_the_band_stage_2049"])
def test_refit_at_larger_banks_vs_spec(gpu, n_utt, D, K, n_blocks):
    """The corpora of test_batch_statistics_kernel_fallbacks_vs_spec with more than 2048 slots: many flagged tokens per block
    (the inactive rows are data points: every token near one founds a component) and the bank just beyond the band stage."""
    from oracle import np_oracle as no
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(n_utt, D, K, seed=4000 + n_utt, N=0, ragged=True, n_slices_max=6, N_range=(3, 9))
    random.seed(5); np.random.seed(5)
    ref = no.SegmentalKMeansWordseg(K, *corpus, n_slices_max=6, init_am_assignments="spread", p_boundary_init=0.5)
    random.seed(5); np.random.seed(5)
    seg = kaw.SegmentalKMeansWordseg(K, *corpus, n_slices_max=6, init_am_assignments="spread", p_boundary_init=0.5, sync="batch",
                                     n_stat_blocks=n_blocks, flag_cap=40000)
    want = no.kmeans_batch_sweep(ref, n_blocks=n_blocks)
    assert seg.segment(1)["sum_neg_len_sqrd_norm"][0] == want
    _assert_state(seg, ref, "sweep")
    info = {}
    moved, K_, obj = kr.kmeans_batch_refit(ref, n_blocks, info)
    got = _refit(seg)
    print("refit", got, "spec", moved, K_, info, obj)
    assert got[:3] == (moved, K_, info["n_tokens"])
    assert np.isclose(got[3], obj, rtol=1e-10, atol=0)
    _assert_state(seg, ref, "refit")


# ------------------------------------------------------------------ serial chain in between, checkpoints, the list kernel
def test_serial_step_between_a_refit_and_a_sweep(gpu):
    """sweep, refit, segment_i (the reference's sequential step: it needs and leaves `assignments`), refit -- whose token lists
    are rebuilt from the serial state --, sweep: the oracle's objects go through the same calls."""
    from oracle import np_oracle as no
    shape = kr.SHAPES[1]
    n_blocks = shape[5]
    ref, seg = _oracle_seg(shape, "rand"), _device_seg(shape, "rand")
    no.kmeans_batch_sweep(ref, n_blocks=n_blocks)
    seg.segment(1)
    for it, op in enumerate(["refit", "serial", "refit", "sweep", "serial", "sweep"]):
        if op == "refit":
            info = {}
            moved, K, _ = kr.kmeans_batch_refit(ref, n_blocks, info)
            assert _refit(seg)[:3] == (moved, K, info["n_tokens"]), it
        elif op == "serial":
            assert seg.segment_i(3) == ref.segment_i(3), it
        else:
            want = no.kmeans_batch_sweep(ref, n_blocks=n_blocks)
            assert seg.segment(1)["sum_neg_len_sqrd_norm"][0] == want, it
        _assert_state(seg, ref, (it, op))


def test_checkpoint_after_a_refit_continues_bit_for_bit(gpu):
    shape = kr.SHAPES[3]
    seg = _device_seg(shape, "spread")
    seg.segment(1)
    seg.kmeans_refit_async()
    sd = seg.state_dict()
    twin = _device_seg(shape, "rand")            # another initial state: everything must come from the checkpoint
    twin.load_state_dict(sd)
    for s in (seg, twin):
        s.kmeans_refit_async()
        s.segment(2, n_iter_inbetween_kmeans=1, kmeans_sync="batch")
    a, b = seg.acoustic_model.components, twin.acoustic_model.components
    assert np.array_equal(seg.utterances.boundaries, twin.utterances.boundaries)
    for name in ("assignments", "K", "counts", "mean_numerators", "means"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert [r["n_mean_updates"] for r in seg.kmeans_refit_records] == [r["n_mean_updates"] for r in twin.kmeans_refit_records]


def test_token_list_kernel_and_argument_checks(gpu):
    """segk_kmeans_refit_collect directly: the dense id list, each entry's slot and the count against the slot arrays (more
    than one chunk of 1 024 slots, a range that starts inside the corpus), the -1 tail, and the refusals."""
    from segmentalist_amd import _abi, kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    torch = gpu
    corpus = make_corpus(300, 16, 40, seed=77, N=12, n_slices_max=5)
    random.seed(3); np.random.seed(3)
    seg = kaw.SegmentalKMeansWordseg(40, *corpus, n_slices_max=5, init_am_assignments="spread", sync="batch")
    seg.segment(1)
    dk, L, ctx = seg._dk, _abi.lib(), _abi.ctx()
    N_max = dk.corpus.N_max
    new_tok, new_k = dk.new_tok.cpu().numpy(), dk.new_k.cpu().numpy()
    for lo, hi in ((0, 300), (37, 251), (5, 5)):
        n_slots = (hi - lo) * N_max
        live = np.flatnonzero(new_k[lo:hi].ravel() >= 0)
        n_list = min(len(live) + 100, n_slots)
        ids = torch.full((n_list + 8,), -7, dtype=torch.int32, device="cuda")
        slots = torch.full((n_list + 8,), -7, dtype=torch.int32, device="cuda")
        chunks = torch.zeros(int(L.segk_kmeans_refit_scratch_words(n_slots)), dtype=torch.int32, device="cuda")
        count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        _abi.check(L.segk_kmeans_refit_collect(ctx, dk._cp(), lo, hi, _abi.ptr(dk.new_tok), _abi.ptr(dk.new_k), _abi.ptr(chunks),
                                               _abi.ptr(ids), _abi.ptr(slots), n_list, _abi.ptr(count), _abi.ptr(dk.status),
                                               _abi.stream()))
        torch.cuda.synchronize()
        assert int(count.item()) == len(live)
        got_ids, got_slots = ids.cpu().numpy(), slots.cpu().numpy()
        assert np.array_equal(got_slots[:len(live)], live + lo * N_max)
        assert np.array_equal(got_ids[:len(live)], new_tok.ravel()[live + lo * N_max])
        assert (got_ids[len(live):n_list] == -1).all() and (got_ids[n_list:] == -7).all()
        assert (got_slots[len(live):n_list] == -1).all() and (got_slots[n_list:] == -7).all()
    dk.check_status()
    assert len(np.flatnonzero(new_k.ravel() >= 0)) > 1024 and new_k.size > 2048
    # refusals, before anything is launched
    ids = torch.zeros(16, dtype=torch.int32, device="cuda")
    args = [ctx, dk._cp(), 0, 300, _abi.ptr(dk.new_tok), _abi.ptr(dk.new_k), _abi.ptr(chunks), _abi.ptr(ids), None, 16,
            _abi.ptr(count), _abi.ptr(dk.status), _abi.stream()]
    for pos, bad in ((2, -1), (3, 301), (9, 300 * N_max + 1), (9, -1), (7, None), (10, None)):
        a = list(args)
        a[pos] = bad
        assert L.segk_kmeans_refit_collect(*a) != 0, (pos, bad)
        assert L.segk_last_error()
    assert L.segk_kmeans_hint_relabel(ctx, dk._cp(), C.byref(dk.m), C.byref(dk.cand), None, _abi.stream()) != 0
    assert L.segk_kmeans_refit_apply(ctx, dk._cp(), C.byref(dk.m), C.byref(dk.cand), 0, 301, _abi.ptr(dk.new_tok), _abi.ptr(dk.new_k),
                                     _abi.ptr(dk.n_flag), _abi.ptr(dk.refit_moved), _abi.ptr(dk.status), _abi.stream()) != 0
    torch.cuda.synchronize()
    dk.check_status()

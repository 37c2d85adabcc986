"""
GPU tests of segk_kmeans_batch_partials_keep (csrc/segk_stats.hip k_batch_sort_sum): a token list that stands from
one call to the next keeps its partial sum in the record; everything the call leaves is the same bit for bit.

Hand-made token lists through the C ABI -- after EVERY call the lists (koff2 and the sorted regions), counts and sums against
sequential numpy, and the kernel's counters (lists kept / summed again per (block, range)) against the NumPy restatement
tests/batch_keep.py, exactly -- and chains of whole sweeps against the same chain with SEGK_BATCH_KEEP=0 and against
oracle/np_oracle.py, with the counters of every call predicted from the lists the SEGK_BATCH_KEEP=0 chain built.
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests import batch_keep as bk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _seq_sum(rows):
    acc = np.zeros(rows.shape[1], np.float64)
    for r in rows:
        acc = acc + r.astype(np.float64)
    return acc


class _Stats(object):
    """n_utt x N_max token slots with hand-made token lists: the statistics launch of a batch sweep on them."""

    def __init__(self, torch, n_utt, N_max, D, K_max, K_act, n_blocks, seed=0, dtype=np.float32):
        from segmentalist_amd.device import DeviceCorpus, DeviceKMeans, Partition
        rng = np.random.RandomState(seed)
        n_emb = n_utt * N_max
        self.X = rng.randn(n_emb, D).astype(dtype)
        vec_ids = np.zeros((n_utt, N_max * (N_max + 1) // 2), np.int32)
        corpus = DeviceCorpus(self.X, vec_ids, np.ones(vec_ids.shape), np.full(n_utt, N_max, np.int32))
        self.dk = DeviceKMeans(corpus, K_max, np.full(n_emb, -1), rng.randn(K_max, D).astype(dtype))
        self.dk.K.fill_(K_act)
        self.part = Partition(n_utt, np.arange(n_utt + 1) * N_max, n_blocks=n_blocks)
        self.torch, self.N_max, self.K_max, self.K_act, self.D, self.n_blocks = torch, N_max, K_max, K_act, D, n_blocks
        self.bounds = [int(x) for x in self.part.local_bounds]
        self.new_sweeper()

    def new_sweeper(self):
        """the sweeper's buffers (sorted, koff, pack, keep) allocated afresh; the restatement starts over with them"""
        from segmentalist_amd.device import KMeansBatchSweeper
        self.sw = KMeansBatchSweeper(self.dk, self.part, flag_cap=64)
        self.model = bk.KeepModel(self.K_max, [(self.bounds[b + 1] - self.bounds[b]) * self.N_max for b in range(self.n_blocks)])

    def call(self, tok, lab):
        from segmentalist_amd import _abi
        from segmentalist_amd.device import check, ptr
        dk, sw, pt, torch = self.dk, self.sw, self.part, self.torch
        dk.new_tok.copy_(torch.from_numpy(tok.astype(np.int32)))
        dk.new_k.copy_(torch.from_numpy(lab.astype(np.int32)))
        check(dk._L.segk_kmeans_batch_partials_keep(dk._ctx, dk._cp(), C.byref(dk.m), ptr(sw.blk_lo), pt.nbl, ptr(dk.new_tok),
                                                    ptr(dk.new_k), ptr(dk.n_flag), ptr(dk.out_total), sw._sorted_ptr, ptr(sw.koff),
                                                    ptr(sw.pack), sw.cap, sw.flag_rows, ptr(dk.out_scalars), _abi.stream(),
                                                    ptr(sw.keep), sw.keep.numel()))
        torch.cuda.synchronize()

    def sums_counts(self):
        nbl, K, D = self.n_blocks, self.K_max, self.D
        pk = self.sw.pack.cpu().numpy()
        o = nbl * K * D
        return pk[:o].reshape(nbl, K, D), pk[o + nbl:o + nbl + nbl * K].view(np.int64).reshape(nbl, K)

    def check(self, tok, lab, keeping=True, fused=True, skip_sums=()):
        """the call's lists, counts and sums against numpy, its counters against the restatement -> the counters [nbl, NR, 2]"""
        lay = bk.layout(bk.token_lists(tok, lab, self.bounds, self.K_act), self.K_max)
        dev = bk.lists_from_device(self.sw.koff.cpu().numpy(), self.sw.sorted.cpu().numpy(), self.bounds, self.N_max, self.K_max)
        sums, cnts = self.sums_counts()
        for b in range(self.n_blocks):
            assert sorted(dev[b]) == sorted(lay[b]), b
            want_n = np.zeros(self.K_act, np.int64)
            for k, (off, rows) in lay[b].items():
                assert dev[b][k][0] == off and np.array_equal(dev[b][k][1], rows), (b, k)
                want_n[k] = len(rows)
                if (b, k) not in skip_sums:
                    assert np.array_equal(sums[b, k], _seq_sum(self.X[rows])), (b, k)
            assert np.array_equal(cnts[b, :self.K_act], want_n), b
            empty = np.nonzero(want_n == 0)[0]
            assert not sums[b, empty].any(), b                              # an empty list is always written: zeros
        got = bk.counters(self.sw.keep.cpu().numpy(), self.n_blocks, self.K_max)
        if fused:
            want = self.model.step(lay, keeping)
            assert np.array_equal(got, want), (got.sum(axis=(0, 1)), want.sum(axis=(0, 1)))
        else:
            self.model.step(lay, False)
            assert not got.any()
        return got


def _random_lists(rng, n_utt, N_max, K_act, fill=0.7):
    """half of the tokens on six components (long lists), half anywhere (K_max = 1000: lists of one or two tokens)"""
    wide = rng.randint(0, K_act, size=(n_utt, N_max))
    few = rng.randint(0, min(6, K_act), size=(n_utt, N_max))
    lab = np.where(rng.rand(n_utt, N_max) < 0.5, wide, few)
    return np.where(rng.rand(n_utt, N_max) < fill, lab, -1).astype(np.int64)


@pytest.mark.parametrize("K_max", [33, 64, 1000])
@pytest.mark.parametrize("D", [2, 100, 128])
def test_edits_between_calls_cost_exactly_the_lists_they_change(gpu, monkeypatch, D, K_max):
    """Eight blocks of 16 utterances x 16 slots (block 1 without a token), one call after every edit."""
    monkeypatch.delenv("SEGK_BATCH_KEEP", raising=False)
    n_utt, N_max, n_blocks = 128, 16, 8
    per = (n_utt // n_blocks) * N_max
    K_act = K_max - 3
    NR = bk.n_ranges(K_max)
    rng = np.random.RandomState(7 * D + K_max)
    lab = _random_lists(rng, n_utt, N_max, K_act).reshape(n_blocks, per)
    lab[1] = -1                                                           # a block with no tokens
    lab[4, :4] = [0, NR, -1, 0]                                           # block 4: components 0 and NR are neighbours in range 0; a free slot
    lab[6, 0] = -1
    tok = rng.permutation(n_utt * N_max).astype(np.int64).reshape(n_blocks, per)
    T = _Stats(gpu, n_utt, N_max, D, K_max, K_act, n_blocks, seed=D)
    shape = (n_utt, N_max)

    def call(**kw):
        T.call(tok.reshape(shape), lab.reshape(shape))
        return T.check(tok.reshape(shape), lab.reshape(shape), **kw).sum(axis=(0, 1))

    live = sum(len(np.unique(lab[b][lab[b] >= 0])) for b in range(n_blocks))
    assert call().tolist() == [0, live]                                   # the first call on a zeroed buffer
    assert call().tolist() == [live, 0]                                   # nothing changed: every list stands
    # a list keeps its length and exchanges one row (two lists of block 3 exchange a row each)
    i = int(np.nonzero(lab[3] >= 0)[0][0])
    j = int(np.nonzero((lab[3] >= 0) & (lab[3] != lab[3, i]))[0][0])
    tok[3, i], tok[3, j] = tok[3, j], tok[3, i]
    assert call().tolist() == [live - 2, 2]
    # a neighbour grows: component 0 of block 4 gets the free slot's token; NR behind it in the region moves and stands
    off_before = T.sw.koff.cpu().numpy().reshape(n_blocks, K_max, 2)[4, NR, 0]
    lab[4, 2] = 0
    assert call().tolist() == [live - 1, 1]
    assert T.sw.koff.cpu().numpy().reshape(n_blocks, K_max, 2)[4, NR, 0] == off_before + 1
    # a token moves between two blocks
    s = int(np.nonzero(lab[5] >= 0)[0][3])
    k = lab[5, s]
    n5, n6 = int((lab[5] == k).sum()), int((lab[6] == k).sum())
    lab[5, s], lab[6, 0], tok[6, 0] = -1, k, tok[5, s]
    live += (n6 == 0) - (n5 == 1)
    assert call().tolist() == [live - (n5 > 1) - 1, (n5 > 1) + 1]
    # a list becomes empty, and comes back
    ke = lab[3, i]
    gone = lab[3] == ke
    lab[3][gone] = -1
    assert call().tolist() == [live - 1, 0]
    lab[3][gone] = ke
    assert call().tolist() == [live - 1, 1]
    # keeping switched off for one call: nothing kept, nothing vouched for in the next one either
    monkeypatch.setenv("SEGK_BATCH_KEEP", "0")
    assert call(keeping=False).tolist() == [0, live]
    monkeypatch.delenv("SEGK_BATCH_KEEP")
    assert call().tolist() == [0, live]
    assert call().tolist() == [live, 0]
    # every token relabelled: fewer than half of the lists stand
    lab[:] = np.where(lab >= 0, rng.randint(0, K_act, size=lab.shape), -1)
    kept, again = call().tolist()
    assert kept < again


def test_a_kept_list_is_not_written_and_a_changed_one_is(gpu, monkeypatch):
    """The record's sums of two lists overwritten between two calls: the one that stands is left alone (the caller's record
    is the kernel's memory: this is what the invariant rests on), the one that changed is summed again."""
    monkeypatch.delenv("SEGK_BATCH_KEEP", raising=False)
    n_utt, N_max, n_blocks, D, K_max = 64, 16, 4, 100, 64
    rng = np.random.RandomState(11)
    lab = _random_lists(rng, n_utt, N_max, K_max - 3)
    tok = rng.permutation(n_utt * N_max).astype(np.int64).reshape(n_utt, N_max)
    T = _Stats(gpu, n_utt, N_max, D, K_max, K_max - 3, n_blocks, seed=3)
    T.call(tok, lab)
    T.check(tok, lab)
    ks = np.unique(lab[32:48][lab[32:48] >= 0])                            # block 2
    k_stands, k_changes = int(ks[0]), int(ks[1])
    u, s = [int(x[0]) for x in np.nonzero(lab[32:48] == k_changes)]
    tok[32 + u, s] = tok[0, 0]                                             # one row of k_changes exchanged
    pk = T.sw.pack[:n_blocks * K_max * D].view(n_blocks, K_max, D)        # (a view of the record's sums)
    pk[2, k_stands] = 12345.0
    pk[2, k_changes] = 12345.0
    T.call(tok, lab)
    T.check(tok, lab, skip_sums={(2, k_stands)})
    sums, _ = T.sums_counts()
    assert (sums[2, k_stands] == 12345.0).all()


def test_a_new_sweeper_keeps_nothing_in_its_first_call(gpu, monkeypatch):
    monkeypatch.delenv("SEGK_BATCH_KEEP", raising=False)
    n_utt, N_max, n_blocks, D, K_max = 48, 16, 3, 100, 64
    rng = np.random.RandomState(5)
    lab = _random_lists(rng, n_utt, N_max, K_max - 3)
    tok = rng.permutation(n_utt * N_max).astype(np.int64).reshape(n_utt, N_max)
    T = _Stats(gpu, n_utt, N_max, D, K_max, K_max - 3, n_blocks, seed=4)
    T.call(tok, lab)
    assert T.check(tok, lab)[:, :, 0].sum() == 0
    T.call(tok, lab)
    assert T.check(tok, lab)[:, :, 1].sum() == 0
    T.new_sweeper()                                                        # the buffers reallocated and zeroed together
    T.call(tok, lab)
    assert T.check(tok, lab)[:, :, 0].sum() == 0
    T.call(tok, lab)
    assert T.check(tok, lab)[:, :, 1].sum() == 0


def test_previous_lists_beyond_the_entries_held_in_lds(gpu, monkeypatch):
    """K_max = 33: two ranges; one block of 640 x 16 slots puts more than 4 096 tokens into each region.  In an unchanged
    second call the lists whose old place ends inside the first 4 096 entries stand, the others are summed again."""
    monkeypatch.delenv("SEGK_BATCH_KEEP", raising=False)
    n_utt, N_max, D, K_max = 640, 16, 2, 33
    rng = np.random.RandomState(9)
    lab = np.where(rng.rand(n_utt, N_max) < 0.92, rng.randint(0, 30, size=(n_utt, N_max)), -1).astype(np.int64)
    tok = rng.permutation(n_utt * N_max).astype(np.int64).reshape(n_utt, N_max)
    T = _Stats(gpu, n_utt, N_max, D, K_max, 30, 1, seed=6)
    T.call(tok, lab)
    T.check(tok, lab)
    T.call(tok, lab)
    got = T.check(tok, lab)
    assert (got[0, :, 0] > 0).all() and (got[0, :, 1] > 0).all() and got.sum() == 30
    lay = bk.layout(bk.token_lists(tok, lab, T.bounds, 30), K_max)[0]
    assert max(o + len(r) for o, r in lay.values()) > bk.KEEP_CAP


def test_two_models_on_one_context_keep_only_their_own_lists(gpu, monkeypatch):
    """Two corpora of equal shape with different rows, the same token lists, sweeping alternately: each sweeper has its own
    buffers; each call's sums are its own corpus's and each model's counters follow its own history."""
    monkeypatch.delenv("SEGK_BATCH_KEEP", raising=False)
    n_utt, N_max, n_blocks, D, K_max = 48, 16, 3, 100, 64
    rng = np.random.RandomState(21)
    lab = _random_lists(rng, n_utt, N_max, K_max - 3)
    tok = rng.permutation(n_utt * N_max).astype(np.int64).reshape(n_utt, N_max)
    A = _Stats(gpu, n_utt, N_max, D, K_max, K_max - 3, n_blocks, seed=1)
    B = _Stats(gpu, n_utt, N_max, D, K_max, K_max - 3, n_blocks, seed=2)
    assert not np.array_equal(A.X, B.X)
    A.call(tok, lab)
    assert A.check(tok, lab)[:, :, 0].sum() == 0
    B.call(tok, lab)
    assert B.check(tok, lab)[:, :, 0].sum() == 0                           # nothing of A's is B's
    lab2 = lab.copy()
    lab2[lab2 == 1] = 2
    A.call(tok, lab2)
    A.check(tok, lab2)
    B.call(tok, lab)
    assert B.check(tok, lab)[:, :, 1].sum() == 0
    A.call(tok, lab2)
    assert A.check(tok, lab2)[:, :, 1].sum() == 0


@pytest.mark.parametrize("D,dtype", [(8, np.float64), (5, np.float32)], ids=["float64", "odd_D"])
def test_the_unfused_path_keeps_nothing(gpu, monkeypatch, D, dtype):
    monkeypatch.delenv("SEGK_BATCH_KEEP", raising=False)
    n_utt, N_max, n_blocks, K_max = 48, 16, 3, 64
    rng = np.random.RandomState(31)
    lab = _random_lists(rng, n_utt, N_max, K_max - 3)
    tok = rng.permutation(n_utt * N_max).astype(np.int64).reshape(n_utt, N_max)
    T = _Stats(gpu, n_utt, N_max, D, K_max, K_max - 3, n_blocks, seed=8, dtype=dtype)
    for _ in range(3):
        T.call(tok, lab)
        T.check(tok, lab, fused=False)


# ====================================================================== whole chains
def _hook(sw, log):
    """every statistics call of the sweeper: what it left, cloned on the stream before the finalize launch"""
    orig = sw._enqueue_back

    def wrapped():
        log.append([t.clone() for t in (sw.koff, sw.sorted, sw.keep, sw.pack)])
        orig()
    sw._enqueue_back = wrapped


# (K_max = 1000 on a corpus this small: with "spread" every token founds a component of its own and no list ever changes;
# "rand" lets two thirds of them change hands over the first sweeps)
CHAINS = [(48, 2, 33, 1, 12, 1, 31, "spread"), (150, 100, 64, 3, 14, 1, 32, "spread"), (160, 128, 1000, 8, 12, 1, 33, "rand"),
          (96, 16, 64, 3, 12, 2, 34, "spread")]


@pytest.mark.parametrize("n_utt,D,K,n_blocks,sweeps,n_batches,seed,init", CHAINS,
                         ids=["D2_K33_one_block", "D100_K64_three_blocks_with_edits", "D128_K1000_eight_blocks", "minibatch"])
def test_chain_equals_the_chain_without_keeping_and_the_oracle(gpu, monkeypatch, n_utt, D, K, n_blocks, sweeps, n_batches, seed, init):
    """After every sweep of a fresh chain (components founded and emptied in the first sweeps, settled later): the record, the
    sorted regions, koff2, means, labels and the sweep record equal the SEGK_BATCH_KEEP=0 chain's bit for bit and the oracle's
    state; the counters of every call are the restatement's, fed with the lists the other chain built.  The second case also
    runs, between sweeps, what must NOT cost a kept list: prepare(), mark_duplicates, un-hinted sweeps and a refit."""
    from oracle import np_oracle as no
    from segmentalist_amd import _abi, kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    from tests import kmeans_refit as kr
    monkeypatch.delenv("SEGK_BATCH_KEEP", raising=False)
    corpus = make_corpus(n_utt, D, K, seed=seed, ragged=True, n_slices_max=5, N_range=(4, 12))
    kw = dict(n_slices_max=5, init_am_assignments=init)
    segs = []
    for _ in range(3):
        random.seed(5); np.random.seed(5)
        segs.append(no.SegmentalKMeansWordseg(K, *corpus, **kw) if not segs else
                    kaw.SegmentalKMeansWordseg(K, *corpus, sync="batch", n_stat_blocks=n_blocks, n_batches=n_batches, **kw))
    ref, A, B = segs
    logs = {}
    for name, seg in (("A", A), ("B", B)):
        logs[name] = []
        _hook(seg._get_sweeper(), logs[name])
    swA = A._get_sweeper()
    bounds = [int(x) for x in swA.part.local_bounds]
    N_max = A._dk.corpus.N_max
    model = bk.KeepModel(K, [(bounds[b + 1] - bounds[b]) * N_max for b in range(n_blocks)])
    totals = np.zeros(n_utt)
    done, halves, mixed = 0, set(), 0
    edits = n_batches == 1 and n_blocks == 3

    def both(fn):
        monkeypatch.setenv("SEGK_BATCH_KEEP", "0")
        rb = fn(B)
        monkeypatch.delenv("SEGK_BATCH_KEEP")
        ra = fn(A)
        gpu.cuda.synchronize()
        return ra, rb

    def compare_calls():
        nonlocal done, mixed
        assert len(logs["A"]) == len(logs["B"]) > done
        for ca, cb in zip(logs["A"][done:], logs["B"][done:]):
            koff_a, srt_a, keep_a, pack_a = [t.cpu().numpy() for t in ca]
            koff_b, srt_b, keep_b, pack_b = [t.cpu().numpy() for t in cb]
            assert np.array_equal(koff_a, koff_b) and np.array_equal(srt_a, srt_b)
            assert np.array_equal(pack_a.view(np.int64), pack_b.view(np.int64)), len(logs["A"])
            want = model.step(bk.lists_from_device(koff_b, srt_b, bounds, N_max, K))
            got = bk.counters(keep_a, n_blocks, K)
            assert np.array_equal(got, want), (done, got.sum(axis=(0, 1)), want.sum(axis=(0, 1)))
            assert bk.counters(keep_b, n_blocks, K)[:, :, 0].sum() == 0
            if want.sum() > 0:
                halves.add(bool(2 * want[:, :, 0].sum() > want.sum()))
                mixed += done >= 1 and want[:, :, 0].sum() > 0 and want[:, :, 1].sum() > 0
            done += 1
        for name in ("means", "new_k", "new_tok"):
            a, b = getattr(A._dk, name), getattr(B._dk, name)
            assert gpu.equal(a.view(gpu.int32) if a.dtype == gpu.float32 else a, b.view(gpu.int32) if b.dtype == gpu.float32 else b), name

    for it in range(sweeps):
        if edits and it == 7:
            for seg in (A, B):                          # the operand images rebuilt, the duplicates marked again, hints dropped
                seg._dk.prepare()
                _abi.check(_abi.lib().segk_kmeans_mark_duplicates(_abi.ctx(), seg._dk._cp(), C.byref(seg._dk.m), None, _abi.stream()))
                seg._get_sweeper()._sweeps_done = 0
        if edits and it == 10:
            kr.kmeans_batch_refit(ref, n_blocks=n_blocks)
            both(lambda s: (s.kmeans_refit_async(), s._kmeans_refit_record())[1])
            compare_calls()
        random.seed(100 + it)
        want = no.kmeans_batch_sweep(ref, n_blocks=n_blocks) if n_batches == 1 else no.kmeans_minibatch_sweep(ref, n_blocks, n_batches, totals)

        def sweep(s):
            random.seed(100 + it)
            return s.segment(1)
        ra, rb = both(sweep)
        compare_calls()
        assert ra["sum_neg_len_sqrd_norm"][0] == rb["sum_neg_len_sqrd_norm"][0] == want, it
        assert ra["n_tokens"][0] == rb["n_tokens"][0] == ref.acoustic_model.get_n_assigned()
        cr, cd = ref.acoustic_model.components, A.acoustic_model.components
        assert np.array_equal(A.utterances.boundaries, ref.utterances.boundaries), it
        assert np.array_equal(cd.assignments, cr.assignments) and cd.K == cr.K, it
        assert np.array_equal(cd.mean_numerators, cr.mean_numerators) and np.array_equal(cd.means, cr.means), it
    # both arms: a call in which more than half of the non-empty lists stand and one in which fewer than half do (at K_max = 1000
    # that is the first call only: most lists there are single tokens that never move), and after the first call at least two
    # calls that keep some lists and sum others again
    assert halves == {True, False} and mixed >= 2, (halves, mixed)

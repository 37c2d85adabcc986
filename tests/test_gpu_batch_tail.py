"""
GPU tests of the batch sweep's tail -- k_kmeans_segment_w8x2 (two utterances per wave), k_batch_sort_sum, k_batch_finalize's
scalar and k_batch_post's relabel part -- each through the C ABI on hand-made inputs, at the shapes where they can go wrong:
an odd utterance count, the two halves of a wave with different lengths, blocked span ends in one half only, per-component
lists around the summing phase's batches of 16, 32 and 64 rows, a slot count that is no multiple of a workgroup.

References: oracle/c_oracle.py (A5 build_vec, A8 fb_kmeans_viterbi) and oracle/np_oracle.py (tree_sum, KMeansComponents'
clean_components), plus plain numpy sequential float64 sums.  Everything is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()          # raises if libsegk.so is missing or the device is not gfx950
    return torch


def _tri(N):
    return N * (N + 1) // 2


def _band(vec_ids, durations, N_max, W):
    """utterances.py band_tables: entry [i, t - 1, w] = the span [t - 1 - w, t)."""
    t = np.arange(1, N_max + 1)[:, None]
    w = np.arange(W)[None, :]
    s = t - 1 - w
    ok = s >= 0
    j = np.where(ok, t * (t - 1) // 2 + s, 0)
    ids = np.where(ok[None], vec_ids[:, j], -1).astype(np.int32)
    dur = np.where(ok[None], durations[:, j], np.nan)
    return np.ascontiguousarray(ids), np.ascontiguousarray(dur)


# ====================================================================== segment (two utterances per wave)
WIP = -0.2
K_MAX_SEG, K_ACT_SEG = 12, 9        # labels 9..11 are "at or above the active count": their tokens are flagged


def _segment_corpus(n_utt, N_cap, seed, blocked=()):
    """Ragged utterances of 1..N_cap landmarks (N = 1 and N = N_cap side by side in the first wave), every span of at most ten
    slices an embedding of its own, random durations; `blocked`: (utterance, kind) with kind "nan_last" (every span ending at
    N has a NaN duration: the backward pass starts blocked), "no_id_mid" (no span ends at N // 2: gamma there is -inf),
    "all_nan" (nothing is finite: the python vec[-1] path)."""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, N_cap + 1, size=n_utt).astype(np.int32)
    if n_utt >= 2:
        lengths[0], lengths[1] = 1, N_cap
    else:
        lengths[0] = N_cap - 13
    if n_utt >= 3:
        lengths[2] = 5
    for u, _ in blocked:
        lengths[u] = max(int(lengths[u]), 9)
    N_max = int(lengths.max())
    vec_ids = np.full((n_utt, _tri(N_max)), -1, dtype=np.int32)
    durations = np.full((n_utt, _tri(N_max)), np.nan)
    n_emb = 0
    for u in range(n_utt):
        for t in range(1, int(lengths[u]) + 1):
            for s in range(max(0, t - 10), t):
                vec_ids[u, t * (t - 1) // 2 + s] = n_emb
                durations[u, t * (t - 1) // 2 + s] = float(t - s) * (1.0 + 0.25 * rng.rand())
                n_emb += 1
    for u, kind in blocked:
        N = int(lengths[u])
        if kind == "nan_last":
            durations[u, _tri(N - 1):_tri(N)] = np.nan
        elif kind == "no_id_mid":
            t = N // 2
            vec_ids[u, _tri(t - 1):_tri(t)] = -1
        elif kind == "all_nan":
            durations[u, :] = np.nan
    cand_k = rng.randint(0, K_MAX_SEG, size=n_emb).astype(np.int32)
    cand_s = -rng.rand(n_emb) * 3.0
    bnd = np.zeros((n_utt, N_max), dtype=np.uint8)
    for u in range(n_utt):
        N = int(lengths[u])
        bnd[u, :N] = rng.rand(N) < 0.4
        bnd[u, N - 1] = 1
    X = rng.randn(n_emb, 4).astype(np.float32)
    return dict(lengths=lengths, N_max=N_max, vec_ids=vec_ids, durations=durations, cand_k=cand_k, cand_s=cand_s, bnd=bnd, X=X)


def _segment_expected(cp, nmax):
    """Per utterance: A5 + A8 of the C oracle, then the tokens of the new boundaries (kmeans_acoustic_wordseg.py:312-313) with
    the labels of the score stage; a span without an embedding or longer than the window is skipped and reported (status)."""
    from oracle import c_oracle
    n_utt, N_max = cp["bnd"].shape
    out = dict(bnd=np.zeros((n_utt, N_max), np.uint8), tok=[], k=np.full((n_utt, N_max), -1, np.int32), n_new=np.zeros(n_utt, np.int32),
               n_flag=np.zeros(n_utt, np.int32), total=np.zeros(n_utt), bad=False)
    for u in range(n_utt):
        N = int(cp["lengths"][u])
        W = nmax if 0 < nmax < N else N
        vids = cp["vec_ids"][u, :_tri(N)].astype(np.int64)
        score = np.where(vids >= 0, cp["cand_s"][np.maximum(vids, 0)], 0.0)
        vec = c_oracle.build_vec(vids, cp["durations"][u, :_tri(N)], score, 0, 1.0, WIP)
        tot, b, _ = c_oracle.fb_kmeans_viterbi(vec, N, 0, nmax)
        out["bnd"][u, :N] = b
        out["total"][u] = tot
        toks, jp = [], 0
        for j in range(N):
            if b[j]:
                t = j + 1
                e = int(vids[t * (t - 1) // 2 + jp])
                if t - 1 - jp >= W or e < 0:
                    out["bad"] = True
                else:
                    toks.append(e)
                jp = j + 1
        ks = cp["cand_k"][np.asarray(toks, dtype=np.int64)] if toks else np.zeros(0, np.int32)
        out["tok"].append(np.asarray(toks, np.int32))
        out["k"][u, :len(toks)] = ks
        out["n_new"][u] = len(toks)
        out["n_flag"][u] = int(np.count_nonzero(ks >= K_ACT_SEG))
    return out


def _run_segment(torch, cp, nmax, utts=None):
    from segmentalist_amd import _abi
    from segmentalist_amd.device import DeviceCorpus, DeviceKMeans, check, ptr, to_dev
    n_utt, N_max = cp["bnd"].shape
    band = _band(cp["vec_ids"], cp["durations"], N_max, nmax) if nmax < N_max else None
    corpus = DeviceCorpus(cp["X"], cp["vec_ids"], cp["durations"], cp["lengths"], band=band)
    assert corpus.N_max == N_max
    np.random.seed(1)
    dk = DeviceKMeans(corpus, K_MAX_SEG, np.full(cp["X"].shape[0], -1), cp["X"][:K_MAX_SEG].copy())
    dk.K.fill_(K_ACT_SEG)
    dk.cand_k.copy_(torch.from_numpy(cp["cand_k"]))
    dk.cand_s.copy_(torch.from_numpy(cp["cand_s"]))
    dk.status.zero_()
    dk.new_tok.fill_(-7)
    dk.new_k.fill_(-7)
    bnd = to_dev(cp["bnd"])
    if utts is None:
        dk.segment(bnd, 0, nmax, WIP, utt0=0, n_utts=n_utt)
    else:
        ul = to_dev(utts, np.int32)
        check(dk._L.segk_kmeans_segment(dk._ctx, dk._cp(), C.byref(dk.m), ptr(ul), 0, len(utts), 0, int(nmax), float(WIP),
                                        C.byref(dk.cand), ptr(bnd), ptr(dk.old_tok), ptr(dk.new_tok), ptr(dk.new_k), ptr(dk.n_old),
                                        ptr(dk.n_new), ptr(dk.n_flag), ptr(dk.out_total), ptr(dk.status), _abi.stream()))
    torch.cuda.synchronize()
    return dict(bnd=bnd.cpu().numpy(), tok=dk.new_tok.cpu().numpy(), k=dk.new_k.cpu().numpy(), n_new=dk.n_new.cpu().numpy(),
                n_flag=dk.n_flag.cpu().numpy(), total=dk.out_total.cpu().numpy(), status=int(dk.status[0].item()))


def _check_segment(got, want, utts=None):
    n_utt = want["bnd"].shape[0]
    sel = np.arange(n_utt) if utts is None else np.asarray(sorted(set(int(u) for u in utts)))
    assert np.array_equal(got["bnd"][sel], want["bnd"][sel])
    assert np.array_equal(got["n_new"][sel], want["n_new"][sel])
    assert np.array_equal(got["n_flag"][sel], want["n_flag"][sel])
    assert np.array_equal(got["k"][sel], want["k"][sel])
    for u in sel:
        assert np.array_equal(got["tok"][u, :want["n_new"][u]], want["tok"][u]), u
    assert np.array_equal(got["total"][sel].view(np.int64), want["total"][sel].view(np.int64))
    assert bool(got["status"] & 1) == want["bad"]


@pytest.mark.parametrize("nmax", [1, 6, 8])
@pytest.mark.parametrize("n_utt", [1, 2, 3, 257])
def test_segment_two_utterances_per_wave_vs_c_oracle(gpu, n_utt, nmax):
    """k_kmeans_segment_w8x2 (N_max <= 32) against the C oracle's A5 + A8: 1, 2, 3 and 257 utterances (the last wave of an odd
    count has one live half), lengths 1..32 with N = 1 beside N = 32 in the first wave, windows of 1, 6 and 8 slices (band
    tables where an utterance is longer than the window, the triangle where it is not)."""
    cp = _segment_corpus(n_utt, 32, 100 * n_utt + nmax)
    want = _segment_expected(cp, nmax)
    if n_utt == 257:
        # a label at or above the active count in one half of a wave only
        nf = want["n_flag"][:256].reshape(-1, 2)
        assert np.any((nf[:, 0] > 0) & (nf[:, 1] == 0)) and np.any((nf[:, 0] == 0) & (nf[:, 1] > 0))
    _check_segment(_run_segment(gpu, cp, nmax), want)


@pytest.mark.parametrize("half", [0, 1], ids=["low_half", "high_half"])
@pytest.mark.parametrize("nmax", [6, 8])
def test_segment_blocked_span_ends_in_one_half(gpu, half, nmax):
    """Utterances whose candidates are all -inf at some span end -- NaN durations at the last span end, no embedding at a
    middle one, nothing finite at all -- in the low halves of their waves only, then in the high halves only; their partners
    are ordinary utterances."""
    blocked = [(10 + half, "nan_last"), (20 + half, "no_id_mid"), (30 + half, "all_nan"), (2 + half, "nan_last")]
    cp = _segment_corpus(41, 32, 7 + half, blocked=blocked)
    want = _segment_expected(cp, nmax)
    assert want["bad"]
    _check_segment(_run_segment(gpu, cp, nmax), want)


def test_segment_utterance_list_in_reversed_order(gpu):
    """The `utts` index-list form, reversed and with a gap: other pairs share a wave than in the range form; utterances that
    are not on the list keep their boundaries."""
    cp = _segment_corpus(257, 32, 55)
    want = _segment_expected(cp, 6)
    utts = np.delete(np.arange(257)[::-1], [3, 100])
    got = _run_segment(gpu, cp, 6, utts=utts)
    _check_segment(got, want, utts=utts)
    for u in (256 - 3, 256 - 100):
        assert np.array_equal(got["bnd"][u], cp["bnd"][u])


def test_segment_33_landmarks_takes_the_one_utterance_kernel(gpu):
    """N_max = 33: the one-utterance-per-wave kernel as before, same results against the oracle."""
    cp = _segment_corpus(67, 33, 91, blocked=[(10, "nan_last"), (21, "no_id_mid")])
    assert cp["N_max"] == 33
    want = _segment_expected(cp, 6)
    _check_segment(_run_segment(gpu, cp, 6), want)


# ====================================================================== sums, finalize scalar, relabel
class _Tail(object):
    """A corpus of n_utt x N_max token slots with hand-made token lists: the statistics launches of a batch sweep on them."""

    def __init__(self, torch, n_utt, N_max, D, K_max, K_act, n_blocks, tok, lab, totals, seed=0):
        from segmentalist_amd.device import DeviceCorpus, DeviceKMeans, KMeansBatchSweeper, Partition
        rng = np.random.RandomState(seed)
        n_emb = n_utt * N_max
        self.X = rng.randn(n_emb, D).astype(np.float32)
        vec_ids = np.zeros((n_utt, _tri(N_max)), np.int32)
        corpus = DeviceCorpus(self.X, vec_ids, np.ones(vec_ids.shape), np.full(n_utt, N_max, np.int32))
        self.random_means = rng.randn(K_max, D).astype(np.float32)
        self.dk = dk = DeviceKMeans(corpus, K_max, np.full(n_emb, -1), self.random_means)
        dk.K.fill_(K_act)
        self.part = Partition(n_utt, np.arange(n_utt + 1) * N_max, n_blocks=n_blocks)
        self.sw = KMeansBatchSweeper(dk, self.part, flag_cap=64)
        dk.new_tok.copy_(torch.from_numpy(tok))
        dk.new_k.copy_(torch.from_numpy(lab))
        dk.n_new.copy_(torch.from_numpy((lab >= 0).sum(axis=1).astype(np.int32)))
        dk.out_total.copy_(torch.from_numpy(totals))
        self.torch, self.K_max, self.D, self.n_blocks, self.cap = torch, K_max, D, n_blocks, 64

    def partials(self):
        from segmentalist_amd import _abi
        from segmentalist_amd.device import check, ptr
        dk, sw, pt = self.dk, self.sw, self.part
        check(dk._L.segk_kmeans_batch_partials(dk._ctx, dk._cp(), C.byref(dk.m), ptr(sw.blk_lo), pt.nbl, ptr(dk.new_tok),
                                               ptr(dk.new_k), ptr(dk.n_flag), ptr(dk.out_total), sw._sorted_ptr, ptr(sw.koff),
                                               ptr(sw.pack), sw.cap, sw.flag_rows, ptr(dk.out_scalars), _abi.stream()))
        self.torch.cuda.synchronize()

    def record(self):
        """(sums [b, k, d], totals [b], counts [b, k], flag words [b, :]) of the packed record (segk.h)."""
        nbl, K, D = self.n_blocks, self.K_max, self.D
        pk = self.sw.pack.cpu().numpy()
        o = nbl * K * D
        fw = (2 + 3 * self.cap + 1) // 2
        return (pk[:o].reshape(nbl, K, D), pk[o:o + nbl], pk[o + nbl:o + nbl + nbl * K].view(np.int64).reshape(nbl, K),
                pk[o + nbl + nbl * K:o + nbl + nbl * K + nbl * fw].view(np.int32).reshape(nbl, 2 * fw))


def _seq_sum(rows):
    """strictly sequential float64 sum of the rows, in order"""
    acc = np.zeros(rows.shape[1], np.float64)
    for r in rows:
        acc = acc + r.astype(np.float64)
    return acc


def _n_ranges(K_max):
    need = (K_max + 31) // 32 if K_max <= 2048 else (K_max + 127) // 128
    nr = 1
    while nr < need:
        nr *= 2
    return nr


@pytest.mark.parametrize("K_max", [33, 64, 1000])
@pytest.mark.parametrize("D", [2, 100, 128])
def test_sort_sum_lists_sums_and_totals_vs_sequential_numpy(gpu, D, K_max):
    """k_batch_sort_sum on eight blocks of 16 utterances x 16 slots: block 0 holds components with 1, 15, 16, 17, 33 and 70
    tokens (lists below, at and across 16 and 32 rows -- the summing phase keeps 32 in flight -- and across its 64-row
    chunks), block 1 no token at all, block 2 every slot on one component, block 3 a few flagged tokens (labels at or above
    the active count), the rest random ragged lists.  Per (block, component): the token list (`koff2` and the sorted region)
    in token order, the count, the strictly sequential float64 sum; per block: the flag list and the sequential total."""
    n_utt, N_max, n_blocks = 128, 16, 8
    K_act = K_max - 3
    rng = np.random.RandomState(1000 * D + K_max)
    per = (n_utt // n_blocks) * N_max                                   # 256 slots per block
    lab = np.full((n_blocks, per), -1, np.int32)
    comps = [0, 5, 6, 17, 29, 8]
    b0 = np.concatenate([np.full(n, k, np.int32) for k, n in zip(comps, [1, 15, 16, 17, 33, 70])] + [np.full(30, 11, np.int32)])
    lab[0, :len(b0)] = rng.permutation(b0)
    lab[2, :] = 7
    for b in range(3, n_blocks):
        lab[b] = np.where(rng.rand(per) < 0.7, rng.randint(0, K_act, size=per), -1)
    lab[3, [5, 77, 78, 200]] = [K_act, K_max - 1, K_act, K_act + 1]
    lab = lab.reshape(n_utt, N_max)
    tok = rng.permutation(n_utt * N_max).astype(np.int32).reshape(n_utt, N_max)
    totals = -rng.rand(n_utt) * 50.0
    totals[16:32] = -rng.rand(16) * 1e-3                                  # (block 1: no token, its total is still summed)
    T = _Tail(gpu, n_utt, N_max, D, K_max, K_act, n_blocks, tok, lab, totals, seed=D)
    T.partials()
    sums, tots, cnts, flags = T.record()
    koff = T.sw.koff.cpu().numpy().reshape(n_blocks, K_max, 2)
    srt = T.sw.sorted.cpu().numpy()
    NR = _n_ranges(K_max)
    lab_b, tok_b = lab.reshape(n_blocks, per), tok.reshape(n_blocks, per)
    for b in range(n_blocks):
        acc = np.float64(0.0)
        for u in range(b * 16, b * 16 + 16):
            acc = acc + totals[u]
        assert tots[b] == acc, b
        for k in range(K_act):
            rows = tok_b[b][lab_b[b] == k]
            off, n = koff[b, k]
            assert n == len(rows) and cnts[b, k] == len(rows), (b, k)
            base = b * per * NR + (k & (NR - 1)) * per
            assert np.array_equal(srt[base + off:base + off + n], rows), (b, k)
            assert np.array_equal(sums[b, k], _seq_sum(T.X[rows])), (b, k)
        fl = np.nonzero(lab_b[b] >= K_act)[0]
        assert flags[b, 0] == len(fl)
        want = np.stack([b * per + fl, lab_b[b][fl], tok_b[b][fl]], axis=1).reshape(-1) if len(fl) else np.zeros(0, np.int64)
        assert np.array_equal(flags[b, 2:2 + 3 * len(fl)], want), b
    assert np.array_equal(cnts[1, :K_act], np.zeros(K_act, np.int64)) and cnts[2, 7] == per


def _finalize_case(torch, n_utt, N_max, n_blocks, seed):
    """Token lists that leave components 1, 4 and 6 of 20 empty: clean_components moves the last ones into the holes, so the
    relabel table is a non-trivial permutation.  Returns (new_k after the finalize launches, the oracle's labels per slot,
    out_scalars, the oracle's block totals)."""
    from oracle import np_oracle as no
    D, K_max, K_act = 8, 40, 20
    rng = np.random.RandomState(seed)
    live = np.asarray([k for k in range(K_act) if k not in (1, 4, 6)], np.int32)
    lab = np.where(rng.rand(n_utt, N_max) < 0.8, live[rng.randint(0, len(live), size=(n_utt, N_max))], -1).astype(np.int32)
    lab.reshape(-1)[:len(live)] = live                                   # every live component has a token
    tok = rng.permutation(n_utt * N_max).astype(np.int32).reshape(n_utt, N_max)
    totals = -rng.rand(n_utt) * 50.0
    T = _Tail(torch, n_utt, N_max, D, K_max, K_act, n_blocks, tok, lab, totals, seed=seed)
    T.partials()
    T.sw._enqueue_back()
    torch.cuda.synchronize()
    # the oracle's components with the same tokens: counts decide which components clean_components removes, and how
    np.random.seed(0)
    ref = no.KMeansComponents(T.X.astype(np.float64), np.full(T.X.shape[0], -1), K_max)
    ref.random_means = T.random_means.astype(np.float64)
    ref.K = K_act
    on = lab >= 0
    ref.assignments[tok[on]] = lab[on]
    ref.counts[:] = np.bincount(lab[on], minlength=K_max)
    ref.mean_numerators[:K_act] = 1.0                                     # (values are not compared here; they must divide)
    ref.clean_components()
    want = np.where(on, ref.assignments[tok], -1)
    bb = no.block_bounds(n_utt, n_blocks)
    blk = []
    for b in range(n_blocks):
        acc = np.float64(0.0)
        for u in range(bb[b], bb[b + 1]):
            acc = acc + totals[u]
        blk.append(acc)
    return T, lab, want, T.dk.out_scalars.cpu().numpy(), blk, ref


@pytest.mark.parametrize("n_blocks", [1, 3, 8, 9])
def test_finalize_total_is_the_oracles_tree_sum(gpu, n_blocks):
    """out_scalars[0] for 1, 3, 8 (the fixed register tree) and 9 blocks against np_oracle.tree_sum of the blocks' sequential
    totals; the relabelled tokens and the component count against the oracle's clean_components."""
    from oracle import np_oracle as no
    T, lab, want, scal, blk, ref = _finalize_case(gpu, 91, 7, n_blocks, 40 + n_blocks)
    assert scal[0] == no.tree_sum(blk)
    assert int(scal[1]) == ref.K == 17 and int(T.dk.K.item()) == 17
    assert int(scal[2]) == int(np.count_nonzero(lab >= 0))
    assert np.array_equal(T.dk.new_k.cpu().numpy(), want)
    assert np.array_equal(T.dk.counts.cpu().numpy(), ref.counts)


def test_post_relabels_every_slot(gpu):
    """k_batch_post's relabel part on 7 001 x 20 = 140 020 slots: more than the workgroups resident at once beside the tile
    workgroups take at one slot per thread, and no multiple of a workgroup's 256.  new_k must be remap[old] wherever old >= 0 and stay -1 elsewhere, with
    remap the oracle's relabelling (a non-trivial permutation: the last components moved into three holes)."""
    T, lab, want, scal, blk, ref = _finalize_case(gpu, 7001, 20, 8, 3)
    got = T.dk.new_k.cpu().numpy()
    remap = T.dk.remap.cpu().numpy()
    on = lab >= 0
    assert np.array_equal(got[~on], np.full(np.count_nonzero(~on), -1))
    assert np.array_equal(got[on], remap[lab[on]])
    assert np.array_equal(got, want)
    used = np.unique(lab[on])
    assert np.any(remap[used] != used) and len(np.unique(remap[used])) == len(used)
    from oracle import np_oracle as no
    assert scal[0] == no.tree_sum(blk)

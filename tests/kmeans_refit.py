"""
Executable specification of the batch refit of the segmental k-means: the reference's in-between Lloyd
iterations -- SegmentalKMeansWordseg.segment(n_iter, n_iter_inbetween_kmeans=m) runs acoustic_model.fit(m,
consider_unassigned=False) after every sweep (kmeans_acoustic_wordseg.py:353-426, kmeans.py:97-173) -- restated in the batch
mode's terms, on the oracle's objects (oracle/np_oracle.py) and from its primitives (block_bounds, tree_sum,
KMeansComponents).

A Lloyd iteration is deterministic given the frozen means, so a batch refit is no different sampler: it is `fit` with the
statistics summed in the batch sweep's fixed order.  The ONE departure from the reference's `fit` is the order of the additions:
`fit` deletes and re-adds only the moved items, in item (row) order, each addition replaying add_item's clamp against the K
of that moment; here ALL tokens are unassigned and re-added in token order (utterance, then segment), as kmeans_batch_sweep
does.  That changes which new label a founded component receives when several tokens name inactive rows in one iteration (and
the summation order of the statistics); with no founded component the assignments, K and counts are those of `fit`.
"""
import numpy as np

from oracle import np_oracle as no


def current_tokens(seg):
    """Per utterance, the embeddings of its current segments in segment order; entries of -1 (a segment of the initial
    segmentation without an embedding) are skipped."""
    u = seg.utterances
    return [[e for e in u.get_segmented_embeds_i(i) if e != -1] for i in range(u.D)]


def kmeans_batch_refit(seg, n_blocks=8, info=None):
    """One batch refit of an oracle SegmentalKMeansWordseg, in place -> (n_mean_updates, K, sum_neg_sqrd_norm).
    info (a dict, optional) receives what the tests' coverage checks need: the number of tokens that named an inactive row
    ("founding"), the number of components the refit emptied ("emptied") and the number of tokens ("n_tokens")."""
    u, c = seg.utterances, seg.acoustic_model.components
    tokens = current_tokens(seg)
    # new labels against the means as they stand: over all K_max rows, inactive random means included
    raw = [[int(np.argmax(c.neg_sqrd_norm(e))) for e in toks] for toks in tokens]
    n_mean_updates = sum(int(k != c.assignments[e]) for toks, ks in zip(tokens, raw) for e, k in zip(toks, ks))
    K_before = c.K
    # unassign all tokens, re-add them in token order with add_item's clamp replayed (assignment / K bookkeeping only)
    for toks in tokens:
        for e in toks:
            c.assignments[e] = -1
    K = c.K
    for toks, ks in zip(tokens, raw):
        for e, k in zip(toks, ks):
            if k > K:
                k = K
            if k == K:
                K += 1
            c.assignments[e] = k
    c.K = K
    # statistics from scratch in the fixed order of kmeans_batch_sweep (step 3)
    bb = no.block_bounds(u.D, n_blocks)
    part_sum, part_cnt = [], []
    for b in range(n_blocks):
        s = np.zeros((c.K_max, c.D), np.float64)
        n = np.zeros(c.K_max, np.int64)
        for i in range(bb[b], bb[b + 1]):
            for e in tokens[i]:
                k = c.assignments[e]
                s[k] += c.X[e]
                n[k] += 1
        part_sum.append(s)
        part_cnt.append(n)
    c.mean_numerators = no.tree_sum(part_sum)
    c.counts = no.tree_sum(part_cnt)
    for k in range(c.K):
        if c.counts[k] != 0:
            c.means[k] = c.mean_numerators[k] / c.counts[k]
    c.clean_components()
    if info is not None:
        info["founding"] = sum(int(k >= K_before) for ks in raw for k in ks)
        info["emptied"] = K - c.K
        info["n_tokens"] = sum(len(t) for t in tokens)
    return n_mean_updates, c.K, c.sum_neg_sqrd_norm()


SHAPES = [(12, 8, 6, 6, "float32", 8), (40, 16, 12, 6, "float32", 8), (25, 5, 30, 4, "float64", 4),
          (64, 39, 40, 6, "float32", 8), (33, 12, 30, 4, "float32", 2)]      # (n_utt, D, K, nmax, dtype, n_blocks)
INITS = ("spread", "rand")
_traces = {}


def new_pair_args(shape, init):
    """(am_K, corpus tuple, keyword arguments) both the oracle's and the product's constructor take for a test case; seed
    `random.seed(5); np.random.seed(5)` before either construction."""
    from tests.golden import cases
    n_utt, D, K, nmax, dtype, _ = shape
    corpus = cases.chain_corpus(n_utt, D, K, 1000 + n_utt, True, 0, nmax, dtype)
    return K, corpus, dict(n_slices_max=nmax, init_am_assignments=init)


def snapshot(seg):
    u, c = seg.utterances, seg.acoustic_model.components
    return {"boundaries": np.array(u.boundaries, copy=True), "assignments": np.array(c.assignments, copy=True), "K": int(c.K),
            "counts": np.array(c.counts, copy=True), "mean_numerators": np.array(c.mean_numerators, copy=True),
            "means": np.array(c.means, copy=True)}


def schedule_trace(shape, init, n_blocks=None):
    """The tests' schedule on the oracle -- a refit on the fresh segmenter, then three rounds of one kmeans_batch_sweep plus
    two refits -- as a list of steps: {"op": "refit" | "sweep", the state after the step (snapshot), and for a refit
    n_mean_updates, sum_neg_sqrd_norm, founding, emptied, n_tokens; for a sweep its total}.  Computed once per case and
    shared (read-only) by the tests that need it."""
    import random
    n_blocks = shape[5] if n_blocks is None else n_blocks
    key = (shape, init, n_blocks)
    if key not in _traces:
        K, corpus, kw = new_pair_args(shape, init)
        random.seed(5); np.random.seed(5)
        ref = no.SegmentalKMeansWordseg(K, *corpus, **kw)
        steps = []

        def refit():
            info = {}
            moved, _, obj = kmeans_batch_refit(ref, n_blocks, info)
            steps.append(dict(snapshot(ref), op="refit", n_mean_updates=moved, sum_neg_sqrd_norm=obj, **info))

        refit()
        for _ in range(3):
            total = no.kmeans_batch_sweep(ref, n_blocks=n_blocks)
            steps.append(dict(snapshot(ref), op="sweep", total=total, n_tokens=ref.acoustic_model.get_n_assigned()))
            refit()
            refit()
        _traces[key] = steps
    return _traces[key]


def kmeans_batch_fit(seg, n_iter, n_blocks=8):
    """Up to n_iter refits, stopping after the first that moves nothing, as KMeans.fit does -> fit's record keys."""
    rec = {"sum_neg_sqrd_norm": [], "components": [], "n_mean_updates": []}
    for _ in range(n_iter):
        moved, K, obj = kmeans_batch_refit(seg, n_blocks)
        rec["sum_neg_sqrd_norm"].append(obj)
        rec["components"].append(K)
        rec["n_mean_updates"].append(moved)
        if moved == 0:
            break
    return rec

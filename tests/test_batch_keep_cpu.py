"""
CPU tests of tests/batch_keep.py, the NumPy restatement behind tests/test_gpu_batch_keep.py: its token lists against the token
lists of oracle/np_oracle.py kmeans_batch_sweep (block by block, token order; their sequential sums combined by the oracle's tree
are the oracle's numerators bit for bit), and the keep decision on hand-made lists.
"""
import random

import numpy as np

from tests import batch_keep as bk
from tests.golden import cases


def _slots(ref):
    """slot arrays [n_utt, N_max] of an oracle segmenter's current tokens and their labels"""
    u, c = ref.utterances, ref.acoustic_model.components
    n_utt, N_max = u.D, int(max(u.lengths))
    tok = np.full((n_utt, N_max), -1, np.int64)
    lab = np.full((n_utt, N_max), -1, np.int64)
    for i in range(n_utt):
        e = [x for x in u.get_segmented_embeds_i(i) if x != -1]
        tok[i, :len(e)] = e
        lab[i, :len(e)] = [c.assignments[x] for x in e]
    return tok, lab


def test_token_lists_and_their_sums_are_the_oracles():
    from oracle import np_oracle as no
    n_utt, D, K, n_blocks = 40, 16, 12, 3
    corpus = cases.chain_corpus(n_utt, D, K, 1040, True, 0, 6, "float32")
    random.seed(5); np.random.seed(5)
    ref = no.SegmentalKMeansWordseg(K, *corpus, n_slices_max=6, init_am_assignments="spread")
    c = ref.acoustic_model.components
    bounds = no.block_bounds(n_utt, n_blocks)
    for it in range(3):
        no.kmeans_batch_sweep(ref, n_blocks=n_blocks)
        tok, lab = _slots(ref)
        lists = bk.token_lists(tok, lab, bounds, c.K)
        sums, cnts = [], []
        for b in range(n_blocks):
            # the oracle's own walk of block b: utterance, then segment
            want = {}
            for i in range(bounds[b], bounds[b + 1]):
                for e in ref.utterances.get_segmented_embeds_i(i):
                    if e != -1:
                        want.setdefault(int(c.assignments[e]), []).append(e)
            assert sorted(want) == sorted(lists[b])
            s, n = np.zeros((c.K_max, D)), np.zeros(c.K_max, np.int64)
            for k, rows in lists[b].items():
                assert list(rows) == want[k], (it, b, k)
                for e in rows:
                    s[k] += c.X[e]
                n[k] = len(rows)
            sums.append(s)
            cnts.append(n)
        assert np.array_equal(no.tree_sum(sums)[:c.K], c.mean_numerators[:c.K]), it
        assert np.array_equal(no.tree_sum(cnts)[:c.K], c.counts[:c.K]), it


def test_layout_puts_a_ranges_lists_member_after_member():
    K_max = 70                                   # three ranges needed -> four: component k in range k & 3 as member k >> 2
    assert bk.sort_shifts(K_max) == (5, 2) and bk.n_ranges(K_max) == 4
    assert bk.n_ranges(33) == 2 and bk.n_ranges(64) == 2 and bk.n_ranges(1000) == 32 and bk.n_ranges(2049) == 32
    lists = [{1: np.arange(3), 5: np.arange(10, 12), 9: np.arange(20, 24), 2: np.arange(7)}]
    lay = bk.layout(lists, K_max)[0]
    assert lay[1][0] == 0 and lay[5][0] == 3 and lay[9][0] == 5 and lay[2][0] == 0


def test_keep_decision():
    K_max = 33                                   # two ranges
    m = bk.KeepModel(K_max, [64], cap=16)
    a = {0: np.array([5, 6, 7]), 2: np.array([1, 2]), 4: np.array([9]), 1: np.array([3, 4])}
    lay = bk.layout([a], K_max)
    assert m.step(lay).tolist() == [[[0, 3], [0, 1]]]                      # the first call keeps nothing
    assert m.step(lay).tolist() == [[[3, 0], [1, 0]]]                      # nothing changed
    b = dict(a)
    b[2] = np.array([1, 8])                                                # same length, one row exchanged
    assert m.step(bk.layout([b], K_max)).tolist() == [[[2, 1], [1, 0]]]
    c = dict(b)
    c[0] = np.array([5, 6, 7, 11])                                         # a neighbour grows: 2 and 4 move, their rows stand
    lay_c = bk.layout([c], K_max)
    assert lay_c[0][2][0] == 4 and lay_c[0][4][0] == 6
    assert m.step(lay_c).tolist() == [[[2, 1], [1, 0]]]
    d = dict(c)
    del d[4]                                                               # a list becomes empty ...
    assert m.step(bk.layout([d], K_max)).tolist() == [[[2, 0], [1, 0]]]
    assert m.step(lay_c).tolist() == [[[2, 1], [1, 0]]]                    # ... and comes back: summed again
    assert m.step(lay_c, keeping=False).tolist() == [[[0, 3], [0, 1]]]     # keeping off: nothing kept, nothing vouched for
    assert m.step(lay_c).tolist() == [[[0, 3], [0, 1]]]
    e = dict(c)
    e[0] = np.arange(100, 114)                                             # 14 + 2 + 1 entries: the last list ends behind the cap of 16
    lay_e = bk.layout([e], K_max)
    m.step(lay_e)
    assert m.step(lay_e).tolist() == [[[2, 1], [1, 0]]]

"""
NumPy restatement of what segk_kmeans_batch_partials_keep keeps (csrc/segk_stats.hip k_batch_sort_sum).

The token lists per (statistics block, component) are a function of the slot arrays new_tok / new_k alone; a list's partial sum
is a function of its row ids alone.  Range workgroup (b, r) owns the components k with k & (NR - 1) == r, laid out one after the
other (member k >> nsh ascending) in its region.  A list is KEPT in a call iff the workgroup's header was valid (the previous
call on the same buffers ran with keeping on and the same shapes), the list is not empty, it has the length it had, its old
place ended inside the first min(S, KEEP_CAP) entries of the region, and its row ids are the old ones in order.  Its offset may
move.  Every other non-empty list is summed again.
"""
import numpy as np

KEEP_CAP = 4096
KEEP_HDR = 20
KEEP_REC = 32


def sort_shifts(K_max):
    """(rsh, nsh): log2 of the components per range (at most), log2 of the number of ranges"""
    rsh = 5 if K_max <= 2048 else 7
    need = (K_max + (1 << rsh) - 1) >> rsh
    nsh = 0
    while (1 << nsh) < need:
        nsh += 1
    return rsh, nsh


def n_ranges(K_max):
    return 1 << sort_shifts(K_max)[1]


def token_lists(tok, lab, bounds, K_act):
    """tok, lab: int [n_utt, N_max] slot arrays (lab < 0: unused slot); bounds: utterance bounds of the blocks.
    -> per block a dict k -> row ids of the block's tokens with label k < K_act, in token order (utterance, slot)."""
    out = []
    for b in range(len(bounds) - 1):
        t = np.asarray(tok[bounds[b]:bounds[b + 1]]).reshape(-1)
        l = np.asarray(lab[bounds[b]:bounds[b + 1]]).reshape(-1)
        d = {}
        for k in np.unique(l[(l >= 0) & (l < K_act)]):
            d[int(k)] = t[l == k].astype(np.int64)
        out.append(d)
    return out


def layout(lists, K_max):
    """per block: dict k -> (offset in the region of range k & (NR - 1), rows): the lists of a range lie member after member"""
    rsh, nsh = sort_shifts(K_max)
    NR = 1 << nsh
    out = []
    for d in lists:
        off = [0] * NR
        lay = {}
        for k in sorted(d, key=lambda k: (k & (NR - 1), k >> nsh)):
            r = k & (NR - 1)
            lay[k] = (off[r], d[k])
            off[r] += len(d[k])
        out.append(lay)
    return out


def lists_from_device(koff, srt, bounds, N_max, K_max):
    """The lists a call left in koff2 [nbl, K_max, 2] and the sorted regions (numpy copies) -> as layout()."""
    NR = n_ranges(K_max)
    koff = np.asarray(koff).reshape(len(bounds) - 1, K_max, 2)
    out = []
    for b in range(len(bounds) - 1):
        p0, S = bounds[b] * N_max, (bounds[b + 1] - bounds[b]) * N_max
        lay = {}
        for k in np.nonzero(koff[b, :, 1] > 0)[0]:
            o, n = koff[b, k]
            base = p0 * NR + (k & (NR - 1)) * S
            lay[int(k)] = (int(o), np.asarray(srt[base + o:base + o + n]).astype(np.int64))
        out.append(lay)
    return out


class KeepModel(object):
    """Feed it the laid-out lists of every call on one set of buffers; step() returns the counters the kernel leaves:
    int [nbl, NR, 2] = (lists kept, non-empty lists summed again) per (block, range)."""

    def __init__(self, K_max, slots_per_block, cap=KEEP_CAP):
        self.K_max, self.NR = K_max, n_ranges(K_max)
        self.slots = list(slots_per_block)
        self.cap = cap
        self.prev = None          # the previous call's layout
        self.valid = False        # ... and whether its headers vouch for the sums

    def step(self, lay, keeping=True):
        NR = self.NR
        cnt = np.zeros((len(lay), NR, 2), np.int64)
        for b, d in enumerate(lay):
            lim = min(self.slots[b], self.cap)
            for k, (off, rows) in d.items():
                if len(rows) == 0:
                    continue
                kept = False
                if keeping and self.valid and k in self.prev[b]:
                    po, pr = self.prev[b][k]
                    kept = len(pr) == len(rows) and po + len(pr) <= lim and np.array_equal(pr, rows)
                cnt[b, k & (NR - 1), 0 if kept else 1] += 1
        self.prev, self.valid = lay, bool(keeping)
        return cnt


def counters(keep_words, nbl, K_max):
    """the two counters per (block, range) out of the keep buffer (a numpy copy)"""
    return np.asarray(keep_words).reshape(nbl, n_ranges(K_max), KEEP_REC)[:, :, KEEP_HDR:KEEP_HDR + 2].astype(np.int64)

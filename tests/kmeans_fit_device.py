"""
Executable specification of KMeans.fit on the device (segmentalist_amd/csrc/segk_fit.hip): ONE Lloyd iteration of
the reference's fit (kmeans.py:97-173) restated as the steps the kernels take, on the oracle's objects (oracle/np_oracle.py).
Nothing here is a different algorithm: after every iteration the state must EQUAL what oracle KMeans.fit leaves
(tests/test_kmeans_fit_device_cpu.py), and the product must equal both (tests/test_gpu_kmeans_fit_device.py).

  items    rows 0..N-1, or the rows with a label, ascending                                   (k_fit_count_items, _collect_items)
  score    np.argmax of neg_sqrd_norm against the means as they stand                         (segk_kmeans_score)
  moves    (row, k_old, k_requested) of the items with k_requested != k_old, in item order    (k_fit_count_moves, k_fit_moves)
  clamp    add_item's clamp replayed over the moves with k_requested >= K, 64 per round       (k_fit_clamp)
  lists    operation 2j = delete of move j, 2j+1 = its add; stable counting sort by component (k_fit_hist, _scan_*, _place)
  apply    per component, its operations in order: float64 numerator -= / += X[i], the count  (k_fit_apply, k_fit_assign)
  clean    clean_components                                                                   (k_kmeans_clean_log, _relabel_log)
"""
import numpy as np

from oracle import np_oracle as no

WAVE = 64              # moves per round of the clamp replay
OPS_CHUNK = 512        # operations per workgroup of the counting sort (FIT_OPS)


def items_of(c, consider_unassigned):
    return np.arange(c.N) if consider_unassigned else np.flatnonzero(c.assignments != -1)


def move_list(c, items):
    """(rows, k_old, k_requested) of the moved items, in item order."""
    req = np.array([int(np.argmax(c.neg_sqrd_norm(i))) for i in items], dtype=np.int64).reshape(-1)
    old = c.assignments[items] if len(items) else np.zeros(0, np.int64)
    sel = req != old
    return np.asarray(items)[sel], old[sel].astype(np.int64), req[sel]


def clamp_serial(req, K, K_max):
    """add_item's clamp (kmeans_components.py:101-104) item by item -> (final labels, K, foundings, true clamps)."""
    fin = np.array(req, copy=True)
    founded = clamped = 0
    for j, k in enumerate(req):
        if k > K:
            k = K
            clamped += 1
        if k == K:
            K += 1
            founded += 1
        fin[j] = k
    assert K <= K_max
    return fin, K, founded, clamped


def clamp_rounds(req, K, K_max):
    """The same as k_fit_clamp takes it: 64 moves per round; inside a round the first lane still asking for a row >= K founds
    component K, the lanes in front of it keep their request -- one ballot per founding.  Once K == K_max nothing changes."""
    fin = np.array(req, copy=True)
    for h0 in range(0, len(req), WAVE):
        if K >= K_max:
            break
        lanes = np.asarray(req[h0:h0 + WAVE])
        first = 0
        while True:
            ask = np.flatnonzero(lanes[first:] >= K)
            if len(ask) == 0:
                break
            f = first + int(ask[0])
            fin[h0 + f] = K
            K += 1
            first = f + 1
    return fin, K


def ordered_lists(old, fin, K_max):
    """Stable counting sort of the 2 * moved operations by component, as the kernels do it: per chunk of OPS_CHUNK operations a
    histogram, per component the exclusive sum over the chunks, the components one behind the other, and inside a chunk the
    operation's rank among those of its component with a smaller number -> (operation numbers sorted, comp_off [K_max + 1]).
    The delete of an item without a label (k_old == -1) is no operation."""
    n_ops = 2 * len(old)
    keys = np.empty(n_ops, np.int64)
    keys[0::2] = old
    keys[1::2] = fin
    n_chunks = (n_ops + OPS_CHUNK - 1) // OPS_CHUNK
    hist = np.zeros((n_chunks, K_max), np.int64)
    for ch in range(n_chunks):
        kk = keys[ch * OPS_CHUNK:(ch + 1) * OPS_CHUNK]
        hist[ch] = np.bincount(kk[kk >= 0], minlength=K_max)
    tot = hist.sum(axis=0)
    base = np.cumsum(hist, axis=0) - hist
    comp_off = np.concatenate([[0], np.cumsum(tot)])
    out = np.full(int(comp_off[-1]), -1, np.int64)
    for ch in range(n_chunks):
        kk = keys[ch * OPS_CHUNK:(ch + 1) * OPS_CHUNK]
        for i, k in enumerate(kk):
            if k < 0:
                continue
            rank = int(np.count_nonzero(kk[:i] == k))
            out[comp_off[k] + base[ch, k] + rank] = ch * OPS_CHUNK + i
    assert (out >= 0).all()
    return out, comp_off


def apply_lists(c, rows, ops, comp_off, info=None):
    """Per component its operations in order, dev_del_item / dev_add_item's arithmetic; means[k] from the LAST operation that
    left the count non-zero (the reference rewrites it after every such operation)."""
    refilled = 0
    for k in range(c.K_max):
        lo, hi = int(comp_off[k]), int(comp_off[k + 1])
        if lo == hi:
            continue
        v = c.mean_numerators[k].copy()
        cnt = int(c.counts[k])
        last = None
        was_zero = False
        for o in ops[lo:hi]:
            x = c.X[rows[o >> 1]]
            if o & 1:
                v = v + x
                cnt += 1
                if was_zero:
                    refilled += 1
                    was_zero = False
            else:
                v = v - x
                cnt -= 1
                was_zero = was_zero or cnt == 0
            if cnt != 0:
                last = (v.copy(), cnt)
        c.mean_numerators[k] = v
        c.counts[k] = cnt
        if last is not None:
            c.means[k, :] = last[0] / last[1]
    if info is not None:
        info["refilled"] = refilled


def fit_step(c, consider_unassigned=True, info=None):
    """One iteration on an oracle KMeansComponents, in place -> (n_mean_updates, K, sum_neg_sqrd_norm).  info (a dict, optional)
    receives what the coverage checks of the tests need."""
    items = items_of(c, consider_unassigned)
    rows, old, req = move_list(c, items)
    K0 = c.K
    hi = np.flatnonzero(req >= K0)
    fin = req.copy()
    fin_hi, K, founded, clamped = clamp_serial(req[hi], K0, c.K_max)
    fin_rounds, K_rounds = clamp_rounds(req[hi], K0, c.K_max)
    assert K == K_rounds and np.array_equal(fin_hi, fin_rounds)
    fin[hi] = fin_hi
    ops, comp_off = ordered_lists(old, fin, c.K_max)
    apply_lists(c, rows, ops, comp_off, info)
    c.assignments[rows] = fin
    c.K = K
    empties = np.flatnonzero(c.counts[:c.K] == 0)
    c.clean_components()
    if info is not None:
        info.update(moved=len(rows), founded=founded, clamped=clamped, n_hi=len(hi), n_empty=len(empties),
                    empty_inside=bool(len(empties) and empties.min() < K - 1), n_items=len(items))
    return len(rows), c.K, c.sum_neg_sqrd_norm()


# --------------------------------------------------------------------------- the cases of both test files
# (name, N, D, K_max, clusters, init, seed, iterations): seeded Gaussian clusters; init "one" = every item in component 0,
# "rand" = KMeans' own, "holes" = "rand" with a third of the rows unassigned, "dup" = every row four times and four
# components to start with: inactive rows hold copies of the same item (argmax ties)
CASES = [
    ("one_start", 40, 3, 12, 9, "one", 3, 6),
    ("empties", 300, 7, 40, 6, "rand", 4, 6),
    ("big_bank", 3000, 16, 2500, 30, "rand", 5, 3),
    ("d5", 200, 5, 12, 6, "rand", 6, 4),
    ("d100", 200, 100, 12, 6, "rand", 7, 4),
    ("d300", 150, 300, 10, 5, "rand", 8, 4),
    ("n1025", 1025, 5, 20, 10, "rand", 9, 4),
    ("n2049", 2049, 5, 20, 10, "rand", 10, 4),
    ("long_chains", 5000, 8, 4, 4, "rand", 11, 4),
    ("ties", 256, 4, 64, 5, "dup", 12, 5),
    ("holes", 300, 6, 24, 8, "holes", 13, 12),
]
CASE_IDS = [c[0] for c in CASES]
_data, _traces = {}, {}


def case_data(case, dtype):
    """(X, initial assignments or "rand") of a case; computed once and shared read-only."""
    name, N, D, K_max, n_clusters, init, seed, _ = case
    key = (name, dtype)
    if key not in _data:
        rs = np.random.RandomState(seed)
        centres = rs.randn(n_clusters, D) * 4.0
        if init == "dup":
            base = centres[rs.randint(n_clusters, size=N // 4)] + rs.randn(N // 4, D) * 0.5
            X = np.tile(base, (4, 1))
        else:
            X = centres[rs.randint(n_clusters, size=N)] + rs.randn(N, D) * 0.5
        X = np.ascontiguousarray(X.astype(dtype))
        if init == "one":
            a = np.zeros(N, np.int64)
        elif init == "dup":
            a = rs.randint(0, 4, N)
        elif init == "holes":
            a = rs.randint(0, K_max, N)
            a[rs.rand(N) < 0.34] = -1
        else:
            a = "rand"
        _data[key] = (X, a)
    return _data[key]


def new_model(cls, case, dtype):
    """cls (the oracle's KMeans or the product's) on the case's data, with the seeds every twin of the case uses."""
    X, a = case_data(case, dtype)
    np.random.seed(case[6])
    return cls(X, case[3], a if isinstance(a, str) else a.copy())


def snapshot(c):
    return {"assignments": np.array(c.assignments, copy=True), "K": int(c.K), "counts": np.array(c.counts, copy=True),
            "mean_numerators": np.array(c.mean_numerators, copy=True), "means": np.array(c.means, copy=True)}


FIELDS = ("assignments", "K", "counts", "mean_numerators", "means")


def oracle_trace(case, dtype, consider_unassigned=True):
    """oracle KMeans.fit, one iteration at a time -> a list of {the state after the iteration, its record values}; stops
    after the iteration that moves nothing, as fit does.  Computed once per (case, dtype, flag)."""
    key = (case[0], dtype, consider_unassigned)
    if key not in _traces:
        ref = new_model(no.KMeans, case, dtype)
        steps = []
        for _ in range(case[7]):
            rec = ref.fit(1, consider_unassigned=consider_unassigned)
            steps.append(dict(snapshot(ref.components), n_mean_updates=rec["n_mean_updates"][0],
                              sum_neg_sqrd_norm=rec["sum_neg_sqrd_norm"][0], components=rec["components"][0]))
            if rec["n_mean_updates"][0] == 0:
                break
        _traces[key] = steps
    return _traces[key]

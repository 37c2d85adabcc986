#!/usr/bin/env python3
"""Time one hinted k-means score call (segk_kmeans_score_hinted) whose delta launch of K1 multiplies a forced number of packed
tiles -- 0, 1, 2, 4, 8, 16 (DIAG_TILES) -- for before/after figures.  Direct score calls as in tests/test_gpu_kmeans_delta.py: a
fresh base (the image exponent changes), then the first 32 (t - 1) + 1 means move, and the call that follows is timed with events.

    python tools/diag_k1_tiles.py [rows [D [K [repeats]]]]          (default: the headline's 1 050 000 x 100, K = 1 000, 5)

Prints per tile count the median, the minimum and the maximum call time in microseconds and the statistics of the timed call
(mode, changed columns, packed tiles, skipped positions).  Under rocprofv3 --kernel-trace the K1 launches can be read off by
their order.

DIAG_MOVED=m1,m2,... adds a second axis: how many of the moved means HAVE rows.  The tile count follows the changed columns of the
image, the hint waves' work the rows whose hinted mean moved (the live rows), and moving the first 32 (t - 1) + 1 means varies both
together.  With DIAG_MOVED the last 32 max(t) components get no rows (idle means: moving one changes a column and no row's
hint); a point (t, m), m <= 32, moves m of the first 32 means, m / (K - idle) of the rows live, and as many idle means as t packed
tiles need beyond them.  Without it the tool is what it was."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from segmentalist_amd.kmeans_components import KMeansComponents


def main():
    a = [int(v) for v in sys.argv[1:]]
    n, D, K, reps = (a + [1050000, 100, 1000, 5][len(a):])[:4]
    rs = np.random.RandomState(0)
    tiles = [int(t) for t in os.environ.get("DIAG_TILES", "0,1,2,4,8,16").split(",")]
    moved = [int(m) for m in os.environ["DIAG_MOVED"].split(",")] if os.environ.get("DIAG_MOVED") else None
    idle = 32 * max(tiles) if moved else 0                      # components without rows, the last ones
    assert moved is None or (max(moved) <= 32 and min(moved) >= 1 and 32 + idle < K), "DIAG_MOVED: 1 .. 32 means of tile 0"
    mu = rs.randn(K, D).astype(np.float32)
    X = mu[rs.randint(0, K - idle, n)] + np.float32(0.3) * rs.randn(n, D).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    means = mu / np.linalg.norm(mu, axis=1, keepdims=True)
    np.random.seed(0)
    c = KMeansComponents(X, np.zeros(n, dtype=int), K)
    d = c.dev
    ident = torch.arange(d.K_max, dtype=torch.int32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def write(m):
        d.means[:K].copy_(torch.from_numpy(np.ascontiguousarray(m)).to(d.means.device))
        d.prepare()

    def call(timed=False):
        if timed:
            ev[0].record()
        d.score_rows(hint_remap=ident)
        if timed:
            ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3 if timed else 0.0

    f = 4.0
    print("rows %d  D %d  K %d; microseconds per hinted call, median of %d" % (n, D, K, reps))
    for t, mv in [(t, m) for t in tiles for m in (moved if moved and t > 0 else [None])]:
        us = []
        for _ in range(reps):
            means = means * np.float32(f)
            f = 1.0 / f
            write(means)
            call(); call(); call()                              # the new base, then settled: every position skipped
            if t > 0:
                m = means.copy()
                if mv is None:
                    m[:32 * (t - 1) + 1] *= np.float32(1.01)
                else:
                    m[:mv] *= np.float32(1.01)
                    m[K - max(32 * (t - 1) + 1 - mv, 0):] *= np.float32(1.01)
                write(m)
            us.append(call(timed=True))
            stats = d.delta_stats()
        print("tiles %2d%s: median %7.1f  min %7.1f  max %7.1f   last call: %s" % (t, "" if mv is None else " moved %2d" % mv, float(np.median(us)), min(us), max(us), (stats,)))
    d.check_status()


if __name__ == "__main__":
    main()

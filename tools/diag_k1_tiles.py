#!/usr/bin/env python3
"""Time one hinted k-means score call (segk_kmeans_score_hinted) whose delta launch of K1 multiplies a forced number of packed
tiles -- 0, 1, 2, 4, 8, 16 (DIAG_TILES) -- for before/after figures.  Direct score calls as in tests/test_gpu_kmeans_delta.py: a
fresh base (the image exponent changes), then the first 32 (t - 1) + 1 means move, and the call that follows is timed with events.

    python tools/diag_k1_tiles.py [rows [D [K [repeats]]]]          (default: the headline's 1 050 000 x 100, K = 1 000, 5)

Prints per tile count the median, the minimum and the maximum call time in microseconds and the statistics of the timed call
(mode, changed columns, packed tiles, skipped positions).  Under rocprofv3 --kernel-trace the K1 launches can be read off by
their order."""
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
    mu = rs.randn(K, D).astype(np.float32)
    X = mu[rs.randint(0, K, n)] + np.float32(0.3) * rs.randn(n, D).astype(np.float32)
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

    tiles = [int(t) for t in os.environ.get("DIAG_TILES", "0,1,2,4,8,16").split(",")]
    f = 4.0
    print("rows %d  D %d  K %d; microseconds per hinted call, median of %d" % (n, D, K, reps))
    for t in tiles:
        us = []
        for _ in range(reps):
            means = means * np.float32(f)
            f = 1.0 / f
            write(means)
            call(); call(); call()                              # the new base, then settled: every position skipped
            if t > 0:
                m = means.copy()
                m[:32 * (t - 1) + 1] *= np.float32(1.01)
                write(m)
            us.append(call(timed=True))
            stats = d.delta_stats()
        print("tiles %2d: median %7.1f  min %7.1f  max %7.1f   last call: %s" % (t, float(np.median(us)), min(us), max(us), (stats,)))
    d.check_status()


if __name__ == "__main__":
    main()

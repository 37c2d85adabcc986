#!/usr/bin/env python3
"""FBGMM.set_K(K) in both forms -- development measurement, not bench.py; the table of profiles/README.md "FBGMM.set_K" comes
from it.

A fresh model per repetition (the call is a one-off): N rows, diagonal components, K_max slots all occupied with unequal sizes
(label k drawn with weight k + 1), cut to --k.  Per form the host wall time of set_K(K, sync=form) up to a device
synchronisation, the same with reassign=False (ranking, relabelling, rebuild of the bank -- and for "batch" the entry into
batch state), and for the batch form the orphan pass alone between two HIP events (FbgmmItemSweeper.reassign_orphans).
--form serial|batch|both; run one form under `rocprofv3 --kernel-trace --stats` for the kernel times."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def inputs(D, N, K_max, seed=0):
    from segmentalist_amd.niw import NIW
    rs = np.random.RandomState(seed)
    mu = 1.5 * rs.randn(max(2, K_max // 2), D)
    X = (mu[rs.randint(0, len(mu), N)] + 0.3 * rs.randn(N, D)).astype(np.float32)
    w = np.arange(1, K_max + 1, dtype=np.float64)
    assign = rs.choice(K_max, N, p=w / w.sum())
    assign[rs.choice(N, K_max, replace=False)] = np.arange(K_max)
    return X, assign, NIW(np.zeros(D), 0.05, D + 3, 0.1 * (D + 3) * np.ones(D))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=("serial", "batch", "both"), default="both")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=39)
    ap.add_argument("--k-max", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from segmentalist_amd.fbgmm import FBGMM
    torch.cuda.set_device(0)
    X, assign, prior = inputs(args.d, args.n, args.k_max)
    counts = np.bincount(assign, minlength=args.k_max)
    orphans = int(np.sort(counts)[:args.k_max - args.k].sum())
    print("set_K on %s: N %d, D %d, diag, K_max %d -> K %d, %d orphans, B x S %d x %d, %d repetitions" % (
        torch.cuda.get_device_name(0), args.n, args.d, args.k_max, args.k, orphans, args.blocks, args.slices, args.repeats), flush=True)

    def model():
        m = FBGMM(X, prior, 1.0, args.k_max, assign.copy(), covariance_type="diag", n_gibbs_blocks=args.blocks,
                  n_stat_blocks=args.slices)
        torch.cuda.synchronize()
        return m

    def wall(form, reassign):
        out = []
        for r in range(args.repeats + 1):              # (the first repetition warms the allocator and the kernels up)
            m = model()
            random.seed(1)
            t0 = time.perf_counter()
            m.set_K(args.k, reassign=reassign, sync="sequential" if form == "serial" else "batch")
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
            m.materialise()
            m.components.dev.check_status()
            assert m.components.K == args.k and m.get_n_assigned() == (args.n if reassign else args.n - orphans)
        return out[1:]

    for form in (("serial", "batch") if args.form == "both" else (args.form,)):
        full, cut = wall(form, True), wall(form, False)
        print("%-6s | set_K median %9.3f ms (%9.3f - %9.3f) | reassign=False %9.3f ms (%9.3f - %9.3f) | difference %9.3f ms"
              % (form, np.median(full), min(full), max(full), np.median(cut), min(cut), max(cut), np.median(full) - np.median(cut)),
              flush=True)
        if form == "batch":
            ms = []
            for r in range(args.repeats + 1):
                m = model()
                old = np.array(m.components.assignments)
                m.set_K(args.k, reassign=False, sync="batch")
                sw = m._get_sweeper()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                sw.reassign_orphans(old)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            ms = ms[1:]
            print("batch  | orphan pass alone (HIP events; %d x prepare, orphan list + tiles, partials) median %9.3f ms (%9.3f - %9.3f) | "
                  "%12.0f orphans/s" % (args.blocks, np.median(ms), min(ms), max(ms), orphans * 1e3 / np.median(ms)), flush=True)


if __name__ == "__main__":
    main()

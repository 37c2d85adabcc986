#!/usr/bin/env python3
"""Held-out labelling and scoring of the stand-alone mixture model (FBGMM.predict / score_samples / predict_log_proba) --
development measurement, not bench.py; the table of profiles/README.md "Held-out rows" comes from it.

Per shape a model of --n rows is built, --settle sampled batch sweeps leave it in a live batch state, and --m query rows that
are not in it (other draws from the same mixture, every 7th scaled by 3) are placed on the device.  Then, each timed with one
HIP event pair per call after --warmup calls:

  labels         FbgmmItemSweeper.predict(labels only, device_out=True): segk_fbb_prepare(-1), the prior rows of the query,
                 the tile kernel with the MAP half alone in its epilogue
  predict        labels and densities: the epilogue's logsumexp pass (an fp64 exp per row and slot) on top
  predict+resp   the same with the [M, K_max] log responsibilities (the kernel's stores and the column permutation)
  MAP sweep      batch_sweep_async(map_assign=True) on the same model afterwards: the sanity line -- a predict pass does the
                 likelihood half of a MAP sweep once, over as many rows, and no statistics

and the routes a checkout without FBGMM.predict has (code this tool's commit did not touch), on a throwaway model over
[X; Xq] with the queries at -1, built from the settled labels:

  log_marg_rows  dev.log_marg_rows over the --m appended rows (one launch of the serial model's score kernel and the copy of
                 the values to the host): the density
  map_assign_i   a loop of --loop calls of map_assign_i over the first appended rows (each adds its row to the model, one
                 launch and one host round trip per row), wall time; the figure for --m rows is EXTRAPOLATED from it

--routes picks among new, baseline; the baseline routes also run on an older checkout (--routes baseline)."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tools.bench_fbgmm_items import inputs, timed  # noqa: E402

# name -> (covariance_type, D, score_precision)
SHAPES = {"fixed_D39": ("fixed", 39, "f64"), "diag_D39": ("diag", 39, "f64"), "full_D39": ("full", 39, "f64"),
          "diag_D39_f32": ("diag", 39, "f32")}


def queries(cov, D, M, K_max, seed=0):
    """rows of the mixture of tools/bench_fbgmm_items.py `inputs` that are not its X"""
    mu = 1.5 * np.random.RandomState(seed).randn(max(2, K_max // 2), D)
    rs = np.random.RandomState(seed + 5000)
    Xq = mu[rs.randint(0, len(mu), M)] + 0.3 * rs.randn(M, D)
    Xq[::7] *= 3.0
    return Xq.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--routes", default="new,baseline")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--k-max", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=2)
    ap.add_argument("--loop", type=int, default=300)
    args = ap.parse_args()
    import torch
    from segmentalist_amd.fbgmm import FBGMM
    torch.cuda.set_device(0)
    routes = args.routes.split(",")
    print("held-out rows on %s: N %d, M %d, K_max %d, B x S %d x %d, %d calls after %d, %d sweeps to settle"
          % (torch.cuda.get_device_name(0), args.n, args.m, args.k_max, args.blocks, args.slices, args.calls, args.warmup, args.settle),
          flush=True)

    def line(name, route, ms, rows, note=""):
        med = float(np.median(ms))
        print("%-13s %-13s | median %10.3f ms (%10.3f - %10.3f) | %13.0f rows/s%s"
              % (name, route, med, min(ms), max(ms), rows * 1e3 / med, note), flush=True)
    for name in args.shapes.split(","):
        cov, D, prec = SHAPES[name]
        X, assign, prior = inputs(cov, D, args.n, args.k_max)
        Xq = queries(cov, D, args.m, args.k_max)
        random.seed(1)
        np.random.seed(1)
        kw = {"score_precision": prec} if prec != "f64" else {}
        m = FBGMM(X, prior, 1.0, args.k_max, assign, covariance_type=cov, n_gibbs_blocks=args.blocks, n_stat_blocks=args.slices, **kw)
        for _ in range(args.settle):
            m.batch_sweep_async()
        torch.cuda.synchronize()
        if "new" in routes:
            sw = m._get_sweeper()
            xq = torch.from_numpy(Xq).cuda()
            out = sw.predict(xq, True, True, False, device_out=True)
            n_new = int((out[0] == int((sw.cnt > 0).sum().item())).sum().item())
            line(name, "labels", timed(torch, lambda: sw.predict(xq, True, False, False, device_out=True), args.calls, args.warmup),
                 args.m)
            line(name, "predict", timed(torch, lambda: sw.predict(xq, True, True, False, device_out=True), args.calls, args.warmup),
                 args.m, "   (%d queries to an empty slot)" % n_new)
            line(name, "predict+resp", timed(torch, lambda: sw.predict(xq, True, True, True, device_out=True), args.calls, args.warmup),
                 args.m)
        labels = None
        if "baseline" in routes:
            m.materialise()
            labels = np.array(m.components.assignments)
        if "new" in routes:
            line(name, "MAP sweep", timed(torch, lambda: m.batch_sweep_async(map_assign=True), args.calls, args.warmup), args.n)
            m.components.dev.check_status()
        if "baseline" in routes:
            both = FBGMM(np.concatenate([X, Xq]), prior, 1.0, args.k_max, np.concatenate([labels, np.full(args.m, -1, np.int64)]),
                         covariance_type=cov)
            ids = np.arange(args.n, args.n + args.m)
            dev = both.components.dev
            ms = []
            for i in range(args.warmup + args.calls):
                torch.cuda.synchronize()
                t0 = time.time()
                dev.log_marg_rows(ids)
                if i >= args.warmup:
                    ms.append(1e3 * (time.time() - t0))
            line(name, "log_marg_rows", ms, args.m, "   (wall time, values on the host)")
            n_loop = min(args.loop, args.m)
            torch.cuda.synchronize()
            t0 = time.time()
            for r in range(n_loop):
                both.map_assign_i(args.n + r)
            torch.cuda.synchronize()
            wall = 1e3 * (time.time() - t0)
            dev.check_status()
            print("%-13s %-13s | %d calls in %.1f ms: %.1f us a row, %.0f rows/s | EXTRAPOLATED to %d rows: %.0f ms"
                  % (name, "map_assign_i", n_loop, wall, 1e3 * wall / n_loop, n_loop * 1e3 / wall, args.m, wall / n_loop * args.m),
                  flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Batch sweeps of the stand-alone mixture model (FBGMM.batch_sweep_async, the sweeps of gibbs_sample(sync="batch") without
the per-sweep materialise()) -- development measurement, not bench.py; the table of profiles/README.md "Stand-alone batch
sweeps" comes from it.

--route items      the new path: --sweeps calls of batch_sweep_async, one HIP event pair around each, after --warmup;
                   --score-precision f32 (diagonal shapes only) runs it with float32 item likelihoods
--route segmenter  the same rows as one-landmark utterances through UnigramAcousticWordseg.batch_sweep_async (the route that
                   existed before: span scores, boundaries and slots of one token per utterance), timed the same way
--route serial     FBGMM.gibbs_sample(sweeps), the serial chain over the items: the record's sample_time of every sweep (host
                   wall time: the sweep's uniforms, one kernel that walks the items, its synchronisation)
The segmenter and serial routes use nothing this tool's commit added, so the file also runs on an older checkout.
--settle N         N sampled batch sweeps before anything is timed (items and serial routes): a chain that has left its start
--map              the MAP sweeps of FBGMM.map_assign.  items: after the sampled sweeps are timed, --sweeps calls of
                   batch_sweep_async(map_assign=True) timed the same way in the same process (a second line, "items-MAP");
                   serial: map_assign(sweeps, sync="sequential") in place of gibbs_sample
Prints the median, the range and items/s per shape; --shapes picks from SHAPES by name."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

# name -> (covariance_type, D)
SHAPES = {"fixed_D39": ("fixed", 39), "fixed_D100": ("fixed", 100), "diag_D39": ("diag", 39), "diag_D100": ("diag", 100),
          "full_D39": ("full", 39)}


def inputs(cov, D, N, K_max, seed=0):
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    rs = np.random.RandomState(seed)
    mu = 1.5 * rs.randn(max(2, K_max // 2), D)
    X = (mu[rs.randint(0, len(mu), N)] + 0.3 * rs.randn(N, D)).astype(np.float32)
    assign = np.arange(N) % K_max
    rs.shuffle(assign)
    if cov == "fixed":
        prior = FixedVarPrior(0.1 * np.ones(D), np.zeros(D), 2.0 * np.ones(D))
    elif cov == "diag":
        prior = NIW(np.zeros(D), 0.05, D + 3, 0.1 * (D + 3) * np.ones(D))
    else:
        prior = NIW(np.zeros(D), 0.05, D + 3, 0.1 * (D + 3) * np.eye(D))
    return X, assign, prior


def timed(torch, fn, sweeps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(sweeps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]          # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("items", "segmenter", "serial"), default="items")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--k-max", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--score-precision", choices=("f64", "f32"), default="f64")
    ap.add_argument("--settle", type=int, default=0)
    ap.add_argument("--map", action="store_true")
    args = ap.parse_args()
    import torch
    from segmentalist_amd.fbgmm import FBGMM
    torch.cuda.set_device(0)
    if args.score_precision != "f64" and args.route != "items":
        ap.error("--score-precision applies to --route items")
    if (args.map or args.settle) and args.route == "segmenter":
        ap.error("--map and --settle apply to the items and serial routes")

    def line(name, route, ms, occupied):
        med = float(np.median(ms))
        print("%-10s %-9s | sweep median %9.3f ms (%9.3f - %9.3f) | %8.2f sweeps/s | %12.0f items/s | K = %d after the run"
              % (name, route, med, min(ms), max(ms), 1e3 / med, args.n * 1e3 / med, occupied), flush=True)
    print("route %s (%s) on %s: N %d, K_max %d, B x S %d x %d, %d sweeps after %d" % (
        args.route, args.score_precision, torch.cuda.get_device_name(0), args.n, args.k_max, args.blocks, args.slices, args.sweeps,
        args.warmup), flush=True)
    # (the keyword only where it is asked for: the fp64 routes of this file also run on a checkout without it)
    kw = {"score_precision": args.score_precision} if args.score_precision != "f64" else {}
    for name in args.shapes.split(","):
        cov, D = SHAPES[name]
        X, assign, prior = inputs(cov, D, args.n, args.k_max)
        random.seed(1)
        np.random.seed(1)
        if args.route == "items":
            m = FBGMM(X, prior, 1.0, args.k_max, assign, covariance_type=cov, n_gibbs_blocks=args.blocks, n_stat_blocks=args.slices,
                      **kw)
            for _ in range(args.settle):
                m.batch_sweep_async()
            ms = timed(torch, m.batch_sweep_async, args.sweeps, args.warmup)
            m.materialise()
            m.components.dev.check_status()
            occupied = m.components.K
            if args.map:
                line(name, args.route, ms, occupied)
                ms = timed(torch, lambda: m.batch_sweep_async(map_assign=True), args.sweeps, args.warmup)
                moved = m._get_sweeper().moved()
                m.materialise()
                m.components.dev.check_status()
                occupied = m.components.K
                print("   (the last MAP sweep moved %d items)" % moved)
                line(name, "items-MAP", ms, occupied)
                continue
        elif args.route == "segmenter":
            from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
            keys = ["u%07d" % i for i in range(args.n)]
            one = np.array([0])
            seg = UnigramAcousticWordseg(
                FBGMM, 1.0, args.k_max, prior, {k: X[i:i + 1] for i, k in enumerate(keys)}, {k: one for k in keys},
                {k: [1] for k in keys}, {k: [1] for k in keys}, seed_boundaries_dict={k: [1] for k in keys},
                seed_assignments_dict={k: [int(assign[i])] for i, k in enumerate(keys)}, covariance_type=cov, n_slices_min=0,
                n_slices_max=1, beta_sent_boundary=-1, sync="sequential", n_gibbs_blocks=args.blocks, n_stat_blocks=args.slices)
            ms = timed(torch, seg.batch_sweep_async, args.sweeps, args.warmup)
            seg.materialise()
            seg._df.check_status()
            occupied = seg.acoustic_model.components.K
        else:
            bkw = dict(n_gibbs_blocks=args.blocks, n_stat_blocks=args.slices) if args.settle else {}
            m = FBGMM(X, prior, 1.0, args.k_max, assign, covariance_type=cov, **bkw)
            for _ in range(args.settle):
                m.batch_sweep_async()
            m.materialise()
            sweep = (lambda n: m.map_assign(n, sync="sequential")) if args.map else m.gibbs_sample
            sweep(min(args.warmup, 1))
            t0 = time.time()
            rec = sweep(args.sweeps)
            wall = time.time() - t0
            ms = [1e3 * t for t in rec["sample_time"]]
            occupied = rec["components"][-1]
            print("   (wall time of the %d calls with their records: %.2f s%s)"
                  % (args.sweeps, wall, "; moved per sweep %s" % rec["n_moved"] if args.map else ""))
        line(name, args.route + ("-MAP" if args.map and args.route == "serial" else ""), ms, occupied)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Batch refits of the segmental k-means between batch sweeps (kmeans_refit_async) on the headline corpus of
bench.py (10 000 utterances x 20 landmarks, D 100, K 1 000, n_slices_max 6, one GPU) -- development measurement, not
bench.py; the table of profiles/README.md "Batch refits between k-means sweeps" comes from it.

--route refit    a fresh sync="batch" segmenter.  Sweeps 1-5 each followed by one refit, then --settle sweeps, then --rounds
                 rounds of [sweep, sweep, refit, sweep]: one HIP event pair around every call, nothing read back in between.
                 Prints ms per refit (sweeps 1-5 one by one; settled chain: median and range), ms of a sweep that follows a
                 sweep and of one that follows a refit, and the hint-miss permille of both kinds of sweep
                 (segk_kmeans_hint_feedback).  --profile-rounds N: only N settled rounds after the settling sweeps, for a run
                 under `rocprofv3 --kernel-trace --stats`.
--route serial   the route that existed before: segment(1, n_iter_inbetween_kmeans=1) on an object built with sync="batch",
                 same corpus and seeds -- KMeans.fit after the batch sweep (the assignment vector to the host, exact_max over
                 the tokens, one del_item and one add_item launch per moved token from a Python loop).  Wall time of the call
                 minus the sweep's own sample_time, on the fresh chain (sweeps 1-5) and after --settle sweeps.  Uses nothing this
                 tool's commit added, so the file also runs on an older checkout.
"""
import argparse
import ctypes as C
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def build(args):
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(args.utts, args.dim, args.K, seed=0, N=args.landmarks, n_slices_max=args.n_slices_max)
    random.seed(0)
    np.random.seed(0)
    return kaw.SegmentalKMeansWordseg(args.K, *corpus, n_slices_max=args.n_slices_max, init_am_assignments="spread", sync="batch")


def fmt(ms):
    return "median %7.3f ms (%7.3f - %7.3f, n %d)" % (float(np.median(ms)), min(ms), max(ms), len(ms))


def route_refit(args, torch):
    from segmentalist_amd import _abi
    seg = build(args)
    L, ctx = _abi.lib(), _abi.ctx()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    def permille():
        # (the figure of the latest hinted call that has reached the host: read after a synchronisation)
        torch.cuda.synchronize()
        launched, seen, pm = C.c_uint32(0), C.c_uint32(0), C.c_int32(0)
        _abi.check(L.segk_kmeans_hint_feedback(ctx, C.byref(launched), C.byref(seen), C.byref(pm)))
        return (int(seen.value), int(pm.value))

    if args.profile_rounds:
        for _ in range(5 + args.settle):
            seg.batch_sweep_async()
        for _ in range(args.profile_rounds):
            seg.batch_sweep_async()
            seg.batch_sweep_async()
            seg.kmeans_refit_async()
            seg.batch_sweep_async()
        torch.cuda.synchronize()
        seg._dk.check_status()
        print("profile run: %d settling sweeps, %d rounds of [sweep, sweep, refit, sweep]" % (5 + args.settle, args.profile_rounds))
        return
    early = []
    for it in range(5):
        s = timed(seg.batch_sweep_async)
        r = timed(seg.kmeans_refit_async)
        torch.cuda.synchronize()
        early.append((s[0].elapsed_time(s[1]), r[0].elapsed_time(r[1]), int(seg._dk.refit_moved.item()), seg.acoustic_model.components.K))
    seg._dk.check_status()
    for it, (s, r, moved, K) in enumerate(early):
        print("sweep %d: %7.3f ms, refit behind it: %7.3f ms, moved %6d tokens, K %4d" % (it + 1, s, r, moved, K), flush=True)
    for _ in range(args.settle):
        seg.batch_sweep_async()
    torch.cuda.synchronize()
    after_sweep, refit, after_refit, pm_sweep, pm_refit, moved = [], [], [], [], [], []
    for _ in range(args.rounds):
        seg.batch_sweep_async()
        e1 = timed(seg.batch_sweep_async)
        pm_sweep.append(permille())
        e2 = timed(seg.kmeans_refit_async)
        e3 = timed(seg.batch_sweep_async)
        pm_refit.append(permille())
        moved.append(int(seg._dk.refit_moved.item()))
        after_sweep.append(e1[0].elapsed_time(e1[1]))
        refit.append(e2[0].elapsed_time(e2[1]))
        after_refit.append(e3[0].elapsed_time(e3[1]))
    seg._dk.check_status()
    print("settled chain (%d sweeps in front), %d rounds; tokens moved per refit: %s" % (5 + args.settle, args.rounds, moved))
    print("  refit step                  %s" % fmt(refit))
    print("  sweep that follows a sweep  %s   hint-miss permille %s" % (fmt(after_sweep), [p[1] for p in pm_sweep]))
    print("  sweep that follows a refit  %s   hint-miss permille %s" % (fmt(after_refit), [p[1] for p in pm_refit]))
    print("  (hinted calls seen: %s)" % [p[0] for p in pm_sweep + pm_refit][-4:])
    # back-to-back, as a chain runs them: wall time of `rounds` x [sweep, refit] against `rounds` x [sweep]
    for name, body in (("sweep", lambda: seg.batch_sweep_async()), ("sweep + refit", lambda: (seg.batch_sweep_async(), seg.kmeans_refit_async()))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.rounds):
            body()
        torch.cuda.synchronize()
        print("  %-13s back to back: %7.3f ms per round (wall, %d rounds)" % (name, 1e3 * (time.perf_counter() - t0) / args.rounds, args.rounds))
    seg._dk.check_status()
    # the driver, records and all (one device-to-host copy per sweep and per refit; the refit scores exactly the tokens, whose
    # number the sweep's record has brought): the figure to set against --route serial
    for name, kw in (("segment(R)", {}), ("segment(R, n_iter_inbetween_kmeans=1, kmeans_sync=\"batch\")",
                                          dict(n_iter_inbetween_kmeans=1, kmeans_sync="batch"))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = seg.segment(args.rounds, **kw)
        torch.cuda.synchronize()
        print("  %s: %7.3f ms per iteration (wall, R = %d; %d tokens)" % (name, 1e3 * (time.perf_counter() - t0) / args.rounds, args.rounds,
                                                                         rec["n_tokens"][-1]))


def route_serial(args, torch):
    seg = build(args)

    def one(tag):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = seg.segment(1, n_iter_inbetween_kmeans=1)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        print("%s: segment(1, n_iter_inbetween_kmeans=1) %9.3f ms, of which the sweep %7.3f ms -> KMeans.fit(1) %9.3f ms; K %d"
              % (tag, 1e3 * wall, 1e3 * rec["sample_time"][0], 1e3 * (wall - rec["sample_time"][0]), rec["components"][0]), flush=True)

    for it in range(5):
        one("sweep %d" % (it + 1))
    seg.segment(args.settle)
    for it in range(min(args.rounds, 5)):
        one("settled (%d sweeps in front)" % (5 + args.settle + it))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("refit", "serial"), default="refit")
    ap.add_argument("--utts", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--landmarks", type=int, default=20)
    ap.add_argument("--n-slices-max", type=int, default=6)
    ap.add_argument("--settle", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--profile-rounds", type=int, default=0)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    print("route %s on %s: %d utterances x %d landmarks, D %d, K %d" % (args.route, torch.cuda.get_device_name(0), args.utts,
                                                                         args.landmarks, args.dim, args.K), flush=True)
    (route_refit if args.route == "refit" else route_serial)(args, torch)


if __name__ == "__main__":
    main()

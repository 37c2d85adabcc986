#!/usr/bin/env python3
"""One Lloyd iteration of KMeans.fit through both routes -- on the device (on_device=True) and item by item
(the default: exact_max, then one del_item and one add_item launch per moved item from a Python loop) -- development
measurement, not bench.py; the table of profiles/README.md "KMeans.fit on the device" comes from it.

Both routes run on twin objects built from the same seeds, so every timed iteration starts from the same state and does the
same work (the tool checks that the two records agree).  An iteration ends with the device-to-host copy of its record, so
it is timed as a whole: a HIP event pair around the call (recorded before it and after it, read after a synchronisation) and
the wall time between two synchronisations.  Shapes that time a first iteration run two device iterations on a throwaway
twin first (the score path's workspaces, the kernels' first launches).

--shape settled  the headline corpus of bench.py (10 000 utterances x 20 landmarks, D 100, K 1 000, n_slices_max 6) as a
                 sync="batch" segmenter after 5 + --settle sweeps: --rounds rounds of [sweep, fit(1, consider_unassigned=False)].
--shape fresh    the same segmenter right after construction: fit(1, consider_unassigned=False) for iterations 1.. --iters.
--shape rows     a stand-alone KMeans of --rows rows, D 39, K_max 100, "rand" assignments: iterations 1.. --iters.  The
                 item-by-item route stops before an iteration once it has used --old-limit seconds.
--route device   only the device route (for a run under `rocprofv3 --kernel-trace --stats`).
The item-by-item route is byte-identical to the parent commit's (segmentalist_amd/kmeans.py's loop and the entry points behind
it are untouched), so it is timed in this build.
"""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def build_segmenter(args):
    from segmentalist_amd import kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(args.utts, args.dim, args.K, seed=0, N=args.landmarks, n_slices_max=args.n_slices_max)
    random.seed(0)
    np.random.seed(0)
    return kaw.SegmentalKMeansWordseg(args.K, *corpus, n_slices_max=args.n_slices_max, init_am_assignments="spread", sync="batch")


def build_rows(args):
    from segmentalist_amd.kmeans import KMeans
    rs = np.random.RandomState(0)
    centres = rs.randn(60, 39) * 3.0
    X = (centres[rs.randint(60, size=args.rows)] + rs.randn(args.rows, 39)).astype(np.float32)
    np.random.seed(0)
    return KMeans(X, 100, "rand")


def timed_fit(torch, model, **kw):
    """-> (event ms, wall ms, record) of model.fit(1, **kw)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    rec = model.fit(1, **kw)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), 1e3 * (time.perf_counter() - t0), rec


def same(r1, r2):
    return r1["n_mean_updates"] == r2["n_mean_updates"] and r1["components"] == r2["components"]


def line(tag, moved, K, dev, old):
    s = "%-22s moved %7d  K %5d   device %9.3f ms (wall %9.3f)" % (tag, moved, K, dev[0], dev[1])
    if old is not None:
        s += "   item by item %11.3f ms (wall %11.3f)" % (old[0], old[1])
        if moved:
            s += " = %7.2f us per moved item" % (1e3 * old[1] / moved)
        s += "   x%.1f" % (old[1] / dev[1])
    print(s, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("settled", "fresh", "rows"), default="settled")
    ap.add_argument("--route", choices=("both", "device"), default="both")
    ap.add_argument("--utts", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--landmarks", type=int, default=20)
    ap.add_argument("--n-slices-max", type=int, default=6)
    ap.add_argument("--settle", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--old-limit", type=float, default=120.0)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    both = args.route == "both"
    print("shape %s, route %s on %s" % (args.shape, args.route, torch.cuda.get_device_name(0)), flush=True)
    if args.shape == "rows":
        # (a throwaway twin takes the first call's costs: the score path's workspaces, the kernels' first launches)
        build_rows(args).fit(2, on_device=True)
        new, old = build_rows(args), (build_rows(args) if both else None)
        print("stand-alone KMeans: %d rows, D 39, K_max 100, \"rand\"" % args.rows, flush=True)
        used = 0.0
        for it in range(args.iters):
            dev = timed_fit(torch, new, on_device=True)
            ref = None
            if old is not None and used < args.old_limit:
                ref = timed_fit(torch, old)
                used += ref[1] / 1e3
                assert same(dev[2], ref[2]), (dev[2], ref[2])
            elif old is not None:
                old = None
                print("(item-by-item route stopped: %.0f s used)" % used)
            line("iteration %d" % (it + 1), dev[2]["n_mean_updates"][0], dev[2]["components"][0], dev, ref)
        return
    segs = [build_segmenter(args)] + ([build_segmenter(args)] if both else [])
    n_emb = segs[0]._dk.corpus.n_emb
    print("segmenter: %d utterances x %d landmarks, D %d, K %d, %d embedding rows" % (args.utts, args.landmarks, args.dim, args.K,
                                                                                       n_emb), flush=True)
    kw_new = dict(consider_unassigned=False, on_device=True, _n_items_bound=int(segs[0]._corpus.lengths_np.sum()))
    if args.shape == "fresh":
        build_segmenter(args).acoustic_model.fit(2, **kw_new)          # (a throwaway twin takes the first call's costs)
        for it in range(args.iters):
            dev = timed_fit(torch, segs[0].acoustic_model, **kw_new)
            ref = timed_fit(torch, segs[1].acoustic_model, consider_unassigned=False) if both else None
            assert ref is None or same(dev[2], ref[2]), (dev[2], ref[2])
            line("fresh, iteration %d" % (it + 1), dev[2]["n_mean_updates"][0], dev[2]["components"][0], dev, ref)
        return
    for seg in segs:
        for _ in range(5 + args.settle):
            seg.batch_sweep_async()
    torch.cuda.synchronize()
    rows = []
    for r in range(args.rounds):
        out = []
        for seg, kw in zip(segs, (kw_new, dict(consider_unassigned=False))):
            seg.batch_sweep_async()
            out.append(timed_fit(torch, seg.acoustic_model, **kw))
        assert len(out) == 1 or same(out[0][2], out[1][2]), (out[0][2], out[1][2])
        line("settled, round %d" % (r + 1), out[0][2]["n_mean_updates"][0], out[0][2]["components"][0], out[0], out[1] if both else None)
        rows.append(out)
    for j, name in enumerate(("device", "item by item")[:len(segs)]):
        ms = [o[j][1] for o in rows]
        print("settled chain (%d sweeps in front), %-12s: median %8.3f ms wall (%8.3f - %8.3f, n %d)"
              % (5 + args.settle, name, float(np.median(ms)), min(ms), max(ms), len(ms)))


if __name__ == "__main__":
    main()

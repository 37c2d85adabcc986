#!/usr/bin/env python3
"""Throughput of the sequential (reference-chain) and batch FBGMM / bigram Gibbs drivers on BASELINE
config 2 shapes (1 000 utterances, D = 39, K = 100) -- development measurement, not bench.py.
--fb-type viterbi: the Viterbi / MAP sweeps of the unigram segmenters, with either --sync (the bigram one has no such mode).
--cov full: the unigram segmenter with full-covariance components in place of --which (D <= 64): --sync sequential its
serial chain (four launches per utterance), --sync batch its batch sweeps (profiles/README.md "Full-covariance batch
sampler"); no oracle timing.
--am-n-iter M (with --sync batch): the time of ONE inner acoustic-model sweep of gibbs_sample(n, am_n_iter=M) over the segmenter's
current tokens, --sweeps repeats of M sweeps each from the batch state, median and range, by the route --am-sync names:
  batch       the acoustic-model batch sweep (am_batch_sweep_async: prepare, segk_fbt_assign, partials per block)
  sequential  what gibbs_sample does without am_sync: leave batch mode (materialise), the serial chain over the tokens, and the
              re-entry into batch mode the next outer sweep pays
  fbb         the same step with segk_fbb_assign on the unchanged token lists (prepare, assign, partials per block), driven
              from this tool only
(profiles/README.md "Acoustic-model batch sweeps").
--am-precision f32 (diagonal components): the float32 inner sweeps -- route `batch` is
am_batch_sweep_async(score_precision="f32") (the tile kernel segk_fbt_assign_diag32 or segk_fbb_assign_diag32 by the dispatch
constant; SEGK_AM32_TILE_MIN=0 forces the tiles), route `fbb` drives segk_fbb_assign_diag32 on the unchanged token lists."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--cpu-utts", type=int, default=40)
    ap.add_argument("--which", default="diag,fixed,bigram")
    ap.add_argument("--sync", default="sequential")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--precision", default="f64")
    ap.add_argument("--fb-type", default="standard", choices=["standard", "viterbi"])
    ap.add_argument("--cov", default=None, choices=["full"])
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--am-n-iter", type=int, default=0)
    ap.add_argument("--am-sync", default="batch", choices=["batch", "sequential", "fbb"])
    ap.add_argument("--am-precision", default="f64", choices=["f64", "f32"])
    args = ap.parse_args()
    if args.am_n_iter > 0 and args.sync != "batch":
        ap.error("--am-n-iter times the inner sweeps of batch mode: it needs --sync batch")
    if args.cov == "full":
        args.which = "full"
    import torch
    from segmentalist_amd import bigram_acoustic_wordseg as baw, fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.synth import make_corpus
    from oracle import np_oracle as no
    D, K = args.dim, args.K
    corpus = make_corpus(args.utts, D, K, seed=0, N=20, n_slices_max=6)
    keys = sorted(corpus[0])[:args.cpu_utts]
    sub = tuple({k: d[k] for k in keys} for d in corpus)
    fixed = (0.002 * np.ones(D), np.zeros(D), 0.002 / 0.05 * np.ones(D))
    diag = (np.zeros(D), 0.05, D + 3, 0.002 * (D + 3) * np.ones(D))
    kw = dict(n_slices_min=0, n_slices_max=6, p_boundary_init=0.5, beta_sent_boundary=-1, lms=1.0, wip=0.0,
              init_am_assignments="rand", time_power_term=1.0)
    okw = dict(kw)
    full = (np.zeros(D), 0.05, D + 3, 0.002 * (D + 3) * np.eye(D))
    if args.sync == "batch":
        kw.update(sync="batch", n_gibbs_blocks=args.blocks, n_stat_blocks=args.slices)
    pk = dict(score_precision=args.precision) if args.sync == "batch" else {}
    lm = {"type": "smooth", "intrp_lambda": 0.1, "a": 0.5, "b": 0.5}
    for which in args.which.split(","):
        if which == "bigram" and args.fb_type == "viterbi":
            print("bigram: no Viterbi mode (fb_type is \"bigram\" or \"unigram\"), skipped", flush=True)
            continue
        random.seed(0)
        np.random.seed(0)
        t0 = time.perf_counter()
        if which == "full":
            # (the constructor takes "full" with sync="sequential" only; the batch sweeps are enqueued below all the same)
            seg = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, NIW(*full), *corpus, covariance_type="full",
                                             fb_type=args.fb_type, **dict(kw, sync="sequential"), **pk)
        elif which == "diag":
            seg = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, NIW(*diag), *corpus, covariance_type="diag",
                                             fb_type=args.fb_type, **kw, **pk)
        elif which == "fixed":
            seg = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, FixedVarPrior(*fixed), *corpus,
                                             covariance_type="fixed", fb_type=args.fb_type, **kw, **pk)
        else:
            seg = baw.BigramAcousticWordseg(K, FixedVarPrior(*fixed), lm, *corpus, covariance_type="fixed",
                                            fb_type="unigram", **kw, **pk)
        torch.cuda.synchronize()
        t_init = time.perf_counter() - t0
        if args.am_n_iter > 0:
            inner_sweeps(seg, which, args)
            continue
        if args.sync == "batch":
            st = []
            for _ in range(args.sweeps + 1):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                seg.batch_sweep_async()
                torch.cuda.synchronize()
                st.append(time.perf_counter() - t1)
            seg._df.check_status()
            st = st[1:]
            cnt, tot, occ = seg._get_sweeper().totals()
            rec = {"components": [occ]}
        else:
            rec = seg.gibbs_sample(args.sweeps)
            st = rec["sample_time"]
        print("%-6s init %.2f s; sweep times %s s -> %.2f sweeps/s (%.1f us/utterance); K=%d"
              % (which, t_init, ["%.3f" % x for x in st], 1.0 / min(st), 1e6 * min(st) / args.utts,
                 rec["components"][-1]), flush=True)
        # oracle on a bounded sample (--cpu-utts 0: device timings only)
        if not keys or which == "full":
            continue
        random.seed(0)
        np.random.seed(0)
        if which == "diag":
            ref = no.UnigramAcousticWordseg(no.FBGMM, 1.0, K, no.NIW(*diag), *sub, covariance_type="diag",
                                            fb_type=args.fb_type, **okw)
        elif which == "fixed":
            ref = no.UnigramAcousticWordseg(no.FBGMM, 1.0, K, no.FixedVarPrior(*fixed), *sub,
                                            covariance_type="fixed", fb_type=args.fb_type, **okw)
        else:
            ref = no.BigramAcousticWordseg(K, no.FixedVarPrior(*fixed), lm, *sub, covariance_type="fixed",
                                           fb_type="unigram", **okw)
        t0 = time.perf_counter()
        for i in range(len(keys)):
            ref.gibbs_sample_i(i)
        dt = time.perf_counter() - t0
        print("%-6s oracle (1 core): %.2f ms/utterance -> %.4f sweeps/s" % (which, 1e3 * dt / len(keys),
                                                                          len(keys) / dt / args.utts), flush=True)


def inner_sweeps(seg, which, args):
    """--am-n-iter: one outer batch sweep (the batch state exists, the workspaces are grown), one untimed repeat, then
    --sweeps timed repeats of args.am_n_iter inner sweeps by the route --am-sync names."""
    import json
    import torch
    from segmentalist_amd._abi import check, ptr
    sw, df, m = seg._get_sweeper(), seg._df, args.am_n_iter
    seg.batch_sweep_async()
    torch.cuda.synchronize()

    f32 = args.am_precision == "f32"
    if f32 and args.am_sync == "sequential":
        raise SystemExit("--am-precision f32 names the batch inner sweeps: --am-sync batch or fbb")

    def batch():
        for _ in range(m):
            seg.am_batch_sweep_async(score_precision="f32" if f32 else None)

    def sequential():
        seg._leave_batch()
        seg.acoustic_model.gibbs_sample(m, consider_unassigned=False)
        sw.enter(seg._dev_bounds)

    def fbb():
        import ctypes
        L, ctx, cp, fp, bp, st = sw._args()
        if f32:
            bp = ctypes.byref(sw._bt_am32())
        for _ in range(m):
            for b in range(sw.B):
                check(L.segk_fbb_prepare(ctx, cp, fp, bp, b, st))
                if f32:
                    check(L.segk_fbb_assign_diag32(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], sw.sweep_index, 1.0,
                                                   ptr(df.new_tok), ptr(df.n_new), st))
                else:
                    check(L.segk_fbb_assign(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, sw._n_utts[b], sw.sweep_index, 1.0, ptr(df.new_tok),
                                            ptr(df.n_new), None, 0, st))
                check(L.segk_fbb_partials(ctx, cp, fp, bp, sw.s_lo, sw.s_n, b, ptr(df.new_tok), ptr(df.n_new), st))
            sw.sweep_index += 1

    route = {"batch": batch, "sequential": sequential, "fbb": fbb}[args.am_sync]
    times = []
    for rep in range(args.sweeps + 1):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        route()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t1) / m)
    df.check_status()
    times = sorted(times[1:])
    n_tok = int(df.n_new.sum().item())
    print(json.dumps({"inner_sweep": which, "am_sync": args.am_sync, "am_precision": args.am_precision,
                      "token_bound_per_block": max(sum(cap) for cap in sw._tok_cap), "am_n_iter": m, "repeats": len(times), "tokens": n_tok,
                      "median_ms": 1e3 * float(np.median(times)), "min_ms": 1e3 * times[0], "max_ms": 1e3 * times[-1],
                      "range_ms": 1e3 * (times[-1] - times[0]), "tokens_per_s": n_tok / float(np.median(times))}), flush=True)


if __name__ == "__main__":
    main()

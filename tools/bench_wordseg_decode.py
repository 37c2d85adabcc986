#!/usr/bin/env python3
"""Decoding held-out utterances with a fitted unigram segmenter (UnigramAcousticWordseg.decode) -- development measurement,
not bench.py; the table of DESIGN.md 4.23 and profiles/decode_bench.txt come from it.

make_corpus(2 x --utts, ...) at the README shape (D = 39, K_max = 100, N = 20, window 6, diagonal components): the first
--utts utterances train a batch segmenter with fb_type "viterbi" (--settle sweeps leave it in a live batch state), the others
are the held-out set.  Per --precision, in ONE session, --calls rounds after --warmup, every round timing in turn (host clock
around work that ends in a device synchronise):

  decode (device)    the call on a held-out corpus that is resident on the device: segk_fbb_prepare(-1), segk_fbi_predict over
                     all candidate rows, segk_fbd_decode, the flattening of the segment arrays; nothing read back
  batch sweep        one Viterbi batch sweep of the model over its own --utts utterances (batch_sweep_async): code the change
                     did not touch -- the comparison the decode must not lose
  decode (dicts)     decode(...) from the four dictionaries, NumPy results: the tables of the held-out utterances built on the
                     host, their upload and the read-back on top

and once, on a second segmenter over training plus held-out utterances (sync "sequential", fb_type "viterbi"): the serial
Viterbi visits gibbs_sample_i of --serial held-out utterances, wall time, EXTRAPOLATED to --utts utterances.  Medians, minima
and maxima of the rounds are printed as JSON lines."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=39)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--precision", default="f64,f32")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--serial", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--slices", type=int, default=8)
    args = ap.parse_args()
    import torch
    from segmentalist_amd import fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.synth import make_corpus
    D, K, U = args.dim, args.K, args.utts
    corpus = make_corpus(2 * U, D, K, seed=0, N=20, n_slices_max=6)
    keys = sorted(corpus[0])
    train = tuple({k: d[k] for k in keys[:U]} for d in corpus)
    held = tuple({k: d[k] for k in keys[U:]} for d in corpus)
    diag = (np.zeros(D), 0.05, D + 3, 0.002 * (D + 3) * np.ones(D))
    kw = dict(n_slices_min=0, n_slices_max=6, p_boundary_init=0.5, beta_sent_boundary=-1, lms=1.0, wip=0.0,
              init_am_assignments="rand", time_power_term=1.0, covariance_type="diag", fb_type="viterbi")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    for prec in args.precision.split(","):
        random.seed(0)
        np.random.seed(0)
        seg = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, NIW(*diag), *train, sync="batch", n_gibbs_blocks=args.blocks,
                                         n_stat_blocks=args.slices, score_precision=prec, **kw)
        for _ in range(args.settle):
            seg.batch_sweep_async()
        torch.cuda.synchronize()
        seg._df.check_status()
        t_prep, (labels, cq) = timed(lambda: seg._heldout_corpus(*held))
        t = {"decode_device": [], "batch_sweep": [], "decode_dicts": []}
        res = None
        for r in range(args.warmup + args.calls):
            a, res = timed(lambda: seg._decode_corpus(labels, cq))
            b, _ = timed(seg.batch_sweep_async)
            c, _ = timed(lambda: seg.decode(*held))
            if r >= args.warmup:
                t["decode_device"].append(a)
                t["batch_sweep"].append(b)
                t["decode_dicts"].append(c)
        seg._df.check_status()
        res = res.numpy()
        line = {"precision": prec, "utterances": U, "held_out_rows": int(cq.n_emb), "segments": int(res.seg_offsets[-1]), "K": res.K,
                "calls": args.calls, "heldout_corpus_once_ms": 1e3 * t_prep}
        for k, v in t.items():
            line[k] = stats(v)
        line["decode_device_us_per_utterance"] = 1e3 * line["decode_device"]["median_ms"] / U
        line["decode_over_sweep"] = line["decode_device"]["median_ms"] / line["batch_sweep"]["median_ms"]
        print(json.dumps(line), flush=True)

    if args.serial > 0:
        random.seed(0)
        np.random.seed(0)
        both = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, 1.0, K, NIW(*diag), *corpus, sync="sequential", **kw)
        torch.cuda.synchronize()
        both.gibbs_sample_i(U)                                       # (first visit: workspaces)
        t0 = time.perf_counter()
        for i in range(U + 1, U + 1 + args.serial):
            both.gibbs_sample_i(i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"serial_viterbi_visits": args.serial, "us_per_utterance": 1e6 * dt / args.serial,
                          "extrapolated_ms_for_%d_utterances" % U: 1e3 * dt / args.serial * U}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Full-covariance span scores (segk_fbgmm_score, cov_type 2): the lane-per-row kernels (k_fc_span_terms + k_fc_span_lse)
against the workgroup-per-row kernel (k_fc_score) on the same rows -- development measurement, not bench.py; the table of
profiles/README.md "Full-covariance segmenter" comes from it.

Per shape: medians of --reps timed calls after --warmup, by HIP events on the launch stream, the whole measurement
repeated --rounds times (the range of the medians is the run-to-run spread).  SEGK_FC_SPAN_MIN, read by the library at
every call, selects the path.  Then the list length at which the paths cross (the threshold FC_SPAN_MIN of
segk_fullcov.hip), and the time per utterance of full gibbs_sample sweeps of the segmenter on the long-utterance case of
tests/fullcov_wordseg.py."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

BIG = "1000000000"


def model(D, K_max, K_active, n_rows, seed=0):
    from segmentalist_amd import fbgmm
    from segmentalist_amd.niw import NIW
    rs = np.random.RandomState(seed)
    mu = rs.randn(max(2, K_active // 2), D)
    X = (mu[rs.randint(0, len(mu), n_rows)] + 0.3 * rs.randn(n_rows, D)).astype(np.float32)
    assign = np.arange(n_rows) % K_active
    rs.shuffle(assign)
    return fbgmm.FBGMM(X, NIW(np.zeros(D), 0.05, D + 3, 0.1 * (D + 3) * np.eye(D)), 1.0, K_max, assign, covariance_type="full")


def time_score(torch, dev, ids_t, n, span_min, reps, warmup):
    os.environ["SEGK_FC_SPAN_MIN"] = span_min
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(warmup):
        dev.score_rows(ids_t.data_ptr(), n=n)
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        dev.score_rows(ids_t.data_ptr(), n=n)
        b.record()
    torch.cuda.synchronize()
    del os.environ["SEGK_FC_SPAN_MIN"]
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3        # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=4)
    args = ap.parse_args()
    import torch
    from segmentalist_amd.device import to_dev
    torch.cuda.set_device(0)
    print("shape                                   | k_fc_score us (range)      | lane-per-row us (range)    | ratio | max rel diff")
    # (D, K_max, K active, rows scored)
    for D, K_max, K_act, n in [(16, 10, 10, 105), (39, 100, 39, 105), (64, 100, 100, 1000)]:
        fm = model(D, K_max, K_act, max(4 * n, 40 * K_act))
        dev = fm.components.dev
        dev.check_status()
        ids = to_dev(np.random.RandomState(1).permutation(fm.components.N)[:n], np.int32)
        old = [time_score(torch, dev, ids, n, BIG, args.reps, args.warmup) for _ in range(args.rounds)]
        a = dev.score[ids.long()].cpu().numpy()
        new = [time_score(torch, dev, ids, n, "1", args.reps, args.warmup) for _ in range(args.rounds)]
        b = dev.score[ids.long()].cpu().numpy()
        print("D %2d K_max %3d (%3d active) %4d rows      | %8.1f (%7.1f-%7.1f) | %8.1f (%7.1f-%7.1f) | %5.2f | %.1e"
              % (D, K_max, K_act, n, np.median(old), min(old), max(old), np.median(new), min(new), max(new),
                 np.median(old) / np.median(new), np.max(np.abs(a - b) / np.abs(a))), flush=True)
    # where the paths cross
    for D, K_max, K_act in [(16, 10, 10), (39, 100, 39)]:
        fm = model(D, K_max, K_act, 40 * K_act)
        dev = fm.components.dev
        line = []
        for n in (1, 2, 4, 8, 16, 32, 64):
            ids = to_dev(np.arange(n), np.int32)
            line.append("n=%d: %.1f / %.1f" % (n, time_score(torch, dev, ids, n, BIG, args.reps, args.warmup),
                                               time_score(torch, dev, ids, n, "1", args.reps, args.warmup)))
        print("D %d K_max %d (%d active), us per call k_fc_score / lane-per-row: %s" % (D, K_max, K_act, "; ".join(line)), flush=True)
    # full sweeps of the segmenter, long utterances (40 .. 70 landmarks, triangles of ~330 rows)
    from segmentalist_amd import fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd.niw import NIW
    from tests import fullcov_wordseg as fw
    ci = fw.LONG_CASE
    for label, span_min in (("k_fc_score", BIG), ("lane-per-row", None)):
        if span_min:
            os.environ["SEGK_FC_SPAN_MIN"] = span_min
        random.seed(1)
        np.random.seed(1)
        seg = uaw.UnigramAcousticWordseg(fbgmm.FBGMM, fw.ALPHA, fw.CASES[ci][2], NIW(*fw.prior_params(ci)), *fw.case_corpus(ci),
                                         **fw.seg_kwargs(ci))
        rec = seg.gibbs_sample(args.sweeps)
        os.environ.pop("SEGK_FC_SPAN_MIN", None)
        n_utt = seg.utterances.D
        print("gibbs_sample, %d utterances of 40-70 landmarks, D 16, %-12s: sweeps %s ms -> %.0f us/utterance (best sweep); K=%d"
              % (n_utt, label, ["%.2f" % (1e3 * t) for t in rec["sample_time"]], 1e6 * min(rec["sample_time"]) / n_utt,
                 rec["components"][-1]), flush=True)


if __name__ == "__main__":
    main()

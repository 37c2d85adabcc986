"""Premise of the delta score pass (segk_score_hint.hip): how many component columns of the fp16x2 tile image K1 multiplies
change from one batch sweep of the bench chain to the next, and against the base pass the library keeps.  Per sweep: the
library's own figures (segk_kmeans_delta_stats: mode, columns changed against the base, packed tiles, positions the hint waves
skipped), columns of the image (piece 0 and constants) and rows of `means` changed against the PREVIOUS sweep, whether the
relabelling was the identity, rows whose hinted column changed against the previous sweep, the undecided-row queue, and the
sweep's time."""
import ctypes as C
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def image_columns(dk, D):
    """[n_tiles * 32, words] int32: per column the piece-0 operands of every k-step and the constant, as K1 reads them."""
    ks = ((D + 15) // 16)
    stride = (ks * 2 * 256 + 32 + 1023) // 1024 * 1024
    t = dk.tiles_b3[1024:].view(-1, stride).view(dtype=__import__("torch").int32)
    n_t = (dk.K_max + 31) // 32
    t = t[:n_t]
    ops = t[:, :ks * 512].reshape(n_t, ks, 2, 2, 32, 4)[:, :, 0]            # [tile][k-step][lane half][column][4 words]
    ops = ops.permute(0, 3, 1, 2, 4).reshape(n_t * 32, -1)
    cst = t[:, ks * 512:ks * 512 + 32].reshape(n_t * 32, 1)
    hdr = dk.tiles_b3[:1].view(dtype=__import__("torch").int32).expand(n_t * 32, 1)
    return __import__("torch").cat([ops, cst, hdr], dim=1).clone()


def main():
    import torch
    from segmentalist_amd import _abi, kmeans_acoustic_wordseg as kaw
    from segmentalist_amd.synth import make_corpus
    n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n_sweeps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    D, K = 100, 1000
    corpus = make_corpus(n_utt, D, K, seed=0, N=20, n_slices_max=6)
    random.seed(0)
    np.random.seed(0)
    seg = kaw.SegmentalKMeansWordseg(K, *corpus, n_slices_max=6, init_am_assignments="spread", sync="batch")
    dk = seg._dk
    ident = torch.arange(dk.K_max, dtype=torch.int32, device=dk.remap.device)
    prev_img = prev_means = None
    print("sweep  mode  cols_vs_base  packed_tiles  hint_skipped | cols_vs_prev  means_vs_prev  remap_ident  rows_hint_col_changed | queue  full_scan  us")
    for sw in range(1, n_sweeps + 1):
        img, means = image_columns(dk, D), dk.means.clone()             # what this sweep's score call multiplies
        hints = dk.cand_k.clone()
        K_prev = int(dk.K.item())                                       # labels the rows can carry
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        seg.batch_sweep_async()
        e1.record()
        torch.cuda.synchronize()
        st = dk.delta_stats()
        out = (C.c_int32 * 2)()
        _abi.check(_abi.lib().segk_kmeans_stage_counts(_abi.ctx(), C.byref(dk.cand), out, _abi.stream()))
        cols = mch = rows = -1
        if prev_img is not None:
            colchg = (img != prev_img).any(dim=1)
            cols = int(colchg.sum().item())
            mch = int((means.view(dtype=torch.int32) != prev_means.view(dtype=torch.int32)).any(dim=1).sum().item())
            ok = (hints >= 0) & (hints < dk.K_max)
            rows = int(colchg[hints.clamp(0, dk.K_max - 1).long()][ok].sum().item())
        print("%5d  %4d  %12d  %12d  %12d | %12d  %13d  %11d  %21d | %5d  %9d  %.0f" % (
            sw, st[0], st[1], st[2], st[3], cols, mch, int(bool((dk.remap == ident)[:K_prev].all().item())), rows, out[0], out[1],
            1000.0 * e0.elapsed_time(e1)), flush=True)
        prev_img, prev_means = img, means


if __name__ == "__main__":
    main()

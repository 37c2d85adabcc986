#!/usr/bin/env python3
"""
Capture the vectors of the full-covariance segmenter tests from the (py3-translated) reference:
tests/golden/fullcov_wordseg.npz.  The walk every case is put through is tests/fullcov_wordseg.py
`run_case`; here it runs on the reference's `UnigramAcousticWordseg(FBGMM, ..., covariance_type="full")`
with both draw functions (`utils.draw` of the components, `_cython_utils.draw` of the backward
sampling) wrapped to record how far each uniform lay from the nearest edge of the cumulative
distribution.  Data only.

The reference's `GaussianComponents` has no `get_assignments`, so with covariance_type="full" its
`gibbs_sample` dies in the debug trace of utterance `i_debug_monitor` (module default 0,
unigram_acoustic_wordseg.py:264-267): the vectors are recorded with `i_debug_monitor = -1`, with
which the reference runs cleanly.

usage: python tests/golden/build_ref.py /tmp/segk_ref && python tests/golden/make_golden_fullcov_wordseg.py /tmp/segk_ref
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
scratch = sys.argv[1] if len(sys.argv) > 1 else "/tmp/segk_ref"
sys.path.insert(0, scratch)

from segmentalist import _cython_utils, fbgmm, niw, unigram_acoustic_wordseg, utils  # noqa: E402
from tests import fullcov_wordseg as fw  # noqa: E402

unigram_acoustic_wordseg.i_debug_monitor = -1

margins = {"comp": [], "bound": []}


def recording(kind):
    def draw_recording(p_k):
        """utils.py:10-21 / _cython_utils.pyx:75-89, same arithmetic; the margin on the side."""
        k_uni = random.random()
        margin, k_out = np.inf, None
        for i in range(len(p_k)):
            k_uni = k_uni - p_k[i]
            margin = min(margin, abs(k_uni))
            if k_uni < 0 and k_out is None:
                k_out = i
        margins[kind].append(margin)
        return len(p_k) - 1 if k_out is None else k_out
    return draw_recording


def take():
    got = list(margins["comp"]), list(margins["bound"])
    del margins["comp"][:], margins["bound"][:]
    return got


def make_ref(ci):
    K = fw.CASES[ci][2]
    return unigram_acoustic_wordseg.UnigramAcousticWordseg(fbgmm.FBGMM, fw.ALPHA, K, niw.NIW(*fw.prior_params(ci)),
                                                           *fw.case_corpus(ci), **fw.seg_kwargs(ci))


def main():
    utils.draw = recording("comp")
    _cython_utils.draw = recording("bound")
    out = {}
    for ci in range(len(fw.CASES)):
        take()
        res = fw.run_case(ci, make_ref, take, log_uniforms=True)
        tag = fw.case_tag(ci)
        for k, v in res.items():
            out[tag + "_" + k] = v
        comps = [int(res["sweep%d_rec_components" % s]) for s in range(fw.N_SWEEPS)]
        cm = np.concatenate([res["sweep%d_margin_comp" % s] for s in range(fw.N_SWEEPS)])
        bm = np.concatenate([res["sweep%d_margin_bound" % s] for s in range(fw.N_SWEEPS)])
        print(tag, "rows", len(res["init_assign"]), "K init", int(res["init_K"]), "components per sweep", comps,
              "least margin comp %s bound %s" % ("%.2e" % cm.min() if cm.size else "-", "%.2e" % bm.min() if bm.size else "-"))
    path = os.path.join(HERE, "fullcov_wordseg.npz")
    np.savez_compressed(path, **out)
    print("fullcov_wordseg.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

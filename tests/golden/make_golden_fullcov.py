#!/usr/bin/env python3
"""
Capture the vectors of the full-covariance FBGMM tests from the (py3-translated) reference:
tests/golden/fullcov.npz.  The walk every case is put through is tests/fullcov.py `run_case`;
here it runs on the reference's `FBGMM` / `GaussianComponents` with `utils.draw` wrapped to record
how far each uniform lay from the nearest edge of the cumulative distribution.  Data only.

usage: python tests/golden/build_ref.py /tmp/segk_ref && python tests/golden/make_golden_fullcov.py /tmp/segk_ref
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
scratch = sys.argv[1] if len(sys.argv) > 1 else "/tmp/segk_ref"
sys.path.insert(0, scratch)

from segmentalist import fbgmm, niw, utils  # noqa: E402
from tests import fullcov  # noqa: E402

margins = []


def draw_recording(p_k):
    """utils.py:10-21, same arithmetic; the margin on the side."""
    k_uni = random.random()
    margin, k_out = np.inf, None
    for i in range(len(p_k)):
        k_uni = k_uni - p_k[i]
        margin = min(margin, abs(k_uni))
        if k_uni < 0 and k_out is None:
            k_out = i
    margins.append(margin)
    return len(p_k) - 1 if k_out is None else k_out


def take_margins():
    got = list(margins)
    del margins[:]
    return got


def main():
    utils.draw = draw_recording
    out = {}
    for ci in range(len(fullcov.CASES)):
        del margins[:]
        res = fullcov.run_case(ci, fbgmm.FBGMM, niw.NIW, take_margins, covariance_type="full")
        tag = fullcov.case_tag(ci)
        for k, v in res.items():
            out[tag + "_" + k] = v
        n_sw = fullcov.N_SWEEPS[ci]
        comps = [int(res["sweep%d_rec_components" % s]) for s in range(n_sw)]
        print(tag, "K init", int(res["init_K"]), "components per sweep", comps, "least margin %.2e"
              % min([res["draw_margin"].min()] + [res["sweep%d_margin" % s].min() for s in range(n_sw)]))
    path = os.path.join(HERE, "fullcov.npz")
    np.savez_compressed(path, **out)
    print("fullcov.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

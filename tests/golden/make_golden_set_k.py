#!/usr/bin/env python3
"""
Capture the vectors of the FBGMM.set_K tests from the (py3-translated) reference: tests/golden/set_k.npz.  The walk every case
is put through is tests/fbgmm_set_k.py `run_case`; here it runs on the reference's `FBGMM` and calls the reference's own
`set_K` (fbgmm.py:139-180), with `setup_components` wrapped to record the assignments after relabelling and `utils.draw`
wrapped to record every uniform consumed and how far it lay from the nearest edge of the cumulative distribution.  The kept
labels are the reference's own `np.argsort(sizes)[-K:]` on the counts before the call: with the pairwise distinct counts
asserted here they are the stable sort's.  As written the reference's main branch cannot run: fbgmm.py:172 passes a list to
setup_components, whose fbgmm.py:124 calls .max() on it; the wrapper passes the same values on as an array.  The early-branch case records the state before the call only (the reference leaves
nothing usable after it; what its gibbs_sample does then is printed).  Data only.

usage: python tests/golden/build_ref.py /tmp/segk_ref && python tests/golden/make_golden_set_k.py /tmp/segk_ref
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
scratch = sys.argv[1] if len(sys.argv) > 1 else "/tmp/segk_ref"
sys.path.insert(0, scratch)

from segmentalist import fbgmm, gaussian_components_fixedvar, niw, utils  # noqa: E402
from tests import fbgmm_items as fi  # noqa: E402
from tests import fbgmm_set_k as sk  # noqa: E402

uniforms, margins = [], []
recording = [False]


def draw_recording(p_k):
    """utils.py:10-21, same arithmetic; the uniform and the margin on the side."""
    k_uni = random.random()
    if recording[0]:
        uniforms.append(k_uni)
    margin, k_out = np.inf, None
    for i in range(len(p_k)):
        k_uni = k_uni - p_k[i]
        margin = min(margin, abs(k_uni))
        if k_uni < 0 and k_out is None:
            k_out = i
    if recording[0]:
        margins.append(margin)
    return len(p_k) - 1 if k_out is None else k_out


def make_model(case, X, a):
    cov, D, K_max = case[0], case[2], case[3]
    params = fi.prior_params(cov, D)
    prior = gaussian_components_fixedvar.FixedVarPrior(*params) if cov == "fixed" else niw.NIW(*params)
    return fbgmm.FBGMM(X, prior, sk.ALPHA, K_max, np.array(a), covariance_type=cov, lms=sk.LMS)


def reference_set_k(model, K, reassign):
    c = model.components
    counts = np.array(c.counts)
    assert sk.distinct_counts(counts), counts
    if c.K <= K:
        model.set_K(K, reassign)
        return None, None
    keep = [int(k) for k in np.argsort(counts)[-K:]]
    assert keep == [int(k) for k in np.argsort(counts, kind="stable")[-K:]]
    seen = {}
    inner = model.setup_components

    def setup(K_new, assignments="rand", X=None):
        # (fbgmm.py:172 hands over a list and fbgmm.py:124 asks it for .max(): as written the reference's main branch ends in an
        # AttributeError.  The list goes on as an array -- the one repair, made here and not in the reference's text)
        assert isinstance(assignments, list)
        seen["K"], seen["assign"] = K_new, np.array(assignments)
        return inner(K_new, np.array(assignments), X)
    model.setup_components = setup
    recording[0] = True
    model.set_K(K, reassign)
    recording[0] = False
    del model.setup_components
    assert seen["K"] == K
    return keep, seen["assign"]


def main():
    utils.draw = draw_recording
    out = {}
    for name, case in sk.CASES.items():
        del uniforms[:], margins[:]
        early = name == sk.EARLY
        res = sk.run_case(name, make_model, reference_set_k, post=not early)
        res["uniforms"], res["margins"] = np.array(uniforms), np.array(margins)
        for k, v in res.items():
            out[name + "_" + k] = v
        if early:
            # what the reference does after its early branch: the attribute says K, the arrays keep the old length
            X, a = sk.case_inputs(case)
            model = make_model(case, X, a)
            model.set_K(case[6])
            try:
                model.gibbs_sample(1)
                print(name, "reference after the early branch: gibbs_sample ran")
            except Exception as e:      # noqa: BLE001
                print(name, "reference after the early branch: K_max", model.components.K_max, "counts of length",
                      len(model.components.counts), "-> gibbs_sample raises", type(e).__name__ + ":", e)
            continue
        n_orphans = int(np.count_nonzero((res["pre_assign"] != -1) & (res["relabel_assign"] == -1)))
        assert len(uniforms) == (n_orphans if case[8] else 0)
        print(name, "K", int(res["pre_K"]), "->", int(res["post_K"]), "counts", res["pre_counts"].tolist(), "kept", res["keep"].tolist(),
              "orphans", n_orphans, "least margin %.2e" % (min(margins) if margins else np.inf))
    path = os.path.join(HERE, "set_k.npz")
    np.savez_compressed(path, **out)
    print("set_k.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

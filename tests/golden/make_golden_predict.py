#!/usr/bin/env python3
"""
Capture the vectors of the FBGMM.predict tests from the (py3-translated) reference: tests/golden/predict.npz.  Per case of
CASES below (inputs of tests/fbgmm_items.py, query rows of tests/fbgmm_predict.py `query_rows`) the reference's own `FBGMM` is
built over [X; Xq] with the queries at -1, and for every query i the reference's own methods are called:

  log_marg_i     `log_marg_i(i)` (fbgmm.py:256-285)
  log_prob_z     the vector of fbgmm.py:436-445, caught where `gibbs_sample_inside_loop_i` hands it to `logsumexp` (the module's
                 name is wrapped for the call), on a deep copy of the model, so that the draw adds the item to the copy alone
  k              `map_assign_i(i)` (fbgmm.py:465-494) on another deep copy: the label the item holds afterwards

The model itself is never grown: every query sees the statistics of the assigned items only.  Data only.

usage: python tests/golden/build_ref.py /tmp/segk_ref && python tests/golden/make_golden_predict.py /tmp/segk_ref
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
scratch = sys.argv[1] if len(sys.argv) > 1 else "/tmp/segk_ref"
sys.path.insert(0, scratch)

from segmentalist import fbgmm, gaussian_components_fixedvar, niw  # noqa: E402
from tests import fbgmm_items as fi  # noqa: E402
from tests import fbgmm_predict as fp  # noqa: E402

# small cases: the three covariance types, both dtypes, one with unassigned items in the model; (name, queries)
CASES = [("fx_D39_K7_n255", 130), ("dg_D39_K65_n257", 130), ("dg_D39_K7_un", 65), ("fx_D3_K7_n5_8x8", 65),
         ("fc_D3_K7_n5_2x2", 65), ("fc_D39_K65", 30)]


def make_model(case, X, a):
    cov, D, K_max = case[0], case[2], case[3]
    params = fi.prior_params(cov, D)
    prior = gaussian_components_fixedvar.FixedVarPrior(*params) if cov == "fixed" else niw.NIW(*params)
    return fbgmm.FBGMM(X, prior, fi.ALPHA, K_max, np.array(a), covariance_type=cov, lms=fi.LMS)


def main():
    out = {}
    inner = fbgmm.logsumexp
    for name, M in CASES:
        case = fi.CASES[name]
        X, a = fi.make_inputs(case)
        Xq = fp.query_rows(case, M=M)
        N = len(X)
        model = make_model(case, np.concatenate([X, Xq]), np.concatenate([a, np.full(M, -1, np.int64)]))
        c = model.components
        K, counts = int(c.K), np.array(c.counts)
        lm, lz, ks = np.zeros(M), np.zeros((M, case[3])), np.zeros(M, np.int64)
        for r in range(M):
            i = N + r
            lm[r] = model.log_marg_i(i)
            seen = []

            def catching(v):
                seen.append(np.array(v))
                return inner(v)
            fbgmm.logsumexp = catching
            try:
                copy.deepcopy(model).gibbs_sample_inside_loop_i(i, anneal_temp=1)
            finally:
                fbgmm.logsumexp = inner
            assert len(seen) == 1 and seen[0].shape == (case[3],)
            lz[r] = seen[0]
            other = copy.deepcopy(model)
            other.map_assign_i(i)
            ks[r] = other.components.assignments[i]
            assert c.assignments[i] == -1 and int(c.K) == K and np.array_equal(c.counts, counts)
        for k, v in (("M", np.int64(M)), ("Xq", Xq), ("log_marg_i", lm), ("log_prob_z", lz), ("k", ks), ("K", np.int64(K))):
            out[name + "/" + k] = v
        print(name, "K", K, "of", case[3], "queries", M, "labelled K:", int(np.count_nonzero(ks == K)), "labels", len(set(ks.tolist())))
    path = os.path.join(HERE, "predict.npz")
    np.savez_compressed(path, **out)
    print("predict.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

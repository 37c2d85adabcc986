#!/usr/bin/env python3
"""
Capture the vectors of the UnigramAcousticWordseg.decode tests from the (py3-translated) reference: tests/golden/decode.npz.
Per case of CASES below (tests/wordseg_decode.py: the model's state after its own sweeps, the held-out utterances of its
recipe) tests/wordseg_decode.py `witness` is run over the REFERENCE's own building blocks: its `process_embeddings` and
`Utterances` over training plus held-out utterances, its `FBGMM` over all rows with the held-out ones at -1, and per held-out
utterance its own

  get_vec_embed_log_probs    unigram_acoustic_wordseg.py:474-511
  forward_backward_viterbi   :759-864
  map_assign_i               fbgmm.py:465-494, on a deep copy of the acoustic model per chosen segment: the label the
                             embedding holds afterwards
  log_marg_i                 fbgmm.py:256-285 of every chosen segment's embedding

The model itself is never grown.  Data only: boundaries, log probabilities, segment rows, labels and log densities.

usage: python tests/golden/build_ref.py /tmp/segk_ref && python tests/golden/make_golden_decode.py /tmp/segk_ref
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
scratch = sys.argv[1] if len(sys.argv) > 1 else "/tmp/segk_ref"
sys.path.insert(0, scratch)

from segmentalist import fbgmm, gaussian_components_fixedvar, niw, unigram_acoustic_wordseg, utterances  # noqa: E402
from tests import wordseg_decode as wd  # noqa: E402
from tests.golden import cases  # noqa: E402

# fixed variance, diagonal, full covariance, and a band held-out corpus (N_max 92)
CASES = ["fixed_small", "diag_K65", "w0_K8", "fixed_small_x_ragged"]


class ReferenceImpl(object):
    process_embeddings = staticmethod(unigram_acoustic_wordseg.process_embeddings)
    Utterances = utterances.Utterances
    viterbi = staticmethod(unigram_acoustic_wordseg.forward_backward_viterbi)

    def segmenter_class(self, name):
        return unigram_acoustic_wordseg.UnigramAcousticWordseg

    def acoustic_model(self, name, X, assignments):
        if name in wd.FULL:
            from tests import fullcov_batch as fcb
            from tests import fullcov_wordseg as fw
            ci, K_max = fcb.SAMPLED[name][:2]
            return fbgmm.FBGMM(X, niw.NIW(*fw.prior_params(ci)), fw.ALPHA, K_max, assignments, covariance_type="full", lms=fw.LMS)
        from tests import fbgmm_long
        m = wd.model_case(name)
        prior = (gaussian_components_fixedvar.FixedVarPrior(*cases.fixed_prior_params(m["D"])) if m["kind"] == "fixed"
                 else niw.NIW(*cases.diag_prior_params(m["D"])))
        return fbgmm.FBGMM(X, prior, 1.0, m["K"], assignments, covariance_type=m["kind"], lms=fbgmm_long.seg_args(m)["lms"])


def main():
    out = {}
    for name in CASES:
        w = wd.witness(name, ReferenceImpl())
        for k, v in w.items():
            out[name + "/" + k] = v
        lab = w["seg_label"]
        print(name, "K", int(w["K"]), "utterances", len(w["log_prob"]), "N_max", w["boundaries"].shape[1], "segments", len(lab),
              "labelled K:", int(np.count_nonzero(lab == w["K"])), "labels", len(set(lab.tolist())))
    path = os.path.join(HERE, "decode.npz")
    np.savez_compressed(path, **out)
    print("decode.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""
Capture the vectors of the SegmentalKMeansWordseg.decode tests from the (py3-translated) reference:
tests/golden/kmeans_decode.npz.  Per case of CASES below (tests/kmeans_decode.py: the model's state after its own two serial
sweeps, the held-out utterances of its recipe) tests/kmeans_decode.py `witness` is run over the REFERENCE's own building blocks:
its `process_embeddings` and `Utterances` over training plus held-out utterances, its `KMeansComponents` over all rows with the
held-out ones at -1 and the fitted model's arrays copied in, and per held-out utterance its own

  get_vec_embed_neg_len_sqrd_norms    kmeans_acoustic_wordseg.py:334-351
  forward_backward_kmeans_viterbi     :449-555
  argmax_neg_sqrd_norm_i / max_...    kmeans_components.py:228-232 of every chosen segment's embedding
  segment_i                           :225-332 on a deep copy, as a second witness of boundaries and objective

Data only: boundaries, objectives, segment rows, labels and scores.

usage: python tests/golden/build_ref.py /tmp/segk_ref && python tests/golden/make_golden_kmeans_decode.py /tmp/segk_ref
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
scratch = sys.argv[1] if len(sys.argv) > 1 else "/tmp/segk_ref"
sys.path.insert(0, scratch)

from segmentalist import kmeans_acoustic_wordseg, kmeans_components, utterances  # noqa: E402
from tests import kmeans_decode as kd  # noqa: E402

# float32, float64, dead ends, and a held-out corpus of N_max 92
CASES = ["km_mid", "km_f64", "dead_end", "long92_w6"]


class ReferenceImpl(object):
    process_embeddings = staticmethod(kmeans_acoustic_wordseg.process_embeddings)
    Utterances = utterances.Utterances
    KMeansComponents = kmeans_components.KMeansComponents
    Segmenter = kmeans_acoustic_wordseg.SegmentalKMeansWordseg
    viterbi = staticmethod(kmeans_acoustic_wordseg.forward_backward_kmeans_viterbi)


def main():
    out = {}
    for name in CASES:
        w, totals2, bounds2 = kd.witness(name, "serial", ReferenceImpl())
        for k, v in w.as_dict().items():
            out[name + "/" + k] = v
        out[name + "/segment_i_objective"] = totals2
        print(name, "K", w.K, "utterances", len(w.objective), "N_max", w.boundaries.shape[1], "segments", len(w.seg_row),
              "rows >= K:", int(np.count_nonzero(w.seg_row >= w.K)), "without an embedding:", int(np.count_nonzero(w.seg_embed < 0)))
    path = os.path.join(HERE, "kmeans_decode.npz")
    np.savez_compressed(path, **out)
    print("kmeans_decode.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

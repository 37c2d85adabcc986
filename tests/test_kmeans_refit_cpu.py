"""
CPU checks of the batch refit's specification (tests/kmeans_refit.py) and of the inputs the GPU test
(tests/test_gpu_kmeans_refit.py) runs on, before the device is asked anything: the schedule reaches every kind of refit the
device code has a path for, the specification does not depend on the number of statistics blocks, a refit that moves
nothing is the identity, and where no component is founded the specification IS the reference's KMeans.fit.
"""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from oracle import np_oracle as no
from tests import kmeans_refit as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, i) for s in kr.SHAPES for i in kr.INITS]
IDS = ["%dx%dx%d-%s" % (s[0], s[1], s[2], i) for s, i in CASES]


def _fresh(shape, init):
    K, corpus, kw = kr.new_pair_args(shape, init)
    random.seed(5); np.random.seed(5)
    return no.SegmentalKMeansWordseg(K, *corpus, **kw)


@pytest.mark.parametrize("shape", kr.SHAPES, ids=["%dx%dx%d" % s[:3] for s in kr.SHAPES])
def test_schedule_reaches_every_kind_of_refit(shape):
    """Per shape (over both inits): the refit on the fresh segmenter moves tokens and empties components in EVERY case; some
    refit after the first sweep founds a component through a token that names an inactive row (every shape but the first,
    whose six components leave no inactive row near a token), some refit after a sweep empties components, and some refit
    moves nothing."""
    founding = emptying = settled = 0
    for init in kr.INITS:
        steps = kr.schedule_trace(shape, init)
        assert [s["op"] for s in steps] == ["refit"] + ["sweep", "refit", "refit"] * 3
        first = steps[0]
        assert first["n_mean_updates"] > 0 and first["emptied"] > 0, (init, first["n_mean_updates"], first["emptied"])
        assert first["n_tokens"] > 0
        for s in steps[2:]:
            if s["op"] != "refit":
                continue
            founding += s["founding"] > 0
            emptying += s["emptied"] > 0
            settled += s["n_mean_updates"] == 0
    if shape != kr.SHAPES[0]:
        assert founding >= 1
    assert emptying >= 1
    assert settled >= 1


@pytest.mark.parametrize("shape,init", CASES, ids=IDS)
def test_refit_does_not_depend_on_the_number_of_blocks(shape, init):
    """One statistics block against the case's own block count, over the whole schedule: assignments, K and counts are equal
    (only the bits of the sums -- and with them, in principle, later argmaxes -- may differ: the comparison stops at the first
    step whose means differ in a bit, having checked that step's labels)."""
    a, b = kr.schedule_trace(shape, init), kr.schedule_trace(shape, init, n_blocks=1)
    for sa, sb in zip(a, b):
        assert np.array_equal(sa["boundaries"], sb["boundaries"])
        assert np.array_equal(sa["assignments"], sb["assignments"])
        assert sa["K"] == sb["K"]
        assert np.array_equal(sa["counts"], sb["counts"])
        if not np.array_equal(sa["means"], sb["means"]):
            break


@pytest.mark.parametrize("shape,init", CASES, ids=IDS)
def test_a_refit_that_moves_nothing_is_the_identity(shape, init):
    steps = kr.schedule_trace(shape, init)
    seen = 0
    for prev, s in zip(steps, steps[1:]):
        if s["op"] == "refit" and s["n_mean_updates"] == 0:
            seen += 1
            for name in ("assignments", "counts", "mean_numerators", "means", "boundaries"):
                assert np.array_equal(prev[name], s[name]), name
            assert prev["K"] == s["K"]
    if not (shape == kr.SHAPES[4] and init == "rand"):
        assert seen >= 1


@pytest.mark.parametrize("shape,init", CASES, ids=IDS)
def test_refit_agrees_with_the_references_fit_where_nothing_is_founded(shape, init):
    """kmeans_batch_refit against oracle KMeans.fit(1, consider_unassigned=False) from the same state, at every refit of the
    schedule that founds no component: equal assignments, K, counts and n_mean_updates; the numerators differ by the order
    of the summation only.  Bound: `fit` reaches a numerator by at most n additions and subtractions of rows, the refit by
    at most n additions, n <= the number of tokens (< 2^9 here), each rounding to half an ulp of a partial sum no larger
    than the sum of |x| -- far inside 64 ulp of the largest |numerator| unless the sums cancel, which these corpora
    (clusters away from the origin) do not."""
    import copy
    n_blocks = shape[5]
    seg = _fresh(shape, init)
    checked = 0

    def compare():
        nonlocal checked
        twin = copy.deepcopy(seg)
        info = {}
        moved, K, _ = kr.kmeans_batch_refit(seg, n_blocks, info)
        if info["founding"]:
            return
        rec = twin.acoustic_model.fit(1, consider_unassigned=False)
        ca, cb = seg.acoustic_model.components, twin.acoustic_model.components
        assert rec["n_mean_updates"][0] == moved
        assert np.array_equal(ca.assignments, cb.assignments)
        assert ca.K == cb.K == K
        assert np.array_equal(ca.counts, cb.counts)
        big = np.abs(cb.mean_numerators).max()
        assert np.abs(ca.mean_numerators - cb.mean_numerators).max() <= 64 * np.spacing(big)
        checked += 1

    compare()
    for _ in range(3):
        no.kmeans_batch_sweep(seg, n_blocks=n_blocks)
        compare()
        compare()
    assert checked >= 1


def test_library_exports_the_refit_entry_points_at_the_unchanged_abi():
    from segmentalist_amd import _abi
    if not os.path.exists(_abi.LIB_PATH):
        _abi.build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "segk.h")).read()
    for name in ("segk_kmeans_refit_scratch_words", "segk_kmeans_refit_collect", "segk_kmeans_refit_apply",
                 "segk_kmeans_hint_relabel", "segk_kmeans_refit_record"):
        assert hasattr(lib, name), name
        assert name in _abi.SIGNATURES
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert lib.segk_abi_version() == _abi.ABI_VERSION == 15
    assert int(re.search(r"#define\s+SEGK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 15
    lib.segk_kmeans_refit_scratch_words.restype = ctypes.c_int64
    lib.segk_kmeans_refit_scratch_words.argtypes = [ctypes.c_int64]
    assert lib.segk_kmeans_refit_scratch_words(1) == 1 and lib.segk_kmeans_refit_scratch_words(1025) == 2

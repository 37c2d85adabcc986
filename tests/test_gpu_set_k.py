"""
GPU tests of `FBGMM.set_K(K, reassign=True, sync=...)`: the serial form against the vectors recorded from the reference
(tests/golden/set_k.npz: every recorded draw is at least 1e-6 in probability clear of the cumulative edges, tests/test_set_k_cpu.py,
so labels must coincide), the batch form against the NumPy specification tests/fbgmm_set_k.py, the shapes that can break the
listed kernel, and the refusals.  Statistics are held to 1e-13, values to the 1e-9 of the fp64 path.
"""
import ctypes as C
import random

import numpy as np
import numpy.testing as npt
import pytest

from tests import fbgmm_items as fi
from tests import fbgmm_set_k as sk

pytestmark = pytest.mark.gpu
RTOL = 1e-9
MAIN = [n for n in sk.CASES if n != sk.EARLY]
DEV_STATE = ("counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "K", "assignments")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


def product_factory(case, X, a):
    return sk.product_model(case, assignments=a, B=3, S=2)


def product_set_k(model, K, reassign, **kw):
    """model.set_K with the assignments it hands to setup_components recorded: (kept labels, assignments after relabelling)
    as the product formed them"""
    old = np.array(model.components.assignments)
    seen = {}
    inner = model.setup_components

    def setup(K_new, assignments="rand", X=None):
        seen["assign"] = np.array(assignments)
        return inner(K_new, assignments, X)
    model.setup_components = setup
    try:
        model.set_K(K, reassign, **kw)
    finally:
        del model.setup_components
    new = seen["assign"]
    if new.max() + 1 < K or np.array_equal(new, old):
        return None, new
    keep = [int(old[np.flatnonzero(new == r)[0]]) for r in range(K)]
    return keep, new


def same_device_state(gpu, a, b):
    for nm in DEV_STATE:
        assert gpu.equal(getattr(a.components.dev, nm), getattr(b.components.dev, nm)), nm


# ------------------------------------------------------------------------------------------------ serial form
@pytest.mark.parametrize("name", MAIN)
def test_serial_form_against_the_reference(gpu, golden, name):
    g = golden("set_k")
    case = sk.CASES[name]
    cov = case[0]
    res = sk.run_case(name, product_factory, product_set_k)
    for key in ("pre_K", "pre_counts", "pre_assign", "keep", "relabel_assign", "post_K", "post_K_max", "post_counts", "post_assign"):
        assert np.array_equal(res[key], g[name + "_" + key]), key
    assert float(res["random_after"]) == float(g[name + "_random_after"])           # the stream ends at the same position
    k = int(res["post_K"])
    for nm in sk.STATS[cov][0]:
        npt.assert_allclose(res["post_" + nm][:k], g["%s_post_%s" % (name, nm)][:k], rtol=1e-13, atol=1e-300, err_msg=nm)
    worst = 0.0
    for nm in sk.STATS[cov][1] + ("log_marg", "log_marg_i"):
        got, want = np.asarray(res["post_" + nm]), g["%s_post_%s" % (name, nm)]
        if got.ndim and got.shape[0] == k == len(want):
            got, want = got[:k], want[:k]
        worst = max(worst, rel(got, want))
    print("%s: values %.3g" % (name, worst))
    assert worst <= RTOL


@pytest.mark.parametrize("name", ["dg_D16", "fc_D3"])
def test_sweeps_of_both_kinds_run_after_the_serial_form(gpu, name):
    """the batch arguments survive setup_components: a serial sweep, then batch sweeps on a sweeper of the object's B x S"""
    case = sk.CASES[name]
    m = sk.product_model(case, B=3, S=2)
    random.seed(3)
    m.set_K(case[6])
    c = m.components
    assert c.K == c.K_max == case[6] and np.all(c.assignments >= 0)
    m.gibbs_sample(1)
    rec = m.gibbs_sample(2, sync="batch")
    sw = m._get_sweeper()
    assert (sw.B, sw.S) == (3, 2) and sw.sweep_index == 2 and sw.df is m.components.dev
    assert len(rec["log_marg"]) == 2 and np.all(np.isfinite(rec["log_marg"]))
    m.components.dev.check_status()
    assert int(m.components.counts.sum()) == case[4]


@pytest.mark.parametrize("sync", ["sequential", "batch"])
def test_early_branch_equals_a_fresh_model(gpu, golden, sync):
    g = golden("set_k")
    name = sk.EARLY
    case = sk.CASES[name]
    X, a = sk.case_inputs(case)
    m = sk.product_model(case, B=3, S=2)
    assert np.array_equal(m.components.counts, g[name + "_pre_counts"]) and m.components.K == int(g[name + "_pre_K"]) <= case[6]
    state = random.getstate()
    m.set_K(case[6], sync=sync)
    assert random.getstate() == state                          # no uniform is consumed
    fresh = sk.product_model(case, assignments=a, B=3, S=2, K_max=case[6])
    m.materialise()
    assert m.components.K_max == case[6] and m.components.K == int(g[name + "_pre_K"])
    same_device_state(gpu, m, fresh)
    assert m._get_sweeper().in_batch_state == (sync == "batch")
    m.gibbs_sample(1)                                          # (the reference fails here)
    m.components.dev.check_status()


def test_the_specification_function_runs_on_the_device_class(gpu, golden):
    """sk.set_k -- the reference's method as a function -- on the device class: item after item through
    gibbs_sample_inside_loop_i, the labels of the recorded reference and of FBGMM.set_K's one kernel call"""
    g = golden("set_k")
    name = "fx_D3"
    case = sk.CASES[name]
    X, a = sk.case_inputs(case)
    random.seed(500 + case[5])
    m = sk.product_model(case)
    keep, new, orphans = sk.set_k(m, case[6], True)
    assert keep == g[name + "_keep"].tolist() and np.array_equal(new, g[name + "_relabel_assign"])
    assert np.array_equal(m.components.assignments, g[name + "_post_assign"])
    assert random.random() == float(g[name + "_random_after"])


# ------------------------------------------------------------------------------------------------ batch form
def check_batch(gpu, m, spec, what, probe=None):
    """slots, likelihoods, partial sums of the device's batch state against the specification's"""
    sw = m._get_sweeper()
    gpu.cuda.synchronize()
    m.components.dev.check_status()
    assert sw.in_batch_state
    assert np.array_equal(sw.slot.cpu().numpy(), spec.slot), what
    assert np.array_equal(sw.n_new.cpu().numpy(), (spec.slot >= 0).astype(np.int32)), what
    if probe is not None:
        got = probe.cpu().numpy()
        worst = max([rel(got[i], ll) for i, ll in spec.ll_log.items()] or [0.0])
        print("%s likelihoods %.3g over %d orphans" % (what, worst, len(spec.ll_log)))
        assert worst <= RTOL, what
        rest = np.ones(len(got), bool)
        rest[list(spec.ll_log)] = False
        assert np.isnan(got[rest]).all(), what                 # only the listed items were evaluated
    worst = 0.0
    for s in range(spec.S):
        for b in range(spec.B):
            cnt, sx, sxx = sw.cell_partials(b, s)
            rc, rx, rxx = spec._partial(s, b)
            assert np.array_equal(cnt, rc), what
            worst = max(worst, rel(sx, rx), rel(sxx, rxx))
    print("%s partials %.3g" % (what, worst))
    assert worst <= 1e-13, what


def batch_pair(gpu, case, a, B, S, sweeps_before=0, **kw):
    """(kept labels, relabelled assignments, orphans, specification after the pass, device model after the same pass with the
    likelihood probe) -- the device pass through the sweeper's own method, on a model cut with reassign=False"""
    cov, K = case[0], case[6]
    X, _ = sk.case_inputs(case)
    am = fi.spec_model(cov, X, case[3], a.copy())
    m = sk.product_model(case, assignments=a.copy(), B=B, S=S, **kw)
    for s in range(sweeps_before):                             # batch sweeps first: the counter is carried over the cut
        m.batch_sweep_async()
    if sweeps_before:
        m.materialise()
        am = fi.spec_model(cov, X, case[3], np.array(m.components.assignments))
    old = np.array(m.components.assignments)
    keep, new, orphans, spec = sk.batch_set_k(am, cov, K, True, B, S, sweep_index=sweeps_before, ll_log=True)
    state = random.getstate()
    got_keep, got_new = product_set_k(m, K, False, sync="batch")
    assert got_keep == keep and np.array_equal(got_new, new)
    sw = m._get_sweeper()
    assert sw.in_batch_state and sw.sweep_index == sweeps_before
    sw.probe_ll = gpu.full((len(a), K), float("nan"), dtype=gpu.float64, device="cuda")
    sw.reassign_orphans(old)
    assert random.getstate() == state                          # no random.random() is consumed
    assert sw.sweep_index == sweeps_before + 1
    return keep, new, orphans, spec, m


def same_view_at_K(gpu, m, spec, case, B, S):
    """materialise(): bit for bit the model constructed from the resulting assignments at K_max = K"""
    canon, K = spec.canonical()
    m.materialise()
    c = m.components
    assert c.K == K and np.array_equal(c.assignments, canon)
    fresh = sk.product_model(case, assignments=canon, B=B, S=S, K_max=case[6])
    same_device_state(gpu, m, fresh)
    assert m._get_sweeper().in_batch_state


@pytest.mark.parametrize("name", list(sk.BATCH_CASES))
def test_batch_form_against_the_specification(gpu, name):
    case = sk.BATCH_CASES[name]
    B, S = case[8], case[9]
    X, a = sk.case_inputs(case)
    before = 1 if name == "dg_D16_4x2" else 0
    keep, new, orphans, spec, m = batch_pair(gpu, case, a, B, S, sweeps_before=before)
    check_batch(gpu, m, spec, name, probe=m._get_sweeper().probe_ll)
    assert np.all(spec.slot[a == -1] == -1)
    same_view_at_K(gpu, m, spec, case, B, S)
    # the whole call in one go gives the same state, and the next batch sweep takes the next value of the counter
    m2 = sk.product_model(case, B=B, S=S)
    for s in range(before):
        m2.batch_sweep_async()
    m2.set_K(case[6], sync="batch")
    assert gpu.equal(m2._get_sweeper().slot, m._get_sweeper().slot) and gpu.equal(m2._get_sweeper().partials, m._get_sweeper().partials)
    m2.batch_sweep_async()
    spec.ll_log = None
    spec.sweep(before + 1, 1.0, True)
    gpu.cuda.synchronize()
    assert m2._get_sweeper().sweep_index == before + 2
    assert np.array_equal(m2._get_sweeper().slot.cpu().numpy(), spec.slot)


def test_batch_form_without_reassign(gpu):
    case = sk.BATCH_CASES["dg_D16_4x2"]
    X, a = sk.case_inputs(case)
    m = sk.product_model(case, B=4, S=2)
    keep, new = sk.rank_and_relabel(np.bincount(a, minlength=case[3]), a, case[6])
    m.set_K(case[6], reassign=False, sync="batch")
    sw = m._get_sweeper()
    assert sw.in_batch_state and sw.sweep_index == 0
    assert np.array_equal(sw.slot.cpu().numpy(), new)
    m.materialise()
    canon = np.array(m.components.assignments)
    assert np.array_equal(canon >= 0, new >= 0) and m.components.K == case[6]


# name -> (cov, dtype, D, K_max, N, seed, target K, 0.0, B, S, orphans per (slice, block) cell)
LAYOUTS = {
    # a block with 0, 1, 63, 64, 65 orphans (the tile edges), one whose items are all orphans
    "edges_4x2": ("diag", "float32", 16, 12, 600, 31, 2, 0.0, 4, 2, [[0, 1, 63, 64], [65, "all", 2, 0]]),
    "slice_with_none_2x2": ("fixed", "float64", 3, 12, 300, 32, 2, 0.0, 2, 2, [[5, 70], [0, 0]]),
    "one_orphan_1x1": ("fixed", "float32", 3, 3, 70, 33, 2, 0.0, 1, 1, [[1]]),
    "fullcov_edges_2x2": ("full", "float32", 16, 12, 400, 34, 2, 0.0, 2, 2, [[64, 0], [65, 1]]),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_orphan_layouts(gpu, name):
    case = LAYOUTS[name]
    B, S, cells = case[8], case[9], case[10]
    a = sk.layout_assignments(case[4], case[3], case[6], B, S, cells, case[5])
    keep, new, orphans, spec, m = batch_pair(gpu, case, a, B, S)
    # the layout is the one asked for
    for s in range(S):
        for b in range(B):
            lo, hi = spec.ranges[s][b]
            n = sum(1 for i in orphans if lo <= i < hi)
            assert n == (hi - lo if cells[s][b] == "all" else cells[s][b]), (s, b)
    check_batch(gpu, m, spec, name, probe=m._get_sweeper().probe_ll)
    same_view_at_K(gpu, m, spec, case, B, S)


def workspace_case():
    """D = 160, K = 50: rows and staged slots take 122 880 bytes of LDS and a tile's logits 25 600 more than the 144 KiB hold,
    so they live in the workspace; sizes 21..80 for the 60 components, the ten smallest go (255 orphans)"""
    case = ("fixed", "float32", 160, 60, 3030, 41, 50, 0.0, 1, 2)
    a = np.random.RandomState(41).permutation(np.repeat(np.arange(60), 21 + np.arange(60)))
    return case, a.astype(np.int64)


def test_logits_in_the_bounded_workspace(gpu, monkeypatch):
    """with the workspace bound at 1 MiB a launch holds 40 tiles and the block's 48 are walked in two launches"""
    monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")
    case, a = workspace_case()
    tiles = 2 * ((1515 + fi.TILE - 1) // fi.TILE)
    assert tiles > (1 << 20) // (fi.TILE * case[6] * 8)
    keep, new, orphans, spec, m = batch_pair(gpu, case, a, 1, 2)
    assert len(orphans) == 255
    check_batch(gpu, m, spec, "bounded workspace", probe=m._get_sweeper().probe_ll)


def test_float32_model_takes_the_fp64_pass(gpu):
    """score_precision="f32": the orphan pass is fp64 all the same -- the fp64 specification's slots and likelihoods"""
    case = sk.BATCH_CASES["dg_D16_4x2"]
    X, a = sk.case_inputs(case)
    keep, new, orphans, spec, m = batch_pair(gpu, case, a, 4, 2, score_precision="f32")
    assert m._get_sweeper().score_diag32
    check_batch(gpu, m, spec, "f32 model", probe=m._get_sweeper().probe_ll)
    m.batch_sweep_async()                                      # the float32 sweeps go on from there
    gpu.cuda.synchronize()
    m.components.dev.check_status()


@pytest.mark.parametrize("name", ["dg_D16", "fc_D16_f64"])
def test_both_forms_keep_the_same_components(gpu, name):
    case = sk.CASES[name]
    X, a = sk.case_inputs(case)
    ser, bat = sk.product_model(case, B=4, S=2), sk.product_model(case, B=4, S=2)
    random.seed(9)
    ks, ns = product_set_k(ser, case[6], True, sync="sequential")
    kb, nb_ = product_set_k(bat, case[6], True, sync="batch")
    assert ks == kb and np.array_equal(ns, nb_)
    bat.materialise()
    stay = ns >= 0
    assert np.array_equal(ser.components.assignments[stay], bat.components.assignments[stay])
    assert ser.components.K == bat.components.K == case[6]
    assert np.all(ser.components.assignments[a >= 0] >= 0) and np.all(bat.components.assignments[a >= 0] >= 0)
    assert not ser._sweeper and bat._get_sweeper().in_batch_state


# ------------------------------------------------------------------------------------------------ refusals
def one_landmark_corpus(X):
    keys = ["u%07d" % i for i in range(len(X))]
    return ({k: X[i:i + 1] for i, k in enumerate(keys)}, {k: np.array([0]) for k in keys}, {k: [1] for k in keys},
            {k: [1] for k in keys}), keys


def test_refusals(gpu):
    from segmentalist_amd import _abi
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    # the acoustic model of a segmenter: refused before anything changes
    X = fi.case_data(3, 7, 40, 5, "float32")
    corpus, keys = one_landmark_corpus(X)
    np.random.seed(2)
    seg = UnigramAcousticWordseg(FBGMM, fi.ALPHA, 7, FixedVarPrior(*fi.prior_params("fixed", 3)), *corpus,
                                 covariance_type="fixed", n_slices_max=1, beta_sent_boundary=-1)
    am = seg.acoustic_model
    comps, dev = am.components, am.components.dev
    before = {nm: getattr(dev, nm).clone() for nm in DEV_STATE}
    state = random.getstate()
    for sync in (None, "sequential", "batch"):
        with pytest.raises(SegkError, match="segmenter"):
            am.set_K(2, sync=sync)
    assert am.components is comps and comps.dev is dev and random.getstate() == state
    for nm in DEV_STATE:
        assert gpu.equal(getattr(dev, nm), before[nm]), nm
    # the library entry: a language model and a corpus with span tables, nothing launched
    case = sk.BATCH_CASES["fx_D3_1x1"]
    m = sk.product_model(case, B=2, S=2)
    old = np.array(m.components.assignments)
    m.set_K(case[6], reassign=False, sync="batch")
    sw = m._get_sweeper()
    gpu.cuda.synchronize()
    L, ctx, cp, fp, bp, st = sw._args()
    was_t = gpu.from_numpy(old.astype(np.int32)).cuda()
    was = _abi.ptr(was_t)

    def untouched(snapshot=[]):
        now = [sw.slot.clone(), sw.n_new.clone(), sw.partials.clone()]
        if not snapshot:
            snapshot.extend(now)
        return all(gpu.equal(x, y) for x, y in zip(now, snapshot)) and sw.sweep_index == 0
    assert untouched()
    f_lm = _abi.FbgmmDev.from_buffer_copy(sw.f)
    f_lm.lm_unigram = m.components.dev.counts.data_ptr()
    rc = L.segk_fbi_assign_orphans(ctx, cp, C.byref(f_lm), bp, 0, sw.S, 0, sw._n_items[0], 0, was, _abi.ptr(sw.new_tok),
                                   _abi.ptr(sw.n_new), None, 0, st)
    assert rc == _abi.SEGK_ERR_UNSUPPORTED and "language model" in L.segk_last_error().decode()
    rc = L.segk_fbi_assign_orphans(ctx, seg._df._cp(), fp, bp, 0, sw.S, 0, sw._n_items[0], 0, was, _abi.ptr(sw.new_tok),
                                   _abi.ptr(sw.n_new), None, 0, st)
    assert rc != 0 and "corpus of items" in L.segk_last_error().decode()
    gpu.cuda.synchronize()
    assert untouched()
    m.components.dev.check_status()

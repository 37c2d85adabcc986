"""
GPU tests of the batch sweeps of the stand-alone mixture model (`FBGMM(..., sync=...)`, `gibbs_sample(..., sync="batch")`,
`batch_sweep_async` / `materialise`) against the NumPy specification tests/fbgmm_items.py.
tests/test_fbgmm_items_cpu.py shows that on these cases every draw is at least 1e-6 in probability clear of the cumulative
edges, so slots must coincide; likelihoods are held to the 1e-9 of the fp64 path, partial sums to 1e-13.
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests import fbgmm_items as fi

pytestmark = pytest.mark.gpu
RTOL = 1e-9


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


def pair(case, probe=None):
    am, spec = fi.spec_of(case)
    m = fi.product_of(case)
    assert np.array_equal(m.components.assignments, spec.slot)
    if probe is not None:
        m._get_sweeper().probe_ll = probe.zeros((len(spec.slot), spec.K_max), dtype=probe.float64, device="cuda")
    return spec, m


def sweep_both(gpu, spec, m, index, temp=1.0, consider_unassigned=True, what=""):
    """One sweep of both; everything the issue holds equal after a sweep."""
    sw = m._get_sweeper()
    spec.ll_log = {} if sw.probe_ll is not None else None
    spec.sweep(index, temp, consider_unassigned)
    m.batch_sweep_async(temp, consider_unassigned)
    gpu.cuda.synchronize()
    m.components.dev.check_status()
    assert sw.sweep_index == index + 1
    assert np.array_equal(sw.slot.cpu().numpy(), spec.slot), what
    if sw.probe_ll is not None:
        got = sw.probe_ll.cpu().numpy()
        worst = max([rel(got[i], ll) for i, ll in spec.ll_log.items()] or [0.0])
        print("%s likelihoods %.3g over %d items" % (what, worst, len(spec.ll_log)))
        assert worst <= RTOL, what
    worst = 0.0
    for s in range(spec.S):
        for b in range(spec.B):
            cnt, sx, sxx = sw.cell_partials(b, s)
            rc, rx, rxx = spec._partial(s, b)
            assert np.array_equal(cnt, rc), what
            worst = max(worst, rel(sx, rx), rel(sxx, rxx))
    print("%s partials %.3g" % (what, worst))
    assert worst <= 1e-13, what


def same_view(m, spec, case):
    """materialise(): assignments and K are canonical(); the serial statistics are, bit for bit, those of a fresh model
    constructed from those assignments.  Returns the fresh model."""
    import torch
    canon, K = spec.canonical()
    c = m.components
    assert c.K == K and np.array_equal(c.assignments, canon)
    fresh = fi.product_of(case, assignments=canon)
    a, b = c.dev, fresh.components.dev
    for nm in ("counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "K", "assignments"):
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm
    return fresh


@pytest.fixture(scope="module")
def finished(gpu):
    """name -> (spec, model) after the sweeps of test_sweeps (later tests go on from there)"""
    return {}


@pytest.mark.parametrize("name", list(fi.CASES))
def test_sweeps(gpu, finished, name):
    case = fi.CASES[name]
    spec, m = pair(case, probe=gpu)
    for s, temp in enumerate(case[8]):
        sweep_both(gpu, spec, m, s, temp, True, "%s sweep %d" % (name, s))
    finished[name] = (spec, m)


@pytest.mark.parametrize("name", fi.UNASSIGNED)
def test_sweeps_without_the_unassigned(gpu, finished, name):
    case = fi.CASES[name]
    spec, m = pair(case, probe=gpu)
    for s, temp in enumerate(case[8]):
        sweep_both(gpu, spec, m, s, temp, False, "%s assigned only, sweep %d" % (name, s))
    assert np.count_nonzero(spec.slot < 0) >= 1
    finished[name + "/assigned"] = (spec, m)


def test_logits_workspace_walked_in_several_launches(gpu, monkeypatch):
    """K_max = 300: a tile's logits do not fit in LDS.  With the workspace bound at 1 MiB a launch holds six tiles and the
    block's eight are walked in two launches: the same slots, likelihoods and partial sums."""
    monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")
    case = fi.CASES["fx_D100_K300_Thalf"]
    spec, m = pair(case, probe=gpu)
    tiles = sum((hi - lo + fi.TILE - 1) // fi.TILE for row in spec.ranges for (lo, hi) in row[:1])
    assert tiles > (1 << 20) // (fi.TILE * case[3] * 8)
    for s, temp in enumerate(case[8]):
        sweep_both(gpu, spec, m, s, temp, True, "bounded workspace, sweep %d" % s)


@pytest.mark.parametrize("name", ["dg_D39_K65_n257", "fx_D39_K65_un/assigned", "fc_D39_K65", "fx_D3_K7_n5_8x8"])
def test_materialise(gpu, finished, name):
    base = name.split("/")[0]
    if name not in finished:
        (test_sweeps_without_the_unassigned if "/" in name else test_sweeps)(gpu, finished, base)
    spec, m = finished[name]
    m.materialise()
    same_view(m, spec, fi.CASES[base])
    assert m._get_sweeper().in_batch_state
    assert np.array_equal(m._get_sweeper().slot.cpu().numpy(), spec.slot)          # (the batch state is not touched)


@pytest.mark.parametrize("name", ["fx_D39_K7_n255", "dg_D39_K7_un", "fc_D3_K7_n5_2x2"])
def test_record_of_gibbs_sample_batch(gpu, name):
    """gibbs_sample(2, sync="batch", anneal_schedule="linear"): after every sweep the record holds the host expressions on
    a fresh model of the specification's canonical assignments."""
    case = fi.CASES[name]
    spec, m = pair(case)
    state = random.getstate()
    rec = m.gibbs_sample(2, sync="batch", anneal_schedule="linear")
    assert random.getstate() == state                         # no random.random() is consumed
    temps = [float(t) for t in 1. / np.linspace(0.1, 1, 2)]
    assert sorted(rec) == ["anneal_temp", "components", "log_marg", "log_prob_X_given_z", "log_prob_z", "sample_time"]
    for s, temp in enumerate(temps):
        spec.sweep(s, temp, True)
        canon, K = spec.canonical()
        fresh = fi.product_of(case, assignments=canon)
        want = {"log_marg": fresh.log_marg(), "log_prob_z": fresh.log_prob_z(), "log_prob_X_given_z": fresh.log_prob_X_given_z(),
                "anneal_temp": temp}
        for k, v in want.items():
            print("%s sweep %d record %s: %.17g against %.17g" % (name, s, k, rec[k][s], v))
            assert abs(rec[k][s] - v) <= RTOL * max(1.0, abs(v)), (k, s)
        assert rec["components"][s] == K
    same_view(m, spec, case)


def test_object_in_batch_mode(gpu):
    """FBGMM(..., sync="batch"): gibbs_sample without a sync argument runs batch sweeps"""
    case = fi.CASES["dg_D39_K65_n257"]
    am, spec = fi.spec_of(case)
    m = fi.product_of(case, sync="batch")
    m.gibbs_sample(2)
    for s in range(2):
        spec.sweep(s, 1.0, True)
    assert np.array_equal(m._get_sweeper().slot.cpu().numpy(), spec.slot)
    same_view(m, spec, case)


def test_two_sweeps_enqueued_back_to_back(gpu):
    case = fi.CASES["fx_D39_K130_n600"]
    _, a = pair(case)
    _, b = pair(case)
    a.batch_sweep_async()
    a.batch_sweep_async()
    for _ in range(2):
        b.batch_sweep_async()
        gpu.cuda.synchronize()
    gpu.cuda.synchronize()
    sa, sb = a._get_sweeper(), b._get_sweeper()
    assert sa.sweep_index == sb.sweep_index == 2
    assert gpu.equal(sa.slot, sb.slot) and gpu.equal(sa.partials, sb.partials) and gpu.equal(sa.n_new, sb.n_new)
    a.components.dev.check_status()


@pytest.mark.parametrize("name", ["dg_D39_K65_n257", "fc_D39_K65"])
def test_serial_sweep_between_batch_sweeps(gpu, name):
    case = fi.CASES[name]
    spec, m = pair(case)
    sweep_both(gpu, spec, m, 0, what="before the serial sweep")
    random.seed(5)
    m.gibbs_sample(1)                                       # the serial chain from the materialised state
    sw = m._get_sweeper()
    assert not sw.in_batch_state
    # the specification rebuilt from the serial result
    spec.slot = np.array(m.components.assignments, dtype=spec.slot.dtype)
    spec.P = [[spec._partial(s, b) for b in range(spec.B)] for s in range(spec.S)]
    sweep_both(gpu, spec, m, sw.sweep_index, what="after the serial sweep")
    assert sw.in_batch_state
    # every serial-mode method leaves batch mode first
    i = int(np.where(spec.slot >= 0)[0][0])
    m.log_marg_i(i)
    assert not sw.in_batch_state
    assert np.array_equal(m.components.assignments, spec.canonical()[0])


def one_landmark_corpus(X):
    keys = ["u%07d" % i for i in range(len(X))]
    return ({k: X[i:i + 1] for i, k in enumerate(keys)}, {k: np.array([0]) for k in keys}, {k: [1] for k in keys},
            {k: [1] for k in keys}), keys


@pytest.mark.parametrize("name", ["fx_D39_K7_n255", "dg_D39_K65_n257", "fc_D39_K65"])
def test_cross_route_through_the_segmenter(gpu, name):
    """The same rows as one-landmark utterances through UnigramAcousticWordseg's batch sweeps (fp64; same B, S, seed; the
    components' draws at the sweep's temperature): the slots after every sweep are the new path's, bit for bit."""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    case = fi.CASES[name]
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, a = fi.make_inputs(case)
    corpus, keys = one_landmark_corpus(X)
    prior = FixedVarPrior(*fi.prior_params(cov, D)) if cov == "fixed" else NIW(*fi.prior_params(cov, D))
    np.random.seed(1)
    seg = UnigramAcousticWordseg(FBGMM, fi.ALPHA, K, prior, *corpus, seed_boundaries_dict={k: [1] for k in keys},
                                 seed_assignments_dict={k: [int(a[i])] for i, k in enumerate(keys)}, covariance_type=cov,
                                 n_slices_min=0, n_slices_max=1, beta_sent_boundary=-1, lms=fi.LMS, sync="sequential",
                                 n_gibbs_blocks=B, n_stat_blocks=S, batch_seed=fi.BATCH_SEED)
    assert np.array_equal(seg.acoustic_model.components.assignments, a)
    m = fi.product_of(case)
    for s, temp in enumerate(case[8]):
        seg.batch_sweep_async(temp, True)
        m.batch_sweep_async(temp, True)
        gpu.cuda.synchronize()
        seg._df.check_status()
        assert gpu.equal(seg._get_sweeper().slot, m._get_sweeper().slot), (name, s)


def test_refusals(gpu, monkeypatch):
    from segmentalist_amd import _abi, device
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    # a model that belongs to a segmenter
    case = fi.CASES["fx_D3_K7_n5_8x8"]
    X, a = fi.make_inputs(case)
    corpus, keys = one_landmark_corpus(X)
    seg = UnigramAcousticWordseg(FBGMM, fi.ALPHA, 7, FixedVarPrior(*fi.prior_params("fixed", 3)), *corpus,
                                 covariance_type="fixed", n_slices_max=1, beta_sent_boundary=-1)
    with pytest.raises(SegkError, match=r"segmenter's gibbs_sample\(sync=\"batch\"\)"):
        seg.acoustic_model.gibbs_sample(1, sync="batch")
    with pytest.raises(SegkError, match="segmenter"):
        seg.acoustic_model.batch_sweep_async()
    # more than one rank
    m = fi.product_of(case)

    class TwoRanks(object):
        rank, world = 0, 2
    monkeypatch.setattr(device, "get_comm", lambda group=None: TwoRanks())
    with pytest.raises(SegkError, match="one process"):
        m.batch_sweep_async()
    monkeypatch.undo()
    # full covariance beyond the batch kernels' limits: refused before anything is launched
    rs = np.random.RandomState(3)
    with pytest.raises(SegkError, match="D <= 64"):
        wide = FBGMM(rs.randn(80, 65).astype(np.float32), NIW(*fi.prior_params("full", 65)), fi.ALPHA, 4,
                     np.arange(80) % 2, covariance_type="full")
        wide.batch_sweep_async()
    many = FBGMM(rs.randn(12, 3).astype(np.float32), NIW(*fi.prior_params("full", 3)), fi.ALPHA, 1025, np.arange(12) % 3,
                 covariance_type="full")
    with pytest.raises(SegkError, match="K_max <= 1024"):
        many.batch_sweep_async()
    # a language model attached to the batch's copy of the model: refused by name, nothing launched
    m.batch_sweep_async()
    gpu.cuda.synchronize()
    sw = m._get_sweeper()
    L, ctx, cp, fp, bp, st = sw._args()
    f_lm = _abi.FbgmmDev.from_buffer_copy(sw.f)
    f_lm.lm_unigram = m.components.dev.counts.data_ptr()
    rc = L.segk_fbi_assign(ctx, cp, C.byref(f_lm), bp, 0, sw.S, 0, sw._n_items[0], 0, 1.0, 1, _abi.ptr(sw.new_tok),
                           _abi.ptr(sw.n_new), None, 0, st)
    assert rc == _abi.SEGK_ERR_UNSUPPORTED and "language model" in L.segk_last_error().decode()
    # a corpus with span tables is not a corpus of items
    rc = L.segk_fbi_assign(ctx, seg._df._cp(), fp, bp, 0, sw.S, 0, sw._n_items[0], 0, 1.0, 1, _abi.ptr(sw.new_tok),
                           _abi.ptr(sw.n_new), None, 0, st)
    assert rc != 0 and "corpus of items" in L.segk_last_error().decode()
    gpu.cuda.synchronize()
    m.components.dev.check_status()

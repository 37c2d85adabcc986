"""
GPU tests of `FBGMM.predict`, `score_samples` and `predict_log_proba` (`FbgmmItemSweeper.predict`; `segk_fbi_predict`,
`segk_fbi_predict_diag32`) against the NumPy specification tests/fbgmm_predict.py, kept on the device's own slots.
tests/test_fbgmm_predict_cpu.py shows that the specification is the serial oracle's value for an unassigned item appended to
X and that every label decision of these cases lies at least 1e-6 (relative) clear of its best competitor, so with
likelihoods held to 1e-9 the labels must coincide.
"""
import ctypes as C
import random

import numpy as np
import pytest

from tests import fbgmm_items as fi
from tests import fbgmm_items_f32 as f32
from tests import fbgmm_items_map as fm
from tests import fbgmm_predict as fp
from tests.test_gpu_fbgmm_items import one_landmark_corpus, rel

pytestmark = pytest.mark.gpu
RTOL = 1e-9
EDGE, EDGE32 = fp.EDGE, fp.EDGE32                        # K_max on either side of the placement rule at D = 39
SIZES = (0, 1, 63, 64, 65, 130)
SIZE_CASES = ["fx_D39_K7_n255", "dg_D100_K130_T10", "fc_D39_K65"]
WITNESS = ["fx_D39_K65_un", "dg_D39_K65_n257", "fc_D64_K7_un_T10"]
STATS = ("counts", "stat_a", "stat_b", "log_prod", "pred", "kconst", "K", "assignments")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def spec_on(case, slots, K_max=None):
    """the batch specification of the case's rows (K_max: the bank's size after set_K) holding `slots`"""
    cov, dtype, D, K, B, S, N, seed = case[:8]
    X, _ = fi.make_inputs(case)
    slots = np.asarray(slots, np.int64)
    am = fi.spec_model(cov, X, K if K_max is None else K_max, fm.partition(slots))
    spec = (fi.FullcovItems if cov == "full" else fi.FbgmmItems)(am, n_gibbs_blocks=B, n_stat_blocks=S, seed=fi.BATCH_SEED)
    spec.slot[:] = slots
    for s in range(spec.S):
        for b in range(spec.B):
            spec.P[s][b] = spec._partial(s, b)
    return spec


def device_slots(m):
    sw = m._get_sweeper()
    return sw.slot.cpu().numpy() if sw.in_batch_state else np.asarray(m.components.assignments)


def check(gpu, m, case, Xq, what, K_max=None, want=None):
    """One worker call with everything asked for and the probe, against the specification on the device's slots; then the
    three public methods.  Returns (specification's prediction, (labels, density, resp) of the device)."""
    sw = m._get_sweeper()
    K = m.components.K_max
    if want is None:
        census = fm.Census()
        want = fp.predict(spec_on(case, device_slots(m), K_max), Xq, census)
        # (a condition on the inputs, as in tests/test_fbgmm_predict_cpu.py: the labels can only be compared where it holds)
        assert census.gap_rel >= fp.MARGIN and census.tie_on_occupied == 0, (what, census.gap_rel)
    probe = gpu.full((len(Xq), K), float("nan"), dtype=gpu.float64, device="cuda")
    label, dens, resp = sw.predict(Xq, True, True, True, probe_ll=probe)
    gpu.cuda.synchronize()
    m.components.dev.check_status()
    ll = probe.cpu().numpy()
    assert np.array_equal(sw.cnt.cpu().numpy(), want.cnt.astype(np.float64)), what
    e_ll, e_d, e_r = rel(ll, want.ll), rel(dens, want.density), rel(resp, want.resp)
    n_new = int(np.count_nonzero(want.label == want.K))
    print("%s: M %d, K %d of %d; likelihoods %.3g, density %.3g, responsibilities %.3g; %d queries to an empty slot, %d labels"
          % (what, len(Xq), want.K, K, e_ll, e_d, e_r, n_new, len(set(want.label.tolist()))))
    assert label.dtype == np.int64 and dens.dtype == np.float64 and resp.shape == (len(Xq), K), what
    assert e_ll <= RTOL and e_d <= RTOL and e_r <= RTOL, what
    assert np.array_equal(label, want.label), what
    assert np.array_equal(m.predict(Xq), label), what
    assert np.array_equal(m.score_samples(Xq), dens), what
    assert np.array_equal(m.predict_log_proba(Xq), resp), what
    return want, (label, dens, resp)


@pytest.mark.parametrize("name", list(fi.CASES) + list(EDGE))
def test_three_states(gpu, name):
    """the initial serial state, the batch state after the case's sweeps (slots that are not canonical), a state after set_K"""
    case = fi.CASES.get(name) or EDGE[name]
    Xq = fp.query_rows(case)
    m = fi.product_of(case)
    check(gpu, m, case, Xq, "%s initial" % name)
    assert not m._get_sweeper().in_batch_state
    for temp in case[8]:
        m.batch_sweep_async(temp)
    assert m._get_sweeper().in_batch_state
    want, _ = check(gpu, m, case, Xq, "%s after %d sweeps" % (name, len(case[8])))
    assert m._get_sweeper().in_batch_state and m._get_sweeper().sweep_index == len(case[8])
    m.materialise()                                         # the labels are those of the reference's view
    assert m.components.K == want.K
    K_new = 3 if case[3] > 3 else case[3]
    state = random.getstate()
    random.seed(len(name))                                  # (the orphans' draws: the same state, and margins, on every run)
    m.set_K(K_new)
    random.setstate(state)
    assert m.components.K_max == K_new
    check(gpu, m, case, Xq, "%s after set_K(%d)" % (name, K_new), K_max=K_new)


@pytest.mark.parametrize("name", SIZE_CASES)
def test_query_sizes(gpu, name):
    case = fi.CASES[name]
    m = fi.product_of(case)
    m.batch_sweep_async(1.0)
    Xq = fp.query_rows(case)
    want = fp.predict(spec_on(case, device_slots(m)), Xq)
    K = case[3]
    for M in SIZES:
        label, dens, resp = m._get_sweeper().predict(Xq[:M], True, True, True)
        assert label.shape == (M,) and dens.shape == (M,) and resp.shape == (M, K), M
        assert label.dtype == np.int64 and dens.dtype == np.float64 and resp.dtype == np.float64
        assert np.array_equal(label, want.label[:M]), M
        assert rel(dens, want.density[:M]) <= RTOL and rel(resp, want.resp[:M]) <= RTOL, M
        assert m.predict(Xq[:M]).shape == (M,) and m.predict_log_proba(Xq[:M]).shape == (M, K)
    # only what is asked for is formed
    assert m._get_sweeper().predict(Xq, False, True, False)[0] is None
    assert m._get_sweeper().predict(Xq, True, False, False)[1:] == (None, None)


def test_eight_tiles_walked_in_two_launches(gpu, monkeypatch):
    """K_max = 1 100: a tile's logits (563 200 bytes) live in the workspace.  With its bound at 3 MiB a launch holds five
    tiles, and the eight of M = 512 are walked in two launches: the bits of the one launch, and the specification's values"""
    name = "fx_D39_K1100"
    case = fi.CASES[name]
    m = fi.product_of(case)
    Xq = fp.query_rows(case, M=512)
    tile = fi.TILE * case[3] * 8
    assert (3 << 20) // tile == 5 and (64 << 20) // tile >= 8 and fp.lds_bytes(case[2], case[3]) > fp.LDS_MAX
    one = m._get_sweeper().predict(Xq, True, True, True)
    monkeypatch.setenv("SEGK_FBI_Z_MIB", "3")
    want, two = check(gpu, m, case, Xq, "%s bounded workspace" % name)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


def test_full_covariance_query_walked_in_chunks(gpu, monkeypatch):
    """cov_type 2: with the table's bound at 1 MiB a chunk is 1 984 rows (31 tiles) of K_max = 65, M = 2 100 takes two: the same bits"""
    name = "fc_D39_K65"
    case = fi.CASES[name]
    m = fi.product_of(case)
    Xq = fp.query_rows(case, M=2100)
    assert ((1 << 20) // (case[3] * 8)) // fi.TILE * fi.TILE == 1984
    one = m._get_sweeper().predict(Xq, True, True, True)
    monkeypatch.setenv("SEGK_FBI_Z_MIB", "1")
    two = m._get_sweeper().predict(Xq, True, True, True)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    tail = np.r_[0:64, 1960:2100]                           # the first tile, and across the chunks' seam to the end
    want = fp.predict(spec_on(case, device_slots(m)), Xq[tail])
    assert np.array_equal(two[0][tail], want.label)
    assert rel(two[1][tail], want.density) <= RTOL and rel(two[2][tail], want.resp) <= RTOL


@pytest.mark.parametrize("name", WITNESS)
def test_second_witness_the_serial_kernels(gpu, name):
    """a throwaway device model over [X; Xq] with the queries at -1: log_marg_i of a dozen queries, map_assign_i of one"""
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    case = fi.CASES[name]
    cov, D, K = case[0], case[2], case[3]
    X, a = fi.make_inputs(case)
    Xq = fp.query_rows(case)
    m = fi.product_of(case)
    label, dens = m.predict(Xq), m.score_samples(Xq)
    prior = FixedVarPrior(*fi.prior_params(cov, D)) if cov == "fixed" else NIW(*fi.prior_params(cov, D))
    both = FBGMM(np.concatenate([X, Xq]), prior, fi.ALPHA, K, np.concatenate([a, np.full(len(Xq), -1, np.int64)]),
                 covariance_type=cov, lms=fi.LMS)
    rows = list(range(0, len(Xq), 11))
    assert len(rows) == 12
    got = np.array([both.log_marg_i(len(X) + r) for r in rows])
    print("%s: log_marg_i of %d appended rows, worst %.3g" % (name, len(rows), rel(dens[rows], got)))
    assert rel(dens[rows], got) <= RTOL
    r = 7                                                   # (a row scaled by 3)
    both.map_assign_i(len(X) + r)
    assert both.components.assignments[len(X) + r] == label[r]


def snapshot(m):
    c, sw = m.components, m._get_sweeper()
    out = {nm: getattr(c.dev, nm).clone() for nm in STATS}
    out.update(slot=sw.slot.clone(), partials=sw.partials.clone(), n_new=sw.n_new.clone())
    return out, (np.array(c.assignments), int(c.K), np.array(c.counts), sw.sweep_index, sw.in_batch_state)


def same(gpu, a, b, names=None):
    for nm in names or a[0]:
        assert gpu.equal(a[0][nm], b[0][nm]), nm
    assert np.array_equal(a[1][0], b[1][0]) and a[1][1] == b[1][1] and np.array_equal(a[1][2], b[1][2]) and a[1][3:] == b[1][3:]


@pytest.mark.parametrize("name", ["dg_D39_K7_un", "fx_D39_K130_n600", "fc_D39_K65"])
def test_read_only(gpu, name):
    case = fi.CASES[name]
    Xq = fp.query_rows(case)
    m, twin = fi.product_of(case), fi.product_of(case)
    state = random.getstate()
    # serial state: nothing of the model moves (the sweeper's own tables are rebuilt by whoever enters next)
    before = snapshot(m)
    m.predict(Xq), m.score_samples(Xq), m.predict_log_proba(Xq)
    gpu.cuda.synchronize()
    same(gpu, before, snapshot(m), STATS)
    assert not m._get_sweeper().in_batch_state
    # batch state: slots, partial sums and the counter stay, and the next sweep is the sweep without a predict
    for mm in (m, twin):
        mm.batch_sweep_async(1.0)
    before = snapshot(m)
    first = m._get_sweeper().predict(Xq, True, True, True)
    again = m._get_sweeper().predict(Xq, True, True, True)
    gpu.cuda.synchronize()
    same(gpu, before, snapshot(m))
    for a, b in zip(first, again):                          # two calls: the same bits
        assert np.array_equal(a, b)
    on_dev = m._get_sweeper().predict(gpu.from_numpy(Xq).cuda(), True, True, True, device_out=True)
    assert all(isinstance(t, gpu.Tensor) and t.is_cuda for t in on_dev)
    for a, b in zip(first, on_dev):
        assert np.array_equal(a, b.cpu().numpy())
    assert gpu.equal(m.predict(Xq, device_out=True), on_dev[0])
    for mm in (m, twin):
        mm.batch_sweep_async(1.0)
    gpu.cuda.synchronize()
    assert gpu.equal(m._get_sweeper().slot, twin._get_sweeper().slot)
    assert gpu.equal(m._get_sweeper().partials, twin._get_sweeper().partials)
    assert m._get_sweeper().sweep_index == twin._get_sweeper().sweep_index == 2
    assert random.getstate() == state
    m.components.dev.check_status()


@pytest.mark.parametrize("name", list(f32.CASES) + list(EDGE32))
def test_float32_likelihoods(gpu, monkeypatch, name):
    """score_precision="f32": the probed likelihoods within the 1e-4 contract of the fp64 specification (empty slots: the
    prior predictive at 1e-9); label, density and responsibilities are the fp64 functions of the device's OWN likelihoods"""
    case = f32.CASES.get(name) or EDGE32[name]
    Xq = fp.query_rows(case, M=512 if name == "dg_D39_K1100" else fp.M_QUERY)
    if name == "dg_D39_K1100":
        monkeypatch.setenv("SEGK_FBI_Z_MIB", "3")           # (eight tiles, five to a launch)
    m = f32.product_of(case)
    sw = m._get_sweeper()
    assert sw.score_diag32
    for state in ("initial", "swept"):
        if state == "swept":
            for temp in case[8]:
                m.batch_sweep_async(temp)
        K = case[3]
        probe = gpu.full((len(Xq), K), float("nan"), dtype=gpu.float64, device="cuda")
        label, dens, resp = sw.predict(Xq, True, True, True, probe_ll=probe)
        gpu.cuda.synchronize()
        m.components.dev.check_status()
        ll = probe.cpu().numpy()
        want = fp.predict(spec_on(case, device_slots(m)), Xq)
        occ = want.cnt > 0
        worst, worst_empty = f32.rel(ll[:, occ], want.ll[:, occ]), f32.rel(ll[:, ~occ], want.ll[:, ~occ])
        own = fp.functions_of(ll, want.cnt, fi.ALPHA, fi.LMS)
        print("%s %s: likelihoods %.3g (occupied), %.3g (empty); density %.3g, responsibilities %.3g on the device's own; "
              "%d labels differ from the fp64 specification's" % (name, state, worst, worst_empty, rel(dens, own.density),
                                                                    rel(resp, own.resp), np.count_nonzero(label != want.label)))
        assert np.isfinite(ll).all()
        assert worst <= f32.CONTRACT and worst_empty <= RTOL
        assert np.array_equal(label, own.label)
        assert rel(dens, own.density) <= RTOL and rel(resp, own.resp) <= RTOL


@pytest.mark.parametrize("name,transform", f32.SETTLED_RUNS, ids=f32.SETTLED_IDS)
def test_float32_likelihoods_on_settled_slots_of_thousands_of_items(gpu, name, transform):
    """segk_fbi_predict_diag32 where a float32 term's rounding is multiplied by a slot's count (f32.SETTLED): held-out rows of
    the case's own clusters against the settled start and against the state after a sweep, the specification on the device's
    own slots.  The rows must first show that they can tell the compensated term from the plain one: the emulation without the
    compensation misses the contract by 2 x or more on them."""
    case = f32.SETTLED[name]
    Xq = f32.settled_queries(case, transform)
    spec = f32.spec_of(case, transform)
    f32.discriminates(spec, "%s %s" % (name, transform), Xq)          # (first; once more below on each state's own slots)
    m = f32.product_of(case, transform)
    sw = m._get_sweeper()
    assert sw.score_diag32
    K = case[3]
    for state in ("settled", "swept"):
        if state == "swept":
            m.batch_sweep_async(1.0)
        probe = gpu.full((len(Xq), K), float("nan"), dtype=gpu.float64, device="cuda")
        label, dens, resp = sw.predict(Xq, True, True, True, probe_ll=probe)
        gpu.cuda.synchronize()
        m.components.dev.check_status()
        ll = probe.cpu().numpy()
        assert np.isfinite(ll).all()
        f32.set_slots(spec, device_slots(m))
        d = spec.derive(*spec.stats_excluding(-1))
        occ = d["active"]
        want, worst, emulated, plain = f32.compare(spec, d, Xq, ll)
        worst_empty = f32.rel(ll[:, ~occ], want[:, ~occ])
        own = fp.functions_of(ll, d["cnt"], fi.ALPHA, fi.LMS)
        print("%s %s %s: largest slot %d items; likelihoods %.3g (occupied), %.3g (empty) on %d held-out rows; the emulation "
              "%.3g, without the compensation %.3g; density %.3g, responsibilities %.3g on the device's own"
              % (name, transform, state, d["cnt"].max(), worst, worst_empty, len(Xq), emulated, plain, rel(dens, own.density),
                 rel(resp, own.resp)))
        assert plain >= f32.DISCRIMINATES * f32.CONTRACT                # (the inputs: or the rows prove nothing)
        assert worst <= f32.CONTRACT and worst_empty <= RTOL
        assert np.array_equal(label, own.label)
        assert rel(dens, own.density) <= RTOL and rel(resp, own.resp) <= RTOL


def test_refusals(gpu, monkeypatch):
    from segmentalist_amd import _abi, device
    from segmentalist_amd._abi import SegkError
    from segmentalist_amd.fbgmm import FBGMM
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.unigram_acoustic_wordseg import UnigramAcousticWordseg
    case = fi.CASES["fx_D3_K7_n5_8x8"]
    X, a = fi.make_inputs(case)
    Xq = fp.query_rows(case)
    # a model that belongs to a segmenter
    corpus, keys = one_landmark_corpus(X)
    seg = UnigramAcousticWordseg(FBGMM, fi.ALPHA, 7, FixedVarPrior(*fi.prior_params("fixed", 3)), *corpus,
                                 covariance_type="fixed", n_slices_max=1, beta_sent_boundary=-1)
    for call in ("predict", "score_samples", "predict_log_proba"):
        with pytest.raises(SegkError, match="segmenter"):
            getattr(seg.acoustic_model, call)(Xq)
    # more than one rank
    m = fi.product_of(case)

    class TwoRanks(object):
        rank, world = 0, 2
    monkeypatch.setattr(device, "get_comm", lambda group=None: TwoRanks())
    with pytest.raises(SegkError, match="one process"):
        m.predict(Xq)
    monkeypatch.undo()
    # another D
    for bad in (Xq[:, :2], np.zeros((4, 5), np.float32), Xq[0]):
        with pytest.raises(SegkError, match="query rows"):
            m.predict(bad)
    # through the C ABI, before any launch: the outputs keep their fill
    m.batch_sweep_async(1.0)
    sw = m._get_sweeper()
    L, ctx, cp, fp_, bp, st = sw._args()
    _abi.check(L.segk_fbb_prepare(ctx, cp, fp_, bp, -1, st))
    M, K = len(Xq), case[3]
    xq = gpu.from_numpy(Xq).cuda()
    prior_q = gpu.zeros(M, dtype=gpu.float64, device="cuda")
    label = gpu.full((M,), -7, dtype=gpu.int32, device="cuda")
    resp = gpu.zeros((M, K), dtype=gpu.float64, device="cuda")
    P = _abi.ptr

    def call(fn=L.segk_fbi_predict, c=cp, f=fp_, b=bp, x=xq, M=M, resp_ld=K):
        return fn(ctx, c, f, b, P(x), 3, M, P(prior_q), P(label), None, P(resp), resp_ld, None, 0, st)
    f_lm = _abi.FbgmmDev.from_buffer_copy(sw.f)
    f_lm.lm_unigram = m.components.dev.counts.data_ptr()
    assert call(f=C.byref(f_lm)) == _abi.SEGK_ERR_UNSUPPORTED and "language model" in L.segk_last_error().decode()
    f_fc = _abi.FbgmmDev.from_buffer_copy(sw.f)
    f_fc.cov_type, f_fc.K_max = 2, 1025
    assert call(f=C.byref(f_fc), resp_ld=1025) == _abi.SEGK_ERR_UNSUPPORTED and "K_max <= 1024" in L.segk_last_error().decode()
    assert call(fn=L.segk_fbi_predict_diag32) == _abi.SEGK_ERR_UNSUPPORTED and "diagonal components" in L.segk_last_error().decode()
    assert call(c=seg._df._cp()) not in (0, _abi.SEGK_ERR_UNSUPPORTED) and "span tables" in L.segk_last_error().decode()
    c_wide = _abi.Corpus.from_buffer_copy(sw.c)
    c_wide.D = 257
    assert call(c=C.byref(c_wide)) not in (0, _abi.SEGK_ERR_UNSUPPORTED) and "D <= 256" in L.segk_last_error().decode()
    assert call(x=None) not in (0, _abi.SEGK_ERR_UNSUPPORTED) and "query rows" in L.segk_last_error().decode()
    assert call(resp_ld=K - 1) not in (0, _abi.SEGK_ERR_UNSUPPORTED) and "leading dimension" in L.segk_last_error().decode()
    b_bare = _abi.FbatchDev.from_buffer_copy(sw.bt)
    b_bare.lconst = None
    assert call(b=C.byref(b_bare)) not in (0, _abi.SEGK_ERR_UNSUPPORTED) and "slot tables" in L.segk_last_error().decode()
    # the float32 form without its tables (a diagonal model with fp64 scores)
    dg = fi.product_of(fi.CASES["dg_D3_K7_n1"])
    dg.batch_sweep_async(1.0)
    sd = dg._get_sweeper()
    Ld, ctxd, cpd, fpd, bpd, std = sd._args()
    rc = Ld.segk_fbi_predict_diag32(ctxd, cpd, fpd, bpd, P(xq), 3, M, P(prior_q), P(label), None, None, 0, None, 0, std)
    assert rc not in (0, _abi.SEGK_ERR_UNSUPPORTED) and "tab32" in L.segk_last_error().decode()
    # no rows: nothing is launched, nothing is written
    assert call(M=0) == 0 and call(M=0, x=None) == 0
    gpu.cuda.synchronize()
    assert bool((label == -7).all()) and bool((resp == 0).all())
    assert m.predict(Xq[:0]).shape == (0,) and m.predict_log_proba(Xq[:0]).shape == (0, K)
    m.components.dev.check_status()

"""
The three consumers of segk_rows_by_label (segk_metrics.hip) -- k_fbgmm_init_stats, k_fc_init and k_metric_log_marg /
k_metric_reduce -- against tests/label_blocks.py where the assignment vector spans more than one block of rows: the loop
over blocks, the uneven block bounds b * n_emb / n_blocks, components that straddle a block edge or are absent from a
block, lists whose length is 8, 9 or 1 (eight rows per fetch, clamped tail), the cap of 64 blocks, blocks past 32 768 rows
whose keys the sort reads from memory, the sort's instantiations by bank size, and the float32 order of the
fixed-variance metric.  tests/test_label_blocks_cpu.py holds every case to the properties it is named for.

Models are built through the public classes from a given assignment vector.  After construction K, counts, assignments
and the two sufficient-statistic arrays must EQUAL the reference (the kernels claim the reference's order of additions
and the library is built with -ffp-contract=off); the derived arrays pass at 1e-13 (logdet_covars of the full-covariance
components at the 1e-9 of tests/test_gpu_fullcov.py: two factorisations).  record_metrics() passes at 1e-8, the
contract for record values, in the FBGMM form and, for fixed-variance models, in the urn form with two concentrations.
Full-covariance models get a corpus with one single-landmark utterance: segk_fbgmm_record_metrics takes cov_type 2 for a
segmenter's corpus only, and its value does not read the utterances.

Every case prints how far the product and the reference each lie from a longdouble evaluation; nothing is asserted on
that print (profiles/README.md "Label blocks" keeps the lines of the two largest cases).
"""
import random
import time

import numpy as np
import numpy.testing as npt
import pytest

from oracle import np_oracle as no
from tests import label_blocks as lb

pytestmark = pytest.mark.gpu
F32 = np.float32
STAT_NAMES = {"fixed": ("mu_N_numerators", "precision_Ns", "precision_preds", "log_prod_precision_preds"),
              "diag": ("m_N_numerators", "S_N_partials", "inv_vars", "log_prod_vars"),
              "full": ("m_N_numerators", "S_N_partials", None, "logdet_covars")}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _tag(name, D, K_max, cov, dtype):
    return "%s-D%d-K%d-%s-%s" % (name, D, K_max, cov, "f32" if dtype is F32 else "f64")


def _prior(cov, params):
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    return FixedVarPrior(*params) if cov == "fixed" else NIW(*params)


def _build(X, labels, K_max, cov, prior):
    from segmentalist_amd.device import DeviceCorpus
    from segmentalist_amd.fbgmm import FBGMM
    kw = {}
    if cov == "full":
        kw["_corpus"] = DeviceCorpus(X, vec_ids=np.zeros((1, 1), np.int32), durations=np.ones((1, 1)), lengths=[1])
    return FBGMM(X, _prior(cov, prior), lb.ALPHA, K_max, assignments=np.array(labels), covariance_type=cov, **kw)


def _same(got, want, what):
    """np.array_equal, with the size of the disagreement in the message."""
    if not np.array_equal(got, want):
        bad = got != want
        relerr = np.abs(got - want)[bad] / np.maximum(np.abs(want[bad]), 1e-300)
        raise AssertionError("%s: %d of %d entries differ from the reference, by up to %.3g relative (first at %s)"
                             % (what, bad.sum(), bad.size, relerr.max(), tuple(np.argwhere(bad)[0])))


def _record_matches(dev, tag, K, n_assigned, lpz, lpx, lpz_urn=None):
    got = dev.record_metrics()
    assert got[2] == K and got[3] == n_assigned, (tag, got)
    npt.assert_allclose(got[0], lpz, rtol=1e-8, err_msg=tag + " log_prob_z")
    npt.assert_allclose(got[1], lpx, rtol=1e-8, err_msg=tag + " log_prob_X_given_z")
    for a, want in zip(lb.URN_A, lpz_urn or ()):
        u = dev.record_metrics(urn=True, urn_a=a)
        assert u[2] == K and u[3] == n_assigned, (tag, a, u)
        npt.assert_allclose(u[0], want, rtol=1e-8, err_msg="%s urn a=%g log_prob_z" % (tag, a))
        npt.assert_allclose(u[1], lpx, rtol=1e-8, err_msg="%s urn a=%g log_prob_X_given_z" % (tag, a))
    return got


def _model_matches(name, D, K_max, cov, dtype):
    """Build the model of a case and hold it to the reference: statistics, derived arrays, record metrics."""
    tag = _tag(name, D, K_max, cov, dtype)
    c = lb.case(name, D, K_max, cov, dtype)
    st = c["stats"]
    t0 = time.time()
    fm = _build(c["X"], c["labels"], K_max, cov, c["prior"])
    comp = fm.components
    assert comp.K == st["K"], tag
    t_build = time.time() - t0
    _same(comp.counts, st["counts"], tag + " counts")
    _same(comp.assignments, st["assignments"], tag + " assignments")
    nm = STAT_NAMES[cov]
    _same(getattr(comp, nm[0]), st["a"], tag + " " + nm[0])
    _same(getattr(comp, nm[1]), st["b"], tag + " " + nm[1])
    if nm[2]:
        npt.assert_allclose(getattr(comp, nm[2]), st["derived"], rtol=1e-13, atol=0, err_msg=tag + " " + nm[2])
        npt.assert_allclose(getattr(comp, nm[3]), st["log_prod"], rtol=1e-13, atol=0, err_msg=tag + " " + nm[3])
    else:
        comp.dev.check_status()
        npt.assert_allclose(getattr(comp, nm[3]), st["log_prod"], rtol=1e-9, atol=1e-9, err_msg=tag + " " + nm[3])
    t0 = time.time()
    got = comp.dev.record_metrics()
    t_rec = time.time() - t0
    hz, hx = lb.metrics_hi(c["X"], c["labels"], K_max, cov, c["prior"], lb.ALPHA)
    print("label_blocks %s: construction %.3f s, record_metrics %.3f s; from the longdouble value: log_prob_X_given_z product "
          "%.2e reference %.2e, log_prob_z product %.2e reference %.2e"
          % (tag, t_build, t_rec, lb.rel(got[1], hx), lb.rel(c["lpx"], hx), lb.rel(got[0], hz), lb.rel(c["lpz"], hz)))
    _record_matches(comp.dev, tag, st["K"], int(st["counts"].sum()), c["lpz"], c["lpx"],
                    c["lpz_urn"] if cov == "fixed" else None)
    return fm


@pytest.mark.parametrize("name,D,K_max,cov,dtype", lb.models(), ids=lb.model_ids())
def test_statistics_and_record_metrics_vs_reference(gpu, name, D, K_max, cov, dtype):
    """Every row of the table (tests/label_blocks.py CASES; what each exercises: EXPECT and the module docstring there).
    d1: fixed-variance models with D = 1 take log_prob_X_given_z from the host expression, because numpy
    sums an (n, 1) float matrix pairwise and the kernel adds row after row: the kernel's own value is 1.4e-5 from the
    reference in float64 on these data and has no digit in common with it in float32.
    bank_tiers at 8 192: the sort's LDS request was 8 bytes past a workgroup's 160 KB with 32 768 staged keys, and the
    constructor failed with "invalid argument" for every bank from 8 187 components on (sort_keys_cap, segk_stats.hip)."""
    _model_matches(name, D, K_max, cov, dtype)


def test_scratch_reuse_across_bank_sizes_on_one_context(gpu):
    """The context's rb_sorted / rb_koff buffers grow and are then reused with another K_max + 1 stride: the widest bank
    first (8 192 components, three blocks), then twelve components in two blocks, forty in three, the widest again."""
    for m in [("bank_tiers", 4, 8192, "diag", F32), ("two_blocks", 5, 12, "fixed", F32), ("three_uneven", 7, 40, "fixed", F32),
              ("bank_tiers", 4, 8192, "diag", F32)]:
        _model_matches(*m)


SWEEPS = [("two_blocks", 5, 12, "fixed", F32), ("two_blocks", 5, 12, "diag", F32), ("three_uneven", 7, 40, "fixed", F32),
          ("three_uneven", 7, 40, "diag", F32)]


@pytest.mark.parametrize("name,D,K_max,cov,dtype", SWEEPS, ids=[_tag(*m) for m in SWEEPS])
def test_record_metrics_after_one_serial_sweep(gpu, name, D, K_max, cov, dtype):
    """gibbs_sample(1) on product and oracle from one `random` state: the assignment vector the metric kernels bucket is
    no longer the one init_stats saw (three_uneven, fixed: eleven components emptied and relabelled).  The oracle's sweep
    takes about 2 s (two_blocks) and 5 s (three_uneven) on the host."""
    tag = _tag(name, D, K_max, cov, dtype)
    c = lb.case(name, D, K_max, cov, dtype)
    ref = no.FBGMM(c["X"], no.FixedVarPrior(*c["prior"]) if cov == "fixed" else no.NIW(*c["prior"]), lb.ALPHA, K_max,
                   np.array(c["labels"]), covariance_type=cov)
    fm = _build(c["X"], c["labels"], K_max, cov, c["prior"])
    random.seed(3)
    rec = ref.gibbs_sample(1)
    after = random.random()
    random.seed(3)
    fm.gibbs_sample(1)
    assert random.random() == after, "the device consumed a different number of uniforms"
    rc, comp = ref.components, fm.components
    labels = np.array(rc.assignments)
    assert np.count_nonzero(labels != c["labels"]) > len(labels) // 2, "the chain did not move"
    assert comp.K == rc.K
    _same(comp.assignments, labels, tag + " assignments")
    _same(comp.counts, rc.counts, tag + " counts")
    nm = STAT_NAMES[cov]
    stats = dict(K=rc.K, counts=rc.counts, assignments=labels, a=getattr(rc, nm[0]), b=getattr(rc, nm[1]))
    lpx = lb.log_prob_X_given_z(c["X"], cov, c["prior"], stats)
    lpz = lb.log_prob_z_fbgmm(rc.counts, lb.ALPHA, K_max)
    npt.assert_allclose(lpx, rec["log_prob_X_given_z"][0], rtol=1e-12)
    npt.assert_allclose(lpz, rec["log_prob_z"][0], rtol=1e-12)
    _record_matches(comp.dev, tag, rc.K, int(rc.counts.sum()), lpz, lpx,
                    [float(lb.log_prob_z_urn(labels, a, K_max)) for a in lb.URN_A] if cov == "fixed" else None)


def test_bank_of_8193_is_refused_and_the_context_stays_usable(gpu):
    """segk_rows_by_label requires K_max <= 8192: the constructor fails with that message, and the next model on the same
    context is built and compared as usual."""
    from segmentalist_amd._abi import SegkError
    c = lb.case("two_blocks", 5, 12, "diag", F32)
    with pytest.raises(SegkError, match="K_max <= 8192"):
        _build(c["X"][:500], np.arange(500) % 12, 8193, "diag", c["prior"])
    _model_matches("two_blocks", 5, 12, "diag", F32)

"""
The FBGMM and bigram samplers at banks of 255 to 4 000 components, against the oracle (oracle/np_oracle.py: the reference's
serial chains) and the specification of the batch sampler (oracle/np_fbgmm_batch.py).  The kernels change form with the
size of the bank; every case below states the branch it reaches and checks it:

  * serial chain, launches per utterance (k_fbgmm_update / _score / _assign, k_unigram_segment; SEGK_FB_CHAIN=0 or a
    model too large for LDS): fb_nt is 512 threads below K_max = 256 and 256 from there on, and every block-wide
    logsumexp, argmax and draw of fb_draw_component then walks several components per thread;
  * serial chain, persistent kernel k_fb_chain: only while the model fits a workgroup's LDS, with the spans' predictive
    terms kept beside it only while those fit too (_chain_form mirrors the launcher's formulas; the wrapper of
    DeviceFbgmm.sequential_sweep records which path ran); relabel-heavy chains empty more than 16 components within one
    utterance (the log held 16 pairs);
  * FBGMM.gibbs_sample (k_fbgmm_gibbs_items) at the same banks;
  * batch sampler, score_precision="f64": tokens per assignment chunk and the form of the partial sums by bank size.

Serial chains: one `random` state for both sides, the device must leave the stream where the oracle does; boundaries,
assignments, K, counts and the language model's counts exact; record values within 1e-8 relative, statistics 1e-10.
"""
import os
import random

import numpy as np
import numpy.testing as npt
import pytest

from oracle import np_oracle as no
from tests.golden import cases
from tests.test_large_banks_cpu import (ORACLE_MODS, RELABEL_IDS, RELABEL_SHAPES, assert_relabel_heavy, build_segmenter,
                                        count_deletions, relabel_corpus)

pytestmark = pytest.mark.gpu

STATS = {"diag": ["m_N_numerators", "S_N_partials", "log_prod_vars", "inv_vars"],
         "fixed": ["mu_N_numerators", "precision_Ns", "log_prod_precision_preds", "precision_preds"]}
RECS = ["log_marg", "log_marg*length", "log_prob_z", "log_prob_X_given_z"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    torch.cuda.set_device(0)
    from segmentalist_amd import _abi
    _abi.ctx()
    return torch


def _product_mods():
    from segmentalist_amd import bigram_acoustic_wordseg as baw, fbgmm, unigram_acoustic_wordseg as uaw
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    return dict(FixedVarPrior=FixedVarPrior, NIW=NIW, FBGMM=fbgmm.FBGMM, UnigramAcousticWordseg=uaw.UnigramAcousticWordseg,
                BigramAcousticWordseg=baw.BigramAcousticWordseg)


def _fb_nt(K_max):
    """fb_nt (segk_fbgmm.hip): the workgroup width of the logits kernels and of the persistent chain."""
    return 256 if K_max >= 256 else 512


def _chain_form(seg):
    """The form segk_fbgmm_sequential_sweep takes for this segmenter: "launches" (the model does not fit a workgroup's LDS,
    more than 64 landmarks, or SEGK_FB_CHAIN=0), else the persistent kernel with the spans' predictive terms kept in LDS
    ("terms") or without them ("no-terms").  The launcher's `lds` and `lds_terms` formulas, both against 150 KB."""
    df = seg._df
    c, KM = df.corpus, df.K_max
    D, NM = c.D, c.N_max
    if NM > 64 or os.environ.get("SEGK_FB_CHAIN", "1") == "0":
        return "launches"
    from segmentalist_amd._abi import SEGK_F32
    max_rows = max(1, int(np.max(np.diff(np.asarray(seg._row_start)))))
    xs = 4 if c.x_dtype == SEGK_F32 else 8
    tri = NM * (NM + 1) // 2
    lds = ((3 * KM * D + 3 * KM + 1 + KM + _fb_nt(KM) + tri + 3 * NM + 2 + 3 * D) * 8 + ((D * xs + 7) & ~7)
           + (2 * tri + max_rows + NM) * 4 + ((NM + 15) & ~15) + max_rows * D * xs + 16
           + ((KM * 8 + NM * 4 + 16) if df.lm is not None else 0) + (2 * NM + 2 + max_rows + KM) * 8 + 16)
    if lds > 150 * 1024:
        return "launches"
    lds_terms = NM * KM * 8 + NM * 4 + ((KM + 15) & ~15) + 16
    if lds + lds_terms <= 150 * 1024 and os.environ.get("SEGK_FB_CHAIN_TERMS", "1") != "0":
        return "terms"
    return "no-terms"


def _state(seg, kind):
    c = seg.acoustic_model.components
    out = dict(bounds=seg.utterances.boundaries.copy(), assign=np.array(c.assignments), K=int(c.K), counts=np.array(c.counts))
    for nm in STATS["diag" if kind == "diag" else "fixed"]:
        out[nm] = np.array(getattr(c, nm)[:c.K])
    if kind == "bigram":
        out["uni"], out["big"] = np.array(seg.lm.unigram_counts), np.array(seg.lm.bigram_counts)
    return out


def _oracle_sweep(ref, anneal):
    """One sweep of the oracle chain; anneal != 1: the boundaries and the assignments annealed (anneal_gibbs_am=True,
    which oracle's gibbs_sample does not offer), the sweep of unigram_acoustic_wordseg.py:437-457 spelled out."""
    if anneal == 1:
        return ref.gibbs_sample(1)
    order = list(range(ref.utterances.D))
    no._shuffle(order)
    lp = 0
    for i in order:
        lp += ref.gibbs_sample_i(i, anneal, anneal_gibbs_am=True)
    am = ref.acoustic_model
    return {"log_marg": [am.log_marg()], "log_marg*length": [lp], "log_prob_z": [am.log_prob_z()],
            "log_prob_X_given_z": [am.log_prob_X_given_z()], "components": [am.components.K], "n_tokens": [am.get_n_assigned()]}


def _oracle_chain(kind, corpus, D, K, nmax, sweeps=2, fb_type="standard", anneal=1.0, relabel_heavy=False):
    """The oracle's chain: the initial state and, per sweep, the `random` state it started from, the next uniform after it,
    the record and the state it left."""
    no.set_shuffle("py3")
    ref = build_segmenter(ORACLE_MODS, kind, corpus, D, K, nmax, fb_type=fb_type)
    per = count_deletions(ref) if relabel_heavy else None
    init = _state(ref, kind)
    want = []
    for _ in range(sweeps):
        st = random.getstate()
        rec = _oracle_sweep(ref, anneal)
        want.append(dict(rng=st, after=random.random(), rec=rec, **_state(ref, kind)))
    if relabel_heavy:
        assert_relabel_heavy(per)
    assert not np.array_equal(want[-1]["bounds"], init["bounds"]), "the chain did not move"
    return init, want


def _watch_path(monkeypatch):
    """Record what every DeviceFbgmm.sequential_sweep call returns: True where the persistent kernel took the sweep, False
    where the utterances went through the launches."""
    from segmentalist_amd import device as dev_mod
    ran = []
    real = dev_mod.DeviceFbgmm.sequential_sweep
    monkeypatch.setattr(dev_mod.DeviceFbgmm, "sequential_sweep", lambda self, *a, **k: ran.append(real(self, *a, **k)) or ran[-1])
    return ran


def _device_matches(monkeypatch, ran, kind, corpus, D, K, nmax, init, want, form, env=None, fb_type="standard", anneal=1.0):
    """The product chain from the oracle's initial state and `random` states against the oracle, sweep by sweep; `form`: the
    form of the serial chain the case must reach (_chain_form, and the path the sweeps took)."""
    env = dict(env or {})
    env.setdefault("SEGK_FB_CHAIN", "1")
    env.setdefault("SEGK_FB_CHAIN_TERMS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seg = build_segmenter(_product_mods(), kind, corpus, D, K, nmax, fb_type=fb_type)
    assert _chain_form(seg) == form
    assert seg._df.K_max == K
    assert np.array_equal(seg.utterances.boundaries, init["bounds"])
    assert np.array_equal(seg.acoustic_model.components.assignments, init["assign"])
    kw = dict(anneal_schedule="linear", anneal_start_temp_inv=1. / anneal, anneal_gibbs_am=True) if anneal != 1 else {}
    for it, w in enumerate(want):
        del ran[:]
        random.setstate(w["rng"])
        rec = seg.gibbs_sample(1, **kw)
        assert random.random() == w["after"], "the device chain consumed a different number of uniforms (sweep %d)" % it
        assert ran and all(r == (form != "launches") for r in ran), (form, ran)
        got = _state(seg, kind)
        for k in ("bounds", "assign", "counts") + (("uni", "big") if kind == "bigram" else ()):
            assert np.array_equal(got[k], w[k]), (it, k)
        assert got["K"] == w["K"], it
        for k in RECS:
            npt.assert_allclose(rec[k][0], w["rec"][k][0], rtol=1e-8, err_msg="%s, sweep %d" % (k, it))
        assert rec["components"][0] == w["rec"]["components"][0] and rec["n_tokens"][0] == w["rec"]["n_tokens"][0], it
        for nm in STATS["diag" if kind == "diag" else "fixed"]:
            npt.assert_allclose(got[nm], w[nm], rtol=1e-10, atol=1e-300, err_msg="%s, sweep %d" % (nm, it))


# ------------------------------------------------------------------ (a, b) both sides of the fb_nt switch
@pytest.mark.parametrize("K", [255, 256])
@pytest.mark.parametrize("kind", ["diag", "fixed", "bigram"])
def test_serial_chain_either_side_of_the_thread_count_switch(gpu, monkeypatch, kind, K):
    """K_max = 255 (fb_nt 512: two lanes per component in fb_logits) and 256 (fb_nt 256: one lane per component, and
    fb_draw_component's loops walk every thread's component), D = 12, 40 ragged utterances of 10-20 landmarks.  The
    same oracle chain against three device forms: the launches per utterance (SEGK_FB_CHAIN=0), the persistent kernel with
    the spans' terms kept (they fit: lds + lds_terms <= 150 KB) and without them (SEGK_FB_CHAIN_TERMS=0)."""
    D, nmax = 12, 6
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(40, D, K, seed=4, ragged=True, n_slices_max=nmax, N_range=(10, 20))
    init, want = _oracle_chain(kind, corpus, D, K, nmax)
    ran = _watch_path(monkeypatch)
    _device_matches(monkeypatch, ran, kind, corpus, D, K, nmax, init, want, "launches", env={"SEGK_FB_CHAIN": "0"})
    _device_matches(monkeypatch, ran, kind, corpus, D, K, nmax, init, want, "terms")
    _device_matches(monkeypatch, ran, kind, corpus, D, K, nmax, init, want, "no-terms", env={"SEGK_FB_CHAIN_TERMS": "0"})


# ------------------------------------------------------------------ (a) banks too large for the persistent kernel
@pytest.mark.parametrize("kind", ["diag", "fixed", "bigram"])
def test_serial_chain_configs4_shape_by_launches(gpu, monkeypatch, kind):
    """configs[4] shape: D = 100, K = 1 000, 100 utterances of 20 landmarks.  3 K_max D doubles are 2.4 MB: the launches per
    utterance (fb_nt 256, four components per thread in every block-wide reduction and draw)."""
    D, K, nmax = 100, 1000, 6
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(100, D, K, seed=0, N=20, n_slices_max=nmax)
    init, want = _oracle_chain(kind, corpus, D, K, nmax)
    _device_matches(monkeypatch, _watch_path(monkeypatch), kind, corpus, D, K, nmax, init, want, "launches")


@pytest.mark.parametrize("kind", ["diag", "fixed", "bigram"])
def test_serial_chain_bank_above_1024_by_launches(gpu, monkeypatch, kind):
    """K = 1 100 at D = 39, 40 utterances of 20 landmarks: five components per thread in fb_draw_component, the bigram
    tables K x K; the launches (the model is 1 MB)."""
    D, K, nmax = 39, 1100, 6
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(40, D, K, seed=1, N=20, n_slices_max=nmax)
    init, want = _oracle_chain(kind, corpus, D, K, nmax)
    _device_matches(monkeypatch, _watch_path(monkeypatch), kind, corpus, D, K, nmax, init, want, "launches")


def test_serial_chain_viterbi_at_a_large_bank(gpu, monkeypatch):
    """fb_type="viterbi" at D = 100, K = 1 000: map_assign_i's argmax in fb_draw_component (64 lanes, each scanning
    K_max / 64 components, then the tie-breaking butterfly) and the Viterbi DP, by the launches."""
    D, K, nmax = 100, 1000, 6
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(50, D, K, seed=2, N=20, n_slices_max=nmax)
    init, want = _oracle_chain("diag", corpus, D, K, nmax, fb_type="viterbi")
    _device_matches(monkeypatch, _watch_path(monkeypatch), "diag", corpus, D, K, nmax, init, want, "launches", fb_type="viterbi")


def test_serial_chain_annealed_at_a_large_bank(gpu, monkeypatch):
    """anneal_temp = 2 for the boundaries and the assignments (anneal_gibbs_am=True) at D = 100, K = 1 000: the second
    block-wide logsumexp of fb_draw_component over four components per thread, by the launches."""
    D, K, nmax = 100, 1000, 6
    from segmentalist_amd.synth import make_corpus
    corpus = make_corpus(50, D, K, seed=3, N=20, n_slices_max=nmax)
    init, want = _oracle_chain("fixed", corpus, D, K, nmax, anneal=2.0)
    _device_matches(monkeypatch, _watch_path(monkeypatch), "fixed", corpus, D, K, nmax, init, want, "launches", anneal=2.0)


# ------------------------------------------------------------------ (b) the persistent kernel's relabel log
@pytest.mark.parametrize("kind,n_utt,D,K,N_range,nmax", RELABEL_SHAPES, ids=RELABEL_IDS)
def test_persistent_chain_relabel_heavy_utterances(gpu, monkeypatch, kind, n_utt, D, K, N_range, nmax):
    """Utterances that empty more than 16 components each (and others 13 to 16, asserted on the oracle side; the same
    shapes as tests/test_large_banks_cpu.py) through the persistent kernel, which fits LDS here without the spans' terms.
    Every emptied component moves the last one into its slot: the kernel logs the pairs, stops after the utterance, and
    the launcher relabels the other utterances' rows from the log -- and with a language model the carried label of the
    corpus's last row too.  The log held 16 pairs: an utterance past that failed the sweep with SEGK_ERR_ARG."""
    corpus = relabel_corpus(n_utt, D, K, N_range, nmax)
    init, want = _oracle_chain(kind, corpus, D, K, nmax, relabel_heavy=True)
    _device_matches(monkeypatch, _watch_path(monkeypatch), kind, corpus, D, K, nmax, init, want, "no-terms")


# ------------------------------------------------------------------ (c) FBGMM.gibbs_sample
@pytest.mark.parametrize("unassigned", [True, False], ids=["consider_unassigned", "assigned_only"])
@pytest.mark.parametrize("K", [255, 256, 1000])
@pytest.mark.parametrize("cov", ["fixed", "diag"])
def test_fbgmm_gibbs_sample_at_large_banks(gpu, cov, K, unassigned):
    """fbgmm.py:288-420 (segk_fbgmm_gibbs_items: fb_nt 512 at K = 255, 256 from K = 256 on) against no.FBGMM.gibbs_sample:
    300 items at D = 16, 30 % of them unassigned at the start, three sweeps from one `random` state."""
    from segmentalist_amd import fbgmm
    from segmentalist_amd.gaussian_components_fixedvar import FixedVarPrior
    from segmentalist_amd.niw import NIW
    D = 16
    X, assign = cases.gauss_state(D, K, 300, 40 + K)
    out = []
    for side in ("oracle", "product"):
        random.seed(3)
        np.random.seed(3)
        if side == "oracle":
            prior = no.FixedVarPrior(*cases.fixed_prior_params(D)) if cov == "fixed" else no.NIW(*cases.diag_prior_params(D))
            fm = no.FBGMM(X, prior, 1.0, K, assign.copy(), covariance_type=cov, lms=1.0)
        else:
            prior = FixedVarPrior(*cases.fixed_prior_params(D)) if cov == "fixed" else NIW(*cases.diag_prior_params(D))
            fm = fbgmm.FBGMM(X, prior, 1.0, K, assign.copy(), covariance_type=cov, lms=1.0)
        rec = fm.gibbs_sample(3, consider_unassigned=unassigned)
        c = fm.components
        out.append(dict(rec=rec, assign=np.array(c.assignments), counts=np.array(c.counts), K=int(c.K), after=random.random(),
                        **{nm: np.array(getattr(c, nm)[:c.K]) for nm in STATS[cov]}))
    want, got = out
    assert got["after"] == want["after"], "the device consumed a different number of uniforms"
    assert np.array_equal(got["assign"], want["assign"])
    assert np.array_equal(got["counts"], want["counts"]) and got["K"] == want["K"]
    for k in ["log_marg", "log_prob_z", "log_prob_X_given_z"]:
        npt.assert_allclose(got["rec"][k], want["rec"][k], rtol=1e-8, err_msg=k)
    assert list(got["rec"]["components"]) == list(want["rec"]["components"])
    for nm in STATS[cov]:
        npt.assert_allclose(got[nm], want[nm], rtol=1e-10, atol=1e-300, err_msg=nm)
    assert not np.array_equal(want["assign"], assign), "the chain did not move"


# ------------------------------------------------------------------ (d) the exact batch sampler
def _fbb_rcap(K, D):
    """Tokens per chunk of segk_fbb_assign (score_precision="f64", K_max > 128): as many rows of K_max doubles as fit in
    80 KB beside (K_max + FBA_R D + FBA_R + 16) doubles, FBB_R = 8 at most."""
    fixed_b = (K + 16 * D + 16 + 16) * 8
    rcap = 8
    while rcap > 1 and fixed_b + rcap * K * 8 > 80 * 1024:
        rcap //= 2
    return rcap


def _fbb_partials(K):
    """segk_fbb_partials: tokens bucketed by slot first (k_fbb_sort) for 256 <= K_max <= 1 024, else the one-step kernel."""
    return "sorted" if 256 <= K <= 1024 and (16 * K + 17) * 4 <= 150 * 1024 else "one-step"


# kind, n_utt, D, K, cseed, nmax, B, S, rcap, partials
BATCH_CASES = [
    ("fixed", 200, 100, 1000, 101, 5, 3, 4, 4, "sorted"),       # configs[4] shape
    ("bigram", 100, 100, 1000, 102, 5, 3, 4, 4, "sorted"),      # the language model's K x K tables at configs[4] shape
    ("fixed", 100, 16, 1024, 103, 5, 3, 4, 8, "sorted"),        # the widest bank with sorted partial sums
    ("fixed", 100, 16, 1025, 104, 5, 3, 4, 8, "one-step"),      # one past it
    ("diag", 60, 64, 1100, 105, 5, 3, 4, 4, "one-step"),
    ("diag", 40, 256, 4000, 106, 5, 2, 2, 1, "one-step"),       # one token per chunk
]


@pytest.mark.parametrize("kind,n_utt,D,K,cseed,nmax,B,S,rcap,partials", BATCH_CASES,
                         ids=["%s_D%d_K%d" % (c[0], c[2], c[3]) for c in BATCH_CASES])
def test_exact_batch_sweeps_at_large_banks(gpu, kind, n_utt, D, K, cseed, nmax, B, S, rcap, partials):
    """score_precision="f64" batch sweeps against oracle/np_fbgmm_batch.py (tests/test_gpu_fbgmm_batch.py's check, two
    sweeps).  The branches, from segk_fbb_assign and segk_fbb_partials:

      fixed   D 100 K 1000: rcap 4 ((1000 + 1600 + 32) 8 + 8 x 8000 bytes > 80 KB, 4 rows fit), sorted partials
      bigram  D 100 K 1000: rcap 4, sorted partials, bigram counts K x K
      fixed   D 16  K 1024: rcap 8, sorted partials (K_max <= 1024)
      fixed   D 16  K 1025: rcap 8, one-step partials (K_max > 1024)
      diag    D 64  K 1100: rcap 4 ((1100 + 1024 + 32) 8 + 8 x 8800 > 80 KB), one-step partials
      diag    D 256 K 4000: rcap 1 ((4000 + 4096 + 32) 8 + 2 x 32000 > 80 KB), one-step partials

    Every draw walks the K_max probabilities in runs of 16 (draw_chunked)."""
    from tests.test_gpu_fbgmm_batch import _sweeps_match_specification
    assert _fbb_rcap(K, D) == rcap and _fbb_partials(K) == partials
    _sweeps_match_specification(gpu, kind, n_utt, D, K, cseed, nmax, B, S, {}, sweeps=2)

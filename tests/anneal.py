"""Cases and host-side checkers of the annealed batch sampler's tests (sync="batch" with a temperature other than 1):
tests/test_anneal_batch_cpu.py checks, with the oracle and the batch specification alone, that every case can see what it
is there for; tests/test_gpu_anneal_batch.py runs the device on the same cases.  Nothing here touches the device.

Why the cases carry their own segmenter keywords: with span scores of log_marg x duration the candidates of a boundary draw
lie hundreds of nats apart and the draw does not depend on the temperature -- a kernel that ignored anneal_temp would give
the specification's chain bit for bit.  time_power_term = 0.0 (a span scores its log-marginal, whatever its length) and a
word insertion penalty near the negative of a typical log-marginal bring segmentations with different numbers of segments
within reach of each other; `sensitivity` measures what is left, and the CPU test holds every case to it.

The pairs are built by the builders of the existing tests -- tests/test_gpu_fbgmm_batch.py::_pair ("chain"),
tests/fbgmm_long.py ("long"), tests/test_gpu_tolerance_modes.py::_pair ("bench") -- not by copies of them."""
import functools

import numpy as np
from scipy.special import logsumexp as _lse

from oracle import np_fbgmm_batch as nb
from oracle import np_oracle as no
from tests import fbgmm_long as fl

# 10: the reference's default start (anneal_start_temp_inv = 0.1); 0.5: what a run to anneal_end_temp_inv = 2 reaches, the
# direction that sharpens
TEMPS = (10.0, 2.0, 0.5)

SLOT_TOL = 1e-4          # the project's bound on a slot draw (tests/test_gpu_tolerance_modes.py), times max(1, 1 / T)


def _chain(kind, n_utt, D, K, cseed, nmax, B, S, T, am, reaches, n_landmarks=0, **kw):
    return dict(src="chain", kind=kind, n_utt=n_utt, D=D, K=K, cseed=cseed, nmax=nmax, B=B, S=S, T=T, am=am, reaches=reaches,
                n_landmarks=n_landmarks, kw=kw, prec="f64")


def _long(name, T, am, reaches, **kw):
    c = dict(fl.CASES[name])
    c["kw"] = dict(c.get("kw", {}), **kw)
    return dict(c, src="long", T=T, am=am, reaches=reaches, prec=c.get("prec", "f64"))


def _bench(kind, prec, n_utt, D, K, form, T, reaches, **kw):
    """form: None, "fused" (segk_fbb_step_diag32) or "0" (SEGK_FBB_ASSIGN_WAVE=0: the block-wide draw kernel)."""
    return dict(src="bench", kind=kind, prec=prec, n_utt=n_utt, D=D, K=K, form=form, nmax=6, B=3, S=2, T=T, am=True,
                reaches=reaches, kw=kw)


TP0 = dict(time_power_term=0.0)

# ---------------------------------------------------------------------------------------------------------------------
# exact mode (score_precision="f64"): the specification's chain bit for bit.  Every case: kind, corpus, window, B x S, T,
# anneal_gibbs_am, segmenter keywords -- and, in `reaches`, the kernel form it is there for.  Corpora: those of
# tests/test_gpu_fbgmm_batch.py (CASES, test_batch_sweeps_with_a_wide_window, test_bigram_batch_sweeps_match_specification),
# tests/fbgmm_long.py and tests/test_gpu_large_banks.py::BATCH_CASES (fewer utterances: the specification's run time).
# am=False where the slots of the corpus do not move with the temperature (fixed-variance components at T < 1: measured
# shares of 0.00), so that no case claims an annealing it cannot see.
# ---------------------------------------------------------------------------------------------------------------------
EXACT = {
    # k_fbb_segment (N_max <= 64), window <= 16: fb_dp_sample_on's LDS path with triangular addressing
    "fixed_w5_fb": _chain("fixed", 24, 8, 10, 77, 5, 3, 4, 10.0, False, "k_fbb_segment, window <= 16; boundaries only", **TP0),
    "fixed_w5_am": _chain("fixed", 24, 8, 10, 77, 5, 3, 4, 10.0, True, "k_fbb_slots<COV 0>, 512 threads: wave per token", **TP0),
    # (n_slices_min = 1: the batch entry points take 0 or 1; see test_anneal_batch_cpu.py for what it changes)
    "diag_w5_am": _chain("diag", 24, 8, 10, 78, 5, 3, 4, 10.0, True, "k_fbb_slots<COV 1>, 512 threads: wave per token",
                         n_slices_min=1, **TP0),
    "diag_w5_fb_T2": _chain("diag", 24, 8, 10, 78, 5, 3, 4, 2.0, False, "k_fbb_segment; boundaries only", **TP0),
    "diag_w5_T05": _chain("diag", 24, 8, 10, 78, 5, 3, 4, 0.5, True, "T < 1, boundaries and slots", **TP0),
    "bigram_w5_fb": _chain("bigram", 30, 8, 12, 91, 5, 3, 4, 10.0, False, "k_fbb_segment; boundaries only, language model", **TP0),
    "bigram_w5_am": _chain("bigram", 30, 8, 12, 91, 5, 3, 4, 10.0, True, "k_fbb_assign_lm, block-wide draw (language model)", **TP0),
    "bigram_n40_T05": _chain("bigram", 12, 8, 12, 91, 5, 3, 4, 0.5, False, "T < 1, language model", n_landmarks=40, **TP0),
    "fixed_n64_w6_T05": _chain("fixed", 8, 8, 10, 93, 6, 2, 2, 0.5, False, "T < 1, 64 landmarks", n_landmarks=64, **TP0),
    # ... window 17..64: candidates beyond one row of sixteen lanes
    "wide_fixed_w20": _chain("fixed", 8, 8, 10, 93, 20, 2, 2, 10.0, True, "k_fbb_segment, window 20", n_landmarks=24, **TP0),
    "wide_diag_w20": _chain("diag", 8, 8, 10, 93, 20, 2, 2, 2.0, True, "k_fbb_segment, window 20", n_landmarks=24, **TP0),
    "wide_fixed_w30_n64": _chain("fixed", 8, 8, 10, 93, 30, 2, 2, 2.0, False, "k_fbb_segment, window 30 at 64 landmarks",
                                 n_landmarks=64, **TP0),
    # k_fbb_segment<BAND> (N_max > 64): the LDS path with FbBandVec addressing
    "long_ragged_fixed": _long("ragged_fixed", 10.0, True, "k_fbb_segment<BAND>", **TP0),
    "long_ragged_fixed_T05": _long("ragged_fixed", 0.5, True, "k_fbb_segment<BAND>, T < 1", **TP0),
    "long_ragged_diag": _long("ragged_diag", 0.5, True, "k_fbb_segment<BAND>, T < 1", **TP0),
    "long_ragged_bigram": _long("ragged_bigram", 0.5, True, "k_fbb_segment<BAND>, T < 1; block-wide draw", **TP0),
    "long_diag_100_w20": _long("diag_100_w20", 2.0, True, "k_fbb_segment<BAND>, window 20", **TP0),
    # k_fbb_slots by bank size.  The large banks' log-marginals sit near +52 (D = 100) and +285 (D = 256) per span: the word
    # insertion penalty takes that off, or the segmentation with the most segments wins at every temperature
    "K300_am": _chain("fixed", 19, 6, 300, 81, 5, 5, 1, 10.0, True, "k_fbb_slots, 256 threads (K_max > 128)", **TP0),
    "bank_rcap4_fixed": _chain("fixed", 40, 100, 1000, 101, 5, 3, 4, 10.0, True, "k_fbb_slots, four tokens per chunk",
                               time_power_term=0.0, wip=-52.0),
    "bank_rcap1_diag": _chain("diag", 16, 256, 4000, 106, 5, 2, 2, 10.0, True, "k_fbb_slots, one token per chunk",
                              time_power_term=0.0, wip=-252.0),
}
# Dropped: the bigram D = 100, K = 40 corpus of tests/test_gpu_fbgmm_batch.py::CASES (at most 1 utterance in 30 moves at any
# temperature and any of time_power_term in {1, 0}, lms in {1, 0.2}); fixed_100_w40 of tests/fbgmm_long.py (sensitive, but
# 11 s per sweep of the specification; diag_100_w20 is the wide-window band case).

# the driver (gibbs_sample with a linear schedule from 1 / T = 0.1) and the two-rank run reuse cases of the table
DRIVER = {"unigram": "diag_w5_am", "bigram": "bigram_w5_am"}
RANKS = "long_ragged_fixed"

# ---------------------------------------------------------------------------------------------------------------------
# tolerance modes (score_precision "f32" / "f16"), value by value: the forms of tests/test_gpu_tolerance_modes.py::CASES on the
# bench generator's corpus (24 utterances of 20 landmarks), each at T = 1 and at the T below, boundaries and slots annealed.
# The language-model cases at D = 16 (the D = 100 corpus costs the specification four times as long and moves no more).  At
# D = 39 the log-marginals sit near +45 per span and the segmentation with the most segments takes most of the probability
# at any temperature: a word insertion penalty of that size takes it off (without it intervals computed at T = 1 reject
# 0.08 of the boundary draws, with it 0.20 and more).
# ---------------------------------------------------------------------------------------------------------------------
TOLERANCE = {
    "diag_f32_launches": _bench("diag", "f32", 24, 39, 100, None, 10.0,
                                "fb_dp_sample_fast32; k_fbb_slots<COV 1, F32> (segk_fbb_assign_diag32)", wip=-46.0, **TP0),
    "diag_f32_fused_K100": _bench("diag", "f32", 24, 39, 100, "fused", 10.0, "k_fbb_step_diag32, one chunk of slots", wip=-46.0,
                                  **TP0),
    "diag_f32_fused_K160": _bench("diag", "f32", 24, 20, 160, "fused", 10.0, "k_fbb_step_diag32, three chunks of 64 slots", **TP0),
    "fixed_f16": _bench("fixed", "f16", 24, 39, 100, None, 10.0, "fb_dp_sample_fast32; k_fbb_slots with llmat", wip=-45.0, **TP0),
    "fixed_f32": _bench("fixed", "f32", 24, 39, 100, None, 10.0, "fb_dp_sample_fast32; k_fbb_slots<COV 0>, fp64 likelihoods",
                        wip=-45.0, **TP0),
    "bigram_f16_wave": _bench("bigram", "f16", 24, 16, 300, None, 10.0, "k_fbb_assign_lm_wave, register form", **TP0),
    "bigram_f16_blockwide": _bench("bigram", "f16", 24, 16, 300, "0", 10.0, "k_fbb_assign_lm with llmat, block-wide draw", **TP0),
    "bigram_f16_K1100": _bench("bigram", "f16", 24, 16, 1100, None, 10.0, "k_fbb_assign_lm_wave, per-slot loops (K_max > 1024)",
                               **TP0),
    # more than 64 landmarks: the fp64 recurrence with the hardware exponential and logarithm (fb_logsumexp_wave_fast,
    # fb_exp_fast) on the LDS path, band addressing
    "long_fixed_f32": _long("fixed_f32", 10.0, True, "k_fbb_segment<BAND> with fast_dp", **TP0),
}


def case_of(name):
    return EXACT[name] if name in EXACT else TOLERANCE[name]


# ---------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------
def build(case, product=False):
    """(oracle segmenter, specification, product segmenter or None) of a case, from identical initial states."""
    c = case_of(case) if isinstance(case, str) else case
    if c["src"] == "chain":
        from tests.test_gpu_fbgmm_batch import _pair
        return _pair(c["kind"], c["n_utt"], c["D"], c["K"], c["cseed"], c["nmax"], c["B"], c["S"], score_precision=c["prec"],
                     n_landmarks=c["n_landmarks"], product=product, **c["kw"])
    if c["src"] == "bench":
        from tests.test_gpu_tolerance_modes import _pair
        return _pair(c["kind"], c["n_utt"], c["D"], c["K"], c["prec"], B=c["B"], S=c["S"], product=product, **c["kw"])
    corpus = fl.corpus_of(c)
    ref, spec = fl.oracle_of(c, corpus=corpus)
    return ref, spec, (fl.product_of(c, corpus=corpus) if product else None)


# ---------------------------------------------------------------------------------------------------------------------
# the specification's draws, recorded
# ---------------------------------------------------------------------------------------------------------------------
class SpecTrace(object):
    """Records, while spec.sweep runs, every backward pass (`dp`: utterance, span-score vector, length, window, temperature,
    sampled boundaries) and every slot draw (`tok`: utterance, position, spec.prior_z(...) and spec.loglik(...) of the token,
    the drawn slot); use as a context manager."""

    def __init__(self, spec):
        self.spec = spec

    def __enter__(self):
        self.dp, self.tok = [], []
        spec, trace = self.spec, self
        self._fb, self._draw, self._u01 = no.forward_backward, nb.draw_chunked, nb.u01
        last = {}

        def forward_backward(vec, log_p_continue, N, n_slices_min, n_slices_max, i_utt, anneal_temp, uniforms=None):
            lp, bnd = trace._fb(vec, log_p_continue, N, n_slices_min, n_slices_max, i_utt, anneal_temp, uniforms=uniforms)
            trace.dp.append(dict(utt=i_utt, vec=np.array(vec), N=N, window=n_slices_max, T=anneal_temp, bounds=np.array(bnd)))
            return lp, bnd

        def u01(seed, sweep, utt, j):
            last["u"] = (utt, j)
            return trace._u01(seed, sweep, utt, j)

        def prior_z(*a):
            last["prior"] = type(spec).prior_z(spec, *a)
            return last["prior"]

        def loglik(*a):
            last["ll"] = type(spec).loglik(spec, *a)
            return last["ll"]

        def draw_chunked(p, u):
            k = trace._draw(p, u)
            utt, j = last["u"]
            trace.tok.append(dict(utt=utt, t=j - spec.seg.utterances.N_max, prior=np.array(last["prior"]),
                                  ll=np.array(last["ll"]), k=k))
            return k

        no.forward_backward, nb.draw_chunked, nb.u01 = forward_backward, draw_chunked, u01
        spec.prior_z, spec.loglik = prior_z, loglik
        return self

    def __exit__(self, *exc):
        no.forward_backward, nb.draw_chunked, nb.u01 = self._fb, self._draw, self._u01
        del self.spec.prior_z, self.spec.loglik
        return False


def _tokens(ref, i):
    return [int(e) for e in ref.utterances.get_segmented_embeds_i(i) if e != -1]


@functools.lru_cache(maxsize=None)
def first_sweeps(name):
    """Sweep 0 of the specification three times from the case's initial state: at T = 1, at the case's T with the assignment
    annealing off, and with it on.  Per run (boundaries, slots per utterance, trace)."""
    c = case_of(name)
    runs = []
    for T, am in ((1.0, False), (c["T"], False), (c["T"], True)):
        ref, spec, _ = build(c)
        with SpecTrace(spec) as trace:
            lp = spec.sweep(0, T, am)
        assert np.all(np.isfinite(lp)), name
        u = ref.utterances
        runs.append(dict(bounds=u.boundaries.copy(), slots=[[int(spec.slot[e]) for e in _tokens(ref, i)] for i in range(u.D)],
                         trace=trace, seed=spec.seed, N_max=u.N_max, T=T, am=am))
    return runs


def sensitivity(name):
    """(share of utterances whose boundaries at the case's T differ from those at T = 1, assignment annealing off in both;
    share of tokens that differ between the runs at T with the assignment annealing on and off -- another slot, or an
    utterance with other boundaries)."""
    one, off, on = first_sweeps(name)
    n_utt = len(one["slots"])
    moved = [not np.array_equal(one["bounds"][i], off["bounds"][i]) for i in range(n_utt)]
    n_tok = n_diff = 0
    for i in range(n_utt):
        n = len(on["slots"][i])
        n_tok += n
        if not np.array_equal(on["bounds"][i], off["bounds"][i]):
            n_diff += n
        else:
            n_diff += sum(a != b for a, b in zip(on["slots"][i], off["slots"][i]))
    return float(np.mean(moved)), n_diff / float(max(n_tok, 1))


# ---------------------------------------------------------------------------------------------------------------------
# checkers: how far a draw's uniform lies outside the interval of what was drawn (0: inside)
# ---------------------------------------------------------------------------------------------------------------------
def _annealed_probabilities(z, T):
    """softmax(z / T) the way the specification forms it (oracle/np_fbgmm_batch.py::FbgmmBatch.sweep, fbgmm.py:446-449;
    np_oracle.forward_backward): normalise, divide by T, normalise again; fp64."""
    z = np.asarray(z, np.float64)
    z = z - _lse(z)
    if T != 1:
        z = 1. / T * z
        z = z - _lse(z)
    with np.errstate(under="ignore"):
        return np.exp(z)


def _outside(p, k, u):
    cum = np.cumsum(p)
    below = cum[k - 1] if k > 0 else 0.0
    above = cum[k] if k < len(p) - 1 else 1.0          # (utils.draw: the last entry takes what rounding leaves)
    return max(0.0, below - u, u - above)


def token_uniform(seed, sweep, utt, N_max, t):
    return nb.u01(seed, sweep, utt, N_max + t)


def slot_draw_distance(prior_z, ll, T, k, u):
    """prior_z: spec.prior_z(d, j_prev, uni, big); ll: the token's log-likelihood under every slot; T: the temperature of the
    slot draws (1 where anneal_gibbs_am is off); k: the drawn slot; u: token_uniform(...).  The distance of u from
    [cum(k - 1), cum(k)), cum the running sum of softmax((prior_z + ll) / T) in slot order."""
    return _outside(_annealed_probabilities(np.asarray(prior_z, np.float64) + np.asarray(ll, np.float64), T), int(k), u)


def boundary_draw_distance(vec, alpha, N, window, T, bounds, seed, sweep, utt):
    """The backward pass of one utterance (unigram_acoustic_wordseg.py:705-756, np_oracle.forward_backward), step by step from
    t = N: the candidates w_s = vec[(t, s)] + alpha[s], shortest segment first (the order the draw walks them),
    p = softmax(w / T) in fp64; the segment read off `bounds` is slot k of that draw and its uniform is
    nb.u01(seed, sweep, utt, j) for the j-th emitted segment.  vec: triangular span scores (score x duration + wip, -inf where
    there is none); alpha: the forward filter's values.  Returns per step (distance of the uniform from the segment's
    interval, M = the largest magnitude among the finite candidates' vec entries, alphas and sums).  No candidate window may
    be all -inf (corpora without NaN durations): the back-tracking branch stays out of it."""
    vec, alpha = np.asarray(vec, np.float64), np.asarray(alpha, np.float64)
    ends = [j + 1 for j in range(N) if bounds[j]]          # segment ends t, increasing; the last is N
    assert ends and ends[-1] == N
    starts = [0] + ends[:-1]
    out = []
    for j, (s0, t) in enumerate(zip(reversed(starts), reversed(ends))):
        lo = max(0, t - window) if window else 0
        i = (t - 1) * t // 2
        s = np.arange(t - 1, lo - 1, -1)                   # shortest segment first
        v, a = vec[i + s], alpha[s]
        w = v + a
        fin = np.isfinite(w)
        assert fin.any(), "a window of -inf candidates: this checker does not follow the back-tracking branch"
        k = t - s0 - 1                                      # length k + 1
        assert 0 <= k < len(w), (t, s0, window)
        M = float(max(np.abs(v[fin]).max(), np.abs(a[fin]).max(), np.abs(w[fin]).max()))
        out.append((_outside(_annealed_probabilities(w, T), k, nb.u01(seed, sweep, utt, j)), M))
    return out


def boundary_bound(M, T):
    """2 delta / T + 1e-5, delta = 4 ulp of float32 at M: the float32 DP forms a candidate from two float32 roundings of
    quantities no larger than M and their sum; a log-weight error of delta moves a cumulative probability by at most
    e^(2 delta / T) - 1; 1e-5 for the hardware exponential and logarithm."""
    return 2. * 4. * float(np.spacing(np.float32(M))) / T + 1e-5


def slot_bound(T):
    return SLOT_TOL * max(1.0, 1.0 / T)

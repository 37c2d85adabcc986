"""
Executable SPECIFICATION of `UnigramAcousticWordseg.decode` (`segk_fbd_decode`): boundaries and transcript of
utterances that are NOT in the model, read-only.  Test infrastructure only, like tests/map_batch.py and tests/fbgmm_predict.py.

A held-out utterance is in no model.  Its candidate embeddings are UNASSIGNED items appended to X, seen against the statistics
of ALL tokens that hold a component -- the batch specification's `derive(*stats_excluding(-1))`, the state segk_fbb_prepare(-1)
leaves.  For an utterance of N landmarks, with the model's n_slices_min, n_slices_max, wip, time_power_term, lms, alpha and
min_duration:

  span scores    vec[j] = log_marg_i(x_e) * dur_j ** time_power_term + wip, -inf where vec_ids[j] == -1 or the duration is NaN
                 (get_vec_embed_log_probs, unigram_acoustic_wordseg.py:474-511); log_marg_i is the held-out log density of
                 tests/fbgmm_predict.py (`functions_of`), lms included
  boundaries,    forward_backward_viterbi(vec, 0.0, N, n_slices_min, n_slices_max) (:759-864) with the oracle's dead-end rule;
  log_prob       among equal maxima the shortest span wins (the largest start index)
  labels         per chosen segment map_assign_i's choice for its embedding against the same frozen statistics: the first index
                 of max_k log(alpha / K_max + n_k) + ll_k, no lms, in the reference view's numbering (an occupied slot its rank
                 among the occupied slots, an empty slot K) -- tests/fbgmm_predict.py's label.  Every segment is labelled
                 INDEPENDENTLY: nothing is added to the bank between segments, the one deliberate difference from a serial
                 Viterbi visit (unigram_acoustic_wordseg.py:252-360)
  no embedding   a chosen segment whose span has no embedding (only after back-tracking from a dead end) is kept: embedding
                 -1, label -1, log density -inf, so that segments and boundaries stay aligned

No uniform, no temperature, no new statistics.

Cases: tests/map_batch.LONG_CASES, brought to their state by the case's own two Viterbi sweeps; the held-out set of a case is
the HELD utterances that follow the case's own in make_corpus(n_utt + HELD, ...) at the same seed and window (the first n_utt
utterances of that call ARE the case's corpus, so the held-out rows share its cluster centres).  CROSS: a model trained on a
triangular corpus decoding a band corpus (the ragged recipes built at the model's window).  FULL: full covariance, the sampled
cases of tests/fullcov_batch.py after their own sweeps.

LDS of k_fbd_decode (restated from segmentalist_amd/csrc/segk_fbdecode.hip; tests/test_wordseg_decode_cpu.py holds it against the
source): k_fbb_segment's without the old token list -- with cells = N_max W (band) or N_max (N_max + 1) / 2 (triangle),
8 (cells + 3 N_max + 2) + 4 cells + (N_max rounded up to 16) bytes.
"""
import numpy as np

from oracle import np_oracle as no
from tests import fbgmm_predict as fp
from tests import map_batch as mbm

MARGIN = mbm.MARGIN              # 1e-6 relative: every DP and label decision of every case (a condition on the inputs)
HELD = 6
# model case -> the LONG_CASES recipe its held-out set is built from, at the MODEL's window
CROSS = {"diag_K65_x_ragged": ("diag_K65", "ragged_diag"), "fixed_small_x_ragged": ("fixed_small", "ragged_fixed")}
# full covariance: names of tests/fullcov_batch.SAMPLED
FULL = ["w0_K8", "w6_long"]
CASES = list(mbm.LONG_CASES) + list(CROSS)
BAND_LDS_MAX = 160 * 1024


def lds_bytes(N_max, W=0):
    """bytes of a k_fbd_decode workgroup: the band of W columns where N_max > 64, else the triangle"""
    cells = N_max * W if N_max > 64 else N_max * (N_max + 1) // 2
    return 8 * (cells + 3 * N_max + 2) + 4 * cells + (N_max + 15) // 16 * 16


def model_case(name):
    return mbm.LONG_CASES[CROSS[name][0] if name in CROSS else name]


def _last(corpus, n):
    keys = sorted(corpus[0])[-n:]
    return tuple({k: d[k] for k in keys} for d in corpus)


def heldout_inputs(name, held=HELD):
    """(embedding_mats, vec_ids_dict, durations_dict, landmarks_dict) of the held-out utterances of a case"""
    from segmentalist_amd.synth import make_corpus
    if name in FULL:
        from tests import fullcov_batch as fcb
        from tests import fullcov_wordseg as fw
        n_utt, D, K, seed, nmax, dtype, fb_type, N_range, variant, shift = fw.CASES[fcb.SAMPLED[name][0]]
        assert not shift
        return _last(make_corpus(n_utt + held, D, K, seed=seed, ragged=True, n_slices_max=nmax, dtype=dtype, noise=0.3,
                                 normalise=False, N_range=N_range), held)
    m = model_case(name)
    r = mbm.LONG_CASES[CROSS[name][1]] if name in CROSS else m
    assert (r["D"], r["cseed"]) == (m["D"], m["cseed"])
    if "N_range" in r:
        corpus = make_corpus(r["n_utt"] + held, r["D"], r["K"], seed=r["cseed"], ragged=True, n_slices_max=m["nmax"],
                             N_range=r["N_range"])
    else:
        corpus = make_corpus(r["n_utt"] + held, r["D"], r["K"], seed=r["cseed"], N=r["N"], n_slices_max=m["nmax"])
    return _last(corpus, held)


def min_duration_of(name):
    return 0 if name in FULL else model_case(name)["kw"].get("min_duration", 0)


_states = {}


def swept(name):
    """(oracle segmenter, batch specification) of a case after its own sweeps (shared: do not modify)"""
    if name not in _states:
        if name in FULL:
            from tests import fullcov_batch as fcb
            ci, K_max, B, S, n_sw, annealed = fcb.SAMPLED[name]
            assert not annealed
            ref, spec = fcb.spec_of(ci, K_max, B, S)
            for sw in range(n_sw):
                spec.sweep(sw)
        else:
            model = CROSS[name][0] if name in CROSS else name
            if model in _states:
                ref, spec = _states[model]
            else:
                ref, spec, _ = mbm.pair(model, product=False)
                for sw in range(mbm.n_sweeps(model)):
                    spec.sweep(sw)
                _states[model] = (ref, spec)
        _states[name] = (ref, spec)
    return _states[name]


def product_swept(name, **kw):
    """the product's segmenter of a case brought to the same state (its batch state live)"""
    import torch
    if name in FULL:
        from tests import fullcov_batch as fcb
        ci, K_max, B, S, n_sw, _ = fcb.SAMPLED[name]
        seg = fcb.product_of(ci, K_max, B, S, **kw)
        n = n_sw
    else:
        model = CROSS[name][0] if name in CROSS else name
        _, _, seg = mbm.pair(model, **kw)
        seg.set_fb_type("viterbi")
        n = mbm.n_sweeps(model)
    for _ in range(n):
        seg.batch_sweep_async()
    torch.cuda.synchronize()
    seg._df.check_status()
    return seg


class Tables(object):
    """the held-out utterances as the oracle's containers: stacked rows, Utterances with p_boundary_init = 0 (no np.random
    draw) and the model's n_slices_min / n_slices_max / min_duration"""

    def __init__(self, inputs, n_slices_min, n_slices_max, min_duration):
        mats, vec_ids_dict, durations_dict, landmarks_dict = inputs
        self.Xq, vec_ids, self.labels = no.process_embeddings(mats, vec_ids_dict)
        self.u = no.Utterances([len(landmarks_dict[k]) for k in self.labels], vec_ids, [durations_dict[k] for k in self.labels],
                               [landmarks_dict[k] for k in self.labels], p_boundary_init=0, n_slices_min=n_slices_min,
                               n_slices_max=n_slices_max, min_duration=min_duration)


def span_vec(u, i, density, time_power_term, wip):
    N = u.lengths[i]
    tri = (N * N + N) // 2
    vec = -np.inf * np.ones(tri)
    for j in range(tri):
        e = u.vec_ids[i, j]
        if e == -1:
            continue
        dur = u.durations[i, j]
        vec[j] = -np.inf if np.isnan(dur) else density[e] * dur ** time_power_term
    return vec + wip


def segments_of(u, i, bnd):
    """(start, end, embedding) of the segments the flags select, in landmark order; -1: the span has no embedding"""
    out, s = [], 0
    for t in range(1, u.lengths[i] + 1):
        if bnd[t - 1]:
            out.append((s, t, int(u.vec_ids[i, t * (t - 1) // 2 + s])))
            s = t
    return out


class Decoded(object):
    """what the specification says of a held-out set; the fields of segmentalist_amd's Decoded, and the span scores kept"""

    def __init__(self, tables, pred):
        u = tables.u
        self.tables, self.pred = tables, pred
        self.utterance_labels = tables.labels
        self.K = pred.K
        self.boundaries = np.zeros((u.D, u.N_max), bool)
        self.log_prob = np.zeros(u.D)
        self.vec = []
        self.seg_offsets = np.zeros(u.D + 1, np.int64)
        self.seg_start, self.seg_end, self.seg_embed, self.seg_label, self.seg_log_marg = [], [], [], [], []

    def close(self):
        for k, dt in (("seg_start", np.int64), ("seg_end", np.int64), ("seg_embed", np.int64), ("seg_label", np.int64),
                      ("seg_log_marg", np.float64)):
            setattr(self, k, np.array(getattr(self, k), dt))
        return self

    def transcript(self, i):
        return [int(k) for k in self.seg_label[self.seg_offsets[i]:self.seg_offsets[i + 1]]]


def decode_from(tables, pred, n_slices_min, n_slices_max, wip, time_power_term, census=None, pz=None):
    """boundaries, log_prob and segments from a Prediction of every candidate row (tests/fbgmm_predict.py)"""
    u = tables.u
    out = Decoded(tables, pred)
    for i in range(u.D):
        N = u.lengths[i]
        vec = span_vec(u, i, pred.density, time_power_term, wip)
        out.vec.append(vec)
        if census is not None:
            census.dp(vec, N, n_slices_max)
        lp, bnd = no.forward_backward_viterbi(vec, 0.0, N, n_slices_min, n_slices_max, i)
        out.log_prob[i] = lp
        out.boundaries[i, :N] = bnd
        for s, t, e in segments_of(u, i, bnd):
            out.seg_start.append(s)
            out.seg_end.append(t)
            out.seg_embed.append(e)
            out.seg_label.append(pred.label[e] if e >= 0 else -1)
            out.seg_log_marg.append(pred.density[e] if e >= 0 else -np.inf)
            if census is not None and e >= 0:
                census.slot(pz + pred.ll[e], pred.cnt)
        out.seg_offsets[i + 1] = len(out.seg_end)
    return out.close()


def decode(spec, inputs, min_duration=0, census=None):
    """The specification on the state of `spec` (oracle/np_fbgmm_batch.py FbgmmBatch or a subclass, any slots) for the
    held-out `inputs`.  census: a tests/map_batch.py Census that takes every DP step and the label decision of every chosen
    segment."""
    seg = spec.seg
    tables = Tables(inputs, seg.n_slices_min, seg.n_slices_max, min_duration)
    d = spec.derive(*spec.stats_excluding(-1))
    ll = np.array([spec.loglik(d, x) for x in tables.Xq]).reshape(len(tables.Xq), spec.K_max)
    pred = fp.functions_of(ll, d["cnt"], spec.alpha, spec.lms)
    pz = np.log(float(spec.alpha) / spec.K_max + d["cnt"])
    return decode_from(tables, pred, seg.n_slices_min, seg.n_slices_max, seg.wip, seg.time_power_term, census, pz)


_decoded = {}


def decoded(name):
    """(specification's Decoded, Census) of a case (shared: do not modify)"""
    if name not in _decoded:
        census = mbm.Census()
        _decoded[name] = (decode(swept(name)[1], heldout_inputs(name), min_duration_of(name), census), census)
    return _decoded[name]


# ------------------------------------------------------------------ the serial witness
HELD_PREFIX = "~"                # held-out keys sort behind every training key


def combined_inputs(train, held):
    """training plus held-out utterances as ONE corpus, the held-out ones last"""
    out = tuple(dict(d) for d in train)
    for d, h in zip(out, held):
        for k, v in h.items():
            d[HELD_PREFIX + k] = v
    return out


def train_inputs(name):
    if name in FULL:
        from tests import fullcov_batch as fcb
        from tests import fullcov_wordseg as fw
        return fw.case_corpus(fcb.SAMPLED[name][0])
    from tests import fbgmm_long
    return fbgmm_long.corpus_of(model_case(name))


class OracleImpl(object):
    """the serial building blocks the witness is assembled from: oracle/np_oracle.py (tests/fullcov_wordseg.py's
    specification classes for full covariance).  tests/golden/make_golden_decode.py has the same over the reference itself."""

    process_embeddings = staticmethod(no.process_embeddings)
    Utterances = no.Utterances
    viterbi = staticmethod(no.forward_backward_viterbi)

    def segmenter_class(self, name):
        if name in FULL:
            from tests import fullcov_wordseg as fw
            return fw.SpecWordseg
        return no.UnigramAcousticWordseg

    def acoustic_model(self, name, X, assignments):
        from tests.golden import cases
        if name in FULL:
            from tests import fullcov_batch as fcb
            from tests import fullcov_wordseg as fw
            ci, K_max = fcb.SAMPLED[name][:2]
            return fw.SpecWordsegFBGMM(X, fw.SpecPrior(*fw.prior_params(ci)), fw.ALPHA, K_max, assignments, lms=fw.LMS)
        from tests import fbgmm_long
        m = model_case(name)
        prior = (no.FixedVarPrior(*cases.fixed_prior_params(m["D"])) if m["kind"] == "fixed"
                 else no.NIW(*cases.diag_prior_params(m["D"])))
        return no.FBGMM(X, prior, 1.0, m["K"], assignments, covariance_type=m["kind"], lms=fbgmm_long.seg_args(m)["lms"])


def witness(name, impl):
    """The serial form of the definition: the segmenter class over training PLUS held-out utterances, the training rows on the
    specification's canonical assignments, the held-out tokens deleted (every held-out row at -1); per held-out utterance
    get_vec_embed_log_probs, forward_backward_viterbi, and per chosen segment map_assign_i on a deep copy of the acoustic
    model -- the model itself is never grown.  Returns dict(log_prob, boundaries, seg_offsets, seg_embed, seg_label,
    seg_log_marg, K), seg_embed in held-out row numbering.  No constructor of a segmenter runs (it would draw boundaries and
    assignments): the instance is given the attributes the two methods read."""
    import copy
    ref, spec = swept(name)
    seg_s = spec.seg
    inputs = combined_inputs(train_inputs(name), heldout_inputs(name))
    X, vec_ids, labels = impl.process_embeddings(inputs[0], inputs[1])
    u = impl.Utterances([len(inputs[3][k]) for k in labels], vec_ids, [inputs[2][k] for k in labels], [inputs[3][k] for k in labels],
                        p_boundary_init=0, n_slices_min=seg_s.n_slices_min, n_slices_max=seg_s.n_slices_max,
                        min_duration=min_duration_of(name))
    a, K = spec.canonical()
    n_train = len(a)
    assert np.array_equal(np.asarray(X[:n_train]), spec.X)
    am = impl.acoustic_model(name, np.asarray(X), np.concatenate([np.asarray(a, np.int64), np.full(len(X) - n_train, -1, np.int64)]))
    cls = impl.segmenter_class(name)
    seg = cls.__new__(cls)
    seg.acoustic_model, seg.utterances = am, u
    seg.wip, seg.time_power_term = seg_s.wip, seg_s.time_power_term
    held = [i for i, k in enumerate(labels) if k.startswith(HELD_PREFIX)]
    assert held == list(range(len(labels) - len(held), len(labels)))
    N_max = max(u.lengths[i] for i in held)
    out = dict(log_prob=np.zeros(len(held)), boundaries=np.zeros((len(held), N_max), bool),
               seg_offsets=np.zeros(len(held) + 1, np.int64), seg_embed=[], seg_label=[], seg_log_marg=[], K=np.int64(K))
    for r, i in enumerate(held):
        N = u.lengths[i]
        tri = (N * N + N) // 2
        vec = seg.get_vec_embed_log_probs(u.vec_ids[i, :tri], u.durations[i, :tri])
        lp, bnd = impl.viterbi(vec, 0.0, N, seg_s.n_slices_min, seg_s.n_slices_max, i)
        out["log_prob"][r] = lp
        out["boundaries"][r, :N] = bnd
        u.boundaries[i, :N] = bnd
        for e in u.get_segmented_embeds_i(i):
            e = int(e)
            if e == -1:
                out["seg_embed"].append(-1)
                out["seg_label"].append(-1)
                out["seg_log_marg"].append(-np.inf)
                continue
            other = copy.deepcopy(am)
            other.map_assign_i(e)
            out["seg_embed"].append(e - n_train)
            out["seg_label"].append(int(other.components.assignments[e]))
            out["seg_log_marg"].append(float(am.log_marg_i(e)))
        out["seg_offsets"][r + 1] = len(out["seg_embed"])
    assert int(am.components.K) == K and np.all(np.asarray(am.components.assignments)[n_train:] == -1)
    for k, dt in (("seg_embed", np.int64), ("seg_label", np.int64), ("seg_log_marg", np.float64)):
        out[k] = np.array(out[k], dt)
    return out


def rel(got, want):
    """largest relative difference, -inf matched exactly"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isneginf(got), np.isneginf(want)):
        return np.inf
    fin = ~np.isneginf(want)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))) if np.any(fin) else 0.0


def assert_equals_witness(dec, w, tol):
    assert dec.K == int(w["K"])
    assert np.array_equal(dec.boundaries, w["boundaries"])
    assert np.array_equal(dec.seg_offsets, w["seg_offsets"])
    assert np.array_equal(dec.seg_embed, w["seg_embed"]) and np.array_equal(dec.seg_label, w["seg_label"])
    worst = max(rel(dec.log_prob, w["log_prob"]), rel(dec.seg_log_marg, w["seg_log_marg"]))
    assert worst <= tol, worst
    return worst

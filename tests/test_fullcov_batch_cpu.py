"""The full-covariance batch specification (tests/fullcov_batch.py) on the CPU: the preconditions the device parity tests
rest on, the densities against the reference-pinned `SpecComponents`, and the degenerate case in which the batch statistics
are the serial chain's."""
import numpy as np
import pytest

from tests import fullcov_batch as fb
from tests import fullcov_wordseg as fw
from tests.map_batch import MARGIN, Census


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))) if a.size else 0.0


@pytest.fixture(scope="module")
def sampled_runs():
    """name -> (spec, margins) after the case's sampled sweeps; computed once."""
    out = {}
    for name, (ci, K, B, S, n, annealed) in fb.SAMPLED.items():
        seg, spec = fb.spec_of(ci, K, B, S)
        spec.margins = fb.Margins()
        temps = fb.anneal_temps(n) if annealed else [1.0] * n
        for s in range(n):
            spec.sweep(s, temps[s], annealed)
        out[name] = spec
    return out


@pytest.mark.parametrize("name", list(fb.SAMPLED))
def test_sampled_preconditions(sampled_runs, name):
    spec = sampled_runs[name]
    m = spec.margins
    print("%s: least draw margin boundary %.3g slot %.3g" % (name, m.boundary, m.slot))
    assert m.boundary >= fb.DRAW_MARGIN and m.slot >= fb.DRAW_MARGIN
    cnt = spec.stats_excluding(-1)[0]
    assert np.count_nonzero(cnt == 0) >= 1                 # the prior predictive of an empty slot is exercised
    if name == "w6_long":
        assert sum(lo == hi for row in spec.ranges for (lo, hi) in row) >= 1


@pytest.mark.parametrize("name", list(fb.MAP) + list(fb.MIXED))
def test_map_preconditions(name):
    if name in fb.MAP:
        ci, K, B, S, n_map = fb.MAP[name]
        n_sampled = 0
    else:
        ci, K, B, S, n_sampled, n_map = fb.MIXED[name]
    seg, spec = fb.spec_of(ci, K, B, S, map_batch=True)
    spec.margins = fb.Margins()
    for s in range(n_sampled):
        spec.sweep(s, viterbi=False)
    if n_sampled:
        # (FbgmmBatch.sweep runs behind MapBatch.sweep: the margins are taken by a second specification)
        seg2, spec2 = fb.spec_of(ci, K, B, S)
        spec2.margins = fb.Margins()
        for s in range(n_sampled):
            spec2.sweep(s)
        assert np.array_equal(spec2.slot, spec.slot)
        assert spec2.margins.boundary >= fb.DRAW_MARGIN and spec2.margins.slot >= fb.DRAW_MARGIN
    spec.census = cen = Census()
    for s in range(n_sampled, n_sampled + n_map):
        spec.sweep(s)
    print("%s: dp margin %.3g slot margin %.3g tokens %d" % (name, cen.dp_margin, cen.slot_margin, cen.tokens))
    assert cen.dp_margin >= MARGIN and cen.slot_margin >= MARGIN
    assert cen.tie_on_occupied == 0 and cen.softmax_disagrees == 0
    assert np.count_nonzero(spec.stats_excluding(-1)[0] == 0) >= 1


@pytest.mark.parametrize("name", ["w0_K8", "w3_f64", "w4_D33", "w7_shift"])
def test_densities_against_spec_components(sampled_runs, name):
    """After the sweeps, for a block b: SpecComponents built from the canonical labels of the tokens outside b gives the
    predictive values and the statistics FullcovBatch derives from its partial sums (other summation orders)."""
    spec = sampled_runs[name]
    b = spec.B - 1
    cnt, sx, sxx = spec.stats_excluding(b)
    d = spec.derive(cnt, sx, sxx)
    inside = np.zeros(len(spec.slot), bool)
    for s in range(spec.S):
        for i in range(*spec.ranges[s][b]):
            inside[spec._tokens(i)] = True
    occ = np.where(cnt > 0)[0]
    remap = -np.ones(spec.K_max, np.int64)
    remap[occ] = np.arange(len(occ))
    canon = np.where((spec.slot >= 0) & ~inside, remap[np.maximum(spec.slot, 0)], -1)
    c = fb.spec_components(spec, canon)
    assert c.K == len(occ)
    assert np.array_equal(c.counts[:c.K], cnt[occ])
    assert _rel(d["m_num"][occ], c.m_N_numerators[:c.K]) <= 1e-13
    assert _rel(d["S"][occ], c.S_N_partials[:c.K]) <= 1e-13
    assert _rel(d["logdet"][occ], c.logdet_covars[:c.K]) <= 1e-9
    rows = np.unique(np.linspace(0, len(spec.slot) - 1, 12).astype(np.int64))
    for i in rows:
        ll = spec.loglik(d, spec.X[i])
        assert _rel(ll[occ], c.log_post_pred(i)) <= 1e-9
        empty = np.where(cnt == 0)[0]
        assert _rel(ll[empty], np.full(len(empty), c.log_prior(i))) <= 1e-9
        assert _rel(spec.log_prior_pred(spec.X[i]), c.cached_log_prior[i]) <= 1e-9


def test_one_utterance_per_block_is_the_serial_statistics():
    """With one utterance per block and S = 1, stats_excluding(b) are the serial specification's statistics after deleting
    that utterance's items."""
    ci, K = 0, 8
    n_utt = fw.CASES[ci][0]
    seg, spec = fb.spec_of(ci, K, n_utt, 1)
    for b in (0, 7, n_utt - 1):
        assert spec.ranges[0][b] == (b, b + 1)
        seg2 = fb.make_spec_seg(ci, K)
        c = seg2.acoustic_model.components
        assert np.array_equal(c.assignments, spec.slot)
        for e in seg2.utterances.get_segmented_embeds_i(b):
            if e != -1:
                c.del_item(e)
        cnt, sx, sxx = spec.stats_excluding(b)
        d = spec.derive(cnt, sx, sxx)
        occ = np.where(cnt > 0)[0]
        assert len(occ) == c.K
        for k in occ:
            e = np.where((spec.slot == k) & (c.assignments >= 0))[0][0]        # a token outside the utterance names the serial label
            ks = c.assignments[e]
            assert cnt[k] == c.counts[ks]
            assert _rel(d["m_num"][k], c.m_N_numerators[ks]) <= 1e-13
            assert _rel(d["S"][k], c.S_N_partials[ks]) <= 1e-13

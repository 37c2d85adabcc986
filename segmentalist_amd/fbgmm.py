"""
Drop-in for segmentalist/fbgmm.py: finite Bayesian Gaussian mixture model, device backed.
"""
import logging
import random
import time

import numpy as np
from scipy.special import gammaln

from .gaussian_components import GaussianComponents
from .gaussian_components_diag import GaussianComponentsDiag
from .gaussian_components_fixedvar import GaussianComponentsFixedVar
from ._abi import SegkError
from .kmeans import _consecutive

logger = logging.getLogger(__name__)


class FBGMM(object):
    def __init__(self, X, prior, alpha, K, assignments="rand", covariance_type="full", lms=1.0, _corpus=None,
                 sync="sequential", n_gibbs_blocks=8, n_stat_blocks=8, batch_seed=0, score_precision="f64"):
        """fbgmm.py:43-91.  sync: the mode of gibbs_sample -- "sequential" is the reference's serial chain over the items
        (draw for draw); "batch" the batch-synchronous blocked Gibbs sampler specified in tests/fbgmm_items.py (the items cut
        into n_stat_blocks slices x n_gibbs_blocks blocks, every block resampled in parallel against the statistics of all
        other blocks, uniforms from the counter-based stream of batch_seed).  The two modes mix freely: gibbs_sample(...,
        sync=...) chooses per call, batch_sweep_async() / materialise() are the asynchronous form.  Direct calls of
        components.add_item / del_item between batch sweeps are not intercepted: call materialise() first; the next batch
        sweep then has to re-enter from the serial state (`_leave_batch()`).
        score_precision: the arithmetic of the batch sweeps' item likelihoods -- "f64", or "f32" with covariance_type="diag":
        the Student-t terms in float32 on the hardware logarithm, within 1e-4 max(|ll|, 1) of the fp64 likelihoods (the
        tolerance contract of the segmenter's score_precision="f32"); statistics, logits and draws stay fp64.  The serial
        sweeps are fp64 either way."""
        assert sync in ("sequential", "batch")
        if score_precision not in ("f64", "f32"):
            raise SegkError("FBGMM takes score_precision 'f64' or 'f32', got %r" % (score_precision,))
        if score_precision == "f32" and covariance_type != "diag":
            raise SegkError("score_precision='f32' exists for diagonal components only (covariance_type=\"diag\", got %r)"
                            % (covariance_type,))
        self.score_precision = score_precision
        self.sync = sync
        self._batch_args = (n_gibbs_blocks, n_stat_blocks, batch_seed)
        self._sweeper = None
        self.alpha = alpha
        self.prior = prior
        self.covariance_type = covariance_type
        self.lms = lms
        self._corpus = _corpus
        self.setup_components(K, assignments, X)

    def setup_components(self, K, assignments="rand", X=None):
        """fbgmm.py:93-137."""
        self._leave_batch()
        self._sweeper = None                # (bound to the components it was built from)
        self._sweep_index = 0               # the counter a new sweeper starts from (set_K carries the old one over)
        if X is None:
            assert hasattr(self, "components")
            X = self.components.X
        N, D = X.shape
        if isinstance(assignments, str) and assignments == "rand":
            assignments = np.random.randint(0, K, N)
        elif isinstance(assignments, str) and assignments == "each-in-own":
            assignments = np.arange(N)
        assignments = _consecutive(np.asarray(assignments))
        kw = dict(_corpus=self._corpus, _alpha=self.alpha, _lms=self.lms)
        if self.covariance_type == "diag":
            self.components = GaussianComponentsDiag(X, self.prior, assignments, K_max=K, **kw)
        elif self.covariance_type == "fixed":
            self.components = GaussianComponentsFixedVar(X, self.prior, assignments, K_max=K, **kw)
        elif self.covariance_type == "full":
            # (the reference would die on a prior without S_0 with an AttributeError further down)
            if np.asarray(getattr(self.prior, "S_0", None)).shape != (D, D):
                raise NotImplementedError("full covariance needs a NIW prior with a D×D S_0")
            self.components = GaussianComponents(X, self.prior, assignments, K_max=K, **kw)
        else:
            assert False, "Invalid covariance type."

    def set_K(self, K, reassign=True, sync=None):
        """fbgmm.py:139-180: keep the `K` largest components -- the kept component at rank r of the ascending order of the
        counts gets label r --, rebuild the bank with K_max = K (`setup_components`), and with `reassign` re-home every
        orphan: an item that was assigned and whose component went.

        sync: None = the mode the object was built with.  "sequential" is the reference's form, draw for draw: the orphans
        in index order through gibbs_sample_inside_loop_i at temperature 1, one random.random() each (one call of the serial
        item kernel over the orphan list).  "batch": the same ranking, relabelling and rebuild, then ONE blocked pass over
        the orphans (specification tests/fbgmm_set_k.py): per block the statistics of every item that holds a slot, a draw
        for each of the block's orphans from the counter-based stream of batch_seed, the orphans of later blocks seeing
        those placed in earlier ones; no random.random() is consumed, the likelihoods are fp64 whatever score_precision,
        the sweep counter goes on from where it stood, and the model is left in batch state (materialise() brings
        `components` up to date, as after batch_sweep_async()).

        Ties: the ranking is np.argsort(counts, kind="stable") on all K_max counts (zeros for the inactive components).
        The reference sorts with NumPy's default kind, which is not stable: among components of equal size its choice
        depends on the NumPy build and the CPU's vector extensions.  With pairwise distinct counts the two agree.

        `components.K <= K`: the reference only overwrites the attribute K_max; its arrays keep their old length and its own
        gibbs_sample then fails on the mismatch.  Here the bank is rebuilt at the new size from the current assignments: K,
        counts, assignments and statistics unchanged, K_max = K -- the model equals FBGMM(X, prior, alpha, K,
        assignments=current).  No uniform is consumed.

        Refused on the acoustic model of a segmenter: the segmenter holds the device object that the rebuild replaces."""
        assert sync in (None, "sequential", "batch")
        sync = self.sync if sync is None else sync
        K = int(K)
        if self.components.dev.corpus.n_utt:
            raise SegkError("set_K: this mixture model is the acoustic model of a segmenter (its corpus carries utterances); "
                            "the segmenter holds the device object that setup_components would replace")
        if K < 1:
            raise SegkError("set_K takes K >= 1, got %d" % K)
        sweep_index = 0 if self._sweeper is None else self._sweeper.sweep_index
        if sync == "batch":
            self._get_sweeper()             # (the refusals, before anything runs)
        self._leave_batch()                 # (materialise(): the reference's view is what is ranked)
        c = self.components
        old = c.assignments
        if c.K <= K:
            new = old
        else:
            keep = np.argsort(c.counts, kind="stable")[-K:]
            table = np.full(c.K_max + 1, -1, dtype=np.int64)            # (the last entry serves the label -1)
            table[keep] = np.arange(K)
            new = table[old]
        self.setup_components(K, new)
        self._sweep_index = sweep_index
        orphans = np.flatnonzero((old != -1) & (new == -1))
        if sync == "batch":
            sw = self._get_sweeper()
            sw.enter()
            if reassign and len(orphans):
                sw.reassign_orphans(old)
        elif reassign and len(orphans):
            dev = self.components.dev
            used = dev.gibbs_items([random.random() for _ in orphans], True, 1, ids=orphans)
            dev.check_status()
            assert used == len(orphans)

    # record metrics (host, from device snapshots) ------------------------------------------------
    def log_prob_z(self):
        """fbgmm.py:208-225."""
        counts = self.components.counts
        K_max = self.components.K_max
        return (gammaln(self.alpha) - gammaln(self.alpha + np.sum(counts))
                + np.sum(gammaln(counts + float(self.alpha) / K_max) - gammaln(self.alpha / K_max)))

    def log_prob_X_given_z(self):
        return self.components.log_marg()

    def log_marg(self):
        return self.log_prob_z() + self.log_prob_X_given_z()

    # batch mode ------------------------------------------------------------------------------------
    def _get_sweeper(self):
        if self._sweeper is None:
            from .device import FbgmmItemSweeper
            B, S, seed = self._batch_args
            self._sweeper = FbgmmItemSweeper(self.components.dev, B, S, seed, score_precision=self.score_precision)
            self._sweeper.sweep_index = self._sweep_index
        return self._sweeper

    def batch_sweep_async(self, anneal_temp=1, consider_unassigned=True, map_assign=False):
        """Enqueue one batch-synchronous sweep over the items; results stay on the device (materialise() brings
        `components` up to date).  map_assign: a MAP sweep (see map_assign; anneal_temp is not used), its moved items
        counted on the device."""
        self._get_sweeper().sweep(float(anneal_temp), consider_unassigned, map_assign)

    def materialise(self):
        """Bring the reference's view (components.K / assignments / statistics) up to date with the batch state."""
        if self._sweeper is not None:
            self._sweeper.materialise()

    def _leave_batch(self):
        if getattr(self, "_sweeper", None) is not None and self._sweeper.in_batch_state:
            self.materialise()
            self._sweeper.invalidate()

    # hot path --------------------------------------------------------------------------------------
    def log_marg_i(self, i):
        """fbgmm.py:256-285 (A4), on the device."""
        assert i != -1
        self._leave_batch()
        return float(self.components.dev.log_marg_rows([i])[0])

    def gibbs_sample_inside_loop_i(self, i, anneal_temp=1):
        """fbgmm.py:422-463 (A10); consumes one random.random() like the reference."""
        self._leave_batch()
        self.components.dev.assign_item(i, random.random(), anneal_temp, map_assign=False)

    def map_assign_i(self, i):
        """fbgmm.py:465-494."""
        self._leave_batch()
        self.components.dev.assign_item(i, 0.0, 1.0, map_assign=True)

    def gibbs_sample(self, n_iter, consider_unassigned=True, anneal_schedule=None, anneal_start_temp_inv=0.1,
                     anneal_end_temp_inv=1, n_anneal_steps=-1, sync=None):
        """fbgmm.py:288-420 on the device: per iteration one kernel walks the items in index order
        (cache statistics, del_item, logits, draw, restore or add_item); the uniforms are the
        `random.random()` values the reference would consume -- one per considered item.
        sync: None = the mode the object was built with; "batch" = the sweeps of this call as batch-synchronous sweeps
        (no random.random() is consumed), the record taken from the reference's view after every sweep."""
        assert sync in (None, "sequential", "batch")
        sync = self.sync if sync is None else sync
        if sync == "batch":
            self._get_sweeper()             # (the refusals, before anything runs)
        else:
            self._leave_batch()
        record_dict = {k: [] for k in ["sample_time", "log_marg", "log_prob_z", "log_prob_X_given_z",
                                       "anneal_temp", "components"]}
        start_time = time.time()
        if anneal_schedule is None:
            get_anneal_temp = iter([])
        elif anneal_schedule == "linear":
            if n_anneal_steps == -1:
                n_anneal_steps = n_iter
            get_anneal_temp = iter(1. / np.linspace(anneal_start_temp_inv, anneal_end_temp_inv, n_anneal_steps))
        elif anneal_schedule == "step":
            assert not n_anneal_steps == -1, "`n_anneal_steps` of -1 not allowed for step annealing schedule"
            n_iter_per_step = int(round(float(n_iter) / n_anneal_steps))
            anneal_list = 1. / np.linspace(anneal_start_temp_inv, anneal_end_temp_inv, n_anneal_steps)
            get_anneal_temp = iter(np.repeat(anneal_list, n_iter_per_step))
        else:
            assert False, "invalid anneal_schedule"
        c = self.components
        dev = c.dev
        for i_iter in range(n_iter):
            anneal_temp = next(get_anneal_temp, anneal_end_temp_inv)
            if sync == "batch":
                self.batch_sweep_async(anneal_temp, consider_unassigned)
                self.materialise()              # the record reads the reference's view
                dev.check_status()
            else:
                n_draws = c.N if consider_unassigned else int(np.count_nonzero(c.assignments != -1))
                used = dev.gibbs_items([random.random() for _ in range(n_draws)], consider_unassigned, anneal_temp)
                dev.check_status()
                assert used == n_draws
            record_dict["sample_time"].append(time.time() - start_time)
            start_time = time.time()
            record_dict["log_marg"].append(self.log_marg())
            record_dict["log_prob_z"].append(self.log_prob_z())
            record_dict["log_prob_X_given_z"].append(self.log_prob_X_given_z())
            record_dict["anneal_temp"].append(anneal_temp)
            record_dict["components"].append(c.K)
            info = "iteration: " + str(i_iter)
            for key in sorted(record_dict):
                info += ", " + key + ": " + str(record_dict[key][-1])
            logger.info(info)
        return record_dict

    def map_assign(self, n_iter, consider_unassigned=True, sync=None, until_converged=False):
        """`n_iter` MAP sweeps over the items: the hard assignment of map_assign_i (fbgmm.py:465-494) in place of the draw
        of a Gibbs sweep -- the way a sampler run is settled into a reproducible labelling.
        sync: None = the mode the object was built with.
          "sequential"  per considered item in index order cache_component_stats, del_item, k = the first maximum of
                        log(alpha / K_max + counts) + log predictive (no lms), `k > K -> K`, then restore or add_item
                        (fbgmm.py:352-405 with 371-389 replaced by 475-491), one kernel per sweep; fp64.
          "batch"       the blocked sweeps of gibbs_sample(sync="batch") with the first slot of the largest logit in place
                        of the draw (specification tests/fbgmm_items_map.py); the likelihoods in the model's
                        score_precision; each sweep takes one value of the sweep counter.
        No random.random() and no uniform of batch_seed is consumed.  Returns the record of gibbs_sample without
        "anneal_temp" and with "n_moved": per sweep the items whose component (batch: slot) changed.  A sweep with
        n_moved == 0 is a fixed point: every later MAP sweep changes nothing.  until_converged: stop after the first such
        sweep; n_iter is then the cap."""
        assert sync in (None, "sequential", "batch")
        sync = self.sync if sync is None else sync
        if sync == "batch":
            sw = self._get_sweeper()        # (the refusals, before anything runs)
        else:
            self._leave_batch()
        c = self.components
        dev = c.dev
        if sync != "batch" and dev.lm is not None:
            raise SegkError("map_assign: map_assign_i has no language-model variant")
        record_dict = {k: [] for k in ["sample_time", "log_marg", "log_prob_z", "log_prob_X_given_z", "components", "n_moved"]}
        start_time = time.time()
        for i_iter in range(n_iter):
            if sync == "batch":
                self.batch_sweep_async(1, consider_unassigned, map_assign=True)
                self.materialise()              # the record reads the reference's view
                n_moved = sw.moved()
            else:
                n_moved = dev.map_items(consider_unassigned)
            dev.check_status()
            record_dict["sample_time"].append(time.time() - start_time)
            start_time = time.time()
            record_dict["log_marg"].append(self.log_marg())
            record_dict["log_prob_z"].append(self.log_prob_z())
            record_dict["log_prob_X_given_z"].append(self.log_prob_X_given_z())
            record_dict["components"].append(c.K)
            record_dict["n_moved"].append(n_moved)
            info = "iteration: " + str(i_iter)
            for key in sorted(record_dict):
                info += ", " + key + ": " + str(record_dict[key][-1])
            logger.info(info)
            if until_converged and n_moved == 0:
                break
        return record_dict

    # held-out rows -----------------------------------------------------------------------------------
    def _predict(self, Xq, device_out, **want):
        sw = self._get_sweeper()        # (the item sweeper's refusals)
        return sw.predict(Xq, device_out=device_out, **want)

    def predict(self, Xq, device_out=False):
        """Labels of held-out rows `Xq` [M, D] (NumPy or a device tensor; converted to the model's dtype): each row is an
        UNASSIGNED item appended to X, labelled as map_assign_i (fbgmm.py:475-491) would label it against the statistics of
        all assigned items -- the first maximum of log(alpha / K_max + counts) + log predictive, no lms -- without adding it.
        int64 [M] in the numbering of `components` (after materialise()); K means "would found a new component".

        Read-only: assignments, K, counts, the statistics, a batch state's slots and partial sums and the sweep counter stay
        bit for bit; no random.random() and no uniform of batch_seed is consumed.  A model in batch state is used as it
        stands (no materialise()).  The likelihoods follow score_precision, as map_assign(sync="batch") does.  device_out:
        a device tensor, without a synchronisation.  Refused on the acoustic model of a segmenter, with more than one rank
        and beyond the full-covariance limits (D <= 64, K_max <= 1024)."""
        return self._predict(Xq, device_out, want_label=True, want_density=False, want_resp=False)[0]

    def score_samples(self, Xq, device_out=False):
        """Log densities of held-out rows, float64 [M]: log_marg_i (fbgmm.py:256-285, lms included) of each row appended
        unassigned.  Read-only like predict."""
        return self._predict(Xq, device_out, want_label=False, want_density=True, want_resp=False)[1]

    def predict_log_proba(self, Xq, device_out=False):
        """Log responsibilities of held-out rows, float64 [M, K_max]: the normalised log_prob_z of
        gibbs_sample_inside_loop_i (fbgmm.py:436-451) at temperature 1 of each row appended unassigned, columns as in
        `components`: the K active components, then the empty ones.  Read-only like predict."""
        return self._predict(Xq, device_out, want_label=False, want_density=False, want_resp=True)[2]

    def get_n_assigned(self):
        """Number of assigned items (the reference counts `assignments != -1`): the sum of the component counts, read
        from the device without copying the assignment vector to the host."""
        return int(self.components.dev.counts.sum().item())

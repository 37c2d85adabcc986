"""
Drop-in for segmentalist/kmeans.py: the k-means acoustic model (`KMeans`).
"""
import logging
import time

import numpy as np

from . import rng
from .kmeans_components import KMeansComponents

logger = logging.getLogger(__name__)


def _consecutive(assignments):
    """Relabel so that the used labels are 0..max without gaps (kmeans.py:88-92)."""
    for k in range(assignments.max()):
        while len(np.nonzero(assignments == k)[0]) == 0:
            assignments[np.where(assignments > k)] -= 1
        if assignments.max() == k:
            break
    return assignments


class KMeans(object):
    def __init__(self, X, K, assignments="rand", _corpus=None, _shard=None):
        self._corpus = _corpus
        self._shard = _shard         # (row_lo, row_hi): the device holds a shard of X (multi-rank batch mode)
        self.setup_components(K, assignments, X)

    def setup_components(self, K, assignments="rand", X=None):
        """kmeans.py:52-94."""
        if X is None:
            assert hasattr(self, "components")
            X = self.components.X
        N, D = X.shape
        if isinstance(assignments, str) and assignments == "rand":
            assignments = np.random.randint(0, K, N)
        elif isinstance(assignments, str) and assignments == "each-in-own":
            assignments = np.arange(N)
        elif isinstance(assignments, str) and assignments == "spread":
            spread = (list(range(K)) * int(np.ceil(float(N) / K)))[:N]
            rng.shuffle(spread)
            assignments = np.array(spread)
        assignments = _consecutive(np.asarray(assignments))
        self.components = KMeansComponents(X, assignments, K, _corpus=self._corpus, _shard=getattr(self, "_shard", None))

    def fit(self, n_iter, consider_unassigned=True, no_empty=True, on_device=False, _n_items_bound=None):
        """
        kmeans.py:97-173: batch (Lloyd) iterations -- every considered item gets the argmax of
        `neg_sqrd_norm` against the means frozen at the start of the iteration, then the changed
        items are moved (del_item/add_item in item order) and empty components removed.
        on_device=True: every iteration is one library call and one small device-to-host copy (DeviceKMeans.fit_step,
        DESIGN.md 4.19) -- no launch per item, no host loop over items, the label vectors stay on the device; the same
        state and the same record, bit for bit (sum_neg_sqrd_norm to its usual tolerance).
        """
        c = self.components
        dk = c.dev
        dk.require_whole_corpus("KMeans.fit")
        record_dict = {"sum_neg_sqrd_norm": [], "components": [], "n_mean_updates": [], "sample_time": []}
        start_time = time.time()
        if on_device:
            # _n_items_bound: what the caller knows about the number of labelled rows (consider_unassigned=False); from the
            # second iteration on the record has the number itself -- moving items does not change it
            bound = None if consider_unassigned else _n_items_bound
            for i_iter in range(n_iter):
                moved, n_comp, n_items, sum_neg = dk.fit_step(consider_unassigned, bound)
                if not consider_unassigned:
                    bound = n_items
                record_dict["sum_neg_sqrd_norm"].append(sum_neg)
                record_dict["components"].append(n_comp)
                record_dict["n_mean_updates"].append(moved)
                record_dict["sample_time"].append(time.time() - start_time)
                start_time = time.time()
                info = "iteration: " + str(i_iter)
                for key in sorted(record_dict):
                    info += ", " + key + ": " + str(record_dict[key][-1])
                logger.info(info)
                if moved == 0:
                    break
            return record_dict
        for i_iter in range(n_iter):
            old = c.assignments
            items = np.arange(c.N) if consider_unassigned else np.where(old != -1)[0]
            _, new_k, _ = dk.exact_max(items.astype(np.int32)) if len(items) else (None, np.zeros(0, int), 0)
            moved = np.where(new_k != old[items])[0]
            for j in moved:
                i = int(items[j])
                dk.del_item(i)
                dk.add_item(i, int(new_k[j]))
            dk.check_status()
            dk.clean_components()

            record_dict["sum_neg_sqrd_norm"].append(c.sum_neg_sqrd_norm())
            record_dict["components"].append(c.K)
            record_dict["n_mean_updates"].append(len(moved))
            record_dict["sample_time"].append(time.time() - start_time)
            start_time = time.time()
            info = "iteration: " + str(i_iter)
            for key in sorted(record_dict):
                info += ", " + key + ": " + str(record_dict[key][-1])
            logger.info(info)
            if len(moved) == 0:
                break
        return record_dict

    def predict(self, Xq, return_score=False):
        """Rows that are NOT in the model against the means as they stand, read-only: per row of Xq
        [M, D] the raw argmax row of `means` over all K_max rows, inactive ones included (argmax_neg_sqrd_norm_i of the row
        appended to X, kmeans_components.py:231-232, first maximum; min(row, K) is the component add_item would give it),
        and with return_score=True also max_neg_sqrd_norm (:228-229) in the dtype of X -> int64 [M] or (int64 [M], [M]).
        Xq is converted to the dtype of X.  One segk_kmeans_score on a context of the model's own, into candidate buffers
        of the call's own: no statistic, no hint of the next sweep and no random state changes.
        Raises SegkError before any launch for more than one rank, a sharded corpus and a D other than the model's."""
        from .device import DeviceCorpus
        dk = self.components.dev
        Xq = np.asarray(Xq)
        if Xq.ndim != 2:
            raise ValueError("predict takes a matrix [M, D], got shape %r" % (Xq.shape,))
        dk.check_heldout(Xq.shape[1], "KMeans.predict")
        dtype = dk.corpus.x_np_dtype
        if Xq.shape[0] == 0:
            return (np.zeros(0, np.int64), np.zeros(0, dtype)) if return_score else np.zeros(0, np.int64)
        _, t = dk.score_heldout(DeviceCorpus(Xq.astype(dtype, copy=False)))
        rows = t[0].cpu().numpy().astype(np.int64)
        return (rows, t[2].cpu().numpy().astype(dtype)) if return_score else rows

    def get_n_assigned(self):
        """Number of assigned items (the reference counts `assignments != -1`): the sum of the component counts, read
        from the device without copying the assignment vector to the host."""
        return int(self.components.dev.counts.sum().item())

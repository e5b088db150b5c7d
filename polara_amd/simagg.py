"""Similarity aggregation, the content-based baselines of the reference's experiments, on the device:
`SimilarityAggregation` ('SIM', hybrid/models.py:25-44: s_u = sum_i t_ui S[., i] over the item similarity) and
`SimilarityAggregationItemColdStart` ('SIM(cs)', coldstart/models.py:101-119: s_c = sum_i sim[c, i] A[., i] over the
training matrix).  Both are one row-wise sparse x sparse product with the per-row top-k fused in (csrc/simagg.hip), whose
sums run in the order of SciPy's product: scores are bit-equal to the reference's, lists a function of the inputs alone.

The first part is the host-side planning of that kernel, pure Python: the values mirror the library's own planning
function (pk_spsp_topk_work_bytes; tests/test_sim_host.py holds the two together)."""
from timeit import default_timer as timer

import numpy as np

from . import i2i
from .coldstart import ItemColdStartEvaluationMixin
from .models import RecommenderModel, _ItemWeightModel, _setting

MAX_TOPK = i2i.MAX_TOPK        # the window candidates are merged by the item-to-item merge kernel: its limit
WINDOW = i2i.WINDOW            # columns of the product one workgroup accumulates in LDS (2048 fp64 accumulators, 16 KiB)
QUARTER = WINDOW // 4          # columns of one wave of the workgroup
LDS_BYTES = WINDOW * 8 + WINDOW * 4 + WINDOW // 8     # accumulators / score keys, item keys, seen bitmap


def n_windows(n_cols):
    return -(-int(n_cols) // WINDOW)


def chunk_rows(n_rows, n_cols, topk):
    """Rows per launch pair of pk_spsp_topk: every row keeps pow2(topk) keys of 12 bytes per window, as in pk_i2i_topk."""
    return i2i.chunk_users(n_rows, n_cols, topk)


def topk_work_bytes(n_rows, n_cols, topk):
    return i2i.topk_work_bytes(n_rows, n_cols, topk)


def check_shapes(l_shape, b_shape):
    """(n_rows, n_inner, n_cols) of the product L B."""
    n_rows, n_inner = (int(x) for x in l_shape)
    if int(b_shape[0]) != n_inner:
        raise ValueError('sparse product: L has %d columns, B has %d rows' % (n_inner, int(b_shape[0])))
    return n_rows, n_inner, int(b_shape[1])


def canonical_csr(m, shape=None):
    """A SciPy CSR copy of `m` (sparse or ndarray) as the kernel wants it: fp64, duplicates summed, strictly increasing
    columns per row."""
    from scipy.sparse import csr_matrix
    m = csr_matrix(m, dtype=np.float64, copy=True)
    if shape is not None and m.shape != tuple(shape):
        raise ValueError('a similarity of shape %s where %s is expected' % (m.shape, tuple(shape)))
    m.sum_duplicates()
    m.sort_indices()
    return m


def stored_csr(m, shape=None):
    """`m` as an fp64 SciPy CSR with every row in its stored order (the left operand: its rows need not be sorted — the
    sums follow the stored order, as SciPy's do)."""
    from scipy.sparse import csr_matrix
    m = csr_matrix(m, dtype=np.float64)
    if shape is not None and m.shape != tuple(shape):
        raise ValueError('a similarity of shape %s where %s is expected' % (m.shape, tuple(shape)))
    return m


def _ones(values):
    """Every nonzero value replaced by 1 (stored zeros stay: seen, no score)."""
    return (values != 0).to(values.dtype)


class SimilarityAggregation(_ItemWeightModel):
    """'SIM' (hybrid/models.py:25-44): the scores of a test user are its known feedback aggregated over the item
    similarity S = `data.item_relations` with the diagonal set to 0.  `dense_output=False` computes T S^T like the
    reference's `T.dot(S.T)` and keeps the sparse branch's candidates (nonzero scores, minus the seen items under
    `filter_seen`, pads -1); `dense_output=True` computes T S, which is what the reference's other branch does (its
    `csc_matvec` walks the CSR arrays of S row by row), with every item a candidate.  For a symmetric S the two products
    are the same.  `implicit` replaces the nonzero TEST values by 1 (`ones_like` after get_test_matrix has dropped zero feedback, models.py:197-201:
    negative feedback counts as 1, zero feedback only as seen).  Candidate rules,
    tie order and `topk` checks are CooccurrenceModel's; INTEGRATION.md §11 lists the differences from the reference."""
    _topk_limit = MAX_TOPK
    _weight_slots = ('_S', '_St')
    _operand_noun = 'similarity'
    _implicit_rule = staticmethod(_ones)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'SIM'

    implicit = _setting('implicit', '_refresh_model', 'nonzero test feedback replaced by 1: new lists, same model')

    @property
    def item_similarity_matrix(self):
        """The device CSR of S with the diagonal removed (None before the build)."""
        return self._S

    def build(self):
        """hybrid/models.py:33-37: a copy of the item relations without the diagonal and without explicit zeros, as a
        canonical device CSR, and its transpose."""
        self._single_process()
        rel = getattr(self.data, 'item_relations', None)
        if rel is None:
            raise ValueError('%s needs item relations: the data model has none (data.item_relations is None)' % self.method)
        start = timer()
        S = canonical_csr(rel)
        n_items = S.shape[0]
        if S.shape[0] != S.shape[1]:
            raise ValueError('item relations of shape %s are not square' % (S.shape,))
        S.setdiag(0)
        S.eliminate_zeros()
        ops = self.ops
        self._S = ops.csr(S.indptr, S.indices, S.data, S.shape)
        self._St = self._S.T
        ops.synchronize()
        self._track(start)
        self.build_stats = {'n_items': n_items, 'nnz': int(S.nnz), 'fill': S.nnz / float(n_items * n_items)}

    def _operand(self):
        return self._S if self.dense_output else self._St


class SimilarityAggregationItemColdStart(ItemColdStartEvaluationMixin, RecommenderModel):
    """'SIM(cs)' (coldstart/models.py:101-119): a cold item scores a training user with the user's feedback aggregated over
    the item's similarity to the training items, `data.cold_items_similarity` [cold items x training items]; the lists
    hold internal user ids (sparse branch: users with a nonzero score, pads -1; nothing is seen).  `implicit` replaces the
    TRAINING values by 1.  `dense_output=True` is not offered: the reference's own branch fails for this model (its
    `csc_matvec` is handed the user x item CSR and indexes the row pointer with item ids).  `representative_users` are not
    consulted, as in the reference."""
    _topk_limit = MAX_TOPK

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'SIM(cs)'
        self._implicit = False
        self._dense_output = False
        self._At = None
        self.build_stats = {}

    implicit = _setting('implicit', '_renew_model', 'training feedback replaced by 1: a new model')
    dense_output = _setting('dense_output', '_refresh_model', 'only the sparse branch exists: True raises at scoring time')

    def _renew_model(self):
        super()._renew_model()
        self._At = None

    def _check_branch(self):
        if self.dense_output:
            raise NotImplementedError('%s: dense_output=True is not supported — the reference\'s dense branch fails for this '
                                      'model (a broadcast ValueError or an IndexError: csc_matvec gets the user x item CSR '
                                      'and indexes its row pointer with item ids)' % self.method)
        if self.comm.world > 1:
            raise NotImplementedError('%s: multi-process scoring is not supported (comm.world = %d)'
                                      % (self.method, self.comm.world))

    def build(self):
        """The reference's build is empty; here the training CSR goes to the device with its CSC image A^T, the right-hand
        side of the product."""
        self._check_branch()
        ops = self.ops
        idx, val, shp = self.data.to_coo(tensor_mode=False, feedback_threshold=self.feedback_threshold)
        start = timer()
        val = np.ones(len(val)) if self.implicit else np.asarray(val, dtype=np.float64)
        A = ops.csr_from_coo(idx[:, 0], idx[:, 1], val, shp)
        self._At = A.T
        ops.synchronize()
        self._track(start)
        self.build_stats = {'n_users': int(shp[0]), 'n_items': int(shp[1]), 'nnz': int(A.nnz)}

    def _cold_similarity(self):
        sim = getattr(self.data, 'cold_items_similarity', None)
        if sim is None:
            raise ValueError('%s needs the similarity of the cold items to the training items: '
                             'data.cold_items_similarity is None' % self.method)
        return sim

    def get_recommendations(self):
        self._check_branch()
        sim = self._cold_similarity()
        if self.verify_integrity:
            self.verify_data_integrity()
        n_cold, n_users = self._cold_shape()
        i2i.check_topk(self.topk, n_users, self._topk_limit)
        self._recs_dev = None
        if n_cold == 0:
            return np.empty((0, self.topk), dtype=np.int64)
        if self._At is None:
            self.build()
        L = stored_csr(sim, (n_cold, self._At.shape[0]))
        ops = self.ops
        recs, _ = ops.spsp_topk(ops.csr(L.indptr, L.indices, L.data, L.shape), self._At, self.topk, False, sparse=True)
        return ops.to_host(recs)

    def slice_recommendations(self, cold_item_meta=None, start=0, stop=None):
        """The scores of cold items [start, stop) against every training user as a SciPy CSR with zeros removed."""
        from scipy.sparse import csr_matrix
        self._check_branch()
        n_cold = self._cold_shape()[0]
        stop = n_cold if stop is None else min(stop, n_cold)
        if self._At is None:
            self.build()
        L = stored_csr(self._cold_similarity(), (n_cold, self._At.shape[0]))
        ops = self.ops
        scores = csr_matrix(ops.to_host(ops.spsp_rows(ops.csr(L.indptr, L.indices, L.data, L.shape), self._At, (start, stop))))
        scores.eliminate_zeros()
        return scores

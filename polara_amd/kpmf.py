"""Kernelized probabilistic matrix factorisation (polara/recommender/hybrid/models.py:47-117, lib/optimize.py:253-301): PMF
whose regulariser couples a row with its neighbours in a kernel matrix — for a sample (m, n) the gradient of P[m] holds
kpm = sum_j Ku[m, j] P[j] in place of P[m], and the gradient of Q[n] the same with Ki and Q.

Everything else is polara_amd/pmf.py: the canonical interactions, the blocked schedule, the epoch loop and its stopping rule,
the adjusters.  What the neighbour reads do to the blocked sweep: two blocks of a stratum share no user and no item, but a
block's regulariser may read a row another block of the stratum is writing.  The semantics here (spelled out per sample in
include/polara_hip.h, pinned bit for bit by tests/kpmf_reference.py):

  * a neighbour row that lies in the block's OWN user (item) part is read live — only this block writes it during the
    stratum, and the block is swept serially;
  * every other neighbour row is read from a snapshot of P (Q) taken when the stratum began.

With blocks = 1 every row is an own-part row and the sweep is the reference's (up to the order of two sums: the tree of
`pm @ qn` as in PMF, and the diagonal term of the kernel row, which is added last).  With blocks > 1 it is a bounded-staleness
variant of it: only the regulariser's neighbour rows are stale, by at most one stratum.  If no kernel edge crosses a part, a
blocked epoch is exactly the reference's sweep on the schedule's permuted list.  Like for PMF, `blocks` is a parameter of the
model: another B is another — deterministic — trajectory.

Not implemented, and refused by name before any work: kernel_type='dif' (a matrix exponential of an n x n matrix, dense),
sparse_kernel_format=False, a `kernel_update` callable, the adjusters PMF refuses, warm start, multi-process builds.

    from polara_amd.kpmf import KernelizedPMF

The class lives in this module and is not among the names of the package's top level, whose list the suite pins."""
import numpy as np

from . import pmf
from .pmf import ProbabilisticMF, RMSPROP_GAMMA, SMOOTHING, sgd_epochs


def default_blocks(nnz, n_users, n_items):
    """The B of `blocks=None`: PMF's rule (pmf.default_blocks), for now.  It is NOT measured for KPMF: a sample here costs a
    gather of its neighbour rows on top of PMF's sample, and every stratum a refresh of the snapshots on top of its launch,
    so the best B is expected elsewhere (tools/bench_kpmf.py measures the epoch over B)."""
    return pmf.default_blocks(nnz, n_users, n_items)


def canonical_kernel(K, n=None):
    """K as a canonical SciPy CSR in fp64 (indices sorted, duplicates summed — the reference's `eye + gamma * R` arrives
    neither sorted nor free of duplicates); stored zeros stay.  A copy: the caller's matrix is not written."""
    import scipy.sparse as sps
    K = sps.csr_matrix(K, dtype=np.float64, copy=True)
    if K.shape[0] != K.shape[1] or (n is not None and K.shape[0] != int(n)):
        raise ValueError('KPMF: a kernel matrix of shape %s for %s entities' % (K.shape, 'its' if n is None else int(n)))
    K.sum_duplicates()
    K.sort_indices()
    return K


def split_kernel(K, n=None):
    """(ptr int64 [n + 1], idx int32, val fp64, diag fp64 [n]): the canonical kernel matrix without its diagonal, and the
    diagonal (0.0 where none is stored) — what the plan of the sweep holds for each side."""
    K = canonical_kernel(K, n)
    n = K.shape[0]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(K.indptr))
    on_diag = K.indices == rows
    diag = np.zeros(n, dtype=np.float64)
    diag[rows[on_diag]] = K.data[on_diag]
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[~on_diag], minlength=n), out=ptr[1:])
    return ptr, K.indices[~on_diag].astype(np.int32), K.data[~on_diag].astype(np.float64), diag


def _refuse_kernel_config(what, kernel_update, sparse_kernel_format):
    if kernel_update is not None:
        raise NotImplementedError('%s: the kernel update %r is not implemented (None: the sparse kernel update of the device sweep)'
                                  % (what, getattr(kernel_update, '__name__', kernel_update)))
    if not sparse_kernel_format:
        raise NotImplementedError('%s: sparse_kernel_format=%r is not implemented (dense kernel matrices)' % (what, sparse_kernel_format))


def kernelized_pmf_sgd(ops, matrix, rank, lrate, sigma, num_epochs, tol, kernel_matrices, kernel_update=None,
                       sparse_kernel_format=True, adjust_gradient=None, adjustment_params=None, seed=None, verbose=False,
                       iter_errors=None, iter_time=None, blocks=None, init=None, stats=None, comm=None):
    """kernelized_pmf_sgd (optimize.py:275-301) on the device: pmf.pmf_sgd with kernel_matrices = (user kernel [n_users x
    n_users], item kernel [n_items x n_items]) as SciPy sparse matrices.  Returns the DEVICE blocks (P, Q)."""
    _refuse_kernel_config('KPMF', kernel_update, sparse_kernel_format)
    Ku, Ki = kernel_matrices
    n_users, n_items = (int(x) for x in matrix.shape)
    if blocks is None:
        blocks = default_blocks(matrix.nnz, n_users, n_items)
    snapshots = []

    def run_epoch(plan, P, Q, eta, lambd, adjust, state):
        if not snapshots:
            snapshots.extend((ops.empty(*P.shape), ops.empty(*Q.shape)))
        return ops.kpmf_epoch(plan, P, Q, eta, lambd, adjust=adjust, state=state, gamma=RMSPROP_GAMMA, smoothing=SMOOTHING,
                              snapshots=tuple(snapshots))
    return sgd_epochs(ops, 'KPMF', matrix, rank, lrate, sigma, num_epochs, tol, lambda b: ops.kpmf_plan(matrix, b, Ku, Ki),
                      run_epoch, adjust_gradient=adjust_gradient, seed=seed, verbose=verbose, iter_errors=iter_errors,
                      iter_time=iter_time, blocks=blocks, init=init, stats=stats, comm=comm)


class KernelizedRecommenderMixin:
    """hybrid/models.py:47-104: the kernel matrices of both entities, built on first use from the data's relations and
    dropped on a data-change event.  As in the reference, the relations matrix itself (unit diagonal) stands where the
    paper has a graph Laplacian: K = I + gamma * R; an entity without relations gets factor_sigma[entity]**2 * I."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.kernel_type = 'reg'
        self.beta = 0.01
        self.gamma = 0.1
        self.sigma = 1
        self.kernel_update = None
        self.sparse_kernel_format = True
        entities = [self.data.fields.userid, self.data.fields.itemid]
        self.factor_sigma = dict.fromkeys(entities, 1)
        self._kernel_matrices = dict.fromkeys(entities)
        self.data.subscribe(self.data.on_change_event, self._clean_kernel_data)

    def _compute_kernel(self, laplacian, kernel_type=None):
        import scipy.sparse as sps
        kernel_type = kernel_type or self.kernel_type
        if kernel_type == 'dif':
            raise NotImplementedError("%s: kernel_type='dif' is not implemented (a dense matrix exponential; 'reg' is)" % self.method)
        if kernel_type == 'reg':
            n_entities = laplacian.shape[0]
            return sps.eye(n_entities).tocsr() + self.gamma * sps.csr_matrix(laplacian)
        raise ValueError('%s: unknown kernel_type %r' % (self.method, kernel_type))

    def _update_kernel_matrices(self, entity):
        import scipy.sparse as sps
        get = getattr(self.data, 'get_relations_matrix', None)
        if get is None:
            raise NotImplementedError('%s: the data object %s has no get_relations_matrix (SimilarityArrayData has)'
                                      % (self.method, type(self.data).__name__))
        laplacian = get(entity)
        if laplacian is None:
            sigma = self.factor_sigma[entity]
            n_entities = self.data.n_users if entity == self.data.fields.userid else self.data.n_items
            kernel_matrix = (sigma ** 2) * sps.eye(n_entities).tocsr()
        else:
            kernel_matrix = self._compute_kernel(laplacian)
        self._kernel_matrices[entity] = kernel_matrix

    def _clean_kernel_data(self):
        self._kernel_matrices = dict.fromkeys(self._kernel_matrices.keys())

    @property
    def item_kernel_matrix(self):
        return self.get_kernel_matrix(self.data.fields.itemid)

    @property
    def user_kernel_matrix(self):
        return self.get_kernel_matrix(self.data.fields.userid)

    def get_kernel_matrix(self, entity):
        if self._kernel_matrices.get(entity, None) is None:
            self._update_kernel_matrices(entity)
        return self._kernel_matrices[entity]


class KernelizedPMF(KernelizedRecommenderMixin, ProbabilisticMF):
    """hybrid/models.py:107-117 on the device sweep of csrc/kpmf.hip.  The data object carries the relations
    (SimilarityArrayData); `blocks` is the B of the blocked sweep (None: `default_blocks`), and with blocks = 1 the sweep is
    the reference's — see the module docstring for what another B means."""
    _device_optimizer = staticmethod(kernelized_pmf_sgd)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.optimizer = kernelized_pmf_sgd
        self.method = 'KPMF'

    def _refuse_before_any_work(self):
        if self.kernel_type != 'reg':
            self._compute_kernel(None)                      # 'dif' is not implemented, anything else is unknown
        _refuse_kernel_config(self.method, self.kernel_update, self.sparse_kernel_format)
        if getattr(self.data, 'warm_start', False):
            raise NotImplementedError('%s: warm start (data.warm_start = True) is not implemented' % self.method)
        if getattr(self.data, 'get_relations_matrix', None) is None:
            self._update_kernel_matrices(self.data.fields.userid)

    def _solve(self, ops, train, **config):
        kernel_matrices = (self.user_kernel_matrix, self.item_kernel_matrix)
        return kernelized_pmf_sgd(ops, train, self.rank, self.learn_rate, self.sigma, self.num_epochs, self.tolerance,
                                  kernel_matrices, kernel_update=self.kernel_update,
                                  sparse_kernel_format=self.sparse_kernel_format, **config)

    def build(self, *args, **kwargs):
        self._require_single_process_build()
        self._refuse_before_any_work()
        super().build(*args, **kwargs)

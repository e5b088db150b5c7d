"""SLIM (X. Ning, G. Karypis, "SLIM: Sparse Linear Methods for Top-N Recommender Systems", ICDM 2011): the sparse
item-to-item weights, for every target item j
    w_j = argmin 1/2 |x_j - X w|^2 + l1 |w|_1 + l2 / 2 |w|^2   subject to w_j[j] = 0 and, with `positive`, w >= 0,
by elastic-net coordinate descent over the dense Gram image G = X^T X on the device: the image is built with its diagonal
(pk_i2i_build_f64, pk_ease_diag_f64), the columns are solved in batches, one workgroup per column (pk_slim_solve_f64: the
arithmetic is fixed in include/polara_hip.h, so the weights are bit-equal to the NumPy restatement of
tests/slim_reference.py), every batch block is compacted to CSR rows of W^T (pk_slim_csr_count / pk_slim_csr_fill) and the
whole is transposed on the device; DESIGN.md 8m.  Scores are s_u = t_u W through the sparse x sparse scoring pass
(pk_spsp_topk), the one SimilarityAggregation runs on.

The first part of the module is the host-side planning (pure Python: shapes, the batch rule, the memory guard and the
parameter checks; tests/test_slim_host.py holds it against the library's own pk_slim_* planning functions), the second the
model."""
from functools import partial
from timeit import default_timer as timer

import numpy as np

from . import i2i, simagg

# ---- planning ------------------------------------------------------------------------------------------------------
MAX_ITEMS = 65536                # pk_slim_max_items: the stated limit of the solver
LDS_ITEMS = 19456                # pk_slim_lds_items: up to here the residual row of a column lives in LDS, beyond it in HBM
BATCH_COLUMNS = 1024             # pk_slim_batch_columns: the columns of a batch unless memory is short
MAX_TOPK = simagg.MAX_TOPK       # the scoring pass is the sparse x sparse one
DEFAULT_L1 = 1.0                 # choices, not measurements
DEFAULT_L2 = 10.0
DEFAULT_TOLERANCE = 1e-4
DEFAULT_MAX_SWEEPS = 100


def gram_leading_dim(n_items):
    """Row stride of the Gram image and of a batch block (pk_i2i_ld): n_items rounded up to a multiple of 8."""
    return i2i.leading_dim(n_items)


def gram_image_bytes(n_items):
    return int(n_items) * gram_leading_dim(n_items) * 8


def residual_in_lds(n_items):
    """Where the solver keeps the residual row of a column by default (pk_set_option('slim_r_global', 1) forces HBM)."""
    return int(n_items) <= LDS_ITEMS


def work_bytes(n_items, n_columns, r_global=None):
    """Scratch of one solve (pk_slim_work_bytes): the diagonal of G, n doubles rounded up to 256 bytes, and with the
    residual rows in HBM one row of n doubles per column of the batch."""
    n, nc = int(n_items), int(n_columns)
    diag = (max(n, 1) * 8 + 255) // 256 * 256
    if n < 1 or nc < 1:
        return diag
    if r_global is None:
        r_global = not residual_in_lds(n)
    return diag + (nc * n * 8 if r_global else 0)


def batch_bytes(n_items, n_columns):
    """The dense block of a batch, its residual rows in HBM (counted whatever the residence: the guard must hold under
    the option too) and the diagonal."""
    return int(n_columns) * gram_leading_dim(n_items) * 8 + work_bytes(n_items, n_columns, r_global=True)


def default_batch_columns(n_items, free_bytes=None):
    """Columns of a batch: min(n_items, 1024) (pk_slim_batch_columns), halved while the batch would take more than a
    sixteenth of the free device memory, so that the dense output never rivals the Gram image; at least 1."""
    n = int(n_items)
    nc = max(1, min(n, BATCH_COLUMNS))
    if free_bytes is not None:
        while nc > 1 and batch_bytes(n, nc) > free_bytes / 16:
            nc = (nc + 1) // 2
    return nc


def check_items(n_items):
    n = int(n_items)
    if n > MAX_ITEMS:
        raise ValueError('SLIM: %d items are more than the %d the solver takes (pk_slim_max_items)' % (n, MAX_ITEMS))
    return n


def check_column_batch(value, n_items=None):
    """None (the default rule) or an integer >= 1; capped at n_items when that is given."""
    if value is None:
        return None
    nc = int(value)
    if nc != value or nc < 1:
        raise ValueError('SLIM: column_batch must be None or an integer >= 1, got %r' % (value,))
    return nc if n_items is None else max(1, min(nc, int(n_items)))


def check_build_memory(n_items, free_bytes, column_batch=None):
    """The build's guard: the Gram image and one batch block (with its scratch) live side by side, so together they must
    fit in half of the free device memory.  Speaks before anything is allocated; returns the bytes needed.  More items
    than pk_slim_max_items() raise ValueError first."""
    n = check_items(n_items)
    nc = check_column_batch(column_batch, n)
    if nc is None:
        nc = default_batch_columns(n, free_bytes)
    need = gram_image_bytes(n) + batch_bytes(n, nc)
    if need > free_bytes / 2:
        raise MemoryError('SLIM: the dense fp64 Gram image (%d bytes) and one batch of %d columns (%d bytes) of %d items take '
                          '%d bytes (%.2f GB), more than half of the %d bytes (%.2f GB) of free device memory'
                          % (gram_image_bytes(n), nc, batch_bytes(n, nc), n, need, need / 1e9, int(free_bytes),
                             free_bytes / 1e9))
    return need


def check_parameters(l1, l2, tol, max_sweeps):
    """(l1, l2, tol, max_sweeps) as floats / int: l1, l2 >= 0 and finite, tol > 0 and finite, max_sweeps >= 1."""
    out = []
    for name, value in (('l1_regularization', l1), ('l2_regularization', l2)):
        v = float(value)
        if not np.isfinite(v) or v < 0:
            raise ValueError('SLIM: %s must be a finite number >= 0, got %r' % (name, value))
        out.append(v)
    t = float(tol)
    if not np.isfinite(t) or not t > 0:
        raise ValueError('SLIM: tolerance must be a finite number > 0, got %r' % (tol,))
    s = int(max_sweeps)
    if s != max_sweeps or s < 1 or s > 2 ** 31 - 1:
        raise ValueError('SLIM: max_sweeps must be an integer >= 1, got %r' % (max_sweeps,))
    return out[0], out[1], t, s


# ---- model -----------------------------------------------------------------------------------------------------------
from .models import _ItemWeightModel, _setting     # noqa: E402  (the planning part above needs neither)


def _parameter(name, index, doc):
    """A solver parameter of the model: checked on assignment, a changed value renews the model."""
    attr = '_' + name

    def fget(self):
        return getattr(self, attr)

    def fset(self, value):
        current = [self._l1_regularization, self._l2_regularization, self._tolerance, self._max_sweeps]
        current[index] = value
        new = check_parameters(*current)[index]
        if new != getattr(self, attr):
            setattr(self, attr, new)
            self._renew_model()
    return property(fget, fset, doc=doc)


class SLIMModel(_ItemWeightModel):
    """SLIM: `item_weights` is the canonical device CSR of W [n_items x n_items] (W[i, j]: the weight of source item i for
    target item j; sorted indices, no stored zeros, no diagonal), `sweeps` the host int32 vector of the sweeps every
    column ran.  `l1_regularization` (1.0), `l2_regularization` (10.0), `tolerance` (1e-4: a column stops when the largest
    change of a sweep is at most tolerance times its largest weight), `max_sweeps` (100) and `positive` (True: w >= 0)
    are the solver's; the defaults are choices, not measurements.  `implicit` replaces training and test feedback by
    their sign, as in EASEModel.  `column_batch` is the number of columns solved per launch (None: the default rule); the
    weights do not depend on it.  A change of any of these renews the model.  `dense_output` (default True): every item is
    a candidate and seen items come after all unseen ones under `filter_seen`; False: the sparse branch's candidates and
    -1 pads, exactly as SimilarityAggregation; a change re-scores and does not rebuild.  Ties go to the lower item
    index.  Single process; INTEGRATION.md has the semantics."""
    _topk_limit = MAX_TOPK
    _weight_slots = ('_W', 'sweeps')

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'SLIM'
        self._l1_regularization = DEFAULT_L1
        self._l2_regularization = DEFAULT_L2
        self._tolerance = DEFAULT_TOLERANCE
        self._max_sweeps = DEFAULT_MAX_SWEEPS
        self._positive = True
        self._column_batch = None
        self._dense_output = True

    l1_regularization = _parameter('l1_regularization', 0, 'l1 of the objective (>= 0): a change renews the model')
    l2_regularization = _parameter('l2_regularization', 1, 'l2 of the objective (>= 0): a change renews the model')
    tolerance = _parameter('tolerance', 2, 'a column stops when max |change| <= tolerance * max |weight| over a sweep: a '
                           'change renews the model')
    max_sweeps = _parameter('max_sweeps', 3, 'the cap on the sweeps of a column (>= 1): a change renews the model')
    positive = _setting('positive', '_renew_model', 'weights constrained to be >= 0: a new model')
    column_batch = _setting('column_batch', '_renew_model', 'columns solved per launch (None: default_batch_columns): a '
                            'change renews the model, the weights stay the same', check=check_column_batch)

    @property
    def item_weights(self):
        """The canonical device CSR of W [n_items x n_items] (None before the build)."""
        return self._W

    def _operand(self):
        return self._W

    def build(self):
        """Gram image with its diagonal -> the columns in batches (solve, compact to CSR rows of W^T) -> device transpose.
        The Gram image and the batch block are dropped as soon as W exists.  A column that reaches `max_sweeps` keeps the
        weights of its last sweep (`build_stats['capped_columns']` counts them)."""
        import torch
        from .ops import DeviceCSR
        self._single_process()
        ops = self.ops
        self._release_weights()
        A = self._training_device_csr()
        n_items = check_items(A.shape[1])
        stages = {'gram_s': 0.0, 'solve_s': 0.0, 'csr_s': 0.0}
        stage = partial(self._stage, stages)

        start = timer()
        free = ops.free_bytes()
        G = stage('gram', lambda: ops.slim_gram(A, self.column_batch))
        batch = check_column_batch(self.column_batch, n_items) or default_batch_columns(n_items, free)
        block = ops.empty(batch, gram_leading_dim(n_items))
        counts, indices, values, sweeps = [], [], [], []
        for j0 in range(0, n_items, batch):
            nc = min(batch, n_items - j0)
            Wt, sw = stage('solve', lambda: ops.slim_solve(G, n_items, j0, nc, self.l1_regularization, self.l2_regularization,
                                                           self.tolerance, self.max_sweeps, self.positive, out=block))
            ptr, idx, vals = stage('csr', lambda: ops.slim_csr(Wt, n_items))
            counts.append(ptr[1:] - ptr[:-1])
            indices.append(idx)
            values.append(vals)
            sweeps.append(sw)
        del G, block

        def transpose():
            indptr = torch.zeros(n_items + 1, dtype=torch.int64, device=ops.device)
            torch.cumsum(torch.cat(counts), 0, out=indptr[1:])
            Wt_csr = DeviceCSR.from_device(ops, indptr, torch.cat(indices), torch.cat(values), (n_items, n_items))
            return ops.csr_transpose(Wt_csr)                 # the rows of W^T are not kept
        W = stage('csr', transpose)
        self._track(start)
        self._W = W
        self.sweeps = ops.to_host(torch.cat(sweeps))
        nnz_w = int(W.nnz)
        self.build_stats = dict(stages, n_items=n_items, nnz=int(A.nnz), nnz_weights=nnz_w,
                                fill=nnz_w / float(n_items * n_items), max_sweeps=int(self.sweeps.max()),
                                mean_sweeps=float(self.sweeps.mean()),
                                capped_columns=int((self.sweeps >= self.max_sweeps).sum()), column_batch=int(batch))

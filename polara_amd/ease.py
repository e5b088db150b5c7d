"""EASE (H. Steck, "Embarrassingly shallow autoencoders for sparse data", WWW 2019): the item-to-item weights
    B = argmin |X - X B|^2 + lambda |B|^2   subject to diag(B) = 0
in closed form, B = I - P diag(1 / diag P) with P = (X^T X + lambda I)^-1, on the device: the Gram matrix is built into the
image of the library's dense Cholesky (pk_i2i_build_f64, pk_ease_diag_f64), factored (pk_chol_f64), the factor inverted in
place (pk_trtri_f64) and P = L^-T L^-1 formed tile by tile straight into the scaled scoring image (pk_ease_weights_f64);
DESIGN.md 8l.  Scores are s_u = t_u B through the item-to-item scoring pass (pk_i2i_topk, dense branch).

The first part of the module is the host-side planning (pure Python: the shapes the kernels work with and the memory guard
of the build; tests/test_ease_host.py holds it against the library's own pk_* planning functions), the second the model."""
from timeit import default_timer as timer

import numpy as np

from . import hybrid, i2i

# ---- planning ------------------------------------------------------------------------------------------------------
TILE = hybrid.TILE               # the block width of the factorisation, the inverse and the weights product
CHUNK = hybrid.CHUNK             # tiles of the inverted triangle one task of a panel product reads
MAX_TOPK = i2i.MAX_TOPK          # the scoring pass is the item-to-item one
DEFAULT_REGULARIZATION = 500.0   # the paper's value for ML-20M


def chol_leading_dim(n_items):
    """Rows and row stride of the Cholesky image (pk_hybrid_ld): n_items rounded up to whole 64 x 64 tiles."""
    return hybrid.leading_dim(n_items)


def weights_leading_dim(n_items):
    """Row stride of the scoring image of B (pk_i2i_ld): n_items rounded up to a multiple of 8."""
    return i2i.leading_dim(n_items)


def chol_image_bytes(n_items):
    return hybrid.image_bytes(n_items)


def weights_image_bytes(n_items):
    return int(n_items) * weights_leading_dim(n_items) * 8


def trtri_work_bytes(n_items):
    """Scratch of the triangular inverse (pk_trtri_work_bytes): the partial blocks of the longest panel product, one per
    chunk of a tile row (a single tile: nothing)."""
    if int(n_items) < 1:
        return 0
    below = chol_leading_dim(n_items) // TILE - 1
    chunks = -(-below // CHUNK)
    return chunks * below * TILE * TILE * 8


def check_build_memory(n_items, free_bytes):
    """The build's guard: the Cholesky image and the weights image are both dense and live side by side while the weights
    are formed, so together they must fit in half of the free device memory.  Returns the bytes needed."""
    need = chol_image_bytes(n_items) + weights_image_bytes(n_items)
    if need > free_bytes / 2:
        raise MemoryError('EASE: the dense fp64 Cholesky image (%d bytes) and the weights image (%d bytes) of %d items take '
                          '%d bytes (%.2f GB), more than half of the %d bytes (%.2f GB) of free device memory'
                          % (chol_image_bytes(n_items), weights_image_bytes(n_items), n_items, need, need / 1e9,
                             int(free_bytes), free_bytes / 1e9))
    return need


def check_regularization(value):
    """lambda >= 0 and finite (0 is allowed: it fails in the factorisation only when an item has no training entries)."""
    lam = float(value)
    if not np.isfinite(lam) or lam < 0:
        raise ValueError('EASE: regularization must be a finite number >= 0, got %r' % (value,))
    return lam


# ---- model -----------------------------------------------------------------------------------------------------------
from .models import _DenseItemModel, _SparseScoresMixin     # noqa: E402  (the planning part above needs neither)


class EASEModel(_SparseScoresMixin, _DenseItemModel):
    """EASE: `item_weights` is the device image of B [n_items x leading dim] (fp64; diagonal and pad columns 0),
    `precision_diagonal` the host vector d = diag (X^T X + lambda I)^-1.  `regularization` is lambda (a change renews the
    model); `implicit` replaces training and test feedback by their sign, as in CooccurrenceModel.  Every item is a
    candidate (the dense branch of the item-to-item scoring): under `filter_seen` seen items come after all unseen ones,
    ties go to the lower item index.  Single process; INTEGRATION.md has the semantics."""
    _topk_limit = MAX_TOPK

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'EASE'
        self._regularization = DEFAULT_REGULARIZATION
        self._implicit = False
        self._pad_const = -1
        self._weights = None
        self.precision_diagonal = None
        self.build_stats = {}

    @property
    def regularization(self):
        """lambda of the objective: a change renews the model"""
        return self._regularization

    @regularization.setter
    def regularization(self, value):
        lam = check_regularization(value)
        if lam != self._regularization:
            self._regularization = lam
            self._renew_model()

    @property
    def implicit(self):
        """feedback values replaced by their sign (training and test): a change renews the model"""
        return self._implicit

    @implicit.setter
    def implicit(self, value):
        if bool(value) != self._implicit:
            self._implicit = bool(value)
            self._renew_model()

    @property
    def dense_output(self):
        """Always True: EASE scores are dense (B has no zero off the diagonal)."""
        return True

    @dense_output.setter
    def dense_output(self, value):
        if not value:
            raise NotImplementedError('EASE scores are dense: the sparse branch of the item-to-item models is not offered '
                                      '(dense_output is fixed at True)')

    def _renew_model(self):
        super()._renew_model()
        self._weights = None               # the dense image is large: freed at once, not when the next build replaces it
        self.precision_diagonal = None

    @property
    def item_weights(self):
        """The device image of B [n_items x leading dim] (columns beyond n_items are 0)."""
        return self._weights

    def build(self):
        """Gram matrix with its diagonal -> Cholesky -> in-place inverse of the factor -> scaled weights; the Cholesky
        image is dropped as soon as B exists.  A pivot that is not positive (lambda = 0 and an item without training
        entries) raises numpy.linalg.LinAlgError naming the item's column."""
        self._single_process()
        ops = self.ops
        self._weights = self.precision_diagonal = None
        rows, cols, val, shp = self._training_triplets()
        n_items = int(shp[1])
        A = ops.csr_from_coo(rows, cols, val, shp)
        if self.implicit:
            import torch
            A = A.with_columns(A.indices, torch.sign(A.values))
        stages = {}

        def stage(name, fn):
            t0 = timer()
            res = fn()
            ops.synchronize()
            stages[name + '_s'] = timer() - t0
            return res

        start = timer()
        img = stage('gram', lambda: ops.ease_gram(A, self.regularization))
        try:
            stage('chol', lambda: ops.chol(img, n_items))
        except np.linalg.LinAlgError as exc:
            col = getattr(exc, 'column', -1)
            err = np.linalg.LinAlgError('EASE: X^T X + %g I is not positive definite: the pivot of item column %d is not '
                                        'positive (an item without training entries needs regularization > 0)'
                                        % (self.regularization, col))
            err.column = col
            raise err from None
        stage('trtri', lambda: ops.trtri(img, n_items))
        B, d = stage('weights', lambda: ops.ease_weights(img, n_items))
        del img
        self._track(start)
        self._weights = B
        self.precision_diagonal = ops.to_host(d)
        self.build_stats = dict(stages, n_items=n_items, nnz=int(A.nnz), image_bytes=int(B.numel() * B.element_size()),
                                chol_image_bytes=chol_image_bytes(n_items))

    def _test_values(self, T):
        if not self.implicit:
            return T
        import torch
        return T.with_columns(T.indices, torch.sign(T.values))

    def _score(self, T, n_items, want_scores=False):
        recs, scores = self.ops.i2i_topk(self._test_values(T), self._weights, n_items, self.topk, self.filter_seen,
                                         sparse=False, want_scores=want_scores)
        return (recs, scores) if want_scores else recs

    _implicit_values = staticmethod(np.sign)

    def _slice_scores(self, T, n_items):
        return self.ops.to_host(self.ops.spmm(T, self._weights))[:, :n_items]      # pk_spmm_csr_ex over B's image

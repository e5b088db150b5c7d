"""EASE (H. Steck, "Embarrassingly shallow autoencoders for sparse data", WWW 2019): the item-to-item weights
    B = argmin |X - X B|^2 + lambda |B|^2   subject to diag(B) = 0
in closed form, B = I - P diag(1 / diag P) with P = (X^T X + lambda I)^-1, on the device: the Gram matrix is built into the
image of the library's dense Cholesky (pk_i2i_build_f64, pk_ease_diag_f64), factored (pk_chol_f64), the factor inverted in
place (pk_trtri_f64) and P = L^-T L^-1 formed tile by tile straight into the scaled scoring image (pk_ease_weights_f64);
DESIGN.md 8l.  Scores are s_u = t_u B through the item-to-item scoring pass (pk_i2i_topk, dense branch).

The first part of the module is the host-side planning (pure Python: the shapes the kernels work with and the memory guard
of the build; tests/test_ease_host.py holds it against the library's own pk_* planning functions), the second the model."""
from functools import partial
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
from .models import _ItemWeightModel, _setting     # noqa: E402  (the planning part above needs neither)


def _dense_only(value):
    if not value:
        raise NotImplementedError('EASE scores are dense: the sparse branch of the item-to-item models is not offered '
                                  '(dense_output is fixed at True)')
    return True


class EASEModel(_ItemWeightModel):
    """EASE: `item_weights` is the device image of B [n_items x leading dim] (fp64; diagonal and pad columns 0),
    `precision_diagonal` the host vector d = diag (X^T X + lambda I)^-1.  `regularization` is lambda (a change renews the
    model); `implicit` replaces training and test feedback by their sign, as in CooccurrenceModel.  Every item is a
    candidate (the dense branch of the item-to-item scoring): under `filter_seen` seen items come after all unseen ones,
    ties go to the lower item index.  Single process; INTEGRATION.md has the semantics."""
    _topk_limit = MAX_TOPK
    _weight_slots = ('_weights', 'precision_diagonal')

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'EASE'
        self._regularization = DEFAULT_REGULARIZATION
        self._dense_output = True

    regularization = _setting('regularization', '_renew_model', 'lambda of the objective: a change renews the model',
                              check=check_regularization)
    dense_output = _setting('dense_output', '_refresh_model', 'Always True: EASE scores are dense (B has no zero off the '
                            'diagonal).', check=_dense_only)

    @property
    def item_weights(self):
        """The device image of B [n_items x leading dim] (columns beyond n_items are 0)."""
        return self._weights

    def _operand(self):
        return self._weights

    def build(self):
        """Gram matrix with its diagonal -> Cholesky -> in-place inverse of the factor -> scaled weights; the Cholesky
        image is dropped as soon as B exists.  A pivot that is not positive (lambda = 0 and an item without training
        entries) raises numpy.linalg.LinAlgError naming the item's column."""
        self._single_process()
        ops = self.ops
        self._release_weights()
        A = self._training_device_csr()
        n_items = A.shape[1]
        stages = {}
        stage = partial(self._stage, stages)
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

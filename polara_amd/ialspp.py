"""iALS++ — implicit ALS by block-subspace steps (Rendle, Krichene, Zhang, Koren: "iALS++: Speeding up matrix factorization
with subspace optimization", 2021), with the frequency-scaled regularisation of the same authors' "Revisiting the performance
of iALS on item recommendation benchmarks" (RecSys 2022).  The objective is `ImplicitALS`'s with a regularisation per row:
    sum over ALL (u, i) of w_ui (p_ui - x_u . y_i)^2 + sum_u lambda_u |x_u|^2 + sum_i lambda_i |y_i|^2,
    w = c, p = 1 on the stored entries;  w = 1, p = 0 elsewhere.
Where `ImplicitALS` solves every row's k x k normal equations exactly (rank <= 128: the system lives in LDS), a half-sweep
here walks over the rank in blocks of d = `block_size` coordinates and minimises the objective exactly over one block of
every row at a time (csrc/ialspp.hip), against cached predictions e_ui = x_u . y_i:  O(nnz k d + n k d^2) per half-sweep
instead of O(nnz k^2 + n k^3), ranks up to 2048.  A block step never increases the objective; with one block over the whole
rank a half-sweep IS the exact half-step, so that configuration is the same fit as `ImplicitALS`.

No ranking quality is claimed for any rank or regularisation: the solver and its arithmetic are what is tested.  Single
process."""
from timeit import default_timer as timer

import numpy as np

from .ials import ImplicitALS, initial_factors


def row_regularization(ops, C, regularization, exponent=0.0, unobserved=1.0):
    """lambda per row of the ops-level CSR `C` [n_rows x n_other]:  regularization * (n_row + unobserved * n_other) ** exponent
    with n_row the stored entries of the row — a float when the exponent is 0 (the scalar path), else a device fp64 vector.
    Computed on the host from the row pointers (n_rows integers): the powers are NumPy's, whatever the device."""
    if float(exponent) == 0.0:
        return float(regularization)
    indptr = np.asarray(ops.to_host(C.indptr), dtype=np.int64)[:int(C.shape[0]) + 1]
    counts = np.diff(indptr).astype(np.float64)
    return ops.to_device(float(regularization) * (counts + float(unobserved) * float(C.shape[1])) ** float(exponent))


def ialspp_fit(ops, C, rank, regularization, num_epochs, block_size, reg_exponent=0.0, reg_unobserved=1.0, seed=None, init=None,
               loss_history=None, iter_time=None, comm=None):
    """`num_epochs` times (user half-sweep, item half-sweep) on the ops-level CSR of confidences C [n_users x n_items], from
    `ials.initial_factors` (or init = (X0, Y0) host arrays).  Returns the DEVICE blocks (X, Y).  loss_history: a list that
    receives the objective after EVERY half-sweep (two entries per epoch)."""
    if comm is not None and getattr(comm, 'world', 1) > 1:
        raise NotImplementedError('iALS++: multi-process builds are not supported (comm.world = %d)' % comm.world)
    n_users, n_items = (int(x) for x in C.shape)
    rank, block_size = int(rank), int(block_size)
    if rank < 1 or rank > ops.ialspp_max_rank():
        raise ValueError('iALS++: rank %d outside 1..%d' % (rank, ops.ialspp_max_rank()))
    if block_size not in ops.ialspp_block_sizes():
        raise ValueError('iALS++: block size %r is not one of %s' % (block_size, tuple(ops.ialspp_block_sizes())))
    Ct = C.T                                                    # one transpose (pk_csr_transpose), kept on the matrix
    if init is None:
        init = initial_factors(n_users, n_items, rank, seed)
    X0, Y0 = (np.asarray(a, dtype=np.float64) for a in init)
    if X0.shape != (n_users, rank) or Y0.shape != (n_items, rank):
        raise ValueError('iALS++: initial factors of shapes %s, %s for (%d x %d), (%d x %d)'
                         % (X0.shape, Y0.shape, n_users, rank, n_items, rank))
    X, Y = ops.to_device(np.ascontiguousarray(X0)), ops.to_device(np.ascontiguousarray(Y0))
    lam_users = row_regularization(ops, C, regularization, reg_exponent, reg_unobserved)
    lam_items = row_regularization(ops, Ct, regularization, reg_exponent, reg_unobserved)
    EU = EI = None                                              # the cached predictions in the storage order of C and of Ct
    GY = ops.gram(Y)
    for _ in range(int(num_epochs)):
        start = timer()
        _, EU = ops.ialspp_half_sweep(C, Y, X, GY, lam_users, block_size, E=EU)
        GX = ops.gram(X)
        if loss_history is not None:
            loss_history.append(ops.ialspp_loss(C, X, Y, lam_users, lam_items, GX=GX, GY=GY))
        _, EI = ops.ialspp_half_sweep(Ct, X, Y, GX, lam_items, block_size, E=EI)
        GY = ops.gram(Y)
        if loss_history is not None:
            loss_history.append(ops.ialspp_loss(C, X, Y, lam_users, lam_items, GX=GX, GY=GY))
        if iter_time is not None:
            iter_time.append(timer() - start)
    return X, Y


class ImplicitALSPP(ImplicitALS):
    """`ImplicitALS` — its confidence pipeline, `fold_in_matrix`, serving, `compute_loss` / `loss_history` (one entry per
    half-sweep), `iterations_time`, `seed` — built by iALS++ half-sweeps, rank 1 .. 2048.

    block_size       d, one of `ops.ialspp_block_sizes()` = (16, 32, 64); the last block of a rank that d does not divide is narrower.
    reg_exponent     nu of Rendle et al. (2022): lambda_row = regularization * (n_row + reg_unobserved * n_other_side) ** nu, n_row
    reg_unobserved   the stored confidences of the row, n_other_side the items for a user row and the users for an item row;
                     reg_unobserved is the paper's alpha_0 (the weight of the unobserved pairs inside the count — the weight
                     of the unobserved pairs in the objective itself is 1 here).  nu = 0 (default): the plain lambda of `ImplicitALS`.
    fold_in_sweeps   warm start: that many user half-sweeps from x = 0 against the built item factors on `fold_in_matrix()`;
                     with one block over the whole rank the first is already the exact fold-in."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'iALS++'
        self.block_size = 64
        self.reg_exponent = 0.0
        self.reg_unobserved = 1.0
        self.fold_in_sweeps = 8

    def _check_shape(self):
        ops = self.ops
        rank = int(self.rank)
        if rank < 1 or rank > ops.ialspp_max_rank():
            raise ValueError('%s: rank %d outside 1..%d' % (self.method, rank, ops.ialspp_max_rank()))
        if self.block_size not in ops.ialspp_block_sizes():
            raise ValueError('%s: block size %r is not one of %s' % (self.method, self.block_size, tuple(ops.ialspp_block_sizes())))
        return rank

    def build(self):
        self._require_single_process_build()
        ops = self.ops
        rank = self._check_shape()
        C = self._confidence_csr(self._training_device_csr())      # scaling (ScaledMatrixMixin) first, confidence second
        self.loss_history = [] if self.compute_loss else None
        self.iterations_time = []
        start = timer()
        X, Y = ialspp_fit(ops, C, rank, self.regularization, self.num_epochs, self.block_size, reg_exponent=self.reg_exponent,
                          reg_unobserved=self.reg_unobserved, seed=self.seed, loss_history=self.loss_history,
                          iter_time=self.iterations_time)
        ops.synchronize()
        self._track(start)
        self._set_factors(X, Y)
        self._items_dev = (self.factors[self.data.fields.itemid], Y, None)

    def fold_in(self):
        """the warm-start users' factors [n_test_users x k] on the device (a view with an even leading dimension):
        `fold_in_sweeps` user half-sweeps from zero on `fold_in_matrix` against the built item factors"""
        ops = self.ops
        self._check_shape()
        Y, GY = self._item_factors_block()
        Cw = self.fold_in_matrix()
        k = int(Y.shape[1])
        block = ops.zeros(int(Cw.shape[0]), k + (k & 1))
        lam = row_regularization(ops, Cw, self.regularization, self.reg_exponent, self.reg_unobserved)
        E = None
        for _ in range(int(self.fold_in_sweeps)):
            _, E = ops.ialspp_half_sweep(Cw, Y, block[:, :k], GY, lam, self.block_size, E=E)
        return block[:, :k]

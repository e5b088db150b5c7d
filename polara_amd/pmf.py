"""Probabilistic matrix factorisation (polara/recommender/models.py:728-787, lib/optimize.py:123-250): P [n_users x k] and
Q [n_items x k] trained by stochastic gradient descent, one sweep over all interactions per epoch.

The reference's sweep is serial: sample k + 1 reads what sample k wrote.  Here the matrix is cut into B x B blocks — users
and items each into B contiguous ranges of about equal interaction count — and the B blocks of one diagonal "stratum"
s = (item part - user part) mod B are swept at once: they share no user row and no item row, so sweeping them side by side
is arithmetically the same as sweeping them one after the other.  A blocked epoch therefore IS the reference's sweep on a
permuted list of interactions (`block_schedule`), and B = 1 is the reference's own order.  Another B is another order of
the samples — another, equally valid, SGD trajectory; `blocks` is a parameter of the model like `seed`.

The sweep itself is csrc/pmf.hip (one launch per stratum, one double — the epoch's squared error — read back per epoch).
Single process.  KernelizedPMF — its transform reads other rows of P and Q, so the blocks of a stratum are no longer
independent — is polara_amd/kpmf.py, on this module's schedule and epoch loop.  Not here: the `adam` adjustment
(`beta ** t` per row is not correctly rounded on either side)."""
import math
from timeit import default_timer as timer

import numpy as np

from . import machine_model
from .csr import coo_to_csr
from .factor_serving import FactorQueriesMixin
from .models import RecommenderModel

ADJUSTERS = ('adagrad', 'rmsprop')      # optimize.py:73-86, with the reference's defaults below (its boilerplate passes the
RMSPROP_GAMMA = 0.9                     # state alone, optimize.py:186-189: the defaults are what it runs with)
SMOOTHING = 1e-6


def default_blocks(nnz, n_users, n_items):
    """The B of `blocks=None`.  An epoch is B launches, each as long as its longest block: about nnz / B**2 samples swept
    one after the other.  With t_s the time of one sample in such a chain and t_l what one more stratum adds, the epoch takes
    B * (t_l + t_s * nnz / B**2),  smallest at  B = sqrt(nnz * t_s / t_l);  B is then capped by the library's bound and by
    min(n_users, n_items).  t_s is measured (machine_model: 'pmf_sample_s'); t_l ('pmf_launch_s') is an effective constant:
    on the ML-20M-shaped matrix the epoch is flat between B = 1 024 and 2 048 (tools/bench_pmf.py), where the blocks' imbalance
    — the longest block stops shrinking like nnz / B**2 — takes over from their length, and the rule lands there (1 370).
    It has been checked on that one matrix only."""
    t_s, t_l = machine_model.value('pmf_sample_s'), machine_model.value('pmf_launch_s')
    b = int(round(math.sqrt(max(int(nnz), 1) * t_s / t_l)))
    return max(1, min(b, int(machine_model.value('pmf_max_blocks')), int(n_users), int(n_items)))


def canonical_interactions(users, items, values, shape):
    """(users int64, items int64, values fp64) in row-major (user, then item) order with duplicates summed: what the
    reference's `get_training_matrix(sparse_format='coo')` and `matrix.nonzero()` hand to its optimizer.  A summed value of
    exactly 0 raises: the reference's `nonzero()` would drop the entry from the indices and keep it in the data."""
    indptr, indices, vals = coo_to_csr(users, items, np.asarray(values, dtype=np.float64), shape)
    if (vals == 0).any():
        raise ValueError('PMF: an interaction with feedback 0 (after summing duplicates)')
    rows = np.repeat(np.arange(int(shape[0]), dtype=np.int64), np.diff(indptr))
    return rows, indices.astype(np.int64), np.asarray(vals, dtype=np.float64)


def _parts(counts, blocks, nnz):
    """part of every user (item): min(prefix_excl * B // nnz, B - 1) — integers only, monotone, so parts are contiguous"""
    counts = np.asarray(counts, dtype=np.int64)
    before = np.cumsum(counts) - counts
    return np.minimum(before * blocks // max(int(nnz), 1), blocks - 1)


def _block_schedule(users, items, n_users, n_items, blocks, order=None, what='PMF'):
    """The one host copy of the schedule, of interactions in canonical order: (perm int64 [nnz], block_ptr int64 [B * B + 1],
    item_part int64 [n_items], item_ptr int64 [B + 1]).  Position p of the schedule holds canonical entry perm[p]; block i of
    stratum s is positions block_ptr[s * B + i] .. block_ptr[s * B + i + 1].  `perm` is the stable sort by s * B + i, so a block
    keeps the canonical order (runs of one user stay together).  The items are cut into parts along `order` (None: the
    identity): part c is order[item_ptr[c] : item_ptr[c + 1]].  Empty parts and empty blocks are legal; B = 1 is the identity.
    `what` names the model in the message."""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    B, nnz = int(blocks), len(users)
    if B < 1 or B > min(int(n_users), int(n_items)):
        raise ValueError('%s: %d blocks for %d users and %d items (1 .. min of the two)' % (what, B, n_users, n_items))
    order = np.arange(int(n_items), dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
    upart = _parts(np.bincount(users, minlength=int(n_users)), B, nnz)
    ordered_parts = _parts(np.bincount(items, minlength=int(n_items))[order], B, nnz)
    ipart = np.empty(int(n_items), dtype=np.int64)
    ipart[order] = ordered_parts
    item_ptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.bincount(ordered_parts, minlength=B), out=item_ptr[1:])
    i, j = upart[users], ipart[items]
    key = ((j - i) % B) * B + i
    perm = np.argsort(key, kind='stable').astype(np.int64)
    block_ptr = np.zeros(B * B + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=B * B), out=block_ptr[1:])
    return perm, block_ptr, ipart, item_ptr


def block_schedule(users, items, n_users, n_items, blocks):
    """(perm, block_ptr) of `_block_schedule` with the items in their own order"""
    return _block_schedule(users, items, n_users, n_items, blocks)[:2]


def schedule_stats(block_ptr, blocks):
    lengths = np.diff(np.asarray(block_ptr, dtype=np.int64))
    B = int(blocks)
    return dict(blocks=B, strata=B, launches_per_epoch=B + 1, empty_blocks=int((lengths == 0).sum()),
                longest_block=int(lengths.max()) if len(lengths) else 0)


def adjuster_name(adjust_gradient, what='PMF'):
    """None, 'adagrad' or 'rmsprop' of what `build` was given: None, one of the names, or a callable called so (the
    reference's function objects; its `identity` is None).  Everything else is not implemented, and says what was asked."""
    if adjust_gradient is None:
        return None
    name = adjust_gradient if isinstance(adjust_gradient, str) else getattr(adjust_gradient, '__name__', None)
    if name in ADJUSTERS:
        return name
    if name == 'identity' and callable(adjust_gradient):
        return None
    raise NotImplementedError('%s: the gradient adjustment %r is not implemented (None, %s)'
                              % (what, name if name is not None else adjust_gradient, ', '.join(repr(a) for a in ADJUSTERS)))


def initial_factors(n_users, n_items, rank, seed=None):
    """(P0, Q0) drawn like optimize.py:172-174: P first, then Q, from `RandomState(seed)` or NumPy's global generator"""
    rnds = np.random if seed is None else np.random.RandomState(seed)
    P0 = rnds.normal(scale=0.1, size=(int(n_users), int(rank)))
    Q0 = rnds.normal(scale=0.1, size=(int(n_items), int(rank)))
    return P0, Q0


def sgd_epochs(ops, what, matrix, rank, lrate, sigma, num_epochs, tol, make_plan, run_epoch, adjust_gradient=None, seed=None,
               verbose=False, iter_errors=None, iter_time=None, blocks=None, init=None, stats=None, comm=None):
    """mf_sgd_boilerplate (optimize.py:158-220) on the device, shared by the sweeps that differ in their plan and their
    epoch alone (pmf_sgd here, kpmf.kernelized_pmf_sgd): the checks, the initial factors, the adjuster's state zeroed before
    every epoch, one host read per epoch, the stopping rule.  make_plan(blocks) -> plan; run_epoch(plan, P, Q, lrate, lambd,
    adjust, state) -> a device tensor of one double.  `what` names the model in the messages.  Returns the DEVICE blocks
    (P, Q)."""
    if comm is not None and getattr(comm, 'world', 1) > 1:
        raise NotImplementedError('%s: multi-process builds are not supported (comm.world = %d)' % (what, comm.world))
    adjust = adjuster_name(adjust_gradient, what)
    n_users, n_items = (int(x) for x in matrix.shape)
    rank = int(rank)
    if rank < 1 or rank > ops.pmf_max_rank():
        raise ValueError('%s: rank %d outside 1..%d' % (what, rank, ops.pmf_max_rank()))
    if blocks is None:
        blocks = default_blocks(matrix.nnz, n_users, n_items)
    start = timer()
    plan = make_plan(blocks)
    plan_time = timer() - start
    if init is None:
        init = initial_factors(n_users, n_items, rank, seed)
    P0, Q0 = (np.asarray(a, dtype=np.float64) for a in init)
    if P0.shape != (n_users, rank) or Q0.shape != (n_items, rank):
        raise ValueError('%s: initial factors of shapes %s, %s for (%d x %d), (%d x %d)'
                         % (what, P0.shape, Q0.shape, n_users, rank, n_items, rank))
    P, Q = ops.to_device(np.ascontiguousarray(P0)), ops.to_device(np.ascontiguousarray(Q0))
    state = (ops.empty(n_users, rank), ops.empty(n_items, rank)) if adjust else None
    lambd = 0.5 * sigma ** 2
    nnz = int(plan['nnz'])
    last_err = np.finfo('f8').max
    training_time = []
    epochs = 0
    for epoch in range(int(num_epochs)):
        start = timer()
        if state is not None:
            state[0].zero_()
            state[1].zero_()
        sse = run_epoch(plan, P, Q, lrate, lambd, adjust, state)
        new_err = float(sse[0].item())                      # the epoch's one host read
        training_time.append(timer() - start)
        epochs += 1
        refined = abs(last_err - new_err) / last_err
        last_err = new_err
        rmse = math.sqrt(new_err / nnz)
        if iter_errors is not None:
            iter_errors.append(rmse)
        if verbose:
            print('Epoch: {}. RMSE: {}'.format(epoch, rmse))
        if refined < tol:
            break
    if iter_time is not None:
        iter_time.extend(training_time)
    if stats is not None:
        stats.update(schedule_stats(ops.to_host(plan['block_ptr']), plan['blocks']), epochs=epochs, plan_time=plan_time)
    return P, Q


def pmf_sgd(ops, matrix, rank, lrate, sigma, num_epochs, tol, adjust_gradient=None, adjustment_params=None, seed=None,
            verbose=False, iter_errors=None, iter_time=None, blocks=None, init=None, stats=None, comm=None):
    """simple_pmf_sgd / mf_sgd_boilerplate (optimize.py:158-250) on the device.  matrix: the training matrix
    [n_users x n_items] as an ops-level CSR (canonical: its entries in storage order are the reference's interactions).
    Returns the DEVICE blocks (P, Q).  `adjustment_params` is accepted and unused, as in the reference, whose boilerplate
    replaces it by the zeroed state before every epoch.  init = (P0, Q0) host arrays instead of the seeded draw."""
    def run_epoch(plan, P, Q, eta, lambd, adjust, state):
        return ops.pmf_epoch(plan, P, Q, eta, lambd, adjust=adjust, state=state, gamma=RMSPROP_GAMMA, smoothing=SMOOTHING)
    return sgd_epochs(ops, 'PMF', matrix, rank, lrate, sigma, num_epochs, tol, lambda b: ops.pmf_plan(matrix, b), run_epoch,
                      adjust_gradient=adjust_gradient, seed=seed, verbose=verbose, iter_errors=iter_errors, iter_time=iter_time,
                      blocks=blocks, init=init, stats=stats, comm=comm)


class ProbabilisticMF(FactorQueriesMixin, RecommenderModel):
    """models.py:728-787.  `factors` holds host arrays — users [n_users x k], items [n_items x k] — and the device copy of
    the user factors stays for the passes.  `blocks` (None: `default_blocks`) is the B of the blocked sweep; with blocks = 1
    the samples are swept in the reference's order.  A rank change invalidates the model."""

    def __init__(self, *args, seed=None, **kwargs):
        self.seed = seed
        super().__init__(*args, **kwargs)
        self.method = 'PMF'
        self.optimizer = pmf_sgd
        self.learn_rate = 0.005
        self.sigma = 1
        self.num_epochs = 25
        self._rank = 10
        self.tolerance = 1e-4
        self.blocks = None
        self.factors = {}
        self.rmse_history = None
        self.show_rmse = False
        self.iterations_time = None
        self.build_stats = {}
        self._factors_dev = None            # (host user factors of `factors`, P on the device) of the last build
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)

    _device_optimizer = staticmethod(pmf_sgd)

    def _solve(self, ops, train, **config):
        """the optimizer's call: (P, Q) on the device"""
        return pmf_sgd(ops, train, self.rank, self.learn_rate, self.sigma, self.num_epochs, self.tolerance, **config)

    def build(self, adjust_gradient=None, adjustment_params=None):
        self._require_single_process_build()
        if self.optimizer is not self._device_optimizer:
            raise NotImplementedError('%s: the optimizer %r is not implemented (only the device sweep, polara_amd.%s.%s)'
                                      % (self.method, getattr(self.optimizer, '__name__', self.optimizer),
                                         self._device_optimizer.__module__.rsplit('.', 1)[-1], self._device_optimizer.__name__))
        adjuster_name(adjust_gradient, self.method)             # refused before any work
        ops = self.ops
        train = self._training_device_csr()
        self.rmse_history = []
        self.iterations_time = []
        stats = {}
        start = timer()
        P, Q = self._solve(ops, train, adjust_gradient=adjust_gradient, adjustment_params=adjustment_params, seed=self.seed,
                           verbose=self.show_rmse, iter_errors=self.rmse_history, iter_time=self.iterations_time,
                           blocks=self.blocks, stats=stats)
        ops.synchronize()
        self._track(start)
        self.build_stats = stats
        self._set_factors(P, Q)

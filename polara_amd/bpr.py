"""Bayesian personalised ranking — BPR-MF (polara/recommender/external/implicit/bprwrapper.py): LearnBPR of Rendle, Freudenthaler,
Gantner and Schmidt-Thieme, "BPR: Bayesian personalized ranking from implicit feedback" (2009), in the shape the third-party
`implicit` package trains it: rank k plus an item bias.  The reference hands the work to that package; here the solver is the
library's own (csrc/bpr.hip), on the blocked schedule of PMF (pmf.py).

Factors carry C = k + 1 columns: P [n_users x C] with column k the constant 1, Q [n_items x C] with column k the item bias, so
that P @ Q.T are the scores.  A sample (u, i, j) — a stored positive (u, i) and a negative j the user has not seen — moves the
user's row and BOTH item rows, so a block of the schedule must own both: the negative is drawn inside the positive's own item
part.  With fixed parts a positive would only ever be ranked against the same n_items / B neighbours; therefore the items are
cut into parts along a fresh seeded permutation every epoch (`item_order`, `reshuffle_items`), at the cost of one plan per
epoch.  B = 1 is plain LearnBPR with negatives from the whole catalogue.

Against `implicit`: fp64, not float32; every stored positive is visited once per epoch in schedule order (`implicit` draws nnz
positives with replacement); negatives are uniform inside the epoch's item part (`implicit` samples them by popularity); a
sample whose PK_BPR_DRAWS = 4 draws are all seen items is skipped and counted; runs are bit-reproducible.  No equality with any
build of `implicit` is claimed.  The sample's arithmetic, the draw stream and the sigmoid are spelled out in
include/polara_hip.h.  Single process; no fold-in (`implicit`'s BPR has none either)."""
from timeit import default_timer as timer

import numpy as np

from . import pmf
from .factor_serving import FactorQueriesMixin
from .models import RecommenderModel

MIN_PART_ITEMS = 64         # default_blocks: an item part averages at least this many items (a choice, not a measurement)


def default_blocks(nnz, n_users, n_items):
    """The B of `blocks=None`: PMF's rule (pmf.default_blocks), further capped at n_items // MIN_PART_ITEMS so that a part
    averages at least 64 items.  A user who has seen a share d of a part loses a sample there with probability d**4; the 64
    keeps the spread of a heavy user's seen share across random parts moderate.  The rule uses PMF's measured
    'pmf_sample_s' / 'pmf_launch_s' (machine_model): a BPR sample and stratum have not been measured on their own
    (tools/bench_bpr.py has not run yet)."""
    return max(1, min(pmf.default_blocks(nnz, n_users, n_items), int(n_items) // MIN_PART_ITEMS))


def item_order(seed, epoch, n_items):
    """pi_ep: the seeded permutation of the items along which epoch `epoch` cuts them into parts (int64 [n_items]) —
    `RandomState([seed, epoch]).permutation(n_items)`, seed and epoch as 32 unsigned bits"""
    return np.random.RandomState(np.array([int(seed), int(epoch)], dtype=np.uint32)).permutation(int(n_items)).astype(np.int64)


def block_schedule(users, items, n_users, n_items, blocks, order=None):
    """pmf.block_schedule with the items cut into parts along `order` (None: the identity): (perm, block_ptr, item_part int64
    [n_items], item_ptr int64 [B + 1]); part c of the items is order[item_ptr[c] : item_ptr[c + 1]]."""
    return pmf._block_schedule(users, items, n_users, n_items, blocks, order, what='BPR')


def initial_factors(n_users, n_items, rank, seed=None):
    """(P0 [n_users x (k + 1)], Q0 [n_items x (k + 1)]): (rand - 0.5) / k draws, P first, then Q, from `RandomState(seed)`
    or NumPy's global generator; column k of P0 is 1, the bias column of Q0 is 0."""
    rnds = np.random if seed is None else np.random.RandomState(seed)
    k = int(rank)
    P0, Q0 = np.ones((int(n_users), k + 1)), np.zeros((int(n_items), k + 1))
    P0[:, :k] = (rnds.rand(int(n_users), k) - 0.5) / k
    Q0[:, :k] = (rnds.rand(int(n_items), k) - 0.5) / k
    return P0, Q0


def pairwise_fit(model, ops, matrix, limits, begin, num_epochs, seed, blocks, default_blocks, reshuffle_items, share, history,
                 iter_time, comm):
    """What bpr_fit and warp.warp_fit share: the driver of a pairwise model on the blocked schedule.  Refused under the name
    `model`, in this order: several processes (before `matrix` is touched); every (what, value, most) of `limits` outside
    1..most; the blocks (None: `default_blocks(nnz, n_users, n_items)`); the seed (None: one draw from NumPy's global generator).
    Then `begin(blocks, seed)` makes the model's own checks and its device state and returns (state, plan_for, run_epoch):
    plan_for(order) is the schedule along a host item order (None: the identity), run_epoch(plan, epoch) draws, sweeps and
    returns the device tensor of the epoch's three counters.  An epoch is: the plan (once, or every epoch when
    `reshuffle_items`), run_epoch, ONE host read of the counters; `history` receives share(counts), `iter_time` the span of all
    that.  Returns (state, blocks, seed, the last plan or None, the time spent planning, the three counters as lists per epoch)."""
    if comm is not None and getattr(comm, 'world', 1) > 1:
        raise NotImplementedError('%s: multi-process builds are not supported (comm.world = %d)' % (model, comm.world))
    n_users, n_items = (int(x) for x in matrix.shape)
    for what, value, most in limits:
        if value < 1 or value > most:
            raise ValueError('%s: %s %d outside 1..%d' % (model, what, value, most))
    if blocks is None:
        blocks = default_blocks(matrix.nnz, n_users, n_items)
    blocks = int(blocks)
    if blocks < 1 or blocks > min(n_users, n_items):
        raise ValueError('%s: %d blocks for %d users and %d items (1 .. min of the two)' % (model, blocks, n_users, n_items))
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 32, dtype=np.uint64))
    seed = int(seed)
    if not 0 <= seed < 2 ** 32:
        raise ValueError('%s: the seed %d does not fit 32 unsigned bits' % (model, seed))
    state, plan_for, run_epoch = begin(blocks, seed)
    plan, plan_time, totals = None, 0.0, ([], [], [])
    for epoch in range(int(num_epochs)):
        start = timer()
        if plan is None or reshuffle_items:
            plan = plan_for(item_order(seed, epoch, n_items) if reshuffle_items else None)
            plan_time += timer() - start
        counts = [int(c) for c in ops.to_host(run_epoch(plan, epoch))]         # the epoch's one host read
        for total, count in zip(totals, counts):
            total.append(count)
        if history is not None:
            history.append(share(counts))
        if iter_time is not None:
            iter_time.append(timer() - start)
    return state, blocks, seed, plan, plan_time, totals


def bpr_fit(ops, matrix, rank, learning_rate, regularization, num_epochs, seed=None, blocks=None, reshuffle_items=True, init=None,
            auc_history=None, iter_time=None, stats=None, comm=None):
    """`num_epochs` LearnBPR sweeps over the stored entries of the ops-level canonical CSR `matrix` [n_users x n_items] (its
    values are ignored).  Returns the DEVICE blocks (P, Q) of k + 1 columns.  seed: 32 unsigned bits (None: one draw from NumPy's
    global generator, reported in `stats`); it seeds the initial factors, the item orders and the negatives.  auc_history
    receives correct / trained of every epoch; stats the schedule's figures and trained / skipped samples per epoch.
    init = (P0, Q0) host arrays of k + 1 columns instead of the seeded draw."""
    rank = int(rank)

    def begin(blocks, seed):
        n_users, n_items = (int(x) for x in matrix.shape)
        P0, Q0 = (np.asarray(a, dtype=np.float64) for a in (initial_factors(n_users, n_items, rank, seed) if init is None else init))
        if P0.shape != (n_users, rank + 1) or Q0.shape != (n_items, rank + 1):
            raise ValueError('BPR: initial factors of shapes %s, %s for (%d x %d), (%d x %d)'
                             % (P0.shape, Q0.shape, n_users, rank + 1, n_items, rank + 1))
        P, Q = ops.to_device(np.ascontiguousarray(P0)), ops.to_device(np.ascontiguousarray(Q0))
        return ((P, Q), lambda order: ops.bpr_plan(matrix, blocks, order),
                lambda plan, epoch: ops.bpr_epoch(plan, ops.bpr_draw_negatives(plan, seed, epoch), P, Q, learning_rate, regularization))

    (P, Q), blocks, seed, _, plan_time, (trained, skipped, _) = pairwise_fit(
        'BPR', ops, matrix, [('rank', rank, ops.bpr_max_rank())], begin, num_epochs, seed, blocks, default_blocks, reshuffle_items,
        lambda counts: counts[2] / counts[0] if counts[0] else float('nan'), auc_history, iter_time, comm)
    if stats is not None:
        stats.update(blocks=blocks, strata=blocks, launches_per_epoch=blocks + 2, reshuffle_items=bool(reshuffle_items), seed=seed,
                     epochs=len(trained), plan_time=plan_time, trained=trained, skipped=skipped)
    return P, Q


class ImplicitBPR(FactorQueriesMixin, RecommenderModel):
    """bprwrapper.py:7-76.  `factors` holds host fp64 arrays of k + 1 columns — users [P | 1], items [Q | bias] —, so that
    their product is the scores; `auc_history` the share of correctly ranked training pairs per epoch (`implicit`'s progress
    figure), `build_stats` the schedule and the trained / skipped samples per epoch.  `random_state` (or `seed=`) seeds the
    build; `num_threads` and `show_progress` are accepted and ignored.  `blocks` (None: `default_blocks`) is the B of the
    blocked sweep, `reshuffle_items` whether every epoch cuts the items along a fresh permutation.  There is no fold-in: warm
    start raises.  A rank change invalidates the model."""

    def __init__(self, *args, seed=None, **kwargs):
        self.random_state = seed
        super().__init__(*args, **kwargs)
        self._rank = 10
        self.learning_rate = 0.01
        self.regularization = 0.01
        self.num_epochs = 100
        self.num_threads = 0
        self.show_progress = False
        self.method = 'BPRMF'
        self.blocks = None
        self.reshuffle_items = True
        self.factors = {}
        self.auc_history = None
        self.iterations_time = None
        self.build_stats = {}
        self._factors_dev = None            # (host user factors of `factors`, [P | 1] on the device) of the last build
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)

    @property
    def seed(self):
        return self.random_state

    @seed.setter
    def seed(self, value):
        self.random_state = value

    def _check_serving(self):
        if self.data.warm_start:
            raise NotImplementedError('%s has no fold-in: BPR cannot serve warm-start users (the reference\'s wrapper asks the '
                                      '`implicit` package for `recalculate_user`, which it does not implement for this model)'
                                      % self.method)

    def build(self):
        self._require_single_process_build()
        ops = self.ops
        train = self._training_device_csr()
        self.auc_history = []
        self.iterations_time = []
        stats = {}
        start = timer()
        P, Q = bpr_fit(ops, train, self.rank, self.learning_rate, self.regularization, self.num_epochs, seed=self.random_state,
                       blocks=self.blocks, reshuffle_items=self.reshuffle_items, auc_history=self.auc_history,
                       iter_time=self.iterations_time, stats=stats)
        ops.synchronize()
        self._track(start)
        self.build_stats = stats
        self._set_factors(P, Q)

"""RecommenderArrayData: the step before `build()` — `RecommenderData.prepare()` of the reference (data.py:232-252,
`_split_data` :388-458) on arrays, on the device.

Raw interactions (external user and item ids in any order, a feedback column, optionally a custom ordering column) are cut
into a training part, a testset and a holdout and renumbered; the result is an `ArrayData`, so every model accepts it
unchanged.  The rules, with p = a row's position in the constructor's arrays:

  fold      user code = rank of the external id among the sorted distinct ids; a row is in the test fold when
            round((fold - 1) * num) <= code < round(fold * num), num = n_users * test_ratio (data.py:509-514)
  holdout   per user, among the candidate rows, the holdout_size smallest by a two-word key (hi, lo):
              top (default)        hi = order value descending, lo = p descending   (nlargest(keep='last'), data.py:746)
              negative_prediction  hi = order value ascending,  lo = p descending   (nsmallest(keep='last'))
              permute_tops         hi as above,                  lo = mix64(mix64(seed) + p)
              random_holdout / no feedback   hi = 0,             lo = mix64(mix64(seed) + p)
  parts     state 4 (warm_start): training = rows outside the fold, testset = fold rows outside the holdout;
            states 2 and 3: training = every row outside the holdout, testset recovered on demand
  sampling  state 4, test_sample t, BEFORE any filter (data.py:757-774): t < 0: per user the -t smallest by (feedback
            ascending, p ascending); t > 0: t rows by lo = mix64(mix64(seed + 1) + p)
  indices   training users numbered by first appearance in the training rows, items by sorted id; unseen items (and, in
            states 2 and 3, users) leave testset and holdout; holdout users with a count other than holdout_size leave; in
            state 4 only users in both testset and holdout stay and are numbered by first appearance in the testset

The two random modes draw from the counter-based stream above (`pk_mix64` of csrc/pk_common.h), NOT from NumPy's Mersenne
Twister, which the reference consumes serially group by group: same statistics, no list parity with the reference.  With
seed=None one seed is taken from `np.random` per prepare and kept as `data.seed_used`.

`ops`: a `HipOps` (default: one is created) — the columns are uploaded once, everything per row stays on the device and
only scalar counts cross until the final arrays are downloaded; the per-user selection is `pk_segment_select`
(csrc/split.hip).  `PrepareNumpyOps()` runs the same pipeline in NumPy where there is no GPU.

Not supported (NotImplementedError naming the option): a fractional holdout_size, test_ratio > 0 without a holdout and
with known users (the reference's state 11), ensure_consistency=False, build_index=False.  `get_entity_index` is
deliberately absent: models.py takes its presence to mean a pandas data object.
"""
from collections import namedtuple

import numpy as np

from . import defaults
from ._lib import PK_SPLIT_ASCENDING, PK_SPLIT_RANDOM_LO, PK_SPLIT_NO_ORDER, PK_SPLIT_POS_ASCENDING
from .data import ArrayData, TestData

DataIndex = namedtuple('DataIndex', 'userid itemid feedback')
UserIndex = namedtuple('UserIndex', 'training test')
EntityIndex = namedtuple('EntityIndex', 'old new')

_NONE = np.iinfo(np.int64).max          # "no row" in the first-appearance tables

# the configuration of defaults.py:5-14 of the reference, plus the seed
_CONFIG = ('shuffle_data', 'test_ratio', 'test_fold', 'warm_start', 'holdout_size', 'test_sample', 'permute_tops',
           'random_holdout', 'negative_prediction')
_LOCAL_DEFAULTS = dict(shuffle_data=False, permute_tops=False, random_holdout=False, negative_prediction=False)
# in state 4 a change of these alone leaves the training part as it is (the `test_update` rule, data.py:351-373)
_TEST_ONLY = frozenset(('holdout_size', 'random_holdout', 'permute_tops', 'negative_prediction', 'test_sample'))


def mix64(z):
    """pk_mix64 (csrc/pk_common.h) on a uint64 array: the splitmix64 output function, a bijection of 64-bit words."""
    z = np.asarray(z, dtype=np.uint64).reshape(-1).copy()
    z += np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


class PrepareNumpyOps:
    """The operator set of the split in NumPy: the same contracts as the device operators, bit for bit (integer work
    throughout).  Keys are int64 arrays holding u64 bit patterns, as on the device."""
    name = 'numpy'

    def upload(self, a, dtype):
        return np.ascontiguousarray(a, dtype=dtype)

    def download(self, a):
        return np.asarray(a)

    def sync(self):
        pass

    def arange(self, n):
        return np.arange(n, dtype=np.int64)

    def full(self, n, value):
        return np.full(n, value, dtype=np.int64)

    def ones_bool(self, n):
        return np.ones(n, dtype=bool)

    def unique_inverse(self, a):
        u, inv = np.unique(a, return_inverse=True)
        return u, inv.reshape(-1).astype(np.int64, copy=False)

    def n_unique(self, a):
        return int(len(np.unique(a)))

    def group_rows(self, codes, n_groups):
        perm = np.argsort(codes, kind='stable').astype(np.int64, copy=False)
        return perm, self.cumsum0(np.bincount(codes, minlength=n_groups))

    def bincount(self, codes, n):
        return np.bincount(codes, minlength=n).astype(np.int64, copy=False)

    def cumsum0(self, counts):
        out = np.zeros(len(counts) + 1, dtype=np.int64)
        np.cumsum(counts, out=out[1:])
        return out

    def first_pos(self, codes, vals, n):
        """out[c] = vals of the first row with code c (vals ascend inside a code, so this is its minimum); _NONE where no row
        has the code."""
        out = np.full(n, _NONE, dtype=np.int64)
        u, at = np.unique(codes, return_index=True)
        out[u] = vals[at]
        return out

    def argsort(self, a):
        return np.argsort(a, kind='stable')

    def nonzero(self, mask):
        return np.flatnonzero(mask)

    def split_keys(self, order_vals, pos, mode, seed):
        pos = np.asarray(pos, dtype=np.int64).view(np.uint64)
        if mode & PK_SPLIT_NO_ORDER:
            hi = np.zeros(len(pos), dtype=np.uint64)
        else:
            b = np.ascontiguousarray(order_vals, dtype=np.float64).view(np.uint64).copy()
            b[(b << np.uint64(1)) == 0] = 0                                      # -0.0 orders as +0.0
            asc = np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))
            hi = asc if mode & PK_SPLIT_ASCENDING else ~asc
        if mode & PK_SPLIT_RANDOM_LO:
            lo = mix64(mix64(np.array([int(seed) & (2 ** 64 - 1)], dtype=np.uint64)) + pos)
        else:
            lo = pos.copy() if mode & PK_SPLIT_POS_ASCENDING else ~pos
        return hi.view(np.int64), lo.view(np.int64)

    def segment_select(self, seg_ptr, key_hi, key_lo, k):
        n = len(key_hi)
        flags = np.zeros(n, dtype=bool)
        if n == 0 or len(seg_ptr) < 2:
            return flags
        seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
        b, e = int(seg_ptr[0]), int(seg_ptr[-1])
        seg = np.repeat(np.arange(len(seg_ptr) - 1, dtype=np.int64), np.diff(seg_ptr))
        order = b + np.lexsort((key_lo[b:e].view(np.uint64), key_hi[b:e].view(np.uint64), seg))
        rank = np.arange(e - b, dtype=np.int64) - (seg_ptr[seg] - b)            # sorted by segment first: seg is unchanged
        flags[order[rank < k]] = True
        return flags


class _HipPrepareOps:
    """The same operator set on the device: `HipOps.group_rows / split_keys / segment_select` (the package's kernels) and
    torch for the elementwise plumbing, gathers and compaction."""
    name = 'hip'

    def __init__(self, hip):
        import torch
        self.hip, self.torch, self.device = hip, torch, hip.device

    def upload(self, a, dtype):
        return self.hip.to_device(np.ascontiguousarray(a, dtype=dtype))

    def download(self, t):
        return t.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize(self.device)

    def arange(self, n):
        return self.torch.arange(n, dtype=self.torch.int64, device=self.device)

    def full(self, n, value):
        return self.torch.full((n,), value, dtype=self.torch.int64, device=self.device)

    def ones_bool(self, n):
        return self.torch.ones(n, dtype=self.torch.bool, device=self.device)

    def unique_inverse(self, a):
        u, inv = self.torch.unique(a, sorted=True, return_inverse=True)
        return u, inv.reshape(-1)

    def n_unique(self, a):
        return int(self.torch.unique(a).numel())

    def group_rows(self, codes, n_groups):
        return self.hip.group_rows(codes, n_groups)

    def bincount(self, codes, n):
        return self.torch.bincount(codes, minlength=n)

    def cumsum0(self, counts):
        out = self.torch.zeros(len(counts) + 1, dtype=self.torch.int64, device=self.device)
        out[1:] = self.torch.cumsum(counts, 0)
        return out

    def first_pos(self, codes, vals, n):
        out = self.full(n, _NONE)
        return out.scatter_reduce_(0, codes, vals, 'amin', include_self=True)

    def argsort(self, a):
        return self.torch.sort(a, stable=True)[1]

    def nonzero(self, mask):
        return self.torch.nonzero(mask).reshape(-1)

    def split_keys(self, order_vals, pos, mode, seed):
        return self.hip.split_keys(order_vals, pos, mode, seed)

    def segment_select(self, seg_ptr, key_hi, key_lo, k):
        return self.hip.segment_select(seg_ptr, key_hi, key_lo, k).bool()


def _config_property(name):
    def getter(self):
        return getattr(self, '_' + name)

    def setter(self, value):
        if getattr(self, '_' + name) != value:
            setattr(self, '_' + name, value)
            self._change_properties.add(name)
    return property(getter, setter)


class RecommenderArrayData(ArrayData):
    __doc__ = __doc__
    profile = False                     # True: synchronise after every stage and add its seconds to `timings`

    def __init__(self, users, items, feedback=None, custom_order=None, config=None, seed=None, ops=None):
        self._change_properties = set()
        for name, value in self.default_configuration().items():
            setattr(self, '_' + name, value)
        self._seed = None
        empty = np.zeros(0, dtype=np.int64)
        ArrayData.__init__(self, (empty, empty, np.zeros(0)), n_users=0, n_items=0)
        for name, value in self.default_configuration().items():       # (the base constructor wrote three of them)
            setattr(self, '_' + name, value)
        self._seed = seed
        self.seed_used = None
        self.index = DataIndex(None, None, None)
        self._state = None
        self._cache = None
        self.timings = {}
        if ops is None:
            from .ops import HipOps
            ops = HipOps()
        self.ops = ops
        self._B = ops if isinstance(ops, PrepareNumpyOps) else _HipPrepareOps(ops)
        self._ingest(users, items, feedback, custom_order)
        if config is not None:
            self.set_configuration(config)
        self._change_properties = {'init'}

    # ---- configuration --------------------------------------------------------------------------------------------
    @classmethod
    def default_configuration(cls):
        return {name: _LOCAL_DEFAULTS[name] if name in _LOCAL_DEFAULTS else getattr(defaults, name) for name in _CONFIG}

    def get_configuration(self):
        return {name: getattr(self, name) for name in _CONFIG}

    def set_configuration(self, params):
        for name, value in params.items():
            if name in _CONFIG or name == 'seed':
                setattr(self, name, value)
            else:
                print('Property %s is undefined.' % name)

    @property
    def ensure_consistency(self):
        return True

    @ensure_consistency.setter
    def ensure_consistency(self, value):
        if not value:
            raise NotImplementedError('ensure_consistency=False is not supported')

    @property
    def build_index(self):
        return True

    @build_index.setter
    def build_index(self, value):
        if not value:
            raise NotImplementedError('build_index=False is not supported')

    def _validate_config(self):
        """data.py:261-272."""
        if self._warm_start and not (self._holdout_size and self._test_ratio):
            raise ValueError('Both holdout_size and test_ratio must be positive when warm_start is set to True')
        if not self._warm_start and (self._holdout_size == 0) and (self._test_ratio > 0):
            raise ValueError('test_ratio cannot be nonzero when holdout_size is 0 and warm_start is set to False')
        assert self._test_ratio < 1, 'Value of test_ratio can\'t be greater than or equal to 1'
        if self._test_ratio:
            max_fold = 1.0 / self._test_ratio
            if self._test_fold > max_fold:
                raise ValueError('Test fold value cannot be greater than {}'.format(max_fold))

    def _target_state(self):
        """1: no holdout, no testset; 2: holdout of every user; 3: holdout of the fold's users, who stay in the training;
        4: the fold's users leave the training (data.py:145)."""
        h = self._holdout_size
        if h < 0 or h != int(h):
            raise NotImplementedError('holdout_size=%r: a fractional holdout_size is not supported' % (h,))
        if h == 0:
            if self._test_ratio > 0:
                raise NotImplementedError('test_ratio > 0 with holdout_size=0 and warm_start=False (a testset of known users '
                                          'without a holdout) is not supported')
            return 1
        if self._test_ratio == 0:
            return 2
        return 4 if self._warm_start else 3

    # ---- lazily updated views: everything ArrayData reads goes through them ------------------------------------
    def update(self, training_only=False):
        if self._change_properties:
            if training_only:
                self.prepare_training_only()
            else:
                self.prepare()

    def _lazy(name):
        def getter(self):
            self.update()
            return self.__dict__['_lazy_' + name]

        def setter(self, value):
            self.__dict__['_lazy_' + name] = value
        return property(getter, setter)

    _train = _lazy('train')
    _test = _lazy('test')
    n_users = _lazy('n_users')
    n_items = _lazy('n_items')
    index = _lazy('index')
    del _lazy

    def _set_holdout_size(self):
        pass                            # the configuration owns holdout_size (data.py: `holdout_size`)

    def set_training_data(self, training):
        raise NotImplementedError('the training part follows from the raw data and the configuration: build a new object')

    def external_items(self, ids):
        """external ids of internal item ids"""
        self.update()
        return self.index.itemid.old[np.asarray(ids, dtype=np.int64)]

    def external_users(self, ids, index_id='training'):
        """external ids of internal user ids of the training (or, in state 4, 'test') numbering"""
        self.update()
        index = getattr(self.index.userid, index_id)
        if index is None:
            raise ValueError('there is no %s user index in this state' % index_id)
        return index.old[np.asarray(ids, dtype=np.int64)]

    # ---- the split --------------------------------------------------------------------------------------------------
    def _tick(self, stage, t0):
        import time
        if self.profile:
            self._B.sync()
            now = time.perf_counter()
            self.timings[stage] = self.timings.get(stage, 0.0) + now - t0
            return now
        return t0

    def _ingest(self, users, items, feedback, custom_order):
        import time
        B = self._B
        users, items = np.asarray(users), np.asarray(items)
        if users.ndim != 1 or users.shape != items.shape:
            raise ValueError('users and items must be one-dimensional arrays of one length')
        if not (np.issubdtype(users.dtype, np.integer) and np.issubdtype(items.dtype, np.integer)):
            raise ValueError('users and items must hold integer ids')
        n = len(users)
        cols = {}
        for name, col in (('feedback', feedback), ('custom_order', custom_order)):
            if col is None:
                cols[name] = None
                continue
            col = np.asarray(col)
            if col.shape != users.shape:
                raise ValueError('%s must have one value per row' % name)
            if name == 'custom_order' and np.issubdtype(col.dtype, np.integer):
                if n and np.abs(col).max() > 2 ** 53:
                    raise ValueError('custom_order: integers beyond 2^53 do not order exactly as fp64')
            col = col.astype(np.float64, copy=False)
            if not np.isfinite(col).all():
                raise ValueError('%s must be finite' % name)
            cols[name] = col
        t0 = time.perf_counter()
        self.timings = {}
        d = dict(n=n)
        u_dev, i_dev = B.upload(users, np.int64), B.upload(items, np.int64)
        d['fb'] = None if cols['feedback'] is None else B.upload(cols['feedback'], np.float64)
        d['order'] = d['fb'] if cols['custom_order'] is None else B.upload(cols['custom_order'], np.float64)
        t0 = self._tick('upload', t0)
        d['users'], d['ucode'] = B.unique_inverse(u_dev)
        d['items'], d['icode'] = B.unique_inverse(i_dev)
        d['n_u'], d['n_i'] = len(d['users']), len(d['items'])
        if n and B.n_unique(d['ucode'] * d['n_i'] + d['icode']) != n:
            raise NotImplementedError('Data has duplicate values')
        d['perm'], d['seg_ptr'] = B.group_rows(d['ucode'], d['n_u'])
        self._tick('user grouping', t0)
        self._raw = d

    def _select(self, rows, seg_ptr, order_vals, mode, seed, k):
        B = self._B
        key_hi, key_lo = B.split_keys(order_vals, rows, mode, seed)
        return B.segment_select(seg_ptr, key_hi, key_lo, k)

    def prepare_training_only(self):
        self.holdout_size = 0
        self.test_ratio = 0
        self.warm_start = False
        self.prepare()

    def prepare(self):
        import time
        self._validate_config()
        state = self._target_state()
        changed = self._change_properties
        if not changed:
            return
        full = not (self._state == 4 and state == 4 and changed <= _TEST_ONLY and self._cache is not None)
        B, d = self._B, self._raw
        seed = self._seed
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 63 - 1))
        self.seed_used = seed = int(seed)
        k = int(self._holdout_size)
        warm = state == 4
        n_u, n_i = d['n_u'], d['n_i']
        ucode, icode = d['ucode'], d['icode']
        t0 = time.perf_counter()

        # -- fold and holdout: the candidate rows lie grouped by user in `perm`; a fold is a range of user codes ----------
        if self._test_ratio > 0:
            num = n_u * self._test_ratio
            lo = min(max(int(round((self._test_fold - 1) * num)), 0), n_u)
            hi = min(max(int(round(self._test_fold * num)), lo), n_u)
        else:
            lo, hi = 0, n_u
        H = T = first_key = None
        if state != 1:
            base, end = (int(x) for x in B.download(d['seg_ptr'][[lo, hi]]))
            cand = d['perm'][base:end]
            seg_ptr = d['seg_ptr'][lo:hi + 1] - base
            if self._random_holdout or d['order'] is None:
                flag = self._select(cand, seg_ptr, None, PK_SPLIT_NO_ORDER | PK_SPLIT_RANDOM_LO, seed, k)
            else:
                mode = (PK_SPLIT_ASCENDING if self._negative_prediction else 0) | (PK_SPLIT_RANDOM_LO if self._permute_tops else 0)
                flag = self._select(cand, seg_ptr, d['order'][cand], mode, seed, k)
            H = cand[flag]
            if warm:
                T = cand[~flag]
                t = self._test_sample
                if t:
                    if t != int(t):
                        raise NotImplementedError('test_sample=%r: a fractional test_sample is not supported' % (t,))
                    if t < 0 and d['fb'] is None:
                        raise ValueError('a negative test_sample needs feedback')
                    fold_user = ucode[T] - lo
                    first_key = B.first_pos(fold_user, T, hi - lo)        # a user's first row BEFORE sampling
                    seg_ptr = B.cumsum0(B.bincount(fold_user, hi - lo))
                    if t < 0:
                        flag = self._select(T, seg_ptr, d['fb'][T], PK_SPLIT_ASCENDING | PK_SPLIT_POS_ASCENDING, 0, -int(t))
                    else:
                        flag = self._select(T, seg_ptr, None, PK_SPLIT_NO_ORDER | PK_SPLIT_RANDOM_LO, seed + 1, int(t))
                    T = T[flag]
        t0 = self._tick('keys and selection', t0)

        # -- the training part and its indices ------------------------------------------------------------------------
        if full:
            if warm:
                train_rows = B.nonzero((ucode < lo) | (ucode >= hi))
            elif state == 1:
                train_rows = B.arange(d['n'])
            else:
                mask = B.ones_bool(d['n'])
                mask[H] = False
                train_rows = B.nonzero(mask)
            t0 = self._tick('partition', t0)
            tu, ti = ucode[train_rows], icode[train_rows]
            first = B.first_pos(tu, train_rows, n_u)                      # users in order of first appearance
            by_first = B.argsort(first)
            n_train_users = int((first != _NONE).sum())
            train_users = by_first[:n_train_users]
            umap = B.full(n_u, -1)
            umap[train_users] = B.arange(n_train_users)
            present = B.bincount(ti, n_i) > 0                             # items in sorted order of their ids
            train_items = B.nonzero(present)
            imap = B.full(n_i, -1)
            imap[train_items] = B.arange(len(train_items))
            fb = None if d['fb'] is None else d['fb'][train_rows]
            c = dict(umap=umap, imap=imap, n_train_users=n_train_users, n_train_items=len(train_items),
                     training=(umap[tu], imap[ti], fb), train_users=d['users'][train_users], train_items=d['items'][train_items],
                     n_train=len(train_rows))
        else:
            c = self._cache
        umap, imap = c['umap'], c['imap']

        # -- filters, the test index, the final order -------------------------------------------------------------------
        test_users = None
        if H is not None:
            H = H[imap[icode[H]] >= 0]
            if warm:
                T = T[imap[icode[T]] >= 0]
            else:
                H = H[umap[ucode[H]] >= 0]
            H = H[B.bincount(ucode[H], n_u)[ucode[H]] == k]
            if warm:
                in_hold, in_test = B.bincount(ucode[H], n_u) > 0, B.bincount(ucode[T], n_u) > 0
                H, T = H[in_test[ucode[H]]], T[in_hold[ucode[T]]]
                key = B.first_pos(ucode[T], T, n_u)                       # surviving users by first appearance ...
                if first_key is not None:                                 # ... in the frame the sampling laid out by user
                    survives = key != _NONE
                    key[lo:hi] = first_key
                    key[~survives] = _NONE
                by_first = B.argsort(key)
                n_test_users = int((key != _NONE).sum())
                test_users = by_first[:n_test_users]
                tmap = B.full(n_u, -1)
                tmap[test_users] = B.arange(n_test_users)
            else:
                tmap = umap

            def triplets(rows):
                users = tmap[ucode[rows]]
                order = B.argsort(users)                                  # stable: original order inside a user
                rows = rows[order]
                return users[order], imap[icode[rows]], None if d['fb'] is None else d['fb'][rows]
            hold, test = triplets(H), (triplets(T) if warm else None)
        else:
            hold = test = None
        t0 = self._tick('indices and filters', t0)

        # -- download ---------------------------------------------------------------------------------------------------------
        def host(trip):
            if trip is None:
                return None
            u, i, f = (None if a is None else B.download(a) for a in trip)
            return self._frozen(u, i, np.ones(len(u)) if f is None else f)
        if full:
            self.__dict__['_lazy_train'] = host(c['training'])
            self.__dict__['_lazy_n_users'], self.__dict__['_lazy_n_items'] = c['n_train_users'], c['n_train_items']
            self._feedback_levels = None
            c['index_train_users'] = EntityIndex(B.download(c['train_users']), np.arange(c['n_train_users'], dtype=np.int64))
            c['index_items'] = EntityIndex(B.download(c['train_items']), np.arange(c['n_train_items'], dtype=np.int64))
            c['training'] = None
        test_index = None
        if test_users is not None:
            test_index = EntityIndex(B.download(d['users'][test_users]), np.arange(len(test_users), dtype=np.int64))
        self.index = DataIndex(UserIndex(c['index_train_users'], test_index), c['index_items'], None)
        self.__dict__['_lazy_test'] = TestData(host(test), host(hold))
        self._n_test_users = None
        self._tick('download', t0)
        self._cache, self._state = c, state
        self._change_properties = set()
        self._notify(self.on_change_event if full else self.on_update_event)


for _name in _CONFIG + ('seed',):
    setattr(RecommenderArrayData, _name, _config_property(_name))
del _name

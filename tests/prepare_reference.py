"""NumPy twin of the split of raw interactions (polara_amd/prepare.py, csrc/split.hip): `mix64`, the key construction, the
segmented selection and the whole `prepare()` pipeline, written for reading — one user at a time, rule by rule (DESIGN.md
§8r) — and sharing no code with the package.  All of it is integer work, so the device path is compared with it bit for bit.

    mix64(z)                                   pk_mix64 (csrc/pk_common.h) on uint64 arrays
    split_keys(order_vals, pos, mode, seed)    pk_split_keys: (key_hi, key_lo) as uint64 arrays
    segment_select(seg_ptr, hi, lo, k)         pk_segment_select: uint8 flags
    prepare_reference(users, items, ...)       the reference's `RecommenderData.prepare()` restated on arrays
"""
import numpy as np

ASCENDING, RANDOM_LO, NO_ORDER, POS_ASCENDING = 1, 2, 4, 8         # include/polara_hip.h: PK_SPLIT_*

DEFAULTS = dict(test_ratio=0.2, test_fold=5, warm_start=True, holdout_size=3, test_sample=None, permute_tops=False,
                random_holdout=False, negative_prediction=False, shuffle_data=False)


def mix64(z):
    z = np.array(z, dtype=np.uint64, ndmin=1)
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def split_keys(order_vals, pos, mode, seed):
    pos = np.asarray(pos, dtype=np.int64).astype(np.uint64)
    if mode & NO_ORDER:
        hi = np.zeros(len(pos), dtype=np.uint64)
    else:
        bits = np.array(order_vals, dtype=np.float64).view(np.uint64)
        bits[(bits << np.uint64(1)) == 0] = 0                        # -0.0 equals +0.0
        negative = (bits >> np.uint64(63)) == 1
        ascending = np.where(negative, ~bits, bits | np.uint64(1 << 63))   # u64 order = numeric order
        hi = ascending if mode & ASCENDING else ~ascending
    if mode & RANDOM_LO:
        lo = mix64(mix64(np.uint64(int(seed) % 2 ** 64)) + pos)
    elif mode & POS_ASCENDING:
        lo = pos
    else:
        lo = ~pos
    return hi, lo


def segment_select(seg_ptr, key_hi, key_lo, k):
    flags = np.zeros(len(key_hi), dtype=np.uint8)
    for b, e in zip(seg_ptr[:-1], seg_ptr[1:]):
        b, e = int(b), int(e)
        if e > b:
            smallest = np.lexsort((key_lo[b:e], key_hi[b:e]))[:k]
            flags[b + smallest] = 1
    return flags


def _per_user(rows, users):
    """{user: its rows, in the order given}, users in order of first appearance"""
    groups = {}
    for r in rows:
        groups.setdefault(int(users[r]), []).append(int(r))
    return groups


def _take(rows, key_hi, key_lo, k):
    rows = np.asarray(rows, dtype=np.int64)
    return rows[np.lexsort((key_lo, key_hi))[:k]]


def prepare_reference(users, items, feedback=None, custom_order=None, config=None, seed=0):
    """dict(training=(u, i, f), train_users, test_users, items: external ids in the order of their new numbers;
    testset, holdout: (u, i, f) sorted by user or None; holdout_size)."""
    cfg = dict(DEFAULTS)
    cfg.update(config or {})
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    n = len(users)
    fb = np.ones(n) if feedback is None else np.asarray(feedback, dtype=np.float64)
    order = custom_order if custom_order is not None else feedback
    k, ratio, fold, warm, t = cfg['holdout_size'], cfg['test_ratio'], cfg['test_fold'], cfg['warm_start'], cfg['test_sample']
    # 1. fold
    distinct = np.unique(users)
    code = np.searchsorted(distinct, users)
    if ratio > 0:
        num = len(distinct) * ratio
        in_fold = (code >= round((fold - 1) * num)) & (code < round(fold * num))
    else:
        in_fold = np.ones(n, dtype=bool)
    state4 = bool(warm and k and ratio > 0)
    # 2. holdout
    in_hold = np.zeros(n, dtype=bool)
    if k >= 1:
        if cfg['random_holdout'] or order is None:
            mode = NO_ORDER | RANDOM_LO
        else:
            mode = (ASCENDING if cfg['negative_prediction'] else 0) | (RANDOM_LO if cfg['permute_tops'] else 0)
        for rows in _per_user(np.flatnonzero(in_fold), users).values():
            hi, lo = split_keys(None if mode & NO_ORDER else np.asarray(order, dtype=np.float64)[rows], rows, mode, seed)
            in_hold[_take(rows, hi, lo, k)] = True
    # 3. parts
    train = ~in_fold if state4 else ~in_hold
    test_frame = list(np.flatnonzero(in_fold & ~in_hold)) if state4 else None
    # 4. test_sample: before any filter; the sampled frame lies user by user, users in order of first appearance
    if state4 and t:
        frame = []
        for rows in _per_user(test_frame, users).values():
            if t < 0:
                hi, lo = split_keys(fb[rows], rows, ASCENDING | POS_ASCENDING, 0)
            else:
                hi, lo = split_keys(None, rows, NO_ORDER | RANDOM_LO, seed + 1)
            frame.extend(int(r) for r in np.sort(_take(rows, hi, lo, abs(t))))
        test_frame = frame
    # 5. training index
    train_rows = np.flatnonzero(train)
    train_users = list(dict.fromkeys(int(u) for u in users[train_rows]))
    train_items = sorted(set(int(i) for i in items[train_rows]))
    user_new = {u: j for j, u in enumerate(train_users)}
    item_new = {i: j for j, i in enumerate(train_items)}
    training = (np.array([user_new[int(u)] for u in users[train_rows]], dtype=np.int64),
                np.array([item_new[int(i)] for i in items[train_rows]], dtype=np.int64), fb[train_rows])
    out = dict(training=training, train_users=np.array(train_users, dtype=np.int64), items=np.array(train_items, dtype=np.int64),
               test_users=None, testset=None, holdout=None, holdout_size=k)
    if k < 1:
        return out
    # 6. filters
    hold_frame = [int(r) for r in np.flatnonzero(in_hold)]
    hold_frame = [r for r in hold_frame if int(items[r]) in item_new]
    if state4:
        test_frame = [r for r in test_frame if int(items[r]) in item_new]
    else:
        hold_frame = [r for r in hold_frame if int(users[r]) in user_new]
    sizes = {u: len(rows) for u, rows in _per_user(hold_frame, users).items()}
    hold_frame = [r for r in hold_frame if sizes[int(users[r])] == k]
    if state4:
        hold_users, test_users_seen = set(int(users[r]) for r in hold_frame), set(int(users[r]) for r in test_frame)
        hold_frame = [r for r in hold_frame if int(users[r]) in test_users_seen]
        test_frame = [r for r in test_frame if int(users[r]) in hold_users]
        # 7. test index: first appearance in the surviving testset
        test_users = list(dict.fromkeys(int(users[r]) for r in test_frame))
        test_new = {u: j for j, u in enumerate(test_users)}
        out['test_users'] = np.array(test_users, dtype=np.int64)
    else:
        test_new = user_new

    # 8. sorted by user, original order inside a user
    def triplets(frame):
        frame = sorted(frame, key=lambda r: (test_new[int(users[r])], r))
        rows = np.array(frame, dtype=np.int64)
        return (np.array([test_new[int(users[r])] for r in frame], dtype=np.int64),
                np.array([item_new[int(items[r])] for r in frame], dtype=np.int64), fb[rows])
    out['holdout'] = triplets(hold_frame)
    if state4:
        out['testset'] = triplets(test_frame)
    return out

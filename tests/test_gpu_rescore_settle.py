"""The settle tier of the first re-scoring (pk_rescore_f64 with user_norm_dev): users whose order the candidate sweep's own
scores already decide get their lists without a gather — the lists stay the exact ones, every other user and every other
route is what it was.  The rule is restated in numpy (rescore_settle_reference.py); shapes: 333 users (partial waves, a
partial last segment), 700 items (22 tiles, the last one partial), the three segment instances (KC = 16, 32, 64)."""
import functools

import numpy as np
import pytest
import torch

import rescore_settle_reference as R

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 333, 700
# rank, list length (-> KC = 16, 32, 64), catalogue: chosen on the CPU (exact scores standing in for the sweep's, R.exact_stand_in)
# so that the restatement alone settles 221 / 300 / 208 of the 333 users — more than half, and more than ten left
CASES = {16: (8, 10, dict(clones=10)), 32: (50, 20, dict()), 64: (64, 50, dict(decay=0.8))}


@functools.lru_cache(maxsize=None)
def decaying_case(KC):
    K, topk, kw = CASES[KC]
    V = R.decaying_catalogue(K, N_ITEMS, K, **kw)
    indptr, indices, values = R.random_csr(np.random.RandomState(K + 1), N_USERS, N_ITEMS, 5, 60, R.popularity(N_ITEMS))
    E = R.fold(indptr, indices, values, V)
    return K, topk, V, indptr, indices, values, E, R.brute_topk(V, E, indptr, indices, topk)


def device_case(ops, V, indptr, indices, values):
    from polara_amd import scoring
    T = ops.csr(indptr, indices, values, (len(indptr) - 1, V.shape[0]))
    return T, scoring.FactorImage(ops, ops.to_device(V))


def first_pass(ops, F, T, topk, settle=True, item_norm=True, negate=None, second=False, perm=None, splits=1, then_without_norm=False):
    """fold-in, candidate sweep and FIRST re-scoring as `scoring.recommend` issues them for one batch: a single sweep with ONE
    list per user (what a pass over many users runs: the segment of the re-scoring kernel is then KC wide — 16 and 32: two
    users and one user per wave with two lanes per candidate, 64: one user per wave) or with `splits` lists per user (a
    small batch: KC * splits candidates, here always the 64-wide segment).  perm (int64 array): passed as `out_perm`, the list
    of user u goes to row perm[u].  then_without_norm: the same call is issued again at once — same stream, same ids, scores
    and flags buffers — without `user_norm`, and the results are those of that second call.  Returns host arrays: ids,
    flags, and what the restatement needs."""
    from polara_amd import scoring
    n, n_items = T.shape
    K, KC = F.K, ops.candidate_capacity(topk)
    Ex = ops.empty(n, F.Kx)
    if F.Q20 is not None and scoring.PACKED_FOLD_IN and topk <= scoring.PACKED_MAX_TOPK:
        ops.fold_q20(T, F.Q20, K, out=Ex, rows=(0, n))
    else:
        ops.spmm(T, F.V32x, out=Ex, rows=(0, n))
    if negate is not None:
        Ex[torch.as_tensor(negate, device=Ex.device), :K] *= -1.0
    E, w = Ex[:, :K], Ex[:, K]
    assert ops.sweep_takes_rows(E)
    seg = 16 if KC * splits <= 16 else 32 if KC * splits <= 32 else 64      # the kernel instance that runs (rescore.hip)
    un = torch.empty(n, dtype=torch.float32, device=Ex.device)
    cs, ci = ops.score_candidates(F.Vp, None, n, n_items, K, T.indptr, T.indices, KC, splits, tile_bound=F.tile_bound,
                                  seen_tiles=T.seen_tiles(), E_rows=(E, w, 1.2e-7), bound_out=un)
    lst, cnt = torch.empty(n, dtype=torch.int32, device=Ex.device), ops.zero_counters(1)
    kw = dict(splits=splits, e_err=w, flagged=(lst, cnt, 0), item_norm=F.vnorm if item_norm else None,
              user_norm=un if settle else None)
    if second:      # the second pass's call (E rows taken as exact) over every user
        kw.update(rows=torch.arange(n, dtype=torch.int32, device=Ex.device), e_exact=True)
    else:
        kw.update(v32=F.V32x)
    if perm is not None:
        kw.update(out_perm=torch.as_tensor(np.asarray(perm, dtype=np.int64), device=Ex.device))
    ids, sc, flags = ops.rescore_topk(F.V, E, n_items, T.indptr, KC, cs, ci, topk, F.vmax, **kw)
    if then_without_norm:
        lst, cnt = torch.empty_like(lst), ops.zero_counters(1)
        kw.update(user_norm=None, flagged=(lst, cnt, 0), out=(ids, sc, flags))
        ops.rescore_topk(F.V, E, n_items, T.indptr, KC, cs, ci, topk, F.vmax, **kw)
    h = ops.to_host
    return dict(ids=h(ids), flags=h(flags), listed=np.sort(h(lst)[:int(cnt.item())]), cs=h(cs), ci=h(ci), un=h(un), w=h(w).copy(),
                vnorm=h(F.vnorm), vmax=float(F.vmax), KC=KC, splits=splits, seg=seg, E=h(E).copy())


def restated(p, topk, K, n_seen, item_norm=True, n_items=N_ITEMS):
    return R.settle(p['cs'], p['ci'], p['KC'], p['splits'], len(p['un']), topk, K, p['un'], p['w'],
                    p['vnorm'] if item_norm else None, p['vmax'], n_items, n_seen)


def check_first_pass(ops, F, T, topk, ref, pk_options, **kw):
    """settled users: flag 8 alone, on no list, ids = the reference's; everybody else: ids, flags and the list of the users to
    re-do are those of the same call with the tier off"""
    on = first_pass(ops, F, T, topk, **kw)
    pk_options('rescore_settle', 0)
    off = first_pass(ops, F, T, topk, **kw)
    pk_options('rescore_settle', 1)
    assert not (off['flags'] & 8).any()
    st = (on['flags'] & 8) != 0
    assert np.array_equal(on['flags'][st], np.full(int(st.sum()), 8))
    assert np.array_equal(on['ids'][st], ref[st])
    assert np.array_equal(on['ids'][~st], off['ids'][~st]) and np.array_equal(on['flags'][~st], off['flags'][~st])
    assert np.array_equal(on['listed'], np.flatnonzero(on['flags'] & 7)) and np.array_equal(on['listed'], np.setdiff1d(off['listed'], np.flatnonzero(st)))
    return on, st


@pytest.mark.parametrize('KC,splits,seg', [(16, 1, 16), (32, 1, 32), (64, 1, 64), (16, 4, 64)])
def test_decaying_norm_catalogue_settles_what_the_rule_says(hip_ops, pk_options, KC, splits, seg):
    from polara_amd import scoring
    ops = hip_ops
    K, topk, V, indptr, indices, values, E, ref = decaying_case(KC)
    assert ops.candidate_capacity(topk) == KC
    T, F = device_case(ops, V, indptr, indices, values)
    on, st = check_first_pass(ops, F, T, topk, ref, pk_options, splits=splits)
    assert on['seg'] == seg and on['splits'] == splits
    if seg == 16:
        # two users per wave, users 2w and 2w + 1: waves where both settle (the scoring is branched round), where neither
        # does, MIXED ones (the settled user's lanes walk no row, its certification runs on empty sums and is replaced),
        # either half settling — and the last wave holds one live user next to a dead segment
        a, b = st[0:N_USERS - 1:2], st[1:N_USERS:2]
        assert (a & b).any() and (~a & ~b).any() and (a & ~b).any() and (~a & b).any() and N_USERS % 2 == 1
    want, margin = restated(on, topk, K, np.diff(indptr))
    print('KC %d x %d lists (segment %d): settled %d of %d on the device, %d by the restatement' % (KC, splits, seg, st.sum(), N_USERS, want.sum()))
    clear = np.abs(margin) > 1e-6
    assert np.array_equal(st[clear], want[clear]) and (~clear).sum() <= 3
    assert st.sum() >= N_USERS / 2 and (~st).sum() >= 10           # both branches are exercised
    # `out_perm` and `user_norm` are arguments of the one call: with the identity and with a shuffle of the 333 users the
    # flags are those of the call without `out_perm`, the list of user u sits in row perm[u], every settled user is flagged 8
    shuffle = np.random.RandomState(KC + splits).permutation(N_USERS)
    assert (shuffle != np.arange(N_USERS)).any()
    for perm in (np.arange(N_USERS), shuffle):
        moved = first_pass(ops, F, T, topk, perm=perm, splits=splits)
        assert np.array_equal(moved['flags'], on['flags']) and np.array_equal(moved['ids'][perm], on['ids'])
        assert np.array_equal(moved['flags'][st], np.full(int(st.sum()), 8))
    # ... and with `out_perm` but no `user_norm` nobody settles
    plain = first_pass(ops, F, T, topk, settle=False, perm=shuffle, splits=splits)
    assert not (plain['flags'] & 8).any()
    # nothing stays behind a call: the same call again on the same stream, into the same flags buffer, without `user_norm`
    # settles nobody — it is the call without the bounds, flag for flag and id for id
    for perm in (None, shuffle):
        again = first_pass(ops, F, T, topk, perm=perm, splits=splits, then_without_norm=True)
        assert not (again['flags'] & 8).any()
        assert np.array_equal(again['flags'], plain['flags']) and np.array_equal(again['ids'] if perm is None else again['ids'][perm], plain['ids'][shuffle])
    # the whole pass with the same number of lists: exact lists, byte-identical with the tier off, and the count it reports
    ops.score_splits_override = splits
    try:
        stats = {}
        got = ops.to_host(scoring.recommend(ops, F, T, topk, True, stats=stats))
        assert stats['item_splits'] == splits and stats['settled_users'] == int(st.sum())
        assert np.array_equal(got, ref)
        pk_options('rescore_settle', 0)
        st0 = {}
        assert np.array_equal(ops.to_host(scoring.recommend(ops, F, T, topk, True, stats=st0)), got)
        assert st0['settled_users'] == 0
        pk_options('rescore_settle', 1)
    finally:
        ops.score_splits_override = 0
    assert np.array_equal(ops.to_host(scoring.recommend(ops, F, T, topk, True)), ref)       # the route a pass of this size takes by default


@functools.lru_cache(maxsize=None)
def planted_case(exact):
    """660 items + 40 planted ones: copies of catalogue rows 1e-7 (relative) shorter — or the same rows again (exact duplicates:
    the order is by index).  Each of the first 40 users has an original among its best eight items, so the pair sits inside
    its top-10; what is left of the 40 copies goes to rows hardly anyone ranks (the restatement on exact scores then settles
    115 of the other users, none of the 40)."""
    K, topk = 50, 10
    base = R.decaying_catalogue(K, N_ITEMS - 40, K, latent=20, decay=0.05, noise=0.1)
    indptr, indices, values = R.random_csr(np.random.RandomState(5), N_USERS, N_ITEMS - 40, 5, 60, R.popularity(N_ITEMS - 40))
    E = R.fold(indptr, indices, values, base)
    S = E @ base.T
    S[np.repeat(np.arange(N_USERS), np.diff(indptr)), indices] = -np.inf
    rank = np.argsort(-S, axis=1, kind='stable')
    assert (np.take_along_axis(S, rank[:, :8], axis=1) > 0).all()
    users, twins = np.arange(40), []
    for u in users:
        if not np.isin(rank[u, :8], twins).any():
            twins.append(int(rank[u, 0]))
    seldom = np.argsort(np.bincount(rank[:, :17].ravel(), minlength=N_ITEMS - 40), kind='stable')
    twins += [int(a) for a in seldom if a not in twins][:40 - len(twins)]
    V = np.vstack([base, base[twins] * (1.0 if exact else 1.0 - 1e-7)])
    same = [(a, N_ITEMS - 40 + k) for k, a in enumerate(twins)] if exact else ()
    return K, topk, V, indptr, indices, values, users, np.array(twins), R.brute_topk(V, E, indptr, indices, topk, same)


@pytest.mark.parametrize('exact', [False, True], ids=['near_ties', 'duplicates'])
def test_ties_inside_the_list_never_settle(hip_ops, pk_options, exact):
    from polara_amd import scoring
    ops = hip_ops
    K, topk, V, indptr, indices, values, users, twins, ref = planted_case(exact)
    T, F = device_case(ops, V, indptr, indices, values)
    on, st = check_first_pass(ops, F, T, topk, ref, pk_options)
    assert on['seg'] == 16 and not st[users].any() and st.any()
    got = ops.to_host(scoring.recommend(ops, F, T, topk, True))
    assert np.array_equal(got, ref)         # (duplicates: the lower index first, as the reference's stable order has it)
    for u in users:       # a planted pair inside the top-10, the original in front of its twin
        pos = {int(i): t for t, i in enumerate(ref[u])}
        assert any(int(a) in pos and pos.get(N_ITEMS - 40 + k, -1) == pos[int(a)] + 1 for k, a in enumerate(twins)), u


def test_users_with_few_unseen_items_keep_the_exact_path(hip_ops, pk_options):
    from polara_amd import scoring
    ops = hip_ops
    K, topk, V, indptr, indices, values, E, ref = decaying_case(16)
    rng = np.random.RandomState(3)
    rows = [indices[indptr[u]:indptr[u + 1]] for u in range(N_USERS)]
    few = [4, 31, 32, 200, 332]
    for k, u in enumerate(few):       # n_items - n_seen = topk - 1, ..., down to 0 unseen items
        rows[u] = np.sort(rng.choice(N_ITEMS, size=N_ITEMS - max(topk - 1 - 3 * k, 0), replace=False)).astype(np.int32)
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ix = np.concatenate(rows).astype(np.int32)
    va = np.random.RandomState(4).randint(1, 6, size=len(ix)).astype(np.float32)
    ref = R.brute_topk(V, R.fold(ip, ix, va, V), ip, ix, topk)
    T, F = device_case(ops, V, ip, ix, va)
    on, st = check_first_pass(ops, F, T, topk, ref, pk_options)
    assert on['seg'] == 16 and not st[few].any() and (on['flags'][few] & 2).all() and st.sum() >= N_USERS / 2
    assert np.array_equal(ops.to_host(scoring.recommend(ops, F, T, topk, True)), ref)


def test_flat_norm_catalogue_needs_no_item_norms(hip_ops, pk_options):
    from polara_amd import scoring
    ops = hip_ops
    K, topk = 50, 10
    V = R.flat_catalogue(11, N_ITEMS, K)
    indptr, indices, values = R.random_csr(np.random.RandomState(12), N_USERS, N_ITEMS, 5, 60)
    ref = R.brute_topk(V, R.fold(indptr, indices, values, V), indptr, indices, topk)
    T, F = device_case(ops, V, indptr, indices, values)
    on, st = check_first_pass(ops, F, T, topk, ref, pk_options)
    plain = first_pass(ops, F, T, topk, item_norm=False)
    assert np.array_equal(plain['ids'], on['ids']) and np.array_equal(plain['flags'], on['flags']) and st.sum() >= N_USERS / 2
    want, margin = restated(on, topk, K, np.diff(indptr), item_norm=False)
    clear = np.abs(margin) > 1e-6
    assert np.array_equal(st[clear], want[clear])
    assert np.array_equal(ops.to_host(scoring.recommend(ops, F, T, topk, True)), ref)


def test_negative_scores(hip_ops, pk_options):
    """every other user's row of E negated behind the fold-in, over a catalogue whose rows share a direction: ALL scores of
    those users are negative — the signs of tau_cert and of the gaps"""
    ops = hip_ops
    K, topk = 50, 10
    V = R.decaying_catalogue(31, N_ITEMS, K, cone=2.0)
    indptr, indices, values = R.random_csr(np.random.RandomState(32), N_USERS, N_ITEMS, 5, 60, R.popularity(N_ITEMS))
    neg = np.arange(0, N_USERS, 2)
    En = R.fold(indptr, indices, values, V)
    En[neg] *= -1.0
    assert ((En @ V.T)[neg] < 0).all()
    ref = R.brute_topk(V, En, indptr, indices, topk)
    T, F = device_case(ops, V, indptr, indices, values)
    on, st = check_first_pass(ops, F, T, topk, ref, pk_options, negate=neg)
    want, margin = restated(on, topk, K, np.diff(indptr))
    clear = np.abs(margin) > 1e-6
    assert np.array_equal(st[clear], want[clear])
    assert st[neg].sum() >= len(neg) / 2 and (~st[neg]).any()       # (the restatement on exact scores: 146 of the 167)
    tau = on['cs'].reshape(on['splits'], -1, on['KC'])[:, :N_USERS, -1].max(axis=0)
    assert (tau[neg] < 0).all()                                     # settled against NEGATIVE thresholds of the sweep


def test_short_lists_have_no_threshold_term(hip_ops, pk_options):
    from polara_amd import scoring
    ops = hip_ops
    K, topk, n_items = 8, 10, 40
    V = R.decaying_catalogue(21, n_items, K, latent=4, noise=0.1)
    rng = np.random.RandomState(22)
    indptr = (np.arange(N_USERS + 1) * (n_items - 12)).astype(np.int64)           # 12 unseen items each: KC = 16 is never full
    indices = np.concatenate([np.sort(rng.choice(n_items, size=n_items - 12, replace=False)) for _ in range(N_USERS)]).astype(np.int32)
    values = rng.randint(1, 6, size=len(indices)).astype(np.float32)
    ref = R.brute_topk(V, R.fold(indptr, indices, values, V), indptr, indices, topk)
    T, F = device_case(ops, V, indptr, indices, values)
    on, st = check_first_pass(ops, F, T, topk, ref, pk_options)
    assert (on['ci'].reshape(on['splits'], -1, on['KC'])[:, :N_USERS, -1] < 0).all()        # no full list anywhere
    want, margin = restated(on, topk, K, np.diff(indptr), n_items=n_items)
    clear = np.abs(margin) > 1e-6
    assert np.array_equal(st[clear], want[clear]) and st.sum() >= 10
    assert np.array_equal(ops.to_host(scoring.recommend(ops, F, T, topk, True)), ref)


def test_routes_where_the_tier_stays_off(hip_ops, pk_options):
    from polara_amd import scoring
    ops = hip_ops
    K, topk, V, indptr, indices, values, E, ref = decaying_case(16)
    T, F = device_case(ops, V, indptr, indices, values)
    st = {}
    ids, sc = scoring.recommend(ops, F, T, topk, True, return_scores=True, stats=st)
    assert st['settled_users'] == 0
    pk_options('rescore_settle', 0)
    ids0, sc0 = scoring.recommend(ops, F, T, topk, True, return_scores=True)
    pk_options('rescore_settle', 1)
    assert torch.equal(ids, ids0) and torch.equal(sc.view(torch.int64), sc0.view(torch.int64))      # bit for bit the parent's kernel
    st = {}
    got = scoring.recommend(ops, F, T, topk, True, queries=ops.to_device(E), stats=st)
    assert st['settled_users'] == 0 and np.array_equal(ops.to_host(got), ref)
    second = first_pass(ops, F, T, topk, second=True)        # the second pass's call, handed the norm bounds all the same
    assert not (second['flags'] & 8).any()

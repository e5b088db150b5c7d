"""Settle at the sweep's exit (pk_score_candidates_f32 with a settle block): the rule of the first re-scoring's settle tier, applied by
the candidate sweep to a group's final lists when the group leaves the sweep — settled users get their ids and flag 8 there
and no candidate row, everybody else is appended to a device-side open list that the first re-scoring takes as its row list.
The route (option "sweep_settle", default on) must give what the tier inside the re-scoring gives (option off): the same
lists, flags, re-fold list and final list, and the same settled set — the one the numpy restatement computes.

Shapes: 75 users (three groups, the last with 11 live lanes), 300 items (10 tiles, the last with 12 real items), one rank per
rank class of the sweep — 12, 24, 40, 50, 72, 88, 104, 120, 150, 200, 250 (ranks 12 and 50: packed fold-in pieces of 2 and 8
lanes) — top-10 / KC 16 and top-20 / KC 32.  Seeds and clone counts were chosen on the
CPU so that the restatement ALONE (exact scores standing in for the sweep's, R.exact_stand_in; error weights 10, 40 and 160
fp32 roundings; with and without the seen filter) settles 20 to 53 of the 75 users and leaves 18 or more of the ordinary ones
open; every case asserts both populations again before it touches the device.

Three users are constructed to stay open: one whose two best items are identical rows of V (exact tie), one with an empty
row (all scores equal), one with fewer than topk unseen items.  The fourth way to stay open — a list that ends unbounded,
PK_IDX_FLOOR — cannot be produced through the library: the sweep writes that mark only if its own bootstrap invariant
breaks (at least KC items beat the bootstrapped threshold by construction).  The re-scoring side of the mark is covered by
test_gpu_kernels.test_rescore_sends_unbounded_lists_to_the_exact_path; the term in the sweep's exit is the same expression."""
import functools

import numpy as np
import pytest
import torch

import rescore_settle_reference as R
from recorded_calls import sweeps

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 75, 300
# (rank, topk) -> (seed, near-clone pairs): one rank per rank class of the sweep (NSTEP 1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16), each with
# top-10 / KC 16 and top-20 / KC 32 — the 22 instances the SETTLE twin of score_candidates_kernel exists for.  On the CPU the
# restatement alone settles 20 to 53 of the 75 users in every one of them (thinnest: rank 104 / top-20 without the seen
# filter at the 160-rounding weight, 20 against the floor of 18.75).
RANKS = (12, 24, 40, 50, 72, 88, 104, 120, 150, 200, 250)
CASES = {(K, topk): (11, 5 if topk == 10 else 0) for K in RANKS for topk in (10, 20)}
FULL_PRODUCT = ((12, 10), (12, 20), (50, 10), (50, 20))      # these take every (output order, filter) combination below
NEAR_TWINS = (60, 120)                               # items whose right-hand neighbour becomes their near-twin
TIE_USER, EMPTY_USER, FEW_USER = 3, 40, 70          # one per group; 70 sits among the 11 live lanes of the last one
CONSTRUCTED = (TIE_USER, EMPTY_USER, FEW_USER)


def _csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = (np.concatenate(rows) if indptr[-1] else np.zeros(0)).astype(np.int32)
    values = np.random.RandomState(len(indices)).randint(1, 6, size=len(indices)).astype(np.float32)
    return indptr, indices, values


# the chunked sweep's cases: every row of the catalogue shares a direction (all scores positive, so every ordinary user gets a
# threshold the norm bound can fall below and its group leaves early) and the empty row moves to the last group, next to the
# user who has seen nearly everything — those two keep THEIR group in the sweep to the last tile
CONE_CASES = {(12, 10): (6, 0), (50, 20): (3, 0)}
CONE_EMPTY_USER = 66


@functools.lru_cache(maxsize=None)
def case(K, topk, cone=False):
    seed, clones = (CONE_CASES if cone else CASES)[(K, topk)]
    EMPTY_USER = CONE_EMPTY_USER if cone else globals()['EMPTY_USER']
    KC = 16 if topk <= 10 else 32
    V = R.decaying_catalogue(seed, N_ITEMS, K, clones=clones, cone=2.0 if cone else 0.0)
    # near-twins, 1e-7 (relative) apart: the sweep's key-only flush sorts leave such a pair in either order, so the exit's own
    # sort has to MOVE list entries — with everything that travels with them (a norm bound that stayed behind once settled
    # users whose best items were a hair apart)
    for j in NEAR_TWINS:
        V[j + 1] = V[j] * (1.0 - 1e-7)
    indptr, indices, _ = R.random_csr(np.random.RandomState(seed + 1), N_USERS, N_ITEMS, 5, 40, R.popularity(N_ITEMS))
    rows = [indices[indptr[u]:indptr[u + 1]] for u in range(N_USERS)]
    rows[EMPTY_USER] = rows[EMPTY_USER][:0]
    rows[FEW_USER] = np.sort(np.random.RandomState(seed + 2).choice(N_ITEMS, size=N_ITEMS - (topk - 3), replace=False)).astype(np.int32)
    # the tie: the best item of TIE_USER over the whole catalogue (so that it leads the list with and without the seen filter)
    # gets a twin, an identical row of V in the place of an item nobody ranks; neither is among the user's seen items
    for _ in range(20):
        ip, ix, va = _csr(rows)
        S = R.fold(ip, ix, va, V) @ V.T
        best = int(np.argmax(S[TIE_USER]))
        if best not in rows[TIE_USER]:
            break
        rows[TIE_USER] = rows[TIE_USER][rows[TIE_USER] != best]
    else:
        raise AssertionError('no unseen best item')
    ranked = np.bincount(np.argsort(-S, axis=1)[:, :2 * KC].ravel(), minlength=N_ITEMS)
    ranked[rows[TIE_USER]] = N_USERS + 1
    ranked[best] = N_USERS + 1
    if cone:
        ranked[40:] = N_USERS + 1        # (the twin's norm must not hold the norm bound up to the last tile: nobody would leave early)
    twin = int(np.argmin(ranked + np.arange(N_ITEMS)[::-1] * 1e-6))      # the least ranked item, the last of those
    V[twin] = V[best]
    ip, ix, va = _csr(rows)
    return K, topk, KC, V, ip, ix, va, (min(best, twin), max(best, twin))


def cpu_populations(K, topk, KC, V, ip, ix, va, filter_seen):
    """what the restatement ALONE makes of the case (exact scores, stand-in error weights): settled mask"""
    E = R.fold(ip, ix, va, V)
    sp, si = (ip, ix) if filter_seen else (np.zeros_like(ip), ix[:0])
    out = []
    for scale in (10.0, 40.0, 160.0):        # the packed fold-in's weights are ~40 fp32 roundings: a factor 4 either way
        w = R.fold_weights(ip, ix, va, V, scale)
        cs, ci, un, vnorm, vmax = R.exact_stand_in(V, E, sp, si, KC, w)
        out.append(R.settle(cs, ci, KC, 1, N_USERS, topk, K, un, w, vnorm, vmax, N_ITEMS, np.diff(sp))[0])
    return out


def both_populations(settled, constructed=CONSTRUCTED):
    normal = np.ones(N_USERS, dtype=bool)
    normal[list(constructed)] = False
    return settled.sum() >= N_USERS / 4 and (~settled & normal).sum() >= 5


def run_pass(ops, monkeypatch, F, T, topk, filter_seen, perm=None, poison=False):
    """`scoring.recommend` as one ids-only batch with the calls of the pass looked into: the sweep's lists and settle block,
    the row list and the flagged lists of the two re-scorings, the flags behind each.  poison: the candidate rows of the
    users the sweep settled are overwritten behind the sweep (item 0 at +inf) — whoever reads them shows in the lists."""
    from polara_amd import scoring
    cap = {'rescore': []}
    sweep, rescore = ops.score_candidates, ops.rescore_topk
    n = T.shape[0]

    def score_candidates(*a, **kw):
        cs, ci = sweep(*a, **kw)
        q = kw.get('settle')
        cap.update(cs=cs, ci=ci, settle=q, un=kw.get('bound_out'), w=kw['E_rows'][1], KC=a[7])
        if q is not None:
            cnt = int(q['open_count'].item())
            cap['open'] = ops.to_host(q['open_list'])[:cnt].copy()
            cap['open_capacity'] = int(q['open_list'].numel())
            if poison:
                dead = torch.ones(n, dtype=torch.bool, device=cs.device)
                dead[q['open_list'][:cnt].long()] = False
                ci.view(-1, a[7])[:n][dead] = 0
                cs.view(-1, a[7])[:n][dead] = float('inf')
        return cs, ci

    def rescore_topk(*a, **kw):
        out = rescore(*a, **kw)
        cap['rescore'].append(dict(rows=kw.get('rows'), n_rows_dev=kw.get('n_rows_dev'), flagged=kw.get('flagged'),
                                   user_norm=kw.get('user_norm'), flags=out[2].clone()))
        return out

    monkeypatch.setattr(ops, 'score_candidates', score_candidates)
    monkeypatch.setattr(ops, 'rescore_topk', rescore_topk)
    stats = {}
    kw = {} if perm is None else {'_out_perm': perm}
    try:
        ops.score_splits_override = 1         # ONE list per user: the sweep a large user set gets (75 users alone would be dealt out)
        ids = ops.to_host(scoring.recommend(ops, F, T, topk, filter_seen, stats=stats, order_users=False, batches=1, **kw))
    finally:
        ops.score_splits_override = 0
        monkeypatch.undo()
    first, second = cap['rescore']

    def listed(f):
        lst, cnt, off = f
        return np.sort(ops.to_host(lst)[:int(cnt.item())] - off)
    h = ops.to_host
    return dict(ids=ids, stats=stats, flags1=h(first['flags']), flags=h(second['flags']), refold=listed(first['flagged']),
                final=listed(second['flagged']), open=cap.get('open'), at_exit=cap['settle'] is not None,
                first_rows=first['rows'], cs=h(cap['cs']), ci=h(cap['ci']), un=None if cap['un'] is None else h(cap['un']),
                w=h(cap['w']).copy(), KC=cap['KC'], open_capacity=cap.get('open_capacity'))


def device_case(ops, V, ip, ix, va):
    from polara_amd import scoring
    return ops.csr(ip, ix, va, (N_USERS, N_ITEMS)), scoring.FactorImage(ops, ops.to_device(V))


def reference(V, ip, ix, va, topk, filter_seen, same):
    E = R.fold(ip, ix, va, V)
    return R.brute_topk(V, E, ip, ix, topk, [same]) if filter_seen else R.brute_topk(V, E, np.zeros_like(ip), ix[:0], topk, [same])


def check_equivalent(on, off, ref, perm=None):
    """the route against the tier: lists, flags behind either re-scoring, re-fold and final lists, the count"""
    assert on['at_exit'] and not off['at_exit'] and on['first_rows'] is not None and off['first_rows'] is None
    want = ref if perm is None else ref[np.argsort(perm)]        # row perm[u] holds user u's list
    assert np.array_equal(off['ids'], want)
    assert np.array_equal(on['ids'], off['ids'])
    assert np.array_equal(on['flags1'], off['flags1']) and np.array_equal(on['flags'], off['flags'])
    assert np.array_equal(on['refold'], off['refold']) and np.array_equal(on['final'], off['final'])
    assert on['stats']['settled_users'] == off['stats']['settled_users'] == int(((on['flags'] & 8) != 0).sum())
    assert on['stats']['refolded_users'] == off['stats']['refolded_users'] and on['stats']['flagged_users'] == off['stats']['flagged_users']
    settled = (on['flags'] & 8) != 0
    assert np.array_equal(on['flags'][settled], np.full(int(settled.sum()), 8))
    return settled


def check_open_list(on, settled, filter_seen, constructed=CONSTRUCTED):
    """the open count is n_users - settled, nobody twice, no padding user, every constructed user exactly once"""
    lst = on['open']
    assert len(lst) == N_USERS - int(settled.sum()) and on['open_capacity'] >= N_USERS
    assert len(np.unique(lst)) == len(lst) and lst.min() >= 0 and lst.max() < N_USERS
    assert np.array_equal(np.sort(lst), np.flatnonzero(~settled))
    for u in constructed if filter_seen else constructed[:2]:     # (without the filter nobody is short of unseen items)
        assert int((lst == u).sum()) == 1, u


ROUTE_CASES = [(K, topk, with_perm, filter_seen) for K, topk in sorted(CASES) for with_perm in (False, True) for filter_seen in (True, False)
               if (K, topk) in FULL_PRODUCT or (with_perm, filter_seen) in ((False, True), (True, False))]


@pytest.mark.parametrize('K,topk,with_perm,filter_seen', ROUTE_CASES,
                         ids=['%d-%d-%s-%s' % (K, topk, 'out_perm' if p else 'plain', 'filter_seen' if f else 'no_filter') for K, topk, p, f in ROUTE_CASES])
def test_route_equals_the_tier_of_the_first_rescoring(hip_ops, pk_options, monkeypatch, K, topk, with_perm, filter_seen):
    ops = hip_ops
    K, topk, KC, V, ip, ix, va, same = case(K, topk)
    assert ops.candidate_capacity(topk) == KC
    assert all(both_populations(s) for s in cpu_populations(K, topk, KC, V, ip, ix, va, filter_seen))
    T, F = device_case(ops, V, ip, ix, va)
    ref = reference(V, ip, ix, va, topk, filter_seen, same)
    perm = torch.as_tensor(np.random.RandomState(7).permutation(N_USERS), dtype=torch.int64, device=ops.device) if with_perm else None
    on = run_pass(ops, monkeypatch, F, T, topk, filter_seen, perm)
    pk_options('sweep_settle', 0)
    off = run_pass(ops, monkeypatch, F, T, topk, filter_seen, perm)
    pk_options('sweep_settle', 1)
    settled = check_equivalent(on, off, ref, None if perm is None else ops.to_host(perm))
    print('rank %d top-%d: %d of %d settled at the exit, %d open, %d re-folded' % (K, topk, settled.sum(), N_USERS, len(on['open']), len(on['refold'])))
    assert both_populations(settled)
    check_open_list(on, settled, filter_seen)
    # the open users' candidate rows are those of the plain sweep, bit for bit
    rows_on, rows_off = on['ci'].reshape(-1, KC)[:N_USERS], off['ci'].reshape(-1, KC)[:N_USERS]
    assert np.array_equal(rows_on[~settled], rows_off[~settled])
    assert np.array_equal(on['cs'].view(np.int32).reshape(-1, KC)[:N_USERS][~settled], off['cs'].view(np.int32).reshape(-1, KC)[:N_USERS][~settled])
    # "rescore_settle" = 0 switches the rule off wherever it runs
    pk_options('rescore_settle', 0)
    none = run_pass(ops, monkeypatch, F, T, topk, filter_seen, perm)
    pk_options('rescore_settle', 1)
    assert not none['at_exit'] and none['stats']['settled_users'] == 0 and np.array_equal(none['ids'], on['ids'])


@pytest.mark.parametrize('K,topk', sorted(CASES))
def test_settled_set_is_the_restatements(hip_ops, pk_options, monkeypatch, K, topk):
    """the settled mask of the route = the numpy rule on the sweep's own lists (taken from the plain sweep of the same inputs:
    the route does not write the settled users' rows — the rows it does write are checked equal in the test above)"""
    ops = hip_ops
    K, topk, KC, V, ip, ix, va, same = case(K, topk)
    T, F = device_case(ops, V, ip, ix, va)
    on = run_pass(ops, monkeypatch, F, T, topk, True)
    pk_options('sweep_settle', 0)
    off = run_pass(ops, monkeypatch, F, T, topk, True)
    pk_options('sweep_settle', 1)
    settled = (on['flags'] & 8) != 0
    vnorm, vmax = ops.to_host(F.vnorm), float(F.vmax)
    want, margin = R.settle(off['cs'], off['ci'], KC, 1, N_USERS, topk, K, off['un'], off['w'], vnorm, vmax, N_ITEMS, np.diff(ip))
    clear = np.abs(margin) > 1e-6            # (within 1e-6 of the bound the device's rounding of the same expressions may decide)
    print('rank %d top-%d: %d settled on the device, %d by the restatement, %d within 1e-6 of a bound' % (K, topk, settled.sum(), want.sum(), (~clear).sum()))
    assert np.array_equal(settled[clear], want[clear]) and (~clear).sum() <= 2
    assert both_populations(settled) and both_populations(want)
    assert not settled[list(CONSTRUCTED)].any() and not want[list(CONSTRUCTED)].any()
    assert (on['flags'][FEW_USER] & 2) and np.array_equal(settled, (off['flags'] & 8) != 0)


@pytest.mark.parametrize('K,topk', [(12, 10), (50, 20)])
def test_groups_that_leave_in_different_chunk_launches(hip_ops, pk_options, monkeypatch, K, topk):
    """the sweep cut into launches of 1, 2, 4, ... tiles (the smallest chunk the entry takes): a group settles in the launch
    it leaves in — once — and the parked lists of the others are not touched by it"""
    ops = hip_ops
    K, topk, KC, V, ip, ix, va, same = case(K, topk, cone=True)
    constructed = (TIE_USER, CONE_EMPTY_USER, FEW_USER)
    assert all(both_populations(s, constructed) for s in cpu_populations(K, topk, KC, V, ip, ix, va, True))
    T, F = device_case(ops, V, ip, ix, va)
    ref = reference(V, ip, ix, va, topk, True, same)
    try:
        ops.score_tiles_per_chunk = 1
        on = run_pass(ops, monkeypatch, F, T, topk, True)
        exits = ops.to_host(ops.score_exit_tiles(N_USERS))[0]
        pk_options('sweep_settle', 0)
        off = run_pass(ops, monkeypatch, F, T, topk, True)
        pk_options('sweep_settle', 1)
    finally:
        ops.score_tiles_per_chunk = 0
    launch = np.searchsorted(np.array([1, 3, 7]), exits, side='right')      # launches cover tiles [0, 1), [1, 3), [3, 7), [7, 10)
    print('exit tiles', exits, 'launches', launch)
    assert len(set(launch.tolist())) >= 2
    settled = check_equivalent(on, off, ref)
    assert both_populations(settled, constructed)
    check_open_list(on, settled, True, constructed)
    one = run_pass(ops, monkeypatch, F, T, topk, True)                     # the single launch settles the same users
    assert np.array_equal((one['flags'] & 8) != 0, settled)


@pytest.mark.parametrize('K,topk', [(50, 10), (12, 20)])
def test_nobody_reads_a_settled_users_candidate_row(hip_ops, monkeypatch, K, topk):
    ops = hip_ops
    K, topk, KC, V, ip, ix, va, same = case(K, topk)
    T, F = device_case(ops, V, ip, ix, va)
    ref = reference(V, ip, ix, va, topk, True, same)
    got = run_pass(ops, monkeypatch, F, T, topk, True, poison=True)
    settled = (got['flags'] & 8) != 0
    assert got['at_exit'] and both_populations(settled)
    assert (got['ci'].reshape(-1, KC)[:N_USERS][settled] == 0).all()       # the poison was in place
    assert np.array_equal(got['ids'], ref)
    check_open_list(got, settled, True)
    assert got['stats']['flagged_users'] == len(got['final']) and got['stats']['refolded_users'] == len(got['refold'])


def test_recorded_and_captured_passes_take_the_route(hip_ops, pk_options):
    """RecordedPass / CapturedPass record whatever sequence `recommend` issues: the settle entry among the recorded calls,
    the replays' lists those of the direct call"""
    from polara_amd import scoring
    ops = hip_ops
    K, topk, KC, V, ip, ix, va, same = case(50, 10)
    T, F = device_case(ops, V, ip, ix, va)
    ref = reference(V, ip, ix, va, topk, True, same)
    try:
        ops.score_splits_override = 1
        rec = scoring.RecordedPass(ops, F, T, topk)
        names = [name for name, _, _ in rec.calls]
        swept = sweeps(rec.calls)
        assert len(swept) == 1 and swept[0]['entry'] == 'pk_score_candidates_f32' and swept[0]['settle'], swept
        assert 'pk_zero_i32' not in names, names
        for _ in range(2):
            assert np.array_equal(ops.to_host(rec.replay()), ref)
        pk_options('sweep_settle', 0)
        swept = sweeps(scoring.RecordedPass(ops, F, T, topk).calls)
        pk_options('sweep_settle', 1)
        assert len(swept) == 1 and swept[0]['entry'] == 'pk_score_candidates_f32', swept
        assert not swept[0]['settle'] and swept[0]['user_bound_out'] and swept[0]['E'], swept
        cap = scoring.CapturedPass(ops, F, T, topk)
        for _ in range(2):
            assert np.array_equal(ops.to_host(cap.replay()), ref)
    finally:
        ops.score_splits_override = 0

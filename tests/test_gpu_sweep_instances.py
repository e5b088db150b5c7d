"""-m gpu: every instance of score_candidates_kernel (csrc/score.hip) on every route, its raw lists held to the sweep's own
contract (sweep_contract_reference.py: ids, scores within the certified error, completeness) against fp64 NumPy.

The kernel is a matrix of instances — NSTEP (k-steps of 16, picked by the rank) x KC (list size) x form — which differ in ring
depth, where the lists live (LDS or global memory), the merge network and the dynamic LDS size.  Every rank class runs at its
smallest rank (most zero padding) and its largest (16 * NSTEP), with KC = 16, 32 and 64; every case runs the routes

  route                                        form(s) of the kernel it launches                          NSTEP    KC
  a  full sweep, 1 launch / chunks of 3 tiles  plain (state parked and resumed)                           all      16 32 64
  b  pruned sweep from the rows of E           plain, fragments built in the prologue (= packed route)    all      16 32 64
  c  pruned sweep with dense seen masks        DENSE for NSTEP <= 8; plain for NSTEP > 8 (request unused) all      16 32 64
  d  item splits (4 / 2), pruned, chunks of 2  STRIDED (independent splits, stream only)                  all      16 32
  e  two-phase, head 8, splits 3 / 2           head: plain or DENSE; tail: STRIDED (+ DENSE), then merge  all      16 32 64
  f  full sweep without a seen filter          plain, no stream                                           all      16 32 64
  pass with scores (`scoring.recommend`)       what the pass picks for 70 users: STRIDED (item splits)    all      16 32 64
  pass, ids only, one list per user            the SETTLE twin (single pruned sweep, settle at the exit)  all (*)  16 32

(the exact pass folds in exactly, so it never settles; the ids-only pass with `score_splits_override = 1` is the one that
launches the SETTLE twin, checked here against the fp64 brute force — the twin's own contract, the settled set, is
test_gpu_sweep_settle.py's, at every rank class too; (*) not at rank 256 itself, whose ids-only pass folds in exactly —
NSTEP 16 settles at rank 209).  At KC = 64 one split is all `score_candidates` takes, which is route b:
STRIDED at KC = 64 is reached through the two-phase sweep only.

Shape: 70 users (three groups, the last with 6 live lanes), 1289 items (41 tiles, the last with 9 real items), a decaying
catalogue inside a cone (all scores positive), rows of 5..40 items drawn by popularity, and three constructed users: an empty
row in group 0, a user who has seen all but 5 items in group 1 (fewer than KC and than topk: keeps the group in the sweep to
the last tile), a user with half the catalogue seen in group 2.  An estimate from the exact scores (asserted per case before
the device is touched) has groups 0 and 2 leave the pruned sweep early and group 1 stay.

Six more users of group 1 have seen every item of the first 8 tiles, the head of the two-phase sweep (and three of every
four items of the next 8 tiles): their head lists stay empty, so the tail sweeps start cold for them — each of the splits fills its rings, flushes and leaves a full list, and the
merge network picks KC of 2 KC or 3 KC real entries.  (For everybody else the head of this decaying catalogue holds nearly the
whole list and the tail pushes next to nothing.)  The counts are asserted on the CPU first and on the raw lists afterwards."""
import functools

import numpy as np
import pytest
import torch

import rescore_settle_reference as R
import sweep_contract_reference as C

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 70, 1289
N_PAD, N_TILES = 96, 41
EMPTY_USER, FEW_USER, LONG_USER = 5, 40, 66            # groups 0, 1, 2
CONSTRUCTED = (EMPTY_USER, FEW_USER, LONG_USER)
TAIL_USERS = (41, 44, 47, 52, 57, 63)                  # group 1: everything in the head of the two-phase sweep seen
SEED_V, SEED_ROWS, CONE = 21, 22, 0.25
EXTRA_SCALE = 1.2e-7
RANKS = {1: (1, 16), 2: (17, 32), 3: (33, 48), 4: (49, 64), 5: (65, 80), 6: (81, 96), 7: (97, 112), 8: (113, 128),
         10: (129, 160), 13: (161, 208), 16: (209, 256)}                # NSTEP -> (smallest, largest rank of the class)
TOPK = {16: 10, 32: 24, 64: 52}                        # the largest top-k each list size takes
HEAD_TILES, DENSE_TILES = 8, 5


def nstep_of(K):
    return min(n for n in RANKS if 16 * n >= K)


@functools.lru_cache(maxsize=None)
def rows_of_the_users():
    ip, ix, _ = R.random_csr(np.random.RandomState(SEED_ROWS), N_USERS, N_ITEMS, 5, 40, R.popularity(N_ITEMS))
    rows = [ix[ip[u]:ip[u + 1]] for u in range(N_USERS)]
    rng = np.random.RandomState(SEED_ROWS + 1)
    rows[EMPTY_USER] = rows[EMPTY_USER][:0]
    rows[FEW_USER] = np.sort(rng.choice(N_ITEMS, size=N_ITEMS - 5, replace=False)).astype(np.int32)
    rows[LONG_USER] = np.sort(rng.choice(N_ITEMS, size=N_ITEMS // 2, replace=False)).astype(np.int32)
    # (and three of every four items of the next 8 tiles: at rank 1 the scores fall with the item index, and the best KC of the
    # rest must still come from more than one tile, that is from more than one split)
    beyond = np.arange(32 * HEAD_TILES, 64 * HEAD_TILES)
    for u in TAIL_USERS:
        rows[u] = np.union1d(rows[u], np.r_[np.arange(32 * HEAD_TILES), beyond[beyond % 4 != 0]]).astype(np.int32)
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ix = np.concatenate(rows).astype(np.int32)
    va = np.random.RandomState(SEED_ROWS + 2).randint(1, 6, size=len(ix)).astype(np.float32)
    return ip, ix, va


@functools.lru_cache(maxsize=None)
def host_case(K):
    """the NumPy side of a rank, computed once and never changed: catalogue, rows, fp64 fold, error weights, the contract's
    reference (exact scores, bounds) with and without the seen filter"""
    ip, ix, va = rows_of_the_users()
    V = R.decaying_catalogue(SEED_V, N_ITEMS, K, latent=min(3, K), cone=CONE)      # (rank 1 has one direction to offer)
    E = R.fold(ip, ix, va, V)
    w = R.fold_weights(ip, ix, va, V)
    ref = C.SweepContract(V, E, (ip, ix))
    for a in (V, E, w, ref.exact, ref.bound):
        a.setflags(write=False)
    return dict(V=V, E=E, w=w, ip=ip, ix=ix, va=va, ref=ref, nof=ref.without_filter())


def estimated_exit_tiles(h, KC):
    """where each group would leave a pruned single sweep whose thresholds were exact: the first tile t at which
    bound_u * tile_bound[t] <= (KC-th best exact score of u's unseen items in the tiles before t) for all of its users"""
    ref = h['ref']
    un = np.linalg.norm(h['E'], axis=1) * (1 + 1e-6) + EXTRA_SCALE * h['w']
    vn = np.linalg.norm(h['V'], axis=1)
    tb = np.maximum.accumulate(vn[::-1])[::-1][::32] * (1 + 3e-6)
    s = np.where(ref.seen_mask, -np.inf, ref.exact)
    exits = np.full(3, N_TILES)
    for g in range(3):
        users = np.arange(32 * g, min(32 * g + 32, N_USERS))
        for t in range(1, N_TILES):
            head = np.sort(s[users, :32 * t], axis=1)[:, ::-1]
            tau = head[:, KC - 1] if head.shape[1] >= KC else np.full(len(users), -np.inf)
            if (un[users] * tb[t] <= tau).all():
                exits[g] = t
                break
    return exits


def tail_conditions(h, KC, splits):
    """what the exact scores say of the second phase of the two-phase sweep: (users with at least KC unseen tail items above
    the KC-th best unseen item of the head — above anything when the head holds fewer than KC —, users whose exact top-KC
    holds items of at least two tail splits)"""
    ref = h['ref']
    s = np.where(ref.seen_mask, -np.inf, ref.exact)
    n_head = 32 * HEAD_TILES
    head = np.sort(s[:, :n_head], axis=1)[:, ::-1]
    tau = head[:, KC - 1]                                            # -inf: fewer than KC unseen items in the head
    beat = ((s[:, n_head:] > tau[:, None]) & np.isfinite(s[:, n_head:])).sum(axis=1)
    top = np.argsort(-s, axis=1, kind='stable')[:, :KC]
    in_tail = (top >= n_head) & np.isfinite(np.take_along_axis(s, top, axis=1))
    split_of = (top // 32 - HEAD_TILES) % splits
    n_splits = np.array([len(set(split_of[u][in_tail[u]])) for u in range(N_USERS)])
    return int((beat >= KC).sum()), int((n_splits >= 2).sum())


@functools.lru_cache(maxsize=None)
def pass_reference(K, topk):
    """fp64 brute force of the pass and the users its comparison takes: the rule of test_fused_scoring_pipeline_exact (the
    k-th and (k+1)-th exact scores more than 1e-12 * max(1, |best|) apart, rows of E not all zero)"""
    h = host_case(K)
    ref = h['ref']
    want = R.brute_topk(h['V'], h['E'], h['ip'], h['ix'], topk)
    chk = np.abs(h['E']).sum(axis=1) > 0
    for u in range(N_USERS):
        ss = np.sort(ref.exact[u][~ref.seen_mask[u]])[::-1]
        if len(ss) > topk:
            chk[u] &= (ss[topk - 1] - ss[topk]) > 1e-12 * max(1.0, abs(ss[0]))
    return want, chk


def device_case(ops, h, K):
    from polara_amd import scoring
    T = ops.csr(h['ip'], h['ix'], h['va'], (N_USERS, N_ITEMS))
    F = scoring.FactorImage(ops, ops.to_device(h['V']))
    ld = K + 1 + (K + 1) % 2                                       # the smallest even leading dimension that holds the weights
    block = np.zeros((N_USERS, ld))
    block[:, :K], block[:, K] = h['E'], h['w']
    Ex = ops.to_device(block)
    E, w = Ex[:, :K], Ex[:, K]
    assert ops.sweep_takes_rows(E)
    Ep, ub = ops.pack_frag_bound(E, extra=w, extra_scale=EXTRA_SCALE)
    st = T.seen_tiles()
    dense, skip = ops.seen_dense(T.indptr, st[0], st[1], N_USERS, DENSE_TILES)
    return dict(T=T, F=F, E=E, w=w, Ep=Ep, ub=ub, st=st, sd=(dense, skip, DENSE_TILES))


def lists(ops, out, KC, n_lists=1):
    cs, ci = ops.to_host(out[0]), ops.to_host(out[1])
    assert cs.size == ci.size == n_lists * N_PAD * KC
    return cs.reshape(n_lists, N_PAD, KC), ci.reshape(n_lists, N_PAD, KC)


def same_bits(a, b):
    return np.array_equal(a[0][:, :N_USERS].view(np.int32), b[0][:, :N_USERS].view(np.int32)) and np.array_equal(a[1][:, :N_USERS], b[1][:, :N_USERS])


def two_phase_with_raw_lists(ops, d, K, KC, splits, seen_dense):
    """`ops.score_two_phase` from the rows of E into work arrays of the test's own: the merged list and the raw ones (slot 0:
    head, then the splits)"""
    total = splits + 1
    ws = torch.empty(total * N_PAD * KC, dtype=torch.float32, device=ops.device)
    wi = torch.empty(total * N_PAD * KC, dtype=torch.int32, device=ops.device)
    out = ops.score_two_phase(d['F'].Vp, None, N_USERS, N_ITEMS, K, d['T'].indptr, KC, HEAD_TILES, splits, None, d['F'].tile_bound,
                              seen_tiles=d['st'], seen_dense=seen_dense, tiles_per_chunk=2, E_rows=(d['E'], d['w'], EXTRA_SCALE),
                              work=(ws, wi))
    return lists(ops, out, KC), lists(ops, (ws, wi), KC, total)


CASES = [(K, KC) for n in sorted(RANKS) for K in RANKS[n] for KC in (16, 32, 64)]


@pytest.mark.parametrize('K,KC', CASES, ids=['nstep%d_rank%d_kc%d%s' % (nstep_of(K), K, KC, '_splits_are_route_b' if KC == 64 else '')
                                            for K, KC in CASES])
def test_every_route_of_the_instance_keeps_the_sweeps_contract(hip_ops, monkeypatch, K, KC):
    from polara_amd import scoring
    ops = hip_ops
    h = host_case(K)
    ref, nof = h['ref'], h['nof']
    topk = TOPK[KC]
    assert ops.candidate_capacity(topk) == KC and ops.candidate_capacity(topk + 1) != KC
    assert ops.lib.pk_pack_kq(K) == 2 * nstep_of(K)
    # ---- conditions of the inputs, from the exact scores alone
    est = estimated_exit_tiles(h, KC)
    assert est[0] < N_TILES // 2 and est[2] < N_TILES // 2 and est[1] == N_TILES, est
    want, chk = pass_reference(K, topk)
    left_out = np.flatnonzero(~chk)
    assert len(np.setdiff1d(left_out, CONSTRUCTED)) <= 2, left_out
    unseen = (~ref.seen_mask).sum(axis=1)
    assert unseen[FEW_USER] == 5 and unseen[EMPTY_USER] == N_ITEMS and abs(unseen[LONG_USER] - N_ITEMS // 2) <= 1
    splits = 3 if KC <= 32 else 2                      # of the two-phase sweep
    assert not ref.seen_mask[list(TAIL_USERS), 32 * HEAD_TILES:].all(axis=1).any() and ref.seen_mask[list(TAIL_USERS), :32 * HEAD_TILES].all()
    cold_tail_users, two_split_users = tail_conditions(h, KC, splits)
    assert cold_tail_users >= len(TAIL_USERS) and two_split_users >= len(TAIL_USERS), (cold_tail_users, two_split_users)

    d = device_case(ops, h, K)
    T, F, st = d['T'], d['F'], d['st']
    rows = (d['E'], d['w'], EXTRA_SCALE)
    one = [C.all_tiles(N_ITEMS)]
    worst, merged_users = {}, {}

    def sweep(Ep=None, **kw):
        return lists(ops, ops.score_candidates(F.Vp, Ep, N_USERS, N_ITEMS, K, T.indptr, T.indices, KC, seen_tiles=st, **kw), KC, kw.get('splits', 1))

    # a. full sweep: one launch, and chunks of 3 tiles
    for name, chunk in (('a_full', 64), ('a_full_chunks_of_3', 3)):
        got = sweep(d['Ep'], tiles_per_chunk=chunk)
        worst[name] = ref.check(KC, got[0], got[1], one)
        assert (ops.to_host(ops.score_exit_tiles(N_USERS))[0] == N_TILES).all()
    # b. pruned single sweep from the rows of E = the packed pruned route, bit for bit
    b = sweep(tile_bound=F.tile_bound, E_rows=rows)
    exits = ops.to_host(ops.score_exit_tiles(N_USERS))[0]
    packed = sweep(d['Ep'], user_bound=d['ub'], tile_bound=F.tile_bound)
    worst['b_pruned_rows'] = ref.check(KC, b[0], b[1], one)
    assert same_bits(b, packed)
    assert exits[1] == N_TILES and (exits[[0, 2]] < N_TILES).any(), (exits, est)
    # c. the same sweep with dense seen masks for the first tiles (NSTEP > 8: the request is not used, the stream serves every tile)
    c = sweep(tile_bound=F.tile_bound, E_rows=rows, seen_dense=d['sd'])
    worst['c_dense'] = ref.check(KC, c[0], c[1], one)
    assert same_bits(c, b)
    # d. item splits, each list against its own tiles (KC = 64 takes one split only: route b)
    S = 64 // KC
    if S > 1:
        got = sweep(tile_bound=F.tile_bound, E_rows=rows, splits=S, tiles_per_chunk=2)
        worst['d_splits'] = ref.check(KC, got[0], got[1], [C.split_tiles(N_ITEMS, s, S) for s in range(S)])
        ex = ops.to_host(ops.score_exit_tiles(N_USERS, S))
        assert ex.shape == (S, 3) and (ex[:, 1] == N_TILES).all() and (ex <= N_TILES).all()
    # e. two-phase: the merged list over all tiles, and = the KC best of the union of the raw lists
    tail = list(TAIL_USERS)
    for name, sd in (('e_two_phase', None), ('e_two_phase_dense', d['sd'])):
        merged, raw = two_phase_with_raw_lists(ops, d, K, KC, splits, sd)
        worst[name] = ref.check(KC, merged[0], merged[1], one)
        raw_tiles = [np.arange(HEAD_TILES)] + [C.split_tiles(N_ITEMS, s, splits, HEAD_TILES) for s in range(splits)]
        # (a split starts from the head's thresholds and keeps only what beats them: C1 and C2 hold for the raw lists, C3 need not)
        worst[name + '_raw'] = ref.check(KC, raw[0], raw[1], raw_tiles, completeness=False)
        # the users who have seen the whole head: an empty head list, and every split sweeps cold and leaves a full list
        assert (raw[1][0, tail] < 0).all() and (raw[1][1:, tail] >= 0).all(), name
        ms, mi = C.merged_best(KC, raw[0], raw[1], N_USERS)
        gs, gi = merged[0][0, :N_USERS], np.maximum(merged[1][0, :N_USERS], -1)
        # as sets (a head list that nothing in the tail beat goes out in the head's own key order): entries sorted by item
        by_item = np.argsort(np.where(mi >= 0, mi, 2 ** 31 - 1), axis=1, kind='stable')
        got_by_item = np.argsort(np.where(gi >= 0, gi, 2 ** 31 - 1), axis=1, kind='stable')
        want_i, want_s = np.take_along_axis(mi, by_item, axis=1), np.take_along_axis(ms, by_item, axis=1)
        got_i, got_s = np.take_along_axis(gi, got_by_item, axis=1), np.take_along_axis(gs, got_by_item, axis=1)
        assert np.array_equal(got_i, want_i), (name, np.flatnonzero((got_i != want_i).any(axis=1))[:5])
        assert np.array_equal(got_s.view(np.int32)[want_i >= 0], want_s.view(np.int32)[want_i >= 0]), name
        # and in the documented order wherever the merge network ran (a tail list holds something)
        moved = (raw[1][1:, :N_USERS] >= 0).any(axis=(0, 2))
        assert np.array_equal(gi[moved], mi[moved]) and np.array_equal(gs[moved].view(np.int32)[mi[moved] >= 0], ms[moved].view(np.int32)[mi[moved] >= 0]), name
        merged_users[name] = int(moved.sum())
        assert moved[tail].all() and merged_users[name] >= len(TAIL_USERS) + 1, (name, merged_users)       # (+ the few-unseen user)
    # f. no seen filter
    got = lists(ops, ops.score_candidates(F.Vp, d['Ep'], N_USERS, N_ITEMS, K, None, None, KC), KC)
    worst['f_no_filter'] = nof.check(KC, got[0], got[1], one)

    print('rank %d (NSTEP %d) KC %d: exits %s (estimate %s), users merged in the two-phase sweeps %s, worst |error| / b %s' % (
        K, nstep_of(K), KC, exits.tolist(), est.tolist(), merged_users, ' '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    # the error budget is used, not vacuous (the constant of test_split_bf16_candidate_scores_stay_inside_the_certified_error)
    assert max(worst.values()) > 1e-3 or K < 16, worst

    # ---- pass level: ids in order and scores against the fp64 brute force
    stats = {}
    ids, sc = scoring.recommend(ops, F, T, topk, True, return_scores=True, stats=stats)
    ids, sc = ops.to_host(ids), ops.to_host(sc)
    assert np.array_equal(ids[chk], want[chk]), (np.flatnonzero((ids != want).any(axis=1) & chk)[:5], stats)
    picked = np.take_along_axis(ref.exact, want, axis=1)
    assert np.allclose(sc[chk], picked[chk], rtol=1e-12, atol=0.0), stats
    # ---- the ids-only pass with one list per user: a single pruned sweep that settles at its exit (the SETTLE twin, KC <= 32)
    took_settle = []
    sweep_entry = ops.score_candidates
    monkeypatch.setattr(ops, 'score_candidates', lambda *a, **kw: (took_settle.append(kw.get('settle') is not None), sweep_entry(*a, **kw))[1])
    monkeypatch.setattr(ops, 'score_splits_override', 1)
    ids_only = ops.to_host(scoring.recommend(ops, F, T, topk, True, order_users=False, batches=1))
    # (rank 256: the image of the approximate fold-in would be 260 columns wide, over its limit of 256 — that pass folds in
    # exactly and nothing settles; the twin's NSTEP 16 instances run at rank 209)
    assert ops.sweep_settles(KC) == (KC <= 32)
    assert took_settle == [KC <= 32 and F.Kx <= 256] and (F.Kx <= 256) == (K < 256), (took_settle, KC, F.Kx)
    assert np.array_equal(ids_only[chk], want[chk]), np.flatnonzero((ids_only != want).any(axis=1) & chk)[:5]


def test_the_users_bounds_are_stored_on_the_routes_no_pass_asks_them_of(hip_ops):
    """`bound_out` with the settle block, and with the two-phase sweep: the arguments are independent in the two entries
    (pk_score_candidates_f32, pk_score_two_phase_f32), but a pass of `scoring.recommend` that settles at the sweep's exit asks for
    no bounds.  Rank 50, KC 16, top-10.  Each route gives what its neighbour without `bound_out` gives — the open users' lists
    bit for bit, the settled users' ids, the flags, the open set — and the stored bounds are those of `ops.pack_frag_bound`.
    The empty user (all scores tie) and the user with 5 unseen items never settle, whatever the scores."""
    ops, K, KC, topk = hip_ops, 50, 16, 10
    d = device_case(ops, host_case(K), K)
    T, F = d['T'], d['F']
    rows = (d['E'], d['w'], EXTRA_SCALE)

    def bounds():
        return torch.full((N_USERS,), -1.0, dtype=torch.float32, device=ops.device)

    def settling_sweep(bound_out):
        q = dict(topk=topk, vmax=F.vmax, item_norm=F.vnorm, out_perm=None, open_count=ops.zero_counters(1),
                 out_idx=torch.full((N_USERS, topk), -7, dtype=torch.int64, device=ops.device),
                 flags=torch.zeros(N_USERS, dtype=torch.int32, device=ops.device),
                 open_list=torch.full((N_USERS,), -1, dtype=torch.int32, device=ops.device))
        out = ops.score_candidates(F.Vp, None, N_USERS, N_ITEMS, K, T.indptr, T.indices, KC, tile_bound=F.tile_bound,
                                   seen_tiles=d['st'], E_rows=rows, bound_out=bound_out, settle=q)
        cs, ci = lists(ops, out, KC)
        open_users = np.sort(ops.to_host(q['open_list'])[:int(ops.to_host(q['open_count'])[0])])
        flags = ops.to_host(q['flags'])
        assert np.array_equal(np.flatnonzero(flags == 0), open_users) and ((flags == 0) | (flags == 8)).all()
        assert EMPTY_USER in open_users and FEW_USER in open_users
        # (a settled user's candidate row is not written: only the open users' rows are compared)
        return cs[0][open_users].view(np.int32), ci[0][open_users], ops.to_host(q['out_idx']), flags

    un = bounds()
    for got, want in zip(settling_sweep(un), settling_sweep(None)):
        assert np.array_equal(got, want)
    assert torch.equal(un, d['ub'])

    def two_phase(bound_out):
        return lists(ops, ops.score_two_phase(F.Vp, None, N_USERS, N_ITEMS, K, T.indptr, KC, HEAD_TILES, 3, None, F.tile_bound,
                                              seen_tiles=d['st'], E_rows=rows, bound_out=bound_out), KC)

    un = bounds()
    assert same_bits(two_phase(un), two_phase(None))
    assert torch.equal(un, d['ub'])

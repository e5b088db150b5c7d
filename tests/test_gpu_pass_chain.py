"""-m gpu: the shortened launch chain of a one-batch scoring pass — the counter reset inside the fold-in's fix-up launch
(csrc/foldq.hip: pk_fold_q20_zero), the exact-row tail as one launch (csrc/rescore.hip: exact_list_kernel) and the lists
written in the caller's row order by the kernels that produce them (`out_perm`), through the C ABI and through
`scoring.recommend`.  Every result is compared with what the longer chain gives: bit for bit where both run on the
device, id for id against NumPy in fp64."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from numpy_ops import NumpyOps
from recorded_calls import given as _given, sweeps as _sweeps
from test_gpu_kernels import rand_csr

pytestmark = pytest.mark.gpu


def item_factors(rng, n, K, decay=0.3):
    return rng.standard_normal((n, K)) * ((np.arange(n) + 1.0) ** -decay)[:, None]


@pytest.mark.parametrize('split', [256, 4096])
def test_fold_in_zeroes_the_counters_in_its_fix_up_launch(hip_ops, split):
    """300 x 2 000, K = 12, a row of 1 500 entries and an empty row: split = 256 cuts the long row into tasks (the fix-up
    kernel sums them and zeroes), split = 4 096 leaves no split row (the fix-up launch is one workgroup that only zeroes)."""
    K = 12
    rng = np.random.RandomState(12)
    n_rows, n_cols = 300, 2000
    indptr, indices, values = rand_csr(rng, n_rows, n_cols, 25, long_rows=[(5, 1500)], empty_rows=[7])
    A = hip_ops.csr(indptr, indices, values, (n_rows, n_cols), split=split)
    assert (A.n_long >= 1) == (split == 256)
    img = hip_ops.q20_encode(hip_ops.to_device(item_factors(np.random.default_rng(K), n_cols, K)))
    assert img is not None
    Kx = -(-(K + 1) // 4) * 4
    want = torch.full((n_rows, Kx), 7.0, dtype=torch.float64, device=hip_ops.device)
    hip_ops.fold_q20(A, img, K, want)
    got = torch.full((n_rows, Kx), 7.0, dtype=torch.float64, device=hip_ops.device)
    counters = torch.full((5,), 7, dtype=torch.int32, device=hip_ops.device)
    hip_ops.fold_q20(A, img, K, got, counters=counters[:4])
    assert np.array_equal(hip_ops.to_host(got).view(np.int64), hip_ops.to_host(want).view(np.int64))
    assert (hip_ops.to_host(got)[7] == 0).all()
    assert hip_ops.to_host(counters).tolist() == [0, 0, 0, 0, 7]                 # exactly the words asked for
    fresh = hip_ops.fold_q20_zero(A, img, K, got, 3)
    assert fresh.dtype == torch.int32 and hip_ops.to_host(fresh).tolist() == [0, 0, 0]


@functools.lru_cache(maxsize=None)
def exact_case():
    """2 500 items (three chunks of 1 024, the last ragged), K = 8, twelve users with seen lists; the NumPy lists in fp64
    (class — unseen first —, score descending, index ascending).  Adjacent scores of every list, the first one left out
    included, are further apart than 1e-9 (asserted here, on the CPU): summation order cannot change an id."""
    n_items, K, topk, n_users = 2500, 8, 5, 12
    rng = np.random.RandomState(2500)
    V, E = rng.randn(n_items, K), rng.randn(n_users, K)
    seen = [np.sort(rng.choice(n_items, rng.randint(0, 300), replace=False)) for _ in range(n_users)]
    seen[4] = np.sort(rng.choice(n_items, n_items - 3, replace=False))      # fewer than topk unseen: seen items re-enter
    seen_ptr = np.r_[0, np.cumsum([len(x) for x in seen])].astype(np.int64)
    seen_idx = np.concatenate(seen).astype(np.int32)
    s = E @ V.T
    want = np.empty((n_users, topk), dtype=np.int64)
    for u in range(n_users):
        cls = np.zeros(n_items, dtype=np.int64)
        cls[seen[u]] = 1
        order = np.lexsort((np.arange(n_items), -s[u], cls))
        want[u] = order[:topk]
        head = order[:topk + 1]
        same_class = cls[head][:-1] == cls[head][1:]
        assert (np.abs(np.diff(s[u, head]))[same_class] > 1e-9).all()
    return V, E, seen_ptr, seen_idx, want, s


def test_exact_tail_is_one_launch_with_self_resetting_tickets(hip_ops):
    V, E, seen_ptr, seen_idx, want, s = exact_case()
    n_items, topk, n_users, n_wg = V.shape[0], want.shape[1], E.shape[0], 4
    ops = hip_ops
    Vd, Ed = ops.to_device(V), ops.to_device(E)
    sp, si = torch.from_numpy(seen_ptr).to(Vd.device), torch.from_numpy(seen_idx).to(Vd.device)
    users = np.random.RandomState(1).permutation(n_users).astype(np.int32)
    lst = torch.from_numpy(users).to(Vd.device)

    def run(count, out_perm=None):
        out_i = torch.full((n_users, topk), -7, dtype=torch.int64, device=Vd.device)
        out_s = torch.full((n_users, topk), -7.0, dtype=torch.float64, device=Vd.device)
        cnt = torch.tensor([count], dtype=torch.int32, device=Vd.device)
        kw = {} if out_perm is None else {'out_perm': out_perm}
        ops.score_exact_list(lst, cnt, Vd, Ed, n_items, sp, si, topk, out_i, out_s, n_wg=n_wg, **kw)
        return out_i, out_s

    def check(out_i, out_s, count, rows=None):
        got_i, got_s = ops.to_host(out_i), ops.to_host(out_s)
        done, rest = users[:count], users[count:]
        at = done if rows is None else rows[done]
        assert np.array_equal(got_i[at], want[done]), count
        assert np.allclose(got_s[done], np.take_along_axis(s[done], want[done], 1), rtol=1e-12, atol=1e-12)
        untouched = np.setdiff1d(np.arange(n_users), at)
        assert (got_i[untouched] == -7).all() and (got_s[rest] == -7.0).all()

    check(*run(0), 0)                                   # an empty list (the normal case of a pass): nothing is written
    for count in (3, 9, 3):                             # within the row slots; beyond them; and again on the same buffer
        first = run(count)
        second = run(count)                             # twice in a row: the tickets went back to zero by themselves
        check(*first, count)
        check(*second, count)
        assert torch.equal(first[0], second[0]) and torch.equal(first[1].view(torch.int64), second[1].view(torch.int64))
    # ids to permuted rows, scores where they were
    perm = np.random.RandomState(2).permutation(n_users).astype(np.int64)
    check(*run(9, torch.from_numpy(perm).to(Vd.device)), 9, rows=perm)
    # two streams, each with a work buffer of its own, in flight together
    main = torch.cuda.current_stream()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    res = []
    for st in streams:
        st.wait_stream(main)
    for rep in range(2):
        for st, count in zip(streams, (9, 3)):
            with torch.cuda.stream(st):
                res.append((run(count), count))
    torch.cuda.synchronize()
    for (out_i, out_s), count in res:
        check(out_i, out_s, count)


def _pass_case(n_users, n_items, rank, mean, long_rows):
    rng = np.random.RandomState(n_items)
    indptr, indices, values = rand_csr(rng, n_users, n_items, mean, long_rows=long_rows, empty_rows=[11])
    V = item_factors(np.random.default_rng(n_items), n_items, rank)
    return indptr, indices, values, V


@functools.lru_cache(maxsize=None)
def pass_case(name):
    """the workload of a pass test and the CPU double's lists for it, computed once"""
    from polara_amd import scoring
    if name == 'pruned':
        # 8 229 users: above ORDER_USERS_MIN, no multiple of 32; some long rows so that activity order differs from row order
        n_users, n_items, rank = 8229, 1500, 12
        case = _pass_case(n_users, n_items, rank, 20, [(r, 300 + r % 200) for r in range(3, n_users, 97)])
    else:
        # 48 items, top-10: users who have seen 40 items or more cannot fill their list with unseen ones -> exact tail;
        # 331 of them, more than the tail's 128 row slots
        n_users, n_items, rank = 8229, 48, 12
        case = _pass_case(n_users, n_items, rank, 8, [(r, 40 + r % 9) for r in range(5, n_users, 25)])
    indptr, indices, values, V = case
    cpu = NumpyOps()
    ref = cpu.to_host(scoring.recommend(cpu, scoring.FactorImage(cpu, cpu.to_device(V)),
                                        cpu.csr(indptr, indices, values, (n_users, n_items)), 10, True))
    return indptr, indices, values, V, (n_users, n_items), np.asarray(ref)


@pytest.mark.parametrize('name', ['pruned', 'exact_tail'])
def test_lists_written_in_the_callers_order_by_their_producers(hip_ops, name):
    from polara_amd import scoring
    indptr, indices, values, V, shape, ref = pass_case(name)
    ops, topk = hip_ops, 10
    assert shape[0] >= scoring.ORDER_USERS_MIN and shape[0] % 32 != 0
    T = ops.csr(indptr, indices, values, shape)
    F = scoring.FactorImage(ops, ops.to_device(V))
    st = {}
    got = ops.to_host(scoring.recommend(ops, F, T, topk, True, stats=st))                 # producers write row perm[u]
    if name == 'exact_tail':
        assert st['flagged_users'] > 128
    plain = ops.to_host(scoring.recommend(ops, F, T, topk, True, order_users=False))     # users swept in the caller's order
    dest = torch.full((shape[0], topk), -5, dtype=torch.int64, device=ops.device)
    assert scoring.recommend(ops, F, T, topk, True, out=dest) is dest                     # the scatter route
    assert np.array_equal(got, plain)
    assert np.array_equal(got, ops.to_host(dest))
    assert np.array_equal(got, ref)
    assert np.array_equal(got, ops.to_host(scoring.recommend(ops, F, T, topk, True)))    # and again (tickets, counters)


def test_one_batch_pass_issues_neither_a_counter_reset_nor_a_scatter(hip_ops, pk_options):
    from polara_amd import scoring
    indptr, indices, values, V, shape, ref = pass_case('pruned')
    ops, topk = hip_ops, 10
    T = ops.csr(indptr, indices, values, shape)
    F = scoring.FactorImage(ops, ops.to_device(V))
    assert F.Q20 is not None
    scoring.recommend(ops, F, T, topk, True)               # per-stream scratch exists afterwards

    def recorded(**kw):
        rec = scoring._CallRecorder(ops.lib)
        ops.lib = rec
        try:
            out = scoring.recommend(ops, F, T, topk, True, **kw)
        finally:
            ops.lib = rec.lib
        names = [name for name, _, _ in rec.calls]
        # the producers of the lists: the re-scorings (rows_dev, out_perm_dev, user_norm_dev: arguments 2, 30 and 31 of 32)
        # and the exact tail (out_perm_dev: the last of 17)
        rescorings = [args for name, _, args in rec.calls if name == 'pk_rescore_f64']
        tails = [args for name, _, args in rec.calls if name == 'pk_score_exact_list_f64']
        assert all(len(a) == 32 for a in rescorings) and all(len(a) == 17 for a in tails)
        return names, ops.to_host(out), rescorings, tails, _sweeps(rec.calls)      # (the sweeps: argument counts checked there)

    names, out, rescorings, tails, swept = recorded()
    assert 'pk_zero_i32' not in names and 'pk_scatter_rows_i64' not in names and 'pk_exact_work_init' not in names, names
    assert 'pk_fold_q20_zero' in names and 'pk_fold_q20' not in names
    # two re-scorings and the exact tail, all three writing through out_perm: no scatter follows
    assert names.count('pk_rescore_f64') == 2 and names[-1] == 'pk_score_exact_list_f64' and len(tails) == 1, names
    assert all(_given(a[30]) for a in rescorings) and _given(tails[0][16])
    # this pass settles where its groups leave the sweep: the first re-scoring takes the open list and no norm bounds
    assert len(swept) == 1 and swept[0]['entry'] == 'pk_score_candidates_f32' and swept[0]['settle'], swept
    assert _given(rescorings[0][2]) and not _given(rescorings[0][31]) and not _given(rescorings[1][31])
    assert np.array_equal(out, ref)
    # ... and with the sweep's exit rule off the first re-scoring settles: everybody, with the bounds the sweep left, as
    # arguments of the same call that writes through out_perm
    pk_options('sweep_settle', 0)
    names, out, rescorings, tails, swept = recorded()
    pk_options('sweep_settle', 1)
    assert len(swept) == 1 and swept[0]['entry'] == 'pk_score_candidates_f32', swept
    assert not swept[0]['settle'] and swept[0]['user_bound_out'] and 'pk_scatter_rows_i64' not in names, (swept, names)
    assert names.count('pk_rescore_f64') == 2 and names[-1] == 'pk_score_exact_list_f64'
    assert all(_given(a[30]) for a in rescorings) and _given(tails[0][16])
    assert not _given(rescorings[0][2]) and _given(rescorings[0][31]) and not _given(rescorings[1][31])
    assert np.array_equal(out, ref)
    dest = torch.empty((shape[0], topk), dtype=torch.int64, device=ops.device)
    names, out, rescorings, tails, swept = recorded(out=dest)
    assert names[-1] == 'pk_scatter_rows_i64' and 'pk_zero_i32' not in names, names
    assert len(rescorings) == 2 and not any(_given(a[30]) for a in rescorings) and not _given(tails[0][16])
    assert np.array_equal(out, ref)
    # a batched pass keeps the separate reset (its streams fork behind it) and the scatter
    names, out, rescorings, tails, swept = recorded(batches=2)
    assert 'pk_zero_i32' in names and names[-1] == 'pk_scatter_rows_i64', names
    assert rescorings and not any(_given(a[30]) for a in rescorings) and not _given(tails[0][16])
    assert np.array_equal(out, ref)

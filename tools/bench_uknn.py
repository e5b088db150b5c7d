"""UserKNN on the synthetic workloads of the sibling tools (synth.make_workload) at the model's default settings (cosine,
100 neighbours), topk 10, every user a test user.  Writes ONE JSON line (`--out`, default profiles/uknn_bench_line.json)
and prints it; every figure is the median of `--reps` (default 5) timed repetitions after one untimed one, with (min, max):
  ml20m.userknn:    the neighbour pass (pk_spsp_knn_f64 over all 138 493 users), the whole build, the entries of N, and a
                    full scoring pass over all users (seconds, users per second);
  ml20m.itemknn:    the ItemKNN build with gram = 'image' and gram = 'sparse' (stages and whole build), and whether both
                    kept the same entries;
  ml20m.composed:   the composition cannot run at this shape (its intermediate is the sparse Gram matrix of the users);
                    the entries its count pass finds (pk_spgemm_count) when that step fits, else "not measured";
  ml1m.neighbours:  in ONE loop that alternates the two — the fused pass, and its COMPOSITION from spgemm_csr (X X^T as a
                    CSR), torch element-wise passes (norm products, shrinkage, quotient, the candidate rule) and a
                    per-row top-K (pk_topk_rows_f64 over the scattered rows, then a gather) — with seconds and the peak
                    device memory above what was allocated before the call, and whether both kept the same entries.
A leg that was not run reads "not measured" (`--skip` takes a comma-separated list of legs).  Single process: a failure ends
the tool with a non-zero status and nothing else is started on the device."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOPK, K = 10, 100
NOT_MEASURED = 'not measured'


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _stat(values, digits=5):
    s = sorted(values)
    return dict(median=round(s[len(s) // 2], digits), min=round(s[0], digits), max=round(s[-1], digits), n=len(s))


def _timed(ops, fn):
    ops.synchronize()
    t0 = time.perf_counter()
    out = fn()
    ops.synchronize()
    return time.perf_counter() - t0, out


def _say(*what):
    print(*what, file=sys.stderr, flush=True)


def _data(workload):
    import numpy as np
    from polara_amd.data import ArrayData
    from polara_amd.synth import make_workload, csr_to_coo_triplets
    csr, _ = make_workload(workload, device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    hold = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    return ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False), (u, i, v), n_users, n_items


def _userknn_leg(data, ops, reps, n_users):
    from polara_amd import UserKNNModel
    m = UserKNNModel(data, ops=ops)
    m.verbose, m.topk = False, TOPK
    stages = {k: [] for k in ('upload_s', 'neighbours_s', 'build_s')}
    for rep in range(reps + 1):                                # the first build pays allocations and code loads
        m.build()
        _say('userknn build', rep, m.build_stats)
        if rep:
            for k in ('upload_s', 'neighbours_s'):
                stages[k].append(m.build_stats[k])
            stages['build_s'].append(m.training_time[-1])
    passes = []
    for rep in range(reps + 1):
        t, recs = _timed(ops, m.get_recommendations)
        m._recommendations = None
        _say('userknn scoring pass', rep, round(t, 4))
        if rep:
            passes.append(t)
    out = {k: _stat(v) for k, v in stages.items()}
    out.update(nnz_weights=int(m.build_stats['nnz']), neighbours=m.neighbours,
               score=dict(topk=TOPK, dense_output=m.dense_output, pass_s=_stat(passes),
                          users_per_s=round(n_users / _stat(passes)['median'], 1), pads=int((recs < 0).sum())))
    return out


def _itemknn_leg(data, ops, reps):
    import torch
    from polara_amd import ItemKNNModel
    out, kept = {}, {}
    for gram in ('image', 'sparse'):
        m = ItemKNNModel(data, ops=ops)
        m.verbose, m.gram = False, gram
        stages = {k: [] for k in ('gram_s', 'prune_s', 'transpose_s', 'build_s')}
        for rep in range(reps + 1):
            m.build()
            _say('itemknn', gram, rep, m.build_stats)
            if rep:
                for k in ('gram_s', 'prune_s', 'transpose_s'):
                    stages[k].append(m.build_stats[k])
                stages['build_s'].append(m.training_time[-1])
        out[gram] = dict({k: _stat(v) for k, v in stages.items()}, nnz_weights=int(m.build_stats['nnz']),
                         image_bytes=int(m.build_stats['image_bytes']))
        kept[gram] = (m.item_weights.indptr.clone(), m.item_weights.indices.clone())
        del m
    out['same_entries'] = bool(all(torch.equal(a, b) for a, b in zip(kept['image'], kept['sparse'])))
    return out


def _count_leg(ops, X, Xt):
    """The entries of X X^T by the count pass of the composition alone (its fill would need 12 bytes for each)."""
    import torch
    from polara_amd.ops import _ptr
    n = int(X.shape[0])
    try:
        indptr = torch.empty(n + 1, dtype=torch.int64, device=ops.device)
        work = ops._work(ops.lib.pk_spgemm_work_bytes(n, n))
        t, rc = _timed(ops, lambda: ops.lib.pk_spgemm_count(ops.stream(), n, int(X.shape[1]), n, _ptr(X.indptr), _ptr(X.indices),
                                                           _ptr(X.values), X.val_kind, _ptr(Xt.indptr), _ptr(Xt.indices),
                                                           _ptr(ops._spsp_values(Xt)), 0, 0, _ptr(indptr), _ptr(work)))
    except (MemoryError, RuntimeError) as e:                   # the scratch of the count pass does not fit
        return dict(count_nnz=NOT_MEASURED, reason=str(e)[:120])
    if rc != 0:
        raise RuntimeError('pk_spgemm_count failed: %d' % rc)
    nnz = int(indptr[-1].item())
    return dict(count_nnz=nnz, count_s=round(t, 5), csr_bytes=nnz * 12 + (n + 1) * 8)


def _composed(ops, X, Xt, row, col, shrink, K):
    """The same selection from what the package had before the fused pass: the sparse Gram matrix as a CSR, element-wise
    torch over its entries, the rows scattered into a dense block, pk_topk_rows_f64, a gather."""
    import torch
    n = int(X.shape[0])
    G = ops.spgemm_csr(X, Xt)
    rows = torch.repeat_interleave(torch.arange(n, device=ops.device), G.indptr[1:] - G.indptr[:-1])
    cols = G.indices.long()
    w = G.values / (row[rows] * col[cols] + shrink)
    cand = (G.values != 0) & torch.isfinite(w) & (w != 0) & (rows != cols)
    dense = torch.full((n, n), float('-inf'), dtype=torch.float64, device=ops.device)
    dense[rows[cand], cols[cand]] = w[cand]
    idx = ops.topk_rows(dense, K)
    return idx, torch.gather(dense, 1, idx)


def _neighbours_leg(ops, triplet, n_users, n_items, reps):
    import numpy as np
    import torch
    from polara_amd import knn
    u, i, v = triplet
    X = ops.csr_from_coo(u, i, v, (n_users, n_items))
    Xt = ops.csr_transpose(X)
    vals = ops.csr_values_host(X)
    q = knn.squared_sums(np.repeat(np.arange(n_users), np.diff(ops.to_host(X.indptr))), vals, n_users)
    row_h, col_h = knn.cosine_vectors(q, 0.5)
    row, col = ops.to_device(row_h), ops.to_device(col_h)
    exclude = torch.arange(n_users, dtype=torch.int32, device=ops.device)
    fused, composed, peak, same = [], [], {'fused': 0, 'composed': 0}, None
    for rep in range(reps + 1):
        for name, fn, times in (('fused', lambda: ops.spsp_knn_slots(X, Xt, knn.KINDS['cosine'], row, col, 0.0, K, False, exclude), fused),
                                ('composed', lambda: _composed(ops, X, Xt, row, col, 0.0, K), composed)):
            ops.synchronize()
            torch.cuda.reset_peak_memory_stats(ops.device)
            base = torch.cuda.memory_allocated(ops.device)
            t, out = _timed(ops, fn)
            peak[name] = max(peak[name], int(torch.cuda.max_memory_allocated(ops.device) - base))
            _say('neighbours', name, rep, round(t, 4))
            if rep:
                times.append(t)
            if name == 'fused':
                kept_fused = out[1]
            elif same is None:                                 # once: the kept columns of every row, as sets
                idx, val = out
                a = torch.sort(torch.where(torch.isinf(val), torch.full_like(idx, -1), idx), 1).values
                b = torch.sort(kept_fused.long(), 1).values
                same = bool(torch.equal(a, b))
            del out
    return dict(n_users=n_users, nnz=int(len(v)), neighbours=K, fused_s=_stat(fused), composed_s=_stat(composed),
                fused_peak_bytes=peak['fused'], composed_peak_bytes=peak['composed'], same_selection=same)


def main():
    from polara_amd.ops import HipOps
    reps = _arg('--reps', 5)
    skip = set(filter(None, _arg('--skip', '').split(',')))
    out_path = _arg('--out', os.path.join(ROOT, 'profiles', 'uknn_bench_line.json'))
    ops = HipOps('cuda:0')
    out = dict(reps=reps, neighbours=K)
    data, triplet, n_users, n_items = _data('ml1m')
    out['ml1m'] = dict(n_users=n_users, n_items=n_items, nnz=int(len(triplet[2])),
                       neighbours=NOT_MEASURED if 'neighbours' in skip else _neighbours_leg(ops, triplet, n_users, n_items, reps))
    del data, triplet
    data, (u, i, v), n_users, n_items = _data('ml20m')
    big = dict(n_users=n_users, n_items=n_items, nnz=int(len(v)))
    big['userknn'] = NOT_MEASURED if 'userknn' in skip else _userknn_leg(data, ops, reps, n_users)
    big['itemknn'] = NOT_MEASURED if 'itemknn' in skip else _itemknn_leg(data, ops, reps)
    if 'count' in skip:
        big['composed'] = dict(count_nnz=NOT_MEASURED)
    else:
        X = ops.csr_from_coo(u, i, v, (n_users, n_items))
        big['composed'] = _count_leg(ops, X, ops.csr_transpose(X))
    out['ml20m'] = big
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(line + '\n')
    print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

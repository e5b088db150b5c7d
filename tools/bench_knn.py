"""ItemKNN and RP3beta on the ML-20M-shaped workload of the sibling tools (synth.make_workload: 138 493 x 26 744 with
2.0e7 ratings; `--workload ml1m` for the small one) at the models' default settings (100 neighbours), topk 10, every user
a test user (its training row as known items).  Writes ONE JSON line (`--out`, default profiles/knn_bench_line.json) and
prints it; every figure is the median of `--reps` (default 5) timed repetitions after one untimed one, with (min, max):
  itemknn, rp3beta:  the stages of the build (gram, prune, transpose: seconds, synchronised after each), the whole build,
                     the entries of W, and a full scoring pass over all users (seconds, users per second);
  prune:             on the cosine image of the workload, in ONE loop that alternates the two: the fused pass
                     (pk_knn_prune_f64) and the COMPOSED alternative — torch element-wise normalisation of the whole image
                     (outer product of the norms, shrinkage, quotient, the non-candidates set to -inf), pk_topk_rows_f64, a
                     gather of the kept values — with seconds and the peak device memory above what was allocated before
                     the call, for both; and whether both kept the same entries.
Single process: a failure ends the tool with a non-zero status and nothing else is started on the device."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOPK = 10


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


def _model_leg(cls, data, ops, reps, n_users):
    m = cls(data, ops=ops)
    m.verbose, m.topk = False, TOPK
    stages = {k: [] for k in ('gram_s', 'prune_s', 'transpose_s', 'build_s')}
    for rep in range(reps + 1):                                # the first build pays allocations and code loads
        m.build()
        if rep:
            for k in ('gram_s', 'prune_s', 'transpose_s'):
                stages[k].append(m.build_stats[k])
            stages['build_s'].append(m.training_time[-1])
    passes = []
    for rep in range(reps + 1):
        t, recs = _timed(ops, m.get_recommendations)
        m._recommendations = None
        if rep:
            passes.append(t)
    out = {k: _stat(v) for k, v in stages.items()}
    out.update(nnz_weights=int(m.build_stats['nnz']), neighbours=m.neighbours, image_bytes=m.build_stats['image_bytes'],
               score=dict(topk=TOPK, dense_output=m.dense_output, pass_s=_stat(passes),
                          users_per_s=round(n_users / _stat(passes)['median'], 1), pads=int((recs < 0).sum())))
    return out


def _composed(ops, G, n, row, col, shrink, K):
    """The same selection from what the package had before the fused pass: element-wise torch over the whole image, then
    pk_topk_rows_f64 (index output), then a gather."""
    import torch
    g = G[:, :n]
    w = g / (row[:, None] * col[None, :] + shrink)
    cand = (g != 0) & torch.isfinite(w) & (w != 0)
    cand.fill_diagonal_(False)
    w = torch.where(cand, w, torch.full((), float('-inf'), dtype=w.dtype, device=w.device))
    idx = ops.topk_rows(w, K)
    val = torch.gather(w, 1, idx)
    return idx, val


def _prune_leg(A, ops, reps, K):
    import torch
    from polara_amd import knn
    n = int(A.shape[1])
    G = ops.knn_gram(A)
    q = ops.to_host(G.diagonal()[:n])
    row_h, col_h = knn.cosine_vectors(q, 0.5)
    row, col = ops.to_device(row_h), ops.to_device(col_h)
    fused, composed, peak = [], [], {'fused': 0, 'composed': 0}
    same = None
    for rep in range(reps + 1):
        for name, fn, times in (('fused', lambda: ops.knn_prune_slots(G, n, knn.KINDS['cosine'], row, col, 0.0, K, False), fused),
                                ('composed', lambda: _composed(ops, G, n, row, col, 0.0, K), composed)):
            ops.synchronize()
            torch.cuda.reset_peak_memory_stats(ops.device)
            base = torch.cuda.memory_allocated(ops.device)
            t, out = _timed(ops, fn)
            peak[name] = max(peak[name], int(torch.cuda.max_memory_allocated(ops.device) - base))
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
    return dict(n_items=n, neighbours=K, image_bytes=int(G.numel() * 8), fused_s=_stat(fused), composed_s=_stat(composed),
                fused_peak_bytes=peak['fused'], composed_peak_bytes=peak['composed'], same_selection=same,
                image_read_GBps=round(G.numel() * 8 / _stat(fused)['median'] / 1e9, 1))


def main():
    import numpy as np
    from polara_amd import ItemKNNModel, RP3BetaModel
    from polara_amd.data import ArrayData
    from polara_amd.ops import HipOps
    from polara_amd.synth import make_workload, csr_to_coo_triplets
    workload, reps = _arg('--workload', 'ml20m'), _arg('--reps', 5)
    out_path = _arg('--out', os.path.join(ROOT, 'profiles', 'knn_bench_line.json'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload(workload, device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    hold = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False)
    out = dict(workload=workload, n_users=n_users, n_items=n_items, nnz=int(len(v)), reps=reps)
    out['itemknn'] = _model_leg(ItemKNNModel, data, ops, reps, n_users)
    out['rp3beta'] = _model_leg(RP3BetaModel, data, ops, reps, n_users)
    out['prune'] = _prune_leg(ops.csr_from_coo(u, i, v, (n_users, n_items)), ops, reps, 100)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(line + '\n')
    print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

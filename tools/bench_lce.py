"""Local Collective Embeddings on the ML-20M-shaped planted matrix of tools/bench_coldstart.py (138 493 x 26 744, 2.0e7
ratings, 3 000 binary labels, ~8 per item): LCE on all items and LCE(cs) with 20 % of the items cold, ranks 10 and 50, top-10.
Prints ONE JSON line per rank:
  graph:    seconds of the host kNN graph (scikit-learn, the reference's call) — once per item set, reused by the builds;
  solver:   seconds per build (16 passes, default parameters) and per pass, library calls per pass;
  update:   the fused update (pk_lce_update_f64) against its composed form (pk_axpbypcz_f64 + pk_tsmm_f64 +
            pk_lce_update_ew_f64) on blocks of the shape of each factor, microseconds per call (mean of a queued batch);
  standard: median seconds of the scoring pass of LCE (all users, seen items filtered, lists copied to the host);
  coldstart: median seconds of the LCE(cs) pass (cold items as queries, users as the catalogue) and of its queries alone;
  numpy:    seconds per pass of the NumPy/SciPy restatement of the solver (tests/lce_reference.py) on this machine.
`--ranks 10,50`, `--no-cold`, `--numpy-passes N` (default 2; 0 = skip).  Timings are synchronised; nothing here is part of
bench.py."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_coldstart import count_launches, item_features, median_of, timed
from polara_amd import lce
from polara_amd.data import ArrayData, ItemColdStartArrayData
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets


def queued(ops, fn, reps=20):
    """mean seconds of `reps` calls queued back to back (launch gaps hidden behind the previous kernel)"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def update_forms(ops, shapes, k):
    """fused against composed on random blocks [m x k] for every factor's m"""
    out = {}
    rng = np.random.default_rng(k)
    B = rng.random((k + 4, k))
    M = ops.to_device(B.T @ B)
    for name, m in shapes.items():
        X, N = ops.to_device(rng.random((m, k))), ops.to_device(rng.random((m, k)))
        c = ops.to_device(rng.random(m))
        row = {}
        for form, fused in (('fused_us', True), ('composed_us', False)):
            if fused and k > ops.lce_fused_max_rank():
                continue
            row[form] = round(1e6 * queued(ops, lambda: ops.lce_update(X, N, M, ma=0.9, a=0.9, lamb=1.0, c=c, fused=fused)), 2)
        row['bytes_moved_min'] = 3 * 8 * m * k
        if 'fused_us' in row:
            row['fused_gb_per_s'] = round(row['bytes_moved_min'] / row['fused_us'] / 1e3, 1)
            row['speedup'] = round(row['composed_us'] / row['fused_us'], 2)
        out[name] = row
    return out


def numpy_pass_seconds(Xs, Xu, A, k, passes):
    import lce_reference as ref
    init = lce.initial_factors(Xs.shape[0], Xs.shape[1], Xu.shape[1], k, seed=0)
    t0 = time.perf_counter()
    hist = ref.solve(Xs, Xu, A, *init, maxiter=passes - 1, epsilon=0.0)[3]
    return (time.perf_counter() - t0) / len(hist), len(hist)


def run(ops, rank, topk, u, i, v, n_users, n_items, F, graphs, cold, numpy_passes):
    out = dict(rank=rank, topk=topk, n_users=n_users, n_items=n_items, n_labels=int(F.shape[1]))
    every_user = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    m = lce.LCEModel(ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=every_user), item_features=F, ops=ops)
    m.verbose, m.rank, m.topk, m.seed = False, rank, topk, 0
    if 'all' not in graphs:
        graphs['all'] = (m._item_graph(m.encode_item_features()), m.graph_time[-1])
    m.item_graph = graphs['all'][0]
    out['graph'] = dict(seconds=round(graphs['all'][1], 3), nnz=int(graphs['all'][0].nnz))
    m.build()
    _, t_build = timed(m.build)
    passes = m.build_stats['passes']
    Xs, train = m.encode_item_features(), m._training_device_csr()
    stats = {}
    args = (ops, Xs, train.T, graphs['all'][0], rank)
    _, t_solve = timed(lambda: lce.local_collective_embeddings(*args, seed=0, stats=stats))
    n1, _ = count_launches(ops, lambda: lce.local_collective_embeddings(*args, seed=0, maxiter=1, epsilon=0.0))
    n2, names = count_launches(ops, lambda: lce.local_collective_embeddings(*args, seed=0, maxiter=2, epsilon=0.0))
    out['solver'] = dict(build_seconds=round(t_build, 4), solve_seconds=round(t_solve, 4), passes=passes,
                         seconds_per_pass=round(t_solve / stats['passes'], 5), library_calls_per_pass=n2 - n1, entry_points=names)
    out['update'] = update_forms(ops, dict(HsT=int(Xs.shape[1]), HuT=n_users, W=n_items), rank)
    m.get_recommendations()
    launches, _ = count_launches(ops, m.get_recommendations)
    out['standard'] = dict(seconds=round(median_of(m.get_recommendations, 15), 6), launches=launches)
    if numpy_passes:
        import scipy.sparse as sps
        Xu = sps.csr_matrix((v, (i, u)), shape=(n_items, n_users))
        per, n = numpy_pass_seconds(Xs, Xu, graphs['all'][0], rank, numpy_passes)
        out['numpy'] = dict(seconds_per_pass=round(per, 3), passes_timed=n,
                            speedup_per_pass=round(per / out['solver']['seconds_per_pass'], 1))
        del Xu
    del m
    torch.cuda.empty_cache()
    if cold:
        cold_items = np.random.RandomState(0).permutation(n_items)[:n_items // 5]
        is_cold = np.zeros(n_items, dtype=bool)
        is_cold[cold_items] = True
        train_ids = np.flatnonzero(~is_cold)
        new_train = np.full(n_items, -1, np.int64)
        new_train[train_ids] = np.arange(len(train_ids))
        new_cold = np.full(n_items, -1, np.int64)
        new_cold[np.sort(cold_items)] = np.arange(len(cold_items))
        tr = ~is_cold[i]
        data = ItemColdStartArrayData((u[tr], new_train[i[tr]], v[tr]), (u[~tr], new_cold[i[~tr]], v[~tr]), F[train_ids].tocsr(),
                                      F[np.sort(cold_items)].tocsr(), n_users=n_users, n_items=len(train_ids))
        mc = lce.LCEModelItemColdStart(data, ops=ops)
        mc.verbose, mc.rank, mc.topk, mc.seed = False, rank, topk, 0
        if 'train' not in graphs:
            graphs['train'] = (mc._item_graph(mc.encode_item_features()), mc.graph_time[-1])
        mc.item_graph = graphs['train'][0]
        mc.build()
        _, t_build = timed(mc.build)
        mc.collect_recommend_stats = True
        mc.get_recommendations()
        st = dict(mc.recommend_stats)
        mc.collect_recommend_stats = False
        mc.get_recommendations()
        t_pass = median_of(mc.get_recommendations, 15)
        launches, _ = count_launches(ops, mc.get_recommendations)
        out['coldstart'] = dict(n_cold=int(data.n_cold_items), graph_seconds=round(graphs['train'][1], 3), build_seconds=round(t_build, 4),
                                seconds=round(t_pass, 6), cold_items_per_s=round(data.n_cold_items / t_pass, 1),
                                tiles_scored_share=round(st['tiles_scored'] / max(1, st['tiles_total']), 4),
                                flagged=int(st['flagged_users']), launches=launches,
                                queries_seconds=round(median_of(mc._cold_queries_device, 30), 7))
        del mc
        torch.cuda.empty_cache()
    return out


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    ranks = [int(x) for x in opt('--ranks', '10,50').split(',')]
    numpy_passes = int(opt('--numpy-passes', '2'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    F = item_features(n_items)
    graphs = {}
    for rank in ranks:
        print(json.dumps(run(ops, rank, 10, u, i, v, n_users, n_items, F, graphs, '--no-cold' not in argv, numpy_passes)), flush=True)


if __name__ == '__main__':
    main()

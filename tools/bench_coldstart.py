"""Item cold start on the ML-20M-shaped workload (synth.make_workload('ml20m'): 138 493 x 26 744, 2.0e7 ratings): 20 % of the
items made cold by a seeded permutation (the reference's split, coldstart/data.py:18-21, 56-64), synthetic binary item
features (3 000 labels, ~8 per item, popularity-skewed), rank 50, top-10, PureSVD(cs) and — with --hybrid — HybridSVD(cs).
Prints ONE JSON line per model:
  build:   seconds of the whole build, and the extra over the parent model's build (users' image, W, G);
  pass:    median seconds of >= 20 passes with the lists copied to the host, cold items / s, (cold item x user) pairs / s,
           share of the sweep's tiles scored, flagged queries, launches of a pass (library calls on the stream);
  queries: seconds of the pass's front end alone, E = (F_cold W) G (SpMM + small product), median of 50;
  cpu (with --cpu): seconds of the NumPy restatement of the same pass on this machine and the rows whose lists differ.
--device-similarity builds S with polara_amd.similarity on the device instead of SciPy (the default).
Timings are synchronised; nothing here is part of bench.py."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import scipy.sparse as sps
import torch

from polara_amd import scoring
from polara_amd.coldstart import HybridSVDItemColdStart, SVDModelItemColdStart
from polara_amd.data import ArrayData, ItemColdStartArrayData, ItemColdStartSimilarityArrayData, SimilarityArrayData
from polara_amd.models import HybridSVD, SVDModel
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def median_of(fn, n):
    return float(np.median([timed(fn)[1] for _ in range(n)]))


def item_features(n_items, n_labels=3000, per_item=8, seed=7):
    """binary features, label popularity ~ 1 / rank^0.8"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_labels + 1) ** 0.8
    p /= p.sum()
    counts = np.maximum(1, rng.poisson(per_item, n_items))
    rows = np.repeat(np.arange(n_items), counts)
    cols = rng.choice(n_labels, size=len(rows), p=p)
    F = sps.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_items, n_labels))
    F.sum_duplicates()
    F.data[:] = 1.0
    return F


def cosine(F, ops=None):
    """S by SciPy on the host (the default: earlier numbers stay comparable) or, given `ops` (--device-similarity), by
    polara_amd.similarity.cosine_similarity on the device."""
    if ops is not None:
        from polara_amd.similarity import cosine_similarity
        return cosine_similarity(F, ops=ops)
    Fn = sps.diags(1.0 / np.sqrt(np.asarray(F.sum(1)).ravel())) @ F
    S = (Fn @ Fn.T).tocsr()
    S.setdiag(1.0)
    S.sum_duplicates()
    return S


def count_launches(ops, fn):
    rec = scoring._CallRecorder(ops.lib)
    ops.lib = rec
    try:
        fn()
    finally:
        ops.lib = rec.lib
    names = [n for n, f, a in rec.calls if getattr(f, 'restype', None) is not None and a and hasattr(a[0], 'value')]
    return len(names), sorted(set(names))


def run(ops, hybrid, u, i, v, n_users, n_items, F, rank, topk, cpu):
    cold_items = np.random.RandomState(0).permutation(n_items)[:n_items // 5]
    is_cold = np.zeros(n_items, dtype=bool)
    is_cold[cold_items] = True
    train_ids = np.flatnonzero(~is_cold)
    new_train = np.full(n_items, -1, np.int64)
    new_train[train_ids] = np.arange(len(train_ids))
    new_cold = np.full(n_items, -1, np.int64)
    new_cold[np.sort(cold_items)] = np.arange(len(cold_items))
    tr = ~is_cold[i]
    training = (u[tr], new_train[i[tr]], v[tr])
    holdout = (u[~tr], new_cold[i[~tr]], v[~tr])
    Ft, Fc = F[train_ids].tocsr(), F[np.sort(cold_items)].tocsr()
    kw = dict(n_users=n_users, n_items=len(train_ids))
    if hybrid:
        S = cosine(Ft, ops if '--device-similarity' in sys.argv else None)
        rel = dict(relations_matrices={'itemid': S, 'userid': None}, relations_indices={'itemid': None, 'userid': None})
        data = ItemColdStartSimilarityArrayData(training, holdout, Ft, Fc, **rel, **kw)
        parent = HybridSVD(SimilarityArrayData(training, holdout=(np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users)),
                                               **rel, **kw), ops=ops)
        m = HybridSVDItemColdStart(data, ops=ops)
    else:
        data = ItemColdStartArrayData(training, holdout, Ft, Fc, **kw)
        parent = SVDModel(ArrayData(training, holdout=(np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users)), **kw), ops=ops)
        m = SVDModelItemColdStart(data, ops=ops)
    for x in (m, parent):
        x.verbose, x.rank, x.topk = False, rank, topk
    out = dict(model=m.method, n_users=n_users, n_train_items=len(train_ids), n_cold=int(data.n_cold_items),
               n_labels=int(F.shape[1]), rank=rank, topk=topk)
    parent.build(return_factors=True)
    _, t_parent = timed(lambda: parent.build(return_factors=True))
    m.build()
    _, t_build = timed(m.build)
    out['build'] = dict(seconds=round(t_build, 4), parent_seconds=round(t_parent, 4), extra_seconds=round(t_build - t_parent, 4))
    n_cold = data.n_cold_items
    m.collect_recommend_stats = True
    recs = m.get_recommendations()
    st = dict(m.recommend_stats)
    m.collect_recommend_stats = False
    m.get_recommendations()
    t_pass = median_of(m.get_recommendations, 25)
    launches, names = count_launches(ops, m.get_recommendations)
    out['pass'] = dict(seconds=round(t_pass, 6), cold_items_per_s=round(n_cold / t_pass, 1),
                       pairs_per_s=float('%.4g' % (n_cold * n_users / t_pass)),
                       tiles_scored_share=round(st['tiles_scored'] / max(1, st['tiles_total']), 4),
                       flagged=int(st['flagged_users']), item_splits=st.get('item_splits'), two_phase=st.get('two_phase', None) and
                       {k: st['two_phase'][k] for k in ('head_tiles', 'splits')}, launches=launches, entry_points=names)
    # the front end of the pass on its own: E = (F_cold W) G
    out['queries'] = dict(seconds=round(median_of(m._cold_queries_device, 50), 7))
    if cpu:
        import coldstart_reference as ref
        W, G = m.item_features_embeddings, m._item_features_transform_helper
        U, sigma = m.factors['userid'], m.factors['singular_values']
        Fk = Fc[:, m.item_features_labels].tocsr()
        t0 = time.perf_counter()
        differ, chunk = 0, 512
        X = U * sigma[None, :]
        for s0 in range(0, n_cold, chunk):
            s = (np.asarray(Fk[s0:s0 + chunk] @ W) @ G) @ X.T
            part = np.argpartition(-s, topk, axis=1)[:, :topk]
            ps = np.take_along_axis(s, part, axis=1)
            order = np.lexsort((part, -ps), axis=1)
            lists = np.take_along_axis(part, order, axis=1)
            differ += int((lists != recs[s0:s0 + chunk]).any(axis=1).sum())
        t_cpu = time.perf_counter() - t0
        out['cpu'] = dict(seconds=round(t_cpu, 3), speedup=round(t_cpu / t_pass, 1), rows=n_cold, rows_differing=differ)
    return out


def main():
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    F = item_features(n_items)
    cpu = '--cpu' in sys.argv
    print(json.dumps(run(ops, False, u, i, v, n_users, n_items, F, 50, 10, cpu)), flush=True)
    if '--hybrid' in sys.argv:
        torch.cuda.empty_cache()
        print(json.dumps(run(ops, True, u, i, v, n_users, n_items, F, 50, 10, cpu)), flush=True)


if __name__ == '__main__':
    main()

"""SimilarityAggregation ('SIM') and SimilarityAggregationItemColdStart ('SIM(cs)') on the ML-20M-shaped workload
(synth.make_workload('ml20m'): 138 493 x 26 744, 2.0e7 ratings) with a seeded feature similarity (3 000 labels, ~8 per
item, popularity-skewed: tools/bench_coldstart.py), topk 10.  Prints ONE JSON line:
  s:      shape, entries and fill of S (diagonal removed);
  sim:    build seconds, full-pass seconds over all users (every user a test user, its training row as known items),
          users per second, pads;
  dense:  the same pass by the only device route the package had before: S as a dense fp64 image through ops.i2i_topk
          (image seconds, pass seconds, rows whose lists differ beyond ties from the sparse kernel's at tolerance 1e-12);
  simcs:  20 % of the items cold: build seconds (training CSR + its CSC image), full-pass seconds over the cold items,
          cold items per second, pads;
  cpu (with --cpu): SciPy's product and a NumPy selection of a seeded sample of rows of both passes on the host (rows per
          second), and the number of sample rows whose device list equals the host's exactly.
--device-similarity builds S with polara_amd.similarity on the device instead of SciPy (the default).
Timings: the second of two identical calls (the first pays allocations and code loads), synchronised."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import scipy.sparse as sps
import torch

from polara_amd import i2i
from polara_amd.data import ItemColdStartSimilarityArrayData, SimilarityArrayData
from polara_amd.ops import HipOps
from polara_amd.simagg import SimilarityAggregation, SimilarityAggregationItemColdStart
from polara_amd.synth import make_workload, csr_to_coo_triplets
from bench_coldstart import cosine, item_features


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def host_sample(L, B, recs, topk, filter_seen, n_sample, seed=0):
    """SciPy's product and the NumPy selection of a seeded sample of L's rows; rows/s and the rows equal to `recs`."""
    import i2i_reference as ref
    import sim_reference as sim
    rows = np.sort(np.random.default_rng(seed).choice(L.shape[0], min(n_sample, L.shape[0]), replace=False))
    Ls = L[rows]
    t0 = time.perf_counter()
    scores = sim.product(Ls, B)
    seen = sim.seen_mask(Ls) if filter_seen else np.zeros(scores.shape, dtype=bool)
    want = ref.select(scores, seen, topk, filter_seen, True)
    t = time.perf_counter() - t0
    return dict(sample_rows=len(rows), seconds=round(t, 3), rows_per_s=round(len(rows) / t, 1),
                exact_rows=int((recs[rows] == want).all(1).sum()))


def main():
    ops = HipOps('cuda:0')
    csr, cfg = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    topk = 10
    F = item_features(n_items)
    out = dict(workload='ml20m', n_users=n_users, n_items=n_items, nnz=int(len(v)), n_labels=int(F.shape[1]), topk=topk)

    # ---- SIM: every user a test user ------------------------------------------------------------------------------
    S = cosine(F, ops if '--device-similarity' in sys.argv else None)      # default: SciPy on the host, as before
    rel = dict(relations_matrices={'itemid': S, 'userid': None}, relations_indices={'itemid': None, 'userid': None})
    hold = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = SimilarityArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False, **rel)
    m = SimilarityAggregation(data, ops=ops)
    m.verbose, m.topk = False, topk
    m.build()
    _, t_build = timed(m.build)
    out['s'] = dict(shape=[n_items, n_items], nnz=int(m.build_stats['nnz']), fill=round(m.build_stats['fill'], 5))
    m.get_recommendations()
    recs, t_pass = timed(m.get_recommendations)
    out['sim'] = dict(build_s=round(t_build, 4), pass_s=round(t_pass, 4), users_per_s=round(n_users / t_pass, 1),
                      pads=int((recs < 0).sum()))
    print('sim', json.dumps(out['sim']), file=sys.stderr, flush=True)

    # ---- the route through the dense image (what the package could do before) ------------------------------------------------
    if '--no-dense' not in sys.argv:
        T, _, _ = m._device_test_csr()
        St = m._St

        def image():
            C = torch.zeros(n_items, i2i.leading_dim(n_items), dtype=torch.float64, device=ops.device)
            rows = torch.repeat_interleave(torch.arange(n_items, device=ops.device), St.indptr[1:] - St.indptr[:-1])
            C[rows, St.indices.long()] = St.values.double()
            return C
        C, t_image = timed(image)
        ops.i2i_topk(T, C, n_items, topk, True, True)
        (dense_recs, _), t_dense = timed(lambda: ops.i2i_topk(T, C, n_items, topk, True, True))
        dense_recs = ops.to_host(dense_recs)
        out['dense'] = dict(image_s=round(t_image, 4), image_bytes=int(C.numel() * 8), pass_s=round(t_dense, 4),
                            users_per_s=round(n_users / t_dense, 1),
                            rows_with_other_lists=int((dense_recs != recs).any(1).sum()))
        del C
        print('dense', json.dumps(out['dense']), file=sys.stderr, flush=True)
    if '--cpu' in sys.argv:
        A = sps.csr_matrix((v, (u, i)), shape=(n_users, n_items))
        Sd = S.copy()
        Sd.setdiag(0)
        Sd.eliminate_zeros()
        B = Sd.T.tocsr()
        B.sort_indices()
        out['cpu_sim'] = host_sample(A, B, recs, topk, True, 500)
    m._renew_model()
    del m
    torch.cuda.empty_cache()

    # ---- SIM(cs): 20 % of the items cold ----------------------------------------------------------------------------
    cold_items = np.sort(np.random.RandomState(0).permutation(n_items)[:n_items // 5])
    is_cold = np.zeros(n_items, dtype=bool)
    is_cold[cold_items] = True
    train_ids = np.flatnonzero(~is_cold)
    new_train = np.full(n_items, -1, np.int64)
    new_train[train_ids] = np.arange(len(train_ids))
    new_cold = np.full(n_items, -1, np.int64)
    new_cold[cold_items] = np.arange(len(cold_items))
    tr = ~is_cold[i]
    training = (u[tr], new_train[i[tr]], v[tr])
    holdout = (u[~tr], new_cold[i[~tr]], v[~tr])
    M = S[cold_items][:, train_ids].tocsr()
    cs = ItemColdStartSimilarityArrayData(training, holdout, F[train_ids].tocsr(), F[cold_items].tocsr(), n_users=n_users,
                                          n_items=len(train_ids), relations_matrices={'itemid': None, 'userid': None},
                                          relations_indices={'itemid': None, 'userid': None},
                                          cold_relations_matrices={'itemid': M})
    c = SimilarityAggregationItemColdStart(cs, ops=ops)
    c.verbose, c.topk = False, topk
    c.build()
    _, t_cbuild = timed(c.build)
    c.get_recommendations()
    crecs, t_cpass = timed(c.get_recommendations)
    L = cs.cold_items_similarity
    out['simcs'] = dict(n_cold=int(cs.n_cold_items), n_train_items=len(train_ids), l_nnz=int(L.nnz),
                        l_fill=round(L.nnz / float(L.shape[0] * L.shape[1]), 5), build_s=round(t_cbuild, 4),
                        pass_s=round(t_cpass, 4), cold_items_per_s=round(cs.n_cold_items / t_cpass, 1),
                        pads=int((crecs < 0).sum()))
    if '--cpu' in sys.argv:
        A = sps.csr_matrix((training[2], (training[0], training[1])), shape=(n_users, len(train_ids)))
        B = A.T.tocsr()
        B.sort_indices()
        out['cpu_simcs'] = host_sample(L, B, crecs, topk, False, 100)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

"""Item-to-item (CooccurrenceModel) and most-popular (PopularityModel) on the ML-20M-shaped workload
(synth.make_workload('ml20m'): 138 493 x 26 744, 2.0e7 ratings), topk 10, every user a test user (its training row
as known items).  Prints ONE JSON line:
  i2i: build seconds, full-pass seconds, users per second, i2i_dtype, image bytes the pass reads per second and that
       rate against 6.3 TB/s;
  mp:  build seconds, full-pass seconds, users per second;
  cpu (with --cpu): SciPy's A.T @ A + setdiag(0) timed on the host, SciPy scoring of a seeded 2 000-user sample timed
       on the host, and the number of sample rows whose device list is tie-aware identical to the host's.
Timings: the second of two identical calls (the first pays allocations and code loads), synchronised."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

from polara_amd import i2i
from polara_amd.data import ArrayData
from polara_amd.models import CooccurrenceModel, PopularityModel
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

HBM_TBPS = 6.3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def cpu_leg(u, i, v, shape, recs, topk, n_sample=2000, seed=0):
    import scipy.sparse as sps
    import i2i_reference as ref
    A = sps.csr_matrix((v, (u, i)), shape=shape)
    t0 = time.perf_counter()
    C = A.T.dot(A)
    C.setdiag(0)
    C.eliminate_zeros()
    t_build = time.perf_counter() - t0
    rows = np.sort(np.random.default_rng(seed).choice(shape[0], min(n_sample, shape[0]), replace=False))
    T = A[rows]
    t0 = time.perf_counter()
    S = T.dot(C).toarray()
    t_score = time.perf_counter() - t0
    seen = T.toarray() != 0
    cls = ref.classes(S, seen, True, True)
    want = ref.select(S, seen, topk, True, True)
    bad = ref.tie_aware_mismatches(recs[rows], want, S, cls)
    return dict(scipy_build_s=round(t_build, 2), scipy_sample_users=len(rows), scipy_sample_score_s=round(t_score, 2),
                scipy_users_per_s=round(len(rows) / t_score, 1), identical_rows=len(rows) - len(bad),
                exact_rows=int((recs[rows] == want).all(1).sum()), c_nnz=int(C.nnz))


def main():
    ops = HipOps('cuda:0')
    csr, cfg = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    topk = 10
    hold = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False)
    out = dict(workload='ml20m', n_users=n_users, n_items=n_items, nnz=int(len(v)), topk=topk)

    m = CooccurrenceModel(data, ops=ops)
    m.verbose, m.topk = False, topk
    m.build()
    _, t_build = timed(m.build)
    m.get_recommendations()
    recs, t_pass = timed(m.get_recommendations)
    elem = 4 if m.i2i_dtype == 'float32' else 8
    bytes_read = len(v) * i2i.leading_dim(n_items) * elem
    out['i2i'] = dict(build_s=round(t_build, 4), pass_s=round(t_pass, 4), users_per_s=round(n_users / t_pass, 1),
                      i2i_dtype=m.i2i_dtype, image_bytes=int(m.build_stats['image_bytes']),
                      pass_bytes=int(bytes_read), pass_TBps=round(bytes_read / t_pass / 1e12, 3),
                      of_hbm=round(bytes_read / t_pass / 1e12 / HBM_TBPS, 3), pads=int((recs < 0).sum()))
    m._renew_model()
    del m
    torch.cuda.empty_cache()

    p = PopularityModel(data, ops=ops)
    p.verbose, p.topk = False, topk
    p.build()
    _, t_pbuild = timed(p.build)
    p.get_recommendations()
    _, t_ppass = timed(p.get_recommendations)
    out['mp'] = dict(build_s=round(t_pbuild, 4), pass_s=round(t_ppass, 4), users_per_s=round(n_users / t_ppass, 1))

    if '--cpu' in sys.argv:
        out['cpu'] = cpu_leg(u, i, v, (n_users, n_items), recs, topk)
    print(json.dumps(out))


if __name__ == '__main__':
    main()

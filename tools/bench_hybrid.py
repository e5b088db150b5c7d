"""HybridSVD on the ML-20M-shaped workload (synth.make_workload('ml20m'): 138 493 x 26 744, 2.0e7 ratings), rank 50,
top-10, every user a test user, with S the cosine similarity of seeded sparse binary item features.  Prints ONE JSON line:
  factor: densify + Cholesky seconds of K = S + I and the fp64 rate they reach (n^3 / 3 flop);
  trmm:   seconds and bytes per second of one 16-column triangular product (the triangle's bytes), against 6.3 TB/s;
  build:  seconds of the whole HybridSVD build (factor, eigensolver, projectors) and its Gramian steps;
  pass:   seconds and users per second of a full scoring pass (exact fold-in against vr), and the same for SVDModel;
  cpu (with --cpu): SciPy's cholesky of the same K on the host, and how many rows of a seeded 2 000-user sample are
       tie-aware identical to the restatement's lists (tests/hybrid_reference.py: T vr vl^T on the host) from the
       model's projectors.
--device-similarity builds S with polara_amd.similarity on the device instead of SciPy (the default).
Timings: the second of two identical calls, synchronised."""
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

from polara_amd import hybrid
from polara_amd.data import SimilarityArrayData
from polara_amd.models import HybridSVD, SVDModel
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

HBM_TBPS = 6.3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def item_similarity(n_items, n_features=2000, density=0.004, seed=7, ops=None):
    rng = np.random.default_rng(seed)
    nnz = int(n_items * n_features * density)
    F = sps.csr_matrix((np.ones(nnz), (rng.integers(0, n_items, nnz), rng.integers(0, n_features, nnz))),
                       shape=(n_items, n_features))
    F = F + sps.csr_matrix((np.ones(n_items), (np.arange(n_items), rng.integers(0, n_features, n_items))), shape=F.shape)
    F.data[:] = 1.0
    if ops is not None:              # --device-similarity: the same S by polara_amd.similarity on the device
        from polara_amd.similarity import cosine_similarity
        return cosine_similarity(F, ops=ops)
    Fn = sps.diags(1.0 / np.sqrt(np.asarray(F.sum(1)).ravel())) @ F
    S = (Fn @ Fn.T).tocsr()
    S.setdiag(1.0)
    S.sum_duplicates()           # canonical, as the model keeps its checked copy of the relations (once per matrix)
    return S


def main():
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    rank, topk = 50, 10
    S = item_similarity(n_items, ops=ops if '--device-similarity' in sys.argv else None)
    out = dict(workload='ml20m', n_users=n_users, n_items=n_items, nnz=int(len(v)), s_nnz=int(S.nnz), rank=rank, topk=topk)
    perm = np.random.default_rng(0).permutation(n_items)

    def factor():
        K = ops.hybrid_densify(S, perm, 1.0)
        ops.chol(K, n_items)
        return K
    factor()
    K, t_factor = timed(factor)
    out['factor'] = dict(seconds=round(t_factor, 4), fp64_TFLOPs=round(n_items ** 3 / 3 / t_factor / 1e12, 2))
    X = torch.randn(n_items, 16, dtype=torch.float64, device=ops.device)
    ops.trmm(K, n_items, X)
    _, t_mm = timed(lambda: ops.trmm(K, n_items, X))
    tri = n_items * (n_items + 1) // 2 * 8
    out['trmm16'] = dict(seconds=round(t_mm, 6), triangle_bytes=tri, TBps=round(tri / t_mm / 1e12, 3),
                         of_hbm=round(tri / t_mm / 1e12 / HBM_TBPS, 3))
    del K
    torch.cuda.empty_cache()

    hold = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = SimilarityArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False,
                               relations_matrices={'itemid': S}, relations_indices={'itemid': None})
    m = HybridSVD(data, ops=ops)
    m.verbose, m.rank, m.topk = False, rank, topk

    def build():
        m._chol = None                   # the factor is part of the build
        m.build()
    build()
    _, t_build = timed(build)
    out['build'] = dict(seconds=round(t_build, 4), gramian_steps=int(m.build_stats.get('gramian_steps', 0)),
                        method=str(m.build_stats.get('method')))
    m.get_recommendations()
    recs, t_pass = timed(m.get_recommendations)
    out['pass'] = dict(seconds=round(t_pass, 4), users_per_s=round(n_users / t_pass, 1))
    p = SVDModel(data, ops=ops)
    p.verbose, p.rank, p.topk = False, rank, topk
    p.build()
    p.get_recommendations()
    _, t_svd = timed(p.get_recommendations)
    out['pass']['svd_seconds'] = round(t_svd, 4)
    out['pass']['vs_svd'] = round(t_pass / t_svd, 2)

    if '--cpu' in sys.argv:
        import scipy.linalg
        import hybrid_reference as ref
        from i2i_reference import tie_aware_mismatches
        Kh = S.toarray() + np.eye(n_items)
        t0 = time.perf_counter()
        L = scipy.linalg.cholesky(Kh, lower=True, overwrite_a=True, check_finite=False)
        t_cpu = time.perf_counter() - t0
        vl, vr = m.get_item_projector()
        rows = np.sort(np.random.default_rng(0).choice(n_users, 2000, replace=False))
        A = sps.csr_matrix((v, (u, i)), shape=(n_users, n_items))
        T = A[rows]
        seen = T.toarray() != 0
        scores, cls, lists = ref.scores_and_lists(T, seen, vl, vr, topk)
        bad = tie_aware_mismatches(recs[rows], lists, scores, cls, tol=1e-9)
        out['cpu'] = dict(scipy_cholesky_s=round(t_cpu, 2), sample_users=len(rows), identical_rows=len(rows) - len(bad))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

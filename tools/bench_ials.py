"""ImplicitALS on the ML-20M-shaped planted matrix (138 493 x 26 744, 2.0e7 ratings 1..5), default confidence log2(rating)
(ratings of 1 are dropped), lambda = 0.01, top-10.  Prints ONE JSON line and writes it to profiles/ials_bench_line.json; per
rank (`--ranks 10,50`):
  confidence: seconds of the confidence round trip (values to the host, NumPy transform, upload, zeros dropped);
  transpose:  seconds of pk_csr_transpose of the confidence matrix;
  user_half_step / item_half_step: median seconds of one half-step (the Gram product timed apart, `gram`);
  loss:       median seconds of the objective (two Gram products, the sparse-term kernel, one read);
  build:      seconds of the 15-epoch build (confidence, transpose, epochs, serving index), `--epochs N` to change;
  pass:       median seconds of the scoring pass (all users, seen items filtered, lists copied to the host);
  fold_in:    median seconds of folding ALL users in against the built item factors (one user half-step);
  numpy:      seconds of the NumPy restatement of one user half-step (tests/ials_reference.py) on this machine, timed on
              `--numpy-rows` rows (default 200, evenly spaced over the users in their own order) and scaled to all rows by
              stored entries — a per-row Python loop, np.linalg.solve per row; 0 = skip.
Timings are synchronised; nothing here is part of bench.py."""
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

from bench_coldstart import median_of, timed
from polara_amd import ials
from polara_amd.data import ArrayData
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

LAMBDA = 0.01


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    ranks = [int(x) for x in opt('--ranks', '10,50').split(',')]
    epochs = int(opt('--epochs', '15'))
    reps = int(opt('--reps', '5'))
    numpy_rows = int(opt('--numpy-rows', '200'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    every_user = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=every_user)
    out = dict(n_users=n_users, n_items=n_items, ratings=len(v), regularization=LAMBDA, epochs=epochs, ranks={})
    for rank in ranks:
        m = ials.ImplicitALS(data, seed=0, ops=ops)
        m.verbose, m.topk, m.rank, m.num_epochs, m.regularization = False, 10, rank, epochs, LAMBDA
        A = m._training_device_csr()
        m._confidence_csr(A)
        C, t_conf = timed(lambda: m._confidence_csr(A))
        ops.csr_transpose(C)
        Ct, t_tr = timed(lambda: ops.csr_transpose(C))
        row = dict(nnz=int(C.nnz), confidence=round(t_conf, 5), transpose=round(t_tr, 6))
        X0, Y0 = ials.initial_factors(n_users, n_items, rank, seed=0)
        X, Y = ops.to_device(X0), ops.to_device(Y0)
        GY = ops.gram(Y)
        ops.ials_half_step(C, Y, LAMBDA, out=X, G=GY)
        row['gram'] = round(median_of(lambda: ops.gram(Y), reps), 6)
        row['user_half_step'] = round(median_of(lambda: ops.ials_half_step(C, Y, LAMBDA, out=X, G=GY), reps), 6)
        GX = ops.gram(X)
        ops.ials_half_step(Ct, X, LAMBDA, out=Y, G=GX)
        row['item_half_step'] = round(median_of(lambda: ops.ials_half_step(Ct, X, LAMBDA, out=Y, G=GX), reps), 6)
        ops.ials_loss(C, X, Y, LAMBDA)
        row['loss'] = round(median_of(lambda: ops.ials_loss(C, X, Y, LAMBDA), reps), 6)
        del X, Y, GX, GY, C, Ct, A
        torch.cuda.empty_cache()
        _, t_build = timed(m.build)
        row['build'] = round(t_build, 4)
        row['build_epoch_median'] = round(float(np.median(m.iterations_time)), 6)
        m.get_recommendations()
        row['pass'] = round(median_of(m.get_recommendations, reps), 6)
        # the fold-in of all users: the training rows as a warm-start test set
        m.data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, test=(u, i, v), holdout=every_user, warm_start=True)
        Cw = m.fold_in_matrix()
        Yd, GYd = m._item_factors_block()
        block = ops.zeros(n_users, rank + (rank & 1))
        ops.ials_half_step(Cw, Yd, LAMBDA, out=block[:, :rank], G=GYd)
        row['fold_in'] = round(median_of(lambda: ops.ials_half_step(Cw, Yd, LAMBDA, out=block[:, :rank], G=GYd), reps), 6)
        _, t_fold_all = timed(m.fold_in)
        row['fold_in_with_matrix'] = round(t_fold_all, 5)
        if numpy_rows:
            import ials_reference as ref
            import scipy.sparse as sps
            keep = v != 1.
            Ch = sps.csr_matrix((np.log2(v[keep]), (u[keep], i[keep])), shape=(n_users, n_items))
            rows = np.linspace(0, n_users - 1, numpy_rows).astype(np.int64)
            sample = Ch[rows]
            Yh = m.factors[m.data.fields.itemid]
            G = Yh.T @ Yh
            t0 = time.perf_counter()
            ref.half_step(sample, Yh, G, LAMBDA, ref.lapack_solve)
            t = time.perf_counter() - t0
            row['numpy'] = dict(rows=int(numpy_rows), rows_nnz=int(sample.nnz), seconds=round(t, 3),
                                scaled_to_all_rows=round(t * Ch.nnz / max(sample.nnz, 1), 1))
        out['ranks'][rank] = row
        del m
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(ROOT, 'profiles', 'ials_bench_line.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

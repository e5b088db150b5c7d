"""ImplicitLMF on the ML-20M-shaped planted matrix (138 493 x 26 744, 2.0e7 ratings 1..5), default confidence log2(rating)
(ratings of 1 are dropped), the model's defaults (learning_rate 1.0, regularization 0.6, neg_prop 30), top-10.  Prints ONE JSON
line and writes it to profiles/lmf_bench_line.json; per rank (`--ranks 10,30,50`):
  plan:       seconds of the two plans (row order, prefix sum of the negatives) on fresh matrices, the transpose timed apart;
  user_half_step / item_half_step: median seconds of one half-step, `samples` its positives + negatives, `gathered_tb_s` the
              rows it gathers (samples x K x 8 bytes) per second, `of_gather_figure` that over the 8.6 TB/s at which uniformly
              random rows of a 38 MB table are gathered into LDS chip-wide (the machine's measured figure for the Infinity Cache);
  build:      seconds of the 30-epoch build (confidence, transpose, plans, epochs, serving index), `--epochs N` to change;
  pass:       median seconds of the scoring pass (all users, seen items filtered, lists copied to the host);
  fold_in:    median seconds of folding ALL users in against the built item factors (`fold_in_epochs` = 10 user half-steps);
  numpy:      seconds of the NumPy restatement of one user half-step (tests/lmf_reference.py) on this machine, timed on
              `--numpy-rows` rows (default 200, evenly spaced over the users) and scaled to all rows by samples; 0 = skip.
`--half-steps-only` stops after the half-steps and `--out NAME` names the file under profiles/: with POLARA_HIP_LIB pointing at a
library whose lmf.hip was compiled with -DPK_LMF_CHAINS=N or -DLMF_THREADS=64, this is how the variants of DESIGN.md were timed.
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
from polara_amd import lmf
from polara_amd.data import ArrayData
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

GATHER_FIGURE_TB_S = 8.6


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    ranks = [int(x) for x in opt('--ranks', '10,30,50').split(',')]
    epochs = int(opt('--epochs', '30'))
    reps = int(opt('--reps', '5'))
    numpy_rows = int(opt('--numpy-rows', '200'))
    out_name = opt('--out', 'lmf_bench_line.json')
    half_steps_only = '--half-steps-only' in argv
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    every_user = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=every_user)
    out = dict(n_users=n_users, n_items=n_items, ratings=len(v), epochs=epochs, chains=int(ops.lib.pk_lmf_chains()), ranks={})
    for rank in ranks:
        m = lmf.ImplicitLMF(data, seed=0, ops=ops)
        m.verbose, m.topk, m.rank, m.num_epochs = False, 10, rank, epochs
        lr, reg, neg_prop, K = m.learning_rate, m.regularization, m.neg_prop, rank + 2
        A = m._training_device_csr()
        C = m._confidence_csr(A)
        _, t_tr = timed(lambda: C.T)
        Ct = C.T
        ops.lmf_plan(m._confidence_csr(A), neg_prop)                                  # warm-up on a matrix of its own
        (users, items), t_plan = timed(lambda: (ops.lmf_plan(C, neg_prop), ops.lmf_plan(Ct, neg_prop)))
        row = dict(nnz=int(C.nnz), neg_prop=neg_prop, transpose=round(t_tr, 6), plan=round(t_plan, 6),
                   user_negatives=users['negatives'], item_negatives=items['negatives'])
        X0, Y0 = lmf.initial_factors(n_users, n_items, rank, seed=0)
        X, Y = ops.to_device(X0), ops.to_device(Y0)
        AX, AY = ops.zeros(n_users, K), ops.zeros(n_items, K)
        for name, plan, fixed, moved, state, pinned in (('user_half_step', users, Y, X, AX, K - 1), ('item_half_step', items, X, Y, AY, K - 2)):
            step = lambda: ops.lmf_half_step(plan, fixed, moved, state, lr, reg, 0, 0, pinned)
            step()
            t = median_of(step, reps)
            samples = int(C.nnz) + plan['negatives']
            tb_s = samples * K * 8 / t / 1e12
            row[name] = dict(seconds=round(t, 6), samples=samples, table_mb=round(fixed.shape[0] * K * 8 / 1e6, 1),
                             gathered_tb_s=round(tb_s, 3), of_gather_figure=round(tb_s / GATHER_FIGURE_TB_S, 3))
        del X, Y, AX, AY, C, Ct, A, users, items
        torch.cuda.empty_cache()
        if half_steps_only:
            out['ranks'][rank] = row
            continue
        _, t_build = timed(m.build)
        row['build'] = round(t_build, 4)
        row['build_epoch_median'] = round(float(np.median(m.iterations_time)), 6)
        m.get_recommendations()
        row['pass'] = round(median_of(m.get_recommendations, reps), 6)
        # the fold-in of all users: the training rows as a warm-start test set
        m.data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, test=(u, i, v), holdout=every_user, warm_start=True)
        m.fold_in()
        row['fold_in'] = round(median_of(m.fold_in, max(1, reps // 2)), 5)
        row['fold_in_epochs'] = int(m.fold_in_epochs)
        if numpy_rows:
            import lmf_reference as ref
            import scipy.sparse as sps
            keep = v != 1.
            Ch = sps.csr_matrix((np.log2(v[keep]), (u[keep], i[keep])), shape=(n_users, n_items))
            rows = np.linspace(0, n_users - 1, numpy_rows).astype(np.int64)
            sample = Ch[rows]
            Yh = m.factors[m.data.fields.itemid]
            Xh = np.ascontiguousarray(m.factors[m.data.fields.userid][rows])
            part = int(sample.nnz + ref.neg_pointers(sample.indptr, n_items, neg_prop)[-1])
            total = int(Ch.nnz + ref.neg_pointers(Ch.indptr, n_items, neg_prop)[-1])
            t0 = time.perf_counter()
            ref.half_step(sample, Yh, Xh, np.zeros_like(Xh), lr, reg, neg_prop, 0, 0, K - 1)
            t = time.perf_counter() - t0
            row['numpy'] = dict(rows=int(numpy_rows), rows_samples=part, seconds=round(t, 3),
                                scaled_to_all_rows=round(t * total / max(part, 1), 1))
        out['ranks'][rank] = row
        del m
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(ROOT, 'profiles', out_name), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

"""ImplicitALSPP on the ML-20M-shaped planted matrix of tools/bench_ials.py (138 493 x 26 744, 2.0e7 ratings 1..5, confidence
log2(rating), lambda = 0.01, top-10).  Prints ONE JSON line and writes it to profiles/ialspp_bench_line.json:
  exact[128]:        median seconds of the exact user / item half-step of ImplicitALS at rank 128 (pk_ials_half_step_f64);
  sweeps[rank][d]:   for `--ranks` (default 128,256,512,1024) and d = 16, 32, 64 the median seconds of a user and an item
                     half-sweep, and their split into predict / tsmm (R = X G[:,pi], all blocks) / block steps (all blocks),
                     each timed apart on the same inputs;
  build / pass:      seconds of the `--epochs` (15) epoch build at `--build-rank` (512, d = 64; 0 = skip) and the median
                     seconds of the scoring pass (all users, seen items filtered, lists copied to the host).
Timings are synchronised host clocks around warmed calls; nothing here is part of bench.py and nothing is asserted."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_coldstart import median_of, timed
from polara_amd import ials, ialspp
from polara_amd.data import ArrayData
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

LAMBDA = 0.01


def sweep_split(ops, Cm, B, A, G, d, reps):
    """median seconds of the parts of one half-sweep of A against the fixed B, and of the whole"""
    k = int(B.shape[1])
    E = ops.ialspp_predict(Cm, A, B)
    blocks = [(p0, min(p0 + d, k)) for p0 in range(0, k, d)]
    R = [ops.tsmm(A, G[:, p0:p1]) for p0, p1 in blocks]

    def steps():
        for (p0, _), r in zip(blocks, R):
            ops.ialspp_block_step(Cm, B, A, E, G, p0, d, LAMBDA, R=r)
    steps()
    row = dict(predict=median_of(lambda: ops.ialspp_predict(Cm, A, B, out=E), reps),
               tsmm=median_of(lambda: [ops.tsmm(A, G[:, p0:p1], out=r) for (p0, p1), r in zip(blocks, R)], reps),
               block_steps=median_of(steps, reps),
               half_sweep=median_of(lambda: ops.ialspp_half_sweep(Cm, B, A, G, LAMBDA, d, E=E), reps))
    return {name: round(t, 6) for name, t in row.items()}


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    ranks = [int(x) for x in opt('--ranks', '128,256,512,1024').split(',')]
    sizes = [int(x) for x in opt('--block-sizes', '16,32,64').split(',')]
    epochs = int(opt('--epochs', '15'))
    build_rank = int(opt('--build-rank', '512'))
    reps = int(opt('--reps', '3'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    every_user = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=every_user)
    m = ialspp.ImplicitALSPP(data, seed=0, ops=ops)
    m.verbose, m.topk, m.regularization = False, 10, LAMBDA
    C = m._confidence_csr(m._training_device_csr())
    Ct = C.T
    out = dict(n_users=n_users, n_items=n_items, ratings=len(v), nnz=int(C.nnz), regularization=LAMBDA, exact={}, sweeps={})
    line_path = os.path.join(ROOT, 'profiles', 'ialspp_bench_line.json')

    def factors(rank):
        X0, Y0 = ials.initial_factors(n_users, n_items, rank, seed=0)
        X, Y = ops.to_device(X0), ops.to_device(Y0)
        ops.ialspp_half_sweep(C, Y, X, ops.gram(Y), LAMBDA, 64)        # one sweep each: factors of a build under way
        ops.ialspp_half_sweep(Ct, X, Y, ops.gram(X), LAMBDA, 64)
        return X, Y

    for rank in ranks:
        X, Y = factors(rank)
        GY, GX = ops.gram(Y), ops.gram(X)
        if rank <= ops.ials_max_rank():
            Xe, Ye = X.clone(), Y.clone()
            ops.ials_half_step(C, Y, LAMBDA, out=Xe, G=GY)
            ops.ials_half_step(Ct, X, LAMBDA, out=Ye, G=GX)
            out['exact'][rank] = dict(user_half_step=round(median_of(lambda: ops.ials_half_step(C, Y, LAMBDA, out=Xe, G=GY), reps), 6),
                                      item_half_step=round(median_of(lambda: ops.ials_half_step(Ct, X, LAMBDA, out=Ye, G=GX), reps), 6))
            del Xe, Ye
        out['sweeps'][rank] = {}
        for d in sizes:
            out['sweeps'][rank][d] = dict(user=sweep_split(ops, C, Y, X.clone(), GY, d, reps),
                                          item=sweep_split(ops, Ct, X, Y.clone(), GX, d, reps))
            print('rank %d d %d: %s' % (rank, d, json.dumps(out['sweeps'][rank][d])), flush=True)
        del X, Y, GX, GY
        torch.cuda.empty_cache()
    del C, Ct
    if build_rank:
        m.rank, m.num_epochs, m.block_size = build_rank, epochs, 64
        _, t_build = timed(m.build)
        out['build'] = dict(rank=build_rank, block_size=64, epochs=epochs, seconds=round(t_build, 4),
                            epoch_median=round(float(np.median(m.iterations_time)), 6))
        m.get_recommendations()
        out['build']['pass'] = round(median_of(m.get_recommendations, reps), 6)
    line = json.dumps(out)
    print(line, flush=True)
    with open(line_path, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

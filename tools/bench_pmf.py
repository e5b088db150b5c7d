"""ProbabilisticMF on the ML-20M-shaped planted matrix (138 493 x 26 744, 2.0e7 ratings), rank 10, top-10.
Prints ONE JSON line:
  plan:    per B the seconds of the device plan (HipOps.pmf_plan: counts, parts, one stable radix sort, three gathers), the
           empty blocks and the longest block;
  epoch:   per B (B = 1 — the reference's serial order — included unless `--no-serial`) the median seconds of one sweep
           (pk_pmf_epoch_f64: B + 1 launches, the squared error read back), samples per second, and the same with adagrad;
  default: the B of pmf.default_blocks for this matrix (its constants: machine_model.py);
  pass:    median seconds of the scoring pass (all users, seen items filtered, lists copied to the host) after a 2-epoch build;
  numpy:   seconds per epoch of the NumPy restatement (tests/pmf_reference.py) on this machine at `--numpy-blocks` (default
           256; it sweeps sample t of all blocks of a stratum at once, so its time falls with B; 0 = skip).
`--blocks 1,64,256,1024,2048,4096`, `--epochs N` timed sweeps per B (default 3; B = 1: one).  Timings are synchronised;
nothing here is part of bench.py."""
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
from polara_amd import pmf
from polara_amd.data import ArrayData
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

RANK, ETA, LAMBD = 10, 0.005, 0.5


def epoch_seconds(ops, plan, n_users, n_items, adjust, reps):
    P0, Q0 = pmf.initial_factors(n_users, n_items, RANK, seed=0)
    P, Q = ops.to_device(P0), ops.to_device(Q0)
    state = (ops.zeros(n_users, RANK), ops.zeros(n_items, RANK)) if adjust else None

    def sweep():
        if state is not None:
            state[0].zero_()
            state[1].zero_()
        return float(ops.pmf_epoch(plan, P, Q, ETA, LAMBD, adjust=adjust, state=state)[0].item())
    first = timed(sweep)
    if reps <= 1:
        return first[1], first[0]
    return median_of(sweep, reps), first[0]


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    blocks = [int(x) for x in opt('--blocks', '1,64,256,1024,2048,4096').split(',')]
    if '--no-serial' in argv:
        blocks = [b for b in blocks if b != 1]
    reps = int(opt('--epochs', '3'))
    numpy_blocks = int(opt('--numpy-blocks', '256'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    A = ops.csr_from_coo(u, i, v, (n_users, n_items))
    nnz = int(A.nnz)
    out = dict(rank=RANK, n_users=n_users, n_items=n_items, nnz=nnz, plan={}, epoch={},
               default=dict(blocks=pmf.default_blocks(nnz, n_users, n_items), rule='sqrt(nnz * pmf_sample_s / pmf_launch_s)'))
    for B in blocks:
        ops.pmf_plan(A, B)
        plan, t_plan = timed(lambda: ops.pmf_plan(A, B))
        stats = pmf.schedule_stats(ops.to_host(plan['block_ptr']), B)
        out['plan'][B] = dict(seconds=round(t_plan, 5), empty_blocks=stats['empty_blocks'], longest_block=stats['longest_block'])
        row = {}
        for adjust in (None, 'adagrad'):
            if B == 1 and adjust:
                continue
            t, sse = epoch_seconds(ops, plan, n_users, n_items, adjust, 1 if B == 1 else reps)
            row[adjust or 'sgd'] = dict(seconds=round(t, 5), samples_per_s=round(nnz / t, 1), first_rmse=round((sse / nnz) ** 0.5, 6))
        out['epoch'][B] = row
        del plan
        torch.cuda.empty_cache()
    every_user = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    m = pmf.ProbabilisticMF(ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=every_user), seed=0, ops=ops)
    m.verbose, m.topk, m.num_epochs = False, 10, 2
    m.blocks = max(b for b in blocks)
    _, t_build = timed(m.build)
    m.get_recommendations()
    out['pass'] = dict(build_seconds=round(t_build, 4), blocks=m.blocks, seconds=round(median_of(m.get_recommendations, 15), 6))
    if numpy_blocks:
        import pmf_reference as ref
        cu, ci, cv = pmf.canonical_interactions(u, i, v, (n_users, n_items))
        host = ref.make_plan(cu, ci, cv, n_users, n_items, numpy_blocks)
        P, Q = pmf.initial_factors(n_users, n_items, RANK, seed=0)
        t0 = time.perf_counter()
        ref.epoch(host, P, Q, ETA, LAMBD)
        out['numpy'] = dict(blocks=numpy_blocks, seconds_per_epoch=round(time.perf_counter() - t0, 2))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()

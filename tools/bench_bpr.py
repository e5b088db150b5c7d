"""ImplicitBPR on the ML-20M-shaped planted matrix (138 493 x 26 744, 2.0e7 positives), ranks 10 and 50, top-10.
Prints ONE JSON line and writes it to profiles/bpr_bench_line.json:
  plan:    per B the seconds of the device plan with a shuffled item order (HipOps.bpr_plan) — paid once per epoch;
  draw:    per B the seconds of the draw launch (pk_bpr_draw_negatives) and the skipped share of the epoch;
  epoch:   per rank and B in {64, 256, default, 1 024} the median seconds of one sweep (pk_bpr_epoch_f64: B + 1 launches, the
           three counters read back) and samples per second;
  default: the B of bpr.default_blocks for this matrix;
  pass:    per rank the median seconds of the scoring pass (all users, seen items filtered, lists copied to the host) after a
           2-epoch build;
  numpy:   seconds per epoch of the NumPy restatement (tests/bpr_reference.py) on this machine, timed on the first
           `--numpy-users` users (default 300; 0 = skip) at B = 1 and scaled by the share of positives.
`--epochs N` timed sweeps per case (default 3).  Timings are synchronised; nothing here is part of bench.py."""
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
from polara_amd import bpr
from polara_amd.data import ArrayData
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

RANKS, LR, REG, SEED = (10, 50), 0.01, 0.01, 0


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    reps = int(opt('--epochs', '3'))
    numpy_users = int(opt('--numpy-users', '300'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    A = ops.csr_from_coo(u, i, v, (n_users, n_items))
    nnz = int(A.nnz)
    default = bpr.default_blocks(nnz, n_users, n_items)
    blocks = sorted({64, 256, default, 1024})
    out = dict(n_users=n_users, n_items=n_items, nnz=nnz, plan={}, draw={}, epoch={r: {} for r in RANKS},
               default=dict(blocks=default, rule='min(pmf.default_blocks, n_items // 64)'), **{'pass': {}})
    order = bpr.item_order(SEED, 0, n_items)
    for B in blocks:
        ops.bpr_plan(A, B, order)
        plan, t_plan = timed(lambda: ops.bpr_plan(A, B, order))
        ops.bpr_draw_negatives(plan, SEED, 0)
        neg, t_draw = timed(lambda: ops.bpr_draw_negatives(plan, SEED, 0))
        out['plan'][B] = dict(seconds=round(t_plan, 5))
        out['draw'][B] = dict(seconds=round(t_draw, 6), skipped_share=round(float((neg < 0).sum().item()) / nnz, 6))
        for rank in RANKS:
            P0, Q0 = bpr.initial_factors(n_users, n_items, rank, seed=SEED)
            P, Q = ops.to_device(P0), ops.to_device(Q0)
            sweep = lambda: ops.to_host(ops.bpr_epoch(plan, neg, P, Q, LR, REG))
            counts = sweep()
            t = median_of(sweep, reps)
            out['epoch'][rank][B] = dict(seconds=round(t, 5), samples_per_s=round(int(counts[0]) / t, 1))
        del plan, neg
        torch.cuda.empty_cache()
    every_user = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    for rank in RANKS:
        m = bpr.ImplicitBPR(ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=every_user), seed=SEED, ops=ops)
        m.verbose, m.topk, m.num_epochs, m.rank = False, 10, 2, rank
        _, t_build = timed(m.build)
        m.get_recommendations()
        out['pass'][rank] = dict(build_seconds=round(t_build, 4), blocks=m.build_stats['blocks'],
                                 skipped=m.build_stats['skipped'], seconds=round(median_of(m.get_recommendations, 15), 6))
    if numpy_users:
        import bpr_reference as ref
        keep = u < numpy_users
        dense = np.zeros((numpy_users, n_items), dtype=np.int8)
        dense[u[keep], i[keep]] = 1
        host = ref.make_plan(dense, 1, ref.item_order(SEED, 0, n_items))
        neg = ref.draw_negatives(host, SEED, 0)
        P, Q = ref.initial_factors(numpy_users, n_items, 10, SEED)
        t0 = time.perf_counter()
        ref.epoch(host, neg, P, Q, LR, REG)
        t = time.perf_counter() - t0
        out['numpy'] = dict(rank=10, users=numpy_users, positives=int(host['nnz']), seconds=round(t, 3),
                            seconds_per_epoch_scaled=round(t * nnz / max(int(host['nnz']), 1), 1))
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'bpr_bench_line.json'), 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()

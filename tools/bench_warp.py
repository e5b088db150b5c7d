"""The WARP sweep of LightFMWrapper on the ML-20M-shaped planted matrix (138 493 x 26 744, 2.0e7 positives), ranks 10 and 50,
max_sampled = 10, with and without item features (8 of `--labels` labels per item, default 1 000, from a seeded draw).
Prints ONE JSON line and writes it to profiles/warp_bench_line.json:
  plan:    per B the seconds of the device plan with a shuffled item order and the features' upload (HipOps.warp_plan) — paid
           once per epoch;
  draw:    per B the seconds of the draw launch (pk_warp_draw_candidates), the buffer's bytes and the share of -1 candidates;
  epoch:   per rank, B in {64, 256, default, 1 024} and with / without features the median seconds of one sweep
           (pk_warp_epoch_f64, the three counters read back), positives per second, the quiet share and the draws per positive;
           with features also `label_share`: B x (one label image + one label step, each timed as a launch of its own through
           pk_warp_label_image_f64 / pk_warp_label_step_f64 — the latter clears G in a second launch, which the epoch does not
           pay per stratum) over the epoch's seconds;
  default: the B of warp.default_blocks for this matrix.
`--epochs N` timed sweeps per case (default 3).  The embeddings move between the timed sweeps, so the quiet share is that of
the first.  Timings are synchronised; nothing here is part of bench.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_coldstart import median_of, timed
from polara_amd import bpr, warp
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

RANKS, LR, D, SEED, LABELS_PER_ITEM = (10, 50), 0.05, 10, 0, 8


def seeded_features(n_items, n_labels, seed):
    from scipy.sparse import csr_matrix
    rng = np.random.RandomState(seed)
    cols = np.stack([rng.choice(n_labels, LABELS_PER_ITEM, replace=False) for _ in range(n_items)]).ravel()
    rows = np.repeat(np.arange(n_items), LABELS_PER_ITEM)
    return csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_items, n_labels))


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    reps = int(opt('--epochs', '3'))
    n_labels = int(opt('--labels', '1000'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    A = ops.csr_from_coo(np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64), (n_users, n_items))
    nnz = int(A.nnz)
    default = warp.default_blocks(nnz, n_users, n_items)
    blocks = sorted({64, 256, default, 1024})
    one_hot = seeded_features(n_items, n_labels, SEED)
    table = warp.loss_table(n_items, D)
    out = dict(n_users=n_users, n_items=n_items, nnz=nnz, max_sampled=D, n_labels=n_labels, labels_per_item=LABELS_PER_ITEM, plan={},
               draw={}, epoch={r: {} for r in RANKS}, default=dict(blocks=default, rule='bpr.default_blocks (unmeasured for WARP)'))
    order = bpr.item_order(SEED, 0, n_items)
    for B in blocks:
        ops.warp_plan(A, B, order, one_hot)
        plan, t_plan = timed(lambda: ops.warp_plan(A, B, order, one_hot))
        plain = dict(plan, features=None)
        ops.warp_draw(plan, SEED, 0, D)
        cand, t_draw = timed(lambda: ops.warp_draw(plan, SEED, 0, D))
        out['plan'][B] = dict(seconds=round(t_plan, 5))
        out['draw'][B] = dict(seconds=round(t_draw, 6), bytes=nnz * D * 4, seen_share=round(float((cand < 0).sum().item()) / (nnz * D), 6))
        for rank in RANKS:
            for featured in (False, True):
                P0, E0, L0 = warp.initial_embeddings(n_users, n_items, n_labels if featured else 0, rank, seed=SEED)
                P, E, L = ops.to_device(P0), ops.to_device(E0), ops.to_device(L0) if featured else None
                state = tuple(None if X is None else torch.ones_like(X) for X in (P, E, L))
                work = (ops.empty(n_items, rank + 1), ops.zeros(n_items, rank + 1)) if featured else None
                sweep = lambda: ops.to_host(ops.warp_epoch(plan if featured else plain, cand, table, P, E, state, LR, L, work=work))
                counts = sweep()
                t = median_of(sweep, reps)
                row = dict(seconds=round(t, 5), positives_per_s=round(nnz / t, 1), quiet_share=round(int(counts[1]) / nnz, 6),
                           draws_per_positive=round(int(counts[2]) / nnz, 3))
                if featured:
                    t_image = median_of(lambda: (ops.warp_label_image(plan, L), ops.synchronize()), 5)
                    t_step = median_of(lambda: (ops.warp_label_step(plan, work[1], L, state[2], LR), ops.synchronize()), 5)
                    row.update(label_image_seconds=round(t_image, 6), label_step_seconds=round(t_step, 6),
                               label_share=round(B * (t_image + t_step) / t, 4))
                out['epoch'][rank].setdefault(B, {})['features' if featured else 'plain'] = row
        del plan, plain, cand
        torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'warp_bench_line.json'), 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()

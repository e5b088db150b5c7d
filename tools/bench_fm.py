"""The sweep of TuriFactorizationRecommender (TCF) on the ML-20M-shaped planted matrix (138 493 x 26 744, 2.0e7 ratings), ranks
10 and 50, with `--item-labels` item labels (default 1 000, 8 per item) and `--user-labels` user labels (default 200, 3 per user)
from seeded draws, the default rule (rmsprop 0.9, step 0.05).  Prints ONE JSON line and writes it to profiles/fm_bench_line.json:
  plan:    per B the seconds of the device plan with both feature uploads (HipOps.fm_plan);
  epoch:   per rank, B in {default, 1 024, --blocks} and feature set (none / items / both) the median seconds of one sweep
           (pk_fm_epoch_f64, the squared error read back), ratings per second, the first epoch's RMSE; `pmf`: the seconds of
           pk_pmf_epoch_f64 (adagrad) on the same plan and B — the yardstick: the FM sample reads two more rows and, with
           features, updates two rows of G — and `ratio` = FM seconds / PMF seconds; with features also `label_share`: B x (the
           label image + the label step of every featured side, each timed as a launch of its own through
           pk_fm_label_image_f64 / pk_fm_label_step_f64 — the latter clears G in a second launch, which the epoch does not pay
           per stratum) over the epoch's seconds;
  pass:    per rank the median seconds of the scoring pass (all users, seen items filtered, lists copied to the host) after a
           2-epoch build with both feature sets;
  default: the B of fm.default_blocks for this matrix.
`--epochs N` timed sweeps per case (default 3); `--blocks 64,256` adds values of B.  The parameters move between the timed
sweeps.  Timings are synchronised; nothing here is part of bench.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from bench_coldstart import median_of, timed
from polara_amd import fm, pmf
from polara_amd.data import ArrayData
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

RANKS, SEED, ITEM_LABELS_PER_ROW, USER_LABELS_PER_ROW, REG = (10, 50), 0, 8, 3, 1e-10


def seeded_features(n_rows, n_labels, per_row, seed):
    from scipy.sparse import csr_matrix
    rng = np.random.RandomState(seed)
    cols = np.argsort(rng.rand(n_rows, n_labels), axis=1)[:, :per_row].ravel()     # `per_row` distinct labels per row
    rows = np.repeat(np.arange(n_rows), per_row)
    return csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_rows, n_labels))


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    reps = int(opt('--epochs', '3'))
    n_il, n_ul = int(opt('--item-labels', '1000')), int(opt('--user-labels', '200'))
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    u, i, v = np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64)
    A = ops.csr_from_coo(u, i, v, (n_users, n_items))
    nnz = int(A.nnz)
    mean = float(np.mean(ops.csr_values_host(A)))
    default = fm.default_blocks(nnz, n_users, n_items)
    hot_i, hot_u = seeded_features(n_items, n_il, ITEM_LABELS_PER_ROW, SEED), seeded_features(n_users, n_ul, USER_LABELS_PER_ROW, SEED + 1)
    adjust, gamma, step = fm.step_rule()
    out = dict(n_users=n_users, n_items=n_items, nnz=nnz, item_labels=n_il, item_labels_per_item=ITEM_LABELS_PER_ROW, user_labels=n_ul,
               user_labels_per_user=USER_LABELS_PER_ROW, rule=dict(adjust=adjust, gamma=gamma, step=step), plan={},
               epoch={r: {} for r in RANKS}, default=dict(blocks=default, rule='pmf.default_blocks (unmeasured for TCF)'))
    for B in sorted({default, 1024} | {int(x) for x in opt('--blocks', '').split(',') if x}):
        ops.fm_plan(A, B, hot_u, hot_i)
        plan, t_plan = timed(lambda: ops.fm_plan(A, B, hot_u, hot_i))
        out['plan'][B] = dict(seconds=round(t_plan, 5))
        sides = dict(none=dict(user=None, item=None), items=dict(user=None, item=plan['features']['item']), both=plan['features'])
        for rank in RANKS:
            P0, Q0 = pmf.initial_factors(n_users, n_items, rank, seed=SEED)
            Pp, Qp = ops.to_device(P0), ops.to_device(Q0)
            pmf_state = (ops.zeros(n_users, rank), ops.zeros(n_items, rank))
            sweep = lambda: float(ops.pmf_epoch(plan, Pp, Qp, step, REG, adjust='adagrad', state=pmf_state)[0].item())
            sweep()
            t_pmf = median_of(sweep, reps)
            del Pp, Qp, pmf_state
            for name, features in sides.items():
                this = dict(plan, features=features)
                with_u, with_i = features['user'] is not None, features['item'] is not None
                host = fm.initial_parameters(n_users, n_items, n_ul, n_il, rank, seed=SEED)
                P, E = ops.to_device(host[0]), ops.to_device(host[1])
                LU, LI = (ops.to_device(host[2]) if with_u else None), (ops.to_device(host[3]) if with_i else None)
                state = tuple(None if X is None else torch.zeros_like(X) for X in (P, E, LU, LI))
                work = (ops.empty(n_users, rank + 2) if with_u else None, ops.zeros(n_users, rank + 3) if with_u else None,
                        ops.empty(n_items, rank + 2) if with_i else None, ops.zeros(n_items, rank + 3) if with_i else None)
                sweep = lambda: float(ops.fm_epoch(this, mean, P, E, LU, LI, state, step, REG, REG, adjust=adjust, gamma=gamma,
                                                   work=work)[0].item())
                sse = sweep()
                t = median_of(sweep, reps)
                row = dict(seconds=round(t, 5), ratings_per_s=round(nnz / t, 1), first_rmse=round((sse / nnz) ** 0.5, 6),
                           pmf=round(t_pmf, 5), ratio=round(t / t_pmf, 3))
                labels = 0.0
                for side, L, SL, G in (('user', LU, state[2], work[1]), ('item', LI, state[3], work[3])):
                    if L is None:
                        continue
                    t_image = median_of(lambda: (ops.fm_label_image(this, side, L), ops.synchronize()), 5)
                    t_step = median_of(lambda: (ops.fm_label_step(this, side, G, L, SL, step, REG, REG, adjust=adjust, gamma=gamma),
                                                ops.synchronize()), 5)
                    row['%s_label_image_seconds' % side], row['%s_label_step_seconds' % side] = round(t_image, 6), round(t_step, 6)
                    labels += t_image + t_step
                if with_u or with_i:
                    row['label_share'] = round(B * labels / t, 4)
                out['epoch'][rank].setdefault(B, {})[name] = row
                del P, E, LU, LI, state, work
                torch.cuda.empty_cache()
        del plan, sides
        torch.cuda.empty_cache()
    out['pass'] = {}
    every_user = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    for rank in RANKS:
        m = fm.TuriFactorizationRecommender(ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=every_user), ops=ops,
                                            item_side_info=hot_i, user_side_info=hot_u)
        m.verbose, m.topk, m.max_iterations, m.rank, m.seed = False, 10, 2, rank, SEED
        _, t_build = timed(m.build)
        m.get_recommendations()
        out['pass'][rank] = dict(build_seconds=round(t_build, 4), blocks=m.build_stats['blocks'], rmse=[round(x, 6) for x in m.rmse_history],
                                 seconds=round(median_of(m.get_recommendations, 15), 6))
        del m
        torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'fm_bench_line.json'), 'w') as f:
        f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()

"""Contextual post-filtering (ItemPostFilteringMixin over SVDModel) on the ML-20M-shaped workload (synth.make_workload('ml20m'):
138 493 x 26 744, 2.0e7 ratings): rank 50, topk 10, one holdout item per user (its first stored interaction), ONE context of
20 values whose item lists grow geometrically from 50 to 13 000 items, every user with a value drawn uniformly.  Prints ONE
JSON line:
  plain_pass_s:   `get_recommendations` of the plain SVDModel (test CSR cached) — the figure to compare with the same script's
                  `--plain-only` run at the parent commit: the hook must not have changed it;
  context_pass_s: `get_recommendations` of the mixin (exact fold-in, the pass on ready-made query rows, the merge kernel);
  foldin_s, base_s: its parts in front of the merge: E = T V in fp64, the plain lists from E;
  merge_s, merge_ordered_s: pk_context_merge_f64 alone on those lists, workgroups in row order / users of one value next
                  to each other (`order`); the two are timed ALTERNATELY in one loop;
  item_rows_gb:   the bytes of item rows the merge reads (list entries x rank x 8), its lower bound on traffic;
  changed_lists, hr_at_10: how many lists the contexts changed and HR@10 with / without them (the values are random here).
Timings: the median of REPS synchronised calls after a warm-up call; (min, max) of every step under `spread`.
`--plain-only`: the plain part alone, importing nothing of the contextual layer (runs at a commit that has none).
`--out FILE` also writes the line to FILE."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from polara_amd import scoring
from polara_amd.data import ArrayData
from polara_amd.models import SVDModel
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

REPS = 15
SPREAD = {}


def record(name, ts):
    ts = sorted(ts)
    SPREAD[name] = [round(ts[0], 5), round(ts[-1], 5)]
    return ts[len(ts) // 2]


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def timed(fn, name, reps=REPS):
    out = fn()                                     # warm-up
    ts = []
    for _ in range(reps):
        out, t = clock(fn)
        ts.append(t)
    return out, record(name, ts)


def context_of(n_items, n_users, n_values=20, lo=50, hi=13000, seed=0):
    rng = np.random.default_rng(seed)
    sizes = np.unique(np.round(np.geomspace(lo, min(hi, n_items), n_values)).astype(np.int64))
    items = np.concatenate([rng.choice(n_items, s, replace=False) for s in sizes])
    values = np.repeat(np.arange(len(sizes)), sizes)
    return (items, values), rng.integers(0, len(sizes), n_users), sizes


def main():
    plain_only = '--plain-only' in sys.argv
    ops = HipOps('cuda:0')
    csr, cfg = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    rank, topk = 50, 10
    first = np.r_[True, u[1:] != u[:-1]]                      # triplets are sorted by user: its first entry is held out
    assert first.sum() == n_users
    train, holdout = (u[~first], i[~first], v[~first]), (u[first], i[first], v[first])
    out = dict(workload='ml20m', n_users=n_users, n_items=n_items, nnz=int(len(v)), rank=rank, topk=topk, reps=REPS)

    plain = SVDModel(ArrayData(train, n_users=n_users, n_items=n_items, holdout=holdout, warm_start=False), ops=ops)
    plain.verbose, plain.rank, plain.topk = False, rank, topk
    plain.build()
    plain_recs, t_plain = timed(plain.get_recommendations, 'plain_pass_s')
    out['plain_pass_s'] = round(t_plain, 5)

    if not plain_only:
        from polara_amd.contextual import ItemPostFilteringMixin
        from polara_amd.data import ItemPostFilteringArrayData

        class ContextualSVD(ItemPostFilteringMixin, SVDModel):
            pass
        mapping, user_values, sizes = context_of(n_items, n_users)
        data = ItemPostFilteringArrayData(train, n_users=n_users, n_items=n_items, holdout=holdout, warm_start=False,
                                          item_context_mapping={'genre': mapping}, holdout_context={'genre': user_values})
        m = ContextualSVD(data, ops=ops)
        m.verbose, m.rank, m.topk = False, rank, topk
        m.build()
        recs, t_ctx = timed(m.get_recommendations, 'context_pass_s')
        m.context_order_users = not m.context_order_users
        m._context_dev = None
        recs_other, t_ctx_other = timed(m.get_recommendations, 'context_pass_other_order_s')
        assert np.array_equal(recs, recs_other)
        m.context_order_users = not m.context_order_users
        m._context_dev = None

        T, _, _ = m._device_test_csr()
        image = m._item_factors_device()
        E, t_fold = timed(lambda: ops.spmm(T, image.fold_in), 'foldin_s')
        base, t_base = timed(lambda: scoring.recommend(ops, image, T, topk, True, queries=E), 'base_s')
        contexts, _ = m._context_images(T, lambda: np.arange(n_users))
        by_value = ops.to_device(np.argsort(ops.to_host(contexts[0].user_value), kind='stable').astype(np.int32))
        seen = (T.indptr, T.indices)
        merged = {None: ops.context_merge(image.V, E, seen, contexts, base)[0],               # warm-up of both
                  'o': ops.context_merge(image.V, E, seen, contexts, base, order=by_value)[0]}
        assert torch.equal(merged[None], merged['o'])
        assert np.array_equal(m._external_ids(merged[None], m._item_inv), recs)
        ts = {None: [], 'o': []}
        for _ in range(REPS):
            for key, order in ((None, None), ('o', by_value)):                              # alternating
                ts[key].append(clock(lambda: ops.context_merge(image.V, E, seen, contexts, base, order=order))[1])
        entries = int(sizes[user_values].sum())
        hold_items = holdout[1]
        out.update(context_pass_s=round(t_ctx, 5), context_pass_other_order_s=round(t_ctx_other, 5),
                   order_users_default=bool(m.context_order_users), foldin_s=round(t_fold, 5), base_s=round(t_base, 5),
                   merge_s=round(record('merge_s', ts[None]), 5), merge_ordered_s=round(record('merge_ordered_s', ts['o']), 5),
                   list_sizes=[int(s) for s in sizes], list_entries=entries, item_rows_gb=round(entries * rank * 8 / 1e9, 2),
                   changed_lists=int((recs != plain_recs).any(1).sum()),
                   hr_at_10=[round(float((plain_recs == hold_items[:, None]).any(1).mean()), 5),
                             round(float((recs == hold_items[:, None]).any(1).mean()), 5)])
    out['spread'] = SPREAD
    line = json.dumps(out)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()

"""Sampled-negatives evaluation (SVDModelSampled) on the ML-20M-shaped workload (synth.make_workload('ml20m'): 138 493 x
26 744, 2.0e7 ratings): rank 50, one holdout item per user (its first stored interaction) ranked against 999 sampled unseen
items, topk 10.  Prints ONE JSON line:
  build_s:      the PureSVD build;
  foldin_s:     P = T V for all users (the fp64 SpMM);
  relabel_s:    the test CSR renamed into the data's item ids for the sampler (once per test CSR: the model caches it);
  sample_s:     999 unseen items for every user (pk_sample_unseen, holdout matrix, seeds and the host check included);
  assemble_s:   the candidates `[holdout | unseen]` renamed into the model's item order and concatenated;
  candidates_s: the gathered product with the top-k fused in (pk_candidates_topk_f64) on those candidates;
  pass_s:       the whole `get_recommendations` (test CSR and its renamed image cached), users per second, and HR@10;
  numpy:        the NumPy restatement of the candidate pass (tests/sampled_reference.py: the same sums, the same selection)
                on a seeded sample of users on this host — seconds, users per second, and the sample rows whose device list
                and scores equal the host's exactly.
Timings: the median of REPS = 7 synchronised calls after one warm-up call (the first pays allocations and code loads); the
spread (min, max) of every step is printed next to it under `spread`.  `--out FILE` also writes the line to FILE."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

from polara_amd.data import RandomSampleArrayData
from polara_amd.ops import HipOps
from polara_amd.sampled import SVDModelSampled
from polara_amd.synth import make_workload, csr_to_coo_triplets
import sampled_reference as ref


REPS = 7
SPREAD = {}


def timed(fn, name=None, reps=REPS):
    out = fn()                                     # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    if name:
        SPREAD[name] = [round(ts[0], 5), round(ts[-1], 5)]
    return out, ts[len(ts) // 2]


def main():
    ops = HipOps('cuda:0')
    csr, cfg = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    rank, topk, n_unseen, n_sample = 50, 10, 999, 2048
    first = np.r_[True, u[1:] != u[:-1]]                      # triplets are sorted by user: its first entry is held out
    assert first.sum() == n_users
    data = RandomSampleArrayData((u[~first], i[~first], v[~first]), n_users=n_users, n_items=n_items,
                                 holdout=(u[first], i[first], v[first]), warm_start=False, seed=0)
    data.unseen_items_num = n_unseen
    m = SVDModelSampled(data, ops=ops)
    m.verbose, m.rank, m.topk = False, rank, topk
    _, t_build = timed(m.build, 'build_s', reps=3)
    out = dict(workload='ml20m', n_users=n_users, n_items=n_items, nnz=int(len(v)), rank=rank, topk=topk,
               candidates=1 + n_unseen, build_s=round(t_build, 4))

    T, _, _ = m._device_test_csr()
    fac = m._item_factors_device()
    P, t_fold = timed(lambda: ops.spmm(T, fac.fold_in), 'foldin_s')
    hold_items = m._holdout_items()
    T_ext, t_relabel = timed(lambda: ops.csr_relabel_cols(T, m._item_inv), 'relabel_s')
    unseen, t_sample = timed(lambda: m._sample(T_ext, hold_items, n_unseen), 'sample_s')
    cand, t_asm = timed(lambda: torch.cat([m._internal(hold_items), m._internal(unseen)], dim=1).contiguous(), 'assemble_s')
    (lists, _), t_cand = timed(lambda: ops.candidates_topk(P, fac.V, cand, topk), 'candidates_s')
    recs, t_pass = timed(m.get_recommendations, 'pass_s')
    assert np.array_equal(recs, ops.to_host(lists))
    m._recommendations = recs
    hr = m.evaluate('relevance')
    out.update(foldin_s=round(t_fold, 5), relabel_s=round(t_relabel, 5), sample_s=round(t_sample, 5), assemble_s=round(t_asm, 5),
               candidates_s=round(t_cand, 5), pass_s=round(t_pass, 5), reps=REPS,
               users_per_s=round(n_users / t_pass, 1), hr_at_10=round(float(hr[0]), 5))

    rows = np.sort(np.random.default_rng(0).choice(n_users, min(n_sample, n_users), replace=False))
    _, scores = ops.candidates_topk(P[rows].contiguous(), fac.V, cand[rows].contiguous(), topk, want_scores=True)
    Ph, Vh, ch = ops.to_host(P[rows]), ops.to_host(fac.V), ops.to_host(cand[rows])
    t0 = time.perf_counter()
    want_lists, want_scores = ref.candidates_topk(Ph, Vh, ch, topk)
    t_np = time.perf_counter() - t0
    out['numpy'] = dict(sample_users=len(rows), seconds=round(t_np, 4), users_per_s=round(len(rows) / t_np, 1),
                        exact_lists=int((recs[rows] == want_lists).all(1).sum()),
                        exact_score_rows=int((ops.to_host(scores) == want_scores).all(1).sum()))
    out['spread'] = SPREAD
    line = json.dumps(out)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()

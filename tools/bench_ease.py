"""EASE (EASEModel) on the ML-20M-shaped workload (synth.make_workload('ml20m'): 138 493 x 26 744, 2.0e7 ratings) at
lambda = 500, topk 10, every user a test user (its training row as known items).  Writes ONE JSON line to
profiles/ease_bench_line.json and prints it:
  build:  the four stages (gram, chol, trtri, weights: seconds, synchronised after each) and the whole build, from the
          second of two identical builds (the first pays allocations and code loads); TFLOP/s of trtri and of the weights
          product against n^3 / 3 flops each;
  score:  a full scoring pass over all users, seconds and users per second;
  cpu:    the NumPy / SciPy restatement (tests/ease_reference.py: dense Gram, np.linalg.inv, scaling) on the first
          --cpu-items items of the catalogue (default 4000: the full catalogue takes minutes), its seconds, the device
          build of the same subset and the distance of the two weight matrices.
Every device leg runs in a child process of its own under a time limit (--limit seconds, default 600): a leg that
fails or runs out of time ends the tool with its exit status, and nothing else is started on the device."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'profiles', 'ease_bench_line.json')
LAMBDA = 500.0
TOPK = 10


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _model(n_items_cap=None):
    import numpy as np
    from polara_amd import EASEModel
    from polara_amd.data import ArrayData
    from polara_amd.ops import HipOps
    from polara_amd.synth import make_workload, csr_to_coo_triplets
    ops = HipOps('cuda:0')
    csr, _ = make_workload('ml20m', device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    if n_items_cap is not None and n_items_cap < n_items:
        keep = i < n_items_cap
        u, i, v, n_items = u[keep], i[keep], v[keep], int(n_items_cap)
    hold = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False)
    m = EASEModel(data, ops=ops)
    m.verbose, m.topk, m.regularization = False, TOPK, LAMBDA
    return m, (u, i, v, (n_users, n_items))


def leg_build():
    m, (_, _, v, (n_users, n_items)) = _model()
    m.build()
    m.build()
    s = m.build_stats
    flops = n_items ** 3 / 3
    return dict(workload='ml20m', n_users=n_users, n_items=n_items, nnz=int(len(v)), regularization=LAMBDA,
                build=dict(gram_s=round(s['gram_s'], 4), chol_s=round(s['chol_s'], 4), trtri_s=round(s['trtri_s'], 4),
                           weights_s=round(s['weights_s'], 4), build_s=round(m.training_time[-1], 4),
                           trtri_TFLOPs=round(flops / s['trtri_s'] / 1e12, 2),
                           weights_TFLOPs=round(flops / s['weights_s'] / 1e12, 2),
                           image_bytes=int(s['image_bytes']), chol_image_bytes=int(s['chol_image_bytes'])))


def leg_score():
    import torch
    m, (_, _, _, (n_users, _)) = _model()
    m.build()
    m.get_recommendations()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs = m.get_recommendations()
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    return dict(score=dict(topk=TOPK, pass_s=round(t, 4), users_per_s=round(n_users / t, 1), pads=int((recs < 0).sum())))


def leg_cpu():
    import numpy as np
    import ease_reference as ref
    n_sub = _arg('--cpu-items', 4000)
    m, (u, i, v, shape) = _model(n_sub)
    A = ref.training_matrix(np.stack([u, i], 1), v, shape)
    t0 = time.perf_counter()
    B_ref, _ = ref.ease_weights(A, LAMBDA)
    t_cpu = time.perf_counter() - t0
    m.build()
    m.build()
    B = m.ops.to_host(m.item_weights)[:, :shape[1]]
    return dict(cpu=dict(items=int(shape[1]), nnz=int(len(v)), numpy_s=round(t_cpu, 3), device_build_s=round(m.training_time[-1], 4),
                         max_abs_diff=float(np.abs(B - B_ref).max()), max_abs_ref=float(np.abs(B_ref).max())))


LEGS = {'build': leg_build, 'score': leg_score, 'cpu': leg_cpu}


def main():
    if '--leg' in sys.argv:                                    # a child: one leg, its JSON on the last line
        print(json.dumps(LEGS[_arg('--leg', '')]()))
        return 0
    limit = _arg('--limit', 600)
    out = {}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg] + [a for a in sys.argv[1:]]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write('bench_ease: the %s leg ran past its limit of %d s; stopping\n' % (leg, limit))
            return 124
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.stderr.write('bench_ease: the %s leg failed with status %d; stopping\n' % (leg, r.returncode))
            return r.returncode if r.returncode > 0 else 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    with open(OUT, 'w') as f:
        f.write(line + '\n')
    print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

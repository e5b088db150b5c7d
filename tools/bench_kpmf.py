"""KernelizedPMF on the ML-20M-shaped planted matrix (138 493 x 26 744, 2.0e7 ratings), rank 10, with seeded symmetric kernel
matrices K = I + 0.1 R of about 8 (users) and about 32 (items) neighbours per row.  Prints ONE JSON line (and writes it to
`--out FILE` when given):
  epoch:    per B the median seconds of one KPMF sweep (pk_kpmf_epoch_f64: per stratum one sweep launch and one snapshot
            refresh) and of one PMF sweep on THE SAME plan in the same run, the two alternated, and their ratio;
  snapshot: the share of the snapshot copies in the device time of a KPMF epoch at `--profile-blocks` (default 1024), from a
            `rocprofv3 --kernel-trace --stats` run of a child process of its own (this file with `--child B`); skipped with
            `--no-profile` or when rocprofv3 is not there;
  rmse:     on the ML-1M-shaped matrix (kernels of the same recipe) the RMSE history of `--rmse-epochs` (default 5) epochs at
            each B against B = 1 (the reference's order): what the stale neighbour rows of a blocked epoch cost.
`--blocks 64,256,1024,2048`, `--epochs N` timed sweeps per B (default 3).  `--markdown` prints the table of DESIGN.md to stderr.
Timings are synchronised; nothing here is part of bench.py."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import scipy.sparse as sps
import torch

from bench_coldstart import timed
from polara_amd import pmf
from polara_amd.ops import HipOps
from polara_amd.synth import make_workload, csr_to_coo_triplets

RANK, ETA, LAMBD, GAMMA = 10, 0.005, 0.5, 0.1


def kernel_matrix(n, neighbours, seed):
    """K = I + GAMMA * R for a seeded symmetric relation R (unit diagonal) with about `neighbours` off-diagonal entries a row"""
    rng = np.random.RandomState(seed)
    m = n * neighbours // 2
    a, b = rng.randint(n, size=m), rng.randint(n, size=m)
    keep = a != b
    upper = sps.csr_matrix((rng.rand(int(keep.sum())), (np.minimum(a, b)[keep], np.maximum(a, b)[keep])), shape=(n, n))
    upper.sum_duplicates()
    R = (upper + upper.T).tocsr()
    R.setdiag(1)
    return sps.eye(n).tocsr() + GAMMA * R


def workload(ops, name):
    csr, _ = make_workload(name, device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    A = ops.csr_from_coo(np.asarray(u), np.asarray(i), np.asarray(v, dtype=np.float64), (n_users, n_items))
    return A, n_users, n_items, kernel_matrix(n_users, 8, 11), kernel_matrix(n_items, 32, 12)


def sweeps(ops, plan, n_users, n_items):
    """(kpmf, pmf): two closures that each run one epoch from factors of their own"""
    out = []
    for kind in ('kpmf', 'pmf'):
        P0, Q0 = pmf.initial_factors(n_users, n_items, RANK, seed=0)
        P, Q = ops.to_device(P0), ops.to_device(Q0)
        if kind == 'kpmf':
            snaps = (ops.empty(n_users, RANK), ops.empty(n_items, RANK))
            out.append(lambda P=P, Q=Q, snaps=snaps: float(ops.kpmf_epoch(plan, P, Q, ETA, LAMBD, snapshots=snaps)[0].item()))
        else:
            out.append(lambda P=P, Q=Q: float(ops.pmf_epoch(plan, P, Q, ETA, LAMBD)[0].item()))
    return out


def child(B):
    """what the profiler wraps: one plan and three KPMF epochs at B, nothing else"""
    ops = HipOps('cuda:0')
    A, n_users, n_items, Ku, Ki = workload(ops, 'ml20m')
    plan = ops.kpmf_plan(A, B, Ku, Ki)
    kpmf_epoch, _ = sweeps(ops, plan, n_users, n_items)
    for _ in range(3):
        kpmf_epoch()
    torch.cuda.synchronize()


def snapshot_share(B):
    """device time of the snapshot copies / device time of all kpmf kernels, from the kernel statistics of a profiled child"""
    if shutil.which('rocprofv3') is None:
        return dict(skipped='rocprofv3 not found')
    tmp = tempfile.mkdtemp(prefix='kpmf_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable,
               os.path.abspath(__file__), '--child', str(B)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=tmp)
        if r.returncode != 0:
            return dict(skipped='the profiled child ended with %d: %s' % (r.returncode, r.stderr[-300:]))
        total = {}
        for path in glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True):
            with open(path, newline='') as f:
                for row in csv.DictReader(f):
                    # (the child runs KPMF epochs only: every pmf_stratum_kernel instance in its trace is a kernelized one)
                    for key in ('kpmf_snapshot_kernel', 'pmf_stratum_kernel', 'pmf_sse_kernel'):
                        if key in row['Name']:
                            total[key] = total.get(key, 0.) + float(row['TotalDurationNs'])
        if 'pmf_stratum_kernel' not in total:
            return dict(skipped='no kernel statistics were written')
        every = sum(total.values())
        return dict(blocks=B, epochs=3, snapshot_ms=round(total.get('kpmf_snapshot_kernel', 0.) / 1e6, 3),
                    sweep_ms=round(total['pmf_stratum_kernel'] / 1e6, 3), share=round(total.get('kpmf_snapshot_kernel', 0.) / every, 4))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def rmse_histories(ops, blocks, epochs):
    A, n_users, n_items, Ku, Ki = workload(ops, 'ml1m')
    nnz = int(A.nnz)
    out = {}
    for B in [1] + [b for b in blocks if b <= min(n_users, n_items)]:
        plan = ops.kpmf_plan(A, B, Ku, Ki)
        kpmf_epoch, _ = sweeps(ops, plan, n_users, n_items)
        out[B] = [round((kpmf_epoch() / nnz) ** 0.5, 6) for _ in range(epochs)]
    return dict(n_users=n_users, n_items=n_items, nnz=nnz, epochs=epochs, history=out)


def markdown(out):
    rows = ['| B | KPMF epoch, ms | PMF epoch, ms | ratio | samples / s |', '|---|---|---|---|---|']
    for B, r in out['epoch'].items():
        rows.append('| %s | %.2f | %.2f | %.2f | %.3g |' % (B, 1e3 * r['kpmf_seconds'], 1e3 * r['pmf_seconds'], r['ratio'],
                                                             r['kpmf_samples_per_s']))
    return '\n'.join(rows)


def main():
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    if '--child' in argv:
        return child(int(opt('--child', '1024')))
    blocks = [int(x) for x in opt('--blocks', '64,256,1024,2048').split(',')]
    reps = int(opt('--epochs', '3'))
    ops = HipOps('cuda:0')
    A, n_users, n_items, Ku, Ki = workload(ops, 'ml20m')
    nnz = int(A.nnz)
    out = dict(rank=RANK, n_users=n_users, n_items=n_items, nnz=nnz, epoch={},
               kernels=dict(gamma=GAMMA, user_neighbours=round((Ku.nnz - n_users) / n_users, 2),
                            item_neighbours=round((Ki.nnz - n_items) / n_items, 2)))
    for B in blocks:
        plan, t_plan = timed(lambda: ops.kpmf_plan(A, B, Ku, Ki))
        kpmf_epoch, pmf_epoch = sweeps(ops, plan, n_users, n_items)
        kpmf_epoch(), pmf_epoch()                                          # first launches
        times = {'kpmf': [], 'pmf': []}
        for _ in range(reps):                                              # alternated: both see the same machine
            times['kpmf'].append(timed(kpmf_epoch)[1])
            times['pmf'].append(timed(pmf_epoch)[1])
        tk, tp = float(np.median(times['kpmf'])), float(np.median(times['pmf']))
        out['epoch'][B] = dict(plan_seconds=round(t_plan, 4), kpmf_seconds=round(tk, 5), pmf_seconds=round(tp, 5), ratio=round(tk / tp, 2),
                               kpmf_samples_per_s=round(nnz / tk, 1))
        del plan, kpmf_epoch, pmf_epoch
        torch.cuda.empty_cache()
    del A
    torch.cuda.empty_cache()
    if '--no-profile' not in argv:
        out['snapshot'] = snapshot_share(int(opt('--profile-blocks', '1024')))
    rmse_epochs = int(opt('--rmse-epochs', '5'))
    if rmse_epochs:
        out['rmse'] = rmse_histories(ops, blocks, rmse_epochs)
    line = json.dumps(out)
    print(line, flush=True)
    if '--out' in argv:
        with open(opt('--out', None), 'w') as f:
            f.write(line + '\n')
    if '--markdown' in argv:
        print(markdown(out), file=sys.stderr)


if __name__ == '__main__':
    main()

"""SLIM (SLIMModel) on the ML-1M- and ML-20M-shaped workloads (synth.make_workload: 6 040 x 3 706 with 1.0e6 ratings,
138 493 x 26 744 with 2.0e7) at the model's default settings (l1 = 1, l2 = 10, tolerance 1e-4, at most 100 sweeps,
positive weights), topk 10, every user a test user (its training row as known items).  Writes ONE JSON line to
profiles/slim_bench_line.json and prints it:
  ml1m:        the three stages of the build (gram, solve, csr: seconds, synchronised after each) and the whole build, from
               the second of two identical builds (the first pays allocations and code loads); the weights (entries, fill),
               the sweeps (max, mean, columns at the cap); a full scoring pass in both branches, seconds and users per second;
  ml1m_global: the solve stage again with the residual rows forced into HBM (pk_set_option('slim_r_global', 1));
  ml20m:       the Gram image and the solve of --columns target columns (default 2048, two batches, spread evenly over the
               catalogue's first batch starts), seconds per column, and the projection of that to all columns — a
               projection, not a measurement; `--full` builds the whole model instead and reports it like ml1m, as
               `ml20m_full` (minutes).
`--only leg[,leg]` runs those legs alone and updates their keys in the existing line.
Every leg runs in a child process of its own under a time limit (--limit seconds, default 600): a leg that fails or runs
out of time ends the tool with its exit status, and nothing else is started on the device."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'slim_bench_line.json')
TOPK = 10


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _model(workload):
    import numpy as np
    from polara_amd import SLIMModel
    from polara_amd.data import ArrayData
    from polara_amd.ops import HipOps
    from polara_amd.synth import make_workload, csr_to_coo_triplets
    ops = HipOps('cuda:0')
    csr, _ = make_workload(workload, device='cuda:0')
    u, i, v = csr_to_coo_triplets(csr)
    n_users, n_items = (int(x) for x in csr['shape'])
    del csr
    hold = (np.arange(n_users), np.zeros(n_users, np.int64), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False)
    m = SLIMModel(data, ops=ops)
    m.verbose, m.topk = False, TOPK
    return m, (u, i, v, (n_users, n_items))


def _build_record(m):
    s = m.build_stats
    return dict(gram_s=round(s['gram_s'], 4), solve_s=round(s['solve_s'], 4), csr_s=round(s['csr_s'], 4),
                build_s=round(m.training_time[-1], 4), nnz_weights=s['nnz_weights'], fill=round(s['fill'], 6),
                max_sweeps=s['max_sweeps'], mean_sweeps=round(s['mean_sweeps'], 2), capped_columns=s['capped_columns'],
                column_batch=s['column_batch'])


def _settings(m):
    return dict(l1=m.l1_regularization, l2=m.l2_regularization, tolerance=m.tolerance, max_sweeps=m.max_sweeps,
                positive=m.positive)


def _full(workload):
    import torch
    m, (_, _, v, (n_users, n_items)) = _model(workload)
    m.build()
    m.build()
    out = dict(n_users=n_users, n_items=n_items, nnz=int(len(v)), settings=_settings(m), build=_build_record(m), score={})
    for dense in (True, False):
        m.dense_output = dense
        m.get_recommendations()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs = m.get_recommendations()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        out['score']['dense' if dense else 'sparse'] = dict(topk=TOPK, pass_s=round(t, 4), users_per_s=round(n_users / t, 1),
                                                            pads=int((recs < 0).sum()))
    return out


def leg_ml1m():
    return dict(ml1m=_full('ml1m'))


def leg_ml1m_global():
    from polara_amd import _lib
    _lib.check(_lib.load().pk_set_option(b'slim_r_global', 1, 0), 'pk_set_option')
    m, _ = _model('ml1m')
    m.build()
    m.build()
    return dict(ml1m_global=dict(solve_s=round(m.build_stats['solve_s'], 4), build_s=round(m.training_time[-1], 4)))


def leg_ml20m():
    if '--full' in sys.argv:
        return dict(ml20m_full=_full('ml20m'))
    from polara_amd import slim
    m, (u, i, v, (n_users, n_items)) = _model('ml20m')
    ops = m.ops
    A = ops.csr_from_coo(u, i, v, (n_users, n_items))
    ops.synchronize()
    t0 = time.perf_counter()
    G = ops.slim_gram(A)
    ops.synchronize()
    gram_s = time.perf_counter() - t0
    batch = slim.default_batch_columns(n_items, ops.free_bytes())
    n_batches = max(1, _arg('--columns', 2048) // batch)
    total_batches = -(-n_items // batch)
    starts = [b * (total_batches // n_batches) * batch for b in range(n_batches)]
    block = ops.empty(batch, slim.gram_leading_dim(n_items))
    solve_s = csr_s = 0.0
    nnz, sweeps = 0, []
    for rep in range(2):                                     # the first round pays allocations and code loads
        solve_s = csr_s = 0.0
        nnz, sweeps = 0, []
        for j0 in starts:
            nc = min(batch, n_items - j0)
            t0 = time.perf_counter()
            Wt, sw = ops.slim_solve(G, n_items, j0, nc, m.l1_regularization, m.l2_regularization, m.tolerance, m.max_sweeps,
                                    m.positive, out=block)
            ops.synchronize()
            t1 = time.perf_counter()
            ptr, _, _ = ops.slim_csr(Wt, n_items)
            ops.synchronize()
            solve_s, csr_s = solve_s + t1 - t0, csr_s + time.perf_counter() - t1
            nnz += int(ptr[-1].item())
            sweeps.append(ops.to_host(sw))
        if rep == 0 and solve_s > 60:
            break                                            # a slow solve is not run twice
    import numpy as np
    sweeps = np.concatenate(sweeps)
    cols = len(sweeps)
    return dict(ml20m=dict(n_users=n_users, n_items=n_items, nnz=int(len(v)), settings=_settings(m), gram_s=round(gram_s, 4),
                           sample=dict(columns=cols, column_batch=int(batch), starts=starts, solve_s=round(solve_s, 4),
                                       csr_s=round(csr_s, 4), solve_ms_per_column=round(1e3 * solve_s / cols, 4),
                                       nnz_weights=nnz, fill=round(nnz / float(cols * n_items), 6),
                                       max_sweeps=int(sweeps.max()), mean_sweeps=round(float(sweeps.mean()), 2),
                                       capped_columns=int((sweeps >= m.max_sweeps).sum())),
                           projected_solve_s=round(solve_s / cols * n_items, 2)))


LEGS = {'ml1m': leg_ml1m, 'ml1m_global': leg_ml1m_global, 'ml20m': leg_ml20m}


def main():
    if '--leg' in sys.argv:                                    # a child: one leg, its JSON on the last line
        print(json.dumps(LEGS[_arg('--leg', '')]()))
        return 0
    limit = _arg('--limit', 600)
    out = {}
    if '--only' in sys.argv and os.path.exists(OUT):
        with open(OUT) as f:
            out = json.loads(f.read())
    for leg in LEGS:
        if '--only' in sys.argv and leg not in _arg('--only', '').split(','):
            continue
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg] + [a for a in sys.argv[1:]]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write('bench_slim: the %s leg ran past its limit of %d s; stopping\n' % (leg, limit))
            return 124
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.stderr.write('bench_slim: the %s leg failed with status %d; stopping\n' % (leg, r.returncode))
            return r.returncode if r.returncode > 0 else 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    with open(OUT, 'w') as f:
        f.write(line + '\n')
    print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

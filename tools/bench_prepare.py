"""RecommenderArrayData.prepare() on the ML-20M-shaped workload (synth.make_workload('ml20m'): 138 493 x 26 744, 2.0e7
ratings, rows shuffled, external ids with gaps) in four configurations: state 4 (warm_start, test_ratio 0.2, fold 5,
holdout 3) and state 3 (the same with warm_start=False), each with the top-rated and with a random holdout.  Writes ONE JSON
line to profiles/prepare_bench_line.json and prints it:
  device: the construction (upload, user grouping: unique ids, duplicate check, stable sort by user) once, then per
          configuration the stages of a full prepare() (keys and selection, partition, indices and filters, download:
          seconds, synchronised after each, from a second run) and its wall time without the synchronisations;
  numpy:  the same object on PrepareNumpyOps (the NumPy operator set of the package, which the tests hold bit-equal to
          the twin of tests/prepare_reference.py; the twin itself walks the users one by one and is not a fair clock),
          on the same box: construction and per-configuration prepare(), seconds;
  ratio:  numpy total / device total, construction included, per configuration.
Each leg runs in a child process of its own under a time limit (--limit seconds, default 900): a leg that fails or runs
out of time ends the tool with its exit status, and nothing else is started on the device."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'prepare_bench_line.json')
BASE = dict(test_ratio=0.2, test_fold=5, holdout_size=3)
CONFIGS = {'state4_top': dict(BASE), 'state4_random': dict(BASE, random_holdout=True),
           'state3_top': dict(BASE, warm_start=False), 'state3_random': dict(BASE, warm_start=False, random_holdout=True)}


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _columns():
    import numpy as np
    from polara_amd.synth import make_workload, csr_to_coo_triplets
    csr, _ = make_workload(_arg('--workload', 'ml20m'), device='cuda:0', scale=_arg('--scale', 1.0))
    u, i, v = csr_to_coo_triplets(csr)
    rng = np.random.default_rng(0)
    p = rng.permutation(len(u))
    return u[p] * 3 + 11, i[p] * 2 + 5, v[p], tuple(int(x) for x in csr['shape'])


def _sync(ops):
    if getattr(ops, 'device', None) is not None:
        import torch
        torch.cuda.synchronize()


def _run(ops):
    from polara_amd.prepare import RecommenderArrayData
    users, items, fb, shape = _columns()
    out = dict(n_users=shape[0], n_items=shape[1], nnz=int(len(users)))
    RecommenderArrayData.profile = True
    RecommenderArrayData(users, items, fb, seed=0, ops=ops)                # first: allocations and code loads
    _sync(ops)
    t0 = time.perf_counter()
    data = RecommenderArrayData(users, items, fb, seed=0, ops=ops)
    _sync(ops)
    out['construct_s'] = round(time.perf_counter() - t0, 4)
    out['construct_stages'] = {k: round(v, 4) for k, v in data.timings.items()}
    out['configs'] = {}
    for name, config in CONFIGS.items():
        res = {}
        for leg in ('warm', 'stages', 'wall'):
            data.profile = leg == 'stages'
            data.set_configuration(dict(RecommenderArrayData.default_configuration(), **config))
            data._change_properties.add('init')                           # a full update every time
            data.timings = {}
            _sync(ops)
            t0 = time.perf_counter()
            data.prepare()
            _sync(ops)
            t = time.perf_counter() - t0
            if leg == 'stages':
                res['stages'] = {k: round(v, 4) for k, v in data.timings.items()}
            elif leg == 'wall':
                res['prepare_s'] = round(t, 4)
        res['training_rows'] = int(len(data.training.userid))
        res['holdout_rows'] = int(len(data.test.holdout.userid))
        res['total_s'] = round(out['construct_s'] + res['prepare_s'], 4)
        out['configs'][name] = res
    return out


def leg_device():
    from polara_amd.ops import HipOps
    return dict(device=_run(HipOps('cuda:0')))


def leg_numpy():
    from polara_amd.prepare import PrepareNumpyOps
    return dict(numpy=_run(PrepareNumpyOps()))


LEGS = {'device': leg_device, 'numpy': leg_numpy}


def main():
    if '--leg' in sys.argv:                                    # a child: one leg, its JSON on the last line
        print(json.dumps(LEGS[_arg('--leg', '')]()))
        return 0
    limit = _arg('--limit', 900)
    out = {}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', leg] + [a for a in sys.argv[1:]]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write('bench_prepare: the %s leg ran past its limit of %d s; stopping\n' % (leg, limit))
            return 124
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.stderr.write('bench_prepare: the %s leg failed with status %d; stopping\n' % (leg, r.returncode))
            return r.returncode if r.returncode > 0 else 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    out['ratio_numpy_over_device'] = {name: round(out['numpy']['configs'][name]['total_s'] / out['device']['configs'][name]['total_s'], 2)
                                      for name in CONFIGS}
    for name in CONFIGS:
        assert out['numpy']['configs'][name]['training_rows'] == out['device']['configs'][name]['training_rows'], name
    line = json.dumps(out)
    with open(OUT, 'w') as f:
        f.write(line + '\n')
    print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

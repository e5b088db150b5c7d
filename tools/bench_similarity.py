"""Item similarity matrices built on the device (polara_amd/similarity.py on csrc/spgemm.hip) against SciPy on the same box,
on the seeded features of tools/bench_coldstart.py::item_features (26 744 items x 3 000 labels, ~8 per item) and, for
`cross_similarity`, on its 20 % cold split (cold items x training items).  Prints ONE JSON line; per kind:
  device:    seconds of the whole call with the result on the host (the second of two calls, synchronised), split into
             `prepare_s` (host vectors, upload, scaling, transpose, plus everything not listed below), `count_s` (the count
             pass and the scan of its counts: one library call), `fill_s` (the fill pass) and `download_s` (the three arrays
             to the host and the SciPy wrapper);
  s:         entries and fill of the result;
  scipy_s:   the reference's expression restated in SciPy (tests/similarity_reference.py) on the host, and for 'cosine' also
             the plain product of tools/bench_coldstart.py::cosine (`scipy_plain_s`);
  bit_equal: whether the device result equals the restated expression bit for bit.
The interpreted weighted Jaccard of the reference is far too slow for the full size: 'jaccard-weighted' is run, on the device
and on the host, on the first 2 000 items only, and the line says so (`items`)."""
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

import similarity_reference as res
from bench_coldstart import cosine, item_features
from polara_amd import similarity as ps
from polara_amd.ops import HipOps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def device_run(ops, build):
    """`build(device=True)` -> DeviceCSR.  The stage split of one call and the host matrix."""
    build(device=True)                                    # pays allocations and code loads
    ops.timers = {}
    S, t_build = wall(lambda: build(device=True))
    timers, ops.timers = ops.timers, None
    ms = {k: sum(e0.elapsed_time(e1) for e0, e1, _ in v) for k, v in timers.items()}
    host, t_down = wall(lambda: ps._finish(S, False))
    count, fill = ms.get('spgemm_count', 0.0) / 1e3, ms.get('spgemm_fill', 0.0) / 1e3
    n_rows, n_cols = S.shape
    return host, dict(total_s=round(t_build + t_down, 4), prepare_s=round(t_build - count - fill, 4), count_s=round(count, 5),
                      fill_s=round(fill, 5), transpose_s=round(ms.get('transpose', 0.0) / 1e3, 5), download_s=round(t_down, 4)), \
        dict(shape=[n_rows, n_cols], nnz=int(host.nnz), fill=round(host.nnz / float(n_rows * n_cols), 6))


def main():
    ops = HipOps('cuda:0')
    F = item_features(26744)
    n_items = F.shape[0]
    cold = np.sort(np.random.RandomState(0).permutation(n_items)[:n_items // 5])
    is_cold = np.zeros(n_items, dtype=bool)
    is_cold[cold] = True
    Ft, Fc = F[~is_cold].tocsr(), F[cold].tocsr()
    out = dict(n_items=n_items, n_labels=int(F.shape[1]), feature_nnz=int(F.nnz), n_cold=int(len(cold)))
    for kind in ('cosine', 'tfidf-cosine', 'jaccard'):
        host, dev, s = device_run(ops, lambda device, kind=kind: ps.similarity(F, kind, ops=ops, device=device))
        want, t_ref = wall(lambda: res.similarity(F, kind, True))
        out[kind] = dict(device=dev, s=s, scipy_s=round(t_ref, 4), bit_equal=bool(res.same_bits(host, want)),
                         speedup=round(t_ref / dev['total_s'], 2))
        if kind == 'cosine':
            out[kind]['scipy_plain_s'] = round(wall(lambda: cosine(F))[1], 4)
        print(kind, json.dumps(out[kind]), file=sys.stderr, flush=True)
    for kind in ('cosine', 'jaccard'):
        host, dev, s = device_run(ops, lambda device, kind=kind: ps.cross_similarity(Fc, Ft, kind, ops=ops, device=device))
        want, t_ref = wall(lambda: res.cross(Fc, Ft, kind))
        out['cross ' + kind] = dict(device=dev, s=s, scipy_s=round(t_ref, 4), bit_equal=bool(res.same_bits(host, want)),
                                    speedup=round(t_ref / dev['total_s'], 2))
        print('cross', kind, json.dumps(out['cross ' + kind]), file=sys.stderr, flush=True)
    # weighted Jaccard: seeded non-binary weights on a 2 000-item subset (the host loop is interpreted)
    W = F[:2000].tocsr().copy()
    W.data = np.random.default_rng(5).integers(1, 30, W.nnz) * 0.1
    host, dev, s = device_run(ops, lambda device: ps.jaccard_similarity_weighted(W, ops=ops, device=device))
    want, t_ref = wall(lambda: res.jaccard_weighted(W, True))
    out['jaccard-weighted'] = dict(items=2000, note='2 000-item subset: the host loop is interpreted', device=dev, s=s,
                                   scipy_s=round(t_ref, 4), bit_equal=bool(res.same_bits(host, want)),
                                   speedup=round(t_ref / dev['total_s'], 2))
    print(json.dumps(out))


if __name__ == '__main__':
    main()

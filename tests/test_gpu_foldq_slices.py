"""-m gpu: the packed fold-in with several row tasks per wave (csrc/foldq.hip: fold_q20_kernel<VT, L, U, T>, T = 2 and 4, through
pk_fold_q20_sliced with T forced), on the ladder, the hand-made image and the reference of test_gpu_foldq_instances.

A wave of T slices runs as long as its longest task, so what can go wrong is what the slices do NOT share: a slice past its own
end that still carries a weight (the canary, item 0, shows it as about 2^31), a shuffle that leaves its slice, a slice beyond
n_tasks that stores, a reduction that crosses slices.  The ladder in its row order puts rows of r, r + 1 (, r + 2, r + 3)
entries, the empty rows next to the 1500-entry one and the halves of split rows into one wave — the worst mix of slice lengths
the mapping meets; the product on the hand-made image does not depend on the summation order and is compared bit for bit.

  branch                                                   ids that reach it
  T = 2, 4 at L = 2, 4, 8; T = 2 at L = 16                 T{2,4}_vals*_L{2,4,8}_K{12,25,49,50}_split*, T2_vals*_L16_K{97,101}_split*
  slices beyond n_tasks (n_tasks = 1, 2, 3 mod 4)          ..._rows10to15 / 10to16 / 10to17
  a wave of empty tasks only, a launch of one task         ..._rows210to212, ..._rows100to101, ..._rows0to1
  the clamp of T to the lane class                         clamped_K{101,202}
  counters, n_tasks == 0, n_long == 0                      ..._zero*_{full,nolong,notasks}
  the refusals                                             refused_T{3,8,0}"""
import numpy as np
import pytest
import torch

import q20_reference as q20
from test_gpu_foldq_instances import (N_ROWS, SENTINEL, SUBSET, check_fold, encoded_image, exact_image, fold_ladder, fold_subset,
                                      kx_of, lib_kappa, out_buffer, reference, rounded_host)      # (ladder: fold_host, image_host)

pytestmark = pytest.mark.gpu

SLICED = [(T, K) for K in (12, 25, 49, 50) for T in (2, 4)] + [(2, 97), (2, 101)]


def sliced_id(T, vbits, K, split=256, tail=''):
    return 'T%d_vals%d_L%d_K%d_split%d%s' % (T, vbits, q20.lanes(K), K, split, tail)


def call_sliced(ops, A, image, K, out, T, rows=None, counters=None):
    """pk_fold_q20_sliced itself, `tasks_per_wave` as given; returns the entry's return code"""
    from polara_amd.ops import _ptr
    img, tab = image
    Kx = out.shape[1]
    t0, n_tasks, l0, n_long = (0, A.n_tasks, 0, A.n_long) if rows is None else A.task_range(*rows)
    p = A.plan
    zero = (None, 0) if counters is None else (_ptr(counters), int(counters.numel()))
    return ops.lib.pk_fold_q20_sliced(
        ops.stream(), n_tasks, _ptr(p['task_row'], t0), _ptr(p['task_begin'], t0), _ptr(p['task_end'], t0), _ptr(p['task_slot'], t0),
        n_long, _ptr(p['long_row'], l0), _ptr(p['long_slot_begin'], l0), _ptr(p['long_slot_end'], l0), _ptr(A.indices),
        _ptr(A.values), A.val_kind, _ptr(img), _ptr(tab), int(A.shape[1]), int(K), int(Kx), _ptr(out), out.stride(0),
        _ptr(A.partial(Kx)), *zero, int(T))


# ---- exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,vbits,K,split', [pytest.param(T, vb, K, sp, id=sliced_id(T, vb, K, sp))
                                             for T, K in SLICED for sp in (256, 64, 2048) for vb in (32, 64)])
def test_sliced_exact(hip_ops, T, vbits, K, split):
    """the unsorted ladder under the three plans, to the last bit, into a strided view of a buffer of sentinels"""
    Kx = kx_of(K)
    A = fold_ladder(hip_ops, vbits, split)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    assert call_sliced(hip_ops, A, exact_image(hip_ops, K), K, out, T) == 0
    check_fold(hip_ops, buf, K, Kx, reference(K, split, lib_kappa(hip_ops, K)))


ROW_RANGES = [(10, 15), (10, 16), (10, 17), (150, 209), (N_ROWS - 2, N_ROWS), (100, 101), (0, 1)]


@pytest.mark.parametrize('T,vbits,K,lo,hi', [pytest.param(T, vb, K, lo, hi, id=sliced_id(T, vb, K, tail='_rows%dto%d' % (lo, hi)))
                                             for T, K in ((2, 50), (4, 50), (4, 12), (2, 101)) for vb in (32, 64)
                                             for lo, hi in ROW_RANGES])
def test_sliced_row_ranges(hip_ops, T, vbits, K, lo, hi):
    """launches of 5, 6 and 7 tasks (the last wave holds slices beyond n_tasks), of 68 with six split rows, of the two trailing
    empty rows only, of one task and of one empty task: the rows of the range are the reference's, every other row keeps
    its sentinels"""
    Kx = kx_of(K)
    A = fold_ladder(hip_ops, vbits)
    n_tasks = A.task_range(lo, hi)[1]
    assert n_tasks == {(10, 15): 5, (10, 16): 6, (10, 17): 7, (150, 209): 68, (N_ROWS - 2, N_ROWS): 2, (100, 101): 1, (0, 1): 1}[lo, hi]
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    assert call_sliced(hip_ops, A, exact_image(hip_ops, K), K, out, T, rows=(lo, hi)) == 0
    inside = (np.arange(N_ROWS) >= lo) & (np.arange(N_ROWS) < hi)
    check_fold(hip_ops, buf, K, Kx, reference(K, 256, lib_kappa(hip_ops, K)), rows=inside)


# ---- the counters ---------------------------------------------------------------------------------------------------------
ZERO_MODES = {'full': None, 'nolong': (10, 150), 'notasks': (5, 5)}


@pytest.mark.parametrize('T,zero_n,mode', [pytest.param(T, z, m, id=sliced_id(T, 32, 50, tail='_zero%d_%s' % (z, m)))
                                           for T in (2, 4) for m in ZERO_MODES for z in (3, 257)])
def test_sliced_zero_counters(hip_ops, T, zero_n, mode):
    """counters [0, zero_n) preset to -1 are zero behind the launch and the ones beyond stay -1: with split rows, without, and
    without a task; the product is the reference's"""
    K, Kx, rows = 50, kx_of(50), ZERO_MODES[mode]
    A = fold_ladder(hip_ops, 32)
    n_tasks, n_long = (A.n_tasks, A.n_long) if rows is None else A.task_range(*rows)[1::2]
    assert (n_tasks > 0, n_long > 0) == {'full': (True, True), 'nolong': (True, False), 'notasks': (False, False)}[mode]
    counters = torch.full((zero_n + 8,), -1, dtype=torch.int32, device=hip_ops.device)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    assert call_sliced(hip_ops, A, exact_image(hip_ops, K), K, out, T, rows=rows, counters=counters[:zero_n]) == 0
    c = hip_ops.to_host(counters)
    assert (c[:zero_n] == 0).all() and (c[zero_n:] == -1).all()
    inside = np.ones(N_ROWS, dtype=bool) if rows is None else (np.arange(N_ROWS) >= rows[0]) & (np.arange(N_ROWS) < rows[1])
    check_fold(hip_ops, buf, K, Kx, reference(K, 256, lib_kappa(hip_ops, K)), rows=inside)


# ---- one task per wave is the old entry -------------------------------------------------------------------------------------
@pytest.mark.parametrize('vbits,K', [pytest.param(vb, K, id='parity_vals%d_K%d' % (vb, K)) for vb, K in ((32, 50), (64, 101), (32, 12))])
def test_one_task_per_wave_is_pk_fold_q20_zero(hip_ops, vbits, K):
    """on the encoder's image, where another order of the sums would show: the same bytes, counters included"""
    A = fold_subset(hip_ops, vbits, K)
    image, _ = encoded_image(hip_ops, K)
    Kx = kx_of(K)
    bufs = [out_buffer(hip_ops, len(SUBSET), Kx) for _ in range(2)]
    counters = torch.full((2, 5), -1, dtype=torch.int32, device=hip_ops.device)
    hip_ops.fold_q20(A, image, K, bufs[0][1], counters=counters[0, :3], tasks_per_wave=1)
    assert call_sliced(hip_ops, A, image, K, bufs[1][1], 1, counters=counters[1, :3]) == 0
    first = hip_ops.to_host(bufs[0][0])
    assert np.abs(first[1:, :K]).max() > 0 and np.array_equal(first, hip_ops.to_host(bufs[1][0]))
    assert hip_ops.to_host(counters).tolist() == [[0, 0, 0, -1, -1]] * 2


# ---- rounded data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,vbits,K', [pytest.param(T, vb, K, id='rounded_' + sliced_id(T, vb, K))
                                       for T, K in ((2, 50), (4, 50), (2, 101)) for vb in (32, 64)])
def test_sliced_rounded(hip_ops, T, vbits, K):
    """the real encoder's image: the bounds of test_gpu_foldq_instances.test_fold_rounded — they do not depend on how many
    groups share a task: a lane still sums U products in fp32 — and two launches return the same bytes"""
    r = rounded_host(K)
    A = fold_subset(hip_ops, vbits, K)
    image, dec = encoded_image(hip_ops, K)
    Kx = kx_of(K)
    buf, out = out_buffer(hip_ops, len(SUBSET), Kx)
    assert call_sliced(hip_ops, A, image, K, out, T) == 0
    got = hip_ops.to_host(buf)
    M, U = r['M'], q20.steps(q20.lanes(K))
    ref = M @ dec
    err, bound = np.abs(got[:, :K] - ref[:, :K]), (U + 2) * 2.0 ** -24 * (M @ np.abs(dec[:, :K])) * 1.001
    far = np.linalg.norm(got[:, :K] - M @ r['V'], axis=1)
    print('largest error / bound: %.3f; largest distance from the exact product / weight: %.3f' % (
        (err / np.maximum(bound, 1e-300)).max(), (far / np.maximum(got[:, K] * 2.0 ** -24, 1e-300)).max()))
    assert (err <= bound).all()
    assert np.allclose(got[:, K], ref[:, K], rtol=(U + 2) * 2.0 ** -24, atol=0)
    assert (far <= got[:, K] * 2.0 ** -24).all()
    assert (got[:, K + 1:Kx] == 0.0).all() and (got[:, Kx:] == SENTINEL).all() and (got[0, :Kx] == 0.0).all()
    buf2, out2 = out_buffer(hip_ops, len(SUBSET), Kx)
    assert call_sliced(hip_ops, A, image, K, out2, T) == 0
    assert np.array_equal(hip_ops.to_host(buf2), got)


@pytest.mark.parametrize('K,asked,runs', [pytest.param(101, 4, 2, id='clamped_K101'), pytest.param(202, 4, 1, id='clamped_K202'),
                                          pytest.param(202, 2, 1, id='clamped_K202_T2')])
def test_tasks_per_wave_is_clamped_to_the_lane_class(hip_ops, K, asked, runs):
    A = fold_subset(hip_ops, 32, K)
    image, _ = encoded_image(hip_ops, K)
    Kx = kx_of(K)
    bufs = [out_buffer(hip_ops, len(SUBSET), Kx) for _ in range(2)]
    assert call_sliced(hip_ops, A, image, K, bufs[0][1], asked) == 0 and call_sliced(hip_ops, A, image, K, bufs[1][1], runs) == 0
    first = hip_ops.to_host(bufs[0][0])
    assert np.abs(first[1:, :K]).max() > 0 and np.array_equal(first, hip_ops.to_host(bufs[1][0]))


# ---- the pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [2, 4])
def test_pass_lists_do_not_depend_on_the_mark(hip_ops, T, monkeypatch):
    """8 229 users (just above scoring.ORDER_USERS_MIN: the pass runs on the activity-ordered image, which carries the mark):
    `recommend` with T tasks per wave on the marked image, and with the mark taken off, returns the same lists — the CPU
    double's — and the marked pass is the one that calls pk_fold_q20_sliced"""
    from polara_amd import ops as ops_module, scoring
    from test_gpu_pass_chain import pass_case
    indptr, indices, values, V, shape, ref = pass_case('pruned')
    ops = hip_ops
    assert shape[0] >= scoring.ORDER_USERS_MIN
    A = ops.csr(indptr, indices, values, shape)
    F = scoring.FactorImage(ops, ops.to_device(V))
    assert F.Q20 is not None and A.by_activity()[0].adjacent_alike and not getattr(A, 'adjacent_alike', False)
    monkeypatch.setattr(ops_module, 'FOLD_TASKS_PER_WAVE', T)
    assert ops.fold_tasks_per_wave(A.by_activity()[0], shape[0]) == 1      # a launch this small keeps one task per wave
    monkeypatch.setattr(ops_module, 'FOLD_SLICED_MIN_WAVES', 0)            # ... unless the floor is taken away
    assert ops.fold_tasks_per_wave(A.by_activity()[0], shape[0]) == T and ops.fold_tasks_per_wave(A, shape[0]) == 1

    def recorded():
        rec = scoring._CallRecorder(ops.lib)
        ops.lib = rec
        try:
            out = ops.to_host(scoring.recommend(ops, F, A, 10, True))
        finally:
            ops.lib = rec.lib
        return [name for name, _, _ in rec.calls], out

    names, marked = recorded()
    assert 'pk_fold_q20_sliced' in names and 'pk_fold_q20_zero' not in names
    A.by_activity()[0].adjacent_alike = False
    names, plain = recorded()
    assert 'pk_fold_q20_sliced' not in names and 'pk_fold_q20_zero' in names
    assert np.array_equal(marked, plain) and np.array_equal(marked, ref)


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [3, 8, 0], ids=lambda T: 'refused_T%d' % T)
def test_sliced_refusals(hip_ops, T):
    """a `tasks_per_wave` other than 1, 2 or 4 returns an error and launches nothing: output and counters keep what they held"""
    K, Kx = 50, 52
    A = fold_ladder(hip_ops, 32)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    counters = torch.full((4,), -1, dtype=torch.int32, device=hip_ops.device)
    assert call_sliced(hip_ops, A, exact_image(hip_ops, K), K, out, T, counters=counters) != 0
    assert b'pk_fold_q20_sliced' in hip_ops.lib.pk_last_error()
    assert (hip_ops.to_host(buf) == SENTINEL).all() and (hip_ops.to_host(counters) == -1).all()

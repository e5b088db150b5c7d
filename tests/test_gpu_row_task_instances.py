"""-m gpu: every instance of the row-task kernels (csrc/spmm.hip, csrc/ttm.hip) at every boundary of their software
pipelines, against NumPy on data whose result does not depend on the summation order.

The launchers pick an instance by the value type of A, the type of the dense block, the mapping (GROUPS 16 / 8 / 4 / 2 / 1 for
an even, even-strided, 16-byte aligned block, else column-per-lane with CPL 1..4), ACC, OFF32 and PRED (plus the list-driven
kernel); the test ids spell the instance out, so that the branches of spmm_groups / spmm_groups_instance, of the three
entries that call them and of PK_TTM_LAUNCH can be ticked off from `pytest --collect-only`:

  test                                     id                                             branch
  test_spmm_exact                          x64_groups{16,8,4,2,1}_nc*_vals{32,64}_acc0_off32  spmm_groups under pk_spmm_csr_ex, XT = double, both edges of every class
                                           x32_groups*_nc*_vals*_acc0_off32                   the same, XT = float
                                           x64_cpl{1,2,3,4}_nc*_vals*_acc0                    its column-per-lane branch; ..._oddld / ..._misaligned:
                                                                                              even nc that must leave the paired kernel
  test_spmm_accumulate                     ..._acc1_off32                                     the ACC twins, `HipOps.spmm_acc`
  test_spmm_accumulate_row_block           ..._acc1_off32_rows150to209                        ACC with row_base
  test_spmm_offsets                        ..._acc{0,1}_off64                                 OFF32 = false (x_rows = 0), bits of off32
  test_spmm_stride_at_the_24_bit_edge      x*_groups16_nc8_stride*_off{32,64}                 spmm_off32: the largest stride of OFF32, the next one
  test_spmm_flagged / test_spmm_rows_list  flagged_/listed_x64_groups*_nc*_vals*_off{32,64}   spmm_groups_instance under pk_spmm_csr_flagged_f64 / pk_spmm_csr_rows_list_f64
  test_spmm_rounded                        rounded_x*_{groups*,cpl*}_nc*_vals*                the precision of every mapping's sums
  test_spmm_plan_with_many_slots           x64_groups4_nc64_vals32_acc0_off32_split64         rows of 2..24 slots
  test_ttm_exact / test_ttm_rounded        ttm_epl{1,2,4,8,16}_ra*_rb*_vals{1,0}              PK_TTM_LAUNCH, both edges of every class
  test_tucker_predict                      predict_r*_L*                                      tucker_predict_kernel

(not reached: OFF32 = false because X ends beyond 4 GiB — that needs a dense block of 4 GiB.)

The ladder: row r has r entries for r = 0..200, then rows of 255, 256, 257, 258, 511, 512, 513, 769, 1500 entries and two
empty rows, so that a task of every length at which `have` / `have_next`, the prefetch two chunks ahead and the groups of 8 / 16
of the column-per-lane kernel switch exists — with split = 256 also as the halves of split rows (257 -> 129 + 128).

Exact data: values 1..5, X integers in [-1000, 1000]; every partial sum is an integer below 2^53 (2^24 for the fp32 block), so
the product is the same in every order and is compared with `np.array_equal`.  No entry references column 0 and X[0, :] = 2^40:
padded lanes gather row 0 with weight 0, one that carried a weight would show.  Rounded data (normals rounded to fp32, so
every product is exact in fp64) sees what the integers cannot, a sum carried in the wrong precision: see `rounded_bound`.

What the net catches, tried on scratch builds with one arithmetic-only change each (new cases failed / run; earlier tests
of the operator):
  spmm_groups_task    `k * U * GROUPS < cnt - 1`   146 / 180 (all but the column-per-lane ones)    17 / 45
  ttm_fixup_kernel    `s < s1 - 1`                 29 / 31                                         4 / 14
  tucker_predict      `sc >= best_s`               16 / 21 (L = 1 has no tie)                      0 / 3: unseen before
  spmm_groups_task    `k * U * GROUPS <= cnt`      3 / 180                                         7 / 45
The last one is no error under the contract of include/polara_hip.h (finite X): the extra register set it consumes carries
weight 0, so it shows only where a register that was never loaded happens to hold a NaN or an infinity."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sps
import torch

pytestmark = pytest.mark.gpu

N_COLS = 2100
LADDER = list(range(201)) + [255, 256, 257, 258, 511, 512, 513, 769, 1500, 0, 0]
N_ROWS = len(LADDER)                                    # 212
SPLIT = 256
SPLIT_ROWS = [r for r, n in enumerate(LADDER) if n > SPLIT]             # 203 .. 209
SUBSET = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257,
          513, 769]
SENTINEL = -7.0
BIG = float(2 ** 40)
U53 = 2.0 ** -53


def groups_of(nc):
    return 16 if nc <= 16 else 8 if nc <= 32 else 4 if nc <= 64 else 2 if nc <= 128 else 1


def slots_of(n, split=SPLIT):
    return -(-n // split) if n > split else 0


# ---- host side: built once, read-only -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder_host():
    rng = np.random.RandomState(2100)
    rows = []
    for r, n in enumerate(LADDER):
        c = np.sort(rng.choice(np.arange(1, N_COLS), n, replace=False))       # column 0: never
        if n and r % 5 == 1:
            c[-1] = N_COLS - 1                                                # the last column: in many rows
        rows.append(c)
    indptr = np.r_[0, np.cumsum(LADDER)].astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    values = rng.randint(1, 6, indptr[-1]).astype(np.int64)
    assert (indices > 0).all() and (indices == N_COLS - 1).sum() > 20 and indptr[-1] == sum(LADDER)
    assert all(len(np.unique(c)) == len(c) for c in rows)
    X = rng.randint(-1000, 1001, (N_COLS, 256)).astype(np.int64)
    S = sps.csr_matrix((values, indices, indptr), shape=(N_ROWS, N_COLS))
    ref = np.asarray(S @ X)                                                   # int64, exact
    assert ref.dtype == np.int64 and np.abs(S).dot(np.abs(X)).max() < 2 ** 24
    pre = rng.randint(-9999, 10000, (N_ROWS, 256)).astype(np.int64)           # what an accumulating launch finds in `out`
    for a in (indptr, indices, values, X, ref, pre):
        a.setflags(write=False)
    return dict(indptr=indptr, indices=indices, values=values, X=X, ref=ref, pre=pre)


@functools.lru_cache(maxsize=None)
def subset_host():
    """the 32 rows of SUBSET (the ladder's columns) with rounded data, their correctly rounded product and sum |a| |x|"""
    h = ladder_host()
    rng = np.random.RandomState(32)
    rows = [LADDER.index(n) for n in SUBSET]
    cols = [h['indices'][h['indptr'][r]:h['indptr'][r + 1]] for r in rows]
    indptr = np.r_[0, np.cumsum(SUBSET)].astype(np.int64)
    indices = np.concatenate(cols).astype(np.int32)
    values = rng.randn(indptr[-1]).astype(np.float32)
    X = rng.randn(N_COLS, 256).astype(np.float32)
    X[0] = 1.0
    ref, mag = fsum_rows(indptr, lambda p0, p1: values[p0:p1, None].astype(np.float64) * X[indices[p0:p1]].astype(np.float64), 256)
    for a in (indptr, indices, values, X, ref, mag):
        a.setflags(write=False)
    return dict(indptr=indptr, indices=indices, values=values, X=X, ref=ref, mag=mag)


def fsum_rows(indptr, products, width):
    """(correctly rounded sums, sums of magnitudes) of the exact per-entry products [n x width] of every row"""
    n_rows = len(indptr) - 1
    ref, mag = np.zeros((n_rows, width)), np.zeros((n_rows, width))
    for r in range(n_rows):
        if indptr[r + 1] > indptr[r]:
            P = products(int(indptr[r]), int(indptr[r + 1]))
            ref[r] = [math.fsum(col) for col in P.T.tolist()]
            mag[r] = [math.fsum(col) for col in np.abs(P).T.tolist()]
    return ref, mag


def rounded_bound(lengths, slots, ref, mag):
    """|got - ref| <= (n + s + 6) 2^-53 sum |a| |x| + 2^-53 |ref|, per element; n the row's length, s its slot count.

    Derivation.  The data are fp32 numbers held in the instance's types, so every product a x is exact in fp64 and an fma
    rounds once, when it adds the product to its accumulator.  A kernel's result is therefore the products summed along SOME
    tree of fp64 additions, each with relative error at most u = 2^-53, and the error of such a sum is at most
    ((1 + u)^d - 1) sum |a| |x| with d the largest number of additions any one product passes through.  Here d is at most n
    (the accumulator chain of a lane; padded steps add 0 and round nothing), + 4 (the lane exchanges that add the partial sums
    of up to 16 groups), + s (the fix-up adds the s partial rows of a split row in slot order; the 8-way fix-up of the TTM:
    ceil(s / 8) + 7 <= s + 6 additions, the ones of an empty partial exact), + 1 (an accumulating launch adds what `out` held).
    (1 + u)^d - 1 <= (d + 1) u for d (d + 1) u <= 1, which gives the factor n + s + 6 for d <= n + s + 5.  The reference is
    the correctly rounded sum (math.fsum over the exact products), itself within u |exact| <= u (1 + u) |ref| of the exact
    one: the second term, its (1 + u) taken from the slack of the first."""
    d = (np.asarray(lengths) + np.asarray(slots) + 6).astype(np.float64)
    return d[:, None] * U53 * mag + U53 * np.abs(ref)


def np_dtype(bits):
    return np.float32 if bits == 32 else np.float64


# ---- device side ----------------------------------------------------------------------------------------------------------
_DEVICE = {}


def device_csr(ops, host, bits, n_rows, split=SPLIT, key=None):
    """the CSR on the device with its values in the asked type (HipOps.csr stores exactly representable fp64 values as fp32)"""
    from polara_amd.ops import DeviceCSR
    k = (key, bits, split)
    if k not in _DEVICE:
        vals = torch.from_numpy(host['values'].astype(np_dtype(bits))).to(ops.device)
        _DEVICE[k] = DeviceCSR.from_device(ops, ops.to_device(host['indptr']), ops.to_device(host['indices']), vals,
                                           (n_rows, N_COLS), split=split)
    return _DEVICE[k]


def ladder(ops, bits, split=SPLIT):
    A = device_csr(ops, ladder_host(), bits, N_ROWS, split, key='ladder')
    assert A.values.dtype == (torch.float32 if bits == 32 else torch.float64)
    return A


def subset(ops, bits):
    return device_csr(ops, subset_host(), bits, len(SUBSET), key='subset')


def plan_slots(ops, A):
    p = A.plan
    return (ops.to_host(p['long_row'])[:A.n_long].tolist(),
            (ops.to_host(p['long_slot_end']) - ops.to_host(p['long_slot_begin']))[:A.n_long].tolist())


def dense(ops, Xh, xbits, nc, layout='plain'):
    """columns [0, nc) of the host block on the device: contiguous, with an odd leading dimension, or as a view whose first
    element lies 8 bytes behind a 16-byte boundary"""
    dt = np_dtype(xbits)
    Xc = np.ascontiguousarray(Xh[:, :nc]).astype(dt)
    if layout == 'plain':
        X = ops.to_device(Xc)
    elif layout == 'oddld':
        X = ops.to_device(np.zeros((Xh.shape[0], nc + 1), dtype=dt))[:, :nc]
        X.copy_(ops.to_device(Xc))
    else:
        assert layout == 'misaligned' and xbits == 64
        X = ops.to_device(np.zeros((Xh.shape[0], nc + 2), dtype=dt))[:, 1:nc + 1]
        X.copy_(ops.to_device(Xc))
        assert X.stride(0) % 2 == 0 and X.data_ptr() % 16 == 8
    return X


def exact_block(ops, xbits, nc, layout='plain'):
    Xh = ladder_host()['X'].astype(np.float64)
    Xh[0] = BIG
    return dense(ops, Xh, xbits, nc, layout)


def out_buffer(ops, n_rows, nc, preload=None):
    """(buffer of sentinels with 3 spare columns, the [n_rows x nc] view a launch writes)"""
    buf = torch.full((n_rows, nc + 3), SENTINEL, dtype=torch.float64, device=ops.device)
    if preload is not None:
        buf[:, :nc] = ops.to_device(preload[:, :nc].astype(np.float64))
    return buf, buf[:, :nc]


def raw_spmm(ops, A, X, out, x_rows, accumulate=0):
    """pk_spmm_csr_ex as HipOps._spmm_launch calls it, with the caller's word on the rows of X (0: unknown, 64-bit offsets)"""
    from polara_amd import _lib
    from polara_amd.ops import _ptr
    p, nc = A.plan, X.shape[1]
    _lib.check(ops.lib.pk_spmm_csr_ex(
        ops.stream(), A.n_tasks, _ptr(p['task_row']), _ptr(p['task_begin']), _ptr(p['task_end']), _ptr(p['task_slot']), A.n_long,
        _ptr(p['long_row']), _ptr(p['long_slot_begin']), _ptr(p['long_slot_end']), _ptr(A.indices), _ptr(A.values), A.val_kind,
        _ptr(X), _lib.PK_VAL_F64 if X.dtype == torch.float64 else _lib.PK_VAL_F32, X.stride(0), nc, _ptr(out), out.stride(0),
        _ptr(A.partial(nc)), 0, int(accumulate), int(x_rows)), 'pk_spmm_csr_ex')
    return out


def raw_flagged(ops, A, X, out, flags, mask, x_rows):
    from polara_amd import _lib
    from polara_amd.ops import _ptr
    p, nc = A.plan, X.shape[1]
    _lib.check(ops.lib.pk_spmm_csr_flagged_f64(
        ops.stream(), A.n_tasks, _ptr(p['task_row']), _ptr(p['task_begin']), _ptr(p['task_end']), _ptr(p['task_slot']), A.n_long,
        _ptr(p['long_row']), _ptr(p['long_slot_begin']), _ptr(p['long_slot_end']), _ptr(A.indices), _ptr(A.values), A.val_kind,
        _ptr(X), X.stride(0), nc, _ptr(out), out.stride(0), _ptr(A.partial(nc)), int(x_rows), _ptr(flags), int(mask)),
        'pk_spmm_csr_flagged_f64')
    return out


def raw_rows_list(ops, A, X, out, lst, cnt, flags, mask, x_rows):
    from polara_amd import _lib
    from polara_amd.ops import _ptr
    p, nc = A.plan, X.shape[1]
    _lib.check(ops.lib.pk_spmm_csr_rows_list_f64(
        ops.stream(), int(lst.numel()), _ptr(lst), _ptr(cnt), 0, _ptr(A._ensure_plan()['row_first_task']), _ptr(p['task_row']),
        _ptr(p['task_begin']), _ptr(p['task_end']), _ptr(p['task_slot']), A.n_long, _ptr(p['long_row']), _ptr(p['long_slot_begin']),
        _ptr(p['long_slot_end']), _ptr(A.indices), _ptr(A.values), A.val_kind, _ptr(X), X.stride(0), nc, _ptr(out), out.stride(0),
        _ptr(A.partial(nc)), int(x_rows), _ptr(flags), int(mask)), 'pk_spmm_csr_rows_list_f64')
    return out


def check_exact(ops, buf, nc, want, rows=None):
    """the first nc columns of `buf` equal `want` (int64) on `rows` (all by default) and everything else is the sentinel"""
    got = ops.to_host(buf)
    hit = np.ones(len(got), dtype=bool) if rows is None else rows
    assert np.array_equal(got[hit, :nc], want[hit, :nc].astype(np.float64))
    assert (got[~hit] == SENTINEL).all() and (got[:, nc:] == SENTINEL).all()


# ---- 1. the plans ---------------------------------------------------------------------------------------------------------
def test_ladder_plan_keeps_its_split_rows(hip_ops):
    for bits in (32, 64):
        A = ladder(hip_ops, bits)
        assert A.n_long == 7 and A.n_slots == 21 and A.n_tasks == N_ROWS - 7 + 21
        assert plan_slots(hip_ops, A) == (SPLIT_ROWS, [2, 2, 2, 2, 3, 4, 6])
        p = A.plan
        first = int(hip_ops.to_host(A._ensure_plan()['row_first_task'])[203])
        halves = (hip_ops.to_host(p['task_end']) - hip_ops.to_host(p['task_begin']))[first:first + 2]
        assert halves.tolist() == [129, 128]                       # 257 -> 129 + 128
    B = subset(hip_ops, 32)
    assert plan_slots(hip_ops, B) == ([SUBSET.index(n) for n in (257, 513, 769)], [2, 3, 4])


# ---- 3. SpMM: exact -------------------------------------------------------------------------------------------------------
PAIRED_NC = [2, 16, 18, 32, 34, 64, 66, 128, 130, 256]
CPL_NC = [1, 63, 65, 127, 129, 191, 193, 255]
F32_NC = [4, 16, 20, 32, 36, 64, 68, 128, 132, 256]


def spmm_id(xbits, nc, vbits, acc=0, off=32, layout='plain'):
    if layout == 'plain' and (xbits == 32 or nc % 2 == 0):
        return 'x%d_groups%d_nc%d_vals%d_acc%d_off%d' % (xbits, groups_of(nc), nc, vbits, acc, off)
    tail = '' if layout == 'plain' else '_' + layout
    return 'x64_cpl%d_nc%d_vals%d_acc%d%s' % ((nc + 63) // 64, nc, vbits, acc, tail)


def spmm_cases(fp64_nc, fp32_nc, layouts=(), **kw):
    cases = [(64, nc, vb, 'plain') for nc in fp64_nc for vb in (32, 64)]
    cases += [(32, nc, vb, 'plain') for nc in fp32_nc for vb in (32, 64)]
    cases += [(64, 64, vb, lay) for lay in layouts for vb in (32, 64)]
    return [pytest.param(*c, id=spmm_id(c[0], c[1], c[2], layout=c[3], **kw)) for c in cases]


@pytest.mark.parametrize('xbits,nc,vbits,layout', spmm_cases(PAIRED_NC + CPL_NC, F32_NC, ('oddld', 'misaligned')))
def test_spmm_exact(hip_ops, xbits, nc, vbits, layout):
    """the full product of the ladder, to the last bit; an even nc with an odd leading dimension or a misaligned first element
    must run on the column-per-lane kernel (the paired kernel's 16-byte loads would fault or read the neighbours)"""
    h = ladder_host()
    A = ladder(hip_ops, vbits)
    X = exact_block(hip_ops, xbits, nc, layout)
    if layout != 'plain':
        assert not hip_ops.spmm_flagged_ok(X)
    elif xbits == 64 and nc % 2 == 0:
        assert hip_ops.spmm_flagged_ok(X)
    buf, out = out_buffer(hip_ops, N_ROWS, nc)
    hip_ops.spmm(A, X, out=out)
    check_exact(hip_ops, buf, nc, h['ref'])
    got = hip_ops.to_host(out)
    assert (got[[0, N_ROWS - 2, N_ROWS - 1]] == 0.0).all()          # empty rows are written, as zeros


def test_spmm_fp32_block_of_six_columns_is_unsupported(hip_ops):
    from polara_amd._lib import PolaraHipError
    _, out = out_buffer(hip_ops, N_ROWS, 6)
    with pytest.raises(PolaraHipError, match='fp32 dense block'):
        hip_ops.spmm(ladder(hip_ops, 32), exact_block(hip_ops, 32, 6), out=out)


def test_spmm_plan_with_many_slots(hip_ops):
    """x64_groups4_nc64_vals32_acc0_off32_split64: every row above 64 entries is split, into 2 .. 24 slots"""
    h = ladder_host()
    A = ladder(hip_ops, 32, split=64)
    long_rows = [r for r, n in enumerate(LADDER) if n > 64]
    assert A.n_long == len(long_rows) == 145
    assert plan_slots(hip_ops, A) == (long_rows, [-(-LADDER[r] // 64) for r in long_rows])
    assert min(plan_slots(hip_ops, A)[1]) == 2 and max(plan_slots(hip_ops, A)[1]) == 24
    buf, out = out_buffer(hip_ops, N_ROWS, 64)
    hip_ops.spmm(A, exact_block(hip_ops, 64, 64), out=out)
    check_exact(hip_ops, buf, 64, h['ref'])
    buf, out = out_buffer(hip_ops, N_ROWS, 64, preload=h['pre'])
    hip_ops.spmm_acc(A, exact_block(hip_ops, 64, 64), out)
    check_exact(hip_ops, buf, 64, h['ref'] + h['pre'])


# ---- ACC ------------------------------------------------------------------------------------------------------------------
ACC_NC, ACC_F32_NC = [1, 16, 32, 64, 65, 128, 256], [16, 32, 64]


@pytest.mark.parametrize('xbits,nc,vbits,layout', spmm_cases(ACC_NC, ACC_F32_NC, acc=1))
def test_spmm_accumulate(hip_ops, xbits, nc, vbits, layout):
    """out += A X: empty rows keep what they held (the early return), split rows add once (the fix-up adds), every other
    row adds its sum"""
    h = ladder_host()
    A = ladder(hip_ops, vbits)
    X = exact_block(hip_ops, xbits, nc)
    buf, out = out_buffer(hip_ops, N_ROWS, nc, preload=h['pre'])
    if xbits == 64:
        hip_ops.spmm_acc(A, X, out)
    else:
        hip_ops._spmm_launch(A, X, out, (0, A.n_tasks, 0, A.n_long), accumulate=True)
    check_exact(hip_ops, buf, nc, h['ref'] + h['pre'])
    empty = [0, N_ROWS - 2, N_ROWS - 1]
    assert np.array_equal(hip_ops.to_host(out)[empty], h['pre'][empty, :nc].astype(np.float64))


BLOCK_LO, BLOCK_HI = 150, LADDER.index(769) + 1


@pytest.mark.parametrize('xbits,nc,vbits', [pytest.param(xb, nc, vb, id=spmm_id(xb, nc, vb, acc=1) + '_rows%dto%d' % (BLOCK_LO, BLOCK_HI))
                                            for xb, nc, vb in ((64, 32, 32), (64, 64, 64), (64, 65, 32), (64, 256, 64), (32, 32, 32), (32, 64, 64))])
def test_spmm_accumulate_row_block(hip_ops, xbits, nc, vbits):
    """a row block of the plan as its own accumulating launch: rows [150, 209) — five split rows among them — land in rows
    [0, 59) of a block that lies inside a larger buffer, whose other rows and columns stay as they were"""
    h = ladder_host()
    A = ladder(hip_ops, vbits)
    X = exact_block(hip_ops, xbits, nc)
    height = BLOCK_HI - BLOCK_LO
    big = torch.full((height + 4, nc + 3), SENTINEL, dtype=torch.float64, device=hip_ops.device)
    block = big[2:2 + height, :nc]
    block.copy_(hip_ops.to_device(h['pre'][BLOCK_LO:BLOCK_HI, :nc].astype(np.float64)))
    rng = A.task_range(BLOCK_LO, BLOCK_HI)
    assert rng[3] == 6 and rng[1] == height - 6 + 15               # 257, 258, 511, 512, 513, 769: 2 + 2 + 2 + 2 + 3 + 4 slots
    hip_ops._spmm_launch(A, X, block, rng, row_base=BLOCK_LO, accumulate=True)
    got = hip_ops.to_host(big)
    want = (h['ref'] + h['pre'])[BLOCK_LO:BLOCK_HI, :nc]
    assert np.array_equal(got[2:2 + height, :nc], want.astype(np.float64))
    assert (got[:2] == SENTINEL).all() and (got[2 + height:] == SENTINEL).all() and (got[:, nc:] == SENTINEL).all()


# ---- OFF32 both ways ------------------------------------------------------------------------------------------------------
CLASS_NC = {16: 16, 8: 32, 4: 64, 2: 128, 1: 256}


@pytest.mark.parametrize('xbits,nc,vbits,acc', [pytest.param(xb, nc, vb, acc, id=spmm_id(xb, nc, vb, acc=acc, off=64))
                                                for xb in (64, 32) for nc in CLASS_NC.values() for vb, acc in ((32, 0), (64, 1))])
def test_spmm_offsets(hip_ops, xbits, nc, vbits, acc):
    """x_rows = 0 (rows of X unknown) takes the kernels with 64-bit offsets: the exact product, and on rounded data the
    bits of the 32-bit form (same mapping, same order)"""
    h = ladder_host()
    A = ladder(hip_ops, vbits)
    X = exact_block(hip_ops, xbits, nc)
    pre = h['pre'] if acc else None
    for x_rows in (0, N_COLS):
        buf, out = out_buffer(hip_ops, N_ROWS, nc, preload=pre)
        raw_spmm(hip_ops, A, X, out, x_rows, accumulate=acc)
        check_exact(hip_ops, buf, nc, h['ref'] + (h['pre'] if acc else 0))
    s = subset_host()
    B = subset(hip_ops, vbits)
    Xr = dense(hip_ops, s['X'], xbits, nc)
    res = []
    for x_rows in (0, N_COLS):
        buf, out = out_buffer(hip_ops, len(SUBSET), nc, preload=s['ref'] if acc else None)
        raw_spmm(hip_ops, B, Xr, out, x_rows, accumulate=acc)
        res.append(hip_ops.to_host(buf))
    assert np.array_equal(res[0], res[1])


@pytest.mark.parametrize('xbits,stride,off', [pytest.param(64, 2 ** 21 - 2, 32, id='x64_groups16_nc8_stride2p21m2_off32'),
                                               pytest.param(64, 2 ** 21, 64, id='x64_groups16_nc8_stride2p21_off64'),
                                               pytest.param(32, 2 ** 22 - 4, 32, id='x32_groups16_nc8_stride2p22m4_off32'),
                                               pytest.param(32, 2 ** 22, 64, id='x32_groups16_nc8_stride2p22_off64')])
def test_spmm_stride_at_the_24_bit_edge(hip_ops, xbits, stride, off):
    """a row stride of 2^24 - 16 bytes is the largest whose 24 bits the one-instruction offset of OFF32 holds; 2^24 bytes
    must take the 64-bit form (its low 24 bits are zero: every row would read row 0)"""
    assert (stride * xbits // 8 < 2 ** 24) == (off == 32) and 3 * stride * xbits // 8 < 2 ** 32
    nc = 8
    indptr = np.array([0, 0, 1, 2, 4, 4, 6], dtype=np.int64)
    indices = np.array([2, 1, 1, 2, 1, 2], dtype=np.int32)
    values = np.array([3, 5, 2, 4, 1, 5], dtype=np.float32)
    A = hip_ops.csr(indptr, indices, values, (6, 3))
    flat = torch.zeros(3 * stride, dtype=torch.float64 if xbits == 64 else torch.float32, device=hip_ops.device)
    X = flat.as_strided((3, nc), (stride, 1))
    Xh = np.random.RandomState(24).randint(-1000, 1001, (3, nc)).astype(np.float64)
    Xh[0] = BIG
    X.copy_(hip_ops.to_device(Xh.astype(np_dtype(xbits))))
    buf, out = out_buffer(hip_ops, 6, nc)
    hip_ops.spmm(A, X, out=out)
    ref = sps.csr_matrix((values.astype(np.int64), indices, indptr), shape=(6, 3)) @ Xh.astype(np.int64)
    check_exact(hip_ops, buf, nc, np.asarray(ref))


# ---- PRED and the list-driven kernel --------------------------------------------------------------------------------------
UNFLAGGED_SPLIT_ROW = LADDER.index(512)
PART_NC = {16: 10, 8: 24, 4: 48, 2: 100, 1: 200}


def chosen_rows():
    """every third row and all split rows but one"""
    hit = np.arange(N_ROWS) % 3 == 0
    hit[SPLIT_ROWS] = True
    assert UNFLAGGED_SPLIT_ROW % 3 != 0
    hit[UNFLAGGED_SPLIT_ROW] = False
    return hit


def part_cases(kind):
    return [pytest.param(nc, vb, off, id='%s_%s' % (kind, spmm_id(64, nc, vb, off=off).replace('_acc0', '')))
            for nc in PART_NC.values() for vb in (32, 64) for off in (32, 64)]


@pytest.mark.parametrize('nc,vbits,off', part_cases('flagged'))
def test_spmm_flagged(hip_ops, nc, vbits, off):
    """the flag-predicated product against NumPy: flagged rows (empty ones and split ones among them) get the product,
    every other row — a split row among them, whose fix-up must not run — keeps what it held"""
    h = ladder_host()
    A = ladder(hip_ops, vbits)
    X = exact_block(hip_ops, 64, nc)
    hit = chosen_rows()
    flags = np.where(hit, np.array([1, 2, 4, 5, 3])[np.arange(N_ROWS) % 5], np.array([0, 8])[np.arange(N_ROWS) % 2]).astype(np.int32)
    buf, out = out_buffer(hip_ops, N_ROWS, nc)
    if off == 32:
        hip_ops.spmm_flagged(A, X, out, hip_ops.to_device(flags), 7)
    else:
        raw_flagged(hip_ops, A, X, out, hip_ops.to_device(flags), 7, 0)
    check_exact(hip_ops, buf, nc, h['ref'], rows=hit)


@pytest.mark.parametrize('nc,vbits,off', part_cases('listed'))
def test_spmm_rows_list(hip_ops, nc, vbits, off):
    """the list-driven product against NumPy: a permuted device-side list shorter than its capacity"""
    h = ladder_host()
    A = ladder(hip_ops, vbits)
    X = exact_block(hip_ops, 64, nc)
    hit = chosen_rows()
    rows = np.flatnonzero(hit)
    lst = np.full(len(rows) + 40, SPLIT_ROWS[-1], dtype=np.int32)             # beyond the count: never read
    lst[:len(rows)] = np.random.RandomState(nc).permutation(rows)
    cnt = hip_ops.to_device(np.array([len(rows)], dtype=np.int32))
    flags = hip_ops.to_device(np.where(hit, 4, 0).astype(np.int32))
    buf, out = out_buffer(hip_ops, N_ROWS, nc)
    if off == 32:
        hip_ops.spmm_rows_list(A, X, out, hip_ops.to_device(lst), cnt, flags, 7)
    else:
        raw_rows_list(hip_ops, A, X, out, hip_ops.to_device(lst), cnt, flags, 7, 0)
    check_exact(hip_ops, buf, nc, h['ref'], rows=hit)


# ---- 2. SpMM: rounded -----------------------------------------------------------------------------------------------------
ROUNDED_NC = {64: [14, 30, 62, 126, 254, 63, 127, 191, 255], 32: [12, 28, 60, 124, 252]}


@pytest.mark.parametrize('xbits,nc,vbits', [pytest.param(xb, nc, vb, id='rounded_' + spmm_id(xb, nc, vb).split('_acc')[0])
                                            for xb in (64, 32) for nc in ROUNDED_NC[xb] for vb in (32, 64)])
def test_spmm_rounded(hip_ops, xbits, nc, vbits):
    """every mapping's sums are carried in fp64 from the first product to the last addition: `rounded_bound`"""
    s = subset_host()
    A = subset(hip_ops, vbits)
    buf, out = out_buffer(hip_ops, len(SUBSET), nc)
    hip_ops.spmm(A, dense(hip_ops, s['X'], xbits, nc), out=out)
    got = hip_ops.to_host(out)
    ref, mag = s['ref'][:, :nc], s['mag'][:, :nc]
    bound = rounded_bound(SUBSET, [slots_of(n) for n in SUBSET], ref, mag)
    err = np.abs(got - ref)
    print('largest error / bound: %.3f' % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all() and (hip_ops.to_host(buf)[:, nc:] == SENTINEL).all()
    assert (got[0] == 0.0).all() and np.array_equal(got[1], ref[1])          # no entry: zero; one entry: the product itself


# ---- 4. TTM ---------------------------------------------------------------------------------------------------------------
TTM_LENGTHS = list(range(71)) + [127, 128, 129, 130, 255, 256, 257, 258, 2305, 4100]
TTM_SUBSET = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2305]
TTM_N1, TTM_N2 = 41, 23
TTM_RANKS = [(1, 1), (7, 9), (8, 8), (5, 13), (8, 16), (3, 43), (16, 16), (257, 1), (16, 32), (19, 27), (31, 33), (32, 32)]
TTM_ROUNDED_RANKS = [(6, 10), (9, 13), (15, 15), (17, 23), (19, 27)]


def epl_of(nout):
    e = (nout + 63) // 64
    return 1 if e <= 1 else 2 if e <= 2 else 4 if e <= 4 else 8 if e <= 8 else 16


def ttm_id(ranks, weighted):
    return 'ttm_epl%d_ra%d_rb%d_vals%d' % (epl_of(ranks[0] * ranks[1]), ranks[0], ranks[1], int(weighted))


@functools.lru_cache(maxsize=None)
def tensor_host(lengths):
    """entries (i0, i1, i2) with `lengths[i0]` entries in slice i0, in shuffled order; no entry references row 0 of a factor"""
    rng = np.random.RandomState(len(lengths))
    nnz = sum(lengths)
    idx = np.stack([np.repeat(np.arange(len(lengths)), lengths), rng.randint(1, TTM_N1, nnz), rng.randint(1, TTM_N2, nnz)], 1)
    idx = idx[rng.permutation(nnz)].astype(np.intp)
    idx.setflags(write=False)
    return idx, (len(lengths), TTM_N1, TTM_N2)


def ttm_reference(idx, val, n0, u, v):
    """res[i0, j * rb + k] = sum over the entries of slice i0 of val u[i1, j] v[i2, k], in the arithmetic of the arguments"""
    res = np.zeros((n0, u.shape[1] * v.shape[1]), dtype=u.dtype)
    order = np.argsort(idx[:, 0], kind='stable')
    bounds = np.searchsorted(idx[order, 0], np.arange(n0 + 1))
    for i0 in range(n0):
        e = order[bounds[i0]:bounds[i0 + 1]]
        if len(e):
            res[i0] = np.einsum('n,nj,nk->jk', val[e], u[idx[e, 1]], v[idx[e, 2]]).ravel()
    return res


def ttm_plan(ops, idx, val, shape, key):
    from polara_amd import tucker
    k = ('ttm', key)
    if k not in _DEVICE:
        _DEVICE[k] = tucker.ModePlan(ops, idx, val, shape, 0, 1, 2)
    return _DEVICE[k]


def test_ttm_plan_keeps_its_split_slices(hip_ops):
    idx, shape = tensor_host(tuple(TTM_LENGTHS))
    mp = ttm_plan(hip_ops, idx, None, shape, 'ones')
    p = mp.plan
    assert mp.vals is None and p['n_long'] == 4
    assert (hip_ops.to_host(p['long_slot_end']) - hip_ops.to_host(p['long_slot_begin'])).tolist() == [2, 2, 10, 17]
    assert hip_ops.to_host(p['long_row']).tolist() == [TTM_LENGTHS.index(n) for n in (257, 258, 2305, 4100)]


@pytest.mark.parametrize('weighted', [True, False], ids=lambda w: 'vals%d' % w)
@pytest.mark.parametrize('ranks', TTM_RANKS, ids=lambda r: 'ttm_epl%d_ra%d_rb%d' % (epl_of(r[0] * r[1]), r[0], r[1]))
def test_ttm_exact(hip_ops, ranks, weighted):
    """integer values 1..5 (or none: the all-ones path) and integer factors in [-30, 30]: every sum is an integer below
    2^53, the result equals the int64 restatement bit for bit.  Row 0 of u and of v, which padded steps read with value 0,
    holds 2^40."""
    from polara_amd import tucker
    idx, shape = tensor_host(tuple(TTM_LENGTHS))
    rng = np.random.RandomState(1000 * ranks[0] + ranks[1])
    val = np.random.RandomState(5).randint(1, 6, len(idx)).astype(np.int64) if weighted else np.ones(len(idx), dtype=np.int64)
    mp = ttm_plan(hip_ops, idx, val.astype(np.float64) if weighted else None, shape, 'weighted' if weighted else 'ones')
    assert (mp.vals is not None) == weighted
    u, v = rng.randint(-30, 31, (TTM_N1, ranks[0])).astype(np.int64), rng.randint(-30, 31, (TTM_N2, ranks[1])).astype(np.int64)
    ref = ttm_reference(idx, val, shape[0], u, v)
    ud, vd = u.astype(np.float64), v.astype(np.float64)
    ud[0], vd[0] = BIG, BIG
    got = hip_ops.to_host(tucker.ttm(hip_ops, mp, hip_ops.to_device(ud), hip_ops.to_device(vd)))
    assert got.shape == ref.shape and np.array_equal(got, ref.astype(np.float64))
    assert (got[0] == 0.0).all()


def test_ttm_of_1025_outputs_is_refused(hip_ops):
    from polara_amd import tucker
    from polara_amd._lib import PolaraHipError
    idx, shape = tensor_host(tuple(TTM_LENGTHS))
    mp = ttm_plan(hip_ops, idx, None, shape, 'ones')
    with pytest.raises(PolaraHipError, match='1024'):
        tucker.ttm(hip_ops, mp, hip_ops.zeros(TTM_N1, 25), hip_ops.zeros(TTM_N2, 41))


@pytest.mark.parametrize('ranks', TTM_ROUNDED_RANKS, ids=lambda r: 'rounded_' + ttm_id(r, True))
def test_ttm_rounded(hip_ops, ranks):
    """`rounded_bound` with n the slice's length: the factors are normals rounded to fp32 and the values signed powers of
    two, so that val u v is exact in fp64 (and so is the kernel's val * u ahead of its fma)"""
    from polara_amd import tucker
    idx, shape = tensor_host(tuple(TTM_SUBSET))
    rng = np.random.RandomState(ranks[0] * ranks[1])
    val = np.random.RandomState(6).choice([-4.0, -1.0, -0.5, 0.25, 0.5, 1.0, 2.0, 4.0], len(idx))
    mp = ttm_plan(hip_ops, idx, val, shape, 'rounded')
    u = rng.randn(TTM_N1, ranks[0]).astype(np.float32).astype(np.float64)
    v = rng.randn(TTM_N2, ranks[1]).astype(np.float32).astype(np.float64)
    order = np.argsort(idx[:, 0], kind='stable')
    indptr = np.searchsorted(idx[order, 0], np.arange(shape[0] + 1))

    def products(p0, p1):
        e = order[p0:p1]
        return ((val[e, None] * u[idx[e, 1]])[:, :, None] * v[idx[e, 2]][:, None, :]).reshape(len(e), -1)
    ref, mag = fsum_rows(indptr, products, ranks[0] * ranks[1])
    got = hip_ops.to_host(tucker.ttm(hip_ops, mp, hip_ops.to_device(u), hip_ops.to_device(v)))
    bound = rounded_bound(TTM_SUBSET, [slots_of(n) for n in TTM_SUBSET], ref, mag)
    err = np.abs(got - ref)
    print('largest error / bound: %.3f' % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all() and (got[0] == 0.0).all()


# ---- Tucker prediction ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [1, 2, 5, 64, 65], ids=lambda L: 'L%d' % L)
@pytest.mark.parametrize('ranks', [(1, 1, 1), (3, 4, 5), (7, 5, 15), (6, 6, 16)], ids=lambda r: 'predict_r%d_%d_%d' % r)
def test_tucker_predict(hip_ops, ranks, L):
    """integer factors and core: the scores are exact, so they equal the int64 einsum and the prediction np.argmax — the
    FIRST maximum: rows 0 and 2 of w are equal, the last L // 2 rows repeat the first L // 2 and the middle row of an odd L
    repeats row 0, so that the best level of EVERY pair comes back at a higher index"""
    r0, r1, r2 = ranks
    rng = np.random.RandomState(100 * r2 + L)
    n_users, n_items = 37, 29
    u, v = rng.randint(-3, 4, (n_users, r0)), rng.randint(-3, 4, (n_items, r1))
    core = rng.randint(-3, 4, ranks)
    w = rng.randint(-3, 4, (L, r2))
    if L >= 3:
        w[2] = w[0]
    w[L - L // 2:] = w[:L // 2]
    w[L // 2] = w[0]
    assert L == 1 or all((w == row).all(1).sum() >= 2 for row in w)
    ud, vd, wd, cd = (hip_ops.to_device(a.astype(np.float64)) for a in (u, v, w, core))
    for n in (0, 1, 255, 256, 257):
        users, items = rng.randint(0, n_users, n).astype(np.int64), rng.randint(0, n_items, n).astype(np.int64)
        ref = np.einsum('abc,na,nb,fc->nf', core, u[users], v[items], w).astype(np.int64)
        pred, scores = hip_ops.tucker_predict(users, items, ud, vd, wd, cd, want_scores=True)
        assert scores.shape == (n, L) and np.array_equal(hip_ops.to_host(scores), ref.astype(np.float64))
        assert pred.dtype == torch.int64 and np.array_equal(hip_ops.to_host(pred), ref.argmax(1) if n else np.zeros(0, dtype=np.int64))
        pred2, none = hip_ops.tucker_predict(users, items, ud, vd, wd, cd, want_scores=False)
        assert none is None and torch.equal(pred, pred2)
        if L >= 2:
            assert ((ref == ref.max(1, keepdims=True)).sum(1) > 1).all()


def test_tucker_predict_of_17_feedback_columns_is_refused(hip_ops):
    from polara_amd._lib import PolaraHipError
    with pytest.raises(PolaraHipError, match='r2 <= 16'):
        hip_ops.tucker_predict(np.zeros(3, np.int64), np.zeros(3, np.int64), np.ones((2, 2)), np.ones((2, 2)), np.ones((4, 17)),
                               np.ones((2, 2, 17)))

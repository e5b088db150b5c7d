"""-m gpu: every instance of the packed fold-in (csrc/foldq.hip: fold_q20_kernel, fold_q20_fixup_kernel) at every boundary of
its software pipeline, against NumPy on a hand-made image whose product does not depend on the summation order.

The launcher picks an instance by the value type of A and the lane class of the rank (L = 2 / 4 / 8 / 16 / 32 lanes per row for
K <= 12 / 25 / 50 / 101 / 202, with U = 1 / 2 / 4 / 4 / 4 steps per register set); the test ids spell the instance out, so that the
branches can be ticked off from `pytest --collect-only`:

  branch                                                          ids that reach it
  launch_fold_q20<float>   L = 2, 4, 8, 16, 32                    vals32_L{2,4,8,16,32}_K*_split256 (test_fold_exact)
  launch_fold_q20<double>  L = 2, 4, 8, 16, 32                    vals64_L{2,4,8,16,32}_K*_split256 (test_fold_exact)
  pk_fold_q20_zero         its refusals                           refused_* (test_fold_refusals)
                           n_tasks == 0                           vals32_L8_K50_split256_zero*_notasks
                           fix-up sums (n_long > 0)               every ..._split256 / ..._split64 id on the full ladder
                           fix-up of one workgroup that only      ..._zero*_nolong, ..._zero*_notasks
                             zeroes (n_long == 0, zero_n > 0)
                           no fix-up (n_long == 0, zero_n == 0)   ..._split2048 (test_fold_plans), ..._rows0to1, ..._rows210to212
  fold_q20_kernel          slot < 0: stores to `out`              every id (205 rows of split256, all rows of split2048)
                           slot >= 0: stores to `partial`         ..._split256 (7 rows, 21 slots), ..._split64 (145 rows of 2 .. 24)
                           an odd number of sets per chunk        not instantiated: L / U = 2, 2, 2, 4, 8 sets
                           `have`, `have_next`, skipped steps     every id on the full ladder: tasks of 0 .. 200, 255 .. 258, 511 ..
                                                                  513, 769 entries and the halves / slots of the split rows
                           prefetch two chunks ahead, at depth    ..._split2048: the row of 1500 entries as ONE task of 24 chunks
                           extra columns (6 L + e < K)            ..._L4_K25, ..._L8_K{49,50}, ..._L16_K{97,101}, ..._L32_K{193,202}
                           none, a partly filled last lane        ..._K{1,7,13,18,26,51,102}
                           zero fill of K + 1 .. Kx - 1           every id with Kx > K + 1; ..._kx1_ld* (test_fold_kx_and_strides):
                                                                  the loop does not run
                           t0, l0 offsets into the plan           ..._rows150to209 (test_fold_row_ranges)
  fold_q20_fixup_kernel    workgroup 0 zeroes, r < n_long sums    ..._zero{1,3,256,257,1000}_full
                           r >= n_long returns                    ..._zero*_nolong, ..._zero*_notasks
  q20_encode_kernel        last workgroup clamped to row n - 1    small_n{1,2,3,4,5,63,64,65}_K* (test_encode_small_catalogues)
(rounded_* and streams_* ids: the same instances on the real encoder's image, tolerance and determinism.)

The ladder is the one of test_gpu_row_task_instances (rows of 0 .. 200, 255, 256, 257, 258, 511, 512, 513, 769, 1500 entries and
two empty rows; no entry references item 0, many rows reference the last item), with values 1 .. 4, under three plans: split =
256 (257 -> 129 + 128), split = 64 (rows of 2 .. 24 slots) and split = 2048 (no row split: the 1500-entry row runs 24 chunks).

Exact data (`image_host`; proven for the committed ranges on the CPU by
test_q20_format.py::test_hand_made_image_makes_the_fold_in_exact): field 0 of a lane in {-32, -16, 0, 16}, field 1 in [0, 31],
fields 2 .. 5 in [-32, 31], digits in [-2, 1], the weight digit in {0, 1}, tab[b] = 2^-(12 + b mod 3).  Every window converts
to fp32 without rounding, fl32(a s) is exact, every fp32 sum of up to U = 4 products fits 24 bits and every fp64 row sum 53:
the product is the same in every order and is compared with `np.array_equal`.  The scale differs between neighbouring
brackets, so that a scale taken from the wrong chunk's index changes the result.  Column K is one rounded multiply,
pk_q20_kappa(K) * (exact digit sum), PER TASK: a split row's column K is the sum, in slot order, of its tasks' rounded products
(`reference` restates that with the host plan of polara_amd.csr.build_row_tasks, which test_fold_plans_are_the_host_plans
holds the device plan to).  Item 0 is the canary: fields 0x7FFFF, digits 127, tab[0] = 1 — a padded lane that carried a weight,
or a step consumed beyond the count with a live weight, shows as about 2^31.

What the net catches, tried on scratch builds with one arithmetic-only change each (new cases failed / run; earlier tests of
the fold-in, tests/test_gpu_foldq.py + tests/test_gpu_pass_chain.py, failed / run):
  fold_q20_kernel        `have = k * U * GROUPS < cnt - 1`                             134 / 227    18 / 62
  fold_q20_kernel        `sn = tab[pk_q20_bracket((unsigned)jc)]` (the current chunk)   124 / 227    17 / 62
  fold_q20_kernel        `p + 128 + lane < n - 1` (the prefetch two chunks ahead)       124 / 227    17 / 62
  fold_q20_fixup_kernel  `s < s1 - 1`                                                   119 / 227    12 / 62
  fold_q20_kernel        `more = p + 64 < n - 1` (wrong for tasks of 64 m + 1 entries)   124 / 227     5 / 62
  fold_q20_kernel        `cnt_next = ... ? (n - p - 64) - 1 : 64` (a skipped gather)      88 / 227     4 / 62
  fold_q20_kernel        `6 * L + e <= K` (the store of an extra column)                  0 / 227     0 / 62
(`more`: none of the 12 cases of the earlier test of the fold-in itself, only the scoring passes behind it.  `cnt_next`: every
exact case but those of L = 2, whose U = 1 has no later step to skip, and no rounded one: SUBSET has no task of
64 m + u GROUPS + 1 entries, the ladder has them all.  What stays green under the first four: the encoder's cases, the
refusals, the plans, the launches without a task or of empty rows only, the determinism of two equally wrong launches — and
split64 under the changes that need a second chunk.  A failing exact case names the row lengths that differ, e.g. "rows of
[129, 130, ... 1500] entries differ" under the third change.)  The last change is no error: it makes the top lane of
an extra column e with 6 L + e == K store to dst[K], and the store of kappa * dsum to dst[K] — by lane L - 1 of the same
wave, later in program order — overwrites it; the memory a launch leaves is the same, with Kx = K + 1 and in a partial slot too
(K = 24, 48, 49, 96, 97, 192, 193, where it stores, are among the ranks of test_fold_exact and test_fold_kx_and_strides)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import q20_reference as q20
from test_gpu_row_task_instances import LADDER, N_COLS, N_ROWS, SENTINEL, SUBSET, device_csr, ladder_host, subset_host

pytestmark = pytest.mark.gpu

SPLITS = (256, 64, 2048)                    # 2048: above the longest row, no row is split
EXACT_K = [1, 6, 7, 12, 13, 18, 24, 25, 26, 48, 49, 50, 51, 96, 97, 101, 102, 192, 193, 202]
CLASS_K = [12, 25, 50, 101, 202]
ROUNDED_K = [12, 13, 25, 50, 51, 101, 202]
EMPTY_ROWS = [0, N_ROWS - 2, N_ROWS - 1]


def fold_id(vbits, K, split=256, tail=''):
    return 'vals%d_L%d_K%d_split%d%s' % (vbits, q20.lanes(K), K, split, tail)


def kx_of(K):
    return -(-(K + 1) // 4) * 4


# ---- host side: built once, read-only -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fold_host():
    """the ladder's index structure with values 1 .. 4"""
    h = ladder_host()
    values = np.random.RandomState(420).randint(1, 5, len(h['indices'])).astype(np.int64)
    values.setflags(write=False)
    return dict(indptr=h['indptr'], indices=h['indices'], values=values)


@functools.lru_cache(maxsize=None)
def image_host(K, n=N_COLS):
    """the hand-made image of `n` items at rank K: fields p [n, L, 6], digits [n, L], the bits, the scale table, what the bits
    decode to and — restated from the fields, not from the decoder — the weight windows in real units (column K / kappa)"""
    L = q20.lanes(K)
    rng = np.random.RandomState(7000 + K)
    p = np.empty((n, L, 6), dtype=np.int64)
    p[:, :, 0] = rng.choice([-32, -16, 0, 16], (n, L))
    p[:, :, 1] = rng.randint(0, 32, (n, L))
    p[:, :, 2:] = rng.randint(-32, 32, (n, L, 4))
    dig = rng.randint(-2, 2, (n, L)).astype(np.int64)
    dig[:, L - 1] = rng.randint(0, 2, n)
    p[0], dig[0] = 0x7FFFF, 127                                               # the canary
    tab = 2.0 ** -(12.0 + np.arange(q20.TAB) % 3)
    tab[0] = 1.0
    bits = q20.pack(p, dig)
    dec = q20.decode(bits, tab, K)
    s = tab[q20.bracket(np.arange(n))]
    weight = (dig[:, L - 1] * 2 ** 24 + ((p[:, L - 1, 0] & 0xFFFFF) << 4) + ((p[:, L - 1, 1] & 0xFFFFF) >> 16)) * s
    for a in (p, dig, bits, tab, dec, weight):
        a.setflags(write=False)
    return dict(p=p, dig=dig, bits=bits, tab=tab, dec=dec, weight=weight)


@functools.lru_cache(maxsize=None)
def host_plan(split):
    from polara_amd.csr import build_row_tasks
    return build_row_tasks(fold_host()['indptr'], split)


@functools.lru_cache(maxsize=None)
def reference(K, split, kappa):
    """fp64 [N_ROWS, K + 1]: columns [0, K) = scipy_csr(int values) @ decode, exact in any order; column K = the sum in slot order
    of kappa * (exact digit sum of the task), what the kernel stores per task and the fix-up adds"""
    h, im, plan = fold_host(), image_host(K), host_plan(split)
    S = sps.csr_matrix((h['values'], h['indices'], h['indptr']), shape=(N_ROWS, N_COLS))
    ref = np.zeros((N_ROWS, K + 1))
    ref[:, :K] = S @ im['dec'][:, :K]
    nnz = int(h['indptr'][-1])
    assert (plan['task_begin'][1:] == plan['task_end'][:-1]).all() and plan['task_begin'][0] == 0 and plan['task_end'][-1] == nnz
    T = sps.csr_matrix((h['values'], h['indices'], np.r_[plan['task_begin'], nnz]), shape=(len(plan['task_row']), N_COLS))
    part = kappa * (T @ im['weight'])                                         # one rounding per task
    for t, r in enumerate(plan['task_row'].tolist()):                         # tasks are in row and slot order
        ref[r, K] += part[t]
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def rounded_host(K):
    """the 32 rows of SUBSET with |fp32 normals| as values and Gaussian factors with the decay of test_gpu_foldq.factors"""
    from test_gpu_foldq import factors
    s = subset_host()
    values = np.abs(s['values'])
    V = factors(np.random.default_rng(K), N_COLS, K)
    M = sps.csr_matrix((values.astype(np.float64), s['indices'], s['indptr']), shape=(len(SUBSET), N_COLS))
    for a in (values, V):
        a.setflags(write=False)
    return dict(indptr=s['indptr'], indices=s['indices'], values=values, V=V, M=M)


# ---- device side ----------------------------------------------------------------------------------------------------------
_DEVICE = {}


def fold_ladder(ops, vbits, split=256):
    A = device_csr(ops, fold_host(), vbits, N_ROWS, split, key='foldq-ladder')
    assert A.values.dtype == (torch.float32 if vbits == 32 else torch.float64)
    return A


def fold_subset(ops, vbits, K):
    return device_csr(ops, rounded_host(K), vbits, len(SUBSET), key='foldq-subset')       # (the values do not depend on K)


def aligned_image(ops, bits):
    raw = torch.empty(bits.size + 128, dtype=torch.uint8, device=ops.device)
    off = (-raw.data_ptr()) % 128
    img = raw[off:off + bits.size].view(bits.shape[0], bits.shape[1])
    img.copy_(torch.from_numpy(bits.copy()).to(ops.device))
    return img


def exact_image(ops, K):
    if ('exact', K) not in _DEVICE:
        im = image_host(K)
        _DEVICE['exact', K] = (aligned_image(ops, im['bits']), ops.to_device(im['tab']))
    return _DEVICE['exact', K]


def encoded_image(ops, K):
    """(device image of the real encoder, what its bits decode to on the host)"""
    if ('encoded', K) not in _DEVICE:
        img = ops.q20_encode(ops.to_device(rounded_host(K)['V']))
        assert img is not None
        dec = q20.decode(ops.to_host(img[0]), ops.to_host(img[1]), K)
        dec.setflags(write=False)
        _DEVICE['encoded', K] = (img, dec)
    return _DEVICE['encoded', K]


def lib_kappa(ops, K):
    kappa = float(ops.lib.pk_q20_kappa(K))
    assert abs(kappa - q20.kappa(K)) < 1e-12 * kappa
    return kappa


def out_buffer(ops, n_rows, Kx, spare=3):
    """(buffer of sentinels with `spare` more columns, the [n_rows x Kx] view a launch writes)"""
    buf = torch.full((n_rows, Kx + spare), SENTINEL, dtype=torch.float64, device=ops.device)
    return buf, buf[:, :Kx]


def check_fold(ops, buf, K, Kx, want, rows=None):
    """on `rows` (a mask; all by default) columns [0, K] of `buf` equal `want` bit for bit and columns (K, Kx) are zero, empty
    rows among them are zero throughout, everything else is the sentinel; a failure names the row LENGTHS that differ"""
    got = ops.to_host(buf)
    hit = np.ones(len(got), dtype=bool) if rows is None else rows
    bad = np.flatnonzero(hit & (got[:, :K + 1] != want).any(axis=1))
    assert len(bad) == 0, 'rows of %s entries differ, first by %s' % (
        [LADDER[r] for r in bad], (got[bad[0], :K + 1] - want[bad[0]])[got[bad[0], :K + 1] != want[bad[0]]][:4])
    assert (got[hit, K + 1:Kx] == 0.0).all()
    empty = [r for r in EMPTY_ROWS if hit[r]]
    assert (got[empty, :Kx] == 0.0).all()
    assert (got[~hit] == SENTINEL).all() and (got[:, Kx:] == SENTINEL).all()
    return got


# ---- the plans ------------------------------------------------------------------------------------------------------------
def test_fold_plans_are_the_host_plans(hip_ops):
    """`reference` sums column K along the host's restatement of the plan: the device plans are that plan"""
    for split, n_long, slots in zip(SPLITS, (7, 145, 0), ((2, 6), (2, 24), None)):
        A, want = fold_ladder(hip_ops, 32, split), host_plan(split)
        assert A.n_long == n_long == len(want['long_row']) and A.n_tasks == len(want['task_row']) and A.n_slots == want['n_slots']
        for name in ('task_row', 'task_begin', 'task_end', 'task_slot'):
            assert np.array_equal(hip_ops.to_host(A.plan[name])[:A.n_tasks], want[name]), name
        if n_long:
            per_row = want['long_slot_end'] - want['long_slot_begin']
            assert (per_row.min(), per_row.max()) == slots
            for name in ('long_row', 'long_slot_begin', 'long_slot_end'):
                assert np.array_equal(hip_ops.to_host(A.plan[name])[:n_long], want[name]), name
    lengths = host_plan(2048)['task_end'] - host_plan(2048)['task_begin']
    assert lengths.max() == 1500 and -(-1500 // 64) == 24
    halves = host_plan(256)['task_end'] - host_plan(256)['task_begin']
    assert halves[LADDER.index(257):LADDER.index(257) + 2].tolist() == [129, 128]


# ---- exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vbits,K', [pytest.param(vb, K, id=fold_id(vb, K)) for K in EXACT_K for vb in (32, 64)])
def test_fold_exact(hip_ops, vbits, K):
    """both edges of every lane class and the ranks where the extra columns and a partly filled last lane appear, to the last
    bit, into a strided view of a buffer of sentinels"""
    Kx = kx_of(K)
    A = fold_ladder(hip_ops, vbits)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    hip_ops.fold_q20(A, exact_image(hip_ops, K), K, out)
    check_fold(hip_ops, buf, K, Kx, reference(K, 256, lib_kappa(hip_ops, K)))


@pytest.mark.parametrize('vbits,K,split', [pytest.param(vb, K, sp, id=fold_id(vb, K, sp))
                                           for K in CLASS_K for sp in (64, 2048) for vb in (32, 64)])
def test_fold_plans(hip_ops, vbits, K, split):
    """rows of 2 .. 24 slots (the fix-up's sum in slot order), and no split at all: the 1500-entry row as one task of 24
    chunks, where the prefetch two chunks ahead runs at depth"""
    Kx = kx_of(K)
    A = fold_ladder(hip_ops, vbits, split)
    assert (A.n_long == 0 and A.partial(Kx) is None) if split == 2048 else A.n_long == 145
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    hip_ops.fold_q20(A, exact_image(hip_ops, K), K, out)
    check_fold(hip_ops, buf, K, Kx, reference(K, split, lib_kappa(hip_ops, K)))


KX_CASES = [(vb, K, dkx, spare) for vb, Ks in ((32, (6, 18, 48, 96, 192)), (64, (7, 25, 49, 97, 193)))
            for K in Ks for dkx in (1, 7) for spare in (0, 3)]


@pytest.mark.parametrize('vbits,K,dkx,spare', [pytest.param(*c, id=fold_id(c[0], c[1], tail='_kx%d_ld%d' % (c[2], c[2] + c[3])))
                                               for c in KX_CASES])
def test_fold_kx_and_strides(hip_ops, vbits, K, dkx, spare):
    """Kx = K + 1 (the zero fill does not run) and K + 7 (odd widths of the partial slots), ldo = Kx and Kx + 3, per lane class
    an even and an odd rank"""
    Kx = K + dkx
    A = fold_ladder(hip_ops, vbits)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx, spare)
    assert out.stride(0) == Kx + spare and out.shape[1] == Kx
    hip_ops.fold_q20(A, exact_image(hip_ops, K), K, out)
    check_fold(hip_ops, buf, K, Kx, reference(K, 256, lib_kappa(hip_ops, K)))


ROW_RANGES = [(150, 209), (0, 1), (N_ROWS - 2, N_ROWS)]


@pytest.mark.parametrize('vbits,K,lo,hi', [pytest.param(vb, K, lo, hi, id=fold_id(vb, K, tail='_rows%dto%d' % (lo, hi)))
                                           for K in CLASS_K for vb in (32, 64) for lo, hi in ROW_RANGES])
def test_fold_row_ranges(hip_ops, vbits, K, lo, hi):
    """a row range is its own launch with offsets into the plan: its rows get the bits of the full launch, every other row
    keeps what it held — (150, 209) holds six of the seven split rows, (0, 1) one empty row, (210, 212) the trailing empty ones"""
    Kx = kx_of(K)
    A = fold_ladder(hip_ops, vbits)
    image = exact_image(hip_ops, K)
    t0, n_tasks, l0, n_long = A.task_range(lo, hi)
    assert (n_tasks, l0, n_long) == ((hi - lo - 6 + 15, 0, 6) if lo == 150 else (hi - lo, 0 if lo == 0 else 7, 0)) and (t0 > 0) == (lo > 0)
    _, full = out_buffer(hip_ops, N_ROWS, Kx)
    hip_ops.fold_q20(A, image, K, full)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    hip_ops.fold_q20(A, image, K, out, rows=(lo, hi))
    inside = (np.arange(N_ROWS) >= lo) & (np.arange(N_ROWS) < hi)
    got = check_fold(hip_ops, buf, K, Kx, reference(K, 256, lib_kappa(hip_ops, K)), rows=inside)
    assert np.array_equal(got[inside, :Kx], hip_ops.to_host(full)[inside])


# ---- the counters ---------------------------------------------------------------------------------------------------------
ZERO_MODES = {'full': None, 'nolong': (10, 150), 'notasks': (5, 5)}


@pytest.mark.parametrize('zero_n,mode', [pytest.param(z, m, id=fold_id(32, 50, tail='_zero%d_%s' % (z, m)))
                                         for m in ZERO_MODES for z in (1, 3, 256, 257, 1000)])
def test_fold_zero_counters(hip_ops, zero_n, mode):
    """pk_fold_q20_zero: counters [0, zero_n) preset to -1 are zero behind the launch, the ones beyond stay -1, the product is
    that of pk_fold_q20 — with split rows (the fix-up sums and zeroes), without (one workgroup that only zeroes), without a task"""
    K, Kx, rows = 50, kx_of(50), ZERO_MODES[mode]
    A = fold_ladder(hip_ops, 32)
    image = exact_image(hip_ops, K)
    n_tasks, n_long = (A.n_tasks, A.n_long) if rows is None else A.task_range(*rows)[1::2]
    assert (n_tasks > 0, n_long > 0) == {'full': (True, True), 'nolong': (True, False), 'notasks': (False, False)}[mode]
    counters = torch.full((zero_n + 8,), -1, dtype=torch.int32, device=hip_ops.device)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    hip_ops.fold_q20(A, image, K, out, rows=rows, counters=counters[:zero_n])
    c = hip_ops.to_host(counters)
    assert (c[:zero_n] == 0).all() and (c[zero_n:] == -1).all()
    plain_buf, plain = out_buffer(hip_ops, N_ROWS, Kx)
    if n_tasks:
        hip_ops.fold_q20(A, image, K, plain, rows=rows)
    inside = np.ones(N_ROWS, dtype=bool) if rows is None else (np.arange(N_ROWS) >= rows[0]) & (np.arange(N_ROWS) < rows[1])
    got = check_fold(hip_ops, buf, K, Kx, reference(K, 256, lib_kappa(hip_ops, K)), rows=inside)
    assert np.array_equal(got, hip_ops.to_host(plain_buf))


# ---- rounded data ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vbits,K', [pytest.param(vb, K, id='rounded_' + fold_id(vb, K)) for K in ROUNDED_K for vb in (32, 64)])
def test_fold_rounded(hip_ops, vbits, K):
    """the real encoder's image of Gaussian factors, |fp32 normals| as values, the 32 lengths of SUBSET: the two bounds the
    project states — the product of the decoded rows to within the kernel's fp32 arithmetic, and the exact product to within
    the weight the launch returns"""
    r = rounded_host(K)
    A = fold_subset(hip_ops, vbits, K)
    image, dec = encoded_image(hip_ops, K)
    Kx = kx_of(K)
    buf, out = out_buffer(hip_ops, len(SUBSET), Kx)
    hip_ops.fold_q20(A, image, K, out)
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


@pytest.mark.parametrize('vbits,K', [pytest.param(vb, K, id='streams_' + fold_id(vb, K)) for vb, K in zip((32, 64, 32, 64, 32), CLASS_K)])
def test_fold_determinism(hip_ops, vbits, K):
    """two launches on two streams of the same HipOps (each with its own partial buffer) return the bits of the launch on
    the current stream — on rounded data, where another order of the sums would show"""
    A = fold_subset(hip_ops, vbits, K)
    image, _ = encoded_image(hip_ops, K)
    Kx = kx_of(K)
    outs = [out_buffer(hip_ops, len(SUBSET), Kx)[1] for _ in range(3)]
    hip_ops.fold_q20(A, image, K, outs[0])
    torch.cuda.synchronize(hip_ops.device)
    for out in outs[1:]:
        with torch.cuda.stream(torch.cuda.Stream(device=hip_ops.device)):
            hip_ops.fold_q20(A, image, K, out)
    torch.cuda.synchronize(hip_ops.device)
    first = hip_ops.to_host(outs[0])
    assert np.isfinite(first).all() and np.abs(first[1:, :K]).max() > 0
    assert np.array_equal(hip_ops.to_host(outs[1]), first) and np.array_equal(hip_ops.to_host(outs[2]), first)


# ---- the encoder on catalogues of a few rows --------------------------------------------------------------------------------
@pytest.mark.parametrize('n,K', [pytest.param(n, K, id='small_n%d_K%d' % (n, K))
                                 for n in (1, 2, 3, 4, 5, 63, 64, 65) for K in (1, 12, 13, 25, 50, 101, 202)])
def test_encode_small_catalogues(hip_ops, n, K):
    """brackets 0 .. 3 of one item each, a last workgroup mostly clamped to row n - 1, digit shuffles next to dead lanes: the
    device decoder and the NumPy decoder agree bit for bit, every row lies within its own D_j, the scales are `q20.scales`"""
    rng = np.random.default_rng(1000 * n + K)
    V = rng.standard_normal((n, K)) * ((np.arange(n) + 1.0) ** -0.4)[:, None]
    if n > 8:
        V[7] = 0.0
    img = hip_ops.q20_encode(hip_ops.to_device(V))
    assert img is not None
    bits, tab = hip_ops.to_host(img[0]), hip_ops.to_host(img[1])
    assert bits.shape == (n, q20.lanes(K) * 16)
    dec = hip_ops.to_host(hip_ops.q20_decode(img, K))
    assert dec.shape == (n, K + 1) and np.array_equal(dec, q20.decode(bits, tab, K))
    err = np.linalg.norm(dec[:, :K] - V, axis=1)
    print('largest error / weight: %.3f' % (err / np.maximum(dec[:, K] * 2.0 ** -24, 1e-300)).max())
    assert (err <= dec[:, K] * 2.0 ** -24).all()
    assert np.array_equal(tab, q20.scales(V))


# ---- refusals -------------------------------------------------------------------------------------------------------------
REFUSALS = {'K203': dict(K=203, Kx=204), 'kx_equals_K': dict(Kx=50), 'ldo_below_kx': dict(ldo=51), 'val_kind7': dict(val_kind=7),
            'no_partial_buffer': dict(partial=None), 'items_2p24': dict(n_items=1 << 24)}


@pytest.mark.parametrize('what', list(REFUSALS), ids=lambda w: 'refused_' + w)
def test_fold_refusals(hip_ops, what):
    """raw pk_fold_q20 calls outside the contract return an error and launch nothing: the output keeps its sentinels"""
    from polara_amd.ops import _ptr
    K, Kx = 50, 52
    A = fold_ladder(hip_ops, 32)
    img, tab = exact_image(hip_ops, K)
    buf, out = out_buffer(hip_ops, N_ROWS, Kx)
    a = dict(K=K, Kx=Kx, ldo=out.stride(0), val_kind=A.val_kind, partial=A.partial(Kx), n_items=N_COLS)
    a.update(REFUSALS[what])
    p = A.plan
    assert A.n_long > 0
    rc = hip_ops.lib.pk_fold_q20(hip_ops.stream(), A.n_tasks, _ptr(p['task_row']), _ptr(p['task_begin']), _ptr(p['task_end']),
                                 _ptr(p['task_slot']), A.n_long, _ptr(p['long_row']), _ptr(p['long_slot_begin']),
                                 _ptr(p['long_slot_end']), _ptr(A.indices), _ptr(A.values), a['val_kind'], _ptr(img), _ptr(tab),
                                 a['n_items'], a['K'], a['Kx'], _ptr(out), a['ldo'], _ptr(a['partial']))
    assert rc != 0 and b'pk_fold_q20' in hip_ops.lib.pk_last_error()
    assert (hip_ops.to_host(buf) == SENTINEL).all()

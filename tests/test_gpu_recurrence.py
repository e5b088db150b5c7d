"""-m gpu: the block Lanczos recurrence inside the library, one call at a time (pk_lanczos_steps / pk_lanczos_products /
pk_lanczos_orth / pk_gramian_apply_f64 through ops.LanczosRecurrence), and the three small entries nothing else calls
directly (pk_tsmm_axpby_f64, pk_orth_check_f64, pk_eigh_psd_rounds_f64) — each against a plain fp64 NumPy/SciPy statement of
the same operation written in this file.  Nothing is taken from the solver's composition of the step: `svd_topk` verifies,
re-looks and falls back, so a wrong mirror image, coupling, `rounded` flag, breakdown flag or span would still end in
"converged" there.

The step is checked against its DEFINITION on the device's own basis: with Q = the device's Q[:, :N] as it stands,
W_ref = A^T (A Q_j) on the host, block column j of T = Q^T W_ref, the next block = the QR factor (positive diagonal) of
W_perp_ref = (I - Q Q^T)^2 W_ref, S_out = W_perp_ref^T W_perp_ref.  Two figures of the reference carry the tolerances that
depend on the input: ratio = |W|_F / |W_perp|_F (W_perp is a difference of terms of size |W|) and cond(W_perp); every test
that uses them first asserts ratio < 1e3 and cond < 1e4, so other inputs fail loudly instead of going lax.

Input cases (CASES / STEP_CONFIGS below), the two figures of the reference on them and the worst value of every asserted
quantity that one run on an MI355X gave (each test prints them as `OBSERVED ...` lines under `pytest -s`).  Worst over steps
1 .. J; the closing step J + 1 (test_last_closes) apart.  "/tol" = observed / the tolerance derived from ratio and cond.

    case            general   general   general   general   general   blocked200  blocked64  blocked96  twoblock112
    A               3000x700  3000x700  3000x700  3000x700  3000x700  40000x200   70000x64   40000x96   70000x112
    values, b, J    f32 16 6  f64 64 4  f32 7 6   f64 4 6   f32 1 6   f32 64 2    f64 16 3   f32 16 4   f32 16 4
    user blocks     1         1         1         1         1         3           2          1          2
    ratio           7.74      3.35      7.22      4.80      25.5      22.1        53.2       31.6       35.3       (< 1e3)
    cond(W_perp)    9.92      6.04      8.02      5.84      1         94.0        28.4       44.5       54.8       (< 1e4)
    Householder     1.1e-15   1.3e-15   1.1e-15   1.0e-15   4.4e-16   1.1e-15     7.8e-16    7.8e-16    1.0e-15    (reference basis)
    T column        1.6e-15   8.5e-16   1.0e-15   8.0e-16   1.4e-15   1.0e-15     8.5e-16    6.3e-16    5.0e-16    (< 1e-12)
    orthonormality  1.2e-15   1.3e-15   1.1e-15   1.1e-15   4.4e-16   1.3e-15     6.7e-16    8.9e-16    8.9e-16    (< 1e-12)
    span            9.4e-16   7.2e-16   9.9e-16   9.9e-16   1.4e-15   9.3e-16     1.4e-15    1.1e-15    1.4e-15    (<= 1e-12)
    R lower / b     2.5e-17   3.9e-18   2.8e-17   8.1e-17   0         1.2e-16     2.0e-15    7.3e-16    9.2e-16    (<= 1e-12)
    direct          2.0e-15   6.0e-16   6.4e-16   2.5e-15   4.8e-16   1.1e-14     7.0e-14    1.9e-14    2.2e-14
    direct /tol     9.9e-4    6.6e-4    6.7e-4    2.5e-3    5.4e-4    1.7e-4      1.7e-3     1.3e-3     2.1e-3     (<= 1)
    coupling /tol   4.7e-4    5.4e-4    4.3e-4    9.9e-4    1.5e-4    4.8e-4      7.7e-4     6.3e-4     1.1e-3     (<= 1)
    flags[1]        6.7e-16   6.7e-16   6.7e-16   4.4e-16   4.4e-16   1.0e-15     8.9e-16    6.7e-16    8.9e-16    (< 1e-4)
    closing: ratio  3.01      3.41      2.90      2.81      2.43      60.5        (full)     46.8       41.2       (< 1e3)
      T column      3.9e-17   2.4e-16   5.9e-17   2.9e-16   5.0e-17   2.7e-16     1.2e-15    3.1e-16    1.5e-16    (< 1e-12)
      coupling /tol 2.6e-4    2.7e-4    3.5e-4    1.9e-4    8.3e-5    1.4e-4      7.5e-8*    2.9e-4     6.3e-4     (<= 1)
    rounded vs exact / bound      0.092  0.104  -  0.100  -  0.240  0.241  0.217  0.224                            (<= 1)
    rounded vs host-rounded / bound  0  7.6e-9  -  6.0e-9  -  0      4.3e-8  0      0                              (<= 1)
    rounded moved (least)         3.7e-8 3.2e-8 -  3.1e-8 -  3.6e-8 2.9e-8 3.9e-8 3.9e-8                           (> 1e-10)
    band of T       1.6e-16   2.4e-16   -         2.9e-16   -         2.7e-16     -          2.4e-16    1.0e-16    (< 1e-12)

    * the full space (N = n): |S|max against (1e-12 |W|_F)^2, see test_last_closes.
    gramian (worst over its handles and widths): general 8.2e-16, blocked200 1.9e-15, blocked64 3.6e-15, blocked96 3.1e-15,
    twoblock112 4.0e-15 (< 1e-13).  Breakdown on the rank-5 matrix: flags = [0, 0.84] after two steps, [0, 0.88] after three.
    pk_tsmm_axpby_f64: at most 2.7e-16 over the seven shapes, the same figure on both load paths (< 1e-13).
    pk_eigh_psd_rounds_f64, n = 5 .. 301: eigenvalues to 6.3e-15 of the largest (<= 1e-12), orthonormality 7.7e-15 (< 1e-12),
    5 or 6 sweeps (3 at n = 5).

So the input-dependent tolerances are at most 1e-13 * 94 * 22 = 2e-10 (direct comparison of the next block) and 5e-11
(coupling), and every fixed one is met with three orders of margin or more.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from polara_amd import _lib
from polara_amd.ops import _ptr

pytestmark = pytest.mark.gpu

NAN = float('nan')

# name -> (rows, columns, mean row length)
CASES = {
    'general': (3000, 700, 25),
    'blocked200': (40000, 200, 5),
    'blocked64': (70000, 64, 4),
    'blocked96': (40000, 96, 5),
    'twoblock112': (70000, 112, 5),
}
# (case, value kind, b, steps J, user blocks of the library's transposed image, rows per block).  The block counts restate
# ensure_blocked_transpose by hand: a block holds 16 384 * max(1, 64 / max(16, b)) users (more where a (block, item) task would
# hold fewer than 64 entries: never here), rounded up to 4096, and a matrix below 32 768 rows or 1 block's rows is one block.
#   40 000 x 200, b = 64: 16 384 rows per block -> 3;   70 000 x 64, b = 16: 65 536 -> 2 ((J + 1) b = 64 fills the space);
#   40 000 x 96, b = 16: 65 536 > 40 000 -> ONE block of 40 000 rows (the third "blocked" shape is blocked at b = 64 only:
#   test_gramian_against_scipy runs it there with 3 blocks);   70 000 x 112, b = 16: 65 536 -> 2, the mid-width shape that IS
#   blocked at b = 16 with room for its four steps, the closing fifth and a sixth block (96 of 112 columns)
STEP_CONFIGS = [
    ('general', 'f32', 16, 6, 1, 3000),
    ('general', 'f64', 64, 4, 1, 3000),
    ('general', 'f32', 7, 6, 1, 3000),
    ('general', 'f64', 4, 6, 1, 3000),
    ('general', 'f32', 1, 6, 1, 3000),
    ('blocked200', 'f32', 64, 2, 3, 16384),
    ('blocked64', 'f64', 16, 3, 2, 65536),
    ('blocked96', 'f32', 16, 4, 1, 40000),
    ('twoblock112', 'f32', 16, 4, 2, 65536),
]
FULL_SPACE = ('blocked64', 'f64', 16, 3, 2, 65536)      # after its 3 steps the basis spans all 64 columns


def _cfg_id(cfg):
    return '%s-%s-b%d' % cfg[:3]


# ---------------------------------------------------------------------------------------------------------- inputs
def rand_csr(seed, m, n, mean, val_kind):
    """Poisson row lengths; rows 0, 7 and m - 2 empty, row 5 of length n - 3, row m - 1 of length n // 2; columns 3 and n - 1
    empty; values integer 1..5 (fp32) or randn (fp64).  The pattern depends on the seed and the shape only."""
    rng = np.random.RandomState(seed)
    allowed = np.setdiff1d(np.arange(n), [3, n - 1])
    counts = rng.poisson(mean, m).clip(0, len(allowed))
    counts[[0, 7, m - 2]] = 0
    counts[5] = n - 3
    counts[m - 1] = n // 2
    order = np.argsort(rng.rand(m, len(allowed)), axis=1)
    take = np.arange(len(allowed))[None, :] < counts[:, None]
    sel = np.zeros((m, len(allowed)), dtype=bool)
    sel[np.nonzero(take)[0], order[take]] = True
    indices = allowed[np.nonzero(sel)[1]].astype(np.int32)           # row-major: sorted within every row
    indptr = np.r_[0, np.cumsum(counts)].astype(np.int64)
    if val_kind == 'f32':
        values = rng.randint(1, 6, indptr[-1]).astype(np.float32)
    else:
        values = rng.randn(indptr[-1])
    return indptr, indices, values


@functools.lru_cache(maxsize=None)
def host_case(name, val_kind):
    m, n, mean = CASES[name]
    indptr, indices, values = rand_csr(sorted(CASES).index(name) + 1, m, n, mean, val_kind)
    M = sps.csr_matrix((values.astype(np.float64), indices, indptr), shape=(m, n))
    assert M.nnz == indptr[-1] and (np.diff(indptr)[[0, 7, m - 2]] == 0).all()
    assert indptr[6] - indptr[5] == n - 3 and indptr[m] - indptr[m - 1] == n // 2
    assert not np.isin(indices, [3, n - 1]).any()
    return dict(M=M, Mt=M.T.tocsr(), absM=abs(M), absMt=abs(M).T.tocsr(), indptr=indptr, indices=indices, values=values, shape=(m, n))


_DEVICE = {}


def device_case(ops, name, val_kind):
    key = (name, val_kind)
    if key not in _DEVICE:
        h = host_case(name, val_kind)
        A = ops.csr(h['indptr'], h['indices'], h['values'], h['shape'])
        assert A.val_kind == (_lib.PK_VAL_F32 if val_kind == 'f32' else _lib.PK_VAL_F64)
        _DEVICE[key] = A
    return _DEVICE[key]


def start_block(n, b, seed=0):
    return np.linalg.qr(np.random.RandomState(1000 + seed + b).randn(n, b))[0]


class Buffers:
    """The buffers of a recurrence, each inside a wider NaN-filled allocation: the basis [n x (cols b + 4)] with Q_1 in its
    first b columns (leading dimension = its full width), T = zeros [cols b x cols b] in the corner of a NaN buffer with a
    leading dimension 6 beyond its width, S_out NaN, flags zeros(2)."""

    def __init__(self, ops, n, b, cols, Q1=None, ldq_spare=4):
        self.ops, self.n, self.b, self.cols = ops, n, b, cols
        self.Q = torch.full((n, cols * b + ldq_spare), NAN, dtype=torch.float64, device=ops.device)
        if Q1 is not None:
            self.Q[:, :b] = ops.to_device(Q1)
        self.Tbuf = torch.full((cols * b + 2, cols * b + 6), NAN, dtype=torch.float64, device=ops.device)
        self.T = self.Tbuf[:cols * b, :cols * b]
        self.T.zero_()
        self.S = torch.full((b, b), NAN, dtype=torch.float64, device=ops.device)
        self.flags = ops.zeros(2)

    def host(self):
        torch.cuda.synchronize()
        h = self.ops.to_host
        return dict(Q=h(self.Q), Tbuf=h(self.Tbuf), S=h(self.S), flags=h(self.flags))

    @classmethod
    def from_host(cls, ops, n, b, cols, state):
        new = cls(ops, n, b, cols)
        new.Q.copy_(ops.to_device(state['Q']))
        new.Tbuf.copy_(ops.to_device(state['Tbuf']))
        new.S.copy_(ops.to_device(state['S']))
        new.flags.copy_(ops.to_device(state['flags']))
        return new


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def states_identical(x, y):
    return all(same_bits(x[k], y[k]) for k in ('Q', 'Tbuf', 'S', 'flags'))


# ------------------------------------------------------------------------------------------------------ references
def reference_step(h, Q, N, b):
    """Step j = N / b by its definition on the GIVEN basis Q [n x N] (fp64, host)."""
    Qj = Q[:, N - b:N]
    W = h['Mt'] @ (h['M'] @ Qj)
    C = Q.T @ W
    Wp = W - Q @ C
    Wp = Wp - Q @ (Q.T @ Wp)                                   # projected twice
    nW, nWp = np.linalg.norm(W), np.linalg.norm(Wp)
    sv = np.linalg.svd(Wp, compute_uv=False)
    Qh, R = np.linalg.qr(Wp)                                    # Householder (LAPACK geqrf), signs fixed to diag(R) > 0
    Qh = Qh * np.where(np.diag(R) < 0, -1.0, 1.0)[None, :]
    return dict(W=W, C=C, Wp=Wp, S=Wp.T @ Wp, Qh=Qh, nW=nW, ratio=nW / max(nWp, 1e-300), cond=sv[0] / max(sv[-1], 1e-300),
                qh_orth=np.abs(Qh.T @ Qh - np.eye(b)).max())


_OBSERVED = {}


def observe(cfg, name, value, worst=max):
    d = _OBSERVED.setdefault(_cfg_id(cfg), {})
    d[name] = worst(d[name], float(value)) if name in d else float(value)
    return value


def report(cfg):
    print('\nOBSERVED %s %s' % (_cfg_id(cfg), ' '.join('%s=%.3g' % kv for kv in sorted(_OBSERVED.get(_cfg_id(cfg), {}).items()))))


_TRAJECTORY = {}


def trajectory(ops, cfg):
    """Steps j = 1 .. J of a configuration, one call each on buffers with room for J + 2 blocks; the buffers are read back
    after every call.  Computed once per configuration and left unchanged: [state after 0 steps, after 1, ..., after J]."""
    if cfg not in _TRAJECTORY:
        name, kind, b, J = cfg[:4]
        n = CASES[name][1]
        rec = ops.lanczos_recurrence(device_case(ops, name, kind), b)
        buf = Buffers(ops, n, b, J + 2, start_block(n, b))
        states = [buf.host()]
        for j in range(1, J + 1):
            rec.steps(buf.Q, buf.T, buf.S, buf.flags, j - 1, 1, False)
            states.append(buf.host())
        _TRAJECTORY[cfg] = states
    return _TRAJECTORY[cfg]


def check_block_column(cfg, h, st, ref, N, b, cols, tag=''):
    """Block column j of T against Q^T W_ref, its mirror image, and everything that must not have been written."""
    Tbuf = st['Tbuf']
    W = cols * b
    T = Tbuf[:W, :W]
    tmax = np.abs(T[:N, :N]).max()
    err = np.abs(T[:N, N - b:N] - ref['C']).max() / tmax
    observe(cfg, tag + 'T_column_rel', err)
    assert err < 1e-12, (N, err)
    assert same_bits(T[N - b:N, :N - b], T[:N - b, N - b:N].T), 'the mirror image is not the transpose, bit for bit (N=%d)' % N
    outside = T.copy()
    outside[:N, :N] = 0.0
    assert not outside.any(), 'T written outside [:N, :N] (N=%d)' % N
    assert np.isnan(Tbuf[W:]).all() and np.isnan(Tbuf[:, W:]).all(), 'T written beyond its width (N=%d)' % N


# ------------------------------------------------------------------------------------------------- 1. the products
# (case, value kind, block_cols of the handle, user blocks, rows per block): see STEP_CONFIGS for the rule
GRAMIAN_HANDLES = [
    ('general', 'f32', 16, 1, 3000), ('general', 'f64', 64, 1, 3000),
    ('blocked200', 'f32', 64, 3, 16384), ('blocked200', 'f32', 16, 1, 40000),
    ('blocked64', 'f64', 16, 2, 65536), ('blocked64', 'f64', 64, 5, 16384),
    ('blocked96', 'f32', 64, 3, 16384), ('blocked96', 'f32', 16, 1, 40000),
    ('twoblock112', 'f32', 16, 2, 65536),
]


@pytest.mark.parametrize('handle', GRAMIAN_HANDLES, ids=lambda c: '%s-%s-cols%d' % c[:3])
def test_gramian_against_scipy(hip_ops, handle):
    """pk_gramian_apply_f64: Z = A^T (A X) to 1e-13 of |Z|max (the suite's figure for spmm), exact zeros for empty columns, the
    same bits twice, strided operands — and the number of SpMM launches the library records for one product: 1 (A X) + one
    per user block of the transposed image, i.e. the blocked image really was used."""
    name, kind, cols, nb, rpb = handle
    h = host_case(name, kind)
    m, n = h['shape']
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), cols)
    rng = np.random.RandomState(cols)
    for nc in ([1, 8, 16, 40, 64] if name == 'general' else [16, 64]):
        X = rng.randn(n, nc)
        Xd = hip_ops.to_device(X)
        Z = hip_ops.to_host(rec.gramian(Xd))
        ref = h['Mt'] @ (h['M'] @ X)
        err = np.abs(Z - ref).max() / np.abs(ref).max()
        observe(handle, 'gramian_rel', err)
        assert err < 1e-13, (nc, err)
        assert not Z[[3, n - 1]].any(), 'rows of Z of the empty columns'
        assert same_bits(Z, hip_ops.to_host(rec.gramian(Xd))), nc
    # the raw entry with ldx / ldz > nc: column slices of wider buffers, NaN beyond
    nc = 16
    Xw = torch.full((n, nc + 3), NAN, dtype=torch.float64, device=hip_ops.device)
    Xw[:, :nc] = Xd[:, :nc]
    Zw = torch.full((n, nc + 5), NAN, dtype=torch.float64, device=hip_ops.device)
    _lib.check(hip_ops.lib.pk_gramian_apply_f64(rec.ctx, rec._stream(), rec.handle, nc, _ptr(Xw), Xw.stride(0), _ptr(Zw), Zw.stride(0)),
               'pk_gramian_apply_f64', hip_ops.lib, rec.ctx)
    Zw = hip_ops.to_host(Zw)
    assert np.isnan(Zw[:, nc:]).all() and same_bits(Zw[:, :nc], hip_ops.to_host(rec.gramian(Xd[:, :nc].contiguous())))
    # the launches of ONE product (the library times every SpMM launch it makes while ops.timers is set)
    hip_ops.timers = {}
    try:
        rec.gramian(Xd)
        rec.collect_timings()
        rows = hip_ops.timers.get('spmm', [])
    finally:
        hip_ops.timers = None
    rec.gramian(Xd)                                              # (switches the context's recording off again)
    meta = [r[2] for r in rows]
    assert len(meta) == 1 + nb, meta
    ve = 4 if kind == 'f32' else 8
    assert meta[0] == (m, n, h['M'].nnz, Xd.shape[1], ve, 8), meta[0]
    assert all(t[1] == rpb and t[3:] == (Xd.shape[1], ve, 8) for t in meta[1:]), meta
    assert [t[0] for t in meta[1:]] == [n] + [0] * (nb - 1) and sum(t[2] for t in meta[1:]) == h['M'].nnz
    edges = np.minimum(np.arange(nb + 1) * rpb, m)
    assert [t[2] for t in meta[1:]] == [int(h['indptr'][e1] - h['indptr'][e0]) for e0, e1 in zip(edges[:-1], edges[1:])]
    report(handle)


# ------------------------------------------------------------------------------- 2. one step against the definition
@pytest.mark.parametrize('cfg', STEP_CONFIGS, ids=_cfg_id)
def test_one_step_against_its_definition(hip_ops, cfg):
    name, kind, b, J = cfg[:4]
    h = host_case(name, kind)
    n = h['shape'][1]
    states = trajectory(hip_ops, cfg)
    Q1 = start_block(n, b)
    assert same_bits(states[0]['Q'][:, :b], Q1)
    for j in range(1, J + 1):
        st = states[j]
        N = j * b
        Q = st['Q'][:, :N]
        assert same_bits(Q, states[j - 1]['Q'][:, :N]), 'step %d changed earlier blocks of the basis' % j
        ref = reference_step(h, Q, N, b)
        observe(cfg, 'ratio', ref['ratio'])
        observe(cfg, 'cond', ref['cond'])
        observe(cfg, 'householder_orth', ref['qh_orth'])
        assert ref['ratio'] < 1e3 and ref['cond'] < 1e4, (j, ref['ratio'], ref['cond'])        # the inputs the tolerances were derived for
        check_block_column(cfg, h, st, ref, N, b, J + 2)
        # the next block
        assert np.isnan(st['Q'][:, N + b:]).all(), 'basis written beyond block %d' % (j + 1)
        Qf = st['Q'][:, :N + b]
        Qn = Qf[:, N:]
        orth = np.abs(Qf.T @ Qf - np.eye(N + b)).max()
        observe(cfg, 'orthonormality', orth)
        assert orth < 1e-12, (j, orth)
        W = ref['W']
        span = np.linalg.norm(W - Qf @ (Qf.T @ W)) / ref['nW']
        observe(cfg, 'span_rel', span)
        assert span <= 1e-12, (j, span)
        R = Qn.T @ ref['Wp']
        low = np.abs(np.tril(R, -1)).max() / np.abs(R).max() if b > 1 else 0.0
        observe(cfg, 'R_lower_rel_over_b', low / b)
        assert low <= b * 1e-12 and (np.diag(R) > 0).all(), (j, low, np.diag(R).min())
        direct = np.abs(Qn - ref['Qh']).max()
        observe(cfg, 'direct_over_tol', direct / (1e-13 * ref['cond'] * ref['ratio']))
        observe(cfg, 'direct_abs', direct)
        assert direct <= 1e-13 * ref['cond'] * ref['ratio'], (j, direct, ref['cond'], ref['ratio'])
        # the coupling
        serr = np.abs(st['S'] - ref['S']).max() / np.abs(ref['S']).max()
        observe(cfg, 'S_rel_over_tol', serr / (1e-12 * max(1.0, ref['ratio'])))
        assert serr <= 1e-12 * max(1.0, ref['ratio']), (j, serr)
        assert st['flags'][0] == 0 and st['flags'][1] < 1e-4, (j, st['flags'])
        observe(cfg, 'flags1', st['flags'][1])
    report(cfg)


# ------------------------------------------------------- 3. the whole step = its halves; m steps in a call = m calls
@pytest.mark.parametrize('cfg', STEP_CONFIGS, ids=_cfg_id)
def test_whole_step_equals_its_halves_and_m_steps_equal_m_calls(hip_ops, cfg):
    name, kind, b, J = cfg[:4]
    n = CASES[name][1]
    m = min(3, J)                                               # (40 000 x 200 at b = 64 has room for two steps only: there m = 2)
    states = trajectory(hip_ops, cfg)                           # route A: steps(j0 = j - 1, m = 1), one call per step
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), b)
    halves = Buffers(ops=hip_ops, n=n, b=b, cols=J + 2, Q1=start_block(n, b))
    for j in range(1, m + 1):
        W = rec.products(halves.Q, j)
        rec.orth(halves.Q, halves.T, halves.S, halves.flags, W, j, False)
        assert states_identical(halves.host(), states[j]), 'products + orth differ from the whole step at j = %d' % j
    many = Buffers(ops=hip_ops, n=n, b=b, cols=J + 2, Q1=start_block(n, b))
    rec.steps(many.Q, many.T, many.S, many.flags, 0, m, False)
    assert states_identical(many.host(), states[m]), 'one call of %d steps differs from %d calls' % (m, m)


# ---------------------------------------------------------------------------------------------------- 4. last_closes
@pytest.mark.parametrize('cfg', STEP_CONFIGS, ids=_cfg_id)
def test_last_closes_needs_no_room_for_a_next_block(hip_ops, cfg):
    """Step J + 1 as the closing one, from the basis J steps left: on a contiguous n x N basis (ldq == N exactly) and on the wide
    buffer, where block J + 2, the flags and everything beyond column block J + 1 of T must stay as they were.  In the
    70 000 x 64 case the basis then spans the whole space (N = 64 = n): W_perp vanishes in exact arithmetic, so the coupling
    is held to |S|max <= (1e-12 |W|_F)^2 there instead of the relative figure (the reference's own W_perp is rounding noise)."""
    name, kind, b, J = cfg[:4]
    h = host_case(name, kind)
    n = h['shape'][1]
    last = trajectory(hip_ops, cfg)[J]
    j, N = J + 1, (J + 1) * b
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), b)
    ref = reference_step(h, last['Q'][:, :N], N, b)
    full = cfg == FULL_SPACE
    assert full == (N == n)
    if not full:
        assert ref['ratio'] < 1e3, ref['ratio']                  # (no next block is formed: cond(W_perp) does not enter)
        observe(cfg, 'closing_ratio', ref['ratio'])

    def check_coupling(S, tag):
        if full:
            observe(cfg, 'closing_S_full_space_over_tol', np.abs(S).max() / (1e-12 * ref['nW']) ** 2)
            assert np.abs(S).max() <= (1e-12 * ref['nW']) ** 2
        else:
            serr = np.abs(S - ref['S']).max() / np.abs(ref['S']).max()
            observe(cfg, 'closing_S_rel_over_tol', serr / (1e-12 * max(1.0, ref['ratio'])))
            assert serr <= 1e-12 * max(1.0, ref['ratio']), (tag, serr)

    wide = Buffers.from_host(hip_ops, n, b, J + 2, last)
    rec.steps(wide.Q, wide.T, wide.S, wide.flags, j - 1, 1, True)
    got = wide.host()
    assert same_bits(got['Q'], last['Q']), 'a closing step wrote the basis'
    assert np.isnan(got['Q'][:, N:N + b]).all() and same_bits(got['flags'], last['flags'])
    check_block_column(cfg, h, got, ref, N, b, J + 2, tag='closing_')
    check_coupling(got['S'], 'wide')

    exact = Buffers.from_host(hip_ops, n, b, J + 2, last)
    Qc = exact.Q[:, :N].contiguous()
    assert Qc.stride(0) == N
    rec.steps(Qc, exact.T, exact.S, exact.flags, j - 1, 1, True)
    got2 = exact.host()
    assert same_bits(hip_ops.to_host(Qc), last['Q'][:, :N]) and same_bits(got2['flags'], last['flags'])
    check_block_column(cfg, h, got2, ref, N, b, J + 2, tag='closing_')
    check_coupling(got2['S'], 'ldq == N')
    # the second half alone closes the same way
    half = Buffers.from_host(hip_ops, n, b, J + 2, last)
    W = rec.products(Qc, j)
    rec.orth(Qc, half.T, half.S, half.flags, W, j, True)
    assert states_identical({**half.host(), 'Q': got2['Q']}, got2)
    report(cfg)


# ------------------------------------------------------------------------------------------------ 5. rounded products
ROUNDED_CONFIGS = [c for c in STEP_CONFIGS if c[2] % 4 == 0]


def rounded_references(h, Qj):
    Q32 = Qj.astype(np.float32).astype(np.float64)
    Y = h['M'] @ Q32
    W32 = h['Mt'] @ Y.astype(np.float32).astype(np.float64)
    W = h['Mt'] @ (h['M'] @ Qj)
    first = h['absMt'] @ (h['absM'] @ np.abs(Qj))               # |A|^T (|A| |Q_j|): both roundings act on terms of this size
    second = h['absMt'] @ np.abs(Y)                             # |A|^T |A fl32(Q_j)|: the rounding of Y alone
    return W, W32, first, second


@pytest.mark.parametrize('cfg', ROUNDED_CONFIGS, ids=_cfg_id)
def test_rounded_products_are_the_products_of_the_fp32_images(hip_ops, cfg):
    """products(rounded=True) = A^T fl32(A fl32(Q_j)) with fp64 accumulation.  Each rounding is relative 2^-24 per entry, so
    |W_dev - W_exact| <= ((1 + 2^-24)^2 - 1) |A|^T |A| |Q_j| elementwise (stated as 2^-23 + 2^-46) plus the fp64 summation
    (1e-13 |W|max); against the host's own rounded product only the device's Y may round to the NEIGHBOURING fp32 (its fp64
    sums differ in the last bits): one fp32 ulp = 2^-23 |Y| per entry.  And the flag must have done something."""
    name, kind, b, J = cfg[:4]
    h = host_case(name, kind)
    n = h['shape'][1]
    last = trajectory(hip_ops, cfg)[J]
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), b)
    Qd = hip_ops.to_device(last['Q'])
    for j in sorted({1, J, J + 1}):
        N = j * b
        Wd = hip_ops.to_host(rec.products(Qd, j, rounded=True))
        W, W32, first, second = rounded_references(h, last['Q'][:, N - b:N])
        wmax = np.abs(W).max()
        slack1 = np.abs(Wd - W) - ((2.0 ** -23 + 2.0 ** -46) * first + 1e-13 * wmax)
        observe(cfg, 'rounded_vs_exact_over_bound', (np.abs(Wd - W) / ((2.0 ** -23 + 2.0 ** -46) * first + 1e-13 * wmax)).max())
        assert (slack1 <= 0).all(), (j, slack1.max())
        moved = np.abs(Wd - W).max() / wmax
        observe(cfg, 'rounded_moved_rel', moved, worst=min)
        assert moved > 1e-10, (j, moved)
        observe(cfg, 'rounded_vs_host_rounded_over_bound', (np.abs(Wd - W32) / (2.0 ** -23 * second + 1e-13 * wmax)).max())
        assert (np.abs(Wd - W32) <= 2.0 ** -23 * second + 1e-13 * wmax).all(), j
        assert not Wd[[3, n - 1]].any()
    report(cfg)


def test_rounded_products_of_an_odd_block_are_the_exact_products(hip_ops):
    """b = 7: the fp32 images need a multiple of four columns; the rounded call is the exact one, bit for bit."""
    cfg = STEP_CONFIGS[2]
    name, kind, b, J = cfg[:4]
    assert b == 7
    last = trajectory(hip_ops, cfg)[J]
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), b)
    Qd = hip_ops.to_device(last['Q'])
    for j in (1, J + 1):
        assert same_bits(hip_ops.to_host(rec.products(Qd, j, rounded=True)), hip_ops.to_host(rec.products(Qd, j, rounded=False)))


BAND_CONFIGS = [c for c in ROUNDED_CONFIGS if c != FULL_SPACE]


@pytest.mark.parametrize('cfg', BAND_CONFIGS, ids=_cfg_id)
def test_rounded_step_keeps_the_band_of_T_only(hip_ops, cfg):
    """steps(rounded=True) at j = J + 1 >= 3 after J exact steps: block column j of T is Q^T W of the ROUNDED product inside the
    band (rows from N - 2b) and exactly 0.0 above it, likewise the mirror image.  The column and its mirror are pre-filled with
    7.0, so a zero there was written by this step."""
    name, kind, b, J = cfg[:4]
    h = host_case(name, kind)
    n = h['shape'][1]
    last = trajectory(hip_ops, cfg)[J]
    j, N = J + 1, (J + 1) * b
    assert j >= 3
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), b)
    buf = Buffers.from_host(hip_ops, n, b, J + 2, last)
    buf.T[:N, N - b:N] = 7.0
    buf.T[N - b:N, :N] = 7.0
    Wd = hip_ops.to_host(rec.products(buf.Q, j, rounded=True))
    rec.steps(buf.Q, buf.T, buf.S, buf.flags, j - 1, 1, False, rounded=True)
    got = buf.host()
    W = (J + 2) * b
    T = got['Tbuf'][:W, :W]
    assert not T[:N - 2 * b, N - b:N].any() and not T[N - b:N, :N - 2 * b].any(), 'entries above the band'
    assert same_bits(T[N - b:N, N - 2 * b:N - b], T[N - 2 * b:N - b, N - b:N].T), 'band block and its mirror image'
    Cd = last['Q'][:, N - 2 * b:N].T @ Wd                                               # the band from the device's own rounded W
    tmax = np.abs(T[:N, :N]).max()
    err = np.abs(T[N - 2 * b:N, N - b:N] - Cd).max() / tmax
    observe(cfg, 'band_rel', err)
    assert err < 1e-12, err
    assert not (T[N - b:N, N - b:N] == 7.0).any(), 'the diagonal block is written'
    assert same_bits(T[:N - b, :N - b], last['Tbuf'][:N - b, :N - b])
    outside = T.copy()
    outside[:N, :N] = 0.0
    assert not outside.any() and np.isnan(got['Tbuf'][W:]).all() and np.isnan(got['Tbuf'][:, W:]).all()
    if N + b <= n:
        # the next block comes from the rounded W: orthonormal and spanning ITS residual (40 000 x 200 at b = 64 has no room
        # for a fourth block: 256 columns in a space of 200)
        Qf = got['Q'][:, :N + b]
        assert np.abs(Qf.T @ Qf - np.eye(N + b)).max() < 1e-12
        assert np.linalg.norm(Wd - Qf @ (Qf.T @ Wd)) <= 1e-12 * np.linalg.norm(Wd)
        assert got['flags'][0] == 0 and got['flags'][1] < 1e-4
    report(cfg)


@pytest.mark.parametrize('cfg', [STEP_CONFIGS[0], STEP_CONFIGS[5]], ids=_cfg_id)
def test_rounded_step_writes_the_full_column_while_it_is_the_band(hip_ops, cfg):
    """j <= 2 (N <= 2b): the whole block column and its mirror image, as in the exact step, from the rounded product."""
    name, kind, b, J = cfg[:4]
    h = host_case(name, kind)
    n = h['shape'][1]
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), b)
    buf = Buffers(hip_ops, n, b, 4, start_block(n, b))
    for j in (1, 2):
        N = j * b
        buf.T[:N, N - b:N] = 7.0
        buf.T[N - b:N, :N] = 7.0
        Wd = hip_ops.to_host(rec.products(buf.Q, j, rounded=True))
        rec.steps(buf.Q, buf.T, buf.S, buf.flags, j - 1, 1, False, rounded=True)
        got = buf.host()
        T = got['Tbuf'][:4 * b, :4 * b]
        Cd = got['Q'][:, :N].T @ Wd
        assert np.abs(T[:N, N - b:N] - Cd).max() < 1e-12 * np.abs(T[:N, :N]).max(), j
        assert same_bits(T[N - b:N, :N - b], T[:N - b, N - b:N].T), j
        if j == 2:
            assert np.abs(T[:b, b:2 * b]).max() > 1e-3 * np.abs(T[:N, :N]).max(), 'the off-diagonal block at j = 2 is kept'
        outside = T.copy()
        outside[:N, :N] = 0.0
        assert not outside.any()


# -------------------------------------------------------------------------------------------------- 6. breakdown
def test_breakdown_is_reported_not_swallowed(hip_ops):
    """A matrix of exact rank 5 under blocks of 8: the residual block loses rank in the first step; within two steps the flags
    say so (the solver's own rule, _raise_on_breakdown), every call returns PK_OK (ops raises otherwise), one more too."""
    rng = np.random.RandomState(3)
    M = sps.csr_matrix(rng.standard_normal((400, 5)) @ rng.standard_normal((5, 90)))
    A = hip_ops.csr(M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data, M.shape)
    b = 8
    rec = hip_ops.lanczos_recurrence(A, b)
    buf = Buffers(hip_ops, 90, b, 5, start_block(90, b))
    for j in (1, 2):
        rec.steps(buf.Q, buf.T, buf.S, buf.flags, j - 1, 1, False)
    fl = buf.host()['flags']
    assert fl[0] != 0 or not (fl[1] < 1e-4), fl
    rec.steps(buf.Q, buf.T, buf.S, buf.flags, 2, 1, False)
    fl2 = buf.host()['flags']
    assert fl2[0] >= fl[0] and (fl2[0] != 0 or not (fl2[1] < 1e-4)), (fl, fl2)          # flags only accumulate
    print('\nOBSERVED breakdown flags after 2 steps %s, after 3 %s' % (fl, fl2))


# ------------------------------------------------------------------------------------------------ 7. argument checks
def test_argument_checks_are_loud_and_launch_nothing(hip_ops):
    """(A pk_mat without its transposed image cannot be made from Python: pk_mat_wrap_device builds the image before it hands
    the handle out — that clause of the checks is not reachable here.)"""
    name, kind = 'general', 'f32'
    n = CASES[name][1]
    b = 16
    rec = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), b)

    def refused(buf, call):
        before = buf.host()
        with pytest.raises(_lib.PolaraHipError, match='bad arguments'):
            call()
        assert states_identical(buf.host(), before), 'a refused call wrote something'

    # ldq one short of (j0 + m + 1) b
    buf = Buffers(hip_ops, n, b, 4, start_block(n, b), ldq_spare=-1)
    assert buf.Q.stride(0) == 4 * b - 1
    refused(buf, lambda: rec.steps(buf.Q, buf.T, buf.S, buf.flags, 2, 1, False))
    refused(buf, lambda: rec.steps(buf.Q, buf.T, buf.S, buf.flags, 0, 3, False))
    refused(buf, lambda: rec.orth(buf.Q, buf.T, buf.S, buf.flags, hip_ops.zeros(n, b), 3, False))
    # ... and the same call closes fine where it needs no next block (NaN blocks: the arithmetic is not the point)
    rec.steps(buf.Q, buf.T, buf.S, buf.flags, 2, 1, True)
    # ldt short
    buf = Buffers(hip_ops, n, b, 4, start_block(n, b))
    Tshort = buf.Tbuf[:, :2 * b - 1].contiguous()
    with pytest.raises(_lib.PolaraHipError, match='bad arguments'):
        rec.steps(buf.Q, Tshort, buf.S, buf.flags, 1, 1, False)
    # j = 0 for the halves, j0 < 0 and m = 0 for the whole
    refused(buf, lambda: rec.products(buf.Q, 0))
    refused(buf, lambda: rec.orth(buf.Q, buf.T, buf.S, buf.flags, hip_ops.zeros(n, b), 0, False))
    refused(buf, lambda: rec.steps(buf.Q, buf.T, buf.S, buf.flags, -1, 1, False))
    refused(buf, lambda: rec.steps(buf.Q, buf.T, buf.S, buf.flags, 0, 0, False))
    # b = 0 (the raw entries: the buffers are real, only b is wrong)
    lib, st = hip_ops.lib, rec._stream()
    refused(buf, lambda: _lib.check(lib.pk_lanczos_steps(rec.ctx, st, rec.handle, 0, 0, 1, 0, _ptr(buf.Q), buf.Q.stride(0), _ptr(buf.T),
                                                         buf.T.stride(0), _ptr(buf.S), _ptr(buf.flags), 0), 'pk_lanczos_steps', lib, rec.ctx))
    Wz = hip_ops.zeros(n, b)
    refused(buf, lambda: _lib.check(lib.pk_lanczos_products(rec.ctx, st, rec.handle, 0, 1, _ptr(buf.Q), buf.Q.stride(0), _ptr(Wz), 0),
                                    'pk_lanczos_products', lib, rec.ctx))
    refused(buf, lambda: _lib.check(lib.pk_lanczos_orth(rec.ctx, st, n, 0, 1, 0, _ptr(buf.Q), buf.Q.stride(0), _ptr(buf.T), buf.T.stride(0),
                                                        _ptr(Wz), _ptr(buf.S), _ptr(buf.flags), 0), 'pk_lanczos_orth', lib, rec.ctx))
    assert not Wz.any()
    refused(buf, lambda: _lib.check(lib.pk_gramian_apply_f64(rec.ctx, st, rec.handle, 0, _ptr(buf.Q), buf.Q.stride(0), _ptr(Wz), b),
                                    'pk_gramian_apply_f64', lib, rec.ctx))
    # (j0 + m) b > 4096 (pk_gram_f64's widest operand): buffers large enough that this is the ONLY clause that fails
    rec64 = hip_ops.lanczos_recurrence(device_case(hip_ops, name, kind), 64)
    big = Buffers(hip_ops, n, 64, 66, start_block(n, 64))
    assert big.Q.stride(0) >= 66 * 64 and big.T.stride(0) >= 65 * 64
    with pytest.raises(_lib.PolaraHipError, match='bad arguments'):
        rec64.steps(big.Q, big.T, big.S, big.flags, 64, 1, False)
    with pytest.raises(_lib.PolaraHipError, match='bad arguments'):
        rec64.orth(big.Q, big.T, big.S, big.flags, hip_ops.zeros(n, 64), 65, True)
    assert float(big.T.abs().sum()) == 0.0 and bool(torch.isnan(big.S).all()) and bool(torch.isnan(big.Q[:, 64:]).all())
    rec64.steps(big.Q, big.T, big.S, big.flags, 0, 1, False)   # the handle is none the worse for it
    assert bool(torch.isfinite(big.S).all())


# ------------------------------------------------------------------------------------------------ 8. pk_tsmm_axpby_f64
def _strided(ops, a, odd):
    """`a` on the device: contiguous, or (odd) with an odd leading dimension > width inside a NaN buffer whose base is one
    double past the allocation's (8-byte aligned only: the kernel's scalar load path)"""
    a = np.atleast_2d(a)
    r, c = a.shape
    if not odd:
        return ops.to_device(a)
    ld = c + 1 + (c % 2)                                            # odd, > c
    flat = torch.full((1 + r * ld,), NAN, dtype=torch.float64, device=ops.device)
    view = flat[1:].view(r, ld)[:, :c]
    view.copy_(ops.to_device(a))
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 == 8
    return view


def _axpby(ops, X, Cm, alpha, beta, Z1, gamma, Z2, out):
    n, lin = X.shape
    lout = Cm.shape[1]
    return ops.lib.pk_tsmm_axpby_f64(ops.stream(), n, lin, lout, _ptr(X), X.stride(0), _ptr(Cm), Cm.stride(0), alpha, beta,
                                     _ptr(Z1), Z1.stride(0) if Z1 is not None else 0, gamma, _ptr(Z2), Z2.stride(0) if Z2 is not None else 0,
                                     _ptr(out), out.stride(0))


@pytest.mark.parametrize('odd', [False, True], ids=['contiguous', 'odd_ld_offset_base'])
@pytest.mark.parametrize('shape', [(1, 1, 1), (63, 5, 3), (65, 33, 7), (777, 10, 72), (640, 64, 64), (5001, 130, 50), (300, 200, 130)])
def test_tsmm_axpby_against_numpy(hip_ops, shape, odd):
    """out = alpha X C + beta Z1 + gamma Z2 (tsmm_kernel<2>: the Chebyshev step of every nested solve) to 1e-13 of |out|max."""
    n, lin, lout = shape
    rng = np.random.RandomState(n + lin)
    X, Cm, Z1, Z2 = rng.randn(n, lin), rng.randn(lin, lout), rng.randn(n, lout), rng.randn(n, lout)
    alpha, beta, gamma = 0.7, -1.3, 0.45
    Xd, Cd, Z1d, Z2d = (_strided(hip_ops, a, odd) for a in (X, Cm, Z1, Z2))
    worst = 0.0
    for use1, use2 in ((True, True), (True, False), (False, True), (False, False)):
        if odd:
            out = _strided(hip_ops, np.full((n, lout + 3), NAN), True)
        else:
            out = torch.full((n, lout + 3), NAN, dtype=torch.float64, device=hip_ops.device)
        _lib.check(_axpby(hip_ops, Xd, Cd, alpha, beta, Z1d if use1 else None, gamma, Z2d if use2 else None, out[:, :lout]),
                   'pk_tsmm_axpby_f64')
        got = hip_ops.to_host(out)
        ref = alpha * (X @ Cm) + (beta * Z1 if use1 else 0.0) + (gamma * Z2 if use2 else 0.0)
        err = np.abs(got[:, :lout] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err < 1e-13, (use1, use2, err)
        assert np.isnan(got[:, lout:]).all(), 'columns beyond lout'
    # alpha = 0, beta = 1: out is Z1, exactly
    out = hip_ops.empty(n, lout)
    _lib.check(_axpby(hip_ops, Xd, Cd, 0.0, 1.0, Z1d, 0.0, None, out), 'pk_tsmm_axpby_f64')
    assert np.array_equal(hip_ops.to_host(out), Z1)
    # out aliasing any input is refused
    sq = hip_ops.to_device(rng.randn(lout, lout))
    full = hip_ops.to_device(rng.randn(n, lout))
    other = hip_ops.to_device(rng.randn(n, lout))
    keep = hip_ops.to_host(full).copy()
    for args in ((full, sq, 1.0, 0.0, None, 0.0, None, full),          # out is X
                 (other, sq, 1.0, 1.0, full, 0.0, None, full),         # out is Z1
                 (other, sq, 1.0, 0.0, None, 1.0, full, full),         # out is Z2
                 (sq, sq, 1.0, 0.0, None, 0.0, None, sq)):             # out is C (and X)
        assert _axpby(hip_ops, *args) != 0
    assert _axpby(hip_ops, full[:1], sq, 1.0, 0.0, None, 0.0, None, sq[:1]) != 0          # out is C alone
    assert np.array_equal(hip_ops.to_host(full), keep)
    print('\nOBSERVED tsmm_axpby %s odd=%s rel=%.3g' % (shape, odd, worst))


# ------------------------------------------------------------------------------------------------ 9. pk_orth_check_f64
@pytest.mark.parametrize('l', [1, 7, 16, 64, 130])
def test_orth_check_bookkeeping(hip_ops, l):
    """flags[1] = max(previous, max |G - I|), flags[0] += sum |info| (negative verdicts counted), info zeroed, a NaN or an inf
    anywhere in G counts as exactly 1.0, two calls accumulate; G with a leading dimension > l inside a NaN buffer.  (The
    kernel the library's Lanczos step itself runs after its three passes.)"""
    rng = np.random.RandomState(l)
    dev = hip_ops.device

    def run(G, info, flags):
        Gw = torch.full((l, l + 3), NAN, dtype=torch.float64, device=dev)
        Gw[:, :l] = hip_ops.to_device(G)
        info_d = torch.tensor(info, dtype=torch.int32, device=dev)
        flags_d = hip_ops.to_device(np.array(flags, dtype=np.float64))
        hip_ops.orth_check(Gw[:, :l], info_d, flags_d)
        return Gw, info_d, flags_d

    G = np.eye(l) + 1e-3 * rng.randn(l, l)
    worst = np.abs(G - np.eye(l)).max()
    for prev in (0.0, worst / 2, 0.5):
        Gw, info_d, flags_d = run(G, [3, -2, 0, 5], [2.0, prev])
        fl = hip_ops.to_host(flags_d)
        assert fl[0] == 12.0 and fl[1] == max(prev, worst), (prev, fl, worst)
        assert not hip_ops.to_host(info_d).any()
    # two calls accumulate (info is cleared by the first: the second adds its own verdicts only)
    G2 = np.eye(l) + 5e-3 * rng.randn(l, l)
    info_d.copy_(torch.tensor([0, -1, 0, 0], dtype=torch.int32))
    Gw[:, :l] = hip_ops.to_device(G2)
    hip_ops.orth_check(Gw[:, :l], info_d, flags_d)
    fl = hip_ops.to_host(flags_d)
    assert fl[0] == 13.0 and fl[1] == max(0.5, worst, np.abs(G2 - np.eye(l)).max()) and not hip_ops.to_host(info_d).any()
    # the last element alone off
    G3 = np.eye(l)
    G3[l - 1, l - 1] = 1.25
    _, _, flags_d = run(G3, [0], [0.0, 0.0])
    assert hip_ops.to_host(flags_d).tolist() == [0.0, 0.25]
    # non-finite entries count as exactly 1.0 — wherever they stand, whatever the running maximum
    for bad in (np.nan, np.inf, -np.inf):
        for pos in {(0, 0), (l - 1, l - 1), (l // 2, l - 1), (l - 1, 0)}:
            for prev in (0.0, 0.5, 3.0):
                Gb = G.copy()
                Gb[pos] = bad
                _, _, flags_d = run(Gb, [1, 0, -1], [0.0, prev])
                fl = hip_ops.to_host(flags_d)
                assert fl[0] == 2.0 and fl[1] == max(prev, 1.0), (bad, pos, prev, fl)


# ------------------------------------------------------------------------------------------- 10. pk_eigh_psd_rounds_f64
@pytest.mark.parametrize('n', [5, 64, 136, 137, 150, 200, 301])
def test_eigh_psd_rounds_called_directly(hip_ops, n):
    """The launch-per-round form of the block Jacobi solve (what ops.eigh_psd re-runs only when a grid barrier of the
    persistent kernel did not complete: never on a healthy machine) on the badly scaled Gram matrix of test_eigh_psd_jacobi,
    held to that test's assertions, and beyond 136 columns to the eigenvalues of pk_eigh_psd_f64."""
    rng = np.random.RandomState(n)
    M = rng.randn(n + 3, n) * np.logspace(0, -6, n)[None, :]   # badly scaled Gram matrix
    S = M.T @ M
    Sd = hip_ops.to_device(S)
    W, R, lam_d = Sd.clone(), hip_ops.empty(n, n), hip_ops.empty(n)
    info_d = torch.zeros(2, dtype=torch.int32, device=hip_ops.device)
    _lib.check(hip_ops.lib.pk_eigh_psd_rounds_f64(hip_ops.stream(), n, _ptr(W), n, _ptr(R), n, _ptr(lam_d), 0, 0.0, _ptr(info_d)),
               'pk_eigh_psd_rounds_f64')
    lam, Cv = hip_ops.to_host(lam_d), hip_ops.to_host(R).T          # rows of R are the eigenvectors
    ref = np.linalg.eigvalsh(S)[::-1]
    assert (np.diff(lam) <= 1e-300 + 1e-14 * lam[0]).all()
    assert np.abs(lam - ref).max() <= 1e-12 * ref[0]
    assert np.abs(Cv.T @ Cv - np.eye(n)).max() < 1e-12
    assert np.abs(S @ Cv - Cv * lam[None, :]).max() <= 1e-11 * ref[0]
    info = hip_ops.to_host(info_d)
    assert info[1] == 1, 'jacobi did not converge: %s' % info
    keep = ref > 1e-10 * ref[0]
    assert np.abs(lam[keep] / ref[keep] - 1).max() < 1e-6
    if n > 136:
        lam_p, _ = hip_ops.eigh_psd(Sd)
        assert np.abs(hip_ops.to_host(lam_p) - lam).max() <= 1e-12 * ref[0]
    print('\nOBSERVED eigh_rounds n=%d lam_err=%.3g orth=%.3g sweeps=%d' % (n, np.abs(lam - ref).max() / ref[0],
                                                                          np.abs(Cv.T @ Cv - np.eye(n)).max(), info[0]))

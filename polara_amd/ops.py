"""HipOps: the device operator set the solvers are written against.

Every method enqueues hand-written HIP kernels from libpolarahip.so (through the C ABI in
include/polara_hip.h) on torch's current HIP stream.  torch is plumbing only: it owns the device
allocations (tensors), the stream and — in polara_amd.dist — the RCCL communicator.
There is no CPU implementation in this package: constructing HipOps without the library or
without a GPU raises.  (tests/ carries a NumPy double of this interface to exercise the
distributed orchestration on CPU with gloo; it never ships.)
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .csr import SPLIT_NNZ


# row tasks per wave of the packed fold-in on a matrix marked `adjacent_alike` (csrc/foldq.hip: fold_q20_kernel's T)
FOLD_TASKS_PER_WAVE = 4
# ... as long as the launch keeps this many waves per SIMD: five rounds of the kernel's residency (90 VGPRs: 5 waves).  T tasks
# per wave are T times fewer waves that each run T times as long, and a launch of a few rounds ends on its longest waves:
# ML-20M-shaped rows at rank 50, ms for T = 1 / 2 / 4 — 8 K tasks 0.017 / 0.029 / 0.052, 28 K 0.040 / 0.049 / 0.084, 56 K 0.076 /
# 0.071 / 0.096, 140 K 0.176 / 0.160 / 0.155 (profiles/foldq_slices_ml20m.txt): T pays from ~27 waves per SIMD, not at ~14
FOLD_SLICED_MIN_WAVES = 25
_PTR_KEEP = None      # scoring.RecordedPass: the tensors whose addresses went into the recorded calls (kept alive with them)


def _ptr(t, offset=0):
    """device pointer of tensor `t`, advanced by `offset` ELEMENTS"""
    if t is None:
        return None
    if _PTR_KEEP is not None:
        _PTR_KEEP.append(t)
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def _raw_stream(index):
    """handle of torch's current stream on device `index` (the call the Python wrappers of torch.cuda.current_stream end in:
    0.3 us instead of 4 — a scoring pass asks a dozen times)"""
    return torch._C._cuda_getCurrentRawStream(index)


class _KernelTimer:
    """Context manager recording HIP events on the launch stream around one kernel call (HipOps._timed)."""
    __slots__ = ('ops', 'name', 'meta', 'e0', 'e1')

    def __init__(self, ops, name, meta):
        self.ops, self.name, self.meta = ops, name, meta

    def __enter__(self):
        if self.ops.timers is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.ops.device))

    def __exit__(self, *exc):
        if self.ops.timers is not None:
            self.e1.record(torch.cuda.current_stream(self.ops.device))
            self.ops.timers.setdefault(self.name, []).append((self.e0, self.e1, self.meta))
        return False


class DeviceCSR:
    """A CSR matrix resident in HBM together with its row-task plan (and, lazily, its transpose).  The plan
    (one wave per task, long rows split) is built on the device (pk_row_plan_*): only three counters visit the host."""

    def __init__(self, ops, indptr, indices, values, shape, split=SPLIT_NNZ):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        values = np.ascontiguousarray(values)
        if values.dtype == np.float64:
            v32 = values.astype(np.float32)
            if np.array_equal(v32.astype(np.float64), values):
                values = v32  # ratings are exactly representable: halve the value stream
        elif values.dtype != np.float32:
            values = values.astype(np.float64)
        dev = ops.device
        self._setup(ops, torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev),
                    torch.from_numpy(values).to(dev), shape, split, nnz=int(indptr[-1]))
        self._host = (indptr, indices, values)

    def _setup(self, ops, indptr, indices, values, shape, split, nnz=None):
        self.ops = ops
        self.shape = (int(shape[0]), int(shape[1]))
        self.indptr, self.indices, self.values = indptr, indices, values
        self.val_kind = _lib.PK_VAL_F32 if values.dtype == torch.float32 else _lib.PK_VAL_F64
        self._host = None
        self.split = split
        self._partial = None
        self._T = None
        self._seen_tiles = None
        self._seen_dense = None
        self.sorted_cols = True     # canonical CSR; False after a bare column renaming (csr_relabel_cols(sort=False))
        self._nnz = nnz
        self._plan = None

    @property
    def nnz(self):
        if self._nnz is None:
            self._nnz = int(self.indptr[-1].item()) - int(self.indptr[0].item())
        return self._nnz

    # ---- the wave-task plan (lazy: a matrix that is only re-indexed or transposed never needs one) ----------------
    def _ensure_plan(self):
        if self._plan is None:
            self._plan = self.ops.row_plan(self.indptr, self.shape[0], self.split)
        return self._plan

    @property
    def plan(self):
        return self._ensure_plan()['arrays']

    @property
    def n_tasks(self):
        return self._ensure_plan()['n_tasks']

    @property
    def n_long(self):
        return self._ensure_plan()['n_long']

    @property
    def n_slots(self):
        return self._ensure_plan()['n_slots']

    def task_range(self, lo, hi):
        """(first task, number of tasks, first long row, number of long rows) of rows [lo, hi): the tasks of a row range
        are a contiguous slice of the plan.  Cached per range (one small device read each)."""
        p = self._ensure_plan()
        key = (int(lo), int(hi))
        if key not in p['ranges']:
            sel = torch.tensor(key, device=self.indptr.device)
            t = p['row_first_task'][sel].tolist()
            l = p['row_long_index'][sel].tolist()
            p['ranges'][key] = (int(t[0]), int(t[1] - t[0]), int(l[0]), int(l[1] - l[0]))
        return p['ranges'][key]

    def partial(self, nc):
        """scratch for the partial sums of split long rows — one buffer per launch stream: two passes over the same
        matrix may be in flight on different streams (bench.py pipelines consecutive passes)"""
        need = self.n_slots * nc
        if need == 0:
            return None
        if not isinstance(self._partial, dict):
            self._partial = {}
        skey = self.ops.stream_key()
        buf = self._partial.get(skey)
        if buf is None or buf.numel() < need:
            buf = self._partial[skey] = torch.empty(need, dtype=torch.float64, device=self.ops.device)
        return buf

    def seen_tiles(self):
        """(tiles, ntiles): this matrix's rows as seen-tile streams for the candidate sweep — a format image of
        the CSR like the transpose, built once per matrix (pk_seen_tiles_build)."""
        if self._seen_tiles is None:
            self._seen_tiles = self.ops.seen_tiles(self.indptr, self.indices, self.shape[0],
                                                   rows_sorted=self.sorted_cols)
        return self._seen_tiles

    def seen_dense(self):
        """(dense masks, skip counts, dense_tiles) of this matrix's rows for the head of the catalogue, or None: the
        seen-tile stream unrolled into one 32-bit mask per (user, tile) for the first tiles — where the candidate sweep
        spends its time (groups leave it after 70-270 of 836 tiles on ML-20M-shaped) and where nearly every tile holds
        a record.  At most 256 tiles and 512 MB; `ops.seen_dense_tiles` overrides (0: off; tests).  Cached like the stream."""
        if getattr(self, '_seen_dense', None) is None:
            n_tiles = -(-self.shape[1] // 32)
            groups = -(-self.shape[0] // 32)
            env = getattr(self.ops, 'seen_dense_tiles', None)
            dt = min(n_tiles, 256) if env is None else min(n_tiles, int(env))
            while dt > 32 and groups * dt * 128 > (512 << 20):
                dt //= 2
            if env is None and n_tiles > 32 * dt:
                dt = 0        # a catalogue this long is swept far beyond the window (S-50M shard, rank 200: groups leave at
                              # tile 440 of 15 625 with a 128-tile window): the masks' loads then only cost (sweep +12 %)
            if dt <= 0 or self.shape[0] == 0:
                self._seen_dense = (None,)
            else:
                tiles, ntiles = self.seen_tiles()
                dense, skip = self.ops.seen_dense(self.indptr, tiles, ntiles, self.shape[0], dt)
                self._seen_dense = (dense, skip, dt)
        return None if self._seen_dense[0] is None else self._seen_dense

    @property
    def T(self):
        """CSR of A^T (= CSC of A), built on the device by pk_csr_transpose (a stable radix sort by column)."""
        if self._T is None:
            self._T = self.ops.csr_transpose(self)
            self._T._T = self
        return self._T

    def transpose_operator(self):
        """What the eigensolver multiplies by for Z = A^T Y: the user-blocked image when the matrix has enough rows for
        the blocking to matter, else the plain transpose."""
        return self.T_blocked() if self.shape[0] >= 2 * BlockedTranspose.MIN_ROWS_PER_BLOCK else self.T

    def by_activity(self):
        """(this matrix with its rows ordered by descending entry count, perm int64: row r of the result = row perm[r]
        of this one) — a format image like the transpose, built once (pk_csr_rows_by_length) and cached.  The image is marked
        `adjacent_alike`: adjacent row tasks are alike in length, which lets the packed fold-in share a wave among them."""
        if getattr(self, '_by_activity', None) is None:
            self._by_activity = self.ops.csr_rows_by_length(self)
        return self._by_activity

    def T_blocked(self, rows_per_block=None):
        """The transposed product cut into row (user) blocks: see BlockedTranspose."""
        if getattr(self, '_Tb', None) is None or (rows_per_block and self._Tb.rows_per_block != rows_per_block):
            self._Tb = BlockedTranspose(self.ops, self, rows_per_block)
        return self._Tb

    @classmethod
    def from_device(cls, ops, indptr, indices, values, shape, split=SPLIT_NNZ):
        """Wraps CSR arrays that already live in HBM."""
        self = cls.__new__(cls)
        self._setup(ops, indptr, indices, values, shape, split)
        return self

    def drop_host(self):
        self._host = None

    def nonneg(self):
        """True when no stored value is negative (checked once): the approximate fold-in's error weight
        sum_j a_uj ||V_j|| needs |a_uj| = a_uj."""
        if getattr(self, '_nonneg', None) is None:
            self._nonneg = bool((self.values >= 0).all().item()) if self.values.numel() else True
        return self._nonneg

    def with_columns(self, indices, values):
        """Same sparsity pattern per row (row pointers, task plan) with new column ids / values."""
        new = DeviceCSR.__new__(DeviceCSR)
        new.__dict__.update(self.__dict__)
        if values is not self.values:
            new._nonneg = None
        new.indices, new.values = indices, values
        new._host = None
        new._partial = None
        new._T = None
        new._Tb = None
        new._by_activity = None
        new._seen_tiles = None
        new._seen_dense = None
        new.__dict__.pop('_recurrences', None)
        return new


class BlockedTranspose:
    """Z = A^T Y with the rows of A (users) cut into blocks: the CSC of every block is one slice of a
    (block, item)-ordered image (pk_csr_transpose with rows_per_block > 0), block b ADDS its share to Z in launch
    order (deterministic).  The rows of Y one launch gathers span rows_per_block users instead of all of them, so
    they stay cache-resident (ML-20M-shaped, nc = 64: 1.14 -> 0.63 ms per product at 16K users per block;
    tools/probes/panel_probe.py).  Used by the eigensolver through HipOps.spmm (it has `.apply`)."""

    MIN_ROWS_PER_BLOCK = 16384

    def __init__(self, ops, A, rows_per_block=None):
        n_rows, n_cols = A.shape
        if not rows_per_block:
            # small enough that a block's rows of Y (nc = 64 fp64) fit the L2s, large enough that a (block, item)
            # task still holds ~64 entries on average (every task costs a descriptor and a wave)
            rows_per_block = max(self.MIN_ROWS_PER_BLOCK, int(64.0 * n_cols * n_rows / max(A.nnz, 1)))
            rows_per_block = -(-rows_per_block // 4096) * 4096
        self.rows_per_block = int(min(rows_per_block, max(n_rows, 1)))
        self.n_blocks = -(-n_rows // self.rows_per_block)
        self.ops = ops
        self.shape = (n_cols, n_rows)
        self.image = ops.csr_transpose(A, rows_per_block=self.rows_per_block)   # DeviceCSR with n_blocks * n_cols rows
        self.ranges = [self.image.task_range(b * n_cols, (b + 1) * n_cols) for b in range(self.n_blocks)]
        edges = self.image.indptr[torch.arange(0, self.n_blocks + 1, device=self.image.indptr.device) * n_cols].tolist()
        self.block_nnz = [int(b - a) for a, b in zip(edges[:-1], edges[1:])]

    def apply(self, Y, out=None):
        ops, M = self.ops, self.image
        n_cols = self.shape[0]
        if out is None:
            out = ops.empty(n_cols, Y.shape[1])
        if Y.shape[1] > 256:
            # one output row per wave in registers: at most 256 columns per launch (HipOps.spmm); wider blocks — builds
            # beyond rank 200, where solver.default_block exceeds 256 — go panel by panel through the leading dimensions
            for c0 in range(0, Y.shape[1], 256):
                self.apply(Y[:, c0:c0 + 256], out[:, c0:c0 + 256])
            return out
        for b, rng in enumerate(self.ranges):
            ops._spmm_launch(M, Y, out, rng, row_base=b * n_cols, accumulate=b > 0,
                             meta_shape=(n_cols if b == 0 else 0, self.rows_per_block, self.block_nnz[b]))
        return out


class _Elapsed:
    """a measured duration in the place of a HIP event pair (the library timed the launch itself)"""

    def __init__(self, ms):
        self.ms = ms

    def elapsed_time(self, other=None):
        return self.ms


class LanczosRecurrence:
    """The recurrence of the block Lanczos build inside the library (pk_lanczos_steps / pk_gramian_apply_f64) on a matrix
    that already lives in HBM: a non-owning handle over the CSR arrays (pk_mat_wrap_device: the library builds its own task
    plan and its user-blocked transpose, sized for `block_cols`-column blocks) in a context of its own (its pool of device
    blocks serves ONE stream: the stream of the first call).  solver._block_lanczos keeps the looks and every decision."""

    def __init__(self, ops, A, block_cols):
        self.ops, self.A, self.b = ops, A, int(block_cols)
        self.ctx = ops.recurrence_ctx()
        self.stream_ptr = torch.cuda.current_stream(ops.device).cuda_stream
        h = C.c_void_p()
        _lib.check(ops.lib.pk_mat_wrap_device(self.ctx, ops.stream(), A.shape[0], A.shape[1], A.nnz, _ptr(A.indptr), _ptr(A.indices),
                                              _ptr(A.values), A.val_kind, self.b, C.byref(h)), 'pk_mat_wrap_device', ops.lib, self.ctx)
        self.handle = h
        self._keep = (A.indptr, A.indices, A.values)        # the borrowed arrays outlive the handle

    def _stream(self):
        st = self.ops.stream()
        if (st.value or 0) != (self.stream_ptr or 0):
            # the context's pool hands blocks on in stream order: a call from another stream first lets the old one drain
            torch.cuda.synchronize(self.ops.device)
            self.stream_ptr = st.value or 0
        return st

    def _timing(self):
        # bench.py's per-launch SpMM records (ops.timers): the library takes them itself for the launches it makes
        want = 1 if self.ops.timers is not None else 0
        if want != getattr(self.ops, '_rec_timing_on', 0):      # (the state of the CONTEXT, which outlives this handle)
            _lib.check(self.ops.lib.pk_ctx_set_option(self.ctx, b'time_spmm', want), 'pk_ctx_set_option', self.ops.lib, self.ctx)
            if not want:      # records nobody will read
                self.ops.lib.pk_ctx_spmm_timings(self.ctx, None, None, 0)
            self.ops._rec_timing_on = want

    def collect_timings(self):
        """moves the library's SpMM records into ops.timers['spmm'] (as (duration, None, meta) with the meta of HipOps.spmm)"""
        if not getattr(self.ops, '_rec_timing_on', 0):
            return
        cap = 1 << 14
        ms = np.zeros(cap)
        meta = np.zeros((cap, 6), dtype=np.int64)
        n = int(self.ops.lib.pk_ctx_spmm_timings(self.ctx, ms.ctypes.data_as(C.c_void_p), meta.ctypes.data_as(C.c_void_p), cap))
        if self.ops.timers is not None:
            rows = self.ops.timers.setdefault('spmm', [])
            for i in range(min(n, cap)):
                rows.append((_Elapsed(float(ms[i])), None, tuple(int(v) for v in meta[i])))

    def steps(self, Q, T, S_out, flags, j0, m, last_closes, rounded=False):
        self._timing()
        assert Q.stride(1) == 1 and T.stride(1) == 1 and S_out.is_contiguous() and S_out.shape == (self.b, self.b)
        _lib.check(self.ops.lib.pk_lanczos_steps(self.ctx, self._stream(), self.handle, self.b, int(j0), int(m), 1 if last_closes else 0,
                                                 _ptr(Q), Q.stride(0), _ptr(T), T.stride(0), _ptr(S_out), _ptr(flags), 1 if rounded else 0),
                   'pk_lanczos_steps', self.ops.lib, self.ctx)

    def products(self, Q, j, rounded=False):
        """W [n_items x b] = A^T (A Q_j) of THIS process's rows (block j of the basis Q): the first half of a step of a
        user-sharded build — the caller sums W over the ranks and hands it to `orth`"""
        self._timing()
        assert Q.stride(1) == 1
        W = self.ops.empty(Q.shape[0], self.b)
        _lib.check(self.ops.lib.pk_lanczos_products(self.ctx, self._stream(), self.handle, self.b, int(j), _ptr(Q), Q.stride(0), _ptr(W),
                                                    1 if rounded else 0), 'pk_lanczos_products', self.ops.lib, self.ctx)
        return W

    def orth(self, Q, T, S_out, flags, W, j, last_closes, rounded=False):
        """the second half of step j from the summed W: block column j of T, the next block of Q, the coupling S"""
        assert Q.stride(1) == 1 and T.stride(1) == 1 and W.is_contiguous() and W.shape == (Q.shape[0], self.b)
        _lib.check(self.ops.lib.pk_lanczos_orth(self.ctx, self._stream(), Q.shape[0], self.b, int(j), 1 if last_closes else 0, _ptr(Q),
                                                Q.stride(0), _ptr(T), T.stride(0), _ptr(W), _ptr(S_out), _ptr(flags), 1 if rounded else 0),
                   'pk_lanczos_orth', self.ops.lib, self.ctx)

    def gramian(self, X):
        self._timing()
        X = X.contiguous()
        Z = self.ops.empty(X.shape[0], X.shape[1])
        _lib.check(self.ops.lib.pk_gramian_apply_f64(self.ctx, self._stream(), self.handle, X.shape[1], _ptr(X), X.stride(0), _ptr(Z),
                                                     Z.stride(0)), 'pk_gramian_apply_f64', self.ops.lib, self.ctx)
        return Z

    def __del__(self):
        # The handle is NOT freed here: a finaliser runs whenever the collector pleases — inside a hipGraph capture, say, where
        # the synchronisation a free implies would invalidate the capture (scoring.CapturedPass; found by the scaling proxy).
        # It is queued on the operator set, which frees queued handles at its next safe point (`lanczos_recurrence`).
        try:
            if getattr(self, 'handle', None):
                self.ops._pending_mat_free.append((self.ctx, self.handle, self._keep))
                self.handle = None
        except Exception:
            pass


class HipOps:
    name = 'hip'

    _queues_warned = False
    _warmed = {}         # device -> {'code', 'pipeline'}: what this process has been through on it (warm_up)
    _warm_lock = __import__('threading').Lock()

    def __init__(self, device=None, warm=None):
        self.lib = _lib.load()  # raises PolaraHipError if the .so is not built
        if not torch.cuda.is_available():
            raise _lib.PolaraHipError('no HIP device visible: polara_amd has no CPU fallback')
        self.device = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._gram_work = None
        self._score_state = None
        self._score_states = None
        import threading
        self.pass_lock = threading.RLock()   # scoring.recommend enqueues a pass as a whole (per-stream scratch state)
        self._aux_streams = []
        self._pending_mat_free = []          # (context, handle, borrowed arrays) of collected LanczosRecurrence objects
        self.score_tiles_per_chunk = 0       # 0 = auto (L2-sized item chunks); tests force tiny chunks
        self.score_splits_override = 0       # 0 = auto (pk_score_splits); tests force item splits
        self.seen_dense_tiles = None         # None = auto window of the dense seen masks (DeviceCSR.seen_dense); tests
        self._info = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._ctx = None     # a coarse-ABI context (its pool of device blocks) for the C++-driven nested eigen-solve
        # optional per-kernel HIP-event timing (bench.py): {'name': [(ev_start, ev_end, meta), ...]}
        self.timers = None
        self.warm_up_s = 0.0
        from . import runtime_info
        rt = runtime_info()
        if not rt['ok'] and not HipOps._queues_warned:
            import warnings
            HipOps._queues_warned = True
            warnings.warn('polara_amd: the HIP runtime of this process works with %s hardware queue(s) (%s); the solver\'s '
                          'monitor stream, the scoring pass streams and RCCL then share queues and serialise: builds under a '
                          'process group were measured 25 %% slower, pipelined scoring 20 %%.  Import polara_amd (or call '
                          'polara_amd.configure_runtime()) before the first use of the device, or export GPU_MAX_HW_QUEUES=8.'
                          % (rt['hw_queues'], rt['source']), RuntimeWarning, stacklevel=2)
        # warm: None / True / 'code' = load the library's code objects (pk_warm_up, a few ms); 'pipeline' = also run the
        # miniature build + passes (an explicit choice of long-lived serving processes: it costs ~0.2 s); False = nothing
        if warm is None or warm is True:
            warm = 'code'
        if warm not in (False, 'code', 'pipeline'):
            raise ValueError("warm must be False, 'code' or 'pipeline'")
        if warm:
            self.warm_up(pipeline=(warm == 'pipeline'))

    def warm_up(self, pipeline=False):
        """What a process pays ONCE.  Always: the library's code objects (pk_warm_up: one load per translation unit instead of
        one inside the first launch of each) — this is all `HipOps()` does by itself.  `pipeline=True` (an explicit call, or
        `HipOps(warm='pipeline')`): also a miniature build and three scoring passes (640 users x 256 items) through the code
        paths of the real ones, which takes the first-call costs that are not ours to load eagerly — the code objects of the
        torch kernels the host layer uses for plumbing, the side stream and the worker thread of the solver's monitors, the
        allocator's small pools.  Round 5 ran that pipeline inside every constructor: the first build looked warm, but a
        process that builds ONE model paid more in total (constructor 0.30 s + build 0.044 s against 0.11 + 0.14; VERDICT r5
        weak #5), so it is opt-in now, for processes that serve for hours.  A failure of the pipeline is an error like any
        other (it runs the product's own kernels).  The reference's `svds` call has no first-call cost (models.py:843-844;
        tools/timing.py:20-34 times the single call).  `self.warm_up_s` accumulates what the calls took."""
        key = (self.device.index if self.device.index is not None else torch.cuda.current_device())
        import time
        t0 = time.perf_counter()
        with HipOps._warm_lock:
            done = HipOps._warmed.setdefault(key, set())
            with torch.cuda.device(self.device):
                if 'code' not in done:
                    _lib.check(self.lib.pk_warm_up(), 'pk_warm_up')
                    done.add('code')
                if pipeline and 'pipeline' not in done:
                    self._warm_pipeline()
                    torch.cuda.synchronize(self.device)
                    done.add('pipeline')
        self.warm_up_s += time.perf_counter() - t0

    def _warm_pipeline(self):
        from . import scoring
        from .solver import svd_topk
        rng = np.random.default_rng(0)
        n_users, n_items, per, k = 640, 256, 12, 4
        # eight item clusters, a user draws from its own: a planted spectrum the solvers settle on in a few steps
        base = (np.arange(n_users) % 8)[:, None] * 32
        cols = np.sort(base + np.argsort(rng.random((n_users, 32)), axis=1)[:, :per], axis=1).astype(np.int32)
        indptr = np.arange(n_users + 1, dtype=np.int64) * per
        vals = rng.integers(1, 6, n_users * per).astype(np.float32)
        A = self.csr(indptr, cols.ravel(), vals, (n_users, n_items))
        _, _, _, rank_dev = self.item_order(A)
        A = self.csr_relabel_cols(A, rank_dev)
        A.transpose_operator()
        V = None
        for method in ('lanczos', 'subspace'):
            _, _, V, _ = svd_topk(self, A, k, tol=1e-8, max_outer=12, max_steps=8, method=method)
        F = scoring.FactorImage(self, V)
        Ta, perm = A.by_activity()
        self.scatter_rows(scoring.recommend(self, F, Ta, 5, True, order_users=False), perm)
        scoring.recommend(self, F, A, 5, True, return_scores=True)
        scoring.recommend(self, F, A, 5, False)

    def _timed(self, name, meta):
        """Context manager recording HIP events on the launch stream around one kernel call."""
        return _KernelTimer(self, name, meta)

    # ---- plumbing ---------------------------------------------------------------------------
    def stream(self):
        return C.c_void_p(_raw_stream(self._dev_index))

    def stream_key(self):
        """the current stream's handle as an int: key of the per-stream scratch buffers"""
        return _raw_stream(self._dev_index)

    def recurrence_ctx(self):
        """the coarse-ABI context (its own pool of device blocks) the library-side Lanczos recurrence runs in — not the one of
        the nested eigen-solves: a monitor holds that one's lock for the whole of its solve, on another thread"""
        if getattr(self, '_ctx_rec', None) is None:
            ctx = C.c_void_p()
            _lib.check(self.lib.pk_ctx_create(self.device.index or 0, C.byref(ctx)), 'pk_ctx_create')
            self._ctx_rec = ctx
        return self._ctx_rec

    def free_pending_handles(self):
        """releases the library handles of recurrence objects that have been collected (never inside a stream capture)"""
        if not self._pending_mat_free or torch.cuda.is_current_stream_capturing():
            return
        pending, self._pending_mat_free = self._pending_mat_free, []
        torch.cuda.synchronize(self.device)
        for ctx, handle, _keep in pending:
            self.lib.pk_mat_free(ctx, handle)

    def lanczos_recurrence(self, A, block_cols):
        """The recurrence object of the device matrix A for blocks of `block_cols` columns (cached on the matrix: the
        handle carries the library's transposed image of A)"""
        self.free_pending_handles()
        cache = A.__dict__.setdefault('_recurrences', {})
        rec = cache.get(int(block_cols))
        if rec is None:
            cache.clear()                            # one transposed image per matrix at a time
            rec = cache[int(block_cols)] = LanczosRecurrence(self, A, block_cols)
        return rec

    def monitor_stream(self):
        """the side stream of the solver's monitors: HIGH priority, so that the microsecond kernels of a nested solve are
        dispatched ahead of the queued workgroups of the sparse products they run next to"""
        if getattr(self, '_monitor_stream', None) is None:
            self._monitor_stream = torch.cuda.Stream(device=self.device, priority=-1)
        return self._monitor_stream

    def aux_streams(self, n):
        """n side streams (created once) for pipelining independent user batches"""
        while len(self._aux_streams) < n:
            self._aux_streams.append(torch.cuda.Stream(device=self.device))
        return self._aux_streams[:n]

    def empty(self, *shape, dtype=torch.float64):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def to_device(self, a, dtype=None):
        a = np.ascontiguousarray(a)
        import warnings
        with warnings.catch_warnings():
            # ArrayData stores read-only views of the caller's columns; torch warns that a tensor over one must not be
            # written to — it is only the source of the copy below
            warnings.simplefilter('ignore', UserWarning)
            t = torch.as_tensor(a)
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device)

    def to_host(self, t):
        return t.detach().cpu().numpy()

    def free_bytes(self):
        """free device memory in bytes (what the memory guards of the dense images compare their needs with)"""
        return int(torch.cuda.mem_get_info(self.device)[0])

    def csr(self, indptr, indices, values, shape, split=SPLIT_NNZ):
        return DeviceCSR(self, indptr, indices, values, shape, split)

    def _work(self, nbytes):
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)

    def row_plan(self, indptr, n_rows, split=SPLIT_NNZ):
        """The wave-task plan of a CSR, built on the device (csr.build_row_tasks restated as kernels)."""
        work = self._work(self.lib.pk_row_plan_work_bytes(n_rows))
        counts = torch.empty(3, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.pk_row_plan_count(self.stream(), n_rows, _ptr(indptr), int(split), _ptr(counts), _ptr(work)),
                   'pk_row_plan_count')
        n_tasks, n_long, n_slots = (int(v) for v in counts.tolist())
        i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        i64 = lambda n: torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        arr = dict(task_row=i32(n_tasks), task_begin=i64(n_tasks), task_end=i64(n_tasks), task_slot=i32(n_tasks),
                   long_row=i32(n_long), long_slot_begin=i32(n_long), long_slot_end=i32(n_long))
        rft, rli = i64(n_rows + 1), i64(n_rows + 1)
        _lib.check(self.lib.pk_row_plan_fill(self.stream(), n_rows, _ptr(indptr), _ptr(work), _ptr(arr['task_row']),
                                             _ptr(arr['task_begin']), _ptr(arr['task_end']), _ptr(arr['task_slot']),
                                             _ptr(arr['long_row']), _ptr(arr['long_slot_begin']), _ptr(arr['long_slot_end']),
                                             _ptr(rft), _ptr(rli)), 'pk_row_plan_fill')
        return dict(arrays=arr, n_tasks=n_tasks, n_long=n_long, n_slots=n_slots, row_first_task=rft, row_long_index=rli,
                    ranges={})

    def mode_plan(self, idx_dev, mode0, mode_u, mode_v, n0, split=256):
        """The entries of a 3-mode COO tensor ordered by mode `mode0` (stable), as pk_ttm_f64 wants them, built on the
        device: (plan dict, idx_u int32, idx_v int32, order int32).  idx_dev: int64 [nnz x 3] on the device.  Own stable
        radix sort of (mode0 index, position) pairs + pk_count_i32 + scan + the device row plan; the host version of the
        same (tucker.ModePlan: `argsort(kind='stable')` + gathers over 1e6 entries, three times per build) was two
        thirds of a CoFFee build's wall time."""
        nnz = int(idx_dev.shape[0])
        n1 = max(nnz, 1)
        keys = idx_dev[:, mode0].to(torch.int32).contiguous()
        pos = torch.arange(n1, dtype=torch.int32, device=self.device)
        keys_tmp, pos_tmp = torch.empty_like(keys), torch.empty_like(pos)
        bits = max(1, int(n0 - 1).bit_length()) if n0 > 1 else 1
        in_tmp = C.c_int32(0)
        if nnz:
            work = self._work(self.lib.pk_radix_work_bytes(nnz))
            _lib.check(self.lib.pk_radix_sort_pairs(self.stream(), nnz, 4, _ptr(keys), _ptr(pos), _ptr(keys_tmp), _ptr(pos_tmp),
                                                    bits, _ptr(work), C.byref(in_tmp)), 'pk_radix_sort_pairs')
        skeys, order = (keys_tmp, pos_tmp) if in_tmp.value else (keys, pos)
        counts = torch.zeros(max(n0, 1), dtype=torch.int32, device=self.device)
        indptr = torch.zeros(n0 + 1, dtype=torch.int64, device=self.device)
        if nnz:
            _lib.check(self.lib.pk_count_i32(self.stream(), nnz, _ptr(skeys), n0, _ptr(counts)), 'pk_count_i32')
            swork = self._work(self.lib.pk_scan_work_bytes(n0))
            _lib.check(self.lib.pk_exclusive_scan_i32(self.stream(), n0, _ptr(counts), _ptr(indptr), _ptr(swork)),
                       'pk_exclusive_scan_i32')
        rp = self.row_plan(indptr, n0, split=split)
        plan = dict(rp['arrays'], n_tasks=rp['n_tasks'], n_long=rp['n_long'], n_slots=rp['n_slots'])
        sel = order[:nnz].long()
        idx_u = idx_dev[:, mode_u].index_select(0, sel).to(torch.int32).contiguous()
        idx_v = idx_dev[:, mode_v].index_select(0, sel).to(torch.int32).contiguous()
        return plan, idx_u, idx_v, order[:nnz]

    def item_counts(self, A):
        """int64 [n_cols] (host): stored entries per column of a DeviceCSR (pk_count_i32) — the popularity of the items."""
        counts = torch.empty(A.shape[1], dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_count_i32(self.stream(), A.indices.numel(), _ptr(A.indices), A.shape[1], _ptr(counts)),
                   'pk_count_i32')
        return counts.cpu().numpy().astype(np.int64)

    def item_order(self, A, comm=None):
        """The internal item order of the device path (csr.popularity_order: descending entry count, ties by id) WITHOUT the
        host in the middle: per-column counts (pk_count_i32), summed over the ranks of `comm` when the rows are sharded, an
        own stable radix sort of (largest count - count, id) pairs, the inverse by one scatter; ONE copy brings back
        (rank int32[n_cols]: id -> position, inv int32[n_cols]: position -> id, counts int64[n_cols]) — plus the rank map
        as a device tensor for the renaming.  (numpy's stable argsort of 26 744 counts takes 1.5 ms, of 100 000: 7 ms — more
        than the renaming itself since the rows are sorted in LDS.)"""
        n = int(A.shape[1])
        counts = torch.empty(n, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_count_i32(self.stream(), A.indices.numel(), _ptr(A.indices), n, _ptr(counts)), 'pk_count_i32')
        sharded = comm is not None and getattr(comm, 'world', 1) > 1
        if sharded:
            counts = comm.allreduce(counts.to(torch.int64)).to(torch.int32)
        # the sort's key width must be the SAME on every rank and cover every key: on one rank the local entry count
        # bounds the counts; over shards of unequal size (ShardedArrayData) no local quantity does, and the keys are
        # int32 anyway — all 32 bits then (an n_items-sized sort: microseconds)
        total = int(A.indices.numel()) if not sharded else (1 << 32) - 1
        keys = (counts.max() - counts).contiguous()
        pos = torch.arange(n, dtype=torch.int32, device=self.device)
        keys_tmp, pos_tmp = torch.empty_like(keys), torch.empty_like(pos)
        in_tmp = C.c_int32(0)
        work = self._work(self.lib.pk_radix_work_bytes(n))
        bits = min(32, max(1, total.bit_length()))
        _lib.check(self.lib.pk_radix_sort_pairs(self.stream(), n, 4, _ptr(keys), _ptr(pos), _ptr(keys_tmp), _ptr(pos_tmp),
                                                bits, _ptr(work), C.byref(in_tmp)), 'pk_radix_sort_pairs')
        inv = pos_tmp if in_tmp.value else pos
        rank = torch.empty_like(inv)
        rank[inv.long()] = torch.arange(n, dtype=torch.int32, device=self.device)
        host = torch.cat([rank, inv, counts]).cpu().numpy()
        return host[:n].copy(), host[n:2 * n].copy(), host[2 * n:].astype(np.int64), rank

    def norm_order(self, V, gather=True):
        """The serving order of the catalogue (pk_row_norm_order_f64): (order int32 [n]: position -> row, rank int32 [n]:
        row -> position, V in that order or None) — rows of V by descending Euclidean norm, ties by id, own radix sort and
        one gather on the device (no library sort, no elementwise plumbing inside a build)."""
        assert V.dtype == torch.float64 and V.dim() == 2 and V.stride(1) == 1
        n, K = int(V.shape[0]), int(V.shape[1])
        order = torch.empty(n, dtype=torch.int32, device=self.device)
        rank = torch.empty(n, dtype=torch.int32, device=self.device)
        Vs = torch.empty((n, K), dtype=torch.float64, device=self.device) if gather else None
        work = self._work(self.lib.pk_row_norm_order_work_bytes(n))
        _lib.check(self.lib.pk_row_norm_order_f64(self.stream(), n, K, _ptr(V), V.stride(0), _ptr(order), _ptr(rank),
                                                  _ptr(Vs) if gather else None, _ptr(work)), 'pk_row_norm_order_f64')
        return order, rank, Vs

    def bincount(self, keys, n_bins):
        """int64 [n_bins] (device): occurrences of each key of a device int64 tensor (pk_count_i32 on the narrowed keys)."""
        k32 = keys.to(torch.int32).contiguous()
        counts = torch.empty(int(n_bins), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_count_i32(self.stream(), k32.numel(), _ptr(k32), int(n_bins), _ptr(counts)), 'pk_count_i32')
        return counts.to(torch.int64)

    # ---- splitting raw interactions (csrc/split.hip; polara_amd/prepare.py) ------------------------------------------
    def group_rows(self, codes, n_groups):
        """(perm int64 [n], seg_ptr int64 [n_groups + 1]) of a device int64 tensor of group codes in [0, n_groups): the row
        positions ordered by code, original order inside a group (own stable radix sort of (code, position) pairs), and
        where every group starts (pk_count_i32 + scan)."""
        n = int(codes.numel())
        assert n < 2 ** 31 and n_groups < 2 ** 31, 'group_rows: 32-bit codes and positions'
        seg_ptr = torch.zeros(int(n_groups) + 1, dtype=torch.int64, device=self.device)
        if n == 0 or n_groups == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.device), seg_ptr
        keys = codes.to(torch.int32).contiguous()
        pos = torch.arange(n, dtype=torch.int32, device=self.device)
        keys_tmp, pos_tmp = torch.empty_like(keys), torch.empty_like(pos)
        bits = max(1, int(n_groups - 1).bit_length())
        in_tmp = C.c_int32(0)
        work = self._work(self.lib.pk_radix_work_bytes(n))
        _lib.check(self.lib.pk_radix_sort_pairs(self.stream(), n, 4, _ptr(keys), _ptr(pos), _ptr(keys_tmp), _ptr(pos_tmp),
                                                bits, _ptr(work), C.byref(in_tmp)), 'pk_radix_sort_pairs')
        skeys, order = (keys_tmp, pos_tmp) if in_tmp.value else (keys, pos)
        counts = torch.empty(int(n_groups), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_count_i32(self.stream(), n, _ptr(skeys), int(n_groups), _ptr(counts)), 'pk_count_i32')
        swork = self._work(self.lib.pk_scan_work_bytes(n_groups))
        _lib.check(self.lib.pk_exclusive_scan_i32(self.stream(), int(n_groups), _ptr(counts), _ptr(seg_ptr), _ptr(swork)),
                   'pk_exclusive_scan_i32')
        return order.to(torch.int64), seg_ptr

    def split_keys(self, order_vals, pos, mode, seed):
        """(key_hi, key_lo): the two-word selection keys of pk_split_keys as int64 tensors holding the u64 bit patterns.
        order_vals: device fp64 [n] or None (mode must then carry PK_SPLIT_NO_ORDER); pos: device int64 [n]."""
        n = int(pos.numel())
        pos = pos.contiguous()
        if order_vals is not None:
            order_vals = order_vals.contiguous()
            assert order_vals.dtype == torch.float64 and order_vals.numel() == n
        assert pos.dtype == torch.int64
        key_hi = torch.empty(n, dtype=torch.int64, device=self.device)
        key_lo = torch.empty(n, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.pk_split_keys(self.stream(), n, _ptr(order_vals), _ptr(pos), int(mode), int(seed) & (2 ** 64 - 1),
                                          _ptr(key_hi), _ptr(key_lo)), 'pk_split_keys')
        return key_hi, key_lo

    def segment_select(self, seg_ptr, key_hi, key_lo, k):
        """uint8 [n] (device): 1 for the min(k, len) entries of every segment with the smallest (key_hi, key_lo) —
        pk_segment_select.  seg_ptr: device int64 [n_seg + 1], ascending within [0, n]."""
        n = int(key_hi.numel())
        n_seg = int(seg_ptr.numel()) - 1
        assert seg_ptr.dtype == torch.int64 and key_hi.dtype == torch.int64 and key_lo.dtype == torch.int64
        assert n_seg >= 0 and key_lo.numel() == n
        seg_ptr, key_hi, key_lo = seg_ptr.contiguous(), key_hi.contiguous(), key_lo.contiguous()
        flags = torch.empty(n, dtype=torch.uint8, device=self.device)
        work = self._work(self.lib.pk_segment_select_work_bytes(n_seg, n))
        _lib.check(self.lib.pk_segment_select(self.stream(), n_seg, n, _ptr(seg_ptr), _ptr(key_hi), _ptr(key_lo), int(k),
                                              _ptr(flags), _ptr(work)), 'pk_segment_select')
        return flags

    def csr_transpose(self, A, rows_per_block=0):
        """CSR of A^T on the device (pk_csr_transpose).  rows_per_block > 0: the (block, column)-ordered image — a
        DeviceCSR with n_blocks * n_cols rows whose row b * n_cols + c holds column c restricted to the rows of block b."""
        n_rows, n_cols = A.shape
        nnz = int(A.indices.numel())
        n_blocks = -(-n_rows // rows_per_block) if rows_per_block else 1
        t_indptr = torch.empty(n_blocks * n_cols + 1, dtype=torch.int64, device=self.device)
        t_indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=self.device)[:nnz]
        t_values = torch.empty(max(nnz, 1), dtype=A.values.dtype, device=self.device)[:nnz]
        work = self._work(self.lib.pk_csr_transpose_work_bytes(nnz))
        with self._timed('transpose', (n_rows, n_cols, nnz)):
            _lib.check(self.lib.pk_csr_transpose(self.stream(), n_rows, n_cols, nnz, _ptr(A.indptr), _ptr(A.indices),
                                                 _ptr(A.values), A.val_kind, int(rows_per_block), _ptr(t_indptr),
                                                 _ptr(t_indices), _ptr(t_values), _ptr(work)), 'pk_csr_transpose')
        T = DeviceCSR.from_device(self, t_indptr, t_indices, t_values, (n_blocks * n_cols, n_rows), A.split)
        T._nnz = nnz
        return T

    def csr_rows_by_length(self, A):
        n_rows = A.shape[0]
        nnz = int(A.indices.numel())
        perm = torch.empty(n_rows, dtype=torch.int32, device=self.device)
        indptr = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        idx = torch.empty_like(A.indices)
        val = torch.empty_like(A.values)
        work = self._work(self.lib.pk_csr_rows_by_length_work_bytes(n_rows))
        _lib.check(self.lib.pk_csr_rows_by_length(self.stream(), n_rows, nnz, _ptr(A.indptr), _ptr(A.indices), _ptr(A.values),
                                                  A.val_kind, _ptr(perm), _ptr(indptr), _ptr(idx), _ptr(val), _ptr(work)),
                   'pk_csr_rows_by_length')
        P = DeviceCSR.from_device(self, indptr, idx, val, A.shape, A.split)
        P._nnz = nnz
        P.sorted_cols = A.sorted_cols
        P._nonneg = getattr(A, '_nonneg', None)
        P.adjacent_alike = True        # rows in order of length: adjacent row tasks are alike (fold_q20's tasks_per_wave)
        return P, perm.long()

    def csr_relabel_cols(self, A, col_map, sort=True):
        """CSR with column j renamed to col_map[j].  `col_map`: int array or device tensor.  The row pointers —
        and with them the row-task plan — are those of A.  sort=True re-sorts every row on the device
        (pk_csr_relabel_sorted: canonical CSR); sort=False only renames (one gather): enough for SpMM, the transpose,
        the seen-tile builder and the exact-row kernel, none of which needs ordered rows (the result carries
        sorted_cols = False)."""
        dev = self.device
        if torch.is_tensor(col_map):
            cm = col_map.to(device=dev, dtype=torch.int32)
        else:
            cm = torch.as_tensor(np.ascontiguousarray(col_map, dtype=np.int32)).to(dev)
        if not sort:
            new = A.with_columns(cm[A.indices.long()], A.values)
            new.sorted_cols = False
            return new
        nnz = int(A.indices.numel())
        idx = torch.empty_like(A.indices)
        val = torch.empty_like(A.values)
        work = self._work(self.lib.pk_csr_relabel_work_bytes(nnz))
        _lib.check(self.lib.pk_csr_relabel_sorted(self.stream(), A.shape[0], A.shape[1], nnz, _ptr(A.indptr), _ptr(A.indices),
                                                  _ptr(A.values), A.val_kind, _ptr(cm.contiguous()), _ptr(idx), _ptr(val),
                                                  _ptr(work)), 'pk_csr_relabel_sorted')
        new = A.with_columns(idx, val)
        new.sorted_cols = True
        return new

    def csr_scale(self, A, row_scale, col_scale):
        """D_r A D_c with the diagonals given as host (or device) fp64 vectors: same pattern and plans, fp64 values
        (pk_csr_scale_f64) — ScaledMatrixMixin's rescaling of the training matrix on the device."""
        rs = torch.as_tensor(np.ascontiguousarray(row_scale, dtype=np.float64)).to(self.device) if not torch.is_tensor(row_scale) else row_scale
        cs = torch.as_tensor(np.ascontiguousarray(col_scale, dtype=np.float64)).to(self.device) if not torch.is_tensor(col_scale) else col_scale
        assert rs.numel() == A.shape[0] and cs.numel() == A.shape[1]
        out = torch.empty(max(int(A.indices.numel()), 1), dtype=torch.float64, device=self.device)[:A.indices.numel()]
        _lib.check(self.lib.pk_csr_scale_f64(self.stream(), A.shape[0], _ptr(A.indptr), _ptr(A.indices), _ptr(A.values), A.val_kind,
                                             _ptr(rs), _ptr(cs), _ptr(out)), 'pk_csr_scale_f64')
        new = A.with_columns(A.indices, out)
        new.val_kind = _lib.PK_VAL_F64
        return new

    def csr_from_coo(self, rows, cols, vals, shape, split=SPLIT_NNZ):
        """COO triplets (host arrays) -> canonical DeviceCSR built ON DEVICE (pk_coo_to_csr: one stable radix sort of
        the 64-bit keys row * n_cols + col, duplicates summed in their original order — what
        `coo_matrix(...).tocsr()` does in models.py:172-175).  `rows` / `cols` may be the two columns of one
        C-contiguous int64 [nnz x 2] array (the `idx` of `to_coo`, data.py:794-817): it is uploaded as it is."""
        n_rows, n_cols = int(shape[0]), int(shape[1])
        dev = self.device
        on_device = torch.is_tensor(rows)
        if on_device:
            # coordinates that already live on the device (the tensor unfoldings of tucker.hooi): int64 tensors
            assert torch.is_tensor(cols) and rows.dtype == cols.dtype == torch.int64 and rows.is_cuda and cols.is_cuda
            base = None
        else:
            rows, cols = np.asarray(rows), np.asarray(cols)
            base = rows.base if (rows.base is not None and rows.base is cols.base) else None
        nnz = int(rows.shape[0])
        if on_device:
            both = torch.empty(2, max(nnz, 1), dtype=torch.int64, device=dev)
            if nnz:
                both[0, :nnz].copy_(rows)
                both[1, :nnz].copy_(cols)
            r_ptr, c_ptr, stride = _ptr(both), _ptr(both, max(nnz, 1)), 1
        elif (base is not None and isinstance(base, np.ndarray) and base.dtype == np.int64 and base.ndim == 2 and
                base.shape == (nnz, 2) and base.flags.c_contiguous and rows.strides == (16,) and cols.strides == (16,)
                and rows.ctypes.data == base.ctypes.data and cols.ctypes.data == base.ctypes.data + 8):
            both = torch.from_numpy(base).to(dev)
            r_ptr, c_ptr, stride = _ptr(both), _ptr(both, 1), 2
        else:
            # two separate host arrays of any integer type: uploaded as they are (no host-side stacking or widening)
            both = torch.empty(2, max(nnz, 1), dtype=torch.int64, device=dev)
            if nnz:
                both[0, :nnz].copy_(self.to_device(rows))       # (to_device: read-only views of the caller's columns are fine)
                both[1, :nnz].copy_(self.to_device(cols))
            r_ptr, c_ptr, stride = _ptr(both), _ptr(both, max(nnz, 1)), 1
        if torch.is_tensor(vals):
            v = vals.to(dev).contiguous()
            if v.dtype not in (torch.float32, torch.float64):
                v = v.to(torch.float64)
        else:
            v = np.ascontiguousarray(vals)
            if v.dtype not in (np.float32, np.float64):
                v = v.astype(np.float64)
            v = torch.from_numpy(v).to(dev)
        if v.dtype == torch.float64 and nnz:
            v32 = v.to(torch.float32)
            if bool((v32.to(torch.float64) == v).all().item()):
                v = v32       # ratings are exactly representable: halve the value stream
        val_kind = _lib.PK_VAL_F32 if v.dtype == torch.float32 else _lib.PK_VAL_F64
        indptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        values = torch.empty(max(nnz, 1), dtype=v.dtype, device=dev)
        info = torch.zeros(4, dtype=torch.int64, device=dev)     # [0] = n_unique, [1] (as int32) = error flag
        work = self._work(self.lib.pk_coo_to_csr_work_bytes(nnz))
        with self._timed('coo_to_csr', (n_rows, n_cols, nnz)):
            _lib.check(self.lib.pk_coo_to_csr(self.stream(), nnz, r_ptr, c_ptr, stride, _ptr(v), val_kind, n_rows, n_cols,
                                              _ptr(indptr), _ptr(indices), _ptr(values), _ptr(info), _ptr(info, 1),
                                              _ptr(work)), 'pk_coo_to_csr')
        n_unique, err = (int(x) for x in info[:2].tolist())
        if err & 0xffffffff:
            raise ValueError('index out of bounds')
        new = DeviceCSR.from_device(self, indptr, indices[:n_unique], values[:n_unique], (n_rows, n_cols), split)
        new._nnz = n_unique
        return new

    def csr_rows(self, A, lo, hi):
        """Row block [lo, hi) of a DeviceCSR (device-side slice; used for user sharding)."""
        p0, p1 = int(A.indptr[lo]), int(A.indptr[hi])
        new = DeviceCSR.from_device(self, (A.indptr[lo:hi + 1] - p0).contiguous(), A.indices[p0:p1].contiguous(),
                                    A.values[p0:p1].contiguous(), (hi - lo, A.shape[1]), A.split)
        new.sorted_cols = A.sorted_cols
        new._nnz = p1 - p0
        return new

    def csr_gather_rows(self, A, rows):
        """The DeviceCSR whose row k is row rows[k] of A (host or device int64 ids; plumbing in torch, no kernel)."""
        rows = rows if torch.is_tensor(rows) else torch.as_tensor(np.ascontiguousarray(rows, dtype=np.int64))
        rows = rows.to(device=self.device, dtype=torch.int64)
        start = A.indptr[rows]
        length = A.indptr[rows + 1] - start
        indptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(length, 0, out=indptr[1:])
        nnz = int(indptr[-1].item())
        pos = torch.repeat_interleave(start - indptr[:-1], length) + torch.arange(nnz, dtype=torch.int64, device=self.device)
        new = DeviceCSR.from_device(self, indptr, A.indices[pos].contiguous(), A.values[pos].contiguous(),
                                    (int(rows.numel()), A.shape[1]), A.split)
        new.sorted_cols = A.sorted_cols
        new._nnz = nnz
        return new

    def randn(self, n, m, seed):
        # device-side Philox stream: identical on every rank for the same seed (the solver relies
        # on all ranks starting from the same block), and no 50 MB host round trip
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed))
        return torch.randn(n, m, generator=g, dtype=torch.float64, device=self.device)

    # ---- K1/K4 ------------------------------------------------------------------------------
    def spmm(self, A, X, out=None, rows=None):
        """out[n_rows x nc] = A @ X (fp64 accumulate, fp64 out).  A: DeviceCSR, X: [n_cols x nc] row-major, fp64
        or fp32 (the fp32 image of the item factors for the approximate fold-in).
        rows=(lo, hi): only rows [lo, hi) are computed (written to the same rows of the FULL-height `out`):
        the tasks of a row range are a contiguous slice of the plan, so a user batch is its own launch."""
        if hasattr(A, 'apply'):   # build(operator=...): a chain of device matrices or a host LinearOperator (operator.py)
            return A.apply(X, out)
        assert X.dtype in (torch.float64, torch.float32) and X.stride(-1) == 1 and X.shape[0] == A.shape[1]
        nc = X.shape[1]
        if out is None:
            out = self.empty(A.shape[0], nc)
        if nc > 256:
            # the kernels hold one output row per wave in registers: at most 256 columns per launch; wider blocks
            # (builds beyond rank ~200) go panel by panel through the leading dimensions
            for c0 in range(0, nc, 256):
                self.spmm(A, X[:, c0:c0 + 256], out=out[:, c0:c0 + 256], rows=rows)
            return out
        rng = (0, A.n_tasks, 0, A.n_long) if rows is None else A.task_range(int(rows[0]), int(rows[1]))
        return self._spmm_launch(A, X, out, rng)

    @staticmethod
    def _plan_side(A, rng):
        """the eight plan arguments of a row-task entry for the plan slice `rng` = (first task, tasks, first long row, long
        rows): the four task arrays from the first task on, the long-row count, the three long-row arrays from the first long row on"""
        p = A.plan
        t0, _, l0, n_long = rng
        return (_ptr(p['task_row'], t0), _ptr(p['task_begin'], t0), _ptr(p['task_end'], t0), _ptr(p['task_slot'], t0), n_long,
                _ptr(p['long_row'], l0), _ptr(p['long_slot_begin'], l0), _ptr(p['long_slot_end'], l0))

    def _spmm_launch(self, A, X, out, rng, row_base=0, accumulate=False, meta_shape=None):
        """one launch of the row-task kernel over the plan slice `rng` = (first task, tasks, first long row, long rows)"""
        nc = X.shape[1]
        x_kind = _lib.PK_VAL_F64 if X.dtype == torch.float64 else _lib.PK_VAL_F32
        meta = None
        if self.timers is not None:   # (output rows, source rows, nnz, nc, value bytes, dense element bytes) of this launch
            shp = meta_shape or (A.shape[0], A.shape[1], A.nnz)
            meta = (shp[0], shp[1], shp[2], nc, A.values.element_size(), X.element_size())
        with self._timed('spmm', meta):
            _lib.check(self.lib.pk_spmm_csr_ex(
                self.stream(), rng[1], *self._plan_side(A, rng), _ptr(A.indices), _ptr(A.values), A.val_kind,
                _ptr(X), x_kind, X.stride(0), nc, _ptr(out), out.stride(0), _ptr(A.partial(nc)), int(row_base),
                1 if accumulate else 0, int(X.shape[0])), 'pk_spmm_csr_ex')
        return out

    def spmm_flagged(self, A, X, out, row_flags, mask=7, rows=None):
        """out[r, :nc] = (A @ X)[r] for the rows with (row_flags[r] & mask) != 0, other rows untouched (fp64 X, even nc):
        the exact re-fold of uncertified users on the plan of the full product.  row_flags: int32 [n_rows] (all rows of A)."""
        assert X.dtype == torch.float64 and X.stride(1) == 1 and X.shape[0] == A.shape[1] and out.stride(1) == 1
        assert row_flags.dtype == torch.int32 and row_flags.is_contiguous() and row_flags.numel() == A.shape[0]
        nc = X.shape[1]
        rng = (0, A.n_tasks, 0, A.n_long) if rows is None else A.task_range(int(rows[0]), int(rows[1]))
        with self._timed('spmm_flagged', (A.shape[0], nc)):
            _lib.check(self.lib.pk_spmm_csr_flagged_f64(
                self.stream(), rng[1], *self._plan_side(A, rng), _ptr(A.indices), _ptr(A.values), A.val_kind, _ptr(X),
                X.stride(0), nc, _ptr(out), out.stride(0), _ptr(A.partial(nc)), int(X.shape[0]), _ptr(row_flags), int(mask)),
                'pk_spmm_csr_flagged_f64')
        return out

    def spmm_rows_list(self, A, X, out, lst, cnt, row_flags, mask=7, rows=None):
        """out[r, :nc] = (A @ X)[r] for the LISTED rows r = rows[0] + lst[i], i < cnt (device-side list and count; fp64 X, even
        nc): the exact re-fold of the users a pass could not certify, at the cost of their entries.  row_flags (int32, all
        rows of A, the listed ones flagged under `mask`) tells the fix-up pass which split rows were redone."""
        assert X.dtype == torch.float64 and X.stride(1) == 1 and X.shape[0] == A.shape[1] and out.stride(1) == 1
        assert lst.dtype == torch.int32 and cnt.dtype == torch.int32 and row_flags.dtype == torch.int32 and row_flags.numel() == A.shape[0]
        nc = X.shape[1]
        lo = 0 if rows is None else int(rows[0])
        # (the task arrays of the WHOLE plan — the kernel finds a listed row's tasks itself —, the long rows of the row range)
        _, _, l0, n_long = (0, A.n_tasks, 0, A.n_long) if rows is None else A.task_range(int(rows[0]), int(rows[1]))
        rft = A._ensure_plan()['row_first_task']
        with self._timed('spmm_rows_list', (int(lst.numel()), nc)):
            _lib.check(self.lib.pk_spmm_csr_rows_list_f64(
                self.stream(), int(lst.numel()), _ptr(lst), _ptr(cnt), lo, _ptr(rft), *self._plan_side(A, (0, A.n_tasks, l0, n_long)),
                _ptr(A.indices), _ptr(A.values), A.val_kind, _ptr(X), X.stride(0), nc, _ptr(out), out.stride(0),
                _ptr(A.partial(nc)), int(X.shape[0]), _ptr(row_flags), int(mask)), 'pk_spmm_csr_rows_list_f64')
        return out

    def spmm_flagged_ok(self, X):
        """can `spmm_flagged` take this dense block (even width and stride, 16-byte aligned)?"""
        return X.dtype == torch.float64 and X.shape[1] % 2 == 0 and X.stride(0) % 2 == 0 and X.data_ptr() % 16 == 0 and 2 <= X.shape[1] <= 256

    # ---- K4q: packed image of the item factors for the approximate fold-in (csrc/foldq.hip) -------------
    def q20_supported(self, n_items, K):
        """does a [n_items x K] factor matrix have a packed image (rank <= 202, below 2^24 rows and 4 GiB)?"""
        L = self.lib.pk_q20_lanes(int(K))
        return L != 0 and n_items < (1 << 24) and n_items * L * 16 < (1 << 32)

    def q20_encode(self, V):
        """(image uint8 [n x L*16], bracket scales fp64 [96]) of fp64 V, or None when the factors do not fit the
        format (non-finite / extreme magnitudes): the caller keeps the fp32 image."""
        assert V.stride(1) == 1 and V.dtype == torch.float64
        n, K = V.shape
        if not self.q20_supported(n, K):
            return None
        nbytes = self.lib.pk_q20_image_bytes(n, K)
        raw = torch.empty(nbytes + 128, dtype=torch.uint8, device=self.device)
        off = (-raw.data_ptr()) % 128
        img = raw[off:off + nbytes].view(n, nbytes // n)
        tab = torch.empty(96, dtype=torch.float64, device=self.device)
        work = torch.empty(768, dtype=torch.uint8, device=self.device)
        info = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_q20_encode_f64(self.stream(), n, K, _ptr(V), V.stride(0), _ptr(img), _ptr(tab), _ptr(work),
                                              _ptr(info)), 'pk_q20_encode_f64')
        if int(info.item()) != 0:
            return None
        return img, tab

    def q20_decode(self, image, K):
        """fp64 [n x (K + 1)]: the rows as the fold-in kernel decodes them, column K = the rows' error weights D_j"""
        img, tab = image
        n = img.shape[0]
        out = self.empty(n, K + 1)
        _lib.check(self.lib.pk_q20_decode_f64(self.stream(), n, K, _ptr(img), _ptr(tab), _ptr(out), out.stride(0)),
                   'pk_q20_decode_f64')
        return out

    def fold_q20(self, A, image, K, out, rows=None, counters=None, tasks_per_wave=None):
        """out[:, :K] = A @ decode(image), out[:, K] = w = A @ D (the certified weight of the image's error),
        zeros up to out's width.  A: DeviceCSR with non-negative values; rows as in `spmm`.
        counters (int32 device tensor): zeroed by the fold-in's fix-up launch (`fold_q20_zero`).
        tasks_per_wave: adjacent row tasks per wave (`pk_fold_q20_sliced`); by default `fold_tasks_per_wave`: more than 1 only
        for a matrix marked `adjacent_alike` (the image `by_activity` builds) and a launch long enough."""
        img, tab = image
        Kx = out.shape[1]
        assert out.dtype == torch.float64 and out.stride(1) == 1 and Kx >= K + 1 and img.shape[0] == A.shape[1]
        t0, n_tasks, l0, n_long = (0, A.n_tasks, 0, A.n_long) if rows is None else A.task_range(int(rows[0]), int(rows[1]))
        if tasks_per_wave is None:
            tasks_per_wave = self.fold_tasks_per_wave(A, n_tasks)
        p = A.plan
        meta = None
        if self.timers is not None:
            meta = (A.shape[0], A.shape[1], A.nnz, Kx, A.values.element_size(), img.shape[1])
        args = (self.stream(), n_tasks, _ptr(p['task_row'], t0), _ptr(p['task_begin'], t0), _ptr(p['task_end'], t0),
                _ptr(p['task_slot'], t0), n_long, _ptr(p['long_row'], l0), _ptr(p['long_slot_begin'], l0),
                _ptr(p['long_slot_end'], l0), _ptr(A.indices), _ptr(A.values), A.val_kind, _ptr(img), _ptr(tab),
                int(A.shape[1]), int(K), int(Kx), _ptr(out), out.stride(0), _ptr(A.partial(Kx)))
        if counters is not None:
            assert counters.dtype == torch.int32 and counters.is_contiguous() and counters.numel() >= 1
        with self._timed('fold_q20', meta):
            if tasks_per_wave != 1:
                zero = (None, 0) if counters is None else (_ptr(counters), int(counters.numel()))
                _lib.check(self.lib.pk_fold_q20_sliced(*args, *zero, int(tasks_per_wave)), 'pk_fold_q20_sliced')
            elif counters is None:
                _lib.check(self.lib.pk_fold_q20(*args), 'pk_fold_q20')
            else:
                _lib.check(self.lib.pk_fold_q20_zero(*args, _ptr(counters), int(counters.numel())), 'pk_fold_q20_zero')
        return out

    def fold_tasks_per_wave(self, A, n_tasks):
        """what `fold_q20` asks pk_fold_q20_sliced for: FOLD_TASKS_PER_WAVE on a matrix marked `adjacent_alike`, halved until
        the launch still has FOLD_SLICED_MIN_WAVES waves per SIMD (T tasks per wave are T times fewer waves: a launch that
        does not fill the device keeps one task per wave); 1 for every other matrix"""
        if not getattr(A, 'adjacent_alike', False):
            return 1
        if getattr(self, '_simds', None) is None:
            self._simds = 4 * torch.cuda.get_device_properties(self.device).multi_processor_count
        T = FOLD_TASKS_PER_WAVE
        while T > 1 and n_tasks < T * FOLD_SLICED_MIN_WAVES * self._simds:
            T //= 2
        return T

    def fold_q20_zero(self, A, image, K, out, n_counters, rows=None):
        """`fold_q20` + `zero_counters(n_counters)` in the launches of the fold-in alone: returns the int32 [n] counters, zero
        once the stream has passed the fold-in (its fix-up launch does it, behind the product and in front of whatever
        follows on the stream)."""
        c = torch.empty(int(n_counters), dtype=torch.int32, device=self.device)
        self.fold_q20(A, image, K, out, rows=rows, counters=c)
        return c

    # ---- K2 ---------------------------------------------------------------------------------
    def gram(self, A, B=None):
        """A^T B  (la x lb), fp64."""
        B = A if B is None else B
        assert A.stride(1) == 1 and B.stride(1) == 1 and A.shape[0] == B.shape[0]
        n, la = A.shape
        lb = B.shape[1]
        need = self.lib.pk_gram_work_bytes(n, la, lb)
        # the partial sums of the row splits: one scratch buffer PER STREAM (a monitor of the block Lanczos build runs its
        # small Gram products on a side stream while the main stream's are in flight)
        key = self.stream_key()
        if self._gram_work is None:
            self._gram_work = {}
        work = self._gram_work.get(key)
        if work is None or work.numel() * 8 < need:
            work = self._gram_work[key] = self.empty((need + 7) // 8)
        G = self.empty(la, lb)
        _lib.check(self.lib.pk_gram_f64(self.stream(), n, la, lb, _ptr(A), A.stride(0), _ptr(B), B.stride(0),
                                        _ptr(G), G.stride(0), _ptr(work)), 'pk_gram_f64')
        return G

    def tsmm(self, X, Cm, out=None):
        """X[n x lin] @ C[lin x lout]."""
        assert X.stride(1) == 1 and Cm.stride(1) == 1 and Cm.shape[0] == X.shape[1]
        n, lin = X.shape
        lout = Cm.shape[1]
        if out is None:
            out = self.empty(n, lout)
        _lib.check(self.lib.pk_tsmm_f64(self.stream(), n, lin, lout, _ptr(X), X.stride(0), _ptr(Cm), Cm.stride(0),
                                        _ptr(out), out.stride(0)), 'pk_tsmm_f64')
        return out

    def eigh_psd(self, S, max_sweeps=0, tol=0.0):
        """Symmetric PSD S (l x l) -> (evals desc [l], evecs [l x l] with COLUMN j = j-th eigenvector)."""
        n = S.shape[0]
        W = S.clone().contiguous()
        R = self.empty(n, n)
        lam = self.empty(n)
        info = self._info if n <= 136 else torch.zeros(2, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_eigh_psd_f64(self.stream(), n, _ptr(W), n, _ptr(R), n, _ptr(lam), max_sweeps, tol,
                                            _ptr(info)), 'pk_eigh_psd_f64')
        if n > 136:
            # block Jacobi: ONE cooperative launch whose workgroups meet at grid barriers.  Its verdict is read (a few
            # solves per build go this way, each followed by a host read of the eigenvalues anyway): 0 = a barrier did
            # not complete or the sweeps ran out — the vectors are then not eigenvectors and the solve is
            # re-done with one launch per round, where stream order is the barrier
            if int(info[1].item()) == 0:
                W.copy_(S)
                _lib.check(self.lib.pk_eigh_psd_rounds_f64(self.stream(), n, _ptr(W), n, _ptr(R), n, _ptr(lam), max_sweeps, tol,
                                                           _ptr(info)), 'pk_eigh_psd_rounds_f64')
                if int(info[1].item()) == 0:
                    raise RuntimeError('pk_eigh_psd_f64: the block Jacobi sweeps did not converge (n=%d)' % n)
        return lam, R.t()  # rows of R are eigenvectors -> return as columns (a view; strides swapped)

    def tsmm_sub(self, Z, X, Cm, out=None):
        """Z - X @ C in one pass (out may be Z itself)."""
        assert X.stride(1) == 1 and Cm.stride(1) == 1 and Z.stride(1) == 1 and Cm.shape[0] == X.shape[1] and Z.shape == (X.shape[0], Cm.shape[1])
        n, lin = X.shape
        lout = Cm.shape[1]
        if out is None:
            out = self.empty(n, lout)
        _lib.check(self.lib.pk_tsmm_sub_f64(self.stream(), n, lin, lout, _ptr(X), X.stride(0), _ptr(Cm), Cm.stride(0),
                                            _ptr(Z), Z.stride(0), _ptr(out), out.stride(0)), 'pk_tsmm_sub_f64')
        return out

    def sym_eig_topk(self, T, k, X0=None, tol=1e-13, max_outer=200, seed=0, stats=None, lam0=None, r0_rel=-1.0, width=None):
        """The k leading eigenpairs of the small dense symmetric PSD device matrix T [n x n] — pk_sym_eig_topk_f64: the
        filtered subspace iteration of solver.py with T as the operator, driven from C++ (hundreds of microsecond
        kernels: from Python each would cost the host ~20 us).  X0: orthonormal start block [rows <= n x l] (missing rows
        are zero) or None.  Returns (basis [n x l] device, Ritz values of its columns (host), residual norms of the active
        block (host), n_lock, converged) — the tuple of solver._subspace_iteration."""
        n = int(T.shape[0])
        assert T.stride(1) == 1 and T.shape[1] == n
        if X0 is not None:
            X0 = X0.contiguous()
            l = int(X0.shape[1])
            if lam0 is not None:      # the Ritz values of the start pairs (a warm look: pk_sym_eig_topk_f64 then skips its first Rayleigh-Ritz step)
                lam0 = np.ascontiguousarray(lam0, dtype=np.float64)
                lam0 = lam0 if len(lam0) == l else None
        else:
            l = min(n, max(int(k), 8, int(width or 0)))       # a cold solve of block width `width`: the library picks its own start
        if self._ctx is None:
            ctx = C.c_void_p()
            _lib.check(self.lib.pk_ctx_create(self.device.index or 0, C.byref(ctx)), 'pk_ctx_create')
            self._ctx = ctx
        basis = self.empty(n, l)
        lam = np.zeros(l)
        res = np.zeros(l)
        counts = np.zeros(5, dtype=np.int32)
        rc = self.lib.pk_sym_eig_topk_f64(self._ctx, self.stream(), n, _ptr(T), T.stride(0), int(k), l,
                                          _ptr(X0) if X0 is not None else None, l, int(X0.shape[0]) if X0 is not None else 0,
                                          float(tol), int(max_outer), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(basis), l,
                                          lam.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p),
                                          counts.ctypes.data_as(C.c_void_p),
                                          lam0.ctypes.data_as(C.c_void_p) if lam0 is not None else None, float(r0_rel))
        if rc != 0:
            raise RuntimeError('pk_sym_eig_topk_f64: ' + (self.lib.pk_ctx_error(self._ctx) or b'').decode())
        if stats is not None:
            stats['outer'] = stats.get('outer', 0) + int(counts[3])
            stats['steps'] = stats.get('steps', 0) + int(counts[4])
        n_lock, n_act = int(counts[0]), int(counts[1])
        return basis[:, :n_lock + n_act], lam[:n_lock + n_act], res[:n_act], n_lock, bool(counts[2])

    def eigh_top(self, S, r):
        """The r leading eigenpairs of symmetric PSD S: (evals desc [r], evecs [n x r]) — pk_eigh_top_f64 (one launch of a
        direct method that checks its own result) where it applies and passes, else the Jacobi kernel's leading columns.
        One small device -> host read per call (the kernel's verdict)."""
        n = int(S.shape[0])
        r = int(r)
        if self.lib.pk_eigh_top_supported(n, r):
            S = S.contiguous()
            R = self.empty(r, n)
            lam = self.empty(r)
            info = torch.zeros(1, dtype=torch.int32, device=self.device)
            work = self._work(self.lib.pk_eigh_top_work_bytes(n))
            _lib.check(self.lib.pk_eigh_top_f64(self.stream(), n, _ptr(S), n, r, _ptr(R), n, _ptr(lam), _ptr(work), _ptr(info)),
                       'pk_eigh_top_f64')
            if int(info.item()) == 1:
                return lam, R.t()
        lam, C = self.eigh_psd(S)
        return lam[:r], C[:, :r]

    def eigh_top_deferred(self, S, r):
        """`eigh_top` without the host read: (evals [r], evecs [n x r], verdict int32[1] on the device).  The results are
        only valid where the verdict is 1 — the caller reads it later (tucker.hooi: once per iteration) and re-does the
        work on the Jacobi route otherwise.  Shapes must satisfy pk_eigh_top_supported."""
        n, r = int(S.shape[0]), int(r)
        assert self.lib.pk_eigh_top_supported(n, r)
        S = S.contiguous()
        R = self.zeros(r, n)
        lam = self.zeros(r)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        work = self._work(self.lib.pk_eigh_top_work_bytes(n))
        _lib.check(self.lib.pk_eigh_top_f64(self.stream(), n, _ptr(S), n, r, _ptr(R), n, _ptr(lam), _ptr(work), _ptr(info)),
                   'pk_eigh_top_f64')
        return lam, R.t(), info

    def chol_rinv(self, G, shift_rel=0.0, info=None):
        """Rinv (l x l upper triangular) with G + shift_rel*trace(G)*I = R^T R; info: int32 device tensor[1]
        (0 = ok, j+1 = non-positive pivot at column j) — not read here, so no host sync."""
        n = G.shape[0]
        assert G.stride(1) == 1
        Rinv = self.empty(n, n)
        if info is None:
            info = torch.zeros(1, dtype=torch.int32, device=self.device)
        need = self.lib.pk_chol_work_bytes(n)
        work = self.empty((need + 7) // 8) if need else None
        _lib.check(self.lib.pk_chol_rinv_f64(self.stream(), n, _ptr(G), G.stride(0), float(shift_rel), _ptr(Rinv), n,
                                             _ptr(work), _ptr(info)), 'pk_chol_rinv_f64')
        return Rinv, info

    def orth_check(self, G, info, flags):
        """flags[0] += sum |info|, flags[1] = max(flags[1], max |G - I|) (NaN counts as 1), info zeroed — the bookkeeping
        of an orthonormalisation pass in one launch (a dozen one-element torch launches before)."""
        assert G.stride(1) == 1 and G.shape[0] == G.shape[1] and info.dtype == torch.int32 and flags.dtype == torch.float64
        _lib.check(self.lib.pk_orth_check_f64(self.stream(), G.shape[0], _ptr(G), G.stride(0), _ptr(info), info.numel(),
                                              _ptr(flags)), 'pk_orth_check_f64')

    def axpbypcz(self, alpha, Z, beta=0.0, Y=None, gamma=0.0, X=None, out=None):
        assert Z.is_contiguous() and (Y is None or Y.is_contiguous()) and (X is None or X.is_contiguous())
        if out is None:
            out = torch.empty_like(Z)
        _lib.check(self.lib.pk_axpbypcz_f64(self.stream(), Z.numel(), float(alpha), _ptr(Z), float(beta), _ptr(Y),
                                            float(gamma), _ptr(X), _ptr(out)), 'pk_axpbypcz_f64')
        return out

    def resid_colnorm2(self, Z, X, theta):
        """sum_i (Z[i,j] - theta[j] X[i,j])^2 per column -> [l] (device tensor)."""
        assert Z.stride(1) == 1 and X.stride(1) == 1 and theta.is_contiguous()
        n, l = Z.shape
        nb = self.lib.pk_resid_blocks(n)
        part = self.empty(nb, l)
        _lib.check(self.lib.pk_resid_colnorm2_f64(self.stream(), n, l, _ptr(Z), Z.stride(0), _ptr(X), X.stride(0),
                                                  _ptr(theta), _ptr(part)), 'pk_resid_colnorm2_f64')
        return part.sum(dim=0)

    def small_mm(self, A, B, transA=False, transB=False):
        A = A.contiguous()
        B = B.contiguous()
        M = A.shape[1] if transA else A.shape[0]
        K = A.shape[0] if transA else A.shape[1]
        N = B.shape[0] if transB else B.shape[1]
        out = self.empty(M, N)
        _lib.check(self.lib.pk_dgemm_small_f64(self.stream(), int(transA), int(transB), M, N, K, _ptr(A),
                                               A.stride(0), _ptr(B), B.stride(0), _ptr(out), out.stride(0)),
                   'pk_dgemm_small_f64')
        return out

    def scale_cols(self, X, s):
        assert X.stride(1) == 1
        _lib.check(self.lib.pk_scale_cols_f64(self.stream(), X.shape[0], X.shape[1], _ptr(X), X.stride(0),
                                              _ptr(s.contiguous())), 'pk_scale_cols_f64')
        return X

    # ---- K3 ---------------------------------------------------------------------------------
    def pack_frag(self, M):
        """f64 [n x K] -> packed f32 MFMA fragments (see csrc/score.hip)."""
        assert M.stride(1) == 1 and M.dtype == torch.float64
        n, K = M.shape
        out = torch.empty(self.lib.pk_pack_elems(n, K), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pk_pack_frag_f32(self.stream(), n, K, _ptr(M), M.stride(0), _ptr(out)),
                   'pk_pack_frag_f32')
        return out

    def candidate_capacity(self, topk):
        return self.lib.pk_candidate_capacity(topk)

    def score_splits(self, n_users, KC, prune=False):
        # item splits for user sets too small to fill the chip: tiles are dealt round-robin, so every split meets the
        # head of the catalogue first and the pruning bound works for each of them — but each split's threshold is
        # the k-th best of ITS items only, so S splits sweep further than one (measured: ML-20M-shaped, 16.9K users,
        # S = 2: 28 % of the tiles instead of 21 %, 1.06 vs 1.02 ms per pass; ML-1M-shaped, 6K users, S = 4: 0.254 vs
        # 0.30 ms).  A pruned sweep is therefore only dealt out when the groups fill less than 1/8 of the wave slots.
        if self.score_splits_override:
            return self.score_splits_override
        if prune and -(-n_users // 32) * 8 > 2048:
            return 1
        return self.lib.pk_score_splits(n_users, KC)

    def pack_frag_bound(self, M, extra=None, extra_scale=0.0):
        """(packed fp32 fragments of M, float32 row bounds ||M[r,:]|| (+ extra_scale * extra[r])) in one pass."""
        assert M.stride(1) == 1 and M.dtype == torch.float64
        n, K = M.shape
        out = torch.empty(self.lib.pk_pack_elems(n, K), dtype=torch.float32, device=self.device)
        bound = torch.empty(n, dtype=torch.float32, device=self.device)
        e_ld = 0 if extra is None else (extra.stride(0) if extra.numel() > 1 else 1)
        with self._timed('pack_frag_bound', (n, K)):
            _lib.check(self.lib.pk_pack_frag_bound_f32(self.stream(), n, K, _ptr(M), M.stride(0), _ptr(out), _ptr(bound),
                                                       _ptr(extra), e_ld, float(extra_scale)), 'pk_pack_frag_bound_f32')
        return out, bound

    def row_norm_bound(self, M):
        """float32 upper bounds of the row 2-norms of fp64 M (pruning bound of the candidate sweep)."""
        assert M.stride(1) == 1
        out = torch.empty(M.shape[0], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pk_row_norm_bound_f32(self.stream(), M.shape[0], M.shape[1], _ptr(M), M.stride(0),
                                                  _ptr(out)), 'pk_row_norm_bound_f32')
        return out

    def v32_image(self, V, bound, ld):
        """(fp32 image [n x ld] of fp64 V with `bound` in column K and zeros beyond, largest bound, all finite?) —
        pk_v32_image_f32: one launch and one 8-byte read instead of the fills, casts, index writes and the norm reduction of
        the host layer's first version (each a torch kernel whose code object a process loaded inside its first build)."""
        assert V.stride(1) == 1 and V.dtype == torch.float64 and bound.dtype == torch.float32
        n, K = int(V.shape[0]), int(V.shape[1])
        out = torch.empty((n, int(ld)), dtype=torch.float32, device=self.device)
        stat = torch.empty(2, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_v32_image_f32(self.stream(), n, K, int(ld), _ptr(V), V.stride(0), _ptr(bound), _ptr(out), _ptr(stat)),
                   'pk_v32_image_f32')
        h = stat.cpu().numpy().view(np.uint32)
        return out, float(np.array([h[0]], dtype=np.uint32).view(np.float32)[0]), not bool(h[1])

    def tile_norm_bound(self, V):
        """float32 [ceil(n/32)]: upper bound of max ||V[i,:]|| over all rows i >= 32*tile (suffix maximum)."""
        assert V.stride(1) == 1
        n = V.shape[0]
        work = torch.empty(n, dtype=torch.float32, device=self.device)
        out = torch.empty(-(-n // 32), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pk_tile_norm_bound_f32(self.stream(), n, V.shape[1], _ptr(V), V.stride(0), _ptr(work),
                                                   _ptr(out)), 'pk_tile_norm_bound_f32')
        return out

    def seen_tiles(self, seen_ptr, seen_idx, n_users, rows_sorted=True):
        """The seen-item lists folded into one (tile << 32 | item mask) record per touched 32-item tile:
        uint64 stream addressed by the same indptr + the record count per user.  rows_sorted=False: rows
        in arbitrary item order (sorted inside the kernel; very long rows fall back to a device sort)."""
        tiles = torch.empty(max(int(seen_idx.numel()), 1), dtype=torch.int64, device=self.device)
        ntiles = torch.empty(n_users, dtype=torch.int32, device=self.device)
        max_row = 0
        if not rows_sorted:
            max_row = int((seen_ptr[1:n_users + 1] - seen_ptr[:n_users]).max().item()) if n_users else 0
            if max_row > self.lib.pk_seen_tiles_max_unsorted_row():
                # rows too long for the in-LDS sort of the builder: re-sort them on the device (identity renaming)
                lo, hi = int(seen_ptr[0]), int(seen_ptr[n_users])
                n_cols = int(seen_idx[lo:hi].max().item()) + 1 if hi > lo else 1
                ident = torch.arange(n_cols, dtype=torch.int32, device=self.device)
                ptr0 = (seen_ptr[:n_users + 1] - lo).contiguous()
                idx = seen_idx[lo:hi].contiguous()
                out_i = torch.empty_like(idx)
                dummy = torch.zeros(hi - lo, dtype=torch.float32, device=self.device)
                work = self._work(self.lib.pk_csr_relabel_work_bytes(hi - lo))
                _lib.check(self.lib.pk_csr_relabel_sorted(self.stream(), n_users, n_cols, hi - lo, _ptr(ptr0), _ptr(idx),
                                                          _ptr(dummy), _lib.PK_VAL_F32, _ptr(ident), _ptr(out_i),
                                                          _ptr(torch.empty_like(dummy)), _ptr(work)), 'pk_csr_relabel_sorted')
                seen_idx = torch.cat([seen_idx[:lo], out_i])
                rows_sorted = True
        with self._timed('seen_tiles', (n_users, int(seen_idx.numel()))):
            _lib.check(self.lib.pk_seen_tiles_build(self.stream(), n_users, _ptr(seen_ptr), _ptr(seen_idx),
                                                    1 if rows_sorted else 0, max_row, _ptr(tiles), _ptr(ntiles)),
                       'pk_seen_tiles_build')
        return tiles, ntiles

    def seen_dense(self, seen_ptr, tiles, ntiles, n_users, dense_tiles):
        """(dense uint32 [groups x dense_tiles x 32], skip int32 [n_users]) from a seen-tile stream (pk_seen_dense_build)."""
        groups = -(-n_users // 32)
        dense = torch.empty((groups, dense_tiles, 32), dtype=torch.int32, device=self.device)
        skip = torch.empty(n_users, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_seen_dense_build(self.stream(), n_users, _ptr(seen_ptr), _ptr(tiles), _ptr(ntiles), int(dense_tiles),
                                                _ptr(dense), _ptr(skip)), 'pk_seen_dense_build')
        return dense, skip

    def sweep_settles(self, KC):
        """does a single pruned sweep with KC candidates settle its clear-cut users itself (`score_candidates(settle=)`)?  The
        library's answer: KC <= 32 and the options "sweep_settle" / "rescore_settle" on."""
        return bool(self.lib.pk_sweep_settles(int(KC)))

    def sweep_takes_rows(self, E):
        """can the candidate sweep read the users' side from these fp64 rows of E (16-byte aligned, even row stride)?  Then
        `score_candidates` / `score_two_phase` take `E_rows=(E, extra, extra_scale)` instead of packed fragments + bounds."""
        if not self.lib.pk_sweep_takes_rows():    # (a probe library carries round 4's sweep tree: packed fragments only)
            return False
        return (E.dtype == torch.float64 and E.dim() == 2 and E.stride(1) == 1 and E.stride(0) % 2 == 0 and E.data_ptr() % 16 == 0)

    @staticmethod
    def _users_side(Ep, user_bound, E_rows, bound_out, K, n_users):
        """the users' side of a sweep entry, eight arguments: packed (Ep, user_bound), or from rows (E, lde, extra, extra_ld,
        extra_scale, user_bound_out) — with `E_rows`, Ep and user_bound are not used"""
        if E_rows is None:
            return _ptr(Ep), _ptr(user_bound), None, 0, None, 0, 0.0, _ptr(bound_out)
        E, extra, scale = E_rows
        assert E.shape[1] >= K
        assert bound_out is None or (bound_out.dtype == torch.float32 and bound_out.is_contiguous() and bound_out.numel() == n_users)
        e_ld = 0 if extra is None else extra.stride(0)      # a column of E's own block: one entry per row, rows `stride` apart
        return (None, None, _ptr(E), E.stride(0), _ptr(extra), int(e_ld), float(scale if extra is not None else 0.0),
                _ptr(bound_out))

    def _sweep_state(self, n_users, slots):
        """the state buffer of a sweep with `slots` lists per user: one per launch stream, grown on demand"""
        need = self.lib.pk_score_state_bytes(n_users, slots)
        if self._score_states is None:
            self._score_states = {}
        skey = self.stream_key()
        if skey not in self._score_states or self._score_states[skey].numel() < need:
            self._score_states[skey] = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._score_state = self._score_states[skey]
        return self._score_state

    @staticmethod
    def _seen_side(seen_ptr, seen_tiles, seen_dense):
        """(seen_ptr, tiles, ntiles) and (dense, skip, dense_tiles) of a sweep entry as pointers; no seen lists: nothing is masked"""
        tiles = ntiles = dense = skip = None
        dtiles = 0
        if seen_ptr is not None:
            tiles, ntiles = seen_tiles
            if seen_dense is not None:
                dense, skip, dtiles = seen_dense
        return (_ptr(seen_ptr), _ptr(tiles), _ptr(ntiles)), (_ptr(dense), _ptr(skip), int(dtiles))

    def score_candidates(self, Vp, Ep, n_users, n_items, K, seen_ptr, seen_idx, KC, splits=1, tiles_per_chunk=0,
                         user_bound=None, tile_bound=None, seen_tiles=None, seen_dense=None, E_rows=None, bound_out=None,
                         settle=None):
        """The candidate sweep as one launch sequence (pk_score_candidates_f32).
        E_rows = (E fp64 [n_users x >= K], extra column or None, extra_scale): the users' fragments and pruning bounds are
        built inside the sweep (Ep and user_bound are not used, tile_bound alone switches the pruning on).  bound_out
        (float32 [n_users], E_rows only): the sweep stores the users' bounds there — what `rescore_topk` takes as `user_norm`.
        settle (E_rows with its extra column, tile_bound, splits == 1, `sweep_settles(KC)`): dict(topk, vmax, item_norm, out_idx,
        out_perm, flags, open_list, open_count) — the settle rule of the first re-scoring runs where a group leaves the sweep:
        settled users get their ids and flag 8 there and no candidate row, everybody else is appended to open_list behind the
        zeroed device counter open_count — the row list of the first re-scoring."""
        n_pad = -(-n_users // 32) * 32
        state = self._sweep_state(n_users, splits)
        cs = torch.empty(splits * n_pad * KC, dtype=torch.float32, device=self.device)
        ci = torch.empty(splits * n_pad * KC, dtype=torch.int32, device=self.device)
        if seen_ptr is not None and seen_tiles is None:
            seen_tiles = self.seen_tiles(seen_ptr, seen_idx, n_users)
        seen, dense = self._seen_side(seen_ptr, seen_tiles, seen_dense)
        blk = None
        if settle is not None:
            assert E_rows is not None and splits == 1 and tile_bound is not None and E_rows[1] is not None
            q = settle
            oi, fl, ol, oc = q['out_idx'], q['flags'], q['open_list'], q['open_count']
            assert oi.dtype == torch.int64 and oi.is_contiguous() and tuple(oi.shape) == (n_users, int(q['topk']))
            assert fl.dtype == torch.int32 and fl.is_contiguous() and fl.numel() == n_users
            assert ol.dtype == torch.int32 and ol.is_contiguous() and ol.numel() >= n_users
            assert oc.dtype == torch.int32 and oc.numel() == 1
            nrm, perm = q.get('item_norm'), q.get('out_perm')
            assert nrm is None or (nrm.dtype == torch.float32 and nrm.is_contiguous() and nrm.numel() == n_items)
            assert perm is None or (perm.dtype == torch.int64 and perm.is_contiguous() and perm.numel() == n_users)
            blk = C.byref(_lib.PkSweepSettle(int(q['topk']), float(q['vmax']), _ptr(nrm), _ptr(oi), _ptr(perm), _ptr(fl), _ptr(ol),
                                             _ptr(oc)))
        users = self._users_side(Ep, user_bound, E_rows, bound_out, K, n_users)
        with self._timed('score_candidates', (n_users, n_items, K)):
            _lib.check(self.lib.pk_score_candidates_f32(self.stream(), n_users, n_items, K, _ptr(Vp), *users, *seen, KC, splits,
                                                        _ptr(cs), _ptr(ci), _ptr(state),
                                                        tiles_per_chunk or self.score_tiles_per_chunk, _ptr(tile_bound), *dense, blk),
                       'pk_score_candidates_f32')
        return cs, ci

    def two_phase_plan(self, n_users, n_items, KC):
        """(head_tiles, splits) of the two-phase pruned sweep for this user set and catalogue, or (0, 0): single sweep."""
        h, s = C.c_int32(0), C.c_int32(0)
        _lib.check(self.lib.pk_score_two_phase_plan(int(n_users), int(n_items), int(KC), C.byref(h), C.byref(s)),
                   'pk_score_two_phase_plan')
        return int(h.value), int(s.value)

    def score_two_phase(self, Vp, Ep, n_users, n_items, K, seen_ptr, KC, head_tiles, splits, user_bound, tile_bound,
                        seen_tiles=None, seen_dense=None, tiles_per_chunk=0, E_rows=None, bound_out=None, work=None):
        """The pruned candidate sweep in two phases (pk_score_two_phase_f32): head sweep, `splits` sweeps of the tail from
        the head's thresholds, merge.  Returns the merged (scores, ids) [n_pad x KC] — a single list per user.
        E_rows, bound_out: as in `score_candidates`.  work = (float32, int32) [(splits + 1) * n_pad * KC]: the caller's arrays
        for the raw lists (slot 0: head, then the splits) instead of scratch of the call's own — whoever wants to read them."""
        n_pad = -(-n_users // 32) * 32
        total = splits + 1
        state = self._sweep_state(n_users, total)
        if work is not None:
            ws, wi = work
            assert ws.dtype == torch.float32 and wi.dtype == torch.int32 and ws.is_contiguous() and wi.is_contiguous()
            assert ws.numel() >= total * n_pad * KC and wi.numel() >= total * n_pad * KC
        else:
            ws = torch.empty(total * n_pad * KC, dtype=torch.float32, device=self.device)
            wi = torch.empty(total * n_pad * KC, dtype=torch.int32, device=self.device)
        cs = torch.empty(n_pad * KC, dtype=torch.float32, device=self.device)
        ci = torch.empty(n_pad * KC, dtype=torch.int32, device=self.device)
        seen, dense = self._seen_side(seen_ptr, seen_tiles, seen_dense)
        users = self._users_side(Ep, user_bound, E_rows, bound_out, K, n_users)
        with self._timed('score_candidates', (n_users, n_items, K)):
            _lib.check(self.lib.pk_score_two_phase_f32(self.stream(), n_users, n_items, K, _ptr(Vp), *users, *seen, KC,
                                                       int(head_tiles), int(splits), _ptr(ws), _ptr(wi), _ptr(cs), _ptr(ci),
                                                       _ptr(state), tiles_per_chunk or self.score_tiles_per_chunk,
                                                       _ptr(tile_bound), *dense),
                       'pk_score_two_phase_f32')
        return cs, ci

    def score_exit_tiles(self, n_users, splits=1):
        """int64 [splits x n_groups]: tile (absolute index) at which each group of 32 users left the last candidate
        sweep; split h of S owns tiles h, h+S, ... and scored ceil((exit - h) / S) of them."""
        groups = -(-n_users // 32)
        rec = self._score_state[:splits * groups * 64 * 16].view(torch.int64).view(splits, groups, 64, 2)
        return rec[:, :, 0, 0].clone()

    def rescore_topk(self, V, E, n_items, seen_ptr, KC, cs, ci, topk, vmax, want_scores=True, splits=1, out=None,
                     rows=None, n_rows_dev=None, e_err=None, e_exact=False, v32=None, flagged=None, item_norm=None,
                     out_perm=None, user_norm=None, first_pass=None):
        """Exact fp64 re-scoring + certification.  rows (int32 tensor): only these users are re-done (outputs
        are still indexed by user: pass the full-size `out`); e_err: per-user error weight of an approximate E
        (flags bit 4 = not certified at that accuracy); v32: fp32 image of V [n_items x >= K], gathered instead
        of V while E is approximate (its rounding joins the certified error); item_norm: float32 [n_items] upper bounds of
        the rows' norms (the order of two entries is then certified against their own norms).  flagged = (list int32, count int32[1],
        offset): every user that ends up flagged is appended to that device-side list as offset + user while the
        kernel runs (the counter is the caller's to zero: `zero_counters`).  out_perm (int64 [n_users]): the id list of user
        u goes to row out_perm[u] of out_idx (scores and flags stay at row u).  user_norm (float32 [n_users]): upper bounds
        of the norms of the rows of E — the users' side of the sweep's pruning bound; on a first pass over an approximate E
        (v32 and e_err given, no rows, not e_exact) the users whose order the sweep's own scores decide are then settled
        without re-scoring (pk_rescore_f64: flags = 8, no score row; `settled_users` counts them).
        first_pass (timers only): a call with a row list is booked as the pass's first re-scoring (the open list of a sweep
        that settled at its exit) instead of the re-scoring of the re-folded users."""
        assert V.stride(1) == 1 and E.stride(1) == 1
        assert v32 is None or (v32.dtype == torch.float32 and v32.stride(1) == 1 and v32.shape[1] >= E.shape[1])
        n_users, K = E.shape
        if out is not None:
            out_idx, out_s, flags = out      # caller-owned (contiguous row slices of the full outputs)
            assert out_idx.is_contiguous() and flags.is_contiguous() and (out_s is None or out_s.is_contiguous())
        else:
            out_idx = torch.empty(n_users, topk, dtype=torch.int64, device=self.device)
            out_s = self.empty(n_users, topk) if want_scores else None
            flags = torch.empty(n_users, dtype=torch.int32, device=self.device)
        n_rows = n_users if rows is None else int(rows.numel())
        e_ld = 0 if e_err is None else (e_err.stride(0) if e_err.numel() > 1 else 1)
        if first_pass is None:
            first_pass = rows is None
        with self._timed('rescore_topk' if first_pass else 'rescore_topk_refolded', (n_rows, KC, K)):
            fl, fc, fo = flagged if flagged is not None else (None, None, 0)
            assert item_norm is None or (item_norm.dtype == torch.float32 and item_norm.is_contiguous() and item_norm.numel() == n_items)
            assert out_perm is None or (out_perm.dtype == torch.int64 and out_perm.is_contiguous() and out_perm.numel() == n_users)
            if user_norm is not None:
                assert user_norm.dtype == torch.float32 and user_norm.is_contiguous() and user_norm.numel() == n_users
            _lib.check(self.lib.pk_rescore_f64(
                self.stream(), n_rows, _ptr(rows), _ptr(n_rows_dev), n_users, n_items, K, _ptr(V),
                V.stride(0), _ptr(v32), 0 if v32 is None else v32.stride(0), _ptr(E), E.stride(0), _ptr(e_err), e_ld,
                1 if e_exact else 0, _ptr(seen_ptr), KC, splits, _ptr(cs), _ptr(ci), topk, float(vmax),
                _ptr(out_idx), _ptr(out_s), _ptr(flags), _ptr(fl), _ptr(fc), int(fo), _ptr(item_norm), _ptr(out_perm),
                _ptr(user_norm)), 'pk_rescore_f64')
        return out_idx, out_s, flags

    @staticmethod
    def settled_users(flags):
        """users of a `rescore_topk(..., user_norm=)` call that its settle tier finished (flag bit 8): a host read"""
        return int((flags & 8).ne(0).sum().item())

    def zero_counters(self, n):
        """int32 [n] device counters, zeroed by a kernel on the current stream (one launch for all the lists of a pass)"""
        c = torch.empty(int(n), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_zero_i32(self.stream(), _ptr(c), int(n)), 'pk_zero_i32')
        return c

    def flag_compact(self, flags, mask=7):
        """(list int32[n], count int32[1]) of the users whose flags intersect `mask` — stays on the device."""
        n = flags.numel()
        lst = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        cnt = torch.empty(1, dtype=torch.int32, device=self.device)
        with self._timed('flag_compact', (n,)):
            _lib.check(self.lib.pk_flag_compact(self.stream(), n, _ptr(flags), int(mask), _ptr(lst), _ptr(cnt)),
                       'pk_flag_compact')
        return lst, cnt

    def fold_rows(self, A, lst, cnt, V, E, row_offset=0):
        """E[row_offset + lst[r], :K] = (A V)[that row] in fp64 for r < cnt (device-side list)."""
        assert V.stride(1) == 1 and E.stride(1) == 1 and V.dtype == torch.float64
        with self._timed('fold_rows', (int(lst.numel()),)):
            _lib.check(self.lib.pk_fold_rows_f64(self.stream(), lst.numel(), _ptr(lst), _ptr(cnt), int(row_offset),
                                                 _ptr(A.indptr), _ptr(A.indices), _ptr(A.values), A.val_kind, _ptr(V),
                                                 V.stride(0), V.shape[1], _ptr(E), E.stride(0)), 'pk_fold_rows_f64')

    def score_exact_rows(self, rows, V, E, n_items, seen_ptr, seen_idx, topk):
        n_rows = rows.numel()
        K = E.shape[1]
        out_idx = torch.empty(n_rows, topk, dtype=torch.int64, device=self.device)
        out_s = self.empty(n_rows, topk)
        work = torch.empty(self.lib.pk_exact_work_bytes(n_rows, n_items), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.pk_score_exact_rows_f64(self.stream(), n_rows, _ptr(rows), n_items, K, _ptr(V),
                                                    V.stride(0), _ptr(E), E.stride(0), _ptr(seen_ptr),
                                                    _ptr(seen_idx), topk, _ptr(out_idx), _ptr(out_s), _ptr(work)),
                   'pk_score_exact_rows_f64')
        return out_idx, out_s

    lists_in_caller_order = True     # `rescore_topk` and `score_exact_list` take `out_perm` (scoring.recommend)

    def score_exact_list(self, lst, cnt, V, E, n_items, seen_ptr, seen_idx, topk, out_idx, out_s, n_wg=128, out_perm=None):
        """score_exact_rows for the device-side list (lst[:cnt]) straight into rows of out_idx / out_s: no host sync, one launch.
        out_perm: as in `rescore_topk`."""
        K = E.shape[1]
        # one work buffer per launch stream (two passes on different streams must not share it) and layout (the tickets at
        # its end are zeroed once, here, and sit where (n_wg, n_items) puts them)
        key = (self.stream_key(), int(n_wg), int(n_items))
        if getattr(self, '_exact_work', None) is None:
            self._exact_work = {}
        work = self._exact_work.get(key)
        if work is None:
            work = torch.empty(self.lib.pk_exact_work_bytes(n_wg, n_items), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.pk_exact_work_init(self.stream(), _ptr(work), int(n_wg), n_items), 'pk_exact_work_init')
            self._exact_work[key] = work
        with self._timed('score_exact_list', (n_items, K, topk)):
            assert out_perm is None or (out_perm.dtype == torch.int64 and out_perm.is_contiguous())
            _lib.check(self.lib.pk_score_exact_list_f64(
                self.stream(), int(n_wg), _ptr(lst), _ptr(cnt), n_items, K, _ptr(V), V.stride(0), _ptr(E), E.stride(0),
                _ptr(seen_ptr), _ptr(seen_idx), topk, _ptr(out_idx), _ptr(out_s), _ptr(work), _ptr(out_perm)),
                'pk_score_exact_list_f64')
        return work

    def scatter_rows(self, src, perm, out=None):
        """out[perm[r], :] = src[r, :] for an int64 [n x width] result (perm None: a copy).  `out`: a device tensor, or a
        PINNED HOST tensor — mapped into the device's address space, the kernel then writes the host-side array of
        get_recommendations itself (no copy-engine transfer behind the pass)."""
        assert src.dtype == torch.int64 and src.is_contiguous() and (perm is None or perm.dtype == torch.int64)
        if out is None:
            out = torch.empty_like(src)
        assert out.dtype == torch.int64 and out.is_contiguous() and out.shape == src.shape
        assert out.is_cuda or out.is_pinned(), 'scatter_rows: a host destination must be pinned (mapped) memory'
        _lib.check(self.lib.pk_scatter_rows_i64(self.stream(), src.shape[0], src.shape[1], _ptr(src), _ptr(perm), _ptr(out)),
                   'pk_scatter_rows_i64')
        return out

    def ids_to_host(self, recs, table=None):
        """The [n x topk] int64 result as a host array: renamed through `table` (host int64 array: internal position ->
        caller's item id, -1 stays -1) on the device, then ONE transfer into pinned memory (the array returned is a view
        of a pinned block of torch's caching host allocator: it goes back to the cache with the array)."""
        assert recs.dtype == torch.int64 and recs.is_contiguous()
        src = recs
        if table is not None:
            key = (table.__array_interface__['data'][0], table.shape[0])
            if getattr(self, '_id_table', (None, None))[0] != key:     # one table at a time: the model's serving index
                self._id_table = (key, torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).to(self.device), table)
            tab = self._id_table[1]
            src = torch.empty_like(recs)
            _lib.check(self.lib.pk_map_ids_i64(self.stream(), recs.numel(), _ptr(recs), _ptr(tab), tab.numel(), _ptr(src)),
                       'pk_map_ids_i64')
        host = torch.empty(recs.shape, dtype=torch.int64, pin_memory=True)
        host.copy_(src, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return host.numpy()

    def eval_ranks(self, recs, hold_row, hold_item):
        """int32 [n_holdout]: 1-based rank of every holdout item in its user's row of the device-resident
        recommendation array (0 = not recommended)."""
        assert recs.dtype == torch.int64 and recs.is_contiguous()
        hr = hold_row.to(device=self.device, dtype=torch.int64).contiguous()
        hi = hold_item.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty(hr.numel(), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_eval_ranks(self.stream(), hr.numel(), _ptr(recs), recs.shape[1], _ptr(hr), _ptr(hi),
                                          _ptr(out)), 'pk_eval_ranks')
        return out

    def eval_metrics(self, recs, topk, hold_ptr, hold_item, hold_rel=None, hold_pos=None, not_rated_penalty=0.0,
                     switch_positive=0.0, alternative=True):
        """float64 [16] (host): sums over the test users of the per-user metric table of pk_eval_user_metrics — tp, fp,
        tn, fn, precision, recall, fallout, specifity, miss_rate, arhr, mrr, map, ndcg, ndcl, valid recs, holdout
        items — from the device-resident recommendation array `recs` [n_users x >= topk] and the holdout (CSR-like
        over the same rows; items in the id space of recs).  Only these 16 numbers leave the device."""
        assert recs.dtype == torch.int64 and recs.stride(1) == 1
        n_users = recs.shape[0]
        dev = self.device
        hp = hold_ptr.to(device=dev, dtype=torch.int64).contiguous()
        hi = hold_item.to(device=dev, dtype=torch.int64).contiguous()
        hr = None if hold_rel is None else hold_rel.to(device=dev, dtype=torch.float64).contiguous()
        hpos = None if hold_pos is None else hold_pos.to(device=dev, dtype=torch.uint8).contiguous()
        table = torch.empty(n_users, self.lib.pk_eval_cols(), dtype=torch.float64, device=dev)
        _lib.check(self.lib.pk_eval_user_metrics(self.stream(), n_users, int(topk), _ptr(recs), recs.stride(0), _ptr(hp),
                                                 _ptr(hi), _ptr(hr), _ptr(hpos), float(not_rated_penalty),
                                                 float(switch_positive), 1 if alternative else 0, _ptr(table)),
                   'pk_eval_user_metrics')
        sums = torch.empty(16, dtype=torch.float64, device=dev)
        work = self._work(self.lib.pk_eval_reduce_work_bytes(n_users))
        _lib.check(self.lib.pk_eval_reduce(self.stream(), n_users, _ptr(table), _ptr(sums), _ptr(work)), 'pk_eval_reduce')
        return sums.cpu().numpy()

    def unique_count(self, ids, n_bins):
        """number of distinct values in [0, n_bins) of an int64 device tensor (coverage, evaluation.py:239-242)"""
        ids = ids.contiguous()
        flags = torch.empty(n_bins + 1, dtype=torch.int32, device=self.device)
        cnt = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.pk_unique_count_i64(self.stream(), ids.numel(), _ptr(ids), int(n_bins), _ptr(flags), _ptr(cnt)),
                   'pk_unique_count_i64')
        return int(cnt.item())

    def topk_rows(self, scores, topk):
        """int64 [n_rows x topk]: columns of the largest scores per row of a dense fp64 device matrix, descending
        (pk_topk_rows_f64: score descending, column ascending)."""
        assert scores.dtype == torch.float64 and scores.stride(-1) == 1 and scores.dim() == 2
        out = torch.empty(scores.shape[0], int(topk), dtype=torch.int64, device=self.device)
        _lib.check(self.lib.pk_topk_rows_f64(self.stream(), scores.shape[0], scores.shape[1], _ptr(scores), scores.stride(0),
                                             int(topk), _ptr(out)), 'pk_topk_rows_f64')
        return out

    # ---- item-to-item / most popular (csrc/i2i.hip) ------------------------------------------------------------
    def _gram_image(self, name, A, rows, ld, diag=None):
        """The fp64 device image [rows x ld] of A^T A for the device CSR A [n_users x n_items]: pk_i2i_build_f64 writes
        rows [0, n_items) from A's CSR and its CSC image, diagonal and pad columns 0; with `diag` pk_ease_diag_f64 then
        sets the diagonal to the items' sums of squares + diag.  Rows beyond n_items are left as allocated.  `name`: the
        kernel-timer entry the launches are recorded under."""
        n_users, n_items = (int(x) for x in A.shape)
        T = A.T
        G = torch.empty(rows, ld, dtype=torch.float64, device=self.device)
        with self._timed(name, (n_users, n_items, A.nnz)):
            _lib.check(self.lib.pk_i2i_build_f64(self.stream(), n_users, n_items, _ptr(A.indptr), _ptr(A.indices),
                                                 _ptr(A.values), A.val_kind, _ptr(T.indptr), _ptr(T.indices),
                                                 _ptr(T.values), _ptr(G), ld), 'pk_i2i_build_f64')
            if diag is not None:
                _lib.check(self.lib.pk_ease_diag_f64(self.stream(), n_items, _ptr(T.indptr), _ptr(T.values), T.val_kind,
                                                     float(diag), _ptr(G), ld), 'pk_ease_diag_f64')
        return G

    def i2i_build(self, A):
        """C = A^T A with the diagonal set to 0 as a dense device image [n_items x i2i.leading_dim(n_items)]
        (`_gram_image`), then certified: fp32 when every entry survives the rounding (pk_i2i_image_f32), else fp64.
        Raises MemoryError before allocating when the fp64 image would take more than half of the free device memory.
        Returns (C, 'float32' | 'float64')."""
        from . import i2i
        n_items = int(A.shape[1])
        ld = i2i.leading_dim(n_items)
        i2i.check_build_memory(n_items, self.free_bytes())
        C64 = self._gram_image('i2i_build', A, n_items, ld)
        C32 = torch.empty(n_items, ld, dtype=torch.float32, device=self.device)
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.pk_i2i_image_f32(self.stream(), C64.numel(), _ptr(C64), _ptr(C32), _ptr(flag)),
                   'pk_i2i_image_f32')
        if int(flag.item()) == 0:
            return C32, 'float32'
        return C64, 'float64'

    def i2i_topk(self, T, C, n_items, topk, filter_seen, sparse, want_scores=False):
        """int64 [n_users x topk] (and fp64 scores or None): the top-k of s_u = T[u] C per row of the device CSR T
        (pk_i2i_topk: fused masking, -1 where a row has fewer candidates).  sparse: the sparse branch's candidates."""
        n_users = int(T.shape[0])
        topk = int(topk)
        out = torch.empty(n_users, topk, dtype=torch.int64, device=self.device)
        scores = torch.empty(n_users, topk, dtype=torch.float64, device=self.device) if want_scores else None
        c_kind = _lib.PK_VAL_F32 if C.dtype == torch.float32 else _lib.PK_VAL_F64
        work = self._work(self.lib.pk_i2i_topk_work_bytes(n_users, int(n_items), topk))
        with self._timed('i2i_topk', (n_users, int(n_items), T.nnz, topk)):
            _lib.check(self.lib.pk_i2i_topk(self.stream(), n_users, int(n_items), _ptr(T.indptr), _ptr(T.indices),
                                            _ptr(T.values), T.val_kind, _ptr(C), c_kind, C.stride(0), topk,
                                            1 if filter_seen else 0, 1 if sparse else 0, _ptr(out), _ptr(scores),
                                            _ptr(work)), 'pk_i2i_topk')
        return out, scores

    # ---- sparse x sparse product with the top-k fused in (csrc/simagg.hip) -----------------------------------------
    @staticmethod
    def _spsp_values(B):
        """B's values as fp64 (DeviceCSR keeps exactly representable values as fp32; the widening is exact), cached."""
        if B.values.dtype == torch.float64:
            return B.values
        if getattr(B, '_values_f64', None) is None or B._values_f64[0] is not B.values:
            B._values_f64 = (B.values, B.values.double())
        return B._values_f64[1]

    def spsp_topk(self, L, B, topk, filter_seen, sparse, want_scores=False):
        """int64 [n_rows x topk] (and fp64 scores or None): the top-k of scores[r] = L[r] B per row of the device CSR L
        against the canonical device CSR B (pk_spsp_topk: sums in SciPy's order, the masking and pads of i2i_topk)."""
        from . import simagg
        n_rows, n_inner, n_cols = simagg.check_shapes(L.shape, B.shape)
        topk = int(topk)
        out = torch.empty(n_rows, topk, dtype=torch.int64, device=self.device)
        scores = torch.empty(n_rows, topk, dtype=torch.float64, device=self.device) if want_scores else None
        work = self._work(self.lib.pk_spsp_topk_work_bytes(n_rows, n_cols, topk))
        with self._timed('spsp_topk', (n_rows, n_cols, L.nnz, topk)):
            _lib.check(self.lib.pk_spsp_topk(self.stream(), n_rows, n_inner, n_cols, _ptr(L.indptr), _ptr(L.indices),
                                             _ptr(L.values), L.val_kind, _ptr(B.indptr), _ptr(B.indices),
                                             _ptr(self._spsp_values(B)), topk, 1 if filter_seen else 0, 1 if sparse else 0,
                                             _ptr(out), _ptr(scores), _ptr(work)), 'pk_spsp_topk')
        return out, scores

    def spsp_rows(self, L, B, rows=None):
        """fp64 [n x n_cols] device block: the rows [lo, hi) = `rows` (default: all) of L B, bit-equal to SciPy's product
        (pk_spsp_rows_f64)."""
        from . import simagg
        n_rows, n_inner, n_cols = simagg.check_shapes(L.shape, B.shape)
        lo, hi = (0, n_rows) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= lo <= hi <= n_rows:
            raise ValueError('spsp_rows: rows [%d, %d) outside the %d rows of L' % (lo, hi, n_rows))
        out = torch.empty(hi - lo, n_cols, dtype=torch.float64, device=self.device)
        with self._timed('spsp_rows', (hi - lo, n_cols, L.nnz)):
            _lib.check(self.lib.pk_spsp_rows_f64(self.stream(), lo, hi - lo, n_inner, n_cols, _ptr(L.indptr), _ptr(L.indices),
                                                 _ptr(L.values), L.val_kind, _ptr(B.indptr), _ptr(B.indices),
                                                 _ptr(self._spsp_values(B)), _ptr(out), n_cols), 'pk_spsp_rows_f64')
        return out

    # ---- sparse x sparse product with CSR output and the similarity epilogues (csrc/spgemm.hip) -------------------
    SPGEMM_OPS = {'mul': 0, 'min': 1}
    SPGEMM_EPILOGUES = {'none': 0, 'jaccard': 1, 'wjaccard': 2}

    def spgemm_csr(self, L, B, op='mul', epilogue='none', diag=False, nf_rows=None, nf_cols=None, col_features=None,
                   rectangular=False):
        """The canonical DeviceCSR (fp64) of L B for the device CSR L (rows summed in their stored order) and the canonical
        device CSR B: pk_spgemm_count (the entries of every (row, window), their scan: indptr) and pk_spgemm_fill (the
        windows again, compacted).  An entry is stored when its sum is != 0; `diag` stores every (r, r) as 1.0.
        epilogue 'jaccard' needs the fp64 entry counts `nf_rows`, `nf_cols` (host or device); 'wjaccard' needs op='min',
        sorted rows in L and `col_features`, the DeviceCSR of the column side's features by item — `rectangular`: the pair
        is walked with the row as j, else with j = max(r, c) (see include/polara_hip.h).  `build_stats`-style timings
        go to the kernel timers as 'spgemm_count' and 'spgemm_fill'."""
        from . import simagg
        n_rows, n_inner, n_cols = simagg.check_shapes(L.shape, B.shape)
        if op not in self.SPGEMM_OPS or epilogue not in self.SPGEMM_EPILOGUES:
            raise ValueError('spgemm_csr: unknown op %r or epilogue %r' % (op, epilogue))

        def vec(x, n, what):
            if x is None:
                return None
            x = x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))
            x = x.to(device=self.device, dtype=torch.float64).contiguous()
            if x.numel() != n:
                raise ValueError('spgemm_csr: %s has %d entries, %d expected' % (what, x.numel(), n))
            return x
        nf_r, nf_c = vec(nf_rows, n_rows, 'nf_rows'), vec(nf_cols, n_cols, 'nf_cols')
        Fc = col_features
        if Fc is not None and Fc.shape[0] != n_cols:
            raise ValueError('spgemm_csr: col_features has %d rows, the product %d columns' % (Fc.shape[0], n_cols))
        f_values = self._spsp_values(Fc) if Fc is not None else None
        b_values = self._spsp_values(B)
        head = (self.stream(), n_rows, n_inner, n_cols, _ptr(L.indptr), _ptr(L.indices), _ptr(L.values), L.val_kind,
                _ptr(B.indptr), _ptr(B.indices), _ptr(b_values), self.SPGEMM_OPS[op], 1 if diag else 0)
        indptr = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        work = self._work(self.lib.pk_spgemm_work_bytes(n_rows, n_cols))
        with self._timed('spgemm_count', (n_rows, n_cols, L.nnz)):
            _lib.check(self.lib.pk_spgemm_count(*head, _ptr(indptr), _ptr(work)), 'pk_spgemm_count')
        nnz = int(indptr[-1].item())
        indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=self.device)[:nnz]
        values = torch.empty(max(nnz, 1), dtype=torch.float64, device=self.device)[:nnz]
        with self._timed('spgemm_fill', (n_rows, n_cols, nnz)):
            _lib.check(self.lib.pk_spgemm_fill(*head, self.SPGEMM_EPILOGUES[epilogue], 1 if rectangular else 0, _ptr(nf_r),
                                               _ptr(nf_c), _ptr(Fc.indptr) if Fc is not None else None,
                                               _ptr(Fc.indices) if Fc is not None else None, _ptr(f_values), _ptr(work), nnz,
                                               _ptr(indices), _ptr(values)), 'pk_spgemm_fill')
        out = DeviceCSR.from_device(self, indptr, indices, values, (n_rows, n_cols))
        out._nnz = nnz
        return out

    # ---- sampled-negatives evaluation (csrc/sampled.hip) ---------------------------------------------------------
    def candidates_topk(self, P, V, cand, topk, want_scores=False):
        """int64 [n_users x topk] column POSITIONS of the best candidates of every user (and the fp64 scores
        [n_users x C] or None): s[u, c] = P[u] . V[cand[u, c]] summed in the reference's order without contraction, the
        selection of topk_rows (pk_candidates_topk_f64).  P: fp64 device [n_users x r] with unit column stride; V: fp64
        device [n_items x r], row- or column-major; cand: int32 device [n_users x C] of item ids, validated here."""
        from . import sampled
        n_users, r, n_items, C = sampled.check_candidate_shapes(P.shape, V.shape, cand.shape, topk)
        assert P.dtype == V.dtype == torch.float64 and P.stride(1) == 1
        if V.stride(1) != 1 and V.stride(0) != 1:
            V = V.contiguous()
        cand = cand.to(self.device, torch.int32).contiguous()
        if n_users and C:
            lo, hi = (int(x) for x in torch.aminmax(cand))
            if lo < 0 or hi >= n_items:
                raise ValueError('candidate item ids span [%d, %d]: outside the %d items of the factors' % (lo, hi, n_items))
        topk = int(topk)
        out = torch.empty(n_users, topk, dtype=torch.int64, device=self.device)
        keep = want_scores or C > self.lib.pk_candidates_fused_max()
        scores = torch.empty(n_users, C, dtype=torch.float64, device=self.device) if keep else None
        with self._timed('candidates_topk', (n_users, n_items, r, C, topk)):
            _lib.check(self.lib.pk_candidates_topk_f64(self.stream(), n_users, n_items, r, _ptr(P), max(P.stride(0), r), _ptr(V), V.stride(0), V.stride(1), _ptr(cand), C, topk, _ptr(out),
                                                       _ptr(scores)), 'pk_candidates_topk_f64')
        return out, (scores if want_scores else None)

    # ---- contextual post-filtering (csrc/context.hip) --------------------------------------------------------------
    def context_lists(self, user_value, value_ptr, value_items, n_users, n_items):
        """The device image of ONE context for `context_merge`, from host arrays, range-checked here (the kernel does not):
        user_value [n_users] (-1: no value), value_ptr [n_values + 1], value_items: serving positions, ascending and
        distinct within a value."""
        from . import contextual
        uv, ptr, items, max_list = contextual.check_context_lists(user_value, value_ptr, value_items, n_users, n_items)
        return contextual.ContextLists(self.to_device(uv), self.to_device(ptr), self.to_device(items), max_list)

    def context_merge(self, V, E, seen, contexts, base_idx, want_class=False, order=None):
        """int64 [n_users x topk] (and the int32 classes or None): the lists `base_idx` of the plain pass with the context
        items of every user on top, ordered by (class descending, score descending, position ascending) — pk_context_merge_f64.
        V: fp64 device item rows in serving order; E: fp64 device query rows (unit column stride); seen: (indptr, indices) of
        the seen CSR or None (filter_seen off); contexts: 1..pk_context_max() images of `context_lists`, in mapping order;
        order: int32 device permutation of the rows (workgroup b serves row order[b]) or None."""
        n_users, topk = (int(x) for x in base_idx.shape)
        n_items, K = (int(x) for x in V.shape)
        n_ctx = len(contexts)
        if not 1 <= n_ctx <= self.lib.pk_context_max():
            raise ValueError('context_merge: %d contexts, 1..%d are supported' % (n_ctx, self.lib.pk_context_max()))
        if tuple(E.shape) != (n_users, K) or E.dtype != torch.float64 or V.dtype != torch.float64 or E.stride(1) != 1 or V.stride(1) != 1:
            raise ValueError('context_merge: fp64 rows E [%d x %d] and V [n_items x %d] with unit column stride expected' % (n_users, K, K))
        if base_idx.dtype != torch.int64 or not base_idx.is_contiguous():
            raise ValueError('context_merge: the base lists are a contiguous int64 [n_users x topk] block')
        for c in contexts:
            if c.user_value.numel() != n_users:
                raise ValueError('context_merge: context values for %d users, %d rows to merge' % (c.user_value.numel(), n_users))
        if order is not None and (order.dtype != torch.int32 or order.numel() != n_users):
            raise ValueError('context_merge: `order` is an int32 permutation of the %d rows' % n_users)
        out = torch.empty_like(base_idx)
        cls = torch.empty(n_users, topk, dtype=torch.int32, device=self.device) if want_class else None
        ptrs = [(C.c_void_p * n_ctx)(*[getattr(c, f).data_ptr() for c in contexts]) for f in ('user_value', 'value_ptr', 'value_items')]
        sp, si = seen if seen is not None else (None, None)
        with self._timed('context_merge', (n_users, n_items, K, topk, n_ctx)):
            _lib.check(self.lib.pk_context_merge_f64(self.stream(), n_users, n_items, K, _ptr(V), V.stride(0), _ptr(E), max(E.stride(0), K),
                                                     _ptr(sp), _ptr(si), n_ctx, ptrs[0], ptrs[1], ptrs[2],
                                                     max(c.max_list for c in contexts), _ptr(base_idx), topk, _ptr(out), _ptr(cls),
                                                     _ptr(order)), 'pk_context_merge_f64')
        return out, cls

    def sample_unseen(self, T, H, n, seeds):
        """int32 device [n_users x n]: n distinct items per user drawn uniformly from the items outside the user's row of
        the device CSR T (sorted columns) and of the device CSR H (None: no second exclusion), in draw order, from one
        uint32 seed per user (pk_sample_unseen; the stream is restated in tests/sampled_reference.py).  Raises ValueError
        before any launch when a user has fewer than n eligible items."""
        from . import sampled
        n_users, n_items = (int(x) for x in T.shape)
        n = int(n)
        if H is not None and tuple(int(x) for x in H.shape) != (n_users, n_items):
            raise ValueError('sample_unseen: exclusions of shape %s and %s' % (tuple(T.shape), tuple(H.shape)))
        if not getattr(T, 'sorted_cols', True):
            raise ValueError('sample_unseen: the rows of the first exclusion matrix must have sorted columns')
        seeds = np.ascontiguousarray(seeds)
        sampled.check_sample_request(n, n_items, len(seeds), n_users, self.lib.pk_sample_max_n())
        excluded = T.indptr[1:] - T.indptr[:-1]
        if H is not None:
            excluded = excluded + (H.indptr[1:] - H.indptr[:-1])
        min_eligible = n_items - (int(excluded.max()) if n_users else 0)        # a lower bound: an item of both rows counts twice
        limit = self.lib.pk_sample_round_limit(n_items, n, max(min_eligible, n))
        if n_users and (min_eligible < n or limit > self.lib.pk_sample_max_rounds()):
            # count the union exactly before giving up
            host = (self.to_host(T.indptr), self.to_host(T.indices), None if H is None else self.to_host(H.indptr),
                    None if H is None else self.to_host(H.indices))
            short = sampled.users_short_of_items(*host, n_items, n)
            if len(short):
                raise ValueError('sample_unseen: %d users have fewer than %d items outside their rows (the first: user %d)'
                                 % (len(short), n, int(short[0])))
            min_eligible = sampled.fewest_eligible_items(*host, n_items)
            limit = self.lib.pk_sample_round_limit(n_items, n, min_eligible)
            if limit > self.lib.pk_sample_max_rounds():
                raise ValueError('sample_unseen: a user has only %d items to draw %d from (of %d): up to %d rounds of 64 draws, '
                                 'more than the %d a launch may take' % (min_eligible, n, n_items, limit,
                                                                          self.lib.pk_sample_max_rounds()))
        out = torch.empty(n_users, n, dtype=torch.int32, device=self.device)
        err = torch.zeros(1, dtype=torch.int32, device=self.device)
        seeds_dev = torch.from_numpy(seeds.astype(np.uint32).view(np.int32)).to(self.device)
        with self._timed('sample_unseen', (n_users, n_items, T.nnz, n)):
            _lib.check(self.lib.pk_sample_unseen(self.stream(), n_users, n_items, _ptr(T.indptr), _ptr(T.indices),
                                                 _ptr(H.indptr) if H is not None else None,
                                                 _ptr(H.indices) if H is not None else None, n, min_eligible, _ptr(seeds_dev),
                                                 _ptr(out),
                                                 _ptr(err)), 'pk_sample_unseen')
        if int(err.item()):
            raise _lib.PolaraHipError('pk_sample_unseen: a user was not done within the round limit')
        return out

    def popular_order(self, scores):
        """int32 [n_items] device: the items by (score descending, item ascending) (pk_popular_order)."""
        scores = scores.to(self.device, torch.float64).contiguous()
        n = int(scores.numel())
        order = torch.empty(n, dtype=torch.int32, device=self.device)
        work = self._work(self.lib.pk_popular_order_work_bytes(n))
        _lib.check(self.lib.pk_popular_order(self.stream(), n, _ptr(scores), _ptr(order), _ptr(work)), 'pk_popular_order')
        return order

    def popular_topk(self, T, order, topk, filter_seen):
        """int64 [n_users x topk]: per row of the device CSR T the first topk items of `order`, unseen ones first under
        filter_seen (pk_popular_topk)."""
        n_users, n_items = (int(x) for x in T.shape)
        out = torch.empty(n_users, int(topk), dtype=torch.int64, device=self.device)
        with self._timed('popular_topk', (n_users, n_items, T.nnz, int(topk))):
            _lib.check(self.lib.pk_popular_topk(self.stream(), n_users, n_items, _ptr(T.indptr), _ptr(T.indices),
                                                _ptr(order), int(topk), 1 if filter_seen else 0, _ptr(out)),
                       'pk_popular_topk')
        return out

    # ---- HybridSVD: dense Cholesky factor of the item similarity (csrc/hybrid.hip) ------------------------------------
    def hybrid_densify(self, S, rank, beta):
        """The image [ld x ld] of K = S + beta I in the internal item order (pk_hybrid_densify_f64): S a SciPy sparse
        matrix in external ids, rank[external id] = internal position.  Raises MemoryError before allocating when the fp64
        image would take more than half of the free device memory."""
        from . import hybrid
        n = int(S.shape[0])
        hybrid.check_factor_memory(n, torch.cuda.mem_get_info(self.device)[0])
        S = S.tocsr()
        if not S.has_canonical_format:
            S = S.copy()
            S.sum_duplicates()
        ld = hybrid.leading_dim(n)
        K = torch.empty(ld, ld, dtype=torch.float64, device=self.device)
        # the index arrays go up as they lie (int32 from SciPy) and are widened on the device
        indptr = self.to_device(S.indptr).to(torch.int64)
        indices = self.to_device(S.indices).to(torch.int64)
        data = self.to_device(np.asarray(S.data, dtype=np.float64))
        rank_dev = self.to_device(np.asarray(rank, dtype=np.int64))
        with self._timed('hybrid_densify', (n, int(S.nnz))):
            _lib.check(self.lib.pk_hybrid_densify_f64(self.stream(), n, _ptr(indptr), _ptr(indices), _ptr(data), _ptr(rank_dev),
                                                      float(beta), _ptr(K), ld), 'pk_hybrid_densify_f64')
        return K

    def chol_image(self, K):
        """A padded image [ld x ld] holding the dense symmetric n x n matrix K (host or device; its lower triangle is what
        the factorisation reads), ready for `chol`."""
        from . import hybrid
        K = torch.as_tensor(np.ascontiguousarray(K) if isinstance(K, np.ndarray) else K)
        n = int(K.shape[0])
        ld = hybrid.leading_dim(n)
        img = torch.zeros(ld, ld, dtype=torch.float64, device=self.device)
        img[:n, :n] = K.to(device=self.device, dtype=torch.float64)
        return img

    def chol(self, A, n):
        """In-place lower Cholesky of the n x n matrix in the image A (pk_chol_f64); one host read of the verdict at the end.
        Raises numpy.linalg.LinAlgError naming the first column whose pivot is not positive (or not finite)."""
        info = torch.empty(1, dtype=torch.int32, device=self.device)
        with self._timed('chol', (int(n),)):
            _lib.check(self.lib.pk_chol_f64(self.stream(), int(n), _ptr(A), A.stride(0), _ptr(info)), 'pk_chol_f64')
        col = int(info.item())
        if col >= 0:
            err = np.linalg.LinAlgError('Cholesky factorisation: the matrix is not positive definite (the pivot of column '
                                        '%d is not positive)' % col)
            err.column = col
            raise err
        return A

    def trmm(self, L, n, X, trans=False, out=None):
        """Y = L X (trans False) or L^T X for X [n x nc] device, L the image of `chol` (pk_trmm_f64, in blocks of at most
        64 columns).  `out`: an [n x nc] destination (its rows may be strided)."""
        from . import hybrid
        n = int(n)
        if X.stride(-1) != 1:
            X = X.contiguous()
        nc = int(X.shape[1])
        Y = out if out is not None else torch.empty(n, nc, dtype=torch.float64, device=self.device)
        if Y.stride(-1) != 1:
            raise ValueError('trmm: the destination must have unit column stride')
        work = self._work(self.lib.pk_trmm_work_bytes(n, min(nc, hybrid.MAX_NC)))
        for c0, c1 in hybrid.column_blocks(nc):
            with self._timed('trmm', (n, c1 - c0, bool(trans))):
                _lib.check(self.lib.pk_trmm_f64(self.stream(), 1 if trans else 0, n, c1 - c0, _ptr(L), L.stride(0),
                                                _ptr(X, c0), X.stride(0), _ptr(Y, c0), Y.stride(0), _ptr(work)), 'pk_trmm_f64')
        return Y

    def trsm(self, L, n, B):
        """X = L^-T B for B [n x r] (host or device), L the image of `chol` (pk_trsm_f64 on a padded copy)."""
        from . import hybrid
        n = int(n)
        B = torch.as_tensor(np.ascontiguousarray(B) if isinstance(B, np.ndarray) else B)
        r = int(B.shape[1])
        W = torch.empty(hybrid.leading_dim(n), r, dtype=torch.float64, device=self.device)
        W[:n] = B.to(device=self.device, dtype=torch.float64)
        with self._timed('trsm', (n, r)):
            _lib.check(self.lib.pk_trsm_f64(self.stream(), n, r, _ptr(L), L.stride(0), _ptr(W), W.stride(0)), 'pk_trsm_f64')
        return W[:n]

    # ---- EASE: closed-form item weights on the Cholesky image (csrc/hybrid.hip) ------------------------------------------
    def ease_gram(self, A, lam):
        """The Cholesky image [ld x ld] of K = A^T A + lam I for the device CSR A: the rows of A^T A and the diagonal go
        straight into the image (`_gram_image`).  Raises MemoryError before allocating when this image and the weights
        image together would take more than half of the free device memory (ease.check_build_memory)."""
        from . import ease
        n_items = int(A.shape[1])
        ease.check_build_memory(n_items, self.free_bytes())
        ld = ease.chol_leading_dim(n_items)
        return self._gram_image('ease_gram', A, ld, ld, diag=lam)

    def trtri(self, img, n):
        """In place W = L^-1 of the lower factor `chol` left in the image (pk_trtri_f64); the padding stays the identity."""
        n = int(n)
        work = self._work(self.lib.pk_trtri_work_bytes(n))
        with self._timed('trtri', (n,)):
            _lib.check(self.lib.pk_trtri_f64(self.stream(), n, _ptr(img), img.stride(0), _ptr(work)), 'pk_trtri_f64')
        return img

    def ease_weights(self, img, n):
        """(B, d) from the image of `trtri`: the scoring image B [n x i2i.leading_dim(n)] of the EASE weights (diagonal and
        pad columns 0) and d = diag (K^-1) [n], both fp64 on the device (pk_ease_weights_f64)."""
        from . import i2i
        n = int(n)
        ldb = i2i.leading_dim(n)
        B = torch.empty(n, ldb, dtype=torch.float64, device=self.device)
        d = torch.empty(n, dtype=torch.float64, device=self.device)
        with self._timed('ease_weights', (n,)):
            _lib.check(self.lib.pk_ease_weights_f64(self.stream(), n, _ptr(img), img.stride(0), _ptr(d), _ptr(B), ldb),
                       'pk_ease_weights_f64')
        return B, d

    # ---- SLIM: sparse item weights by coordinate descent over the Gram image (csrc/slim.hip) ----------------------------
    def slim_gram(self, A, column_batch=None):
        """The Gram image [n_items x slim.gram_leading_dim(n_items)] of G = A^T A WITH its diagonal for the device CSR A
        (`_gram_image` with 0 added to the diagonal); the pad columns are 0.  Raises ValueError beyond
        pk_slim_max_items() and MemoryError before allocating when the image and one batch block of `column_batch` columns
        (default: the default rule) would take more than half of the free device memory (slim.check_build_memory)."""
        from . import slim
        n_items = int(A.shape[1])
        slim.check_build_memory(n_items, self.free_bytes(), column_batch)
        return self._gram_image('slim_gram', A, n_items, slim.gram_leading_dim(n_items), diag=0.0)

    def slim_solve(self, G, n, j0, nc, l1, l2, tol, max_sweeps, positive=True, out=None):
        """(Wt_block, sweeps): the target columns [j0, j0 + nc) of the SLIM problem over the Gram image G of n items, as the
        rows of a dense fp64 device block [nc x slim.gram_leading_dim(n)] of W^T (pad columns exactly 0), and the int32
        device vector of the sweeps run per column (pk_slim_solve_f64: the contract of include/polara_hip.h).  `out`: a
        block of at least nc rows to write into."""
        from . import slim
        n, j0, nc = int(n), int(j0), int(nc)
        slim.check_items(n)
        l1, l2, tol, max_sweeps = slim.check_parameters(l1, l2, tol, max_sweeps)
        if not 0 <= j0 <= j0 + nc <= n:
            raise ValueError('slim_solve: columns [%d, %d) outside the %d items' % (j0, j0 + nc, n))
        ldw = slim.gram_leading_dim(n)
        if out is None:
            out = torch.empty(max(nc, 1), ldw, dtype=torch.float64, device=self.device)
        if out.dtype != torch.float64 or out.shape[0] < nc or out.stride(0) < n or out.stride(1) != 1:
            raise ValueError('slim_solve: the output block does not hold %d rows of %d fp64 columns' % (nc, n))
        block = out[:nc]
        sweeps = torch.empty(max(nc, 1), dtype=torch.int32, device=self.device)[:nc]
        work = self._work(self.lib.pk_slim_work_bytes(n, nc))
        with self._timed('slim_solve', (n, nc)):
            _lib.check(self.lib.pk_slim_solve_f64(self.stream(), n, _ptr(G), G.stride(0), j0, nc, l1, l2, tol, max_sweeps,
                                                  1 if positive else 0, _ptr(block), out.stride(0), _ptr(sweeps), _ptr(work)),
                       'pk_slim_solve_f64')
        return block, sweeps

    def slim_csr(self, Wt_block, n):
        """(indptr int64 [nc + 1], indices int32, values fp64), all on the device: the rows of the block of `slim_solve` as
        CSR rows — an entry is stored when it is != 0, in ascending index order (pk_slim_csr_count, pk_slim_csr_fill)."""
        n, nc = int(n), int(Wt_block.shape[0])
        indptr = torch.empty(nc + 1, dtype=torch.int64, device=self.device)
        work = self._work(8 * nc)
        with self._timed('slim_csr', (n, nc)):
            _lib.check(self.lib.pk_slim_csr_count(self.stream(), nc, n, _ptr(Wt_block), Wt_block.stride(0), _ptr(indptr),
                                                  _ptr(work)), 'pk_slim_csr_count')
            nnz = int(indptr[-1].item())
            indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=self.device)[:nnz]
            values = torch.empty(max(nnz, 1), dtype=torch.float64, device=self.device)[:nnz]
            _lib.check(self.lib.pk_slim_csr_fill(self.stream(), nc, n, _ptr(Wt_block), Wt_block.stride(0), _ptr(indptr), nnz,
                                                 _ptr(indices), _ptr(values)), 'pk_slim_csr_fill')
        return indptr, indices, values

    # ---- ItemKNN / RP3beta: top-K pruning of the normalised Gram image (csrc/knn.hip) ---------------------------------
    def knn_gram(self, A):
        """The Gram image [n_items x i2i.leading_dim(n_items)] of G = A^T A WITH its true diagonal for the device CSR A
        (`_gram_image` with 0 added to the diagonal); the pad columns are 0.  Raises MemoryError before allocating when
        the image would take more than half of the free device memory (i2i.check_build_memory)."""
        from . import i2i
        n_items = int(A.shape[1])
        i2i.check_build_memory(n_items, self.free_bytes())
        return self._gram_image('knn_gram', A, n_items, i2i.leading_dim(n_items), diag=0.0)

    def csr_row_scaled_power(self, A, row_scale, alpha):
        """The DeviceCSR (fp64, pattern and plans of A) with the values row_scale[u] * a^alpha for the host fp64 vector
        `row_scale` [n_rows].  a^alpha is exact NumPy: with alpha != 1 and values other than 1 the DISTINCT stored values
        are powered on the host (np.power; a stored 0 stays 0, also at alpha = 0) and gathered, so every stored value is one
        IEEE product of two known doubles."""
        alpha = float(alpha)
        vals = A.values.to(torch.float64)
        if alpha != 1.0 and vals.numel() and not bool((vals == 1.0).all().item()):
            distinct, where = torch.unique(vals, return_inverse=True)
            table = self.to_host(distinct)
            table = np.where(table == 0, 0.0, np.power(table, alpha))      # a stored 0 stays 0 (no walk), also at alpha = 0
            vals = self.to_device(table)[where]
        rows = torch.repeat_interleave(torch.arange(A.shape[0], device=self.device), A.indptr[1:] - A.indptr[:-1])
        scale = self.to_device(np.ascontiguousarray(row_scale, dtype=np.float64))
        new = A.with_columns(A.indices, scale[rows] * vals)
        new.val_kind = _lib.PK_VAL_F64
        return new

    def knn_prune_slots(self, G, n, kind, row, col, shrink, K, normalize):
        """(count int32 [n], idx int32 [n x K], val fp64 [n x K]), all on the device: the K best normalised entries of
        every row of the fp64 image G [>= n rows, row stride >= n], in ascending column order, pads idx -1 / val 0
        (pk_knn_prune_f64: the contract of include/polara_hip.h).  `kind`: knn.KINDS; row, col: n doubles each, host arrays
        or device tensors."""
        from . import knn
        n, K = int(n), knn.check_neighbours(K)
        if (G.dtype != torch.float64 or G.dim() != 2 or G.stride(1) != 1 or G.shape[0] < n or G.shape[1] < n
                or G.device.type != self.device.type
                or (self.device.index is not None and G.device.index != self.device.index)):
            raise ValueError('knn_prune: the image does not hold %d rows of %d fp64 columns on %s' % (n, n, self.device))
        vec = []
        for name, v in (('row', row), ('col', col)):
            v = v if torch.is_tensor(v) else self.to_device(np.asarray(v, dtype=np.float64))
            v = v.to(device=self.device, dtype=torch.float64).contiguous()
            if v.numel() != n:
                raise ValueError('knn_prune: `%s` holds %d numbers for %d items' % (name, v.numel(), n))
            vec.append(v)
        count = torch.empty(n, dtype=torch.int32, device=self.device)
        idx = torch.empty(n, K, dtype=torch.int32, device=self.device)
        val = torch.empty(n, K, dtype=torch.float64, device=self.device)
        with self._timed('knn_prune', (n, K)):
            _lib.check(self.lib.pk_knn_prune_f64(self.stream(), n, _ptr(G), G.stride(0), int(kind), _ptr(vec[0]), _ptr(vec[1]),
                                                 float(shrink), K, 1 if normalize else 0, _ptr(count), _ptr(idx), _ptr(val)),
                       'pk_knn_prune_f64')
        return count, idx, val

    def knn_prune(self, G, n, kind, row, col, shrink, K, normalize):
        """The canonical DeviceCSR [n x n] (fp64) of `knn_prune_slots`: indptr is the cumulative sum of the counts,
        indices and values the non-pad slots in row-major order."""
        n = int(n)
        count, idx, val = self.knn_prune_slots(G, n, kind, row, col, shrink, K, normalize)
        indptr = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(count, 0, out=indptr[1:])
        stored = idx >= 0
        W = DeviceCSR.from_device(self, indptr, idx[stored], val[stored], (n, n))
        return W

    # ---- the neighbour pass without an image (csrc/uknn.hip) and scoring with a separate seen set ------------------------
    def _own_csr(self, A, what):
        """`A` must be a DeviceCSR of this device (its addresses are handed to a kernel)."""
        for t in (getattr(A, 'indptr', None), getattr(A, 'indices', None), getattr(A, 'values', None)):
            if not torch.is_tensor(t) or t.device.type != self.device.type or (
                    self.device.index is not None and t.device.index != self.device.index):
                raise ValueError('%s is no device CSR on %s' % (what, self.device))
        if A.indptr.dtype != torch.int64 or A.indices.dtype != torch.int32 or A.values.dtype not in (torch.float32, torch.float64):
            raise ValueError('%s: int64 indptr, int32 indices and fp32 or fp64 values expected' % what)
        return A

    def spsp_knn_slots(self, L, B, kind, row, col, shrink, K, normalize, exclude=None):
        """(count int32 [n_rows], idx int32 [n_rows x K], val fp64 [n_rows x K]), all on the device: the K best normalised
        entries of every row of L B for the device CSR L [n_rows x n_inner] and the canonical device CSR B [n_inner x
        n_cols], in ascending column order, pads idx -1 / val 0 (pk_spsp_knn_f64: the contract of include/polara_hip.h; no
        image of the product exists).  `kind`: knn.KINDS; row: n_rows doubles, col: n_cols doubles, host arrays or device
        tensors; exclude: None or n_rows int32 column ids (negative: nothing) a row may not keep."""
        from . import knn, simagg
        self._own_csr(L, 'spsp_knn: L')
        self._own_csr(B, 'spsp_knn: B')
        n_rows, n_inner, n_cols = simagg.check_shapes(L.shape, B.shape)
        K = knn.check_neighbours(K)
        vec = []
        for name, v, n in (('row', row, n_rows), ('col', col, n_cols)):
            v = v if torch.is_tensor(v) else self.to_device(np.asarray(v, dtype=np.float64))
            v = v.to(device=self.device, dtype=torch.float64).contiguous()
            if v.numel() != n:
                raise ValueError('spsp_knn: `%s` holds %d numbers, %d expected' % (name, v.numel(), n))
            vec.append(v)
        if exclude is not None:
            exclude = exclude if torch.is_tensor(exclude) else torch.as_tensor(np.asarray(exclude, dtype=np.int32))
            exclude = exclude.to(device=self.device, dtype=torch.int32).contiguous()
            if exclude.numel() != n_rows:
                raise ValueError('spsp_knn: `exclude` holds %d ids for %d rows' % (exclude.numel(), n_rows))
        count = torch.empty(n_rows, dtype=torch.int32, device=self.device)
        idx = torch.empty(n_rows, K, dtype=torch.int32, device=self.device)
        val = torch.empty(n_rows, K, dtype=torch.float64, device=self.device)
        work = self._work(self.lib.pk_spsp_knn_work_bytes(n_rows, n_cols, K))
        with self._timed('spsp_knn', (n_rows, n_cols, L.nnz, K)):
            _lib.check(self.lib.pk_spsp_knn_f64(self.stream(), n_rows, n_inner, n_cols, _ptr(L.indptr), _ptr(L.indices),
                                                _ptr(L.values), L.val_kind, _ptr(B.indptr), _ptr(B.indices),
                                                _ptr(self._spsp_values(B)), int(kind), _ptr(vec[0]), _ptr(vec[1]), float(shrink),
                                                _ptr(exclude), K, 1 if normalize else 0, _ptr(count), _ptr(idx), _ptr(val),
                                                _ptr(work)), 'pk_spsp_knn_f64')
        return count, idx, val

    def spsp_knn(self, L, B, kind, row, col, shrink, K, normalize, exclude=None):
        """The canonical DeviceCSR [n_rows x n_cols] (fp64) of `spsp_knn_slots`, built as `knn_prune` builds its own."""
        count, idx, val = self.spsp_knn_slots(L, B, kind, row, col, shrink, K, normalize, exclude)
        indptr = torch.zeros(count.numel() + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(count, 0, out=indptr[1:])
        stored = idx >= 0
        return DeviceCSR.from_device(self, indptr, idx[stored], val[stored], (int(L.shape[0]), int(B.shape[1])))

    def spsp_topk_seen(self, L, B, seen, topk, filter_seen, sparse, want_scores=False):
        """`spsp_topk` with the seen set of row r taken from row r of the device CSR `seen` [n_rows x n_cols] (its pattern;
        sorted columns) instead of L's own row, so L's inner dimension need not be the catalogue (pk_spsp_topk_seen)."""
        from . import simagg
        self._own_csr(L, 'spsp_topk_seen: L')
        self._own_csr(B, 'spsp_topk_seen: B')
        self._own_csr(seen, 'spsp_topk_seen: seen')
        n_rows, n_inner, n_cols = simagg.check_shapes(L.shape, B.shape)
        if tuple(seen.shape) != (n_rows, n_cols) or not getattr(seen, 'sorted_cols', True):
            raise ValueError('spsp_topk_seen: the seen set is %s (sorted columns: %s), the scores are %d x %d'
                             % (tuple(seen.shape), getattr(seen, 'sorted_cols', True), n_rows, n_cols))
        topk = int(topk)
        out = torch.empty(n_rows, topk, dtype=torch.int64, device=self.device)
        scores = torch.empty(n_rows, topk, dtype=torch.float64, device=self.device) if want_scores else None
        work = self._work(self.lib.pk_spsp_topk_work_bytes(n_rows, n_cols, topk))
        with self._timed('spsp_topk_seen', (n_rows, n_cols, L.nnz, topk)):
            _lib.check(self.lib.pk_spsp_topk_seen(self.stream(), n_rows, n_inner, n_cols, _ptr(L.indptr), _ptr(L.indices),
                                                  _ptr(L.values), L.val_kind, _ptr(B.indptr), _ptr(B.indices),
                                                  _ptr(self._spsp_values(B)), _ptr(seen.indptr), _ptr(seen.indices), topk,
                                                  1 if filter_seen else 0, 1 if sparse else 0, _ptr(out), _ptr(scores),
                                                  _ptr(work)), 'pk_spsp_topk_seen')
        return out, scores

    # ---- item cold start -----------------------------------------------------------------------------------------
    def coldstart_queries(self, F, W, G):
        """E = (F W) G for the cold items of a DeviceCSR over the training labels, fp64: the SpMM and the tall-skinny product
        of the build (pk_spmm_csr_ex, pk_tsmm_f64), the second writing straight into a block whose rows are 16-byte aligned
        with an even leading dimension (what `sweep_takes_rows` asks for; the padding column of an odd rank is zeroed).
        Returns the [n_cold x rank] view.  (A fused kernel was built and measured slower: DESIGN.md 8c.)"""
        assert W.dtype == torch.float64 and W.stride(1) == 1 and G.dtype == torch.float64 and G.stride(1) == 1
        n_cold, rank = int(F.shape[0]), int(W.shape[1])
        if F.shape[1] != W.shape[0] or tuple(G.shape) != (rank, rank):
            raise ValueError('coldstart_queries: features %s, W %s, G %s do not fit' % (F.shape, tuple(W.shape), tuple(G.shape)))
        lde = rank + (rank & 1)
        block = self.zeros(n_cold, lde) if lde != rank else self.empty(n_cold, lde)
        with self._timed('coldstart_queries', (n_cold, int(W.shape[0]), rank)):
            self.tsmm(self.spmm(F, W), G, out=block[:, :rank])
        return block[:, :rank]

    def clamp_min(self, E, lo=0.0):
        """E <- max(E, lo) in place (pk_clamp_min_f64): LCE's cold-start queries (coldstart/models.py:144)."""
        assert E.dtype == torch.float64 and E.dim() == 2 and E.stride(1) == 1
        _lib.check(self.lib.pk_clamp_min_f64(self.stream(), int(E.shape[0]), int(E.shape[1]), _ptr(E), E.stride(0), float(lo)),
                   'pk_clamp_min_f64')
        return E

    # ---- Local Collective Embeddings (csrc/lce.hip) ----------------------------------------------------------------
    def csr_scaled(self, A, s):
        """A DeviceCSR with the pattern (and plan) of A and the fp64 values s * A.values"""
        new = A.with_columns(A.indices, A.values.to(torch.float64) * float(s))
        new.val_kind = _lib.PK_VAL_F64
        return new

    def csr_values(self, A):
        return A.values

    def spmm_acc(self, A, X, out):
        """out += A @ X (pk_spmm_csr_ex with accumulate = 1; the sums of a row are added to what `out` holds)"""
        assert X.dtype == torch.float64 and X.stride(-1) == 1 and X.shape[0] == A.shape[1] and out.shape[0] == A.shape[0]
        for c0 in range(0, X.shape[1], 256):        # one output row per wave in registers: 256 columns per launch
            self._spmm_launch(A, X[:, c0:c0 + 256], out[:, c0:c0 + 256], (0, A.n_tasks, 0, A.n_long), accumulate=True)
        return out

    def lce_fused_max_rank(self):
        return int(self.lib.pk_lce_fused_max_rank())

    def lce_update(self, X, N, M1, ma=1.0, M2=None, mb=0.0, a=1.0, lamb=0.0, c=None, fused=None):
        """X <- X o (a N) / max(X M + (lamb + c_i) X, 1e-10) in place, M = ma M1 + mb M2 (k x k).  fused=None: one launch
        (pk_lce_update_f64) up to lce_fused_max_rank(), above it the composition M -> pk_tsmm_f64 -> pk_lce_update_ew_f64;
        True / False force one form (False at any rank: the comparison of tools/bench_lce.py; True above the bound raises)."""
        assert X.dtype == torch.float64 and X.dim() == 2 and X.stride(1) == 1 and N.stride(1) == 1 and tuple(N.shape) == tuple(X.shape)
        m, k = int(X.shape[0]), int(X.shape[1])
        assert tuple(M1.shape) == (k, k) and M1.stride(1) == 1 and (M2 is None or (tuple(M2.shape) == (k, k) and M2.stride(1) == 1))
        assert c is None or (c.dtype == torch.float64 and c.numel() == m and c.is_contiguous())
        if fused is None:
            fused = k <= self.lce_fused_max_rank()
        if fused:
            with self._timed('lce_update', (m, k)):
                _lib.check(self.lib.pk_lce_update_f64(self.stream(), m, k, _ptr(X), X.stride(0), _ptr(N), N.stride(0), _ptr(M1),
                                                      M1.stride(0), float(ma), _ptr(M2), M2.stride(0) if M2 is not None else 0,
                                                      float(mb), float(a), float(lamb), _ptr(c)), 'pk_lce_update_f64')
            return X
        with self._timed('lce_update_composed', (m, k)):
            M = self.axpbypcz(float(ma), M1.contiguous(), float(mb) if M2 is not None else 0.0, M2.contiguous() if M2 is not None else None)
            P = self.tsmm(X, M)
            _lib.check(self.lib.pk_lce_update_ew_f64(self.stream(), m, k, _ptr(X), X.stride(0), _ptr(N), N.stride(0), _ptr(P),
                                                     P.stride(0), float(a), float(lamb), _ptr(c)), 'pk_lce_update_ew_f64')
        return X

    def lce_dots(self, pairs, bias=0.0):
        """[1 + n] device doubles: out[1 + p] = sum_ij w[i] P[i, j] Q[i, j] of pairs[p] = (coef, P, Q | None, w | None) and
        out[0] = bias + sum_p coef_p out[1 + p] (pk_lce_dots_f64: two launches, fixed summation order, no atomics)."""
        n = len(pairs)
        vp = C.c_void_p * n
        ptr = lambda t: None if t is None else t.data_ptr()
        for _, P, Q, w in pairs:
            assert P.dtype == torch.float64 and P.dim() == 2 and (P.stride(1) == 1 or P.shape[1] == 1)
            assert Q is None or (Q.dtype == torch.float64 and tuple(Q.shape) == tuple(P.shape) and (Q.stride(1) == 1 or Q.shape[1] == 1))
            assert w is None or (w.dtype == torch.float64 and w.numel() == P.shape[0] and w.is_contiguous())
        Pa = vp(*[ptr(p[1]) for p in pairs])
        Qa = vp(*[ptr(p[2]) for p in pairs])
        wa = vp(*[ptr(p[3]) for p in pairs])
        ma = (C.c_int64 * n)(*[int(p[1].shape[0]) for p in pairs])
        ka = (C.c_int32 * n)(*[int(p[1].shape[1]) for p in pairs])
        lp = (C.c_int64 * n)(*[int(p[1].stride(0)) for p in pairs])
        lq = (C.c_int64 * n)(*[int(p[2].stride(0)) if p[2] is not None else 0 for p in pairs])
        co = (C.c_double * n)(*[float(p[0]) for p in pairs])
        if _PTR_KEEP is not None:
            _PTR_KEEP.extend(t for p in pairs for t in p[1:] if t is not None)
        out = self.empty(1 + n)
        if getattr(self, '_lce_dots_work', None) is None:
            self._lce_dots_work = {}
        work = self._lce_dots_work.get(self.stream_key())
        if work is None:
            work = self._lce_dots_work[self.stream_key()] = self._work(self.lib.pk_lce_dots_work_bytes())
        _lib.check(self.lib.pk_lce_dots_f64(self.stream(), n, Pa, Qa, wa, ma, ka, lp, lq, co, float(bias), _ptr(out), _ptr(work)),
                   'pk_lce_dots_f64')
        return out

    # ---- Probabilistic matrix factorisation (csrc/pmf.hip) -----------------------------------------------------------
    def pmf_max_rank(self):
        return int(self.lib.pk_pmf_max_rank())

    @staticmethod
    def _schedule_parts(cnt, B, nnz):
        """pmf._parts on the device: the part of every user (item) from its entry counts (int64), integers only"""
        return torch.clamp((torch.cumsum(cnt, 0) - cnt) * B // max(nnz, 1), max=B - 1)

    def _block_schedule(self, A, blocks, what, item_order=None):
        """The one copy of the blocked schedule (pmf.block_schedule) behind pmf_plan and bpr_plan, built on the device with
        integer arithmetic only and the library's stable radix sort of (s * B + i, position) pairs.  item_order (a device
        int64 permutation of the items, None: the identity): the items are cut into parts along it.  Returns (users, items,
        ucnt, icnt — int64, canonical order —, perm, block_ptr, the item parts along the order [n_items] int64)."""
        n_users, n_items = A.shape
        B, nnz = int(blocks), int(A.nnz)
        if B < 1 or B > min(n_users, n_items):
            raise ValueError('%s: %d blocks for %d users and %d items (1 .. min of the two)' % (what, B, n_users, n_items))
        if B > _lib.PK_PMF_MAX_BLOCKS:
            raise ValueError('%s: %d blocks, the library takes at most %d' % (what, B, _lib.PK_PMF_MAX_BLOCKS))
        if nnz >= 2 ** 31:
            raise ValueError('%s: %d interactions, the schedule is indexed with 32 bits' % (what, nnz))
        dev = self.device
        indptr = A.indptr[:n_users + 1]
        items = A.indices[:nnz].to(torch.int64)
        ucnt = indptr[1:] - indptr[:-1]
        users = torch.repeat_interleave(torch.arange(n_users, dtype=torch.int64, device=dev), ucnt, output_size=nnz)
        icnt = self.bincount(items, n_items) if nnz else torch.zeros(n_items, dtype=torch.int64, device=dev)
        part = lambda cnt: self._schedule_parts(cnt, B, nnz)
        if item_order is None:
            ordered_parts = ipart = part(icnt)
        else:
            ordered_parts = part(icnt[item_order])
            ipart = torch.empty_like(ordered_parts)
            ipart[item_order] = ordered_parts
        i, j = part(ucnt)[users], ipart[items]
        keys = (torch.remainder(j - i, B) * B + i).to(torch.int32).contiguous()
        block_ptr = torch.zeros(B * B + 1, dtype=torch.int64, device=dev)
        n1 = max(nnz, 1)
        pos = torch.arange(n1, dtype=torch.int32, device=dev)
        in_tmp = C.c_int32(0)
        pos_tmp = torch.empty_like(pos)
        if nnz:
            block_ptr[1:] = torch.cumsum(self.bincount(keys, B * B), 0)
            keys_tmp = torch.empty_like(keys)
            bits = max(1, int(B * B - 1).bit_length())
            work = self._work(self.lib.pk_radix_work_bytes(nnz))
            _lib.check(self.lib.pk_radix_sort_pairs(self.stream(), nnz, 4, _ptr(keys), _ptr(pos), _ptr(keys_tmp), _ptr(pos_tmp),
                                                    bits, _ptr(work), C.byref(in_tmp)), 'pk_radix_sort_pairs')
        perm = (pos_tmp if in_tmp.value else pos)[:nnz].to(torch.int64)
        return users, items, ucnt, icnt, perm, block_ptr, ordered_parts

    def pmf_plan(self, A, blocks):
        """The blocked schedule of pmf.block_schedule for the entries of the canonical DeviceCSR `A` [n_users x n_items],
        built on the device with integer arithmetic only (so that it equals the host plan element for element) and the
        library's stable radix sort of (s * B + i, position) pairs.  Returns a dict: perm, block_ptr (int64), users, items
        (int32) and vals (fp64) in schedule order, row_nnz / col_nnz (the entry counts as fp64), blocks, nnz, shape."""
        n_users, n_items = A.shape
        B, nnz = int(blocks), int(A.nnz)
        with self._timed('pmf_plan', (n_users, n_items, nnz, B)):
            users, items, ucnt, icnt, perm, block_ptr, _ = self._block_schedule(A, B, 'PMF')
            vals = A.values[:nnz].to(torch.float64)
            if nnz and bool((vals == 0).any().item()):
                raise ValueError('PMF: an interaction with feedback 0 (after summing duplicates)')
            return dict(blocks=B, nnz=nnz, shape=(n_users, n_items), perm=perm, block_ptr=block_ptr,
                        users=users[perm].to(torch.int32).contiguous(), items=items[perm].to(torch.int32).contiguous(),
                        vals=vals[perm].contiguous(), row_nnz=ucnt.to(torch.float64).contiguous(),
                        col_nnz=icnt.to(torch.float64).contiguous())

    _PMF_ADJUST = {None: 0, 'adagrad': 1, 'rmsprop': 2}

    @staticmethod
    def _check_row_blocks(what, blocks, rows, cols):
        """every block is fp64 [n x cols] with unit column stride, n running through `rows` again and again"""
        for X, n in zip(blocks, tuple(rows) * len(blocks)):
            if X.dtype != torch.float64 or X.dim() != 2 or tuple(X.shape) != (n, cols) or X.stride(1) != 1 or X.stride(0) < cols:
                raise ValueError('%s: a block of shape %s, strides %s for [%d x %d] fp64 rows' % (what, tuple(X.shape), X.stride(), n, cols))

    @staticmethod
    def _check_plan(plan, what, users=(), items=(), entries=(), **others):
        """B of a plan of `what`_plan: block_ptr holds B * B + 1 elements, the named tensors one per user, per item and per
        entry, and the `others` as many as given"""
        B = int(plan['blocks'])
        n_users, n_items = plan['shape']
        want = dict(others, block_ptr=B * B + 1)
        for names, n in ((users, n_users), (items, n_items), (entries, plan['nnz'])):
            want.update((name, n) for name in names)
        if any(name not in plan or plan[name].numel() != n for name, n in want.items()):
            raise ValueError('%s: not a plan of %s_plan' % (what, what.lower()))
        return B

    def _pmf_sweep(self, what, B, plan, P, Q, eta, lambd, adjust, state, gamma, smoothing, sizes=(), kernelized=(), snapshots=()):
        """pmf_epoch and kpmf_epoch behind their plan checks: rank, adjuster, state and blocks checked under the model's name
        `what`, then pk_pmf_epoch_f64, or pk_kpmf_epoch_f64 with its `sizes` and `kernelized` arguments in their places"""
        n_users, n_items = plan['shape']
        k = int(P.shape[1])
        if k < 1 or k > self.pmf_max_rank():
            raise ValueError('%s: rank %d outside 1..%d' % (what, k, self.pmf_max_rank()))
        if adjust not in self._PMF_ADJUST:
            raise ValueError('%s: unknown gradient adjustment %r' % (what, adjust))
        if adjust and (state is None or len(state) != 2):
            raise ValueError('%s: the gradient adjustment %r needs state = (SP, SQ)' % (what, adjust))
        self._check_row_blocks(what, (P, Q) + tuple(snapshots) + (tuple(state) if adjust else ()), (n_users, n_items), k)
        SP, SQ = state if adjust else (None, None)
        work = self.empty(int(self.lib.pk_pmf_work_doubles(B)))       # the block sums of the squared error
        out = self.empty(1)
        name = what.lower() + '_epoch'
        entry = 'pk_%s_f64' % name
        with self._timed(name, (plan['nnz'], k, B)):
            _lib.check(getattr(self.lib, entry)(
                self.stream(), B, k, int(plan['nnz']), *sizes, _ptr(plan['block_ptr']), _ptr(plan['users']), _ptr(plan['items']),
                _ptr(plan['vals']), _ptr(P), P.stride(0), _ptr(Q), Q.stride(0), _ptr(plan['row_nnz']), _ptr(plan['col_nnz']),
                *kernelized, float(eta), float(lambd), self._PMF_ADJUST[adjust], _ptr(SP), SP.stride(0) if adjust else 0, _ptr(SQ),
                SQ.stride(0) if adjust else 0, float(gamma), float(smoothing), _ptr(work), _ptr(out)), entry)
        return out

    def pmf_epoch(self, plan, P, Q, eta, lambd, adjust=None, state=None, gamma=0.9, smoothing=1e-6):
        """One SGD sweep over the plan's interactions (pk_pmf_epoch_f64: one launch per stratum and one for the squared
        error), P [n_users x k] and Q [n_items x k] updated in place.  adjust: None, 'adagrad' or 'rmsprop' with
        state = (SP, SQ) of the shapes of P and Q, zeroed by the caller before every epoch.  Returns a device tensor of one
        double: the epoch's squared error."""
        B = self._check_plan(plan, 'PMF', users=('row_nnz',), items=('col_nnz',), entries=('users',))
        return self._pmf_sweep('PMF', B, plan, P, Q, eta, lambd, adjust, state, gamma, smoothing)

    # ---- Kernelized probabilistic matrix factorisation (csrc/kpmf.hip) ------------------------------------------------------
    def kpmf_plan(self, A, blocks, Ku, Ki):
        """pmf_plan(A, blocks) plus what the kernelized sweep reads: user_part / item_part (int32: the part of every user and
        item in the schedule) and, for the kernel matrices Ku [n_users x n_users] and Ki [n_items x n_items] (SciPy sparse,
        made canonical here), their off-diagonal CSR (ku_ptr int64, ku_idx int32, ku_val fp64) and their diagonal (ku_diag
        fp64, 0 where none is stored); likewise ki_*.  Everything on the device."""
        from . import kpmf
        plan = self.pmf_plan(A, blocks)
        n_users, n_items = plan['shape']
        B, nnz = plan['blocks'], plan['nnz']
        with self._timed('kpmf_plan', (n_users, n_items, nnz, B)):
            plan['user_part'] = self._schedule_parts(plan['row_nnz'].to(torch.int64), B, nnz).to(torch.int32).contiguous()
            plan['item_part'] = self._schedule_parts(plan['col_nnz'].to(torch.int64), B, nnz).to(torch.int32).contiguous()
            for side, K, n in (('ku', Ku, n_users), ('ki', Ki, n_items)):
                ptr, idx, val, diag = kpmf.split_kernel(K, n)
                plan[side + '_ptr'], plan[side + '_idx'] = self.to_device(ptr), self.to_device(idx)
                plan[side + '_val'], plan[side + '_diag'] = self.to_device(val), self.to_device(diag)
        return plan

    def kpmf_epoch(self, plan, P, Q, eta, lambd, adjust=None, state=None, gamma=0.9, smoothing=1e-6, snapshots=None):
        """One kernelized SGD sweep over the plan's interactions (pk_kpmf_epoch_f64: per stratum one launch of the sweep and
        one that refreshes the snapshots, and one for the squared error), P and Q updated in place.  adjust / state as in
        pmf_epoch.  snapshots = (P_snap, Q_snap) of the shapes of P and Q (leading dimensions of their own; allocated here
        when None): whatever they hold is overwritten, and they equal P and Q when the epoch ends.  Returns a device tensor
        of one double: the epoch's squared error."""
        n_users, n_items = plan['shape']
        if snapshots is None:
            snapshots = (self.empty(n_users, int(P.shape[1])), self.empty(n_items, int(P.shape[1])))
        if len(snapshots) != 2:
            raise ValueError('KPMF: snapshots = (P_snap, Q_snap)')
        B = self._check_plan(plan, 'KPMF', users=('row_nnz', 'user_part', 'ku_diag'), items=('col_nnz', 'item_part', 'ki_diag'),
                             entries=('users',), ku_ptr=n_users + 1, ki_ptr=n_items + 1)
        PS, QS = snapshots
        kernelized = [_ptr(plan[name]) for name in ('user_part', 'item_part', 'ku_ptr', 'ku_idx', 'ku_val', 'ku_diag', 'ki_ptr',
                                                    'ki_idx', 'ki_val', 'ki_diag')] + [_ptr(PS), PS.stride(0), _ptr(QS), QS.stride(0)]
        return self._pmf_sweep('KPMF', B, plan, P, Q, eta, lambd, adjust, state, gamma, smoothing, sizes=(n_users, n_items),
                               kernelized=kernelized, snapshots=snapshots)

    # ---- Bayesian personalised ranking (csrc/bpr.hip) -------------------------------------------------------------------
    def bpr_max_rank(self):
        return int(self.lib.pk_bpr_max_rank())

    def bpr_plan(self, A, blocks, item_order=None):
        """The schedule of one BPR epoch (bpr.block_schedule) for the stored entries of the canonical DeviceCSR `A`
        [n_users x n_items]: PMF's schedule with the items cut into parts along `item_order` (a host permutation of the
        items; None: the identity).  Returns a dict: perm (the canonical index of every position), block_ptr, item_ptr (int64),
        users, items (the schedule's, int32), item_order, item_part (int32), matrix, blocks, nnz, shape."""
        n_users, n_items = A.shape
        B, nnz = int(blocks), int(A.nnz)
        if not getattr(A, 'sorted_cols', True):
            raise ValueError('BPR: the training matrix must be canonical (sorted columns)')
        if item_order is None:
            order = torch.arange(n_items, dtype=torch.int64, device=self.device)
        else:
            host = np.ascontiguousarray(item_order, dtype=np.int64)
            if host.shape != (n_items,) or not np.array_equal(np.sort(host), np.arange(n_items)):
                raise ValueError('BPR: item_order is not a permutation of the %d items' % n_items)
            order = self.to_device(host)
        with self._timed('bpr_plan', (n_users, n_items, nnz, B)):
            users, items, _, _, perm, block_ptr, ordered_parts = self._block_schedule(A, B, 'BPR', None if item_order is None else order)
            item_ptr = torch.zeros(B + 1, dtype=torch.int64, device=self.device)
            item_ptr[1:] = torch.cumsum(self.bincount(ordered_parts, B), 0)
            item_part = torch.empty(n_items, dtype=torch.int32, device=self.device)
            item_part[order] = ordered_parts.to(torch.int32)
            return dict(blocks=B, nnz=nnz, shape=(n_users, n_items), perm=perm.contiguous(), block_ptr=block_ptr, item_ptr=item_ptr,
                        users=users[perm].to(torch.int32).contiguous(), items=items[perm].to(torch.int32).contiguous(),
                        item_order=order.to(torch.int32).contiguous(), item_part=item_part, matrix=A)

    def _bpr_check_plan(self, plan):
        return self._check_plan(plan, 'BPR', items=('item_order', 'item_part'), entries=('users', 'items', 'perm'),
                                item_ptr=int(plan['blocks']) + 1)

    def _pair_draw(self, what, name, entry, B, plan, seed, epoch, draws=()):
        """bpr_draw_negatives and warp_draw (`name`) behind their plan checks: seed and epoch checked under the model's name
        `what`, the int32 output [nnz (x draws)] allocated, then `entry` with `draws` in its place among the arguments both take"""
        seed, epoch = int(seed), int(epoch)
        if not (0 <= seed < 2 ** 32 and 0 <= epoch < 2 ** 32):
            raise ValueError('%s: seed %d and epoch %d must fit 32 unsigned bits' % (what, seed, epoch))
        n_users, n_items = plan['shape']
        A, nnz = plan['matrix'], int(plan['nnz'])
        out = torch.empty(max(nnz, 1), *draws, dtype=torch.int32, device=self.device)[:nnz]
        with self._timed(name, (nnz, *draws, B)):
            _lib.check(getattr(self.lib, entry)(
                self.stream(), nnz, n_users, n_items, B, *draws, _ptr(plan['users']), _ptr(plan['items']), _ptr(plan['perm']),
                _ptr(plan['item_order']), _ptr(plan['item_part']), _ptr(plan['item_ptr']), _ptr(A.indptr), _ptr(A.indices), seed, epoch,
                _ptr(out)), entry)
        return out

    @staticmethod
    def _rank_of_columns(what, P, max_rank):
        """k of a block of k + 1 columns (the pairwise sweeps' [P | 1]), in range under the model's name `what`"""
        k = int(P.shape[1]) - 1
        if k < 1 or k > max_rank:
            raise ValueError('%s: rank %d outside 1..%d' % (what, k, max_rank))
        return k

    def bpr_draw_negatives(self, plan, seed, epoch):
        """int32 [nnz] (device): the negative of every position of the plan's schedule, -1 where all PK_BPR_DRAWS draws were
        seen items (pk_bpr_draw_negatives; the stream is spelled out in include/polara_hip.h)."""
        return self._pair_draw('BPR', 'bpr_draw_negatives', 'pk_bpr_draw_negatives', self._bpr_check_plan(plan), plan, seed, epoch)

    def bpr_epoch(self, plan, neg, P, Q, learning_rate, regularization):
        """One LearnBPR sweep over the plan's positives with the negatives `neg` (pk_bpr_epoch_f64: one launch per stratum and
        one for the counters), P [n_users x (k + 1)] (column k: the constant 1) and Q [n_items x (k + 1)] (column k: the bias)
        updated in place.  Returns a device tensor of three int64: trained, skipped, correct."""
        n_users, n_items = plan['shape']
        k = self._rank_of_columns('BPR', P, self.bpr_max_rank())
        self._check_row_blocks('BPR', (P, Q), (n_users, n_items), k + 1)
        B = self._bpr_check_plan(plan)
        if neg.dtype != torch.int32 or neg.dim() != 1 or neg.numel() != plan['nnz'] or (neg.numel() and neg.stride(0) != 1):
            raise ValueError('BPR: the negatives must be int32 [%d] (bpr_draw_negatives)' % plan['nnz'])
        work = self._work(self.lib.pk_bpr_work_bytes(B))              # the counters of every block
        out = torch.empty(3, dtype=torch.int64, device=self.device)
        with self._timed('bpr_epoch', (plan['nnz'], k, B)):
            _lib.check(self.lib.pk_bpr_epoch_f64(self.stream(), B, k, int(plan['nnz']), _ptr(plan['block_ptr']), _ptr(plan['users']),
                                                 _ptr(plan['items']), _ptr(neg), _ptr(P), P.stride(0), _ptr(Q), Q.stride(0),
                                                 float(learning_rate), float(regularization), _ptr(work), _ptr(out)),
                       'pk_bpr_epoch_f64')
        return out

    def bpr_sigmoid(self, x):
        """1 / (1 + exp(x)) elementwise by the sweep's own sequence of IEEE operations (pk_bpr_sigmoid_f64)"""
        if x.dtype != torch.float64 or not x.is_contiguous():
            raise ValueError('BPR: the sigmoid takes a contiguous fp64 tensor')
        out = torch.empty_like(x)
        _lib.check(self.lib.pk_bpr_sigmoid_f64(self.stream(), x.numel(), _ptr(x), _ptr(out)), 'pk_bpr_sigmoid_f64')
        return out

    # ---- LightFM with the WARP loss (csrc/warp.hip) ----------------------------------------------------------------------
    def warp_max_rank(self):
        return int(self.lib.pk_warp_max_rank())

    def warp_plan(self, A, blocks, item_order=None, features=None):
        """bpr_plan(A, blocks, item_order) plus plan['features']: None, or for a SciPy one-hot matrix `features` [n_items x
        n_labels] a dict on the device — a (fp64 [n_items]: 1 / (1 + labels of the item)), F_lab = diag(a) one_hot as CSR
        (row_ptr int64, row_idx int32, row_val fp64) and as CSC (col_ptr, col_idx: items ascending, col_val), n_labels."""
        from . import warp
        plan = self.bpr_plan(A, blocks, item_order)
        plan['features'] = None
        if features is not None:
            n_items = plan['shape'][1]
            if int(features.shape[0]) != n_items:
                raise ValueError('LightFM: features for %d items, the training matrix has %d' % (features.shape[0], n_items))
            a, F = warp.feature_weights(features)
            Fc = F.tocsc()
            Fc.sort_indices()
            up = lambda x, dt: self.to_device(np.ascontiguousarray(x, dtype=dt))
            plan['features'] = dict(n_labels=int(F.shape[1]), a=up(a, np.float64), row_ptr=up(F.indptr, np.int64),
                                    row_idx=up(F.indices, np.int32), row_val=up(F.data, np.float64), col_ptr=up(Fc.indptr, np.int64),
                                    col_idx=up(Fc.indices, np.int32), col_val=up(Fc.data, np.float64))
        return plan

    def _warp_check_plan(self, plan):
        B = self._bpr_check_plan(plan)
        f = plan.get('features', None)
        if f is not None:
            n_items = plan['shape'][1]
            if (f['a'].numel() != n_items or f['row_ptr'].numel() != n_items + 1 or f['col_ptr'].numel() != f['n_labels'] + 1
                    or f['row_idx'].numel() != f['row_val'].numel() or f['col_idx'].numel() != f['row_idx'].numel()
                    or f['col_val'].numel() != f['row_idx'].numel()):
                raise ValueError('LightFM: not a plan of warp_plan (item features)')
        return B, f

    def warp_draw(self, plan, seed, epoch, max_sampled):
        """int32 [nnz x max_sampled] (device): the candidates of every position of the plan's schedule, -1 where the draw is an
        item of the user's row (pk_warp_draw_candidates; the stream is spelled out in include/polara_hip.h)."""
        B, _ = self._warp_check_plan(plan)
        D = int(max_sampled)
        if D < 1 or D > _lib.PK_WARP_MAX_SAMPLED:
            raise ValueError('LightFM: max_sampled %d outside 1..%d' % (D, _lib.PK_WARP_MAX_SAMPLED))
        return self._pair_draw('LightFM', 'warp_draw', 'pk_warp_draw_candidates', B, plan, seed, epoch, (D,))

    def warp_label_image(self, plan, L):
        """S = F_lab L [n_items x (k + 1)] in the storage-order sum of the sweep (pk_warp_label_image_f64)"""
        _, f = self._warp_check_plan(plan)
        if f is None:
            raise ValueError('LightFM: the plan has no item features')
        n_items = plan['shape'][1]
        k = int(L.shape[1]) - 1
        self._check_row_blocks('LightFM', (L,), (f['n_labels'],), k + 1)
        S = self.empty(n_items, k + 1)
        _lib.check(self.lib.pk_warp_label_image_f64(self.stream(), k, n_items, f['n_labels'], _ptr(f['row_ptr']), _ptr(f['row_idx']),
                                                    _ptr(f['row_val']), _ptr(L), L.stride(0), _ptr(S), S.stride(0)),
                   'pk_warp_label_image_f64')
        return S

    def warp_representation(self, plan, E, L=None):
        """Q = a o E_id + F_lab E_lab (a copy of E_id without item features): every product and sum rounded on its own"""
        if plan.get('features', None) is None:
            return E.clone()
        return E * plan['features']['a'][:, None] + self.warp_label_image(plan, L)

    def warp_epoch(self, plan, cand, table, P, E, state, learning_rate, L=None, work=None):
        """One WARP sweep over the plan's positives with the candidates `cand` and the loss table `table` (host, fp64
        [max_sampled]) — pk_warp_epoch_f64: per stratum the sweep's launch and, with item features, one before it (the label
        image) and one after (the label step); then the counters.  P [n_users x (k + 1)] (column k: the constant 1), E
        [n_items x (k + 1)] and, with features, L [n_labels x (k + 1)] are updated in place, and so is state = (AP, AE, AL),
        their adagrad state (AL None without features).  work = (S, G), two [n_items x (k + 1)] blocks (allocated here when
        None; G is zero when the epoch ends).  Returns a device tensor of three int64: trained, quiet, draws."""
        n_users, n_items = plan['shape']
        k = self._rank_of_columns('LightFM', P, self.warp_max_rank())
        B, f = self._warp_check_plan(plan)
        if len(state) != 3:
            raise ValueError('LightFM: state = (AP, AE, AL)')
        AP, AE, AL = state
        self._check_row_blocks('LightFM', (P, E, AP, AE), (n_users, n_items), k + 1)
        nnz = int(plan['nnz'])
        if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != nnz or not cand.is_contiguous():
            raise ValueError('LightFM: the candidates must be int32 [%d x max_sampled] (warp_draw)' % nnz)
        D = int(cand.shape[1])
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.shape != (D,) or D < 1 or D > _lib.PK_WARP_MAX_SAMPLED:
            raise ValueError('LightFM: a loss table of shape %s for %d candidates per positive (1..%d)'
                             % (table.shape, D, _lib.PK_WARP_MAX_SAMPLED))
        table_dev = self.to_device(table)
        n_labels, S, G = 0, None, None
        names = ('a', 'row_ptr', 'row_idx', 'row_val', 'col_ptr', 'col_idx', 'col_val')
        if f is not None:
            n_labels = f['n_labels']
            if L is None or AL is None:
                raise ValueError('LightFM: item features need the label embeddings L and their state AL')
            self._check_row_blocks('LightFM', (L, AL), (n_labels,), k + 1)
            S, G = work if work is not None else (self.empty(n_items, k + 1), self.empty(n_items, k + 1))
            self._check_row_blocks('LightFM', (S, G), (n_items,), k + 1)
            feats = [_ptr(f[name]) for name in names]
        else:
            if L is not None:
                raise ValueError('LightFM: label embeddings without item features in the plan')
            L = AL = None
            feats = [None] * len(names)
        ld = lambda X: X.stride(0) if X is not None else 0
        counters = self._work(self.lib.pk_warp_work_bytes(B))         # the counters of every block
        out = torch.empty(3, dtype=torch.int64, device=self.device)
        with self._timed('warp_epoch', (nnz, k, B, D, n_labels)):
            _lib.check(self.lib.pk_warp_epoch_f64(self.stream(), B, k, nnz, n_items, n_labels, D, _ptr(plan['block_ptr']),
                                                  _ptr(plan['users']), _ptr(plan['items']), _ptr(cand), _ptr(table_dev), _ptr(P),
                                                  P.stride(0), _ptr(E), E.stride(0), _ptr(AP), AP.stride(0), _ptr(AE), AE.stride(0),
                                                  float(learning_rate), *feats, _ptr(L), ld(L), _ptr(AL), ld(AL), _ptr(S), ld(S),
                                                  _ptr(G), ld(G), _ptr(counters), _ptr(out)), 'pk_warp_epoch_f64')
        return out

    def warp_label_step(self, plan, G, L, AL, learning_rate):
        """The label step alone (pk_warp_label_step_f64): every label's gradient summed from G over its items in ascending
        order, one adagrad step on L with the state AL, and G cleared — all in place."""
        _, f = self._warp_check_plan(plan)
        if f is None:
            raise ValueError('LightFM: the plan has no item features')
        n_items = plan['shape'][1]
        k = int(L.shape[1]) - 1
        self._check_row_blocks('LightFM', (G,), (n_items,), k + 1)
        self._check_row_blocks('LightFM', (L, AL), (f['n_labels'],), k + 1)
        _lib.check(self.lib.pk_warp_label_step_f64(self.stream(), k, n_items, f['n_labels'], _ptr(f['col_ptr']), _ptr(f['col_idx']),
                                                   _ptr(f['col_val']), _ptr(G), G.stride(0), _ptr(L), L.stride(0), _ptr(AL),
                                                   AL.stride(0), float(learning_rate)), 'pk_warp_label_step_f64')

    # ---- Factorisation model with side features (csrc/fm.hip) -----------------------------------------------------------
    _FM_FEATURE_KEYS = ('a', 'row_ptr', 'row_idx', 'row_val', 'col_ptr', 'col_idx', 'col_val')

    def fm_max_rank(self):
        return int(self.lib.pk_fm_max_rank())

    def fm_plan(self, A, blocks, user_features=None, item_features=None, normalize=False):
        """pmf_plan(A, blocks) plus plan['features'] = {'user': .., 'item': ..}: per side None, or for a SciPy one-hot matrix
        [n_rows x n_labels] a dict on the device in warp_plan's layout — a (fp64 [n_rows]), F = diag(a) one_hot as CSR (row_ptr
        int64, row_idx int32, row_val fp64) and as CSC (col_ptr, col_idx: rows ascending, col_val), n_labels.  a = 1 unless
        `normalize`, which gives LightFM's 1 / (1 + labels of the row) (fm.side_features)."""
        from . import fm
        plan = self.pmf_plan(A, blocks)
        plan['features'] = {}
        for side, features, n in (('user', user_features, plan['shape'][0]), ('item', item_features, plan['shape'][1])):
            plan['features'][side] = None
            if features is None:
                continue
            if int(features.shape[0]) != n:
                raise ValueError('TCF: features for %d %ss, the training matrix has %d' % (features.shape[0], side, n))
            a, F = fm.side_features(features, normalize)
            Fc = F.tocsc()
            Fc.sort_indices()
            up = lambda x, dt: self.to_device(np.ascontiguousarray(x, dtype=dt))
            plan['features'][side] = dict(n_labels=int(F.shape[1]), a=up(a, np.float64), row_ptr=up(F.indptr, np.int64),
                                          row_idx=up(F.indices, np.int32), row_val=up(F.data, np.float64),
                                          col_ptr=up(Fc.indptr, np.int64), col_idx=up(Fc.indices, np.int32),
                                          col_val=up(Fc.data, np.float64))
        return plan

    def _fm_check_plan(self, plan):
        """(B, user features, item features) of a plan of fm_plan"""
        B = self._check_plan(plan, 'PMF', users=('row_nnz',), items=('col_nnz',), entries=('users', 'vals'))
        sides = plan.get('features', None)
        if not isinstance(sides, dict) or set(sides) != {'user', 'item'}:
            raise ValueError('TCF: not a plan of fm_plan')
        for f, n in zip((sides['user'], sides['item']), plan['shape']):
            if f is not None and (f['a'].numel() != n or f['row_ptr'].numel() != n + 1 or f['col_ptr'].numel() != f['n_labels'] + 1
                                  or f['row_idx'].numel() != f['row_val'].numel() or f['col_idx'].numel() != f['row_idx'].numel()
                                  or f['col_val'].numel() != f['row_idx'].numel()):
                raise ValueError('TCF: not a plan of fm_plan (features)')
        return B, sides['user'], sides['item']

    def _fm_side(self, plan, side):
        _, fu, fi = self._fm_check_plan(plan)
        if side not in ('user', 'item'):
            raise ValueError('TCF: side %r (\'user\' or \'item\')' % (side,))
        f = fu if side == 'user' else fi
        if f is None:
            raise ValueError('TCF: the plan has no %s features' % side)
        return f, plan['shape'][0 if side == 'user' else 1]

    def _fm_rank(self, X):
        k = int(X.shape[1]) - 2
        if k < 1 or k > self.fm_max_rank():
            raise ValueError('TCF: rank %d outside 1..%d' % (k, self.fm_max_rank()))
        return k

    def fm_label_image(self, plan, side, L):
        """S = F L [n_rows x (k + 2)] of one side ('user' / 'item') in the storage-order sum of the sweep (pk_fm_label_image_f64)"""
        f, n = self._fm_side(plan, side)
        k = self._fm_rank(L)
        self._check_row_blocks('TCF', (L,), (f['n_labels'],), k + 2)
        S = self.empty(n, k + 2)
        _lib.check(self.lib.pk_fm_label_image_f64(self.stream(), k, n, f['n_labels'], _ptr(f['row_ptr']), _ptr(f['row_idx']),
                                                  _ptr(f['row_val']), _ptr(L), L.stride(0), _ptr(S), S.stride(0)),
                   'pk_fm_label_image_f64')
        return S

    def fm_representation(self, plan, side, X, L=None):
        """a o X + F L of one side (a copy of X without features on it): every product and sum rounded on its own"""
        _, fu, fi = self._fm_check_plan(plan)
        f = fu if side == 'user' else fi
        if f is None:
            return X.clone()
        return X * f['a'][:, None] + self.fm_label_image(plan, side, L)

    def fm_label_step(self, plan, side, G, L, SL, step, reg, lin_reg, adjust=None, gamma=0.9, label_factors=True, smoothing=1e-6):
        """The label step of one side alone (pk_fm_label_step_f64): every label's gradient and sample count summed from G
        [n_rows x (k + 3)] over its rows in ascending order, one adjusted step on L with the state SL (None without adjuster),
        and G cleared — all in place."""
        f, n = self._fm_side(plan, side)
        k = self._fm_rank(L)
        if adjust not in self._PMF_ADJUST:
            raise ValueError('TCF: unknown gradient adjustment %r' % (adjust,))
        self._check_row_blocks('TCF', (G,), (n,), k + 3)
        self._check_row_blocks('TCF', (L,) + ((SL,) if adjust else ()), (f['n_labels'],), k + 2)
        _lib.check(self.lib.pk_fm_label_step_f64(self.stream(), k, int(side == 'item'), int(bool(label_factors)), n, f['n_labels'],
                                                 _ptr(f['col_ptr']), _ptr(f['col_idx']), _ptr(f['col_val']), _ptr(G), G.stride(0),
                                                 _ptr(L), L.stride(0), _ptr(SL) if adjust else None, SL.stride(0) if adjust else 0,
                                                 float(step), float(reg), float(lin_reg), self._PMF_ADJUST[adjust], float(gamma),
                                                 float(smoothing)), 'pk_fm_label_step_f64')

    def fm_epoch(self, plan, mean, P, E, LU, LI, state, step, reg, lin_reg, adjust=None, gamma=0.9, work=None, label_factors=True,
                 smoothing=1e-6):
        """One sweep over the plan's ratings (pk_fm_epoch_f64: per stratum the sweep's launch and, per side with features, one
        before it (the label image) and one after (the label step); then the squared error).  P [n_users x (k + 2)], E [n_items
        x (k + 2)] and, per side with features, LU / LI [n_labels x (k + 2)] (None otherwise) are updated in place, and so is
        state = (SP, SE, SLU, SLI), the adjuster's state of the four blocks (None without adjuster; None for a side without
        features).  work = (SU, GU, SI, GI): the images [n x (k + 2)] and the gradient rows [n x (k + 3)] (allocated here when
        None; G is zero when the epoch ends).  Returns a device tensor of one double: the epoch's squared error."""
        n_users, n_items = plan['shape']
        k = self._fm_rank(P)
        B, fu, fi = self._fm_check_plan(plan)
        if adjust not in self._PMF_ADJUST:
            raise ValueError('TCF: unknown gradient adjustment %r' % (adjust,))
        if adjust and (state is None or len(state) != 4):
            raise ValueError('TCF: the gradient adjustment %r needs state = (SP, SE, SLU, SLI)' % (adjust,))
        SP, SE, SLU, SLI = state if adjust else (None,) * 4
        self._check_row_blocks('TCF', (P, E) + ((SP, SE) if adjust else ()), (n_users, n_items), k + 2)
        if work is not None and len(work) != 4:
            raise ValueError('TCF: work = (SU, GU, SI, GI)')
        ld = lambda X: X.stride(0) if X is not None else 0
        sides = []
        for side, f, n, L, SL, buffers in (('user', fu, n_users, LU, SLU, None if work is None else work[:2]),
                                           ('item', fi, n_items, LI, SLI, None if work is None else work[2:])):
            if f is None:
                if L is not None:
                    raise ValueError('TCF: %s label embeddings without %s features in the plan' % (side, side))
                sides += [0] + [None] * len(self._FM_FEATURE_KEYS) + [None, 0, None, 0, None, 0, None, 0]
                continue
            if L is None or (adjust and SL is None):
                raise ValueError('TCF: %s features need the label embeddings and, with an adjuster, their state' % side)
            self._check_row_blocks('TCF', (L,) + ((SL,) if adjust else ()), (f['n_labels'],), k + 2)
            S, G = buffers if buffers is not None else (self.empty(n, k + 2), self.empty(n, k + 3))
            self._check_row_blocks('TCF', (S,), (n,), k + 2)
            self._check_row_blocks('TCF', (G,), (n,), k + 3)
            if not adjust:
                SL = None
            sides += [f['n_labels']] + [_ptr(f[name]) for name in self._FM_FEATURE_KEYS]
            sides += [_ptr(L), ld(L), _ptr(SL), ld(SL), _ptr(S), ld(S), _ptr(G), ld(G)]
        nnz = int(plan['nnz'])
        sse_work = self.empty(int(self.lib.pk_pmf_work_doubles(B)))      # the block sums of the squared error
        out = self.empty(1)
        with self._timed('fm_epoch', (nnz, k, B, 0 if fu is None else fu['n_labels'], 0 if fi is None else fi['n_labels'])):
            _lib.check(self.lib.pk_fm_epoch_f64(
                self.stream(), B, k, nnz, n_users, n_items, _ptr(plan['block_ptr']), _ptr(plan['users']), _ptr(plan['items']),
                _ptr(plan['vals']), float(mean), _ptr(P), P.stride(0), _ptr(E), E.stride(0), float(step), float(reg), float(lin_reg),
                self._PMF_ADJUST[adjust], _ptr(SP), ld(SP), _ptr(SE), ld(SE), float(gamma), float(smoothing),
                int(bool(label_factors)), *sides, _ptr(sse_work), _ptr(out)), 'pk_fm_epoch_f64')
        return out

    # ---- Implicit ALS (csrc/ials.hip) ----------------------------------------------------------------------------------
    def ials_max_rank(self):
        return int(self.lib.pk_ials_max_rank())

    def csr_values_host(self, A):
        """the stored values of a DeviceCSR as a host fp64 array (storage order)"""
        return self.to_host(A.values.to(torch.float64))

    def csr_replace_values(self, A, values, drop_zeros=False):
        """The DeviceCSR `A` with the host fp64 array `values` in place of its stored values (same pattern and plans);
        drop_zeros: entries whose new value is exactly 0 leave the pattern (a new matrix when there are any)."""
        values = np.ascontiguousarray(values, dtype=np.float64)
        if values.shape != (int(A.indices.numel()),):
            raise ValueError('csr_replace_values: %s values for %d stored entries' % (values.shape, A.indices.numel()))
        keep = values != 0 if drop_zeros else None
        if keep is None or keep.all():
            new = A.with_columns(A.indices, self.to_device(values))
            new.val_kind = _lib.PK_VAL_F64
            return new
        csum = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))
        indptr = csum[self.to_host(A.indptr)]
        keep_dev = self.to_device(keep)
        new = DeviceCSR.from_device(self, self.to_device(indptr), A.indices[keep_dev].contiguous(), self.to_device(values[keep]),
                                    A.shape, A.split)
        new._nnz = int(csum[-1])
        new.sorted_cols = A.sorted_cols
        return new

    def _ials_row_order(self, Cm):
        """int32 [n_rows] on the device: the rows of `Cm` by descending length, ties by row (the library's stable radix sort);
        kept on the matrix"""
        order = getattr(Cm, '_ials_order', None)
        if order is None:
            n = int(Cm.shape[0])
            lengths = (Cm.indptr[1:n + 1] - Cm.indptr[:n]).to(torch.int32)
            longest = int(lengths.max().item()) if n else 0
            keys = (longest - lengths).contiguous()
            pos = torch.arange(max(n, 1), dtype=torch.int32, device=self.device)[:n].contiguous()
            if n > 1 and longest > 0:
                keys_tmp, pos_tmp = torch.empty_like(keys), torch.empty_like(pos)
                in_tmp = C.c_int32(0)
                work = self._work(self.lib.pk_radix_work_bytes(n))
                _lib.check(self.lib.pk_radix_sort_pairs(self.stream(), n, 4, _ptr(keys), _ptr(pos), _ptr(keys_tmp), _ptr(pos_tmp),
                                                        max(1, longest.bit_length()), _ptr(work), C.byref(in_tmp)),
                           'pk_radix_sort_pairs')
                pos = pos_tmp if in_tmp.value else pos
            order = Cm._ials_order = pos
        return order

    def _ials_check(self, Cm, X, Y, what):
        k = int(Y.shape[1])
        if k < 1 or k > self.ials_max_rank():
            raise ValueError('iALS: rank %d outside 1..%d' % (k, self.ials_max_rank()))
        for M, n in ((X, Cm.shape[0]), (Y, Cm.shape[1])):
            if M is not None and (M.dtype != torch.float64 or M.dim() != 2 or tuple(M.shape) != (n, k) or M.stride(1) != 1
                                  or M.stride(0) < k):
                raise ValueError('iALS %s: a block of shape %s, strides %s for [%d x %d] fp64 rows'
                                 % (what, tuple(M.shape), M.stride(), n, k))
        return k

    def ials_half_step(self, Cm, Y, regularization, out=None, G=None, row_order=None):
        """One half-step of the alternating least squares (pk_ials_half_step_f64): for every row u of the DeviceCSR of
        confidences `Cm` [n_rows x n_cols], x_u = (G + lambda I + sum_i (c_ui - 1) y_i y_i^T)^-1 sum_i c_ui y_i against the
        fixed block Y [n_cols x k].  G = Y^T Y (computed by `gram` when None).  Returns X [n_rows x k] (`out` when given: a
        view with a leading dimension is fine).  A row whose matrix is not positive definite raises a ValueError naming
        how many there are and the first; their rows of X hold zeros.  row_order: int32 device permutation of the rows
        (None: by descending length) — it changes which workgroup starts when, never a bit of the result."""
        n_rows, n_cols = Cm.shape
        k = self._ials_check(Cm, out, Y, 'half-step')
        if G is None:
            G = self.gram(Y)
        if G.dtype != torch.float64 or tuple(G.shape) != (k, k) or G.stride(1) != 1:
            raise ValueError('iALS half-step: G of shape %s for rank %d' % (tuple(G.shape), k))
        X = self.empty(n_rows, k) if out is None else out
        conf = Cm.values if Cm.values.dtype == torch.float64 else Cm.values.to(torch.float64)
        order = self._ials_row_order(Cm) if row_order is None else row_order
        if order.dtype != torch.int32 or order.numel() != n_rows or not order.is_contiguous():
            raise ValueError('iALS half-step: row_order must be a contiguous int32 permutation of the %d rows' % n_rows)
        info = torch.empty(2, dtype=torch.int32, device=self.device)
        work = self._work(self.lib.pk_ials_work_bytes(n_rows, k))
        with self._timed('ials_half_step', (n_rows, n_cols, int(Cm.indices.numel()), k)):
            _lib.check(self.lib.pk_ials_half_step_f64(self.stream(), n_rows, n_cols, k, _ptr(Cm.indptr), _ptr(Cm.indices), _ptr(conf),
                                                      _ptr(order), _ptr(Y), Y.stride(0), _ptr(G), G.stride(0), float(regularization),
                                                      _ptr(X), X.stride(0), _ptr(info), _ptr(work)), 'pk_ials_half_step_f64')
        bad, first = (int(v) for v in info.tolist())
        if bad:
            raise ValueError('iALS half-step: %d row(s) whose normal equations are not positive definite, the first is row %d '
                             '(their factors are set to zero)' % (bad, first))
        return X

    def ials_loss(self, Cm, X, Y, regularization, GX=None, GY=None):
        """The objective  sum over ALL pairs of w (p - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2)  (w = c, p = 1 on the stored
        entries of `Cm`; w = 1, p = 0 elsewhere) as a float:  tr(X^T X Y^T Y) + the sparse term (pk_ials_loss_nz_f64) +
        lambda (tr X^T X + tr Y^T Y).  GX / GY: the Gram matrices when the caller has them."""
        n_rows, n_cols = Cm.shape
        k = self._ials_check(Cm, X, Y, 'loss')
        GX = self.gram(X) if GX is None else GX
        GY = self.gram(Y) if GY is None else GY
        conf = Cm.values if Cm.values.dtype == torch.float64 else Cm.values.to(torch.float64)
        out = self.empty(1)
        work = self._work(self.lib.pk_ials_work_bytes(n_rows, k))
        with self._timed('ials_loss', (n_rows, n_cols, int(Cm.indices.numel()), k)):
            _lib.check(self.lib.pk_ials_loss_nz_f64(self.stream(), n_rows, n_cols, k, _ptr(Cm.indptr), _ptr(Cm.indices), _ptr(conf),
                                                    _ptr(X), X.stride(0), _ptr(Y), Y.stride(0), _ptr(out), _ptr(work)),
                       'pk_ials_loss_nz_f64')
        gx, gy = self.to_host(GX), self.to_host(GY)
        return float((gx * gy).sum() + float(out[0].item()) + float(regularization) * (np.trace(gx) + np.trace(gy)))

    # ---- iALS++ (csrc/ialspp.hip) ---------------------------------------------------------------------------------------
    def ialspp_max_rank(self):
        return int(self.lib.pk_ialspp_max_rank())

    def ialspp_block_sizes(self):
        return (16, 32, 64)

    def _ialspp_check(self, Cm, X, Y, what, E=None):
        k = int(Y.shape[1])
        if k < 1 or k > self.ialspp_max_rank():
            raise ValueError('iALS++: rank %d outside 1..%d' % (k, self.ialspp_max_rank()))
        for M, n in ((X, Cm.shape[0]), (Y, Cm.shape[1])):
            if M is not None and (M.dtype != torch.float64 or M.dim() != 2 or tuple(M.shape) != (n, k) or M.stride(1) != 1
                                  or M.stride(0) < k):
                raise ValueError('iALS++ %s: a block of shape %s, strides %s for [%d x %d] fp64 rows'
                                 % (what, tuple(M.shape), M.stride(), n, k))
        nnz = int(Cm.indices.numel())
        if E is not None and (E.dtype != torch.float64 or tuple(E.shape) != (nnz,) or not E.is_contiguous()):
            raise ValueError('iALS++ %s: predictions of shape %s for %d stored entries (contiguous fp64)' % (what, tuple(E.shape), nnz))
        return k

    def ialspp_predict(self, Cm, X, Y, out=None):
        """E [nnz] fp64 in the storage order of the DeviceCSR `Cm`: e = x_u . y_i for every stored entry (u, i)
        (pk_ialspp_predict_f64).  X [n_rows x k], Y [n_cols x k]; views with a leading dimension are fine."""
        n_rows, n_cols = Cm.shape
        E = self.empty(int(Cm.indices.numel())) if out is None else out
        k = self._ialspp_check(Cm, X, Y, 'predict', E)
        with self._timed('ialspp_predict', (n_rows, n_cols, int(Cm.indices.numel()), k)):
            _lib.check(self.lib.pk_ialspp_predict_f64(self.stream(), n_rows, n_cols, k, _ptr(Cm.indptr), _ptr(Cm.indices), _ptr(X),
                                                      X.stride(0), _ptr(Y), Y.stride(0), _ptr(E)), 'pk_ialspp_predict_f64')
        return E

    def _ialspp_regularization(self, regularization, n_rows):
        """(scalar, device vector or None) of a float or a device fp64 vector [n_rows]"""
        if isinstance(regularization, torch.Tensor):
            if regularization.dtype != torch.float64 or tuple(regularization.shape) != (n_rows,) or not regularization.is_contiguous():
                raise ValueError('iALS++: per-row regularization of shape %s for %d rows (contiguous fp64)'
                                 % (tuple(regularization.shape), n_rows))
            return 0.0, regularization
        return float(regularization), None

    def ialspp_block_step(self, Cm, Y, X, E, G, p0, block_size, regularization, R=None, row_order=None):
        """One block step of iALS++ (pk_ialspp_block_step_f64), IN PLACE on X [n_rows x k] and on the cached predictions E
        [nnz]: for every row u of the DeviceCSR of confidences `Cm`, with pi = [p0, min(p0 + block_size, k)),
            g = G[pi,:] x_u + lambda_u x_pi + sum_i ((c_i - 1) e_i - c_i) y_{i,pi},   H = G[pi,pi] + lambda_u I + sum_i (c_i - 1) y_{i,pi} y_{i,pi}^T
            delta = H^-1 g,   x_pi -= delta,   e_i -= y_{i,pi} . delta
        against the fixed block Y [n_cols x k], G = Y^T Y.  regularization: a float, or a device fp64 vector of one value per
        row.  R [n_rows x |pi|] = X G[:,pi] (formed here by `tsmm` when None; it must belong to the X the step starts from).
        A row whose H is not positive definite raises a ValueError naming how many there are and the first; x_pi and e of
        those rows are left as they were.  row_order as in `ials_half_step`: never a bit of the result."""
        n_rows, n_cols = Cm.shape
        k = self._ialspp_check(Cm, X, Y, 'block step', E)
        p0, block_size = int(p0), int(block_size)
        if block_size not in self.ialspp_block_sizes():
            raise ValueError('iALS++ block step: block size %d is not one of %s' % (block_size, self.ialspp_block_sizes()))
        if p0 < 0 or p0 >= k:
            raise ValueError('iALS++ block step: block start %d outside the rank %d' % (p0, k))
        p1 = min(p0 + block_size, k)
        if G.dtype != torch.float64 or tuple(G.shape) != (k, k) or G.stride(1) != 1:
            raise ValueError('iALS++ block step: G of shape %s for rank %d' % (tuple(G.shape), k))
        lam, lam_rows = self._ialspp_regularization(regularization, n_rows)
        if R is None:
            R = self.tsmm(X, G[:, p0:p1]) if n_rows else self.empty(0, p1 - p0)
        if R.dtype != torch.float64 or tuple(R.shape) != (n_rows, p1 - p0) or R.stride(1) != 1 or (n_rows and R.stride(0) < p1 - p0):
            raise ValueError('iALS++ block step: R of shape %s, strides %s for [%d x %d] fp64 rows'
                             % (tuple(R.shape), R.stride(), n_rows, p1 - p0))
        conf = Cm.values if Cm.values.dtype == torch.float64 else Cm.values.to(torch.float64)
        order = self._ials_row_order(Cm) if row_order is None else row_order
        if order.dtype != torch.int32 or order.numel() != n_rows or not order.is_contiguous():
            raise ValueError('iALS++ block step: row_order must be a contiguous int32 permutation of the %d rows' % n_rows)
        info = torch.empty(2, dtype=torch.int32, device=self.device)
        work = self._work(self.lib.pk_ialspp_work_bytes(n_rows, block_size))
        with self._timed('ialspp_block_step', (n_rows, n_cols, int(Cm.indices.numel()), k, block_size)):
            _lib.check(self.lib.pk_ialspp_block_step_f64(self.stream(), n_rows, n_cols, k, p0, block_size, _ptr(Cm.indptr),
                                                         _ptr(Cm.indices), _ptr(conf), _ptr(order), _ptr(Y), Y.stride(0), _ptr(G),
                                                         G.stride(0), lam, _ptr(lam_rows), _ptr(R), max(R.stride(0), p1 - p0),
                                                         _ptr(X), X.stride(0), _ptr(E), _ptr(info), _ptr(work)),
                       'pk_ialspp_block_step_f64')
        bad, first = (int(v) for v in info.tolist())
        if bad:
            raise ValueError('iALS++ block step: %d row(s) whose block system is not positive definite, the first is row %d '
                             '(their factors are left unchanged)' % (bad, first))
        return X

    def ialspp_half_sweep(self, Cm, Y, X, G, regularization, block_size, E=None):
        """One half-sweep of iALS++ in place on X: the predictions of X and Y (into `E` when given), then the block steps
        over [0, d), [d, 2 d), .. in ascending order.  Returns (X, E)."""
        E = self.ialspp_predict(Cm, X, Y, out=E)
        for p0 in range(0, int(Y.shape[1]), int(block_size)):
            self.ialspp_block_step(Cm, Y, X, E, G, p0, block_size, regularization)
        return X, E

    def ialspp_loss(self, Cm, X, Y, reg_rows, reg_cols, GX=None, GY=None):
        """The objective of iALS++ as a float:  sum over ALL pairs of w (p - x_u . y_i)^2 + sum_u reg_rows[u] |x_u|^2 +
        sum_i reg_cols[i] |y_i|^2  (reg_rows / reg_cols: floats or device fp64 vectors) =  tr(X^T X Y^T Y) + the sparse term
        + the regularisation.  The sparse term is pk_ials_loss_nz_f64's up to its rank; above it, it is summed from the
        predictions (pk_ialspp_predict_f64) and the confidences."""
        n_rows, n_cols = Cm.shape
        k = self._ialspp_check(Cm, X, Y, 'loss')
        GX = self.gram(X) if GX is None else GX
        GY = self.gram(Y) if GY is None else GY
        conf = Cm.values if Cm.values.dtype == torch.float64 else Cm.values.to(torch.float64)
        if k <= self.ials_max_rank():
            out = self.empty(1)
            work = self._work(self.lib.pk_ials_work_bytes(n_rows, k))
            _lib.check(self.lib.pk_ials_loss_nz_f64(self.stream(), n_rows, n_cols, k, _ptr(Cm.indptr), _ptr(Cm.indices), _ptr(conf),
                                                    _ptr(X), X.stride(0), _ptr(Y), Y.stride(0), _ptr(out), _ptr(work)),
                       'pk_ials_loss_nz_f64')
            sparse = float(out[0].item())
        else:
            s = self.ialspp_predict(Cm, X, Y)
            sparse = float((conf * (1.0 - s) ** 2 - s * s).sum().item())
        reg = 0.0
        for lam, M, Gm, n in ((reg_rows, X, GX, n_rows), (reg_cols, Y, GY, n_cols)):
            lam, lam_rows = self._ialspp_regularization(lam, n)
            reg += float(lam * torch.trace(Gm).item()) if lam_rows is None else float((lam_rows * (M * M).sum(dim=1)).sum().item())
        return float((self.to_host(GX) * self.to_host(GY)).sum() + sparse + reg)

    # ---- Logistic matrix factorisation (csrc/lmf.hip) --------------------------------------------------------------------
    def lmf_max_rank(self):
        return int(self.lib.pk_lmf_max_rank())

    def lmf_plan(self, Cm, neg_prop):
        """What a half-step over the rows of the DeviceCSR of confidences `Cm` [n_rows x n_cols] needs beside the matrix, made
        once and kept on the matrix (as `Cm.T` is): a dict with row_order (int32 [n_rows]: longest rows first, the iALS order),
        neg_ptr (int64 [n_rows + 1]: the exclusive prefix sum of m = min(n_cols, n * neg_prop) over the rows), negatives (their
        total: the negatives of one half-step), neg_prop, matrix, shape."""
        neg_prop = int(neg_prop)
        if neg_prop < 1 or neg_prop >= 2 ** 31:
            raise ValueError('LMF: neg_prop %d < 1' % neg_prop)
        plans = Cm.__dict__.setdefault('_lmf_plans', {})
        plan = plans.get(neg_prop)
        if plan is None:
            n_rows, n_cols = (int(x) for x in Cm.shape)
            with self._timed('lmf_plan', (n_rows, n_cols, int(Cm.indices.numel()), neg_prop)):
                lengths = Cm.indptr[1:n_rows + 1] - Cm.indptr[:n_rows]
                neg_ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=self.device)
                neg_ptr[1:] = torch.cumsum(torch.clamp(lengths * neg_prop, max=n_cols), 0)
                plan = plans[neg_prop] = dict(row_order=self._ials_row_order(Cm), neg_ptr=neg_ptr, negatives=int(neg_ptr[-1].item()),
                                              neg_prop=neg_prop, matrix=Cm, shape=(n_rows, n_cols))
        return plan

    @staticmethod
    def _lmf_stream(seed, round):
        seed, round = int(seed), int(round)
        if not (0 <= seed < 2 ** 32 and 0 <= round < 2 ** 32):
            raise ValueError('LMF: seed %d and round %d must fit 32 unsigned bits' % (seed, round))
        return seed, round

    def lmf_half_step(self, plan, Y, X, A, lr, reg, seed, round, pinned, row_order=None):
        """One half-step of logistic matrix factorisation (pk_lmf_half_step_f64; the arithmetic is spelled out in
        include/polara_hip.h), IN PLACE on X [n_rows x K] and on its AdaGrad state A [n_rows x K] against the fixed block Y
        [n_cols x K], K = rank + 2: every non-empty row of the plan's matrix takes one full-batch AdaGrad step on its positives
        and on min(n_cols, n * neg_prop) negatives drawn inside the kernel from the stream (seed, round).  pinned: the column of
        X that holds the constant 1 (touched neither in X nor in A; -1: none).  Views with a leading dimension are fine.
        row_order: int32 device permutation of the rows (None: the plan's) — never a bit of the result.  Returns X."""
        Cm = plan['matrix']
        n_rows, n_cols = plan['shape']
        K = int(Y.shape[1])
        if K < 3 or K - 2 > self.lmf_max_rank():
            raise ValueError('LMF: rank %d outside 1..%d' % (K - 2, self.lmf_max_rank()))
        for M, n in ((X, n_rows), (A, n_rows), (Y, n_cols)):
            if M.dtype != torch.float64 or M.dim() != 2 or tuple(M.shape) != (n, K) or M.stride(1) != 1 or M.stride(0) < K:
                raise ValueError('LMF half-step: a block of shape %s, strides %s for [%d x %d] fp64 rows'
                                 % (tuple(M.shape), M.stride(), n, K))
        pinned = int(pinned)
        if pinned < -1 or pinned >= K:
            raise ValueError('LMF half-step: pinned column %d outside -1..%d' % (pinned, K - 1))
        seed, round = self._lmf_stream(seed, round)
        order = plan['row_order'] if row_order is None else row_order
        if order.dtype != torch.int32 or order.numel() != n_rows or not order.is_contiguous():
            raise ValueError('LMF half-step: row_order must be a contiguous int32 permutation of the %d rows' % n_rows)
        conf = Cm.values if Cm.values.dtype == torch.float64 else Cm.values.to(torch.float64)
        with self._timed('lmf_half_step', (n_rows, n_cols, int(Cm.indices.numel()), plan['negatives'], K)):
            _lib.check(self.lib.pk_lmf_half_step_f64(self.stream(), n_rows, n_cols, K, _ptr(Cm.indptr), _ptr(Cm.indices), _ptr(conf),
                                                     _ptr(order), _ptr(plan['neg_ptr']), seed, round, pinned, plan['neg_prop'],
                                                     _ptr(Y), Y.stride(0), float(lr), float(reg), _ptr(X), X.stride(0), _ptr(A),
                                                     A.stride(0)), 'pk_lmf_half_step_f64')
        return X

    def lmf_draw_negatives(self, plan, seed, round):
        """int32 [plan['negatives']] (device): the negatives the half-step of (seed, round) draws, row after row in draw order
        (pk_lmf_draw_negatives: the kernel's own draw function; the stream is spelled out in include/polara_hip.h)."""
        Cm = plan['matrix']
        n_rows, n_cols = plan['shape']
        seed, round = self._lmf_stream(seed, round)
        total = plan['negatives']
        out = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)[:total]
        _lib.check(self.lib.pk_lmf_draw_negatives(self.stream(), n_rows, n_cols, _ptr(Cm.indptr), _ptr(plan['neg_ptr']), plan['neg_prop'],
                                                  seed, round, _ptr(out)), 'pk_lmf_draw_negatives')
        return out

    def dense_scores(self, V, E):
        n_rows, K = E.shape
        n_items = V.shape[0]
        out = self.empty(n_rows, n_items)
        _lib.check(self.lib.pk_dense_scores_f64(self.stream(), n_rows, n_items, K, _ptr(V), V.stride(0), _ptr(E),
                                                E.stride(0), _ptr(out), out.stride(0)), 'pk_dense_scores_f64')
        return out

    # ---- K5 ---------------------------------------------------------------------------------
    def ttm(self, plan, idx1, idx2, vals, u, v, n0):
        """res[n0 x (ra*rb)] of the sorted-by-mode0 tensor described by `plan` (see tucker.py)."""
        ra, rb = u.shape[1], v.shape[1]
        res = self.empty(n0, ra * rb)
        partial = self.empty(plan['n_slots'] * ra * rb) if plan['n_slots'] else None
        _lib.check(self.lib.pk_ttm_f64(
            self.stream(), plan['n_tasks'], _ptr(plan['task_row']), _ptr(plan['task_begin']),
            _ptr(plan['task_end']), _ptr(plan['task_slot']), plan['n_long'], _ptr(plan['long_row']),
            _ptr(plan['long_slot_begin']), _ptr(plan['long_slot_end']), _ptr(idx1), _ptr(idx2), _ptr(vals),
            _ptr(u), u.stride(0), ra, _ptr(v), v.stride(0), rb, _ptr(res), res.stride(0), _ptr(partial)),
            'pk_ttm_f64')
        return res

    def tucker_predict(self, users, items, u, v, w, core, want_scores=False):
        """pk_tucker_predict_f64: for each (user, item) pair the index of the feedback level with the largest
        reconstructed Tucker score (CoffeeModel.predict_feedback, models.py:1068-1091).  users / items: host or device
        int64; u, v, w, core: host arrays or device tensors.  Returns (pred int64 device tensor, scores | None)."""
        dev = lambda a, dt: (a if torch.is_tensor(a) else self.to_device(np.ascontiguousarray(a, dtype=dt))).contiguous()
        users, items = dev(users, np.int64), dev(items, np.int64)
        u, v, w, core = (dev(a, np.float64) for a in (u, v, w, core))
        r0, r1, r2 = (int(x) for x in core.shape)
        assert u.shape[1] == r0 and v.shape[1] == r1 and w.shape[1] == r2 and users.numel() == items.numel()
        n, L = int(users.numel()), int(w.shape[0])
        pred = torch.empty(n, dtype=torch.int64, device=self.device)
        scores = self.empty(n, L) if want_scores else None
        _lib.check(self.lib.pk_tucker_predict_f64(self.stream(), n, _ptr(users), _ptr(items), _ptr(u), u.stride(0), _ptr(v),
                                                  v.stride(0), _ptr(w), w.stride(0), _ptr(core), r0, r1, r2, L, _ptr(pred),
                                                  _ptr(scores)), 'pk_tucker_predict_f64')
        return pred, scores

    def synchronize(self):
        torch.cuda.synchronize(self.device)

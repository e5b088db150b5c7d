"""Host-side planning of the item-to-item and most-popular device paths (csrc/i2i.hip): the shapes and limits the
kernels work with, the memory guard of the build and the `topk` checks.  Pure Python: the values mirror the library's
own planning functions (pk_i2i_*; tests/test_i2i_host.py holds the two together) so that they can be checked and
explained without a device."""

MAX_TOPK = 1024            # pk_i2i_max_topk: the per-window candidate lists are merged in 2 x 1024 keys of LDS
COLS = 8                   # columns of C a scoring lane owns (two 16-byte fp32 loads)
WINDOW = 256 * COLS        # columns of C one scoring workgroup covers (pk_i2i_window)
BUILD_WINDOW = 8192        # fp64 columns of C one build workgroup accumulates in LDS (pk_i2i_build_window)
CAND_BUDGET = 512 << 20    # bytes of window candidates per launch pair: users are scored in chunks under it
POPULAR_MAX_ITEMS = 1 << 19   # pk_popular_topk keeps a user's seen bitmap (n_items bits) in 64 KiB of LDS


def leading_dim(n_items):
    """Row stride (elements) of the dense C: n_items rounded up to a whole lane's columns (16-byte aligned rows)."""
    return -(-int(n_items) // COLS) * COLS


def n_windows(n_items):
    return -(-leading_dim(n_items) // WINDOW)


def pow2(topk):
    p = 1
    while p < topk:
        p <<= 1
    return p


def chunk_users(n_users, n_items, topk):
    """Users per launch pair of pk_i2i_topk: every user keeps pow2(topk) keys of 12 bytes per window."""
    if n_users <= 0 or n_items <= 0 or not 1 <= topk <= MAX_TOPK:
        return 0
    per_user = n_windows(n_items) * pow2(topk) * 12
    return int(min(n_users, max(1, CAND_BUDGET // per_user)))


def topk_work_bytes(n_users, n_items, topk):
    n = chunk_users(n_users, n_items, topk) * n_windows(n_items) * pow2(topk)
    return n * 12 + 256


def build_image_bytes(n_items):
    """Bytes of the fp64 build image of C (n_items rows of leading_dim(n_items) doubles)."""
    return int(n_items) * leading_dim(n_items) * 8


def check_build_memory(n_items, free_bytes):
    """The build's guard: C is stored dense, so the fp64 image must fit in half of the free device memory."""
    need = build_image_bytes(n_items)
    if need > free_bytes / 2:
        raise MemoryError('item-to-item: the dense fp64 build image of C (%d x %d items) takes %.2f GB, more than half of '
                          'the %.2f GB of free device memory' % (n_items, n_items, need / 1e9, free_bytes / 1e9))
    return need


def check_topk(topk, n_items, limit=MAX_TOPK):
    """topk > n_items raises like get_topk_elements (models.py:561-563 through np.argpartition); above the device limit
    a ValueError names the limit."""
    topk, n_items = int(topk), int(n_items)
    if topk > n_items:
        raise ValueError('kth(=%d) out of bounds (%d)' % (n_items - topk, n_items))
    if topk < 1:
        raise ValueError('topk must be at least 1, got %d' % topk)
    if limit is not None and topk > limit:
        raise ValueError('topk = %d is above the device limit of %d for this model' % (topk, limit))
    return topk

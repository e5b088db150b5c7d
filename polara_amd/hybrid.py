"""Host-side planning of the HybridSVD device path (csrc/hybrid.hip): the shapes and limits of the dense Cholesky factor
of the item-similarity matrix, the memory guard of the build and the mapping of `features_weight`.  Pure Python: the
values mirror the library's own planning functions (pk_hybrid_ld, pk_hybrid_max_nc, pk_trmm_work_bytes;
tests/test_hybrid_host.py holds the two together) so that they can be checked and explained without a device."""

TILE = 64                  # the kernels' tile / block width: the image is padded to whole tiles
MAX_NC = 64                # pk_hybrid_max_nc: columns of X one triangular product takes
CHUNK = 32                 # tiles of L one task of the triangular product reads


def leading_dim(n_items):
    """Rows and row stride (elements) of the factor's image: n_items rounded up to whole 64 x 64 tiles."""
    return -(-int(n_items) // TILE) * TILE


def image_bytes(n_items):
    """Bytes of the fp64 image of K / L (leading_dim(n_items) rows of leading_dim(n_items) doubles)."""
    ld = leading_dim(n_items)
    return ld * ld * 8


def trmm_work_bytes(n_items, nc):
    """Scratch of one triangular product: a partial block per chunk of a strip when a strip has more than one chunk."""
    strips = leading_dim(n_items) // TILE
    chunks = -(-strips // CHUNK)
    return chunks * leading_dim(n_items) * int(nc) * 8 if chunks > 1 else 0


def check_factor_memory(n_items, free_bytes):
    """The build's guard: the factor is stored dense, so its fp64 image must fit in half of the free device memory."""
    need = image_bytes(n_items)
    if need > free_bytes / 2:
        raise MemoryError('HybridSVD: the dense fp64 Cholesky factor of the item similarity (%d x %d items) takes %.2f GB, '
                          'more than half of the %.2f GB of free device memory' % (n_items, n_items, need / 1e9,
                                                                                    free_bytes / 1e9))
    return need


def beta_of(features_weight):
    """K = S + beta I with beta = (1 - w) / w (hybrid/models.py:283-284)."""
    w = float(features_weight)
    if not 0.0 < w <= 1.0:
        raise ValueError('features_weight must lie in (0, 1], got %r' % features_weight)
    return (1.0 - w) / w


def column_blocks(nc, limit=MAX_NC):
    """[(c0, c1), ...]: the column ranges a product of nc columns is cut into (at most `limit` per call)."""
    return [(c0, min(int(nc), c0 + limit)) for c0 in range(0, int(nc), limit)]

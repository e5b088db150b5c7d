"""What the tests of the blocked sweeps and of the factor models share (test_gpu_bpr.py, test_gpu_warp.py, test_gpu_pmf.py,
test_gpu_kpmf.py, test_gpu_ials.py, test_gpu_lce.py, test_warp_host.py): a dense 0/1 matrix as a device CSR, blocks with a
leading dimension of their own and the check that nothing was written around them, bit equality, and the matrix of the
many-strata case."""
import numpy as np


def device_csr(ops, dense):
    users, items = np.nonzero(dense)
    return ops.csr_from_coo(users.astype(np.int64), items.astype(np.int64), np.ones(len(users)), dense.shape)


def strided(ops, a, pad=3, off=1):
    """`a` on the device inside a wider block: leading dimension a.shape[1] + pad, first column `off`"""
    import torch
    block = torch.zeros(a.shape[0], a.shape[1] + pad, dtype=torch.float64, device=ops.device)
    view = block[:, off:off + a.shape[1]]
    view.copy_(ops.to_device(a))
    return view


def padding_is_zero(view):
    """nothing was written around a view made by `strided`"""
    base = view._base.clone()
    off = view.storage_offset() % base.stride(0)
    base[:, off:off + view.shape[1]] = 0
    return not bool(base.any())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


MANY_STRATA_BLOCKS = 257
MANY_STRATA_SEED = 4                # of the epoch: with it BPR and WARP (max_sampled 3) both train a sample of stratum 256


def many_strata_matrix():
    """300 users x 280 items, about 2 % dense plus one entry per user (1 925 entries): with B = 257 there are more strata, all
    non-empty, than the 256 threads the counters' reduction strides them over, so its second trip runs"""
    dense = (np.random.RandomState(3).rand(300, 280) < 0.02).astype(np.int8)
    dense[np.arange(300), np.arange(300) % 280] = 1
    return dense


def trained_in_the_last_stratum(plan, trained):
    """whether a position of stratum B - 1 of the plan is among the trained ones (a boolean per position of the schedule)"""
    B = plan['blocks']
    return bool(np.asarray(trained)[plan['block_ptr'][(B - 1) * B]:].any())

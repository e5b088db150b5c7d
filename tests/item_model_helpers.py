"""What the device tests of the item-weight models share (test_gpu_ease.py, test_gpu_slim.py, test_gpu_gram.py): the
training matrix as a device CSR under the implicit rule, the cached fixtures of a reference module, and a model over
`ArrayData` with its settings."""
import functools

import numpy as np


def device_csr(hip_ops, idx, val, shape, implicit=False):
    v = np.sign(val) if implicit else val
    return hip_ops.csr_from_coo(idx[:, 0], idx[:, 1], v, shape)


def cached_fixture(ref):
    """fixture(name, implicit) -> (idx, val, shape, SciPy training matrix) of `ref`'s named fixture, computed once."""
    @functools.lru_cache(maxsize=None)
    def fixture(name, implicit):
        idx, val, shape = ref.training(name)
        return idx, val, shape, ref.training_matrix(idx, val, shape, implicit)
    return fixture


def model(name, hip_ops, idx, val, shape, test=None, holdout=None, **settings):
    """The model class `name` of the package over the training triplet (warm start when test rows are given), quiet,
    with `settings` assigned in order."""
    import polara_amd
    from polara_amd.data import ArrayData
    data = ArrayData((idx[:, 0], idx[:, 1], val), n_users=shape[0], n_items=shape[1], test=test, holdout=holdout,
                     warm_start=test is not None)
    m = getattr(polara_amd, name)(data, ops=hip_ops)
    m.verbose = False
    for key, value in settings.items():
        setattr(m, key, value)
    return m


def limits_case():
    """(pairs, val, shape, holdout) of the stated-limits tests: 40 users over 1030 items, more than the 1024 of a list."""
    rng = np.random.default_rng(3)
    n_users, n_items = 40, 1030
    u = np.repeat(np.arange(n_users), 30)
    pairs = np.unique(np.stack([u, rng.integers(0, n_items, len(u))], 1), axis=0)
    val = rng.integers(1, 6, len(pairs)).astype(np.float64)
    hold = (np.arange(n_users), rng.integers(0, n_items, n_users), np.ones(n_users))
    return pairs, val, (n_users, n_items), hold

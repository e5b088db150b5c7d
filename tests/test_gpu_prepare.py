"""The split of raw interactions on the device: pk_split_keys and pk_segment_select against the NumPy twin
(tests/prepare_reference.py) byte for byte, the whole `prepare()` through HipOps against the host path and the reference's
fixtures, and one model end to end."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from polara_amd import ArrayData, SVDModel
from polara_amd.prepare import PrepareNumpyOps, RecommenderArrayData
import prepare_reference as twin
from test_prepare_host import EXPECTED, check_against_fixture, from_fixture, raw_columns, same_arrays

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3, 8, 9, 6, 4)             # every combination the pipeline uses, and hi = 0 with lo = ~p


def device_keys(ops, vals, pos, mode, seed):
    hi, lo = ops.split_keys(None if vals is None else ops.to_device(vals), ops.to_device(pos), mode, seed)
    return hi, lo


def test_split_keys_match_the_twin(hip_ops):
    rng = np.random.default_rng(0)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1.5, 1.5, -1e300, 1e300, 3.0, 3.0000000000000004])
    vals = np.r_[special, rng.choice(special, 1000), rng.normal(size=1000)]
    pos = np.r_[0, 1, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 40, rng.integers(0, 2 ** 33, len(vals) - 7)].astype(np.int64)
    for mode in MODES:
        for seed in (0, 1, 2 ** 64 - 1):
            hi, lo = device_keys(hip_ops, None if mode & 4 else vals, pos, mode, seed)
            thi, tlo = twin.split_keys(vals, pos, mode, seed)
            assert np.array_equal(hi.cpu().numpy().view(np.uint64), thi), (mode, seed)
            assert np.array_equal(lo.cpu().numpy().view(np.uint64), tlo), (mode, seed)
    hi = twin.split_keys(special[:4], np.arange(4), 1, 0)[0]
    assert hi[0] == hi[1] and hi[3] < hi[0] < hi[2]                   # -0.0 = +0.0; denormals keep their sign and order


def key_sets(rng, n, seg):
    """(name, order values, mode): key_hi from 3 distinct values, all equal, all distinct; key_lo in every mode"""
    kinds = (('three', rng.choice([1.0, 2.0, 5.0], n)), ('equal', np.full(n, 4.0)), ('distinct', rng.permutation(n) - n / 2))
    for name, vals in kinds:
        for mode in (0, 1, 2, 3, 8, 9):
            yield name, vals, mode
    yield 'none', None, 6


def check_select(ops, seg, ks, seed=3):
    rng = np.random.default_rng(seed)
    n = int(seg[-1])
    pos = (rng.permutation(n) + 2 ** 31 - n // 2).astype(np.int64)       # positions on both sides of 2^31
    seg_dev = ops.to_device(seg)
    for name, vals, mode in key_sets(rng, n, seg):
        hi, lo = device_keys(ops, vals, pos, mode, seed)
        thi, tlo = twin.split_keys(vals, pos, mode, seed)
        assert np.array_equal(hi.cpu().numpy().view(np.uint64), thi) and np.array_equal(lo.cpu().numpy().view(np.uint64), tlo)
        for k in ks:
            flags = ops.segment_select(seg_dev, hi, lo, k).cpu().numpy()
            want = twin.segment_select(seg, thi, tlo, k)
            assert flags.dtype == np.uint8 and flags.tobytes() == want.tobytes(), (name, mode, k)


def test_segment_select_mixed_lengths(hip_ops):
    """the wave path (<= 256) and the workgroup path in one call, empty segments between"""
    lens = [0, 1, 2, 63, 64, 65, 255, 256, 257, 0, 1025, 4097, 0]
    seg = np.r_[0, np.cumsum(lens)].astype(np.int64)
    ks = sorted({1, 3, 64, 65} | {k for length in lens for k in (length - 1, length, length + 1) if k >= 1})
    check_select(hip_ops, seg, ks)


def test_segment_select_one_long_segment(hip_ops):
    """70 000 entries: beyond the one-workgroup path (32 768), the whole-grid radix select"""
    seg = np.array([0, 70000], dtype=np.int64)
    check_select(hip_ops, seg, (1, 3, 64, 65, 69999, 70000, 70001))


def test_segment_select_long_and_short_together(hip_ops):
    """two whole-grid segments, one of them taken whole, between short ones; flags outside every segment are 0"""
    seg = np.array([7, 40007, 40007, 40012, 110012, 110312], dtype=np.int64)
    rng = np.random.default_rng(5)
    n = 110400
    vals, pos = rng.choice([1.0, 2.0], n), rng.permutation(n).astype(np.int64)
    hi, lo = device_keys(hip_ops, vals, pos, 0, 0)
    thi, tlo = twin.split_keys(vals, pos, 0, 0)
    for k in (2, 300, 40000, 50000):
        flags = hip_ops.segment_select(hip_ops.to_device(seg), hi, lo, k).cpu().numpy()
        want = np.zeros(n, dtype=np.uint8)
        want[7:110312] = twin.segment_select(seg - 7, thi[7:110312], tlo[7:110312], k)
        assert flags.tobytes() == want.tobytes(), k
    empty = hip_ops.segment_select(hip_ops.to_device(np.zeros(1, dtype=np.int64)), hi, lo, 1)
    assert int(empty.sum()) == 0


@pytest.mark.parametrize('name', EXPECTED)
def test_fixture_through_hipops(hip_ops, name):
    g = load_golden(name)
    dev = from_fixture(g, ops=hip_ops)
    check_against_fixture(dev, g)
    same_arrays(dev, from_fixture(g))


@pytest.mark.parametrize('config', [dict(random_holdout=True), dict(permute_tops=True),
                                    dict(permute_tops=True, negative_prediction=True), dict(test_sample=3),
                                    dict(random_holdout=True, warm_start=False, test_ratio=0, holdout_size=2)])
def test_random_modes_equal_the_twin(hip_ops, config):
    users, items, fb = raw_columns(1, n_users=300)
    cfg = dict(dict(test_ratio=0.25, test_fold=2, holdout_size=3), **config)
    for seed in (0, 1):
        dev = RecommenderArrayData(users, items, fb, config=cfg, seed=seed, ops=hip_ops)
        same_arrays(dev, twin.prepare_reference(users, items, fb, None, cfg, seed=seed))
        same_arrays(dev, RecommenderArrayData(users, items, fb, config=cfg, seed=seed, ops=hip_ops))     # two runs
    dev.holdout_size = 2                                                  # the test-side update on the device
    same_arrays(dev, twin.prepare_reference(users, items, fb, None, dict(cfg, holdout_size=2), seed=1))


def test_model_end_to_end(hip_ops):
    users, items, fb = raw_columns(12, n_users=600, n_items=200)
    config = dict(test_ratio=0.2, test_fold=3, holdout_size=1)
    dev = RecommenderArrayData(users, items, fb, config=config, seed=0, ops=hip_ops)
    host = RecommenderArrayData(users, items, fb, config=config, seed=0, ops=PrepareNumpyOps())
    plain = ArrayData(host.training, n_users=host.n_users, n_items=host.n_items, test=host.test.testset,
                      holdout=host.test.holdout, warm_start=True)
    out = []
    for data in (dev, plain):
        m = SVDModel(data, ops=hip_ops)
        m.verbose = False
        m.rank, m.topk = 8, 10
        m.build()
        out.append((m.get_recommendations(), m.evaluate('hits')))
    assert out[0][0].shape == (dev.get_test_shape()[0], 10) and out[0][0].shape[0] > 50
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]

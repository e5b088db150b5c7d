"""CPU: the packed factor image's format as restated in tests/q20_reference.py (the encoder of csrc/foldq.hip row by row,
and the decoder that defines the bits) keeps its contract — every row decodes to within its own error weight — on the
shapes the scoring pass uses, including the rows the format has to work for: zero rows, a bracket's largest entry in an
extra (digit-carried) column, one-column and full-width ranks."""
import numpy as np
import pytest

import q20_reference as q20


@pytest.mark.parametrize('K', [1, 10, 12, 13, 25, 50, 51, 100, 101, 200, 202])
def test_restated_encoder_keeps_the_error_weight_contract(K):
    rng = np.random.default_rng(K)
    n = 1500
    V = rng.standard_normal((n, K)) * ((np.arange(n) + 1.0) ** -0.5)[:, None]
    V[7] = 0.0
    V[100, K - 1] = np.abs(V[64:128]).max() * 1.5
    V[101, K - 1] = -np.abs(V[64:128]).max() * 1.4
    bits, tab = q20.encode(V)
    assert bits.shape == (n, q20.lanes(K) * 16) and bits.dtype == np.uint8
    dec = q20.decode(bits, tab, K)
    err = np.linalg.norm(dec[:, :K] - V, axis=1)
    assert (err <= dec[:, K] * 2.0 ** -24).all()
    vn = np.linalg.norm(V, axis=1)
    ok = vn > 0
    # about half a 20-bit step of the bracket's scale per entry: 2^24 * (4.3 / 2^19) / sqrt(12) ~ 40 times an fp32 rounding
    assert 10.0 < np.median(dec[ok, K] / vn[ok]) < 80.0
    assert (dec[7, :K] == 0).all() or np.abs(dec[7, :K]).max() <= tab[q20.bracket(7)] * 4096.0


def _exact_ranks():
    from test_gpu_foldq_instances import EXACT_K
    return EXACT_K


@pytest.mark.parametrize('K', _exact_ranks())
def test_hand_made_image_makes_the_fold_in_exact(K):
    """the image test_gpu_foldq_instances.py writes with `pack` (and its ladder's values) make every step of the fold-in exact,
    so that its product can be compared bit for bit: (i) the windows convert to fp32 without rounding, (ii) they keep their
    magnitudes, (iii) an fp32 chain of U products rounds nowhere, (iv) a row's fp64 sums span less than 53 bits"""
    from test_gpu_foldq_instances import CLASS_K, KX_CASES, LADDER, N_COLS, fold_host, image_host
    assert set(CLASS_K) | {c[1] for c in KX_CASES} <= set(_exact_ranks())          # every rank that is compared exactly
    im, h = image_host(K), fold_host()
    L, n = q20.lanes(K), N_COLS
    U = q20.steps(L)
    assert h['values'].min() == 1 and h['values'].max() == 4 and h['indices'].min() == 1 and h['indices'].max() == n - 1
    w = q20._windows(np.ascontiguousarray(im['bits']).view(np.uint32).reshape(n, L, 4))      # int64 [n, L, 7]
    # `pack` wrote the fields where the windows start: the fields and digits come back out of the bits
    assert np.array_equal(w[..., :6] >> 12, im['p']) and np.array_equal(w[..., 6] >> 24, im['dig'])
    assert (w[0, :, :5] == 0x7FFFF7FF).all() and (w[0, :, 5] == 0x7FFFF000).all() and (w[0, :, 6] == 0x7F7FFFF7).all() and im['tab'][0] == 1.0
    live, main, digit = w[1:], w[1:, :, :6], w[1:, :, 6]
    assert np.array_equal(q20.f32(live), live.astype(np.float64))                                      # (i)
    assert np.abs(main).max() <= 2 ** 17 and (digit % 256 == 0).all() and np.abs(digit).max() <= 2 ** 25      # (ii)
    assert digit[:, L - 1].min() >= 0 and digit.min() < 0
    s = im['tab'][q20.bracket(np.arange(n))]
    assert set(np.unique(s[1:])) == {2.0 ** -12, 2.0 ** -13, 2.0 ** -14} and (np.diff(im['tab'][1:]) != 0).all()
    assert np.array_equal(im['dec'][1:, K], q20.kappa(K) * im['weight'][1:]) and np.array_equal(im['weight'][1:], digit[:, L - 1] * s[1:])
    # (iii) in units of 2^-14 (main windows) and 2^-6 (digit windows) every product a s w is an integer, and U of the largest
    # stay within the 24 bits of an fp32 significand: no fma of a chain rounds, whatever the entries
    assert U * 4 * np.abs(main).max() * 2.0 ** -12 / 2.0 ** -14 <= 2 ** 24
    assert U * 4 * np.abs(digit).max() * 2.0 ** -12 / (256 * 2.0 ** -14) <= 2 ** 24
    # ... and 3000 emulated chains: fl32(a s) exact, then fp32 fused multiply-adds (the exact product and sum, rounded once)
    rng = np.random.RandomState(K)
    items, a = rng.randint(1, n, (3000, U)), rng.randint(1, 5, (3000, U))
    a_s = (a * s[items]).astype(np.float32)
    assert np.array_equal(a_s.astype(np.float64), a * s[items])
    acc = np.zeros((3000, L, 7), dtype=np.float32)
    exact = np.zeros((3000, L, 7), dtype=np.int64)
    for u in range(U):
        x = w[items[:, u]].astype(np.float32)
        acc = (a_s[:, u, None, None].astype(np.float64) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        exact += (a[:, u] * np.rint(s[items[:, u]] * 2.0 ** 14).astype(np.int64))[:, None, None] * w[items[:, u]]
    assert np.array_equal(acc.astype(np.float64) * 2.0 ** 14, exact.astype(np.float64))
    # (iv) the decoded columns are multiples of 2^-21 (an extra column's lowest digit: 2 * 2^8 * 2^-14 / 65536), the weights
    # of 2^-6; the longest row's sum of magnitudes stays below 2^53 of them
    dec = im['dec'][1:, :K]
    assert np.array_equal(np.rint(dec * 2.0 ** 21), dec * 2.0 ** 21) and np.array_equal(np.rint(im['weight'] * 64.0), im['weight'] * 64.0)
    assert max(LADDER) == 1500 and 1500 * 4 * np.abs(dec).max() * 2.0 ** 21 < 2 ** 53 and 1500 * 4 * im['weight'][1:].max() * 64.0 < 2 ** 53


def test_brackets_are_contiguous_index_ranges_four_per_octave():
    j = np.arange(1 << 16)
    b = q20.bracket(j)
    assert (np.diff(b) >= 0).all() and (np.diff(b) <= 1).all() and b[0] == 0 and b.max() < q20.TAB
    assert q20.bracket((1 << 24) - 1) < q20.TAB
    # four brackets per octave from 4 on: rows 2^e .. 2^(e+1) - 1 split into quarters
    for e in range(2, 16):
        assert len(np.unique(b[1 << e:1 << (e + 1)])) == 4
    assert [q20.lanes(k) for k in (1, 12, 13, 25, 26, 50, 51, 101, 102, 202, 203)] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 0]

"""CPU checks of tests/syrk_reference.py: the inputs and bounds that tests/test_gpu_syrk.py holds the weighted SYRK
kernels to are fair (two independent float64 implementations meet them) and sharp (one dropped row, or two swapped
columns of one 16-wide block, do not)."""
import numpy as np
import pytest

import syrk_reference as sr


def test_launcher_arithmetic():
    assert [sr.effective_splits(1000, 130, s) for s in sr.SPLIT_COUNTS] == [8, 8, 8, 24, 64, 128]
    assert sr.effective_splits(*sr.MANY_SPLITS_CASE) == 1008
    for N, S in sr.AUTO_SPLIT_ROWS:
        assert sr.effective_splits(N, 130) == S
    assert sr.effective_splits(30399, 130) == 8 and sr.effective_splits(40000, 1024) == 16
    assert sr.effective_splits(10 ** 6, 1024) == 128
    assert sr.rows_per_split(1, 8) == 16 and sr.rows_per_split(1000, 8) == 128 and sr.rows_per_split(5003, 24) == 224
    assert sr.num_tiles(130) == 3 and sr.num_tiles(2050) == 153
    # the factor: L + S + 2 roundings of 2^-53, 1 % for the second order
    assert sr.elementwise_bound(1000, 8) == (128 + 8 + 2) * 2.0 ** -53 * 1.01
    assert sr.elementwise_bound(1000, 8, extra=8) == (128 + 16 + 2) * 2.0 ** -53 * 1.01


def test_int_case_is_exact_in_float64():
    """Largest N of the GPU file: all sums are integers below 2^53 (in fact below 2^21), so float64 in ANY order is exact;
    the int64 product, NumPy's float64 product and the split emulation coincide bitwise."""
    rng = np.random.default_rng(1)
    N, P = 45605, 130
    X, c, y = sr.int_case(rng, N, P)
    assert np.all(c != 0) and np.all(np.abs(c) <= 4) and np.all(np.abs(X) <= 3) and np.all(np.abs(y) <= 3)
    assert {-4, -1, 1, 4} <= set(np.unique(c).astype(int)) and {-3, 0, 3} <= set(np.unique(X).astype(int))
    A = sr.int_gram(np.abs(X), np.abs(c))
    assert A.max() < 2 ** 53 and 36 * 10 ** 6 < 2 ** 53           # the sum of the magnitudes bounds every partial sum
    want = sr.int_gram(X, c)
    assert want.dtype == np.int64 and np.array_equal(want[:5], X.astype(np.int64).T[:5] @ (c.astype(np.int64)[:, None] * X.astype(np.int64)))
    assert np.array_equal(X.T @ (c[:, None] * X), want)
    assert np.array_equal(X.T @ (c * y), sr.int_xty(X, c, y))
    for S in (8, 16, 24, 64, 128):
        assert np.array_equal(sr.emulate_splits(X, c, S), want)


@pytest.mark.parametrize('N,P', sr.SPLIT_SHAPES + [sr.MANY_SPLITS_CASE[:2]])
def test_split_emulation_exact_for_every_split_count(N, P):
    rng = np.random.default_rng(N + P)
    X, c, _ = sr.int_case(rng, N, P)
    want = sr.int_gram(X, c)
    counts = sr.SPLIT_COUNTS if (N, P) in sr.SPLIT_SHAPES else [sr.MANY_SPLITS_CASE[2]]
    for s in counts:
        assert np.array_equal(sr.emulate_splits(X, c, sr.effective_splits(N, P, s)), want)


@pytest.mark.parametrize('N,P,n_splits', sr.BOUND_CASES)
def test_bound_is_attainable_and_sharp(N, P, n_splits):
    d = sr.real_reference(N, P)
    X, c = d['X'], d['c']
    S = sr.effective_splits(N, P, n_splits)
    bound = sr.elementwise_bound(N, S) * d['A']
    assert np.all(bound > 0)
    assert np.log10(np.abs(c).max() / np.abs(c).min()) > 3.5 and np.any(c < 0) and np.any(c > 0)
    S64 = X.T @ (c[:, None] * X)
    r_np, r_emu = sr.max_ratio(S64, d['S_ref'], bound), sr.max_ratio(sr.emulate_splits(X, c, S), d['S_ref'], bound)
    print('N {} P {} splits {}: error / bound  numpy {:.4f}  split emulation {:.4f}'.format(N, P, S, r_np, r_emu))
    assert r_np <= 1.0 and r_emu <= 1.0
    # the shortcut sums, same form
    bound_r = sr.elementwise_bound(N, S, extra=8) * d['A_r']
    assert sr.max_ratio(X.T @ (c * d['y']), d['r_ref'], bound_r) <= 1.0
    # one row missing
    n = N // 2
    keep = np.arange(N) != n
    assert sr.max_ratio(X[keep].T @ (c[keep, None] * X[keep]), d['S_ref'], bound) > 1.0
    # two columns of one 16-wide block swapped (rows 16..31, columns 0..15 of the result)
    bad = S64.copy()
    bad[16:32, [3, 4]] = bad[16:32, [4, 3]]
    assert sr.max_ratio(bad, d['S_ref'], bound) > 1.0
    # ... and the same in the last, partial block
    bad = S64.copy()
    bad[P - 2:, [P - 2, P - 1]] = bad[P - 2:, [P - 1, P - 2]]
    assert sr.max_ratio(bad, d['S_ref'], bound) > 1.0

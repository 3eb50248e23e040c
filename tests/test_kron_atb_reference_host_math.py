"""CPU-only: the oracles of tests/kron_atb_reference.py are fair.  At the shapes of tests/test_gpu_kron_atb.py the two oracles
agree, a plain float64 NumPy evaluation and a float64 emulation of the kernels' split order sit inside the entry-wise bounds, and
kernel-style mutations (a 16-row stage dropped, two columns of a 16-block swapped, the pair decode off by one for a single v, a
k-quarter of a sliver slot lost, the weight applied twice on one side) break exact equality and leave the bounds.  The measured
error / bound ratios are printed (-s) and recorded in DESIGN.md section 25."""
import numpy as np
import pytest

import kron_atb_reference as kr

P528 = kr.SLIVER_P


# ---- geometry --------------------------------------------------------------------------------------------------------------
def test_split_geometry_replicas():
    for N, q, S in kr.KRON_SPLIT_CASES:
        assert kr.kron_splits(N, q) == S
    assert kr.kron_splits(16389, 64) == 64 and kr.kron_splits(50, 64) == 8 and kr.kron_splits(10 ** 6, 64) == 64
    assert kr.kron_tiles(64) == (2080, 17, 153) and kr.kron_tiles(32) == (528, 5, 15) and kr.kron_tiles(1) == (1, 1, 1)
    for N, PA, PB, S in kr.ATB_MODE0_SPLIT_CASES:
        assert kr.atb_splits(N, PA, PB, 0) == S
    # 25 workgroups per split without the slivers, 16 with them: (4608 + 12) / 25 = 184 against 288 -> 128
    assert kr.atb_splits(10 ** 6, P528, P528, 0) == 128 and kr.atb_splits(40000, P528, P528, 1) == 128
    assert kr.atb_splits(4101, P528, P528, 1) == 16 and kr.atb_splits(4101, 31, P528, 2) == 16 and kr.atb_splits(100, 2, 2, 0) == 8
    assert kr.atb_splits(10 ** 6, 31, P528, 2) == 128
    for N in (1, 15, 16, 17, 255, 257, 4101, 32775):
        for S in (8, 16, 72, 128):
            L = kr.rows_per_split(N, S)
            assert L % 16 == 0 and L * S >= N and L >= 16
    assert kr.kron_K(32775, 15) == 272 + 128 + 4
    K = kr.atb_K(1000, P528, P528, 1)
    assert K[0, 0] == 128 + 8 + 2 and K[0, 512] == K[512, 0] == K[527, 527] == 128 + 8 + 5
    assert np.all(kr.atb_K(1000, P528, P528, 0) == 128 + 8 + 2)
    assert kr.atb_K(4101, 31, P528, 2)[0, 0] == 272 + 16 + 3 and kr.atb_K(4101, 31, P528, 2)[520, 3] == 272 + 16 + 6


def test_triangular_decode_at_every_column():
    """The kernels' decode of v (a float32 square root, then two integer corrections) against the row-major lower triangle,
    at every v of q = 64; without the corrections float32 is already right here, so the corrections are what an off-by-one
    mutation has to get past."""
    a, b = kr.tri_pairs(64)
    v = np.arange(2080)
    g = ((np.sqrt(np.float32(8.0) * v.astype(np.float32) + np.float32(1.0)) - np.float32(1.0)) * np.float32(0.5)).astype(np.int64)
    g = np.where(g * (g + 1) // 2 > v, g - 1, g)
    g = np.where((g + 1) * (g + 2) // 2 <= v, g + 1, g)
    assert np.array_equal(g, a) and np.array_equal(v - g * (g + 1) // 2, b)
    assert np.all(b <= a) and a[-1] == 63 and b[-1] == 63
    x = kr.xtilde(np.arange(3.0)[None, :] + 2.0)
    assert np.array_equal(kr.kron_rows(x), [[1, 2, 4, 3, 6, 9, 4, 8, 12, 16]])


# ---- exact oracle ------------------------------------------------------------------------------------------------------------
def shows(mutation, N):
    """Whether a mutation must change integer data of N rows: with a handful of rows two columns can coincide, and the third
    k-quarter of a stage is empty below 9 rows."""
    return N >= {'columns_swapped': 8, 'quarter_lost': 9}.get(mutation, 1)


def check_kron_exact(N, q, with_ld=True):
    Z, c = kr.int_kron_case(np.random.default_rng(100003 * q + N), N, q)
    want = kr.exact_kron(Z, c)
    assert np.array_equal(want, want.T) and np.abs(want).max() < 2.0 ** 53
    assert np.array_equal(kr.emulate_kron(Z, c), want), kr.describe_kron(N, q)
    if with_ld:
        ref, A = kr.ld_kron(Z, c)
        assert np.array_equal(ref.astype(np.float64), want) and np.all(ref == want), kr.describe_kron(N, q)
        assert np.all(np.abs(ref) <= A)
    return Z, c, want


@pytest.mark.parametrize('group', [0, 1, 2, 3])
def test_kron_oracles_agree_every_width(group):
    for q in range(16 * group + 1, 16 * group + 17):
        Z, c, want = check_kron_exact(kr.KRON_Q_SWEEP_N, q, with_ld=q <= 40)
        for m in kr.KRON_MUTATIONS:
            if 2 <= q <= 40 or q >= 63:
                assert not np.array_equal(kr.emulate_kron(Z, c, m), want), (q, m)


def test_kron_oracles_agree_every_row_count():
    for N in list(range(1, 49)) + kr.KRON_N_EXTRA + [200, 300, 1001]:
        Z, c, want = check_kron_exact(N, kr.KRON_N_SWEEP_Q)
        for m in kr.KRON_MUTATIONS:
            if shows(m, N):
                assert not np.array_equal(kr.emulate_kron(Z, c, m), want), (N, m)


@pytest.mark.parametrize('N,q,splits', kr.KRON_SPLIT_CASES)
def test_kron_oracles_agree_split_cases(N, q, splits):
    """The longdouble reference is skipped at q = 63 (a minute of longdouble products); the float64 product and the emulation
    of 72 splits are exact there for the same reason.  At q = 64 only the premise is checked (the same code at one more
    column)."""
    if q == 64:
        Z, c = kr.int_kron_case(np.random.default_rng(100003 * q + N), N, q)
        Uk = kr.kron_rows(Z)
        kr.assert_margin(c, Uk, Uk)
        assert np.abs(Uk).max() == 9 and np.abs(c).max() == 4 and np.abs(c).min() == 1
        return
    Z, c, want = check_kron_exact(N, q, with_ld=q < 32)
    if q < 32:
        assert not np.array_equal(kr.emulate_kron(Z, c, 'stage_dropped'), want)


def check_atb_exact(N, PA, PB, mode, with_ld=True):
    A, B, c = kr.int_atb_case(np.random.default_rng(100003 * PA + 1009 * PB + N), N, PA, PB)
    want = kr.exact_atb(A, B, c)
    assert np.array_equal(kr.emulate_atb(A, B, c, mode), want), kr.describe_atb(N, PA, PB, mode)
    if with_ld:
        ref, Ab = kr.ld_atb(A, B, c)
        assert np.all(ref == want) and np.all(np.abs(ref) <= Ab)
    muts = kr.SLIVER_MUTATIONS if kr.is_sliver(PA, PB, mode) else kr.ATB_MUTATIONS
    for m in muts:
        if shows(m, N):
            assert not np.array_equal(kr.emulate_atb(A, B, c, mode, m), want), (N, PA, PB, mode, m)


@pytest.mark.parametrize('PA,PB', kr.ATB_MODE0_SHAPES)
def test_atb_oracles_agree_shapes(PA, PB):
    check_atb_exact(100, PA, PB, 0)


def test_atb_oracles_agree_row_counts():
    PA, PB = kr.ATB_MODE0_N_SWEEP
    for N in list(range(1, 49)) + [255, 257]:
        check_atb_exact(N, PA, PB, 0, with_ld=N % 7 == 0)
    for N, PA, PB, S in kr.ATB_MODE0_SPLIT_CASES:
        check_atb_exact(N, PA, PB, 0, with_ld=N < 10000)


def test_sliver_oracles_agree_row_counts():
    """Mode 1 at 528 x 528: the quarter emulation is exact on integers at every N, and a lost quarter shows as soon as that
    quarter holds a row (N >= 9: rows 8..11 of the first stage)."""
    for N in list(range(1, 49, 3)) + [255, 257, 4101]:
        A, B, c = kr.int_atb_case(np.random.default_rng(100003 * P528 + 1009 * P528 + N), N, P528, P528)
        want = kr.exact_atb(A, B, c)
        assert np.array_equal(kr.emulate_atb(A, B, c, 1), want), N
        lost = kr.emulate_atb(A, B, c, 1, 'quarter_lost')
        assert np.array_equal(lost, want) == (N < 9), N
        wrong = lost != want
        assert not wrong[~kr.slot_masks()['(bi=0, 4)']].any()


def test_kron32_oracles_agree():
    for N in kr.KRON32_N:
        x, B, c = kr.int_atb_case(np.random.default_rng(4242 + N), N, 31, P528)
        want = kr.exact_atb_kron32(x, B, c)
        assert np.array_equal(kr.emulate_atb(x, B, c, 2), want)
        if N <= 257:
            ref, Ab = kr.ld_atb_kron32(x, B, c)
            assert np.all(ref == want)
        for m in kr.SLIVER_MUTATIONS:
            if shows(m, N):
                assert not np.array_equal(kr.emulate_atb(x, B, c, 2, m), want), (N, m)


# ---- bounded oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,q', kr.KRON_BOUND_SHAPES)
def test_kron_bound_holds_for_float64_and_fails_for_mutations(N, q):
    d = kr.real_kron_reference(N, q)
    bound = kr.bound_of(kr.kron_K(N, q), d['A'])
    assert np.all(bound > 0) and np.all(np.isfinite(bound.astype(np.float64)))
    mags = np.abs(d['ref'][d['ref'] != 0]).astype(np.float64)
    assert mags.max() / mags.min() > 1e6                        # entries span many decades: a max-norm check sees only the top
    Uk = kr.kron_rows(d['Z'])
    r_plain = kr.max_ratio(Uk.T @ (d['c'][:, None] * Uk), d['ref'], bound)
    r_emul = kr.max_ratio(kr.emulate_kron(d['Z'], d['c']), d['ref'], bound)
    print('kron CPU {}: K {}, plain float64 {:.4f}, split emulation {:.4f}'.format(kr.describe_kron(N, q), kr.kron_K(N, q), r_plain, r_emul))
    assert r_plain <= 1.0 and r_emul <= 1.0
    for m in kr.KRON_MUTATIONS:
        r = kr.max_ratio(kr.emulate_kron(d['Z'], d['c'], m), d['ref'], bound)
        assert r > 1.0, (m, r)
    # one rounding error too many in a single entry is seen: the bound is not slack by orders of magnitude at the entry level
    K = kr.emulate_kron(d['Z'], d['c'])
    K[-1, 0] += float(bound[-1, 0]) * 2.5
    assert kr.max_ratio(K, d['ref'], bound) > 1.0


def test_kron_power_of_two_scaling_is_exact_in_float64():
    N, q = 1000, 16
    d = kr.real_kron_reference(N, q)
    e = np.random.default_rng(N + q).integers(-10, 11, size=q)
    a, b = kr.tri_pairs(q)
    ev = e[a] + e[b]
    K1 = kr.emulate_kron(d['Z'], d['c'])
    K2 = kr.emulate_kron(np.ldexp(d['Z'], e[None, :]), d['c'] * 128.0)
    assert np.array_equal(K2, np.ldexp(K1, 7 + ev[:, None] + ev[None, :]))


def test_sliver_bounds_hold_for_float64_and_fail_for_mutations():
    N, PA, PB = kr.ATB_REAL_SHAPE
    d = kr.real_atb_reference(N, PA, PB)
    plain = (d['c'][:, None] * d['A']).T @ d['B']
    for mode in (0, 1):
        bound = kr.bound_of(kr.atb_K(N, PA, PB, mode), d['Abound'])
        r_plain = kr.max_ratio(plain, d['ref'], bound)
        r_emul = kr.max_ratio(kr.emulate_atb(d['A'], d['B'], d['c'], mode), d['ref'], bound)
        print('atb CPU {}: plain float64 {:.4f}, split emulation {:.4f}'.format(kr.describe_atb(N, PA, PB, mode), r_plain, r_emul))
        assert r_plain <= 1.0 and r_emul <= 1.0
        for m in (kr.SLIVER_MUTATIONS if mode else kr.ATB_MUTATIONS):
            assert kr.max_ratio(kr.emulate_atb(d['A'], d['B'], d['c'], mode, m), d['ref'], bound) > 1.0, (mode, m)


def test_kron32_bound_holds_for_float64_and_fails_for_mutations():
    N = kr.KRON32_REAL_N
    d = kr.real_kron32_reference(N)
    bound = kr.bound_of(kr.atb_K(N, 31, P528, 2), d['Abound'])
    Xk = kr.kron_rows(kr.xtilde(d['x']))
    r_plain = kr.max_ratio((d['c'][:, None] * Xk).T @ d['B'], d['ref'], bound)
    r_emul = kr.max_ratio(kr.emulate_atb(d['x'], d['B'], d['c'], 2), d['ref'], bound)
    print('kron32 CPU {}: plain float64 {:.4f}, split emulation {:.4f}'.format(kr.describe_atb(N, 31, P528, 2), r_plain, r_emul))
    assert r_plain <= 1.0 and r_emul <= 1.0
    for m in kr.SLIVER_MUTATIONS:
        assert kr.max_ratio(kr.emulate_atb(d['x'], d['B'], d['c'], 2, m), d['ref'], bound) > 1.0, m

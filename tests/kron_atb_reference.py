"""Inputs, split geometry and plain references for the Kronecker SYRK  K4 = sum_n c_n u_n u_n^T  (u_n = packed lower triangle
of z_n z_n^T, wsyrk_kron_kernel) and the two-operand product  C = A^T diag(c) B  (atb_glds_kernel<0 | 1 | 2>) of
csrc/k_wsyrk.hip; used by tests/test_gpu_kron_atb.py.  NumPy only: tests/test_kron_atb_reference_host_math.py shows on the CPU
that every input is fair and that every bound holds for plain float64 and fails for kernel-style mutations.

Two oracles, as for the tiled SYRK (tests/syrk_reference.py, section 22):

  exact     z, A, B, x in -3..3, c in the non-zero integers -4..4.  |c u u| <= 4 * 9 * 9 = 324, so every partial sum over up
            to 1e6 rows is an integer below 2^53 and every summation order, fused or not, gives the same float64: the device
            result must be BITWISE the float64 BLAS product of the integer-valued operands (exact for the same reason; the
            margin is asserted from the actual maxima).
  bounded   real data against a longdouble reference, entry by entry:  |got - ref| <= K 2^-53 1.01 A_ij, A the same sum with
            every factor replaced by its magnitude, K counted from the algorithm with S splits of L rows each:
              Kronecker SYRK          L + S + 4   row operand fl(fl(c z_a) z_b): 2, column operand fl(z_c z_d): 1, the product is
                                                  fused into the sum; at most L additions inside a split, S in the split
                                                  reduction, 1 for the comparison with the rounded reference
              A^T c B, plain          L + S + 2   fl(c a): 1, L, S, 1
              A^T c B, sliver slots   L + S + 5   the same and the 3 additions of the four k-quarters when the tiles are unpacked
                                                  (a quarter's chain has L / 4 terms; L is kept as the bound)
              generated A (mode 2)    one more    fl(fl(x~_a x~_b) c): 2 roundings where the plain kernel has 1
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import syrk_reference as sr

LD, U, WS_TILE, WS_KC = sr.LD, sr.U, sr.WS_TILE, sr.WS_KC
SLIVER_P = 4 * WS_TILE + 16                    # 528: the width at which the 16-column slivers ride on the interior tiles
KRON32_Q = 32                                  # mode 2: x~ = [1, x], x of 31 columns


# ---- the packed lower triangle ------------------------------------------------------------------------------------------
def tri_pairs(q):
    """(a, b), b <= a, of the packed columns v = a (a + 1) / 2 + b, v = 0 .. q (q + 1) / 2 - 1."""
    a, b = np.tril_indices(q)
    assert np.array_equal(a * (a + 1) // 2 + b, np.arange(q * (q + 1) // 2))
    return a, b


def kron_rows(Z):
    """U[n, v] = Z[n, a_v] Z[n, b_v] in the dtype of Z (one rounding per element in float64)."""
    a, b = tri_pairs(Z.shape[1])
    return Z[:, a] * Z[:, b]


def kron_row_operand(Z, c):
    """The kernel's row-side operand fl(fl(c z_a) z_b)."""
    a, b = tri_pairs(Z.shape[1])
    return (c[:, None] * Z[:, a]) * Z[:, b]


def xtilde(x):
    return np.hstack([np.ones((x.shape[0], 1), dtype=x.dtype), x])


# ---- what the launchers compute from the shape -----------------------------------------------------------------------------
def _clamp_splits(s, N):
    s = (s + 7) // 8 * 8
    s = min(s, N // 256 // 8 * 8, 128)
    return max(s, 8)


def kron_tiles(q):
    pv = q * (q + 1) // 2
    nb = (pv + WS_TILE - 1) // WS_TILE
    return pv, nb, nb * (nb + 1) // 2


def kron_splits(N, q):
    """launch_wsyrk_kron: about 9216 workgroups, at least 256 rows per split, between 8 and 128."""
    T = kron_tiles(q)[2]
    return _clamp_splits((9216 + T // 2) // T, N)


def is_sliver(PA, PB, mode):
    return mode == 1 and PA == SLIVER_P and PB == SLIVER_P


def atb_splits(N, PA, PB, mode):
    """launch_atb (modes 0, 1: about 4608 workgroups; 16 per split in sliver mode) and launch_atb_kron32 (mode 2: 128)."""
    if mode == 2:
        return _clamp_splits(128, N)
    TW = 16 if is_sliver(PA, PB, mode) else (-(-PA // WS_TILE)) * (-(-PB // WS_TILE))
    return _clamp_splits((4608 + TW // 2) // TW, N)


def rows_per_split(N, S):
    return sr.rows_per_split(N, S)


def kron_K(N, q):
    S = kron_splits(N, q)
    return rows_per_split(N, S) + S + 4


def atb_K(N, PA, PB, mode):
    """The factor K of every entry of C (a matrix for the sliver modes: the edge slots carry 3 more additions)."""
    S = atb_splits(N, PA, PB, mode)
    base = rows_per_split(N, S) + S + 2 + (1 if mode == 2 else 0)
    rows, cols = (SLIVER_P, SLIVER_P) if mode == 2 else (PA, PB)
    K = np.full((rows, cols), float(base))
    if mode == 2 or is_sliver(PA, PB, mode):
        K[4 * WS_TILE:, :] += 3
        K[:4 * WS_TILE, 4 * WS_TILE:] += 3
    return K


def describe_kron(N, q):
    pv, nb, T = kron_tiles(q)
    S = kron_splits(N, q)
    return 'N {} q {}: Pv {} tile rows {} tiles {} splits {} rows/split {}'.format(N, q, pv, nb, T, S, rows_per_split(N, S))


def describe_atb(N, PA, PB, mode):
    S = atb_splits(N, PA, PB, mode)
    return 'N {} PA {} PB {} mode {}: splits {} rows/split {}{}'.format(N, PA, PB, mode, S, rows_per_split(N, S),
                                                                       ' (sliver)' if mode == 2 or is_sliver(PA, PB, mode) else '')


def kron_entry(i, j, q):
    """Where entry (i, j) of K4 lives: its index pairs, its 128-tile and its 16-block."""
    a, b = tri_pairs(q)
    return '(a, b | c, d) = ({}, {} | {}, {}), tile ({}, {}), block ({}, {})'.format(
        a[i], b[i], a[j], b[j], i // WS_TILE, j // WS_TILE, (i % WS_TILE) // 16, (j % WS_TILE) // 16)


def sliver_slot(i, j):
    """The slot of entry (i, j) of a 528 x 528 result in the sliver modes."""
    ti, tj = i // WS_TILE, j // WS_TILE
    if ti < 4 and tj < 4:
        return 'interior tile ({}, {})'.format(ti, tj)
    if ti < 4:
        return 'slot (bi = {}, 4): column groups summed'.format(ti)
    if tj < 4:
        return 'slot (4, bj = {}): row groups summed'.format(tj)
    return 'corner (4, 4)'


def slot_masks():
    """name -> boolean mask over the 528 x 528 result: the interior, each (bi, 4), each (4, bj), the corner."""
    i, j = np.indices((SLIVER_P, SLIVER_P))
    ti, tj = i // WS_TILE, j // WS_TILE
    out = {'interior': (ti < 4) & (tj < 4), 'corner': (ti == 4) & (tj == 4)}
    for b in range(4):
        out['(bi={}, 4)'.format(b)] = (ti == b) & (tj == 4)
        out['(4, bj={})'.format(b)] = (ti == 4) & (tj == b)
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------
def int_kron_case(rng, N, q):
    """(Z, c): integers as float64, Z in -3..3, c non-zero in -4..4."""
    Z, c, _ = sr.int_case(rng, N, q)
    return Z, c


def real_kron_case(rng, N, q):
    """Z normal with column j scaled by 10^u_j, u in [-1.5, 1.5] (fourth-order products inside 10^+-6); c of mixed sign,
    |c| log-uniform over 1e-2 .. 1e2."""
    Z = rng.normal(size=(N, q)) * 10.0 ** rng.uniform(-1.5, 1.5, size=q)
    c = rng.choice([-1.0, 1.0], size=N) * 10.0 ** rng.uniform(-2.0, 2.0, size=N)
    return Z, c


def int_atb_case(rng, N, PA, PB):
    A, c, _ = sr.int_case(rng, N, PA)
    B = rng.integers(-3, 4, size=(N, PB)).astype(np.float64)
    return A, B, c


def real_atb_case(rng, N, PA, PB, narrow_a=False):
    """A, B as real_case (columns scaled by 10^u, u in [-3, 3]; [-1.5, 1.5] for an A whose columns are multiplied in pairs)."""
    A, c, _ = sr.real_case(rng, N, PA)
    if narrow_a:
        A = rng.normal(size=(N, PA)) * 10.0 ** rng.uniform(-1.5, 1.5, size=PA)
    B, _, _ = sr.real_case(rng, N, PB)
    return A, B, c


def assert_margin(c, left, right):
    """The exact oracle's premise from the actual maxima: N max|c| max|left| max|right| < 2^53, so no partial sum in any order
    can round."""
    N = left.shape[0]
    top = float(N) * np.abs(c).max() * np.abs(left).max() * np.abs(right).max()
    assert top < 2.0 ** 53, top
    for v in (c, left, right):
        assert np.array_equal(v, np.rint(v)), 'integer data expected'


# ---- references ------------------------------------------------------------------------------------------------------------
def exact_kron(Z, c):
    """K4 of integer data: a float64 BLAS product of integer-valued operands (exact: see assert_margin)."""
    Uk = kron_rows(Z)
    assert_margin(c, Uk, Uk)
    return Uk.T @ (c[:, None] * Uk)


def exact_atb(A, B, c):
    assert_margin(c, A, B)
    return (c[:, None] * A).T @ B


def exact_atb_kron32(x, B, c):
    Xk = kron_rows(xtilde(x))
    return exact_atb(Xk, B, c)


def _ld(v):
    return np.asarray(v, dtype=np.float64).astype(LD)


def ld_tn(left, right, lower_only=False):
    """left^T right with products and sums in longdouble (operands longdouble, observation axis made contiguous: einsum's own
    loop -- there is no BLAS for longdouble -- over 32-row blocks of the result on a few threads); lower_only computes block
    rows of the lower triangle and mirrors them (a symmetric product)."""
    LT, RT = np.ascontiguousarray(left.T), np.ascontiguousarray(right.T)
    PA, PB = LT.shape[0], RT.shape[0]
    out = np.zeros((PA, PB), dtype=LD)

    def block(i0):
        i1 = min(i0 + 32, PA)
        j1 = i1 if lower_only else PB
        out[i0:i1, :j1] = np.einsum('ik,jk->ij', LT[i0:i1], RT[:j1])

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(block, range(0, PA, 32)[::-1]))           # the long block rows first
    if lower_only:
        out = np.tril(out) + np.tril(out, -1).T
    return out


def ld_kron(Z, c):
    """(K4_ref, A): the longdouble reference and the magnitude sum sum |c| |u_i| |u_j| of the entry-wise bound."""
    Ul = kron_rows(_ld(Z))
    cl = _ld(c)
    ref = ld_tn(cl[:, None] * Ul, Ul, lower_only=True)
    Ua = np.abs(Ul)
    return ref, ld_tn(np.abs(cl)[:, None] * Ua, Ua, lower_only=True)


def ld_atb(A, B, c):
    """(C_ref, A_bound) for operands given in float64 or longdouble."""
    Al, Bl, cl = A.astype(LD), B.astype(LD), _ld(c)
    return ld_tn(cl[:, None] * Al, Bl), ld_tn(np.abs(cl)[:, None] * np.abs(Al), np.abs(Bl))


def ld_atb_kron32(x, B, c):
    return ld_atb(kron_rows(xtilde(_ld(x))), B, c)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


KRON_BOUND_SHAPES = [(1000, 16), (4101, 23), (2000, 64), (32775, 15)]
ATB_REAL_SHAPE = (1000, SLIVER_P, SLIVER_P)              # mode 0 against mode 1 on real data
KRON32_REAL_N = 4101


@functools.lru_cache(maxsize=None)
def real_kron_reference(N, q):
    """The seeded real case of shape (N, q) with its references, computed once per process; read-only."""
    Z, c = real_kron_case(np.random.default_rng(9000011 * q + N), N, q)
    ref, A = ld_kron(Z, c)
    return _freeze(dict(Z=Z, c=c, ref=ref, A=A))


@functools.lru_cache(maxsize=None)
def real_atb_reference(N, PA, PB):
    A, B, c = real_atb_case(np.random.default_rng(8000009 * PA + 17 * PB + N), N, PA, PB)
    ref, Ab = ld_atb(A, B, c)
    return _freeze(dict(A=A, B=B, c=c, ref=ref, Abound=Ab))


@functools.lru_cache(maxsize=None)
def real_kron32_reference(N):
    x, B, c = real_atb_case(np.random.default_rng(6000011 + N), N, KRON32_Q - 1, SLIVER_P, narrow_a=True)
    ref, Ab = ld_atb_kron32(x, B, c)
    return _freeze(dict(x=x, B=B, c=c, ref=ref, Abound=Ab))


def bound_of(K, A):
    return K * (U * 1.01) * A


max_ratio, worst_entry = sr.max_ratio, sr.worst_entry


# ---- float64 emulations of the split order, with the kernels' mutations ------------------------------------------------------
def _split_ranges(N, S):
    rps = rows_per_split(N, S)
    return [(min(s * rps, N), min((s + 1) * rps, N)) for s in range(S)]


def emulate_tn(left, right, S):
    """One float64 product per split, partials added in split order (an empty split adds a zero matrix)."""
    out = np.zeros((left.shape[1], right.shape[1]))
    for r0, r1 in _split_ranges(left.shape[0], S):
        out = out + (left[r0:r1].T @ right[r0:r1] if r1 > r0 else 0.0)
    return out


def emulate_kron(Z, c, mutation=None):
    """The Kronecker kernel's order in float64: row operand fl(fl(c z_a) z_b), column operand fl(z_c z_d), one product per
    split.  mutation: None or one of KRON_MUTATIONS."""
    N, q = Z.shape
    S = kron_splits(N, q)
    R, Cc = kron_row_operand(Z, c), kron_rows(Z)
    pv = R.shape[1]
    v = min(pv - 1, 5 * pv // 7)                                  # a packed column with b >= 1 when q >= 2
    a, b = tri_pairs(q)
    if mutation == 'decode_off_by_one' and pv > 1:
        b2 = b[v] - 1 if b[v] > 0 else b[v] + 1 if b[v] < a[v] else a[v] - 1      # another column of z for this one v
        R = R.copy(); Cc = Cc.copy()
        R[:, v] = (c * Z[:, a[v]]) * Z[:, b2]; Cc[:, v] = Z[:, a[v]] * Z[:, b2]
    if mutation == 'weight_twice_on_one_side':
        R = c[:, None] * R
    K = emulate_tn(R, Cc, S)
    K = np.tril(K) + np.tril(K, -1).T                             # the kernel computes the lower tiles, the unpacking mirrors them
    i0 = (pv - 1) // 16 * 16                                      # the last 16-block row (ragged unless 16 | Pv)
    if mutation == 'stage_dropped':                               # rows 0..15 never reach block row i0
        r1 = min(16, N)
        K[i0:, :] -= R[:r1, i0:].T @ Cc[:r1]
        K[:, i0:] = K[i0:, :].T
    if mutation == 'columns_swapped' and pv > 1:                  # two columns of the last 16-block row trade places
        j = max(i0 - 1, 0)
        K[i0:, [j, j + 1]] = K[i0:, [j + 1, j]]
    return K


KRON_MUTATIONS = ['stage_dropped', 'columns_swapped', 'decode_off_by_one', 'weight_twice_on_one_side']


def emulate_atb(A, B, c, mode, mutation=None):
    """The two-operand kernels' order in float64; A is the explicit left operand (for mode 2 the caller passes x and the packed
    triangle is formed here with one rounding).  In the sliver modes the edge slots are sums of four k-quarters (rows 4 g .. 4 g
    + 3 of every 16-row stage), each reduced over the splits on its own and added in the order of g."""
    if mode == 2:
        A = kron_rows(xtilde(A))
    N, PA = A.shape
    PB = B.shape[1]
    S = atb_splits(N, 31 if mode == 2 else PA, PB, mode)
    L = A * c[:, None]
    if mutation == 'weight_twice_on_one_side':
        L = L * c[:, None]
    C = emulate_tn(L, B, S)
    if mutation == 'stage_dropped':                               # the first tile row loses rows 0..15
        r1 = min(16, N)
        C[:min(WS_TILE, PA), :] -= L[:r1, :WS_TILE].T @ B[:r1]
    if mutation == 'columns_swapped' and PB > 1:                  # two columns of the first 16-block row trade places
        C[:16, [0, 1]] = C[:16, [1, 0]]
    if mode == 2 or is_sliver(PA, PB, mode):
        E = 4 * WS_TILE
        edge = np.zeros_like(C)
        quarter = (np.arange(N) % 16) // 4
        lost = 2 if mutation == 'quarter_lost' else -1
        for g in range(4):
            rows = quarter == g
            Lg, Bg = np.where(rows[:, None], L, 0.0), np.where(rows[:, None], B, 0.0)
            part = np.zeros_like(C)
            part[:E, E:] = emulate_tn(Lg[:, :E], Bg[:, E:], S)
            part[E:, :] = emulate_tn(Lg[:, E:], Bg, S)
            if g == lost:
                part[:WS_TILE, E:] = 0.0                          # slot (bi = 0, 4) loses its third quarter
            edge = edge + part
        C[:E, E:] = edge[:E, E:]
        C[E:, :] = edge[E:, :]
    return C


ATB_MUTATIONS = ['stage_dropped', 'columns_swapped', 'weight_twice_on_one_side']
SLIVER_MUTATIONS = ATB_MUTATIONS + ['quarter_lost']


# ---- the shapes of tests/test_gpu_kron_atb.py -------------------------------------------------------------------------------
KRON_Q_SWEEP_N = 50                                         # a. every q in 1..64
KRON_N_SWEEP_Q = 16                                         # b. every N in 1..48 and the five below
KRON_N_EXTRA = [127, 128, 129, 255, 257]
KRON_SPLIT_CASES = [(4101, 16, 16), (6149, 23, 24), (32775, 15, 128), (18437, 63, 72), (16389, 64, 64)]      # c. (N, q, splits)
ATB_MODE0_SHAPES = [(2, 2), (2, 130), (16, 512), (128, 128), (130, 128), (128, 130), (126, 258), (256, 256), (258, 386),
                    (SLIVER_P, SLIVER_P)]                   # j. at N = 100
ATB_MODE0_N_SWEEP = (258, 130)
ATB_MODE0_SPLIT_CASES = [(4101, 130, 130, 16), (32771, 130, 130, 128)]
SLIVER_N_EXTRA = [255, 257, 4101, 32771]
KRON32_N = [1, 15, 16, 17, 33, 257, 4101]

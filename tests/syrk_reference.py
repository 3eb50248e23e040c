"""Inputs and plain references for the tiled weighted SYRK  S = X^T diag(c) X  (csrc/k_wsyrk.hip) and the shortcut sums
r = X^T (c o y) that ride on its diagonal tiles; used by tests/test_gpu_syrk.py.  NumPy only: importable and runnable
without the library, so tests/test_syrk_reference_host_math.py can show on the CPU that every input is fair.

Two oracles:

  exact     small-integer data.  Every partial sum of c_n x_ni x_nj is an integer far below 2^53, so every summation
            order, fused or not, gives the same float64: the device result must be BITWISE the int64 matrix product.
  bounded   real data against a longdouble reference, entry by entry:
                |S_ij - Sref_ij| <= (L + S + 2) 2^-53 1.01 A_ij,     A = |X|^T diag(|c|) |X|,
            S = the number of splits of the observation axis, L = rows per split.  Every term c_n x_ni x_nj is rounded
            once (the c_n scaling; the matrix cores fuse the product into the sum), joins a chain of at most L additions
            inside its split, and its split's partial then joins a chain of at most S additions: at most L + S + 1
            roundings (1 + d), |d| <= 2^-53, on the way of any term, whatever the order inside a split.  One more covers
            the reference's own rounding to float64 on comparison; 1.01 covers the second-order terms ((L + S) 2^-53 is
            below 1e-11 at every size here).  It is a bound on the algorithm, not fitted to a kernel.
"""
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53                            # unit roundoff of float64
WS_TILE = 128                             # tile width of the kernel
WS_KC = 16                                # rows per stage


# ---- what the launcher computes from (N, P, n_splits) --------------------------------------------------------------
def num_tiles(P):
    nb = (P + WS_TILE - 1) // WS_TILE
    return nb * (nb + 1) // 2


def effective_splits(N, P, n_splits=0):
    """The split count the library uses: a user value rounded up to a multiple of 8; 0 = the automatic choice
    (about 18 work items per compute unit, at least ~1900 rows per split, between 8 and 128)."""
    if n_splits > 0:
        return (n_splits + 7) // 8 * 8
    T = num_tiles(P)
    s = (4608 + T // 2) // T
    s = (s + 7) // 8 * 8
    s = min(s, N // 1900 // 8 * 8, 128)
    return max(s, 8)


def rows_per_split(N, S):
    """ceil(N / S) rounded up to whole 16-row stages, at least one stage."""
    rps = -(-N // S)
    return max(-(-rps // WS_KC) * WS_KC, WS_KC)


def elementwise_bound(N, n_splits, extra=0):
    """The factor of A in the entry-wise bound for `n_splits` (effective) splits of N rows; `extra` further additions
    (8 for the eight-group reduction of the shortcut sums)."""
    L = rows_per_split(N, n_splits)
    return (L + n_splits + extra + 2) * U * 1.01


# ---- inputs -------------------------------------------------------------------------------------------------------
def int_case(rng, N, P):
    """(X, c, y) as float64 holding small integers: X and y in -3..3, c in the NON-ZERO integers -4..4 (no missing row
    can hide behind a zero weight).  |c x x| <= 36, so sums over up to 1e6 rows stay below 2^26."""
    X = rng.integers(-3, 4, size=(N, P)).astype(np.float64)
    c = (rng.integers(1, 5, size=N) * rng.choice([-1, 1], size=N)).astype(np.float64)
    y = rng.integers(-3, 4, size=N).astype(np.float64)
    return X, c, y


def real_case(rng, N, P):
    """(X, c, y): X normal with column j scaled by 10^u_j, u uniform in [-3, 3]; c of mixed sign with magnitudes
    log-uniform over four decades (1e-2 .. 1e2); y normal."""
    X = rng.normal(size=(N, P)) * 10.0 ** rng.uniform(-3.0, 3.0, size=P)
    c = rng.choice([-1.0, 1.0], size=N) * 10.0 ** rng.uniform(-2.0, 2.0, size=N)
    y = rng.normal(size=N)
    return X, c, y


# ---- references ---------------------------------------------------------------------------------------------------
def int_gram(X, c):
    """X^T diag(c) X as an int64 matrix product (operands with the observation axis contiguous: NumPy's integer matmul
    has no BLAS behind it, einsum's contiguous inner loop is ten times faster)."""
    Xi, ci = X.astype(np.int64), c.astype(np.int64)
    assert np.array_equal(Xi, X) and np.array_equal(ci, c), 'integer data expected'
    XT = np.ascontiguousarray(Xi.T)
    return np.einsum('ik,jk->ij', XT, XT * ci[None, :])


def int_xty(X, c, y):
    """X^T (c o y) as an int64 product."""
    return X.astype(np.int64).T @ (c.astype(np.int64) * y.astype(np.int64))


def ld_gram(X, c):
    """X^T diag(c) X with products and sums in longdouble (block rows of the lower triangle, mirrored)."""
    Xl = np.asarray(X, dtype=np.float64).astype(LD)
    XT = np.ascontiguousarray(Xl.T)                       # both operands with the observation axis contiguous:
    CXT = np.ascontiguousarray((np.asarray(c, dtype=np.float64).astype(LD)[:, None] * Xl).T)     # einsum's own loop
    P = Xl.shape[1]                                       # (no BLAS for longdouble) then runs at ~2 ns per product
    S = np.zeros((P, P), dtype=LD)
    for i0 in range(0, P, WS_TILE):
        i1 = min(i0 + WS_TILE, P)
        S[i0:i1, :i1] = np.einsum('ik,jk->ij', XT[i0:i1], CXT[:i1])
    low = np.tril(S)
    return low + np.tril(S, -1).T


def ld_xty(X, cy):
    return np.asarray(X, dtype=np.float64).astype(LD).T @ np.asarray(cy, dtype=np.float64).astype(LD)


# the shapes of real_case that tests/test_gpu_syrk.py uses, with the seed of each
REAL_SHAPES = [(1000, 130), (4099, 254), (5003, 258), (30407, 130), (2000, 1024)]


@functools.lru_cache(maxsize=None)
def real_reference(N, P):
    """The seeded real_case of shape (N, P) with its longdouble references, computed once per process and shared:
    dict(X, c, y, S_ref, A, r_ref, A_r); r is for cy = fl(c y).  Callers must not modify the arrays."""
    rng = np.random.default_rng(7000003 * P + N)
    X, c, y = real_case(rng, N, P)
    cy = c * y
    out = dict(X=X, c=c, y=y, S_ref=ld_gram(X, c), A=ld_gram(np.abs(X), np.abs(c)),
               r_ref=ld_xty(X, cy), A_r=ld_xty(np.abs(X), np.abs(cy)))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- float64 emulation of the split order -----------------------------------------------------------------------------
def emulate_splits(X, c, n_splits):
    """Plain float64 emulation of the kernel's split order: one product per split of `rows_per_split` rows, partials
    added in split order (empty splits add a zero matrix, as on the device).  n_splits is the effective count."""
    N, P = X.shape
    rps = rows_per_split(N, n_splits)
    S = np.zeros((P, P))
    for s in range(n_splits):
        r0, r1 = min(s * rps, N), min((s + 1) * rps, N)
        if r1 > r0:
            S = S + X[r0:r1].T @ (c[r0:r1, None] * X[r0:r1])
        else:
            S = S + 0.0
    return S


def max_ratio(S, S_ref, bound):
    """Largest |S - S_ref| / bound over the entries (longdouble difference); NaN-safe: a non-finite entry gives inf."""
    err = np.abs(np.asarray(S, dtype=LD) - S_ref)
    ratio = np.where(np.isfinite(err), err / bound, np.inf)
    return float(np.max(ratio))


def worst_entry(S, S_ref, bound):
    err = np.abs(np.asarray(S, dtype=LD) - S_ref)
    ratio = np.where(np.isfinite(err), err / bound, np.inf)
    k = int(np.argmax(ratio))
    return np.unravel_index(k, ratio.shape), float(ratio.flat[k])


# ---- the cases of tests/test_gpu_syrk.py that the CPU file replays ------------------------------------------------------
BOUND_CASES = [(1000, 130, 0), (4099, 254, 0), (5003, 258, 24), (30407, 130, 0), (2000, 1024, 64)]      # (N, P, n_splits)
SPLIT_SHAPES = [(1000, 130), (5003, 258)]
SPLIT_COUNTS = [1, 5, 8, 20, 64, 128]                      # round to 8, 8, 8, 24, 64, 128
MANY_SPLITS_CASE = (100, 66, 1001)                         # rounds to 1008: one tile, almost every split empty
AUTO_SPLIT_ROWS = [(30407, 16), (45605, 24)]               # P = 130: N and the automatic split count there

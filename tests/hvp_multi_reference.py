"""Inputs and plain references for the fused multi-vector pass (csrc/k_hvp_multi.hip), used by tests/test_gpu_hvp_multi.py:

    full form   R[q] = X^T diag(c) X u_q  (+ the diagonal prior term a o u_q)       `ctx.hvp_multi`
    row form    T[n][q] = s_n x_n . z_q                                             `ctx.rows_times_matrix`

NumPy only: importable and runnable without the library, so tests/test_hvp_multi_reference_host_math.py can show on the
CPU that every input is fair and every oracle sharp.

Two oracles:

  exact     small-integer data (X, U, Zt in -3..3, weights non-zero in -4..4, prior entries 1..4).  A term c x x u is at
            most 108 in magnitude, a sum over 1024 columns and 6145 rows stays below 2^30: every partial sum is an integer
            far below 2^53, so every summation order, fused or not, gives the same float64 and the device result must be
            BITWISE the int64 product.
  bounded   real data against a longdouble reference, entry by entry:
                |R - R_ref| <= K_R 2^-53 1.01 A_R,      A_R = |X|^T diag(|c|) |X| |U|^T  (+ |a| o |u|)
                |T - T_ref| <= K_T 2^-53 1.01 A_T,      A_T = |s| o (|X| |Zt|^T)
            K counts the roundings (1 + d), |d| <= 2^-53, that any single term c_n x_np x_nk u_qk can meet on its way
            into the result.  It follows the algorithm, not a kernel's measured error:

              P + NW   into T.  A wave owns P_pad / NW columns and adds their products on two chains of matrix-core
                       instructions, joins the two chains (1 addition) and the NW partial tiles of the waves meet in LDS
                       (NW - 1 additions).  The padded columns meet zeros of U: adding an exact zero does not round, so at
                       most one rounding per REAL column, P in all, plus the NW joins.
              1        the scaling of T by the row's weight.
              8 ceil(nchunks / grid)
                       into a workgroup's accumulator: an 8-row chunk is two 16 x 16 x 4 instructions per tile, i.e. 8
                       additions, and a workgroup takes every grid-th chunk (the product x_np (c T) is fused into the sum).
              grid     the fixed-order reducer adds the grid = min(256, nchunks) partials of the workgroups (eight strided
                       chains, then the eight chain sums: the empty chains of a small grid add exact zeros).
              1        the prior term a u joining the sum.
              1        the reference's own rounding to float64 on comparison.

            K_R is their sum; K_T = P + NW + 1 + 1 (the first two items and the final rounding).  1.01 covers the
            second-order terms (K 2^-53 < 2e-13 at every size here).

The mutations of the host-math file are the mistakes such a kernel makes: a dropped tail row, a weight taken from the
neighbouring row, two output columns exchanged, a vector given its neighbour's result, the row past N counted with the
clamped data of row N - 1.  Each must break the exact oracle and leave the bound by two orders of magnitude.
"""
import numpy as np

LD = np.longdouble
U_ROUND = 2.0 ** -53                      # unit roundoff of float64
HM_ROWS = 8                               # observations per chunk
HM_MAX_GRID = 256                         # one workgroup per compute unit
HM_COLS = 128                             # columns per LDS-DMA instruction: P is padded to a multiple


# ---- what the launcher computes from (N, P, tuning) ----------------------------------------------------------------
def padded_cols(P):
    return -(-P // HM_COLS) * HM_COLS


def n_blocks(P):
    """NB, the template parameter: 1..8."""
    return padded_cols(P) // HM_COLS


def eight_waves_apply(P):
    return n_blocks(P) % 2 == 0


def n_waves(P, four_waves=False):
    """Eight waves per workgroup where the 128-column blocks split evenly and tuning bit 2 is clear, four otherwise."""
    return 8 if eight_waves_apply(P) and not four_waves else 4


def n_chunks(N):
    return -(-N // HM_ROWS)


def grid(N):
    return min(HM_MAX_GRID, n_chunks(N))


def chunks_per_workgroup(N):
    return -(-n_chunks(N) // grid(N))


def roundings_T(P, four_waves=False):
    return P + n_waves(P, four_waves) + 1 + 1


def roundings_R(N, P, four_waves=False):
    return P + n_waves(P, four_waves) + 1 + 8 * chunks_per_workgroup(N) + grid(N) + 1 + 1


def bound_T(P, four_waves=False):
    """The factor of A_T in the entry-wise bound of the row form."""
    return roundings_T(P, four_waves) * U_ROUND * 1.01


def bound_R(N, P, four_waves=False):
    """The factor of A_R in the entry-wise bound of the full form."""
    return roundings_R(N, P, four_waves) * U_ROUND * 1.01


# ---- inputs -------------------------------------------------------------------------------------------------------
def int_case(rng, N, P, Q, off=0):
    """dict(X (N x P), c (N), U (Q x (off + P)), a (off + P)) as float64 holding small integers: X and U in -3..3, c in the
    NON-ZERO integers -4..4 (no missing row can hide behind a zero weight), the prior diagonal a in 1..4."""
    X = rng.integers(-3, 4, size=(N, P)).astype(np.float64)
    c = (rng.integers(1, 5, size=N) * rng.choice([-1, 1], size=N)).astype(np.float64)
    U = rng.integers(-3, 4, size=(Q, off + P)).astype(np.float64)
    a = rng.integers(1, 5, size=off + P).astype(np.float64)
    return dict(X=X, c=c, U=U, a=a, off=off)


def real_case(rng, N, P, Q, off=0):
    """Same shapes: X normal with column j scaled by 10^u_j, u uniform in [-3, 3]; c of mixed sign with magnitudes
    log-uniform over four decades (1e-2 .. 1e2); the rows of U normal on scales 10^v_q, v uniform in [-2, 2]; the prior
    diagonal integers 1..4 (the layout's pre-block rows are then exactly a o u)."""
    X = rng.normal(size=(N, P)) * 10.0 ** rng.uniform(-3.0, 3.0, size=P)
    c = rng.choice([-1.0, 1.0], size=N) * 10.0 ** rng.uniform(-2.0, 2.0, size=N)
    U = rng.normal(size=(Q, off + P)) * 10.0 ** rng.uniform(-2.0, 2.0, size=(Q, 1))
    a = rng.integers(1, 5, size=off + P).astype(np.float64)
    return dict(X=X, c=c, U=U, a=a, off=off)


def case_seed(N, P, Q, off=0):
    return 1000003 * P + 7919 * N + 101 * Q + off


def make_case(kind, N, P, Q, off=0):
    rng = np.random.default_rng(case_seed(N, P, Q, off) + (0 if kind == 'int' else 500000007))
    return (int_case if kind == 'int' else real_case)(rng, N, P, Q, off)


# ---- references ---------------------------------------------------------------------------------------------------
def _as_int(*arrs):
    out = []
    for v in arrs:
        vi = v.astype(np.int64)
        assert np.array_equal(vi, v), 'integer data expected'
        out.append(vi)
    return out


def _rows_product(X, s, Zt):
    """diag(s) X Zt^T in the dtype of the operands (einsum: NumPy has no BLAS for int64 and longdouble)."""
    return s[:, None] * np.einsum('nk,qk->nq', X, Zt)


def _full_product(X, c, U, a, off):
    """Rows q: X^T diag(c) X u_q[off:] scattered at `off`, plus a o u_q; operands with the contracted axis contiguous."""
    Ug = np.ascontiguousarray(U[:, off:])
    cT = np.ascontiguousarray(_rows_product(X, c, Ug).T)                    # Q x N
    out = a[None, :] * U
    out[:, off:] += np.einsum('qn,pn->qp', cT, np.ascontiguousarray(X.T))
    return out


def int_full(case):
    X, c, U, a = _as_int(case['X'], case['c'], case['U'], case['a'])
    return _full_product(X, c, U, a, case['off'])


def ld_full(case):
    return _full_product(*(np.asarray(case[k], dtype=np.float64).astype(LD) for k in ('X', 'c', 'U', 'a')), case['off'])


def abs_full(case):
    """A_R: the same product of the absolute values, in longdouble."""
    return _full_product(*(np.abs(np.asarray(case[k], dtype=np.float64)).astype(LD) for k in ('X', 'c', 'U', 'a')), case['off'])


def f64_full(case):
    """Plain float64 NumPy evaluation (BLAS order): an honest implementation that must sit inside the bound."""
    X, c, U, a, off = case['X'], case['c'], case['U'], case['a'], case['off']
    out = a[None, :] * U
    out[:, off:] += (c[:, None] * (X @ U[:, off:].T)).T @ X
    return out


def int_rows(X, s, Zt):
    return _rows_product(*_as_int(X, s, Zt))


def ld_rows(X, s, Zt):
    return _rows_product(*(np.asarray(v, dtype=np.float64).astype(LD) for v in (X, s, Zt)))


def abs_rows(X, s, Zt):
    return _rows_product(*(np.abs(np.asarray(v, dtype=np.float64)).astype(LD) for v in (X, s, Zt)))


def f64_rows(X, s, Zt):
    return s[:, None] * (X @ Zt.T)


# ---- mutations: what a subtly wrong kernel would return, formed from the reference in its own arithmetic ----------------
def _row_term(X, T, n, off, V):
    """The contribution of row n with unit weight: outer(T[n], x_n) scattered at `off` (Q x V)."""
    out = np.zeros((T.shape[1], V), dtype=T.dtype)
    out[:, off:] = np.outer(T[n], X[n])
    return out


def weight_swap_row(c, live):
    """The first row with a non-zero term (`live`) whose neighbour (the zero padding behind the last row) carries another
    weight."""
    cpad = np.append(c, 0.0)
    return int(np.flatnonzero((cpad[:-1] != cpad[1:]) & live)[0])


def vector_swap_row(U):
    """The first vector whose neighbour (the zero padding behind the last vector) is another vector."""
    Upad = np.vstack([U, np.zeros((1, U.shape[1]))])
    return int(np.flatnonzero(np.any(Upad[:-1] != Upad[1:], axis=1))[0])


def full_mutations(case, ref, conv):
    """{name: mutated result} for the full form; `ref` = int_full / ld_full of `case`, `conv` casts the inputs to its dtype."""
    X, c, U = conv(case['X']), conv(case['c']), conv(case['U'])
    off, V, N = case['off'], case['U'].shape[1], case['X'].shape[0]
    T = np.einsum('nk,qk->nq', X, np.ascontiguousarray(U[:, off:]))          # unscaled
    out = {}
    out['last row dropped'] = ref - c[N - 1] * _row_term(X, T, N - 1, off, V)
    n = weight_swap_row(case['c'], np.any(T != 0, axis=1) & np.any(X != 0, axis=1))
    other = c[n + 1] if n + 1 < N else c[n] * 0
    out["neighbour's weight"] = ref + (other - c[n]) * _row_term(X, T, n, off, V)
    m = ref.copy(); m[:, [off, off + 1]] = m[:, [off + 1, off]]
    out['columns swapped'] = m
    q = vector_swap_row(case['U'])
    m = ref.copy(); m[q] = ref[q + 1] if q + 1 < ref.shape[0] else 0          # vector Q is the zero padding
    out["next vector's result"] = m
    out['row past N counted'] = ref + c[N - 1] * _row_term(X, T, N - 1, off, V)
    return out


def rows_mutations(X, s, Zt, ref, conv):
    """{name: mutated result} for the row form over all N rows (the row past N writes nothing here: four mutations)."""
    Xc, sc, Zc = conv(X), conv(s), conv(Zt)
    N = X.shape[0]
    out = {}
    m = ref.copy(); m[N - 1] = 0
    out['last row dropped'] = m
    n = weight_swap_row(s, np.any(ref != 0, axis=1))
    other = sc[n + 1] if n + 1 < N else sc[n] * 0
    m = ref.copy(); m[n] = other * (Zc @ Xc[n])
    out["neighbour's weight"] = m
    p = int(np.flatnonzero(np.any(Zt[:, :-1] != Zt[:, 1:], axis=0))[0])        # the first two columns that differ in Zt
    Zs = Zc.copy(); Zs[:, [p, p + 1]] = Zs[:, [p + 1, p]]
    out['columns swapped'] = _rows_product(Xc, sc, Zs)                        # (the contraction reads U one column off)
    q = vector_swap_row(Zt)
    m = ref.copy(); m[:, q] = ref[:, q + 1] if q + 1 < ref.shape[1] else 0
    out["next vector's result"] = m
    return out


def to_int(v):
    return np.asarray(v).astype(np.int64)


def to_ld(v):
    return np.asarray(v, dtype=np.float64).astype(LD)


def max_ratio(S, S_ref, bound):
    """Largest |S - S_ref| / bound over the entries (longdouble difference); a non-finite entry gives inf, an entry whose
    bound is zero must be exact."""
    err = np.abs(np.asarray(S).astype(LD) - S_ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, np.where(np.isfinite(err), err / bound, np.inf))
    return float(np.max(ratio))


def worst_entry(S, S_ref, bound):
    err = np.abs(np.asarray(S).astype(LD) - S_ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, np.where(np.isfinite(err), err / bound, np.inf))
    k = int(np.argmax(ratio))
    return tuple(int(i) for i in np.unravel_index(k, ratio.shape)), float(ratio.flat[k])


# ---- the shapes of tests/test_gpu_hvp_multi.py, replayed by the CPU file ------------------------------------------------
P_GRID = [2, 4, 30, 126, 128, 130, 254, 256, 258, 382, 384, 510, 512, 640, 768, 770, 896, 1022, 1024]      # NB = 1..8
Q_GRID = [1, 2, 7, 15, 16, 17, 33]
N_GRID = [1, 7, 8, 9, 17, 2047, 2048, 2049, 4097, 6145]


def _full_cases():
    cases = set()
    for P in P_GRID:                           # every width at one chunk, two chunks, and workgroup 0 taking a second chunk
        for N in (1, 9, 2049):
            cases.add((N, P, 16))
    for P in (2, 130, 1024):                   # every row count at the narrowest width, a 2-column tail block, the widest
        for N in N_GRID:
            cases.add((N, P, 16))
    for P in (130, 512):                       # every vector count (more than one 16-block at 17 and 33)
        for Q in Q_GRID:
            cases.add((2049, P, Q))
    return sorted(cases, key=lambda t: (t[1], t[0], t[2]))


FULL_CASES = _full_cases()                     # (N, P, Q)
GLM_OFF_CASES = [(2049, 130, 7), (9, 512, 16), (17, 2, 1)]      # (N, P, Q) with a 3-entry block in front: V = D = P + 3
GLM_OFF = 3

ROWS_N = 4099
ROWS_P = [2, 126, 130, 384, 640, 1024]
ROWS_Q = [1, 5, 16, 21]
ROWS_WINDOWS = [(0, 4099), (0, 1), (3, 12), (8, 16), (2041, 4099), (4091, 4099), (4098, 4099)]


def rows_case(kind, P, Q):
    """(X (ROWS_N x P), s (ROWS_N, non-zero on every row), Zt (Q x P)) of the row form; X and s are those of the width P
    whatever Q."""
    c = make_case(kind, ROWS_N, P, 1)
    return c['X'], c['c'], make_case(kind, 1, P, Q)['U']

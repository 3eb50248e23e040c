"""Launch geometry, inputs and plain references for the fused observation pass (csrc/k_glm.hip), used by
tests/test_gpu_glm_pass.py:

    value   f    = sum_n w_n l(y_n, z_n) + 1/2 (eta - m)^T diag(a) (eta - m),     z_n = x_n . beta
    grad    g    = X^T (w o l'(y, z)) scattered at the coefficient offset + a o (eta - m)
    rows    G[n] = l'(y_n, z_n) x_n                                                `ctx.obs_grad`
    HVP     H u  = X^T (cw o (X u)) + a o u,     cw_n = w_n l''(y_n, z_n) cached by the gradient pass

NumPy only: importable and runnable without the library, so tests/test_glm_pass_reference_host_math.py can show on the
CPU that every input is fair and every oracle sharp.  The layout is an unbounded box evaluated in vector coordinates, so
the packing Jacobian is exactly the identity and nothing stands between the test and the kernels.

Three routes (launch_glm_pass), all ending in the two-level fixed-order reducer:

    narrow   P <= 1024          glm_pass_kernel<NIT>, NIT = 1, 2, 4, 8; 2048 workgroups of 4 waves x 2 rows at most
    wide1    1025 .. 4096       glm_pass_wide1_kernel<NW, NIT>: <2,6>, <2,8>, <4,6>, <4,8>; the grid is what the chip holds
    wide2    P > 4096, or tuning bit 0 above 1024: glm_wide_rows_kernel + glm_wide_accum_kernel

The grid of wide1 is occupancy x compute units, asked of the runtime.  This module cannot know the occupancy; it knows
that it lies between 1 workgroup per compute unit and the hardware ceiling of 8 waves per SIMD (16 workgroups of two
waves, 8 of four, on each of 256 compute units).  `plan` therefore carries both ends: the ceiling chooses the row counts
of the multi-stage cases (N above four full rounds of the LARGEST possible grid: at least three stages whatever the
occupancy), and every rounding count takes the end that makes it larger (stages from the smallest grid, reducer chains
from the largest).

Two oracles:

  exact     small integers: X and beta in -3..3, y, a, m integers (no row with l' = 0), weights non-zero in -4..4, lik_info = 1, in one of four
            settings whose loss terms are exact in float64:
              gaussian      at an integer beta: l' = z - y, l'' = 1, l = d^2 / 2 -- integers and half-integers;
              logistic0     at beta = 0: sig = 1/2, l'' = 1/4 -- gradient, rows and HVP exact (the value is w log 2, not exact:
                            it is held to the bound below);
              poisson0      at beta = 0: e^z = 1 -- everything exact;
              logistic800   z a non-zero multiple of 800 (beta = 800 on the column of ones, +-1600 or 0 elsewhere, so
                            x . beta / 800 is odd): exp(-|z|) underflows to 0, sig is exactly 0 or 1, l'' = 0 and
                            l = max(z, 0) - y z.  Value and gradient exact, the HVP exactly the prior term.
            Every partial sum is a multiple of 1/4 below 2^51 (`partial_sum_ceiling`), so every summation order gives the
            same float64 and the device result must be BITWISE the int64 one.
  bounded   real data (columns of X over six decades, weights of mixed sign over four, |z| <= 30) against np.longdouble,
            entry by entry, under a first-order bound built from counted roundings (1 + d), |d| <= 2^-53:

              |g_j - ref_j| <= 2^-53 1.01 sum_n |w_n| |x_nj| ( K_acc |l'_n| + |l''_n| K_z sum_p |x_np beta_p| + L1_n ) + prior

            and the same pattern for the value (l, l') and the HVP (cw_n, |x_n . u|).  K_z: the per-lane products and
            additions, the group_sums butterfly, the NW - 1 joins of wide1, the 128-column chunk loop and wave_sum of
            wide2.  K_acc: the coefficient, one multiply and one addition per row of every stage the wave runs, the three
            wave joins (none on wide1), the reducer chains, the prior term joining, the reference rounded to float64.  A
            multiply and an addition count as two roundings: no FMA contraction is assumed.  L1_n (L0_n, L2_n) is the loss
            evaluation written out from `loss_eval` in `loss_roundings`; the device's exp and log1p get E_ULP = 2 ulp each
            (one ulp of margin over the 1 ulp that is believed, not verified, to be documented for both).

The mutations of the host-math file are the mistakes this kernel can make.  Each must change the integer result and leave
the bound by two orders of magnitude.
"""
import numpy as np

LD = np.longdouble
U_ROUND = 2.0 ** -53                      # unit roundoff of float64
SECOND_ORDER = 1.01
E_ULP = 2                                 # ulp allowed to the device's exp and log1p (an ulp is at most 2 U_ROUND relative)

GAUSSIAN, LOGISTIC, POISSON = 'gaussian', 'logistic', 'poisson'
LOSSES = (GAUSSIAN, LOGISTIC, POISSON)
INT_SETTINGS = ('gaussian', 'logistic0', 'poisson0', 'logistic800')
LOSS_OF = {'gaussian': GAUSSIAN, 'logistic0': LOGISTIC, 'poisson0': POISSON, 'logistic800': LOGISTIC}

PASS_MAX_COLS = 1024
NARROW_MAX_GRID = 2048
WIDE_ROWS = 2048                          # rows per block of the accumulation pass of wide2
WIDE2_MAX_GRID = 4096
N_CU = 256
WAVES_PER_CU_MAX = 32                     # 8 per SIMD


def cdiv(a, b):
    return -(-a // b)


# ---- what the launcher computes from (N, P, tuning bit 0) ----------------------------------------------------------
def route(P, two_pass=False):
    if P <= PASS_MAX_COLS:
        return 'narrow'
    return 'wide1' if P <= 4 * PASS_MAX_COLS and not two_pass else 'wide2'


def wide1_shape(P):
    """(NW, NIT) of the one-pass wide kernel."""
    return (2, 6) if P <= 1536 else (2, 8) if P <= 2048 else (4, 6) if P <= 3072 else (4, 8)


def wide1_slot_ceiling(P):
    """The largest grid the hardware could hold: 8 waves per SIMD."""
    return N_CU * (WAVES_PER_CU_MAX // wide1_shape(P)[0])


def plan(N, P, two_pass=False):
    """dict: route; nit / nw; rows per stage; grid_lo <= grid <= grid_hi of the main kernel; stages_lo / stages_hi a wave
    runs; nblk_lo / nblk_hi vector partials and nval_hi value partials handed to the reducer; rows_per_round (rows between
    two stages of one wave, for the largest grid)."""
    r = route(P, two_pass)
    pl = dict(route=r, N=N, P=P, rows_per_stage=2)
    if r == 'narrow':
        grid = max(1, min(NARROW_MAX_GRID, cdiv(cdiv(N, 2), 4)))
        pl.update(nit=1 if P <= 128 else 2 if P <= 256 else 4 if P <= 512 else 8, nw=4, grid_lo=grid, grid_hi=grid)
        pl['stages_lo'] = pl['stages_hi'] = cdiv(N, grid * 8)          # wave 0 of workgroup 0 runs the most
        pl['rows_per_round'] = grid * 8
        pl['nblk_lo'] = pl['nblk_hi'] = pl['nval_hi'] = grid
    elif r == 'wide1':
        nw, nit = wide1_shape(P)
        pairs = cdiv(N, 2)
        lo, hi = max(1, min(pairs, N_CU)), max(1, min(pairs, wide1_slot_ceiling(P)))
        pl.update(nit=nit, nw=nw, grid_lo=lo, grid_hi=hi, stages_lo=cdiv(N, 2 * hi), stages_hi=cdiv(N, 2 * lo),
                  rows_per_round=2 * hi, nblk_lo=lo, nblk_hi=hi, nval_hi=hi)
    else:
        grid1 = max(1, min(WIDE2_MAX_GRID, cdiv(N, 4)))
        pl.update(nit=cdiv(P, 128), nw=4, rows_per_stage=1, grid_lo=grid1, grid_hi=grid1)
        pl['stages_lo'] = pl['stages_hi'] = cdiv(N, grid1 * 4)
        pl['rows_per_round'] = grid1 * 4
        pl['nblk_lo'] = pl['nblk_hi'] = cdiv(N, WIDE_ROWS)
        pl['nval_hi'] = grid1
    pl['two_level'] = pl['nblk_hi'] >= 256
    return pl


def stage_boundaries(pl):
    """Rows at which a wave of the main kernel begins another stage (for both ends of the wide1 grid)."""
    N = pl['N']
    steps = {pl['rows_per_round']} | ({2 * pl['grid_lo']} if pl['route'] == 'wide1' else set())
    return sorted({b for s in steps for b in range(s, N, s)})[:8]


def block_of_row(pl, n, what='vec'):
    """The workgroup whose partial holds row n (largest grid of wide1); `what` = 'vec' or 'val' (they differ on wide2)."""
    n = np.asarray(n)
    if pl['route'] == 'narrow':
        return (n // 8) % pl['grid_hi']
    if pl['route'] == 'wide1':
        return (n // 2) % pl['grid_hi']
    return n // WIDE_ROWS if what == 'vec' else (n // 4) % pl['grid_hi']


# ---- counted roundings ----------------------------------------------------------------------------------------------
def _reduce_one_level(nblk):
    # a slice adds every eighth partial on four chains (the tail joins chain 0: up to 3 more), (s0 + s1) + (s2 + s3), then
    # the eight slices in order
    return cdiv(nblk, 8) // 4 + 3 + 2 + 7


def reducer_roundings(nblk):
    if nblk >= 256:
        return 16 + _reduce_one_level(cdiv(nblk, 16))
    return _reduce_one_level(nblk)


def value_reducer_roundings(nval):
    return cdiv(nval, 512) + 9                                    # a strided chain per thread, then the 512-wide tree


def k_z(pl):
    """Roundings a product x_np beta_p can meet on its way into z (the same for t = x . u)."""
    if pl['route'] == 'wide2':
        return 2 + cdiv(pl['P'], 128) + 6                         # product, pair sum, the chunk loop, wave_sum
    k = 2 + pl['nit'] + 6                                         # product, pair sum, the it loop, group_sums (2 swaps + 4 DPP)
    return k + (pl['nw'] - 1 if pl['route'] == 'wide1' else 0)


def _reducer_hi(pl):
    return max(reducer_roundings(pl['nblk_lo']), reducer_roundings(pl['nblk_hi']))


def k_acc(pl):
    """Roundings a term coef_n x_nj can meet on its way into an output entry (the coefficient's own product included)."""
    if pl['route'] == 'wide2':
        chain = min(WIDE_ROWS, pl['N'])
        chain = cdiv(chain, 4)                                    # a wave of the accumulation pass takes every fourth row
        joins = 3
    else:
        chain = 2 * pl['stages_hi']                               # two rows per stage
        joins = 3 if pl['route'] == 'narrow' else 0
    return 1 + 1 + chain + joins + _reducer_hi(pl) + 1 + 1        # coef, multiply, ..., the prior term joining, the reference


def k_val(pl):
    """Roundings a term w_n l_n can meet on its way into the value."""
    joins = 2 + (0 if pl['route'] == 'wide1' else 3)              # the rows of a stage, then the waves
    return 1 + pl['stages_hi'] + joins + value_reducer_roundings(pl['nval_hi']) + 1 + 1


def k_quad_value(V):
    return 2 + cdiv(V, 1024) + 10 + 1                             # a d, d (a d) / 2, the strided chain, the 1024-wide tree, the scale


K_QUAD_VEC = 2                                                    # a (eta - m) or a u, times the scale


# ---- the loss terms -------------------------------------------------------------------------------------------------
def loss_terms(loss, y, z):
    """(l, l', l'') in the dtype of z, by the formulas of `loss_eval`; l'' of the logistic loss as e / (1 + e)^2, which does
    not cancel."""
    if loss == GAUSSIAN:
        d = z - y
        return d * d / 2, d, np.ones_like(z)
    if loss == LOGISTIC:
        e = np.exp(-np.abs(z))
        sig = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
        return np.maximum(z, 0) + np.log1p(e) - y * z, sig - y, e / ((1 + e) * (1 + e))
    ez = np.exp(z)
    return ez - y * z, ez - y, ez


def loss_roundings(loss, y, z):
    """(L0, L1, L2, D1, D2) per row, float64: |l_hat - l| <= U (L0 + |l'| Ez), |l'_hat - l'| <= U (L1 + D1 Ez),
    |l''_hat - l''| <= U (L2 + D2 Ez) to first order, when z_hat = z + U Ez' with |Ez'| <= Ez.  Written out from loss_eval:

      gaussian  d = z - y (1); l' = lik d (lik = 1: exact); l = 0.5 lik d d: d twice (2) and two products (the factor 0.5
                is exact) -> 4; l'' exact.
      logistic  e = exp(-|z|): E ulp = 2 E U relative.  1 + e (1) and the division (1): 2 U sig; the error of e moves sig by
                sig (1 - sig) 2 E U.  l' = sig - y (1).  l'' = sig (1 - sig): the error ds of sig enters as |1 - 2 sig| ds, then
                1 - sig (1, absolute U (1 - sig) sig after the product) and the product (1).  l = (max(z, 0) + log1p(e)) - y z:
                log1p 2 E U log1p(e), the error of e moves it by 2 E U e / (1 + e), the sum (1), y z (1), the difference (1).
      poisson   ez = exp(z): 2 E U ez, in all three terms; l' = ez - y (1); l = ez - y z: the product (1), the difference (1).
    """
    y, z = np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64)
    l0, l1, l2 = loss_terms(loss, y, z)
    if loss == GAUSSIAN:
        return 4 * np.abs(l0), np.abs(l1), np.zeros_like(z), np.ones_like(z), np.zeros_like(z)
    if loss == LOGISTIC:
        e = np.exp(-np.abs(z))
        sig = l1 + y
        ds = 2 * sig + 2 * E_ULP * l2
        sp = np.maximum(z, 0) + np.log1p(e)
        L0 = 2 * E_ULP * np.log1p(e) + 2 * E_ULP * e / (1 + e) + sp + np.abs(y * z) + np.abs(l0)
        return L0, np.abs(l1) + ds, np.abs(1 - 2 * sig) * ds + 2 * l2, l2, l2 * np.abs(1 - 2 * sig)
    ez = l2
    return 2 * E_ULP * ez + np.abs(y * z) + np.abs(l0), 2 * E_ULP * ez + np.abs(l1), 2 * E_ULP * ez, ez, ez


# ---- inputs ---------------------------------------------------------------------------------------------------------
def case_seed(N, P, off, tag):
    return 1000003 * P + 7919 * N + 13 * off + 104729 * (1 + (INT_SETTINGS + LOSSES).index(tag))


def int_case(setting, N, P, off=0):
    """Small-integer inputs as float64: X (N x P, column 0 all ones), y, w (non-zero), beta (V = off + P), a, m (V), U (2 x V)."""
    rng = np.random.default_rng(case_seed(N, P, off, setting))
    V = off + P
    X = rng.integers(-3, 4, size=(N, P), dtype=np.int8).astype(np.float64)
    X[:, 0] = 1.0
    w = (rng.integers(1, 5, size=N) * rng.choice([-1, 1], size=N)).astype(np.float64)
    loss = LOSS_OF[setting]
    if loss == GAUSSIAN:
        y = rng.integers(-3, 4, size=N)
    elif loss == LOGISTIC:
        y = rng.integers(0, 2, size=N)
    else:
        y = rng.integers(0, 5, size=N)
    beta = rng.integers(-3, 4, size=V).astype(np.float64)
    if setting in ('logistic0', 'poisson0'):
        beta[off:] = 0.0
    elif setting == 'logistic800':
        beta[off:] = 1600.0 * rng.integers(-1, 2, size=P)
        beta[off] = 800.0
    # no row may hide behind a zero coefficient: l' = 0 is moved away (gaussian: y off z; poisson0: y off 1), and at
    # logistic800, where a correctly classified row has l = l' = 0, three rows of four are misclassified
    z = (X @ beta[off:]).astype(np.int64)
    if setting == 'gaussian':
        y = np.where(y == z, y + 1, y)
    elif setting == 'poisson0':
        y = np.where(y == 1, 5, y)
    elif setting == 'logistic800':
        y = np.where(np.arange(N) % 4 == 3, z > 0, z < 0).astype(np.int64)
    a = rng.integers(1, 5, size=V).astype(np.float64)
    m = rng.integers(-3, 4, size=V).astype(np.float64)
    U = rng.integers(-3, 4, size=(2, V)).astype(np.float64)
    return dict(kind='int', setting=setting, loss=loss, X=X, y=y.astype(np.float64), w=w, beta=beta, a=a, m=m, U=U, off=off)


Z_MAX = 30.0


def real_case(loss, N, P, off=0):
    """Same shapes: X normal with column j scaled by 10^s_j, s uniform in [-3, 3], column 0 all ones; weights of mixed sign,
    log-uniform over 1e-2 .. 1e2; y real (gaussian), 0/1 (logistic), counts (poisson); beta_j normal / 10^s_j, scaled down
    where needed so that |z| <= 30; the rows of U likewise on scales 10^v_q, v in [-2, 2]; a in 1..4, m = 0.  The row with
    the largest |w l'| stands last, so that nothing at the edge of the row range can hide below the other rows' rounding."""
    rng = np.random.default_rng(case_seed(N, P, off, loss) + 500000007)
    V = off + P
    scale = 10.0 ** rng.uniform(-3.0, 3.0, size=P)
    scale[0] = 1.0
    X = rng.normal(size=(N, P)) * scale
    X[:, 0] = 1.0
    w = rng.choice([-1.0, 1.0], size=N) * 10.0 ** rng.uniform(-2.0, 2.0, size=N)
    if loss == GAUSSIAN:
        y = rng.normal(size=N)
    elif loss == LOGISTIC:
        y = rng.integers(0, 2, size=N).astype(np.float64)
    else:
        y = rng.poisson(1.0, size=N).astype(np.float64)
    beta = rng.normal(size=V)
    beta[off:] /= scale
    zmax = float(np.max(np.abs(X @ beta[off:])))
    if zmax > Z_MAX:
        beta[off:] *= Z_MAX / zmax * (1.0 - 1e-9)
    U = rng.normal(size=(2, V)) * 10.0 ** rng.uniform(-2.0, 2.0, size=(2, 1))
    U[:, off:] /= scale
    a = rng.integers(1, 5, size=V).astype(np.float64)
    k = int(np.argmax(np.abs(w * loss_terms(loss, y, X @ beta[off:])[1])))
    for v in (X, y, w):
        v[[k, N - 1]] = v[[N - 1, k]]
    return dict(kind='real', setting=loss, loss=loss, X=X, y=y, w=w, beta=beta, a=a, m=np.zeros(V), U=U, off=off)


def make_case(tag, kind, N, P, off=0):
    return int_case(tag, N, P, off) if kind == 'int' else real_case(tag, N, P, off)


def partial_sum_ceiling(setting, N, P):
    """An upper bound of every |partial sum| of the integer case times 4 (all terms are multiples of 1/4): value, gradient,
    HVP and the prior term, whatever the order.  Must stay below 2^53."""
    zmax = {'gaussian': 9 * P, 'logistic0': 0, 'poisson0': 0, 'logistic800': 800 + 4800 * (P - 1)}[setting]
    l0 = {'gaussian': (zmax + 4) ** 2 / 2.0, 'logistic0': 1.0, 'poisson0': 1.0, 'logistic800': 2.0 * zmax}[setting]
    l1 = {'gaussian': zmax + 4, 'logistic0': 0.5, 'poisson0': 4.0, 'logistic800': 1.0}[setting]
    tmax = 9 * P
    prior = 4 * 6 * 6 * (P + 3)
    return 4.0 * max(4 * l0 * N + prior, 4 * l1 * 3 * N + 24, 4 * tmax * 3 * N + 12, zmax, tmax)


# ---- references -----------------------------------------------------------------------------------------------------
def _scatter(vec_P, off, V, dtype):
    out = np.zeros(V, dtype=dtype)
    out[off:] = vec_P
    return out


def _tmatvec(C, X):
    """C (Q x N) @ X (N x P) for the dtypes NumPy has no BLAS for (int64, longdouble): row blocks of X scaled and added, every
    access contiguous."""
    if X.dtype == np.float64:
        return C @ X
    out = np.zeros((C.shape[0], X.shape[1]), dtype=X.dtype)
    step = max(1, (1 << 18) // X.shape[1])
    for q in range(C.shape[0]):
        for r0 in range(0, X.shape[0], step):
            out[q] += (X[r0:r0 + step] * C[q, r0:r0 + step, None]).sum(axis=0)
    return out


def evaluate(case, dtype):
    """The formulas in `dtype` (np.longdouble: the reference; np.float64: an honest plain evaluation)."""
    conv = lambda v: np.asarray(v, dtype=np.float64).astype(dtype)
    X, y, w, beta, a, m, U = (conv(case[k]) for k in ('X', 'y', 'w', 'beta', 'a', 'm', 'U'))
    off, V = case['off'], case['beta'].size
    z = X @ beta[off:]
    l0, l1, l2 = loss_terms(case['loss'], y, z)
    r = beta - m
    cw = w * l2
    T = np.ascontiguousarray((X @ np.ascontiguousarray(U[:, off:].T)).T)      # 2 x N
    hvp = a[None, :] * U
    hvp[:, off:] += _tmatvec(cw[None, :] * T, X)
    return dict(z=z, l0=l0, l1=l1, l2=l2, lp=l1, cw=cw, T=T, ops=(X, y, w, beta),
                value=np.sum(w * l0) + np.sum(a * r * r) / 2,
                grad=_scatter(_tmatvec((w * l1)[None, :], X)[0], off, V, dtype) + a * r, hvp=hvp)


def obs_rows(case, lp, n0, n1, dtype):
    """Rows n0..n1 of `ctx.obs_grad` in vector coordinates: lp_n x_n at the coefficient offset, zero elsewhere."""
    off, V = case['off'], case['beta'].size
    out = np.zeros((n1 - n0, V), dtype=dtype)
    out[:, off:] = np.asarray(lp[n0:n1]).astype(dtype)[:, None] * case['X'][n0:n1].astype(dtype)
    return out


def int_terms(setting, y, z):
    """(2 l, 2 l', 4 l'') as int64 (l is None where it is not exact)."""
    if setting == 'gaussian':
        d = z - y
        return d * d, 2 * d, np.full_like(z, 4)
    if setting == 'logistic0':
        assert not np.any(z)
        return None, 1 - 2 * y, np.ones_like(z)
    if setting == 'poisson0':
        assert not np.any(z)
        return np.full_like(z, 2), 2 * (1 - y), np.full_like(z, 4)
    assert np.all(z % 800 == 0) and np.all(z != 0)
    return 2 * (np.maximum(z, 0) - y * z), 2 * ((z > 0).astype(np.int64) - y), np.zeros_like(z)


def _as_int(*arrs):
    out = []
    for v in arrs:
        vi = np.asarray(v).astype(np.int64)
        assert np.array_equal(vi, v), 'integer data expected'
        out.append(vi)
    return out


def int_evaluate(case):
    """The exact oracle in int64, returned as float64 (every entry a multiple of 1/4 below 2^51: the division is exact).
    value is None for 'logistic0'."""
    X, y, w, beta, a, m, U = _as_int(*(case[k] for k in ('X', 'y', 'w', 'beta', 'a', 'm', 'U')))
    off, V = case['off'], beta.size
    z = X @ beta[off:]
    t0, t1, t2 = int_terms(case['setting'], y, z)
    r = beta - m
    out = dict(z=z, t0=t0, t1=t1, t2=t2, ops=(X, y, w, beta))
    out['value_n'] = None if t0 is None else int(np.sum(w * t0) + np.sum(a * r * r))
    out['grad_n'] = _scatter(_tmatvec((w * t1)[None, :], X)[0], off, V, np.int64) + 2 * a * r
    T = np.ascontiguousarray((X @ np.ascontiguousarray(U[:, off:].T)).T)
    hvp_n = 4 * a[None, :] * U
    hvp_n[:, off:] += _tmatvec((w * t2)[None, :] * T, X)
    out['value'] = None if t0 is None else out['value_n'] / 2.0
    out['grad'] = out['grad_n'] / 2.0
    out['hvp'] = hvp_n / 4.0
    out['lp'] = t1 / 2.0
    out['cw'] = (w * t2) / 4.0
    return out


# ---- the bound --------------------------------------------------------------------------------------------------------
def bounds(case, pl):
    """Entry-wise bounds (float64) of value, grad (V), hvp (2 x V), and per row of lp; `rows` gives the bound of a window
    of `ctx.obs_grad`."""
    X, y, w, beta, a, m, U = (np.asarray(case[k], dtype=np.float64) for k in ('X', 'y', 'w', 'beta', 'a', 'm', 'U'))
    off, V = case['off'], beta.size
    aX, aw = np.abs(X), np.abs(w)
    z = X @ beta[off:]
    l0, l1, l2 = loss_terms(case['loss'], y, z)
    L0, L1, L2, D1, D2 = loss_roundings(case['loss'], y, z)
    Kz, Ka, Kv = k_z(pl), k_acc(pl), k_val(pl)
    Ez = Kz * (aX @ np.abs(beta[off:]))
    r = beta - m
    f = U_ROUND * SECOND_ORDER
    dl1 = L1 + D1 * Ez                                             # |lp_hat - lp| / U
    out = dict(dl1=dl1, off=off, V=V, X=X, l1=l1)
    out['value'] = f * (np.sum(aw * (np.abs(l1) * Ez + L0 + Kv * np.abs(l0))) + k_quad_value(V) * np.sum(a * r * r) / 2)
    out['grad'] = f * (_scatter((aw * (dl1 + Ka * np.abs(l1))) @ aX, off, V, np.float64) + (K_QUAD_VEC + 1) * np.abs(a * r))
    T = U[:, off:] @ X.T
    Et = Kz * (np.abs(U[:, off:]) @ aX.T)
    dcw = aw * (L2 + D2 * Ez + np.abs(l2))                         # |cw_hat - cw| / U: the curvature, then its product with w
    coef = dcw[None, :] * np.abs(T) + np.abs(w * l2)[None, :] * (Et + Ka * np.abs(T))
    hv = (K_QUAD_VEC + 1) * np.abs(a[None, :] * U)
    hv[:, off:] += coef @ aX
    out['hvp'] = f * hv
    return out


def obs_rows_bound(b, n0, n1):
    """lp_n x_n: the error of lp_n, the product, the scaling by one, the reference rounded."""
    out = np.zeros((n1 - n0, b['V']))
    aX = np.abs(b['X'][n0:n1])
    out[:, b['off']:] = U_ROUND * SECOND_ORDER * (b['dl1'][n0:n1, None] + 3 * np.abs(b['l1'][n0:n1, None])) * aX
    return out


def worst_entry(S, S_ref, bound):
    """(index, ratio) of the largest |S - S_ref| / bound (longdouble difference); a non-finite entry gives inf, an entry
    whose bound is zero must be exact."""
    err = np.abs(np.atleast_1d(np.asarray(S)).astype(LD) - np.atleast_1d(S_ref))
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, np.where(np.isfinite(err), err / np.atleast_1d(bound), np.inf))
    k = int(np.argmax(ratio))
    return tuple(int(i) for i in np.unravel_index(k, ratio.shape)), float(ratio.flat[k])


def max_ratio(S, S_ref, bound):
    return worst_entry(S, S_ref, bound)[1]


# ---- mutations: what a subtly wrong kernel would return, formed from the reference in its own arithmetic ------------------
MUTATIONS = ('last row dropped', 'row past N counted', "stage partner's y and w", "previous stage's z",
             "one wave's columns missing from z", 'columns exchanged', 'last block missing from the reducer',
             "one workgroup's value partial missing")


def mutations(case, pl, ev):
    """(reference, {name: (value, grad)}) of the mistakes that apply at this shape, in the arithmetic of `ev`:
    int_evaluate(case) (the numerators: twice the value and the gradient, int64; the Gaussian setting, whose terms are exact
    at every z) or evaluate(case, LD).  The free choices (which pair of rows, which stage) fall on the row where the mistake
    moves the coefficient most."""
    off, V = case['off'], case['beta'].size
    N, P = case['X'].shape
    X, y, w, beta = ev['ops']
    if 'grad_n' in ev:
        assert case['setting'] == 'gaussian'
        terms = lambda yy, zz: int_terms(case['setting'], yy, zz)[:2]
        value, grad, dt = ev['value_n'], ev['grad_n'], np.int64
    else:
        terms = lambda yy, zz: loss_terms(case['loss'], yy, zz)[:2]
        value, grad, dt = ev['value'], ev['grad'], LD
    z = ev['z']
    t0, t1 = terms(y, z)
    c0, c1 = w * t0, w * t1

    def dgrad(rows, dc):
        return _scatter(np.atleast_1d(dc) @ X[np.atleast_1d(rows)], off, V, dt)

    def best(delta):
        return int(np.argmax(np.abs(np.asarray(delta, dtype=np.float64))))

    out = {}
    out['last row dropped'] = (value - c0[N - 1], grad - dgrad(N - 1, c1[N - 1]))
    out['row past N counted'] = (value + c0[N - 1], grad + dgrad(N - 1, c1[N - 1]))
    if N >= 2:
        rows = np.arange(N - N % 2)
        n0, n1 = terms(y[rows ^ 1], z[rows])
        d0, d1 = w[rows ^ 1] * n0 - c0[rows], w[rows ^ 1] * n1 - c1[rows]
        k = best(d1)
        if d1[k] != 0:
            out["stage partner's y and w"] = (value + d0[k], grad + dgrad(rows[k], d1[k]))
    step = pl['rows_per_round'] if pl['rows_per_round'] < N else 2
    if N > step:
        rows = np.arange(step, N)
        n0, n1 = terms(y[rows], z[rows - step])
        d0, d1 = w[rows] * n0 - c0[rows], w[rows] * n1 - c1[rows]
        k = best(d1)
        if d1[k] != 0:                                             # (a single column of ones gives every row the same z)
            out["previous stage's z"] = (value + d0[k], grad + dgrad(rows[k], d1[k]))
    if P >= 2:
        lo = pl['nit'] * 128 if pl['route'] == 'wide1' else P // 2
        hi = min(P, 2 * lo) if pl['route'] == 'wide1' else P
        n0, n1 = terms(y, z - X[:, lo:hi] @ beta[off + lo:off + hi])
        d0, d1 = w * n0 - c0, w * n1 - c1
        k = best(d1)
        if d1[k] != 0:
            out["one wave's columns missing from z"] = (value + d0[k], grad + dgrad(k, d1[k]))
        j = off + int(np.flatnonzero(grad[off:-1] != grad[off + 1:])[0]) if np.any(grad[off:-1] != grad[off + 1:]) else None
        if j is not None:
            g = grad.copy()
            g[[j, j + 1]] = g[[j + 1, j]]
            out['columns exchanged'] = (value, g)
    rows = np.flatnonzero(block_of_row(pl, np.arange(N), 'vec') == block_of_row(pl, N - 1, 'vec'))
    out['last block missing from the reducer'] = (value, grad - dgrad(rows, c1[rows]))
    rows = np.flatnonzero(block_of_row(pl, np.arange(N), 'val') == block_of_row(pl, N - 1, 'val'))
    out["one workgroup's value partial missing"] = (value - np.sum(c0[rows]), grad)
    return dict(value=value, grad=grad), out


def small_column_mutation(case, ev, limit):
    """One row's term missing from the gradient entry of the smallest column of X: the largest such term below `limit`.
    Returns (mutated gradient, entry index)."""
    off = case['off']
    j = 1 + int(np.argmin(np.max(np.abs(case['X'][:, 1:]), axis=0)))
    term = (ev['l1'] * case['w'].astype(LD)) * case['X'][:, j].astype(LD)
    ok = np.abs(term) < limit
    n = int(np.argmax(np.where(ok, np.abs(term), -1.0)))
    g = ev['grad'].copy()
    g[off + j] -= term[n]
    return g, off + j


# ---- the shapes of tests/test_gpu_glm_pass.py, replayed by the CPU file ----------------------------------------------------
NARROW_P = [1, 2, 3, 127, 128, 129, 130, 255, 256, 257, 258, 511, 512, 513, 514, 770, 1022, 1023, 1024]
NARROW_P_GRID_N = [1, 9, 2049]
NARROW_N_GRID_P = [2, 130]
NARROW_N = [1, 2, 3, 7, 8, 9, 65, 257, 2039, 2040, 2041, 2049, 4353, 16383, 16384, 16385, 16386, 16391, 32767, 32769, 49153]
NARROW_N_AT_1024 = [16385, 32769]
WIDE1_P = [1026, 1153, 1536, 1538, 2047, 2048, 2050, 3001, 3072, 3074, 4095, 4096]
WIDE1_N = [1, 2, 3, 1001]
WIDE1_MULTI_P = [1026, 2048, 2050, 4096]
WIDE1_TWO_PASS_N = 1001
WIDE2_P = [4097, 4098, 4224, 4225]
WIDE2_N = [1, 5, 2047, 2048, 2049, 4097]
WIDE2_FORCED = [(16389, 1026), (4097, 1026)]                    # (N, P) under tuning bit 0
ADOPTED_P = [130, 1024, 2048, 4098]
ADOPTED_N = [9, 2049]
PRE_BLOCK_P = [130, 1026]
PRE_BLOCK_N = 2049
GLM_OFF = 3
ZERO_WEIGHTS = (2049, 130)
REAL_N = [9, 2049]
REAL_EXTRA = [(16391, 130)]
GAUSSIAN_ONLY_ABOVE = 16384                                       # row counts above this run the Gaussian setting only ...
GAUSSIAN_ONLY_ENTRIES = 9000000                                   # ... and so do designs of more entries (4097 rows above 4096 columns)


def wide1_multi_N(P):
    """Four full rounds of the largest grid the hardware could hold, plus 1 and plus 2 rows: at least three stages with
    dead slots, an odd tail of one live row and an even one, whatever the occupancy."""
    base = 4 * wide1_slot_ceiling(P)
    return [base + 1, base + 2]


def int_settings_at(N, P):
    """The exact settings a shape runs: all four where it is small; the Gaussian one alone (the only one whose z varies)
    at the large ones, which are there for the row axis."""
    return ('gaussian',) if N > GAUSSIAN_ONLY_ABOVE or N * P > GAUSSIAN_ONLY_ENTRIES else INT_SETTINGS


def int_shapes():
    """Every (N, P, two_pass, off) of an integer case of the GPU file."""
    s = set()
    s.update((N, P, False, 0) for P in NARROW_P for N in NARROW_P_GRID_N)
    s.update((N, P, False, 0) for P in NARROW_N_GRID_P for N in NARROW_N)
    s.update((N, 1024, False, 0) for N in NARROW_N_AT_1024)
    s.update((N, P, False, 0) for P in WIDE1_P for N in WIDE1_N)
    s.update((N, P, False, 0) for P in WIDE1_MULTI_P for N in wide1_multi_N(P))
    s.update((WIDE1_TWO_PASS_N, P, True, 0) for P in WIDE1_P)
    s.update((N, P, False, 0) for P in WIDE2_P for N in WIDE2_N)
    s.update((N, P, True, 0) for (N, P) in WIDE2_FORCED)
    s.update((N, P, False, 0) for P in ADOPTED_P for N in ADOPTED_N)
    s.update((PRE_BLOCK_N, P, False, GLM_OFF) for P in PRE_BLOCK_P)
    s.add(ZERO_WEIGHTS + (False, 0))
    return sorted(s, key=lambda t: (t[1], t[0], t[2], t[3]))


def real_shapes():
    """Every (N, P, two_pass, off) of a real-data case of the GPU file (each runs the three losses)."""
    s = set((N, P, False, 0) for P in NARROW_P + WIDE1_P + WIDE2_P for N in REAL_N)
    s.update((N, P, False, 0) for (N, P) in REAL_EXTRA)
    s.update((PRE_BLOCK_N, P, False, GLM_OFF) for P in PRE_BLOCK_P)
    return sorted(s, key=lambda t: (t[1], t[0], t[2], t[3]))


def obs_windows(pl, V):
    """Windows of `ctx.obs_grad`: the head, the tail and one across each stage boundary; at most 4096 rows and about two
    million entries each."""
    N = pl['N']
    rows = max(16, min(4096, (1 << 21) // V))
    wins = {(0, min(N, rows)), (max(0, N - rows), N)}
    for b in stage_boundaries(pl):
        wins.add((max(0, b - 16), min(N, b + 16)))
    return sorted(wins)

"""Reference for the per-row kernels of the mixture model (`csrc/k_mixture_rows.h`): values, local gradient, statistics and
the Schur operand of simplex rows, row by row.  NumPy, longdouble and mpmath only; nothing here touches a GPU, the product or
`oracle/mixture.py`.  Used by tests/test_gpu_mixture_rows.py; tests/test_mixture_rows_reference_host_math.py
shows on the CPU that it agrees with the oracle and with exact AD, that every builder stays inside its design, and calibrates the
conditioning-limited bound.

Row n:  logits l = [0, f_n], p = softmax(l), s = x~_n Lam (x~ = (1, x_n)), g = -w (s - log p - 1),
    val2 = [-sum w p.s, sum w p.log p],   gz_j = p_{j+1} (g_{j+1} - g.p),
    H_nn[i, j] = d_ij p_i (w + g_i - g.p) + p_i p_j (2 g.p - w - g_i - g_j)     (i, j = 1 .. K-1; derived in `mp_row`)
    J[k, i] = p_k (d_ki - p_i),   A_n = J H_nn^-1 J^T  (K x K),
    S64 = U^T diag(w) U with U = [x~ (32) | p (32)],   R[(j, j'), (k, k')] = sum_n w_n^2 x~_nj x~_nj' A_n[k, k'].

Three evaluations share the formulas:
  `evaluate`            vectorised; p, log p, s, g, the sums and their entry-wise bounds in longdouble, A_n in float64 from the
                        scaled block of the kernel's coordinates (LAPACK, batched);
  `mp_row`              one row in mpmath, in the ORIGINAL coordinates (reference category 0, no scaling) at a precision that
                        covers the conditioning 1 / p_min of that form: the truth for probes and for the calibration;
  `woodbury_A`, `scaled_cholesky_A`   float64 restatements of the two device routes, written from the kernel's comments.

Bounds.  Sums and the gradient: |got - ref| <= U * 1.01 * B, B a running first-order count in units of U = 2^-53 of the roundings
in the kernel text (the constants below name each count).  A_n and R: conditioning-limited, e_n = max |A^ - A|_kk' / sqrt(A_kk
A_k'k') <= 8 unit_n, unit_n = max(U kappa_n, the measured e_n of the float64 restatement of the row's route); where the truth of
a row is too expensive (N K^2 > LD_BUDGET: the K = 32 cases of 32771 and 65539 rows), unit_n = U kappa_n max(1, CAL) with CAL the
calibration maximum of e / (U kappa) recorded below.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import mpmath as mp

LD = np.longdouble
U = 2.0 ** -53
SLACK = 1.01
E_ULP = 2                      # the project's figure for the device's exp and log, in ulp
EXPU = 2 * E_ULP               # ... in units of U: an ulp is 2 U
K_HALF = 5                     # mx_half_sum: four DPP steps and one permlane swap = five additions on the way of every term
K_WAVE = 6                     # mx_wave_sum: six butterfly levels
K_WG = 3                       # ((v0 + v1) + v2) + v3 over the four waves of a workgroup
A_FACTOR = 8                   # the device's allowance in units of unit_n (2-ulp exp / log, reduction trees, MFMA order)
FAST_THRESHOLD = 0.05          # the kernel takes the Woodbury route when dmin > 0.05 w
DENSE_BAND = (0.005, 0.04)     # designed dmin / w of a dense row
FAST_MIN = 0.2                 # ... and of a fast row: nothing in between, so no rounding flips a route
MAX_GRID, DENSE_MAX_GRID = 4096, 2048

# Calibration maxima of e / (U kappa) of the float64 restatement of a row's route, per route and K, rounded up to an integer:
# over ALL rows of every case of the GPU file with N K^2 <= LD_BUDGET (truth: the longdouble Woodbury form, itself checked
# against mpmath), over 8192 rows (largest kappa, even strides, probes) of the two larger K = 32 cases.  The row with
# p_min ~ 1e-200 is left out (see CAL_SAT200).  tests/test_mixture_rows_reference_host_math.py::test_calibration asserts them.
CAL = {('fast', 7): 8, ('fast', 13): 14, ('fast', 25): 11, ('fast', 31): 6, ('fast', 2): 7, ('fast', 3): 7, ('fast', 4): 10, ('fast', 5): 48, ('fast', 8): 8, ('fast', 17): 24, ('fast', 32): 76,
       ('dense', 2): 27, ('dense', 4): 6, ('dense', 5): 32, ('dense', 8): 8, ('dense', 17): 31, ('dense', 32): 82}
# logits 461 apart: the rounding of l - max alone is 461 U on the small probabilities in any float64 evaluation (measured: 203,
# 358 and 526 U kappa at kappa = 1); such a row is bounded by its own measured unit, never by CAL
CAL_SAT200 = 4 * 461


def k_s(V):
    """s = sum_{j <= V} x~_j Lam_jk: V + 1 products and additions in sequence, and the reference's rounding."""
    return V + 2


def trips(N):
    grid = min(MAX_GRID, ((N + 1) // 2 + 3) // 4)
    return -(-((N + 1) // 2) // (4 * grid)), grid


def k_val(N):
    """Additions on the way of one term of val2: the lane's running sum over its trips, the wave butterfly, the four waves,
    then mixture_val_reduce_kernel: ceil(grid / 256) per thread, a butterfly, four waves; and the reference's rounding."""
    t, grid = trips(N)
    return t + K_WAVE + K_WG + -(-grid // 256) + K_WAVE + K_WG + 1


def k_gram(N):
    """S64 by the narrow Gram kernel (64 columns): stages of 16 rows, min(1024, ceil(stages / 8)) workgroups; whatever the order
    inside a workgroup, a term meets at most its workgroup's rows + 4 additions, then at most `grid` in the reduction of the
    block partials; fl(w u) is one more and the reference's rounding another."""
    stages = -(-N // 16)
    grid = max(1, min(1024, -(-stages // 8)))
    return 16 * -(-stages // grid) + 4 + grid + 2


def k_gemm(N, V, K):
    """The N-term sum of R = Xk^T Amat (rows per split + splits + 2, edge slots + 3, generated operand
    + 1), one rounding for x~_j x~_j' where the operand is written out, one for the w^2 A of the row kernel, one for this
    reference's A_n rounded to float64."""
    import kron_atb_reference as kr
    q, lda = V + 1, K * (K + 1) // 2
    ldk, lda = q * (q + 1) // 2 + (q * (q + 1) // 2 & 1), lda + (lda & 1)
    mode = 2 if (V == 31 and K == 32) else 1
    return float(np.max(kr.atb_K(N, ldk, lda, mode))) + 3


# ---- the row quantities, vectorised ----------------------------------------------------------------------------------------
def _prelude(fz, x, w, lam, dtype):
    fz = np.asarray(fz, dtype=np.float64)
    N, KM = fz.shape
    K = KM + 1
    ell = np.zeros((N, K), dtype=dtype)
    ell[:, 1:] = fz
    d = ell - ell.max(axis=1, keepdims=True)
    ex = np.exp(d)
    den = ex.sum(axis=1, keepdims=True)
    p = ex / den
    logden = np.log(den)
    logp = d - logden
    xt = np.hstack([np.ones((N, 1)), np.asarray(x, dtype=np.float64)]).astype(dtype)
    lam = np.asarray(lam, dtype=dtype)
    wc = np.asarray(w, dtype=dtype)[:, None]
    s = xt @ lam
    g = -wc * (s - logp - 1)
    gdotp = (g * p).sum(axis=1, keepdims=True)
    return dict(N=N, K=K, d=d, den=den, logden=logden, p=p, logp=logp, xt=xt, lam=lam, w=wc, s=s, g=g, gdotp=gdotp,
                m=np.argmax(ell, axis=1))                 # the first maximum, as the kernel's __ffs


def swap_perm(m, K):
    """perm[n]: categories 0 and m_n change places (an involution)."""
    perm = np.tile(np.arange(K), (m.size, 1))
    perm[np.arange(m.size), m] = 0
    perm[:, 0] = m
    return perm


def scaled_block(p, g, w, m, want_M=True):
    """The kernel's coordinates: reference category m (arg-max), D-scaling.  Returns ps, d (N, K-1), M (N, K-1, K-1) and
    Jhat (N, K, K-1) = J D^-1 with  M_ij = r_i r_j (2 g.p - w - g_i - g_j) + d_ij d_i,  Jhat[k, i] = r_i (d_ki - p_k)."""
    N, K = p.shape
    perm = swap_perm(m, K)
    ps, gs = np.take_along_axis(p, perm, 1), np.take_along_axis(g, perm, 1)
    w = np.asarray(w, dtype=p.dtype).reshape(N, 1)
    gp = (g * p).sum(axis=1, keepdims=True)
    d = w + gs[:, 1:] - gp
    if not want_M:
        return perm, ps, d, None, None
    r = np.sqrt(ps[:, 1:])
    M = r[:, :, None] * r[:, None, :] * ((2 * gp - w)[:, :, None] - gs[:, 1:, None] - gs[:, None, 1:])
    idx = np.arange(K - 1)
    M[:, idx, idx] += d
    Jhat = -ps[:, :, None] * r[:, None, :]
    Jhat[:, idx + 1, idx] += r
    return perm, ps, d, M, Jhat


def _unswap(A, perm):
    A = np.take_along_axis(A, perm[:, :, None], 1)
    return np.take_along_axis(A, perm[:, None, :], 2)


def scaled_cholesky_A(p, g, w, m=None, blk=None):
    """Dense route, from the kernel's header comment: M = D^-1 H D^-1 = L L^T, Y = L^-1 (J D^-1)^T, A = Y^T Y, in the
    coordinates with the arg-max category as the reference; float64, batched LAPACK.  Raises LinAlgError on a row that is not
    positive definite."""
    m = np.argmax(p, axis=1) if m is None else m
    perm, _, _, M, Jhat = scaled_block(p, g, w, m) if blk is None else blk
    L = np.linalg.cholesky(M)
    Y = np.linalg.solve(L, np.swapaxes(Jhat, 1, 2))          # (N, K-1, K)
    return _unswap(np.swapaxes(Y, 1, 2) @ Y, perm)


def woodbury_terms(p, g, w, m, blk=None):
    N, K = p.shape
    perm, ps, d = (scaled_block(p, g, w, m, want_M=False) if blk is None else blk)[:3]
    w = np.asarray(w, dtype=p.dtype).reshape(N, 1)
    t = np.zeros_like(ps)
    t[:, 1:] = ps[:, 1:] / d
    alpha = t.sum(axis=1, keepdims=True)
    sumq = ps[:, 1:].sum(axis=1, keepdims=True)
    beta = sumq - 0.5 * w * alpha
    gamma = (ps[:, 1:] * d).sum(axis=1, keepdims=True) - w * sumq + 0.25 * w * w * alpha
    det = alpha * gamma - (beta - 1) * (beta - 1)
    return perm, ps, t, alpha, beta, gamma, det, w


def woodbury_A(p, g, w, m=None):
    """Fast route, from the comment in mixture_rows_kernel: M = Dg - r s^T - s r^T, a diagonal plus a rank-two term, so
    A = diag(t) - t p^T - p t^T + alpha p p^T - [a1 a2] T^-1 [a1 a2]^T; float64."""
    m = np.argmax(p, axis=1) if m is None else m
    perm, ps, t, alpha, beta, gamma, det, w = woodbury_terms(p, g, w, m)
    K = p.shape[1]
    a1 = t - alpha * ps
    a2 = ps - 0.5 * w * t - beta * ps
    a2[:, 0] = -beta[:, 0] * ps[:, 0]
    t11, t12, t22 = gamma / det, (1 - beta) / det, alpha / det
    A = -(t[:, :, None] * ps[:, None, :]) - ps[:, :, None] * t[:, None, :] + alpha[:, :, None] * ps[:, :, None] * ps[:, None, :]
    idx = np.arange(K)
    A[:, idx, idx] += t
    b1, b2 = a1 * t11 + a2 * t12, a1 * t12 + a2 * t22
    A -= a1[:, :, None] * b1[:, None, :] + a2[:, :, None] * b2[:, None, :]
    return _unswap(A, perm)


def routing(p, g, w, m, want_eig=True, blk=None):
    """dmin / w, det T, and the smallest eigenvalue, the 2-norm and the condition number of the scaled block M, per row."""
    blk = scaled_block(p, g, w, m) if blk is None else blk
    d, M = blk[2], blk[3]
    w = np.asarray(w, dtype=np.float64).ravel()
    with np.errstate(divide='ignore', invalid='ignore'):
        out = dict(dmin_w=np.where(w > 0, d.min(axis=1) / np.where(w > 0, w, 1.0), -np.inf))
    out['det'] = woodbury_terms(p, g, w, m, blk)[6][:, 0]
    if want_eig:
        ev = np.linalg.eigvalsh(M)
        out['eig_min'], out['norm'] = ev[:, 0], np.max(np.abs(ev), axis=1)
        with np.errstate(divide='ignore'):
            out['kappa'] = np.where(ev[:, 0] > 0, out['norm'] / np.where(ev[:, 0] > 0, ev[:, 0], 1.0), np.inf)
    return out


def _pool():
    return ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1)))      # LAPACK and BLAS release the GIL


def routing_chunked(p, g, w, m, chunk=4096):
    w = np.asarray(w, dtype=np.float64).ravel()
    with _pool() as pool:
        parts = list(pool.map(lambda c: routing(p[c:c + chunk], g[c:c + chunk], w[c:c + chunk], m[c:c + chunk]), range(0, p.shape[0], chunk)))
    return {k: np.concatenate([r[k] for r in parts]) for k in parts[0]}


def tri_pairs(q):
    a, b = np.tril_indices(q)
    return a, b


LD_BUDGET = 1e7               # N K^2 up to which A_n of `evaluate` is the Woodbury form in longdouble


def evaluate(fz, x, w, lam, want_A=True, keep_A=None, chunk=4096, units=None, truth=None):
    """Everything the row kernels return for (fz (N, K-1), x (N, V), w (N), lam (V+1, K)), with the entry-wise bounds.
    want_A=False stops before the factorisations (values, gradient, statistics only); keep_A: rows whose A_n is returned;
    units: {row: unit_n} of rows whose unit was measured against the truth (probes), truth: {row: A_n} from mp_row for them.
    A_n is the Woodbury form evaluated in longdouble (2^-11 of the float64 restatements' error) where N K^2 <= LD_BUDGET, and
    the float64 scaled Cholesky otherwise; there the bound of R carries one more unit_n per row for the reference itself."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    N, V = x.shape
    P = _prelude(fz, x, w, lam, LD)
    K, q = P['K'], V + 1
    p, logp, g, gdotp, wc = P['p'], P['logp'], P['g'], P['gdotp'], P['w']
    f = lambda a: np.asarray(a, dtype=np.float64)
    # ---- roundings, in units of U (first order; SLACK takes the rest) -----------------------------------------------------
    absd = np.abs(f(P['d']))
    rel_ex = EXPU + absd                                      # exp and the rounding of l - max (U |l - max| on the argument)
    rel_den = (f(p) * rel_ex).sum(axis=1, keepdims=True) + K_HALF
    rel_p = rel_ex + rel_den + 1                              # the quotient
    abs_logp = absd + rel_den + EXPU * np.abs(f(P['logden'])) + np.abs(f(logp))
    sabs = f(np.abs(P['xt']) @ np.abs(P['lam']))
    abs_s = k_s(V) * sabs
    G = f(wc) * (sabs + np.abs(f(logp)) + 1.0)                # the absolute terms of g
    abs_g = f(wc) * (abs_s + abs_logp) + 3 * G                # two subtractions and the product by w
    agp = np.abs(f(g * p))
    Gp = G * f(p)
    abs_gdotp = (abs_g * f(p) + Gp * (rel_p + 1)).sum(axis=1, keepdims=True) + K_HALF * Gp.sum(axis=1, keepdims=True)
    out = dict(N=N, V=V, K=K, m=P['m'], z=f(p), rel_p=rel_p, p_ld=p, g_ld=g)
    gz = p[:, 1:] * (g[:, 1:] - gdotp)
    out['gz'] = f(gz)
    out['gz_bound'] = U * SLACK * (f(p[:, 1:]) * (abs_g[:, 1:] + abs_gdotp + (G[:, 1:] + Gp.sum(axis=1, keepdims=True)) * (2 + rel_p[:, 1:]))
                                   + np.abs(out['gz']))
    # ---- val2 ------------------------------------------------------------------------------------------------------------
    t_lin, t_ent = -wc * p * P['s'], wc * p * logp
    out['val2'] = np.array([float(t_lin.sum()), float(t_ent.sum())])
    kv = k_val(N)
    wp = f(wc * p)
    b_lin = (wp * sabs * (rel_p + 2) + wp * abs_s).sum() + kv * (wp * sabs).sum()
    b_ent = (np.abs(f(t_ent)) * (rel_p + 2) + wp * abs_logp).sum() + kv * np.abs(f(t_ent)).sum()
    out['val2_bound'] = U * SLACK * np.array([b_lin, b_ent])
    # ---- S64 -------------------------------------------------------------------------------------------------------------
    Uq = np.hstack([P['xt'], p])                              # the q + K columns that are not padding
    rel_u = np.hstack([np.zeros((N, q)), rel_p])
    S = Uq.T @ (wc * Uq)
    Ua = np.abs(f(Uq))
    Sabs = Ua.T @ (f(wc) * Ua)
    Srel = (Ua * rel_u).T @ (f(wc) * Ua)
    cols = np.concatenate([np.arange(q), 32 + np.arange(K)])
    S64, B64 = np.zeros((64, 64)), np.zeros((64, 64))
    S64[np.ix_(cols, cols)] = f(S)
    B64[np.ix_(cols, cols)] = U * SLACK * (k_gram(N) * Sabs + Srel + Srel.T)
    out['S64'], out['S64_bound'] = S64, B64
    if not want_A:
        return out
    # ---- A_n, row by row, and R --------------------------------------------------------------------------------------------
    p64, g64 = f(p), f(g)
    cal = np.array([max(1.0, CAL.get(('dense' if dn else 'fast', K), np.nan)) for dn in (False, True)])
    parts = []
    ld_A = N * K * K <= LD_BUDGET
    P64 = _prelude(fz, x, w, lam, np.float64) if ld_A else None
    out['ld_A'] = ld_A
    ja, jb = tri_pairs(q)
    ka, kb = tri_pairs(K)
    Rp, Rb, Ra = (np.zeros((ja.size, ka.size)) for _ in range(3))
    keep = {} if keep_A is None else {int(n): None for n in keep_A}
    xt64 = f(P['xt'])
    w2 = w * w

    def work(c0):
        sl = slice(c0, min(N, c0 + chunk))
        blk = scaled_block(p64[sl], g64[sl], w[sl], P['m'][sl])
        rt = routing(p64[sl], g64[sl], w[sl], P['m'][sl], blk=blk)
        rt['dense'] = ~(rt['dmin_w'] > FAST_THRESHOLD)
        rt['unit'] = U * rt['kappa'] * cal[rt['dense'].astype(int)]
        unit_c = rt['unit']
        if ld_A:
            A = f(woodbury_A(p[sl], g[sl], LD(1) * w[sl], P['m'][sl]))
            rt['e'] = restatement_error(P64, sl, rt['dense'], A)
            rt['unit'] = np.maximum(U * rt['kappa'], rt['e'])                 # the issue's unit_n, measured row by row
            unit_c = rt['unit']
        else:
            A = scaled_cholesky_A(p64[sl], g64[sl], w[sl], P['m'][sl], blk=blk)
            rt['e'] = np.full(A.shape[0], np.nan)
        for n, A_n in (truth or {}).items():
            if sl.start <= n < sl.stop:
                A[n - sl.start] = A_n
        for n, u_n in (units or {}).items():
            if sl.start <= n < sl.stop:
                unit_c[n - sl.start] = u_n
        kept = {n: A[n - sl.start].copy() for n in keep if sl.start <= n < sl.stop}
        Ap = A[:, ka, kb]
        sd = np.sqrt(np.abs(np.diagonal(A, axis1=1, axis2=2)))
        scale = sd[:, ka] * sd[:, kb]
        nz = np.any(xt64[sl, 1:] != 0.0, axis=1)                 # rows with x = 0 touch the (0, 0) row of R only
        Xp = w2[sl, None][nz] * xt64[sl][nz][:, ja] * xt64[sl][nz][:, jb]
        Rp, Ra, Rb = Xp.T @ Ap[nz], np.abs(Xp).T @ np.abs(Ap[nz]), np.abs(Xp).T @ (scale[nz] * unit_c[:, None][nz])
        z0 = w2[sl][~nz]
        Rp[0] += z0 @ Ap[~nz]
        Ra[0] += z0 @ np.abs(Ap[~nz])
        Rb[0] += (z0 * unit_c[~nz]) @ scale[~nz]
        return rt, kept, Rp, Ra, Rb

    # chunks in parallel, added up in chunk order: the same result for any number of threads
    with _pool() as pool:
        for rt, kept, rp, ra, rb in pool.map(work, range(0, N, chunk)):
            parts.append(rt)
            keep.update(kept)
            Rp += rp
            Ra += ra
            Rb += rb
    out.update({k: np.concatenate([r[k] for r in parts]) for k in parts[0]})
    # A_FACTOR unit_n for the device; for the reference itself a quarter unit where A_n is the longdouble form (measured against
    # mpmath in the host-math file; its rounding to float64 is counted in k_gemm), one unit where it is a float64 restatement
    Bp = (A_FACTOR + (0.25 if ld_A else 1)) * Rb + U * SLACK * k_gemm(N, V, K) * Ra
    R, RB = np.zeros((q, q, K, K)), np.zeros((q, q, K, K))
    for src, dst in ((Rp, R), (Bp, RB)):
        for (a, b) in ((ja, jb), (jb, ja)):
            dst[a[:, None], b[:, None], ka[None, :], kb[None, :]] = src
            dst[a[:, None], b[:, None], kb[None, :], ka[None, :]] = src
    out['R'], out['R_bound'] = R.reshape(q * q, K * K), RB.reshape(q * q, K * K)
    out['A_rows'] = keep
    return out


def a_errors(A_hat, A):
    """a_error for a batch of rows."""
    sd = np.sqrt(np.abs(np.diagonal(A, axis1=1, axis2=2)))
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.max(np.abs(A_hat - A) / (sd[:, :, None] * sd[:, None, :]), axis=(1, 2))


def restatement_error(P64, sl, dense, A_truth):
    """e_n of the float64 restatement of each row's route (everything in float64 from the float64 inputs) against A_truth."""
    p, g, w, m = P64['p'][sl], P64['g'][sl], P64['w'][sl, 0], P64['m'][sl]
    e = np.zeros(p.shape[0])
    if np.any(~dense):
        e[~dense] = a_errors(woodbury_A(p[~dense], g[~dense], w[~dense], m[~dense]), A_truth[~dense])
    if np.any(dense):
        e[dense] = a_errors(scaled_cholesky_A(p[dense], g[dense], w[dense], m[dense]), A_truth[dense])
    return e


def a_error(A_hat, A):
    """e = max |A^ - A|_kk' / sqrt(A_kk A_k'k'): scale-free, small entries do not hide (the square roots are taken apart: a
    saturated row has A_kk A_k'k' below the smallest float64)."""
    sd = np.sqrt(np.abs(np.diag(np.asarray(A, dtype=np.float64))))
    return float(np.max(np.abs(np.asarray(A_hat, dtype=np.float64) - A) / (sd[:, None] * sd[None, :])))


# ---- one row in mpmath --------------------------------------------------------------------------------------------------
def mp_row(f_row, x_row, w_n, lam, dps=None):
    """z_n, the gradient row and A_n of one row, inputs taken as exact float64, in the original coordinates: H_nn over the free
    categories 1 .. K-1 of reference category 0,  d2 p_k / d f_i d f_j = p_k [(d_ki - p_i)(d_kj - p_j) - p_i (d_ij - p_j)],  so
    sum_k g_k d2 p_k = d_ij p_i (g_i - g.p) + p_i p_j (2 g.p - g_i - g_j), and J^T diag(w / p) J = w (d_ij p_i - p_i p_j).
    This H has an eigenvalue of the order of w p_0 or w p_min: the precision is 60 digits plus twice log10(1 / p_min)."""
    f_row, x_row = np.asarray(f_row, dtype=np.float64), np.asarray(x_row, dtype=np.float64)
    ell = np.concatenate([[0.0], f_row])
    pmin = np.exp(ell.min() - ell.max()) / ell.size
    digits = 60 + 2 * int(np.ceil(-np.log10(max(pmin, 1e-300)))) if dps is None else dps
    with mp.workdps(digits):
        K = ell.size
        l = [mp.mpf(float(v)) for v in ell]
        mx = max(l)
        ex = [mp.exp(v - mx) for v in l]
        den = mp.fsum(ex)
        p = [e / den for e in ex]
        xt = [mp.mpf(1)] + [mp.mpf(float(v)) for v in x_row]
        w_ = mp.mpf(float(w_n))
        s = [mp.fsum(xt[j] * mp.mpf(float(lam[j, k])) for j in range(len(xt))) for k in range(K)]
        g = [-w_ * (s[k] - mp.log(p[k]) - 1) for k in range(K)]
        gp = mp.fsum(g[k] * p[k] for k in range(K))
        gz = [p[k] * (g[k] - gp) for k in range(1, K)]
        H = mp.matrix(K - 1, K - 1)
        for i in range(1, K):
            for j in range(1, K):
                H[i - 1, j - 1] = p[i] * p[j] * (2 * gp - w_ - g[i] - g[j]) + (p[i] * (w_ + g[i] - gp) if i == j else 0)
        J = mp.matrix(K, K - 1)
        for k in range(K):
            for i in range(1, K):
                J[k, i - 1] = p[k] * ((1 if k == i else 0) - p[i])
        A = J * (mp.inverse(H) * J.T)
        return (np.array([float(v) for v in p]), np.array([float(v) for v in gz]),
                np.array([[float(A[a, b]) for b in range(K)] for a in range(K)]))


@functools.lru_cache(maxsize=None)
def _mp_row_cached(fb, xb, w_n, lb, K, V):
    return mp_row(np.frombuffer(fb), np.frombuffer(xb), w_n, np.frombuffer(lb).reshape(V + 1, K))


def mp_row_of(prob, n):
    fz, x, lam = prob['fz'], prob['x'], prob['lam']
    return _mp_row_cached(fz[n].tobytes(), x[n].tobytes(), float(prob['w'][n]), np.ascontiguousarray(lam).tobytes(), lam.shape[1], x.shape[1])


def calibrate_row(prob, n):
    """(route, kappa, e of the Woodbury restatement, e of the scaled-Cholesky restatement) of one row, both run in float64 from
    the float64 inputs, against the mpmath truth."""
    sl = slice(n, n + 1)
    P = _prelude(prob['fz'][sl], prob['x'][sl], prob['w'][sl], prob['lam'], np.float64)
    rt = routing(P['p'], P['g'], prob['w'][sl], P['m'])
    A = mp_row_of(prob, n)[2]
    with np.errstate(all='ignore'):
        e_w = a_error(woodbury_A(P['p'], P['g'], prob['w'][sl], P['m'])[0], A)
    e_c = a_error(scaled_cholesky_A(P['p'], P['g'], prob['w'][sl], P['m'])[0], A)
    return ('fast' if rt['dmin_w'][0] > FAST_THRESHOLD else 'dense'), float(rt['kappa'][0]), e_w, e_c


def calibration_rows(prob, limit):
    """All rows where that is cheap; otherwise, per route, the `limit` / 4 rows of largest kappa and as many at even strides."""
    N = prob['N']
    if N <= limit:
        return list(range(N))
    P = _prelude(prob['fz'], prob['x'], prob['w'], prob['lam'], np.float64)
    rt = routing_chunked(P['p'], P['g'], prob['w'], P['m'])
    rows = set(pr['n'] for pr in prob.get('probes', ()))
    for sel in (rt['dmin_w'] > FAST_THRESHOLD, rt['dmin_w'] <= FAST_THRESHOLD):
        idx = np.flatnonzero(sel)
        if idx.size:
            rows.update(idx[np.argsort(rt['kappa'][idx])[-(limit // 4):]].tolist())
            rows.update(idx[::max(1, idx.size // (limit // 4))][:limit // 4].tolist())
    return sorted(rows)


def probe_unit(prob, n):
    """unit_n of a row whose truth is known: max(U kappa_n, the measured e of the restatement of its route)."""
    route, kappa, e_w, e_c = calibrate_row(prob, n)
    return max(U * kappa, e_w if route == 'fast' else e_c)


# ---- problem builders ---------------------------------------------------------------------------------------------------
def cycle_pattern(N):
    """True = dense.  Pairs (fast, dense), (dense, fast), (dense, dense), (fast, fast) in turn; an odd last row is dense."""
    base = np.array([0, 1, 1, 0, 1, 1, 0, 0], dtype=bool)
    pat = np.resize(base, N)
    if N % 2:
        pat[-1] = True
    return pat


def _base(N, V, K, rng):
    x = rng.poisson(2.0, size=(N, V)).astype(np.float64)
    w = rng.uniform(0.5, 1.5, N)
    lam = np.empty((V + 1, K))
    lam[0] = np.log(rng.dirichlet(np.full(K, 50.0)))
    lam[1:] = np.log(rng.dirichlet(np.full(V, 5.0), size=K).T) + np.log(V)     # centred: s stays of the order of sqrt(sum x)
    return x, w, lam


def _dmin_w(fz, x, w, lam):
    """min over the categories but the arg-max of (w + g_k - g.p) / w, without forming the block."""
    P = _prelude(fz, x, w, lam, np.float64)
    d = (P['w'] + P['g'] - P['gdotp']) / P['w']
    d[np.arange(d.shape[0]), P['m']] = np.inf
    return d.min(axis=1), P


def _place(x, w, lam, dense, rng, delta=None, target=None):
    """Logits at the optimum of every row (f = s - s_0) plus a perturbation delta; a dense row has the logit of one category
    that is not the arg-max lowered, by bisection on the reference's dmin / w, until it is at `target`."""
    N, V = x.shape
    K = lam.shape[1]
    s = np.hstack([np.ones((N, 1)), x]) @ lam
    delta = np.clip(0.15 * rng.normal(size=(N, K)), -0.35, 0.35) if delta is None else delta
    ell = s + delta
    m = np.argmax(ell, axis=1)
    c = (m + 1 + rng.integers(0, K - 1, size=N)) % K            # any category but the arg-max
    rows = np.flatnonzero(dense)
    target = rng.uniform(0.008, 0.035, N) if target is None else target
    lo, hi = np.full(rows.size, -4.0), np.zeros(rows.size)

    def fz_of(t):
        e = ell.copy()
        e[rows, c[rows]] = ell[rows, c[rows]] + t
        return e[:, 1:] - e[:, :1]
    for _ in range(44):
        mid = 0.5 * (lo + hi)
        dm = _dmin_w(fz_of(mid)[rows], x[rows], w[rows], lam)[0]
        up = dm > target[rows]
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    return np.ascontiguousarray(fz_of(0.5 * (lo + hi)))


def check_design(prob, indefinite=()):
    """The builder's invariants, from the reference alone, for ALL rows (rows listed in `indefinite` excepted: they are
    asserted indefinite): the route of every row as designed, nothing in (0.04, 0.2), every block positive definite with its
    smallest eigenvalue at least 1e6 U ||M||."""
    fz, x, w, lam, dense = prob['fz'], prob['x'], prob['w'], prob['lam'], prob['dense']
    P = _prelude(fz, x, w, lam, LD)
    p, g = np.asarray(P['p'], dtype=np.float64), np.asarray(P['g'], dtype=np.float64)
    rt = routing_chunked(p, g, w, P['m'])
    ok = np.ones(fz.shape[0], dtype=bool)
    ok[list(indefinite)] = False
    ok &= w > 0
    dm = rt['dmin_w']
    assert np.all((dm[ok & dense] >= DENSE_BAND[0]) & (dm[ok & dense] <= DENSE_BAND[1])), 'a dense row left its band'
    assert np.all(dm[ok & ~dense] >= FAST_MIN), 'a fast row below {}'.format(FAST_MIN)
    assert np.all(rt['eig_min'][ok] >= 1e6 * U * rt['norm'][ok]), 'a row is not safely positive definite'
    assert np.all(rt['det'][ok] < 0)
    for n in indefinite:
        assert rt['eig_min'][n] < -1e6 * U * rt['norm'][n], 'row {} was meant to be indefinite'.format(n)
    return rt


def routed_problem(N, V, K, pattern='cycle', seed=0):
    rng = np.random.default_rng([seed, N, V, K])
    x, w, lam = _base(N, V, K, rng)
    if isinstance(pattern, str):
        dense = cycle_pattern(N) if pattern == 'cycle' else np.zeros(N, dtype=bool)         # 'fast': no dense row
    else:
        dense = np.asarray(pattern, dtype=bool)
    fz = _place(x, w, lam, dense, rng)
    prob = dict(N=N, V=V, K=K, x=x, w=w, lam=lam, fz=fz, dense=dense)
    check_design(prob)
    return prob


def with_indefinite_row(prob, kind):
    """One row of a routed problem made indefinite.  'dense': a dense-route row of the second trip (n >= 32768) and 'last': the
    odd last row, both with d_c lowered to -0.3 w (M has a negative diagonal entry); 'fast': a fast-route row with every
    d_k >= 0.2 w whose det T >= 0: logits flat but for a small bump on the category the data favours, which is then the
    reference category -- its own d is not among the d_k, and v = 1 gives v^T H v = p_m (1 - p_m - eps_m (2 p_m - 1)) < 0."""
    x, w, lam, dense, N = prob['x'], prob['w'], prob['lam'], prob['dense'], prob['N']
    fz = prob['fz'].copy()
    if kind in ('dense', 'last'):
        n = N - 1 if kind == 'last' else int(np.flatnonzero(dense & (np.arange(N) >= 32768) & (np.arange(N) < N - 1))[0])
        assert dense[n]
        sub = dict(x=x[n:n + 1], w=w[n:n + 1], lam=lam)
        rng = np.random.default_rng(n)
        fz[n] = _place(sub['x'], sub['w'], lam, np.array([True]), rng, target=np.array([-0.3]))[0]
    else:
        K = lam.shape[1]
        s = np.hstack([np.ones((N, 1)), x]) @ lam
        top = np.argmax(s, axis=1)
        ell = np.zeros((N, K))
        ell[np.arange(N), top] = 0.01
        cand = (ell[:, 1:] - ell[:, :1])
        P = _prelude(cand, x, w, lam, np.float64)
        rt = routing(P['p'], P['g'], w, P['m'], want_eig=False)
        hit = np.flatnonzero(~dense & (rt['dmin_w'] >= FAST_MIN + 0.05) & (rt['det'] > 1e-3))
        assert hit.size, 'no fast row with det T >= 0 in this problem'
        n = int(hit[hit.size // 2])
        fz[n] = cand[n]
    out = dict(prob, fz=fz, bad_row=n)
    rt = check_design(out, indefinite=(n,))
    if kind == 'fast':
        assert rt['dmin_w'][n] >= FAST_MIN and rt['det'][n] >= 0
    else:
        assert rt['dmin_w'][n] < 0
    return out


def probe_plan(N, K, positions):
    """One probe per position: (row, kind, arg-max category).  Kinds in turn, so that fast and dense rows, every required
    arg-max category and the special rows are all among them whatever the positions."""
    ms = [0, 1, K - 1] + ([15, 16] if K > 16 else [])
    kinds = ['fast', 'dense', 'tie', 'zero', 'sat12', 'sat200']
    plan = []
    for i, n in enumerate(positions):
        kind = kinds[i] if i < len(kinds) else ('dense' if i % 2 else 'fast')
        m = ms[i % len(ms)]
        if kind in ('sat12', 'sat200') and m == 0:
            m = K - 1
        if kind == 'zero':
            m = 0
        if kind == 'tie':
            m = 1 if K > 2 else 0
        plan.append((int(n), kind, m))
    return plan


def probe_problem(N, V, K, positions, seed=0):
    """x = 0 except at the probe rows n_i, where x = c_i e_{j_i} with distinct columns j_i: R[(j_i, j_i), :] = w^2 c_i^2 vec(A_n)
    and S64[j_i, 32 + k] = w c_i z_nk are single terms.  The kind and arg-max category of every probe are designed through Lam
    (row 1 + j_i has its maximum at m_i) and c_i; see probe_plan."""
    positions = [int(n) for n in positions]
    assert len(positions) <= V and len(set(positions)) == len(positions) and max(positions) < N
    rng = np.random.default_rng([seed, N, V, K, 7])
    _, w, lam = _base(N, V, K, rng)
    x = np.zeros((N, V))
    plan = probe_plan(N, K, positions)
    cols = rng.permutation(V)[:len(plan)]
    dense = cycle_pattern(N)
    delta = np.clip(0.15 * rng.normal(size=(N, K)), -0.35, 0.35)
    probes = []
    for (n, kind, m), j in zip(plan, cols):
        row = lam[1 + j]
        top = int(np.argmax(row))
        row[[top, m]] = row[[m, top]]                             # the maximum of the row now sits at category m ...
        row[m] += 1.0                                             # ... at least 1 above the rest
        gap = row[m] - np.partition(row, -2)[-2]
        spread = np.ptp(lam[0])
        c = np.ceil(4.0 * spread / gap) + 1.0                      # c * gap dominates the spread of log pi: arg-max s = m
        if kind == 'zero':
            row[:] = 0.0                                           # s = Lam_0 + const: logits 0 are near the optimum
            c = 1.0
        if kind == 'tie':
            m2 = m + 2 if m + 2 < K else m + 1
            if m2 < K:
                row[m2] = row[m]
                lam[0, m2] = lam[0, m]
        if kind in ('sat12', 'sat200'):
            c = (27.7 if kind == 'sat12' else 461.0) / np.ptp(row)
        x[n, j] = c
        dense[n] = kind == 'dense'
        if kind != 'fast' and kind != 'dense':
            delta[n] = 0.0
        probes.append(dict(n=n, kind=kind, m=m, j=int(j), c=float(c)))
    fz = _place(x, w, lam, dense, rng, delta=delta)
    for pr in probes:
        n = pr['n']
        if pr['kind'] == 'zero':
            fz[n] = 0.0
        if pr['kind'] == 'tie' and K > 2:
            m2 = pr['m'] + 2 if pr['m'] + 2 < K else pr['m'] + 1
            fz[n, m2 - 1] = fz[n, pr['m'] - 1] if pr['m'] >= 1 else 0.0
    prob = dict(N=N, V=V, K=K, x=x, w=w, lam=lam, fz=fz, dense=dense, probes=probes)
    rt = check_design(prob)
    ell = np.hstack([np.zeros((N, 1)), fz])
    for pr in probes:
        n, l = pr['n'], ell[pr['n']]
        assert int(np.argmax(l)) == pr['m'], (pr, l)
        assert np.count_nonzero(x[n]) == 1 and x[n, pr['j']] == pr['c']
        pmin = np.exp(l.min() - l.max() - np.log(np.sum(np.exp(l - l.max()))))
        if pr['kind'] == 'tie' and K > 2:
            assert np.count_nonzero(l == l.max()) == 2             # bit-equal floats
        if pr['kind'] == 'zero':
            assert not np.any(l)
        if pr['kind'] == 'sat12':
            assert 1e-14 < pmin < 1e-11 and pr['m'] != 0
        if pr['kind'] == 'sat200':
            assert 1e-215 < pmin < 1e-195 and pr['m'] != 0
        assert bool(rt['dmin_w'][n] <= FAST_THRESHOLD) == (pr['kind'] == 'dense')
    return prob


def grid_probe_positions(N=65539):
    """Rows 0, 1 (both halves of pair 0); 32766 .. 32769: the last pair of wave 3 of the last workgroup in its first trip and
    the first pair of wave 0 of workgroup 0 in its second; 65534, 65535: wave 3 of the last workgroup in its second (and last)
    trip; N - 3 .. N - 1: the third trip, which only waves 0 and 1 of workgroup 0 take, the last pair half valid.  Five of the
    pairs have both halves probed."""
    assert N == 65539
    return [0, 1, 32766, 32767, 32768, 32769, 65534, 65535, N - 3, N - 2, N - 1]


# ---- the cases of tests/test_gpu_mixture_rows.py (the CPU file checks the builders and calibrates on exactly these) ---------
GRID_CASES = [(65539, 2, 3), (65539, 7, 5), (32771, 6, 17), (32771, 31, 32)]        # three trips, three, two, two (kron32 GEMM)
DENSE_STRIDE_CASE = (32771, 7, 5)                                                  # forced dense: 32771 > 4 * 2048 rows
ROUTED_CASES = [(37, 3, 2), (61, 5, 4), (45, 9, 8), (131, 17, 17), (150, 31, 32), (2, 1, 2)]
ROUTED_BIG = (32771, 7, 5)
# more than 2048 rows (two workgroups on a CU) at K whose last 1 KiB store segment of a row leaves lanes 12 .. 15 of a 16 unmasked:
# the 16-byte stores of DESIGN.md section 38, "what the tests found"
STORE_CASES = [(4099, 2, 7), (4099, 3, 13), (4099, 2, 17), (4099, 3, 25), (4099, 2, 31)]
PROBE_CASES = [(65539, 31, 32, 'all'), (65539, 7, 5, 'a'), (65539, 7, 5, 'b')]


def probe_positions(which):
    pos = grid_probe_positions()
    if which == 'all':
        return pos
    # 20001 and 40010, 40011: the middle of the first and of the second trip
    return [0, 1, 32767, 32768, 32769, 65537, 65538] if which == 'a' else [32766, 65534, 65535, 65536, 20001, 40010, 40011]


@functools.lru_cache(maxsize=9)
def grid_case(N, V, K):
    return routed_problem(N, V, K, 'fast', seed=1)


@functools.lru_cache(maxsize=8)
def routed_case(N, V, K):
    return routed_problem(N, V, K, 'cycle', seed=2)


@functools.lru_cache(maxsize=3)
def probe_case(N, V, K, which):
    return probe_problem(N, V, K, probe_positions(which), seed=3)


def all_cases():
    for c in GRID_CASES:
        yield ('grid',) + c, lambda c=c: grid_case(*c)
    for c in STORE_CASES:
        yield ('store',) + c, lambda c=c: grid_case(*c)
    for c in ROUTED_CASES + [ROUTED_BIG]:
        yield ('routed',) + c, lambda c=c: routed_case(*c)
    for c in PROBE_CASES:
        yield ('probe',) + c, lambda c=c: probe_case(*c)


def max_ratio(got, ref, bound):
    """max |got - ref| / bound with 0 / 0 = 0: a zero bound passes only on an exactly equal result."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def worst(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    i = np.unravel_index(np.argmax(r), r.shape)
    return 'entry {}: got {!r} want {!r} bound {:.3e} ratio {:.3f}'.format(i, np.asarray(got)[i], np.asarray(ref)[i], np.asarray(bound)[i], r[i])

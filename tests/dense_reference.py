"""Plain references for the dense Cholesky, the solves by inverse diagonal blocks and CG on a resident matrix
(csrc/k_linalg.hip), and the inputs of tests/test_gpu_dense_linalg.py.  NumPy / SciPy only: importable and runnable
without the library, so tests/test_dense_reference_host_math.py can show on the CPU that every input is fair -- LAPACK
and a NumPy emulation of the device algorithm sit inside every bound the GPU file asserts.

Bounds, eps = 2^-52:
  forward   ||X - Xref||_F / ||Xref||_F <= eps kappa_2(S)            first-order bound of any Cholesky solve
  backward  max|B - S X| / (||S||_inf max|X| + max|B|) <= n eps      kappa_2 <= 1e6 (Cholesky, ~(3n + 1) eps)
                                                       <= n eps sqrt(kappa_2) above: a solve through explicit inverses
            of triangular blocks is conditionally backward stable, its residual may carry kappa(L_jj) <= sqrt(kappa_2(S))
  lrvb_cov  ||cov - M Xref||_F <= eps kappa_2 ||M||_F ||Xref||_F,    Xref = S^-1 M^T
"""
import numpy as np
import scipy.linalg as sla

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
NB = 64                                   # block size of the device factorisation


# ---- helpers ----------------------------------------------------------------------------------------------------
def spd_with_spectrum(rng, n, kappa):
    """Q diag(logspace(0, -log10 kappa, n)) Q^T, symmetrised; Q from a QR of a Gaussian matrix.  kappa_2 = kappa for
    n >= 2 (1 for n = 1) by construction."""
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.logspace(0.0, -np.log10(kappa), n)
    S = (Q * lam) @ Q.T
    return 0.5 * (S + S.T)


def kappa_by_construction(n, kappa):
    return 1.0 if n == 1 else float(kappa)


def refined_solve(S, B):
    """S^-1 B: LAPACK cho_solve refined in longdouble (residual and update accumulated in longdouble) until the
    longdouble residual stops decreasing.  Returns a longdouble array of B's shape; it stands in for the exact solution
    (relative residual ~1e-19 kappa on x86, three to four orders below every asserted bound)."""
    S = np.asarray(S, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    B2 = B.reshape(B.shape[0], -1)
    c = sla.cho_factor(S, lower=True)
    Sl, Bl = S.astype(LD), B2.astype(LD)
    X = sla.cho_solve(c, B2).astype(LD)
    R = Bl - Sl @ X
    rn = np.max(np.abs(R))
    for _ in range(40):
        if rn == 0.0:
            break
        Xn = X + sla.cho_solve(c, R.astype(np.float64)).astype(LD)
        Rn = Bl - Sl @ Xn
        rnn = np.max(np.abs(Rn))
        if not rnn < rn:
            break
        X, R, rn = Xn, Rn, rnn
    return X.reshape(B.shape)


def forward_error(X, Xref):
    d = np.asarray(X, dtype=LD).reshape(np.shape(Xref)) - np.asarray(Xref, dtype=LD)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(np.asarray(Xref, dtype=LD) ** 2)))


def forward_error_columns(X, Xref):
    """forward_error of every column on its own."""
    Xr = np.asarray(Xref, dtype=LD)
    d = np.asarray(X, dtype=LD) - Xr
    return (np.sqrt(np.sum(d * d, axis=0)) / np.sqrt(np.sum(Xr * Xr, axis=0))).astype(np.float64)


def backward_error(S, X, B):
    S = np.asarray(S, dtype=np.float64)
    X2 = np.asarray(X, dtype=np.float64).reshape(S.shape[0], -1)
    B2 = np.asarray(B, dtype=np.float64).reshape(S.shape[0], -1)
    R = B2.astype(LD) - S.astype(LD) @ X2.astype(LD)
    den = np.max(np.sum(np.abs(S), axis=1)) * np.max(np.abs(X2)) + np.max(np.abs(B2))
    return float(np.max(np.abs(R)) / den)


def first_bad_pivot(S):
    """Unblocked lower Cholesky in longdouble, reading the lower triangle only: the 1-based index of the first pivot that
    is not a positive finite number (`not > 0`; NaN compares false; +Inf has no square root to divide by), or 0."""
    A = np.tril(np.asarray(S, dtype=np.float64)).astype(LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    with np.errstate(all='ignore'):
        for k in range(n):
            d = A[k, k] - np.sum(L[k, :k] * L[k, :k])
            if not (d > 0 and np.isfinite(d)):
                return k + 1
            L[k, k] = np.sqrt(d)
            if k + 1 < n:
                L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return 0


def bounds(n, kappa):
    """(forward, backward) bounds asserted for an n x n matrix of condition kappa."""
    return EPS * kappa, (n * EPS if kappa <= 1e6 else n * EPS * np.sqrt(kappa))


def cov_error(cov, M, Xref):
    """(||cov - M Xref||_F, ||M||_F ||Xref||_F) with the product in longdouble."""
    ref = np.asarray(M, dtype=np.float64).astype(LD) @ np.asarray(Xref, dtype=LD)
    d = np.asarray(cov, dtype=np.float64).astype(LD) - ref
    scale = np.sqrt(np.sum(np.asarray(M, dtype=LD) ** 2)) * np.sqrt(np.sum(np.asarray(Xref, dtype=LD) ** 2))
    return float(np.sqrt(np.sum(d * d))), float(scale)


def true_residual(S, x, b):
    """||S x - b|| / ||b|| with the product in longdouble."""
    r = np.asarray(S, dtype=np.float64).astype(LD) @ np.asarray(x, dtype=np.float64).astype(LD) - np.asarray(b, dtype=np.float64).astype(LD)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(np.asarray(b, dtype=LD) ** 2)))


# ---- NumPy emulation of the device algorithm --------------------------------------------------------------------
def _diag_block_factor(blk):
    """The diagonal step: four columns at a time, reciprocal square roots, the trailing row updated with
    u = Lp^-T y against the raw entries of the other rows.  blk: 64 x 64, lower triangle, identity padding."""
    a = blk.copy()
    bad = 0
    with np.errstate(all='ignore'):
        for j in range(0, NB, 4):
            x = a[:, j:j + 4].copy()
            p = x[j:j + 4]
            d0 = p[0, 0]
            rs0 = 1.0 / np.sqrt(d0)
            l10, l20, l30 = p[1, 0] * rs0, p[2, 0] * rs0, p[3, 0] * rs0
            d1 = p[1, 1] - l10 * l10
            rs1 = 1.0 / np.sqrt(d1)
            l21, l31 = (p[2, 1] - l20 * l10) * rs1, (p[3, 1] - l30 * l10) * rs1
            d2 = p[2, 2] - l20 * l20 - l21 * l21
            rs2 = 1.0 / np.sqrt(d2)
            l32 = (p[3, 2] - l30 * l20 - l31 * l21) * rs2
            d3 = p[3, 3] - l30 * l30 - l31 * l31 - l32 * l32
            rs3 = 1.0 / np.sqrt(d3)
            if bad == 0:
                for q, d in enumerate((d0, d1, d2, d3)):
                    if not (d > 0.0 and np.isfinite(d)):
                        bad = j + q + 1
                        break
            y0 = x[:, 0] * rs0
            y1 = (x[:, 1] - y0 * l10) * rs1
            y2 = (x[:, 2] - y0 * l20 - y1 * l21) * rs2
            y3 = (x[:, 3] - y0 * l30 - y1 * l31 - y2 * l32) * rs3
            a[:, j], a[:, j + 1], a[:, j + 2], a[:, j + 3] = y0, y1, y2, y3
            u3 = y3 * rs3
            u2 = (y2 - l32 * u3) * rs2
            u1 = (y1 - l21 * u2 - l31 * u3) * rs1
            u0 = (y0 - l10 * u1 - l20 * u2 - l30 * u3) * rs0
            t = x[j + 4:]
            a[:, j + 4:] = (((a[:, j + 4:] - np.outer(u0, t[:, 0])) - np.outer(u1, t[:, 1])) - np.outer(u2, t[:, 2])) - np.outer(u3, t[:, 3])
    return np.tril(a), bad


def _tri_inverse(L):
    """W = L^-1 of a 64 x 64 lower block, 16 -> 32 -> 64:  inv [[P, 0], [Q, R]] = [[P^-1, 0], [-R^-1 Q P^-1, R^-1]]."""
    W = np.zeros((NB, NB))
    with np.errstate(all='ignore'):
        for w in range(4):
            s = slice(16 * w, 16 * w + 16)
            Lw, x = L[s, s], np.zeros((16, 16))
            for i in range(16):
                x[i] = ((np.arange(16) == i).astype(np.float64) - Lw[i, :i] @ x[:i]) / Lw[i, i]
            W[s, s] = x
        for h in range(2):
            a, b = slice(32 * h, 32 * h + 16), slice(32 * h + 16, 32 * h + 32)
            W[b, a] = -(W[b, b] @ (L[b, a] @ W[a, a]))
        a, b = slice(0, 32), slice(32, 64)
        W[b, a] = -(W[b, b] @ (L[b, a] @ W[a, a]))
    return W


def emulated_factor(S):
    """Right-looking blocked Cholesky with 64-column blocks, the lower triangle alone read.  Returns (L, [W_j], info):
    the factor, the explicit inverses of its diagonal blocks, and the 1-based index of the first bad pivot (0: none)."""
    A = np.tril(np.asarray(S, dtype=np.float64))
    n = A.shape[0]
    Ws, info = [], 0
    with np.errstate(all='ignore'):
        for j0 in range(0, n, NB):
            nb = min(NB, n - j0)
            blk = np.eye(NB)
            blk[:nb, :nb] = A[j0:j0 + nb, j0:j0 + nb]
            L, bad = _diag_block_factor(blk)
            if bad and not info:
                info = j0 + bad
            A[j0:j0 + nb, j0:j0 + nb] = L[:nb, :nb]
            W = _tri_inverse(L)
            Ws.append(W)
            if j0 + nb < n:
                P = A[j0 + nb:, j0:j0 + nb] @ W.T
                A[j0 + nb:, j0:j0 + nb] = P
                A[j0 + nb:, j0 + nb:] -= np.tril(P @ P.T)
    return A, Ws, info


def _forward(L, Ws, X):
    n = L.shape[0]
    nblk = len(Ws)
    sl = [slice(j * NB, min(n, (j + 1) * NB)) for j in range(nblk)]
    nb0 = sl[0].stop - sl[0].start
    X[sl[0]] = Ws[0][:nb0, :nb0] @ X[sl[0]]
    for jb in range(nblk - 1):
        X[sl[jb].stop:] -= L[sl[jb].stop:, sl[jb]] @ X[sl[jb]]
        nb = sl[jb + 1].stop - sl[jb + 1].start
        X[sl[jb + 1]] = Ws[jb + 1][:nb, :nb] @ X[sl[jb + 1]]
    return X


def emulated_solve(L, Ws, B):
    """S^-1 B by products with the stored inverse blocks, forward then backward."""
    B = np.asarray(B, dtype=np.float64)
    n = L.shape[0]
    X = _forward(L, Ws, np.array(B.reshape(n, -1), order='C'))
    nblk = len(Ws)
    sl = [slice(j * NB, min(n, (j + 1) * NB)) for j in range(nblk)]
    nb = sl[-1].stop - sl[-1].start
    X[sl[-1]] = Ws[-1][:nb, :nb].T @ X[sl[-1]]
    for jb in range(nblk - 1, 0, -1):
        X[:sl[jb].start] -= L[sl[jb], :sl[jb].start].T @ X[sl[jb]]
        X[sl[jb - 1]] = Ws[jb - 1].T @ X[sl[jb - 1]]
    return X.reshape(B.shape)


def emulated_cov(L, Ws, M):
    """M S^-1 M^T = Y^T Y with Y = L^-1 M^T: one forward substitution and a product."""
    Y = _forward(L, Ws, np.array(np.asarray(M, dtype=np.float64).T, order='C'))
    return Y.T @ Y


def lapack_solve(S, B):
    return sla.cho_solve(sla.cho_factor(np.asarray(S, dtype=np.float64), lower=True), np.asarray(B, dtype=np.float64))


def host_pcg(S, b, Minv=None, tol=1e-10, maxiter=0):
    """The documented loop of lrvb_cg_solve_matrix: stops when the recurrence residual ||r|| < tol ||b||."""
    D = b.size
    x, r = np.zeros(D), b.copy()
    p, rho_prev = None, 0.0
    atol = tol * np.linalg.norm(b)
    for it in range(maxiter or 10 * D):
        z = r if Minv is None else Minv @ r
        if np.linalg.norm(r) < atol:
            return x, 0, it
        rho = r @ z
        p = z.copy() if it == 0 else z + (rho / rho_prev) * p
        q = S @ p
        alpha = rho / (p @ q)
        x, r, rho_prev = x + alpha * p, r - alpha * q, rho
    return x, maxiter or 10 * D, maxiter or 10 * D


# ---- the inputs of tests/test_gpu_dense_linalg.py -----------------------------------------------------------------
SWEEP_N = (1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 67, 127, 128, 129, 191, 192, 193, 257)
SWEEP_KAPPA = 1e4
SWEEP_NRHS = (1, 3, 63, 64, 65, 130)
SWEEP_Q = (1, 5, 64, 65)
COND_N = (65, 130, 193)
COND_KAPPA = (1e2, 1e6, 1e10, 1e12)
COND_NRHS = 5
SYM_CASES = ((65, 65), (193, 130))
PIVOT_N, PIVOT_KAPPA = 130, 1e2
PIVOT_POSITIONS = (0, 1, 2, 3, 60, 61, 62, 63, 64, 65, 66, 67, 124, 125, 126, 127, 128, 129)
NONFINITE_DIAG = (0, 2, 63, 64, 67, 129)                       # NaN / +Inf at [k, k]
NONFINITE_BELOW = ((1, 0), (3, 1), (63, 5), (64, 63), (70, 3), (129, 64), (129, 128))   # NaN at [i, k], i > k
LOWER_N = (5, 65, 130)
ROUTE_N, ROUTE_KAPPA = (129, 130), 1e2
ROUTE_NRHS, ROUTE_NRHS_FUSED = 16400, 16384
ROUTE_UNIQUE = 400
STATE_SIZES = (193, 65, 130)
DEV_D = (65, 130)
CG_D = (63, 254, 255, 256, 258, 512, 514, 1024, 1026)
CG_KAPPA, CG_TOL = 1e2, 1e-10

_cache = {}


def _memo(key, make):
    if key not in _cache:
        out = make()
        for a in (out if isinstance(out, tuple) else (out,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def sweep_case(n):
    """(S, kappa, B (n x 130), Xref, M (65 x n), Xref_M = S^-1 M^T); the tests take leading columns / rows."""
    def make():
        rng = np.random.default_rng(7000 + n)
        S = spd_with_spectrum(rng, n, SWEEP_KAPPA)
        B = rng.normal(size=(n, max(SWEEP_NRHS)))
        M = rng.normal(size=(max(SWEEP_Q), n))
        return S, kappa_by_construction(n, SWEEP_KAPPA), B, refined_solve(S, B), M, refined_solve(S, M.T)
    return _memo(('sweep', n), make)


def cond_case(n, kappa):
    """(S, B (n x 5), Xref, d): d = 2^k, k uniform in [-20, 20] per coordinate; D S D and D B are exact."""
    def make():
        rng = np.random.default_rng(8000 + n + int(np.log10(kappa)))
        S = spd_with_spectrum(rng, n, kappa)
        B = rng.normal(size=(n, COND_NRHS))
        d = np.ldexp(1.0, rng.integers(-20, 21, size=n))
        return S, B, refined_solve(S, B), d
    return _memo(('cond', n, kappa), make)


def sym_case(n, Q):
    def make():
        rng = np.random.default_rng(8500 + n)
        return spd_with_spectrum(rng, n, SWEEP_KAPPA), rng.normal(size=(Q, n))
    return _memo(('sym', n, Q), make)


def pivot_matrix():
    return _memo('pivot', lambda: spd_with_spectrum(np.random.default_rng(9001), PIVOT_N, PIVOT_KAPPA))


def broken_pivot(k):
    """pivot_matrix() with the leading minor of order k + 1 made negative."""
    S = pivot_matrix().copy()
    L = np.linalg.cholesky(S)
    S[k, k] -= 1.5 * L[k, k] ** 2
    return S


def nonfinite_cases():
    """[(tag, matrix)]: all zero, NaN on / below the diagonal (mirrored), +Inf on the diagonal."""
    out = [('zero', np.zeros((PIVOT_N, PIVOT_N)))]
    for k in NONFINITE_DIAG:
        for name, v in (('nan', np.nan), ('inf', np.inf)):
            S = pivot_matrix().copy()
            S[k, k] = v
            out.append(('{}[{},{}]'.format(name, k, k), S))
    for i, k in NONFINITE_BELOW:
        S = pivot_matrix().copy()
        S[i, k] = S[k, i] = np.nan
        out.append(('nan[{},{}]'.format(i, k), S))
    return out


def expected_nonfinite_index(tag):
    """The index the issue states for the case, independent of first_bad_pivot (None for +Inf: derived by it)."""
    if tag == 'zero':
        return 1
    if tag.startswith('nan'):
        i, _ = tag[4:-1].split(',')
        return int(i) + 1
    return None


def lower_case(n):
    def make():
        rng = np.random.default_rng(9100 + n)
        return spd_with_spectrum(rng, n, SWEEP_KAPPA), rng.normal(size=(n, 7))
    return _memo(('lower', n), make)


def route_case(n):
    """(S, B (n x 16400), Xref).  B repeats ROUTE_UNIQUE distinct columns (400 is no multiple of the 64-column tile, so
    every tile sees another alignment of them): the longdouble refinement runs on the distinct columns only, and every one
    of the 16400 columns still has its own reference.  The fused control takes the leading 16384 columns."""
    def make():
        rng = np.random.default_rng(9200 + n)
        S = spd_with_spectrum(rng, n, ROUTE_KAPPA)
        B0 = rng.normal(size=(n, ROUTE_UNIQUE))
        reps = -(-ROUTE_NRHS // ROUTE_UNIQUE)
        B = np.ascontiguousarray(np.tile(B0, (1, reps))[:, :ROUTE_NRHS])
        return S, B, np.ascontiguousarray(np.tile(refined_solve(S, B0), (1, reps))[:, :ROUTE_NRHS])
    return _memo(('route', n), make)


def state_case(n):
    def make():
        rng = np.random.default_rng(9300 + n)
        S = spd_with_spectrum(rng, n, SWEEP_KAPPA)
        B = rng.normal(size=(n, 6))
        return S, B, refined_solve(S, B)
    return _memo(('state', n), make)


def dev_case(D):
    def make():
        rng = np.random.default_rng(9400 + D)
        return spd_with_spectrum(rng, D, SWEEP_KAPPA), rng.normal(size=(D, 9)), rng.normal(size=(11, D))
    return _memo(('dev', D), make)


def cg_case(D):
    def make():
        rng = np.random.default_rng(9500 + D)
        return spd_with_spectrum(rng, D, CG_KAPPA), rng.normal(size=D)
    return _memo(('cg', D), make)

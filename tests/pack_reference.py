"""References for the packing layer (`csrc/k_pack.hip`): the free <-> vector maps of box, log-Cholesky and simplex blocks,
their Jacobians, the second-order term sum_k g_k d2 eta_k, and the products J^T A and J^T H J.  NumPy, mpmath and longdouble
only; nothing here touches a GPU or the project's own oracle.

Two oracles share the code below:
  exact   inputs for which every device result is an integer or a multiple of 1/16 far below 2^53, so that any order of
          summation gives the same float64 (`exact_theta`, `int_matrix`; `assert_exact_margin` checks the margin from the
          actual maxima).  The reference runs in float64 and the device must match bitwise.
  bound   real data over decades (`real_theta`, `real_matrix`); the reference runs in longdouble (box and simplex maps in
          mpmath at 200 bits) together with the matrix of absolute terms, and the device must sit inside
          K * 2^-53 * 1.01 * (absolute terms), K counted from the kernel text (the K_* constants).

A layout is a list of ('box', name, n, lb, ub) | ('psd', name, k, diag_lb) | ('simplex', name, rows, K), as in helpers.make_par.
"""
import numpy as np
import mpmath as mp

LD = np.longdouble
U = 2.0 ** -53
SLACK = 1.01
E_ULP = 2                      # the project's figure for the device's exp and log, in ulp
EXPU = 2 * E_ULP               # ... in units of U = 2^-53: an ulp is 2 U
PREC = 200
TINY = 8 * 2.0 ** -1074          # results in the subnormal range: a few units of the subnormal spacing, absolute

# ---- rounding counts, from the text of k_pack.hip (units of U, on the scale of the absolute terms) ------------------------
# box_eval, one-sided: x = exp(+-f) [EXPU]; eta = x + lb: one addition, relative to the result.
K_BOX1_X = EXPU + 1            # eta' and eta'' = +-x, and the reference rounded to float64
# box_eval, two-sided: ef = exp(-|f|) [EXPU], 1 + ef [1], the quotient [1]: s and its complement cost EXPU + 2 each
K_S = EXPU + 2
K_BOX2_ETA = K_S + 2           # r = ub - lb [1], r * s [1]; the final + lb and the reference: 2 |eta| added apart
K_BOX2_D1 = 2 * K_S + 4        # s * (1 - s) [1], r [1], r * sp [1], reference [1]
K_BOX2_D2 = 2 * K_BOX2_D1 + 5  # d1 * (1 - 2 s): the error of (1 - 2 s) is 2 s K_S + 1 <= 2 K_S + 1 absolute; one product more
# jt_apply_kernel, one product: a term L_tb * G_t meets the exp of a diagonal L entry [EXPU], the factor 2 [0], one MFMA
# accumulation per k-step from its own step to the last (at most kr steps; a step is counted as a product and an addition,
# 2 roundings: the internal rounding of the f64 MFMA is not assumed fused), the closing * L_aa (a second exp and a product:
# EXPU + 1) and the reference's rounding [1].  Raised from the issue's proposal E + kr + 2 before any GPU run: E ulp are 2E U,
# the closing factor carries its own exp, and no fusion is assumed.
def k_jt(k):
    kr = (k + 3) & ~3
    return 2 * EXPU + 2 * kr + 2
K_JT_BOX1 = EXPU + 2           # d1 * A: exp, one product, the reference
K_JT_BOX2 = K_BOX2_D1 + 1
# psd_jac_kernel: dL * v with v one L entry or exactly twice one: two exps at most, one product, the reference
K_PSD_JAC = 2 * EXPU + 2
# psd_constrain_kernel: a chain of j + 1 products and additions [2 k], two exps per term, + diag_lb [1], the reference [1]
def k_psd_eta(k):
    return 2 * EXPU + 2 * k + 2
# psd_third_kernel: dLab dLcd gs (1|2): two exps, three products; the diagonal term laa (2 g laa + sum g f): a chain of k - a
# products and additions, two exps, two products; v joins T [1]; the reference [1]
def k_psd_third(k):
    return 2 * EXPU + 2 * k + 6
# simplex: see simplex_rel_p


# ---- layout ------------------------------------------------------------------------------------------------------------
def ld_idx(a, b):
    return b + a * (a + 1) // 2


def blocks_of(spec):
    out, fo, vo = [], 0, 0
    for s in spec:
        if s[0] == 'box':
            b = dict(kind='box', name=s[1], nf=s[2], nv=s[2], lb=float(s[3]), ub=float(s[4]))
        elif s[0] == 'psd':
            m = s[2] * (s[2] + 1) // 2
            b = dict(kind='psd', name=s[1], nf=m, nv=m, k=s[2], diag_lb=float(s[3]))
        else:
            b = dict(kind='simplex', name=s[1], nf=s[2] * (s[3] - 1), nv=s[2] * s[3], rows=s[2], K=s[3])
        b['fo'], b['vo'] = fo, vo
        fo += b['nf']
        vo += b['nv']
        out.append(b)
    return out, fo, vo


def sizes(spec):
    _, D, V = blocks_of(spec)
    return D, V


def to_ld(x):
    """mpf -> longdouble through a float64 head and tail (64 bits are kept)."""
    hi = float(x)
    if not np.isfinite(hi) or hi == 0.0:
        return LD(hi)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


# ---- box, from the definition, in mpmath ------------------------------------------------------------------------------------
def box_mp(f, lb, ub):
    """eta, eta', eta'' of one box coordinate as mpf.  eta = f | lb + e^f | ub - e^-f | lb + (ub - lb) / (1 + e^-f)."""
    return box_mp_at(mp.mpf(float(f)), lb, ub)


def box_mp_at(f, lb, ub):
    with mp.workprec(PREC):
        has_lb, has_ub = np.isfinite(lb), np.isfinite(ub)
        if not has_lb and not has_ub:
            return f, mp.mpf(1), mp.mpf(0)
        if has_lb and not has_ub:
            x = mp.exp(f)
            return mp.mpf(lb) + x, x, x
        if has_ub and not has_lb:
            x = mp.exp(-f)
            return mp.mpf(ub) - x, x, -x
        r = mp.mpf(ub) - mp.mpf(lb)
        s = 1 / (1 + mp.exp(-f))
        # s (1 - s) = 1 / ((1 + e^-f)(1 + e^f)): no subtraction, so 200 bits hold at |f| = 800 too;  1 - 2 s = -tanh(f / 2)
        d1 = r / ((1 + mp.exp(-f)) * (1 + mp.exp(f)))
        return mp.mpf(lb) + r * s, d1, -d1 * mp.tanh(f / 2)


def box_arrays(f, lb, ub):
    """(eta, eta', eta'') as longdouble arrays and their bounds (float64 arrays, absolute) for the device's box_eval."""
    n = len(f)
    val = np.zeros((3, n), dtype=LD)
    bnd = np.zeros((3, n))
    has_lb, has_ub = np.isfinite(lb), np.isfinite(ub)
    for i in range(n):
        e, d1, d2 = box_mp(f[i], lb, ub)
        val[:, i] = [to_ld(e), to_ld(d1), to_ld(d2)]
        ae, a1 = abs(float(e)), abs(float(d1))
        if not has_lb and not has_ub:
            continue                                                   # eta = f, 1, 0: exact
        if has_lb != has_ub:
            x = a1
            bnd[:, i] = [K_BOX1_X * x + 2 * ae, K_BOX1_X * x, K_BOX1_X * x]
        else:
            with mp.workprec(PREC):
                rs = abs(float(e - mp.mpf(lb)))
            bnd[:, i] = [K_BOX2_ETA * rs + 2 * ae, K_BOX2_D1 * a1, K_BOX2_D2 * a1]
    return val, bnd * (U * SLACK)


# ---- log-Cholesky ------------------------------------------------------------------------------------------------------------
def chol_factor(f, k, dtype=LD):
    L = np.zeros((k, k), dtype=dtype)
    L[np.tril_indices(k)] = np.asarray(f, dtype=dtype)
    d = np.arange(k)
    L[d, d] = np.exp(L[d, d])
    return L


def psd_eta(f, k, diag_lb, dtype=LD, absval=False):
    L = chol_factor(f, k, dtype)
    if absval:
        L = np.abs(L)
    A = L @ L.T + dtype(abs(diag_lb) if absval else diag_lb) * np.eye(k, dtype=dtype)
    return A[np.tril_indices(k)]


def psd_dA(L, a, b):
    """The definition: dA = dL L^T + L dL^T for dL = dL_ab e_a e_b^T, dL_ab = L_aa on the diagonal (f_aa -> exp) and 1 below."""
    k = L.shape[0]
    dL = np.zeros_like(L)
    dL[a, b] = L[a, a] if a == b else 1
    return dL @ L.T + L @ dL.T


def psd_jac_dense_definition(f, k, dtype=LD):
    """m x m Jacobian column by column from psd_dA (small k only: O(m k^3))."""
    L = chol_factor(f, k, dtype)
    r, c = np.tril_indices(k)
    J = np.zeros((len(r), len(r)), dtype=dtype)
    for col in range(len(r)):
        J[:, col] = psd_dA(L, r[col], c[col])[r, c]
    return J


def psd_gather_rows(k, a):
    """Column (a, b) of J has its entries in the k vector rows (a, t) for t <= a and (t, a) for t > a -- row a and column a
    of the symmetric dA -- with values dL_ab L_tb, twice that at t = a (both terms of dA meet there), zero for t < b."""
    t = np.arange(k)
    return np.where(t <= a, ld_idx(a, np.minimum(t, a)), ld_idx(np.maximum(t, a), a))


def psd_jt_apply(f, k, A, dtype=LD, absval=False):
    """Rows of J^T A of one block (A: the block's m vector rows x Q) through the column sparsity of J."""
    L = chol_factor(f, k, dtype)
    if absval:
        L = np.abs(L)
    out = np.zeros((k * (k + 1) // 2, A.shape[1]), dtype=dtype)
    for a in range(k):
        G = A[psd_gather_rows(k, a)].copy()
        G[a] *= 2
        R = L[:, :a + 1].T @ G                      # row b: sum_t L_tb G_t (L_tb = 0 for t < b)
        R[a] *= L[a, a]
        out[ld_idx(a, 0):ld_idx(a, a) + 1] = R
    return out


def psd_third(f, k, g, dtype=LD, absval=False):
    """sum_{i >= j} g_ij d2 A_ij / df_ab df_cd, from differentiating dA = dL L^T + L dL^T once more:
    d2A = dL_ab dL_cd (e_a e_b^T e_d e_c^T + e_c e_d^T e_b e_a^T) + [ab = cd, a = b] L_aa (e_a (L e_a)^T + (L e_a) e_a^T),
    contracted with the lower-triangular matrix Gl of g."""
    L = chol_factor(f, k, dtype)
    Gl = np.zeros((k, k), dtype=dtype)
    Gl[np.tril_indices(k)] = np.asarray(g, dtype=dtype)
    if absval:
        L, Gl = np.abs(L), np.abs(Gl)
    S = Gl + Gl.T                                    # <Gl, e_a e_c^T + e_c e_a^T>
    m = k * (k + 1) // 2
    T = np.zeros((m, m), dtype=dtype)
    for b in range(k):
        a = np.arange(b, k)
        idx = ld_idx(a, b)
        dl = np.ones(len(a), dtype=dtype)
        dl[0] = L[b, b]
        T[np.ix_(idx, idx)] = dl[:, None] * dl[None, :] * S[b:, b:]
        T[idx[0], idx[0]] += L[b, b] * (Gl[b, :] @ L[:, b] + Gl[:, b] @ L[:, b])
    return T


# ---- simplex, in mpmath ----------------------------------------------------------------------------------------------------------
def simplex_row_mp(frow):
    with mp.workprec(PREC):
        z = [mp.mpf(0)] + [mp.mpf(float(v)) for v in frow]
        mx = max(z)
        e = [mp.exp(v - mx) for v in z]
        tot = mp.fsum(e)
        return [v / tot for v in e]


def simplex_rel_p(frow):
    """Relative bound (units of U) of the device's p_k = exp(f_k - lse), lse = mx + log(sum_j exp(f_j - mx)): the sum s >= 1
    meets K additions, an exp per term and the rounding of f_j - mx (at most max|f_j - mx| in the relative error of a term);
    log [EXPU |log s|, log s <= log K], mx + log s [|lse|]; the argument f_k - lse is rounded [|f_k - lse|] and carries the
    error of lse; the final exp [EXPU]; the reference [1]."""
    z = np.concatenate([[0.0], np.asarray(frow, dtype=np.float64)])
    K = len(z)
    mx = z.max()
    lse = mx + np.log(np.sum(np.exp(z - mx)))
    return 2 * EXPU + K + 2 + EXPU * np.log(K) + np.max(np.abs(z - mx)) + abs(lse) + np.abs(z - lse)


def simplex_row_all(frow, g=None):
    """p (K), J (K x K-1), T (K-1 x K-1, for weights g) of one row as longdouble, with absolute bounds (float64)."""
    K = len(frow) + 1
    p = simplex_row_mp(frow)
    rel = simplex_rel_p(frow)
    pf = np.array([float(v) for v in p])
    P = np.array([to_ld(v) for v in p], dtype=LD)
    pb = rel * pf
    J = np.zeros((K, K - 1), dtype=LD)
    Jb = np.zeros((K, K - 1))
    T = np.zeros((K - 1, K - 1), dtype=LD)
    Tb = np.zeros((K - 1, K - 1))
    with mp.workprec(PREC):
        for kk in range(K):
            for j in range(K - 1):
                d = 1 if kk == j + 1 else 0
                J[kk, j] = to_ld(p[kk] * (d - p[j + 1]))
                Jb[kk, j] = pf[kk] * (d + pf[j + 1]) * (rel[kk] + rel[j + 1] + 3)
        if g is not None:
            for i in range(K - 1):
                for j in range(K - 1):
                    acc, accb = mp.mpf(0), 0.0
                    for kk in range(K):
                        di, dj, dij = (1 if kk == i + 1 else 0), (1 if kk == j + 1 else 0), (1 if i == j else 0)
                        acc += mp.mpf(float(g[kk])) * p[kk] * ((di - p[i + 1]) * (dj - p[j + 1]) - p[i + 1] * (dij - p[j + 1]))
                        scale = abs(float(g[kk])) * pf[kk] * ((di + pf[i + 1]) * (dj + pf[j + 1]) + pf[i + 1] * (dij + pf[j + 1]))
                        accb += scale * (rel[kk] + 2 * rel[i + 1] + 2 * rel[j + 1] + 8 + 2 * K)
                    T[i, j] = to_ld(acc)
                    Tb[i, j] = accb
    return P, pb * (U * SLACK), J, Jb * (U * SLACK), T, Tb * (U * SLACK)


# ---- whole layouts -----------------------------------------------------------------------------------------------------------------
def constrain(spec, theta, dtype=LD):
    """eta (dtype) and its absolute bound (float64)."""
    blocks, D, V = blocks_of(spec)
    eta, bnd = np.zeros(V, dtype=dtype), np.zeros(V)
    for b in blocks:
        f = np.asarray(theta[b['fo']:b['fo'] + b['nf']], dtype=np.float64)
        vs = slice(b['vo'], b['vo'] + b['nv'])
        if b['kind'] == 'box':
            val, bb = box_arrays(f, b['lb'], b['ub'])
            eta[vs], bnd[vs] = val[0].astype(dtype), bb[0]
        elif b['kind'] == 'psd':
            eta[vs] = psd_eta(f, b['k'], b['diag_lb'], dtype)
            bnd[vs] = k_psd_eta(b['k']) * U * SLACK * psd_eta(f, b['k'], b['diag_lb'], LD, True).astype(np.float64)
        else:
            K = b['K']
            for r in range(b['rows']):
                P, pb = simplex_row_all(f[r * (K - 1):(r + 1) * (K - 1)])[:2]
                eta[b['vo'] + r * K:b['vo'] + (r + 1) * K] = P.astype(dtype)
                bnd[b['vo'] + r * K:b['vo'] + (r + 1) * K] = pb
    return eta, bnd


def box_d(spec, theta):
    """Per box block: (values 3 x n longdouble, bounds 3 x n)."""
    blocks, _, _ = blocks_of(spec)
    return {b['name']: box_arrays(np.asarray(theta[b['fo']:b['fo'] + b['nf']], dtype=np.float64), b['lb'], b['ub'])
            for b in blocks if b['kind'] == 'box'}


def jt_apply(spec, theta, A, dtype=LD, absval=False, boxes=None):
    """J(theta)^T A (D x Q) in `dtype`; absval: |J|^T |A|.  Simplex blocks go through their dense row Jacobians."""
    blocks, D, V = blocks_of(spec)
    A = np.asarray(A, dtype=dtype)
    if absval:
        A = np.abs(A)
    boxes = box_d(spec, theta) if boxes is None else boxes
    out = np.zeros((D, A.shape[1]), dtype=dtype)
    for b in blocks:
        f = np.asarray(theta[b['fo']:b['fo'] + b['nf']], dtype=np.float64)
        fs, vs = slice(b['fo'], b['fo'] + b['nf']), slice(b['vo'], b['vo'] + b['nv'])
        if b['kind'] == 'box':
            d1 = boxes[b['name']][0][1].astype(dtype)
            out[fs] = (np.abs(d1) if absval else d1)[:, None] * A[vs]
        elif b['kind'] == 'psd':
            out[fs] = psd_jt_apply(f, b['k'], A[vs], dtype, absval)
        else:
            K = b['K']
            for r in range(b['rows']):
                J = simplex_row_all(f[r * (K - 1):(r + 1) * (K - 1)])[2].astype(dtype)
                if absval:
                    J = np.abs(J)
                out[b['fo'] + r * (K - 1):b['fo'] + (r + 1) * (K - 1)] = J.T @ A[b['vo'] + r * K:b['vo'] + (r + 1) * K]
    return out


def jt_count(spec):
    """K of one structured product, per free row (D,): the block's own count."""
    blocks, D, _ = blocks_of(spec)
    K = np.zeros(D)
    for b in blocks:
        fs = slice(b['fo'], b['fo'] + b['nf'])
        if b['kind'] == 'box':
            two = np.isfinite(b['lb']) and np.isfinite(b['ub'])
            one = np.isfinite(b['lb']) != np.isfinite(b['ub'])
            K[fs] = K_JT_BOX2 if two else (K_JT_BOX1 if one else 2)
        elif b['kind'] == 'psd':
            K[fs] = k_jt(b['k'])
        else:
            K[fs] = np.nan                                          # the dense route has no bound oracle here
    return K


def jt_apply_bounded(spec, theta, A):
    boxes = box_d(spec, theta)
    ref = jt_apply(spec, theta, A, LD, False, boxes)
    absm = jt_apply(spec, theta, A, LD, True, boxes).astype(np.float64)
    return ref, jt_count(spec)[:, None] * (U * SLACK) * absm


def jthj(spec, theta, H, dtype=LD, absval=False, boxes=None):
    """J^T H J = J^T (J^T H^T)^T."""
    boxes = box_d(spec, theta) if boxes is None else boxes
    W = jt_apply(spec, theta, np.asarray(H, dtype=dtype).T, dtype, absval, boxes)
    return jt_apply(spec, theta, W.T, dtype, absval, boxes)


def third_order(spec, theta, g, dtype=LD, boxes=None):
    """T (D x D) and its absolute bound."""
    blocks, D, V = blocks_of(spec)
    boxes = box_d(spec, theta) if boxes is None else boxes
    T, B = np.zeros((D, D), dtype=dtype), np.zeros((D, D))
    for b in blocks:
        f = np.asarray(theta[b['fo']:b['fo'] + b['nf']], dtype=np.float64)
        gb = np.asarray(g[b['vo']:b['vo'] + b['nv']], dtype=np.float64)
        fs = slice(b['fo'], b['fo'] + b['nf'])
        if b['kind'] == 'box':
            val, bb = boxes[b['name']]
            i = np.arange(b['fo'], b['fo'] + b['nf'])
            T[i, i] = gb.astype(dtype) * val[2].astype(dtype)
            B[i, i] = np.abs(gb) * bb[2] + 2 * U * SLACK * np.abs(gb * val[2].astype(np.float64))
        elif b['kind'] == 'psd':
            T[fs, fs] = psd_third(f, b['k'], gb, dtype)
            B[fs, fs] = k_psd_third(b['k']) * U * SLACK * psd_third(f, b['k'], gb, LD, True).astype(np.float64)
        else:
            K = b['K']
            for r in range(b['rows']):
                o = b['fo'] + r * (K - 1)
                res = simplex_row_all(f[r * (K - 1):(r + 1) * (K - 1)], gb[r * K:(r + 1) * K])
                T[o:o + K - 1, o:o + K - 1] = res[4].astype(dtype)
                B[o:o + K - 1, o:o + K - 1] = res[5]
    return T, B


def free_hessian_bounded(spec, theta, g, H):
    """J^T H J + T in longdouble and the bound of the device's two products plus the accumulated second-order term."""
    boxes = box_d(spec, theta)
    P = jthj(spec, theta, H, LD, False, boxes)
    Pabs = jthj(spec, theta, H, LD, True, boxes).astype(np.float64)
    T, Tb = third_order(spec, theta, g, LD, boxes)
    kk = jt_count(spec)
    ref = P + T
    bound = (kk[:, None] + kk[None, :]) * (U * SLACK) * Pabs + Tb + U * SLACK * np.abs(ref.astype(np.float64))
    return ref, bound


def dense_jac(spec, theta, dtype=LD):
    """V x D Jacobian (psd blocks from the definition: small k only) and its bound for the dense device kernels."""
    blocks, D, V = blocks_of(spec)
    boxes = box_d(spec, theta)
    J, B = np.zeros((V, D), dtype=dtype), np.zeros((V, D))
    for b in blocks:
        f = np.asarray(theta[b['fo']:b['fo'] + b['nf']], dtype=np.float64)
        fs, vs = slice(b['fo'], b['fo'] + b['nf']), slice(b['vo'], b['vo'] + b['nv'])
        if b['kind'] == 'box':
            val, bb = boxes[b['name']]
            J[vs, fs] = np.diag(val[1].astype(dtype))
            B[vs, fs] = np.diag(bb[1])
        elif b['kind'] == 'psd':
            Jb = psd_jac_dense_definition(f, b['k'], dtype)
            J[vs, fs] = Jb
            B[vs, fs] = K_PSD_JAC * U * SLACK * np.abs(Jb.astype(np.float64))
        else:
            K = b['K']
            for r in range(b['rows']):
                res = simplex_row_all(f[r * (K - 1):(r + 1) * (K - 1)])
                sl = (slice(b['vo'] + r * K, b['vo'] + (r + 1) * K), slice(b['fo'] + r * (K - 1), b['fo'] + (r + 1) * (K - 1)))
                J[sl], B[sl] = res[2].astype(dtype), res[3]
    return J, B


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def exact_theta(spec, rng):
    """0 on every exponentiated coordinate (log-Cholesky diagonals, bounded boxes, simplex logits), integers -3..3 elsewhere:
    L has a unit diagonal, eta' is 1 (one-sided) or r / 4 (two-sided), eta'' of a two-sided box is 0."""
    blocks, D, _ = blocks_of(spec)
    th = np.zeros(D)
    for b in blocks:
        fs = slice(b['fo'], b['fo'] + b['nf'])
        if b['kind'] == 'box' and not np.isfinite(b['lb']) and not np.isfinite(b['ub']):
            th[fs] = rng.integers(-3, 4, b['nf'])
        elif b['kind'] == 'psd':
            v = rng.integers(-3, 4, b['nf']).astype(np.float64)
            v[ld_idx(np.arange(b['k']), np.arange(b['k']))] = 0.0
            th[fs] = v
    return th


def int_matrix(rng, shape):
    return rng.integers(-3, 4, shape).astype(np.float64)


def real_theta(spec, rng):
    blocks, D, _ = blocks_of(spec)
    th = np.zeros(D)
    for b in blocks:
        fs = slice(b['fo'], b['fo'] + b['nf'])
        if b['kind'] == 'box':
            th[fs] = rng.uniform(-8, 8, b['nf'])
        elif b['kind'] == 'psd':
            v = 10.0 ** rng.uniform(-3, 1, b['nf']) * rng.choice([-1.0, 1.0], b['nf'])
            d = ld_idx(np.arange(b['k']), np.arange(b['k']))
            v[d] = rng.uniform(-6, 6, b['k'])
            th[fs] = v
        else:
            th[fs] = rng.uniform(-4, 4, b['nf'])
    return th


def real_matrix(rng, shape):
    """Normal entries, column j scaled by 10^u_j, u in [-3, 3]."""
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 3, shape[-1])


def assert_exact_margin(absmax, what=''):
    """Every exact result is a multiple of 1/16; 16 * (sum of absolute terms) must stay far below 2^53."""
    assert 16.0 * float(absmax) < 2.0 ** 53 / 1024, (what, float(absmax))


def assert_sixteenths(x, what=''):
    x = np.asarray(x, dtype=np.float64)
    assert np.array_equal(np.round(x * 16.0), x * 16.0), what


# ---- reports ------------------------------------------------------------------------------------------------------------------------
def locate_free(spec, row):
    blocks, _, _ = blocks_of(spec)
    for b in blocks:
        if b['fo'] <= row < b['fo'] + b['nf']:
            e = row - b['fo']
            if b['kind'] == 'psd':
                a = int((np.sqrt(8.0 * e + 1.0) - 1.0) / 2)
                while ld_idx(a + 1, 0) <= e:
                    a += 1
                while ld_idx(a, 0) > e:
                    a -= 1
                return b['name'], (a, e - ld_idx(a, 0))
            return b['name'], (e,)
    raise IndexError(row)


def describe_mismatch(spec, got, want):
    """First wrong entry as (block, (a, b), column), its 16-row MFMA tile mt, and the count of wrong entries per block."""
    got, want = np.asarray(got), np.asarray(want)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not bad.any():
        return ''
    rows = np.atleast_2d(bad.reshape(bad.shape[0], -1))
    r, c = np.argwhere(rows)[0]
    name, pos = locate_free(spec, int(r))
    per = {}
    for rr in np.flatnonzero(rows.any(axis=1)):
        nm = locate_free(spec, int(rr))[0]
        per[nm] = per.get(nm, 0) + int(rows[rr].sum())
    mt = pos[1] // 16 if len(pos) == 2 else None
    return 'first wrong entry: block {!r} {} column {} (mt = {}): got {!r}, want {!r}; wrong entries per block: {}'.format(
        name, pos, int(c), mt, float(got.reshape(rows.shape)[r, c]), float(want.reshape(rows.shape)[r, c]), per)


def ratio(got, ref, bound):
    """max |got - ref| / bound over the entries; an entry with bound 0 must be equal (ratio inf otherwise)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(q)) if q.size else 0.0


# ---- a NumPy emulation of jt_apply_kernel's gather, with single mistakes (tests/test_pack_reference_host_math.py) ----------------------
MISTAKES = ('no_factor_2', 'no_laa', 'skip_k_step', 'last_tile_unwritten', 'padding_not_zeroed', 'gather_swapped',
            'transposed_read_swapped', 'box_d2_sign')


def emulate_jt_psd(f, k, A, mistake=None, trans_in=False):
    """float64 emulation of the kernel's walk over one block: staging of G (factor 2, gather), L with zero padding, 16-row
    tiles mt with k-steps from 4 mt, the closing * L_aa.  A: m x Q (or Q x m when trans_in)."""
    kr, KP = (k + 3) & ~3, (k + 15) & ~15
    m = k * (k + 1) // 2
    Q = A.shape[0] if trans_in else A.shape[1]
    Lfull = chol_factor(f, k, np.float64)
    Ls = np.zeros((kr, KP))
    Ls[:k, :k] = Lfull
    if mistake == 'padding_not_zeroed':
        Ls[:k, :k] = Lfull + np.triu(np.full((k, k), 3.0), 1)          # stale values above the diagonal
    out = np.full((m, Q), 12345.0)                                     # what the output buffer held before
    for a in range(k):
        G = np.zeros((kr, Q))
        for t in range(k):
            if mistake == 'gather_swapped':
                v = ld_idx(a, t)                                       # (a, t) also for t > a: lands in row a + 1
            else:
                v = ld_idx(a, t) if t <= a else ld_idx(t, a)
            if trans_in:
                row = A[:, v] if mistake != 'transposed_read_swapped' else A[v, :]      # A square here
            else:
                row = A[v]
            G[t] = row * (2.0 if (t == a and mistake != 'no_factor_2') else 1.0)
        mt = 0
        while 16 * mt <= a:
            acc = np.zeros((16, Q))
            for kk in range(4 * mt + (1 if mistake == 'skip_k_step' else 0), kr // 4):
                for t in range(4 * kk, 4 * kk + 4):
                    acc += Ls[t, 16 * mt:16 * mt + 16, None] * G[t][None, :]
            last = 16 * (mt + 1) > a
            if not (mistake == 'last_tile_unwritten' and last):
                for b in range(16 * mt, min(16 * mt + 16, a + 1)):
                    out[ld_idx(a, b)] = acc[b - 16 * mt] * (Ls[a, a] if (b == a and mistake != 'no_laa') else 1.0)
            mt += 1
    return out


def box_eval_f64(f, lb, ub, complement='direct', d2_sign=1.0):
    """float64 NumPy of the device's box_eval.  complement: 'direct' takes 1 - s as ef / (1 + ef) for f >= 0 (the present
    code); 'subtract' is the earlier 1 - s everywhere, kept to record what it lost."""
    f = np.asarray(f, dtype=np.float64)
    has_lb, has_ub = np.isfinite(lb), np.isfinite(ub)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        if not has_lb and not has_ub:
            return f.copy(), np.ones_like(f), np.zeros_like(f)
        if has_lb and not has_ub:
            x = np.exp(f)
            return x + lb, x, d2_sign * x
        if has_ub and not has_lb:
            x = np.exp(-f)
            return ub - x, x, -d2_sign * x
        ef = np.exp(-np.abs(f))
        s = np.where(f >= 0, 1.0 / (1.0 + ef), ef / (1.0 + ef))
        cs = np.where(f >= 0, ef / (1.0 + ef), 1.0 - s) if complement == 'direct' else 1.0 - s
        r, sp = ub - lb, s * cs
        return r * s + lb, r * sp, d2_sign * (r * sp * (1.0 - 2.0 * s))


def simplex_row_f64(frow):
    """float64 NumPy of the device's simplex row: p, J, and the complement 1 - p_j as the kernels form it."""
    z = np.concatenate([[0.0], np.asarray(frow, dtype=np.float64)])
    mx = z.max()
    lse = mx + np.log(np.sum(np.exp(z - mx)))
    p = np.exp(z - lse)
    K = len(z)
    J = p[:, None] * (np.eye(K)[:, 1:] - p[None, 1:])
    return p, J


def simplex_third_f64(frow, g, drop_common=False):
    p, _ = simplex_row_f64(frow)
    K = len(p)
    T = np.zeros((K - 1, K - 1))
    for i in range(K - 1):
        for j in range(K - 1):
            s = 0.0
            for kk in range(K):
                di, dj = (1.0 if kk == i + 1 else 0.0) - p[i + 1], (1.0 if kk == j + 1 else 0.0) - p[j + 1]
                common = 0.0 if drop_common else p[i + 1] * ((1.0 if i == j else 0.0) - p[j + 1])
                s += g[kk] * p[kk] * (di * dj - common)
            T[i, j] = s
    return T


# ---- the layouts of tests/test_gpu_pack.py (shared with the host-math file) ------------------------------------------------------------
INF = np.inf


def a_spec(k, diag_lb=0.25):
    return [('box', 'lo', 3, -2.0, 5.0), ('psd', 'm', k, diag_lb), ('box', 'free', 2, -INF, INF)]


def d_spec(k):
    return [('box', 'lo', 3, 0.0, INF), ('box', 'hi', 2, -INF, 4.0), ('box', 'two', 2, -2.0, 5.0), ('psd', 'm', k, 0.5),
            ('box', 'free', 2, -INF, INF)]


def b_spec(k1, k2, nb):
    if nb == 1:                                       # ONE box block: the per-block box kernels, not the fused ones
        return [('psd', 'm1', k1, 0.5), ('box', 'hi', 1, -INF, 3.0), ('psd', 'm2', k2, 0.0)]
    n1 = nb // 3
    return [('box', 'lo', n1, 0.0, INF), ('psd', 'm1', k1, 0.5), ('box', 'two', n1, -1.0, 2.0), ('psd', 'm2', k2, 0.0),
            ('box', 'hi', nb - 2 * n1, -INF, 3.0)]


B_CASES = [(16, 17, 1), (17, 4, 15), (32, 33, 16), (33, 1, 17), (60, 61, 33), (63, 3, 15), (3, 5, 33)]
C_CASES = [(5, False), (17, False), (33, False), (63, False), (64, False), (65, False), (5, True), (17, True)]
A_EDGE_K = (16, 17, 32, 33, 48, 49, 60, 61, 63)
A_EDGE_Q = (1, 63, 64, 65, 128, 129)
G_F = [0.0, -0.0] + [s * v for v in (1e-300, 1.0, 10.0, 20.0, 30.0, 36.0, 37.0, 40.0, 700.0, 745.0, 800.0) for s in (1.0, -1.0)]
G_SPEC = [('box', 'free', len(G_F), -INF, INF), ('box', 'lo', len(G_F), 3.0, INF), ('box', 'hi', len(G_F), -INF, 4.0),
          ('box', 'two', len(G_F), -2.0, 5.0)]


def simplex_rows(K, rng):
    """Logit rows of case h: ordinary, all zeros, one logit at +700, one at -700, all at -700."""
    rows = [rng.uniform(-4, 4, K - 1), np.zeros(K - 1), rng.uniform(-4, 4, K - 1), rng.uniform(-4, 4, K - 1), np.full(K - 1, -700.0)]
    rows[2][0] = 700.0
    rows[3][-1] = -700.0
    return rows

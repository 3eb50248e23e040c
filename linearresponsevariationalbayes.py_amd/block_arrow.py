"""Host algebra of a symmetric block-arrow matrix: a dense global block Hgg (n_global x n_global), G local
2 K x 2 K blocks `loc` (G x 2 K x 2 K, group g in the coordinates [e_g0 .. e_g,K-1 | i_g0 .. i_g,K-1]) and a border Hx (R x 2 G K)
between the R coupled global coordinates `rows` and the local part of the vector, whose order is [e (G K, group-major) | i (G K)].
It is the Hessian of the logistic mixed models (glmm_slopes.py; the random intercept of glmm.py is K = 1).  Plain numpy and
scipy: nothing here touches the device.

The border is never regrouped: Hx viewed as (R, 2, G, K) gives coordinate i of every group as one R x G slab, a right-hand side
viewed as (2, G, K, Q) gives it as one G x Q slab, and the local factors L_g (A_g = L_g L_g^T) act on the slabs element-wise with
G-vectors as coefficients -- (2 K)^2 fused multiply-adds per triangular pair.  Each contraction over the groups is one GEMM.
"""
import numpy as np
from scipy import linalg as sp_linalg
from scipy import sparse as sp_sparse


def _to_groups(x, G, K):
    """Local part (2 G K [x Q], order [e (G K) | i (G K)]) -> G x 2 K x Q."""
    x = np.asarray(x, dtype=np.float64).reshape(2, G, K, -1)
    return np.concatenate([x[0], x[1]], axis=1)


def _from_groups(x, G, K):
    """G x 2 K x Q -> 2 G K x Q in the order of the local part."""
    return np.concatenate([x[:, :K].reshape(G * K, -1), x[:, K:].reshape(G * K, -1)], axis=0)


def _local_index(G, K):
    """Position, in the local part of the vector, of coordinate i of group g's block: G x 2 K."""
    gk = np.arange(G * K).reshape(G, K)
    return np.concatenate([gk, G * K + gk], axis=1)


def _local_chol(loc):
    """The Cholesky factors of all local blocks at once, from their lower triangles: (L, 1 / diag L) as 2 K x 2 K x G and 2 K x G,
    so that every entry is one contiguous G-vector.  The recurrence runs over the at most 8 rows, vectorised over the groups."""
    A = np.ascontiguousarray(np.asarray(loc, dtype=np.float64).transpose(1, 2, 0))
    n, G = A.shape[0], A.shape[2]
    L, dinv = np.zeros((n, n, G)), np.empty((n, G))
    for j in range(n):
        p = A[j, j] - np.sum(L[j, :j] ** 2, axis=0)
        if not np.all(p > 0):
            raise np.linalg.LinAlgError('a 2 K x 2 K local block is not positive definite')
        L[j, j] = np.sqrt(p)
        dinv[j] = 1.0 / L[j, j]
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j], axis=0)) * dinv[j]
    return L, dinv


def _forward(L, dinv, B, T, coef):
    """T_i = (B_i - sum_{j < i} L_ij T_j) / L_ii on lists of slabs (T may be B); `coef` shapes a G-vector to multiply a slab."""
    for i in range(len(B)):
        if T[i] is not B[i]:
            T[i][...] = B[i]
        for j in range(i):
            T[i] -= coef(L[i, j]) * T[j]
        T[i] *= coef(dinv[i])


def _backward(L, dinv, T, coef):
    """In place: X_i = (T_i - sum_{j > i} L_ji X_j) / L_ii."""
    n = len(T)
    for i in reversed(range(n)):
        for j in range(i + 1, n):
            T[i] -= coef(L[j, i]) * T[j]
        T[i] *= coef(dinv[i])


def _row_slabs(X, G, K):
    """The 2 K coordinate slabs (G x Q views) of a local part X (2 G K x Q)."""
    X4 = X.reshape(2, G, K, -1)
    return [X4[h, :, k] for h in range(2) for k in range(K)]


def _along_rows(c):
    return c[:, None]


def _local_solve_rows(chol, X, G, K):
    """In place: H_ll^-1 X for a local part X (2 G K x Q, C-contiguous)."""
    T = _row_slabs(X, G, K)
    _forward(*chol, T, T, _along_rows)
    _backward(*chol, T, _along_rows)
    return X


def _half_border(chol, Hx, G, K):
    """U (R x 2 K G) with U U^T = Hx H_ll^-1 Hx^T: slab i is row i of L_g^-1 C_g^T for every group."""
    R = Hx.shape[0]
    Hx4 = Hx.reshape(R, 2, G, K)
    U = np.empty((R, 2 * K, G))
    _forward(*chol, [Hx4[:, h, :, k] for h in range(2) for k in range(K)], [U[:, i] for i in range(2 * K)], lambda c: c)
    return U.reshape(R, 2 * K * G)


def block_arrow_to_free(cf, j1, j2, n_global, G, K, dense=None):
    """The pieces of `glmm_slopes_closed_forms` in FREE coordinates for an element-wise packing (j1 = d eta / d theta, j2 = its
    second derivative, both D-vectors): (grad, Hgg, rows, Hx, loc).
    dense = (lo, J, H2): the global coordinates lo .. lo + n - 1 are packed by a map with the dense n x n Jacobian J
    (d eta / d theta) and second derivative H2 (n x n x n, [eta, theta, theta]) instead -- the log-Cholesky map of a positive
    definite matrix; j1 must be 1 and j2 0 there.  The global Jacobian is then block-diagonal with this one dense block, and
    its second-order term enters the global block only."""
    g, ng = cf['grad'], n_global
    jg = j1[:ng]
    Hgg = cf['Hgg'] * jg[:, None] * jg[None, :] + np.diag(g[:ng] * j2[:ng])
    rows = cf['rows']
    Hx = None if cf['Hx'] is None else cf['Hx'] * jg[rows][:, None] * j1[ng:][None, :]
    if dense is not None:
        lo, J, H2 = dense
        sl = slice(lo, lo + J.shape[0])
        Hgg[:, sl] = Hgg[:, sl] @ J
        Hgg[sl, :] = J.T @ Hgg[sl, :]
        Hgg[sl, sl] += np.einsum('i,ipq->pq', g[sl], H2)
        g = g.copy()
        g[sl] = J.T @ g[sl]
        if Hx is not None:
            at = np.flatnonzero((rows >= lo) & (rows < lo + J.shape[0]))       # the block's coordinates among the coupled rows
            if at.size != J.shape[0]:
                raise ValueError('the dense block must lie within the coupled rows')
            Hx[at] = J.T @ Hx[at]
    jl = _to_groups(j1[ng:], G, K)[:, :, 0]
    dl = _to_groups(g[ng:] * j2[ng:], G, K)[:, :, 0]
    loc = cf['loc'] * jl[:, :, None] * jl[:, None, :]
    kk = np.arange(2 * K)
    loc[:, kk, kk] += dl
    return g * j1, Hgg, rows, Hx, loc


def block_arrow_matvec(Hgg, rows, Hx, loc, v):
    """H v for the block arrow: O(n_global^2 + P G K + G K^2)."""
    ng, G, K = Hgg.shape[0], loc.shape[0], loc.shape[1] // 2
    v = np.asarray(v, dtype=np.float64).ravel()
    vg, vl = v[:ng], v[ng:]
    og = Hgg @ vg
    og[rows] += Hx @ vl
    ol = Hx.T @ vg[rows] + _from_groups(np.einsum('gij,gj->gi', loc, _to_groups(vl, G, K)[:, :, 0]), G, K)[:, 0]
    return np.concatenate([og, ol])


def block_arrow_dense(Hgg, rows, Hx, loc):
    ng, G, K = Hgg.shape[0], loc.shape[0], loc.shape[1] // 2
    D = ng + 2 * G * K
    H = np.zeros((D, D))
    H[:ng, :ng] = Hgg
    H[rows, ng:] = Hx
    H[ng:, rows] = Hx.T
    li = ng + _local_index(G, K)
    H[li[:, :, None], li[:, None, :]] = loc
    return H


def block_arrow_sparse(Hgg, rows, Hx, loc):
    """The block arrow as a scipy CSR matrix: the non-zeros of the global block and of the border, every entry of the local blocks."""
    ng, G, K = Hgg.shape[0], loc.shape[0], loc.shape[1] // 2
    D = ng + 2 * G * K
    rows = np.asarray(rows)
    gr, gc = np.nonzero(Hgg)
    xr, xc = np.nonzero(Hx)
    li = ng + _local_index(G, K)
    lr = np.broadcast_to(li[:, :, None], loc.shape).ravel()
    lc = np.broadcast_to(li[:, None, :], loc.shape).ravel()
    data = np.concatenate([Hgg[gr, gc], Hx[xr, xc], Hx[xr, xc], np.asarray(loc).ravel()])
    ri = np.concatenate([gr, rows[xr], ng + xc, lr])
    ci = np.concatenate([gc, ng + xc, rows[xr], lc])
    return sp_sparse.coo_matrix((data, (ri, ci)), shape=(D, D)).tocsr()


def block_arrow_schur_term(rows, Hx, loc):
    """M = sum_g C_g A_g^-1 C_g^T on the coupled rows (host route; the device route is lrvb_glmm_slopes_schur / lrvb_glmm_schur)."""
    G, K = loc.shape[0], loc.shape[1] // 2
    U = _half_border(_local_chol(loc), Hx, G, K)
    return U @ U.T


def block_arrow_local_solve(loc, B):
    """A_g^-1 B_g for every group (B: G x 2 K [x Q])."""
    B = np.asarray(B, dtype=np.float64)
    G, n = loc.shape[0], loc.shape[1]
    X = B.reshape(G, n, -1).copy()
    T = [X[:, i] for i in range(n)]
    chol = _local_chol(loc)
    _forward(*chol, T, T, _along_rows)
    _backward(*chol, T, _along_rows)
    return X.reshape(B.shape)


def block_arrow_solve(Hgg, rows, Hx, loc, R, schur_solve=None):
    """H^-1 R for the block arrow (R: D x Q or a D-vector) without the dense matrix: the G local blocks are solved, the result is
    reduced onto the coupled global rows, the Schur complement is factored and solved, and the local parameters are
    back-substituted -- O(P G K Q + G K^3 + n_global^3).  `schur_solve` (n_global x Q -> n_global x Q) replaces the host
    factorisation of the Schur complement, e.g. by the factor resident on the global context after
    `global_hessian(..., want_host=False)` + `chol_factor_last`.  A local block or a Schur complement that is not positive
    definite raises `np.linalg.LinAlgError`."""
    ng, G, K = Hgg.shape[0], loc.shape[0], loc.shape[1] // 2
    R = np.asarray(R, dtype=np.float64)
    vec = R.ndim == 1
    R2 = R.reshape(ng + 2 * G * K, -1)
    chol = _local_chol(loc)
    tl = _local_solve_rows(chol, R2[ng:].copy(), G, K)                   # H_ll^-1 R_l
    rhs = R2[:ng].copy()
    rhs[rows] -= Hx @ tl
    if schur_solve is None:
        U = _half_border(chol, Hx, G, K)
        S = Hgg.copy()
        S[np.ix_(rows, rows)] -= U @ U.T
        L = np.linalg.cholesky(0.5 * (S + S.T))                          # LinAlgError where it is not positive definite
        xg = sp_linalg.cho_solve((L, True), rhs)
    else:
        xg = np.asarray(schur_solve(np.ascontiguousarray(rhs)), dtype=np.float64).reshape(ng, -1)
    tl -= _local_solve_rows(chol, Hx.T @ xg[rows], G, K)                 # H_ll^-1 H_lg x_g
    out = np.vstack([xg, tl])
    return out.ravel() if vec else out


def block_arrow_solve_by_phases(R, n_global, rows, s, forward, schur_solve, back):
    """H^-1 R for the block arrow (R: D x Q or a D-vector) where the local blocks and the border are held by somebody else -- the
    device (lrvb_glmm_slopes_solve_forward / _back) or a numpy restatement of it -- as L_g (A_g = L_g L_g^T) and U_g = L_g^-1 C_g,
    C_g (2 K x R) being group g's border with its coupled side in the coordinates of the holder: Hx[r, l] = s_r C_g[l, r].

        forward(R_local: G x 2 K x Q) -> sum_g U_g^T L_g^-1 R_local,g   (R x Q; the holder keeps T_g = L_g^-1 R_local,g)
        schur_solve(rhs: n_global x Q) -> S^-1 rhs                      (S = Hgg - Hx H_ll^-1 Hx^T)
        back(x_coupled: R x Q, = s o x_g[rows]) -> L_g^-T (T_g - U_g x_coupled)   (G x 2 K x Q)

    This function packs the local rows into groups (`_to_groups`), does the n_global-sized step in between and unpacks."""
    R = np.asarray(R, dtype=np.float64)
    vec = R.ndim == 1
    rows, s = np.asarray(rows), np.asarray(s, dtype=np.float64)
    ng, K = int(n_global), int(n_global) - len(rows)               # the K rows i_mu are the global rows that do not couple
    R2 = R.reshape(R.shape[0], -1)
    if K < 1 or (R2.shape[0] - ng) % (2 * K) or R2.shape[0] <= ng:
        raise ValueError('R must have n_global + 2 G K rows')
    G = (R2.shape[0] - ng) // (2 * K)
    red = np.asarray(forward(np.ascontiguousarray(_to_groups(R2[ng:], G, K)))).reshape(len(rows), -1)
    rhs = R2[:ng].copy()
    rhs[rows] -= s[:, None] * red
    xg = np.asarray(schur_solve(np.ascontiguousarray(rhs)), dtype=np.float64).reshape(ng, -1)
    xl = np.asarray(back(np.ascontiguousarray(s[:, None] * xg[rows]))).reshape(G, 2 * K, -1)
    out = np.vstack([xg, _from_groups(xl, G, K)])
    return out.ravel() if vec else out


# ---- group blocks of H^-1 and the variance of a row's linear predictor ---------------------------------------
def unpack_group_cov(buf, P, K):
    """The G' x (K K + K P) group-covariance buffer of the device, rows [Sigma_uu (K x K, row-major) | Sigma_ubeta (K x P, k-major)],
    as (cov_u G' x K x K, cov_beta_u G' x P x K)."""
    buf = np.asarray(buf, dtype=np.float64).reshape(-1, K * K + K * P)
    return buf[:, :K * K].reshape(-1, K, K).copy(), np.ascontiguousarray(buf[:, K * K:].reshape(-1, K, P).transpose(0, 2, 1))


def block_arrow_group_cov_by_phases(n_global, rows, P, K, s, schur_solve, group_blocks, n_closed=None):
    """The blocks of H^-1 that predictions need, where the local factor is held by somebody else (the device, or a numpy
    restatement of it) as L_g and U_g = L_g^-1 C_g with Hx[r, l] = s_r C_g[l, r] (`block_arrow_solve_by_phases`):

        schur_solve(rhs: n_global x R) -> S^-1 rhs;   W = (S^-1)[rows, rows] from the unit columns of `rows`
        group_blocks(W: R x R, s) -> (G + 1) x (K K + K P): row g = [(A_g^-1 + Y_g W Y_g^T)[:K, :K] | -(Y_g W)[:K, :P]],
                                     Y_g = L_g^-T (U_g diag(s)); row G = the pseudo-group [W[mu, mu] | W[mu, :P]]

    n_closed: the closed columns behind [m | i_beta] among the coupled rows (None: the 3 K of the independent-effects models).

    Returns (cov_beta P x P, the buffer)."""
    rows, s = np.asarray(rows), np.asarray(s, dtype=np.float64)
    R = len(rows)
    want = 2 * P + (3 * K if n_closed is None else int(n_closed))
    if R != want or s.shape != (R,):
        raise ValueError('expected the {} coupled rows and their scaling'.format(want))
    E = np.zeros((int(n_global), R))
    E[rows, np.arange(R)] = 1.0
    W = np.ascontiguousarray(np.asarray(schur_solve(E), dtype=np.float64).reshape(int(n_global), R)[rows])
    buf = np.asarray(group_blocks(W, s), dtype=np.float64)
    return W[:P, :P].copy(), buf


def _host_group_blocks(chol, U3, P, K, mu=None):
    """group_blocks of `block_arrow_group_cov_by_phases` in numpy from (L, 1 / diag L) of `_local_chol` and U3 (R x 2 K x G: slab i is
    row i of L_g^-1 C_g for every group).  mu: where the means of mu_k sit among the coupled rows (None: 2 P + 3 k)."""
    L, dinv = chol
    R, G = U3.shape[0], U3.shape[2]
    mu = 2 * P + 3 * np.arange(K) if mu is None else np.asarray(mu)

    def group_blocks(W, s):
        Y = [U3[:, i] * s[:, None] for i in range(2 * K)]
        _backward(L, dinv, Y, lambda c: c)
        Ye = np.stack(Y[:K])                                               # K x R x G: the rows of e_g.
        Eg = np.einsum('krg,rc->kcg', Ye, W)
        Ai = np.zeros((2 * K, 2 * K, G))                                   # A_g^-1, column by column
        for k in range(K):
            T = [np.full((1, G), 1.0 if i == k else 0.0) for i in range(2 * K)]
            _forward(L, dinv, T, T, lambda c: c)
            _backward(L, dinv, T, lambda c: c)
            for l in range(K):
                Ai[l, k] = T[l][0]
        uu = Ai[:K, :K].transpose(2, 0, 1) + np.einsum('kcg,lcg->gkl', Eg, Ye)
        ub = -Eg[:, :P].transpose(2, 0, 1)                                 # G x K x P
        buf = np.empty((G + 1, K * K + K * P))
        buf[:G, :K * K], buf[:G, K * K:] = uu.reshape(G, -1), ub.reshape(G, -1)
        buf[G, :K * K], buf[G, K * K:] = W[np.ix_(mu, mu)].ravel(), W[mu, :P].ravel()
        return buf
    return group_blocks


def block_arrow_group_cov(Hgg, rows, Hx, loc, P, K, population=False, mu=None):
    """(cov_beta P x P, cov_u G x K x K, cov_beta_u G x P x K): the blocks of H^-1 between the means of beta and the means e_g. of
    every group's effects, from the pieces of the block arrow -- O(G K R^2 + n_global^3), no dense matrix.  With
    Y_g = A_g^-1 C_g^T (2 K x R) and W = (S^-1)[rows, rows]:  Cov(rows, l_g) = -W Y_g^T,  Cov(l_g, l_g) = A_g^-1 + Y_g W Y_g^T.
    population=True appends the pseudo-group G of a population-level prediction (u = mu): cov_u[G] = W[mu, mu],
    cov_beta_u[G] = W[:P, mu].  mu: where the means of mu_k sit among the coupled rows (None: 2 P + 3 k of R = 2 P + 3 K)."""
    ng, G = Hgg.shape[0], loc.shape[0]
    R = len(rows)
    chol = _local_chol(loc)
    U = _half_border(chol, Hx, G, K)
    S = Hgg.copy()
    S[np.ix_(rows, rows)] -= U @ U.T
    Ls = np.linalg.cholesky(0.5 * (S + S.T))
    cov_beta, buf = block_arrow_group_cov_by_phases(ng, rows, P, K, np.ones(R), lambda rhs: sp_linalg.cho_solve((Ls, True), rhs),
                                                    _host_group_blocks(chol, U.reshape(R, 2 * K, G), P, K, mu),
                                                    n_closed=None if mu is None else R - 2 * P)
    cov_u, cov_bu = unpack_group_cov(buf, P, K)
    return (cov_beta, cov_u, cov_bu) if population else (cov_beta, cov_u[:G], cov_bu[:G])


def predict_rows(x, z, gid, offset, m, v, e, r, cov_beta, cov_u, cov_beta_u):
    """(rho, var_mf, var_lrvb) of rows with design (x N x P, z N x K), group index gid (into e, r, cov_u, cov_beta_u: the
    pseudo-group of a population-level row included) and offset (N, or None):
        rho = o + x . m + z . e_g,   var_mf = (x o x) . v + (z o z) . r_g,
        var_lrvb = x^T S_bb x + 2 x^T S_bu,g z + z^T S_uu,g z."""
    x, z, gid = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64), np.asarray(gid)
    rho = x @ m + np.sum(z * e[gid], axis=1)
    if offset is not None:
        rho = rho + np.asarray(offset, dtype=np.float64)
    var_mf = (x * x) @ v + np.sum(z * z * r[gid], axis=1)
    var_lr = (np.einsum('np,pq,nq->n', x, cov_beta, x) + 2.0 * np.einsum('np,npk,nk->n', x, cov_beta_u[gid], z)
              + np.einsum('nk,nkl,nl->n', z, cov_u[gid], z))
    return rho, var_mf, var_lr

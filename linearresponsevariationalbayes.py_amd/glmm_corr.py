"""Mixed models with K <= 4 CORRELATED random effects per group -- lme4's `(1 + x | g)`:

    u_g ~ N(mu, Lambda^-1),   Lambda ~ Wishart(nu0, W0^-1)  (E Lambda = nu0 W0^-1),   mu_k ~ N(mu0, 1 / kappa0),   beta_j ~ N(0, 1 / tau_beta)

with the likelihoods of the independent-effects classes (Bernoulli; Poisson with an offset) and q(beta) = UVNParamVector(P),
q(mu) = UVNParamVector(K), q(Lambda) = WishartParam(K) (df n, scale V), q(u) = UVNParamArray (G, K), pushed in this order.  q(u_g)
stays mean-field; the linear-response covariance on top is where the correlation shows.  Vector coordinates

    eta = [m (P) | i_beta (P) | e_mu (K) | i_mu (K) | n | vech V (Kv = K (K + 1) / 2, the order of vectorize_ld_matrix) | e (G K) | i (G K)]

n_global = 2 P + 2 K + 1 + Kv.  With d_g = e_g - e_mu, r = 1 / i, E Lambda = n V and E log|Lambda| = psi_K(n / 2) + K log 2 + log|V|:

    KL = data term (that of the independent-effects model: rho_n and s_n depend on (m, v, e, r) only)
       + 1/2 sum_g [ d_g^T E Lambda d_g + sum_k E Lambda_kk (r_gk + 1 / i_mu_k) ] - 1/2 G E log|Lambda|
       - 1/2 (nu0 - K - 1) E log|Lambda| + 1/2 tr(W0 E Lambda) - wishart_entropy(n, V)
       + sum_k [ 1/2 kappa0 ((e_mu_k - mu0)^2 + 1 / i_mu_k) + 1/2 log i_mu_k ] + 1/2 sum_gk log i_gk
       + 1/2 tau_beta sum_j (m_j^2 + 1 / i_beta_j) + 1/2 sum_j log i_beta_j

At K = 1 this is the independent-effects model under n = 2 a, V = 1 / (2 b), nu0 = 2 a0, W0 = 2 b0.

The Hessian is a block arrow whose closed border is DENSE: every e_gk couples to every e_mu_l and to every entry of (n, vech V).
The coupled global coordinates are [m | i_beta | e_mu (K) | n | vech V]: NC = K + 1 + Kv closed columns, R = 2 P + NC <= 143 (the
i_mu do not couple).  The closed entries of group g are affine in d_g (`glmm_corr_border_tables`), which is what the device
entries lrvb_glmm_arrow_schur / _solve_forward / _solve_back / _group_cov take; the O(N) entries, the streamed influence and the
predict entries are those of the independent-effects classes, unchanged.  V is packed by the log-Cholesky map: the global
Jacobian of the free coordinates is block-diagonal with one dense Kv x Kv block (`block_arrow_to_free(..., dense=)`).
"""
import numpy as np
from scipy import special

from . import expfam
from .block_arrow import (block_arrow_to_free, block_arrow_schur_term, block_arrow_group_cov, block_arrow_group_cov_by_phases,
                          _to_groups)
from . import _hip
from .glmm_slopes import _SlopesArrow, LogisticGLMMSlopesObjective
from .glmm_poisson import PoissonGLMMObjective
from .models import DeviceContext, sym_to_vech, vech_to_sym
from .packing import HyperVectorParam, pos_def_matrix_free_to_vector_jac, pos_def_matrix_free_to_vector_hess
from .quadform import duplication_matrix, vech_dupT


def n_closed(K):
    """NC: the closed columns [e_mu (K) | n | vech V] of the coupled rows."""
    return K + 1 + K * (K + 1) // 2


def corr_coupled_rows(P, K):
    """The R = 2 P + NC global coordinates the border couples to: [m | i_beta | e_mu | n | vech V] (the i_mu are skipped)."""
    return np.concatenate([np.arange(2 * P + K), 2 * P + 2 * K + np.arange(1 + K * (K + 1) // 2)])


def _split_eta_corr(eta, P, K, G):
    Kv = K * (K + 1) // 2
    ng = 2 * P + 2 * K + 1 + Kv
    o = 2 * P + 2 * K
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    return eta[:P], eta[P:2 * P], eta[2 * P:2 * P + K], eta[2 * P + K:o], float(eta[o]), vech_to_sym(eta[o + 1:ng]), e, ig


def _mv_polygamma(order, x, K):
    return float(np.sum(special.polygamma(order, x - 0.5 * np.arange(K))))


def glmm_corr_border_tables(K, n, V, jac=None):
    """(A0 2 K x NC, A1 2 K x K x NC): the closed border entries of group g, before the chain factors of the local coordinates,
    are closed_g[i][c] = A0[i][c] + sum_l A1[i][l][c] d_gl, i over [e_g. | r_g.], c over [e_mu (K) | n | vech V]:

        e_gk | e_mu_l: A0 = -n V_kl        e_gk | n: A1[k][l] = V_kl        e_gk | V_ab: A1[k][l] = n (d_ka d_lb + d_kb d_la), n d_ka d_la at a = b
        r_gk | n: A0 = 1/2 V_kk            r_gk | V_kk: A0 = 1/2 n

    jac (NC x NC): d closed coordinates / d the caller's coordinates; the NC axis of both tables is multiplied by it."""
    NC = n_closed(K)
    A0, A1 = np.zeros((2 * K, NC)), np.zeros((2 * K, K, NC))
    A0[:K, :K] = -n * V
    A1[:K, :, K] = V
    ra, rb = np.tril_indices(K)
    for j, (a, b) in enumerate(zip(ra, rb)):
        c = K + 1 + j
        if a == b:
            A1[a, a, c] = n
            A0[K + a, c] = 0.5 * n
        else:
            A1[a, b, c] = A1[b, a, c] = n
    A0[K + np.arange(K), K] = 0.5 * np.diag(V)
    if jac is not None:
        A0, A1 = A0 @ jac, A1 @ jac
    return np.ascontiguousarray(A0), np.ascontiguousarray(A1)


def glmm_corr_closed_forms(P, K, G, eta, data, tau_beta, mu0, kappa0, nu0, W0, want_hess=True):
    """The N-independent part of the model in VECTOR coordinates from the data pieces of `glmm_slopes_closed_forms` (same dict,
    same coordinates (m, v, e, r)).  Returns dict: 'value', 'grad' (D), and with want_hess 'Hgg' (n_global x n_global), 'rows'
    (`corr_coupled_rows`), 'Hx' (R x 2 G K; None without the border) and 'loc' (G x 2 K x 2 K, coordinates [e_g. | i_g.])."""
    eta = np.asarray(eta, dtype=np.float64)
    Kv, GK = K * (K + 1) // 2, G * K
    ng = 2 * P + 2 * K + 1 + Kv
    m, ib, e_mu, i_mu, n, V, e, ig = _split_eta_corr(eta, P, K, G)
    W0 = np.asarray(W0, dtype=np.float64)
    v, r = 1.0 / ib, 1.0 / ig
    d = e - e_mu[None, :]
    dsum = np.sum(d, axis=0)
    S = d.T @ d + np.diag(np.sum(r, axis=0) + G / i_mu)
    T = S + W0
    Vd = np.diag(V)
    value = (data['value'] + 0.5 * n * np.sum(V * T) - 0.5 * (G + nu0 - K - 1.0) * expfam.e_log_det_wishart(n, V)
             - expfam.wishart_entropy(n, V) + np.sum(0.5 * kappa0 * ((e_mu - mu0) ** 2 + 1.0 / i_mu) + 0.5 * np.log(i_mu))
             + 0.5 * np.sum(np.log(ig)) + 0.5 * tau_beta * (np.sum(m * m) + np.sum(v)) + 0.5 * np.sum(np.log(ib)))
    out = dict(value=float(value))
    if data.get('g_glob') is None:
        return out
    gd, gl = np.asarray(data['g_glob']), np.asarray(data['g_loc'])
    dv, dr = -v * v, -r * r
    g_v = gd[P:] + 0.5 * tau_beta
    g_r = gl[:, K:] + 0.5 * n * Vd[None, :]
    iem, iim, inn = 2 * P + np.arange(K), 2 * P + K + np.arange(K), 2 * P + 2 * K
    iV = inn + 1 + np.arange(Kv)
    Vi = np.linalg.inv(V)
    pg1, pg2 = _mv_polygamma(1, 0.5 * n, K), _mv_polygamma(2, 0.5 * n, K)
    g = np.empty(ng + 2 * GK)
    g[:P] = gd[:P] + tau_beta * m
    g[P:2 * P] = g_v * dv + 0.5 / ib
    g[iem] = -n * (V @ dsum) + kappa0 * (e_mu - mu0)
    g[iim] = -0.5 * (n * Vd * G + kappa0) / i_mu ** 2 + 0.5 / i_mu
    g[inn] = 0.5 * np.sum(V * T) + 0.25 * (n - G - nu0) * pg1 - 0.5 * K
    g[iV] = vech_dupT(0.5 * n * T - 0.5 * (G + nu0) * Vi)
    g[ng:ng + GK] = (gl[:, :K] + n * d @ V).ravel()
    g[ng + GK:] = (g_r * dr + 0.5 / ig).ravel()
    out['grad'] = g
    if not want_hess:
        return out
    Hb, B, L = np.asarray(data['Hb']), data.get('border'), np.asarray(data['loc'])
    eye = np.eye(K)
    Dup = duplication_matrix(K)
    Hgg = np.zeros((ng, ng))
    Hgg[:P, :P] = Hb[0] + tau_beta * np.eye(P)
    Hgg[:P, P:2 * P] = Hb[1] * dv[None, :]
    Hgg[P:2 * P, :P] = Hgg[:P, P:2 * P].T
    Hgg[P:2 * P, P:2 * P] = Hb[2] * dv[:, None] * dv[None, :] + np.diag(g_v * 2.0 * v ** 3 - 0.5 / ib ** 2)
    Hgg[np.ix_(iem, iem)] = G * n * V + kappa0 * eye
    Hgg[iem, inn] = Hgg[inn, iem] = -(V @ dsum)
    # d S / d e_mu_k = -(1_k dsum^T + dsum 1_k^T), d S / d i_mu_k = -G / i_mu_k^2 1_k 1_k^T; the V rows are Dup^T vec(1/2 n dS)
    dS_emu = -(eye[:, :, None] * dsum[None, None, :] + dsum[None, :, None] * eye[:, None, :])          # [k, a, b]
    Hgg[np.ix_(iem, iV)] = vech_dupT(0.5 * n * dS_emu)
    Hgg[np.ix_(iV, iem)] = Hgg[np.ix_(iem, iV)].T
    Hgg[iim, iim] = (n * Vd * G + kappa0) / i_mu ** 3 - 0.5 / i_mu ** 2
    Hgg[iim, inn] = Hgg[inn, iim] = -0.5 * Vd * G / i_mu ** 2
    dS_imu = -(G / i_mu ** 2)[:, None, None] * (eye[:, :, None] * eye[:, None, :])
    Hgg[np.ix_(iim, iV)] = vech_dupT(0.5 * n * dS_imu)
    Hgg[np.ix_(iV, iim)] = Hgg[np.ix_(iim, iV)].T
    Hgg[inn, inn] = 0.25 * pg1 + 0.125 * (n - G - nu0) * pg2
    Hgg[inn, iV] = Hgg[iV, inn] = vech_dupT(0.5 * T)
    Hgg[np.ix_(iV, iV)] = 0.5 * (G + nu0) * Dup.T @ np.kron(Vi, Vi) @ Dup
    rows = corr_coupled_rows(P, K)
    jl = np.concatenate([np.ones((G, K)), dr], axis=1)          # chain of the local coordinates [e | r(i)]
    loc = L * jl[:, :, None] * jl[:, None, :]
    loc[:, :K, :K] += n * V[None]
    kk = np.arange(K)
    loc[:, K + kk, K + kk] += g_r * 2.0 * r ** 3 - 0.5 / ig ** 2
    out.update(Hgg=Hgg, rows=rows, Hx=None, loc=loc)
    if B is None:
        return out
    B = np.asarray(B).reshape(G, 4, K, P)
    NC = n_closed(K)
    R = 2 * P + NC
    Hx = np.zeros((R, 2, G, K))                                 # [row, e or i, g, k]
    Hx[:P, 0] = B[:, 0].transpose(2, 0, 1)
    Hx[:P, 1] = B[:, 1].transpose(2, 0, 1) * dr[None]
    Hx[P:2 * P, 0] = B[:, 2].transpose(2, 0, 1) * dv[:, None, None]
    Hx[P:2 * P, 1] = B[:, 3].transpose(2, 0, 1) * dv[:, None, None] * dr[None]
    o = 2 * P
    Hx[o:o + K, 0] = -n * V[:, None, :]                        # [l, g, k] = -n V_kl
    Hx[o + K, 0] = d @ V
    # d S / d e_gk = 1_k d_g^T + d_g 1_k^T, d S / d r_gk = 1_k 1_k^T
    dS_e = eye[None, :, :, None] * d[:, None, None, :] + d[:, None, :, None] * eye[None, :, None, :]   # [g, k, a, b]
    Hx[o + K + 1:, 0] = vech_dupT(0.5 * n * dS_e).transpose(2, 0, 1)
    Hx[o + K, 1] = 0.5 * Vd[None, :] * dr
    dS_r = eye[:, :, None] * eye[:, None, :]
    Hx[o + K + 1:, 1] = vech_dupT(0.5 * n * dS_r).T[:, None, :] * dr[None]
    out['Hx'] = Hx.reshape(R, 2 * GK)
    return out


class _CorrelatedArrow(_SlopesArrow):
    """`_SlopesArrow` for correlated effects: the parameter layout above, the closed forms, the dense block of the free Jacobian,
    and the Schur entry, the device-resident solve and the group covariance on the lrvb_glmm_arrow_* entries."""

    # ---- layout ---------------------------------------------------------------------------------------------------------------
    def _n_global(self):
        return 2 * self.P + 2 * self.K + 1 + self.K * (self.K + 1) // 2

    def _split(self, eta):
        return _split_eta_corr(eta, self.P, self.K, self.G)

    def _layout(self, par, names):
        P, K, G = self.P, self.K, self.G
        ng, GK, o = self._n_global(), G * K, 2 * P + 2 * K
        want = [(names[0], 'mean', 0, P), (names[0], 'info', P, 2 * P), (names[1], 'mean', 2 * P, 2 * P + K), (names[1], 'info', 2 * P + K, o),
                (names[2], 'df', o, o + 1), (names[2], 'v', o + 1, ng), (names[3], 'mean', ng, ng + GK), (names[3], 'info', ng + GK, ng + 2 * GK)]
        msg = ('the parameter must be [UVNParamVector {} ({}) | UVNParamVector {} ({}) | WishartParam {} ({}) | UVNParamArray {} ({}, {})] '
               'in this order, the group effects pushed last'.format(names[0], P, names[1], K, names[2], K, names[3], G, K))
        if any(name not in par.vector_indices_dict for name, _, _, _ in want):
            raise ValueError(msg)
        return want, msg, 'the parameter holds more than the blocks of the model'

    def _index_packing(self, par):
        lb = []
        for blk in par.layout_blocks():
            if blk['kind'] == _hip.BLOCK_PSD and len(lb) == 2 * self.P + 2 * self.K + 1 and blk['dim0'] == self.K:
                lb.extend([-np.inf] * blk['vec_size'])           # the log-Cholesky block of V: `_dense_block`, 1 and 0 element-wise
                continue
            if blk['kind'] != _hip.BLOCK_BOX or np.isfinite(blk['ub']) or blk['free_size'] != blk['vec_size']:
                raise ValueError('every coordinate but the scale matrix must be unconstrained or bounded below only')
            lb.extend([blk['lb']] * blk['vec_size'])
        self._lb = np.asarray(lb, dtype=np.float64)
        self._bounded = np.isfinite(self._lb)

    def _declare_effect_prior(self, lambda_prior):
        K = self.K
        nu0, W0 = (K + 1.0, np.eye(K)) if lambda_prior is None else lambda_prior
        W0 = np.atleast_2d(_hip.as_f64(W0))
        if W0.shape != (K, K) or not float(nu0) > K - 1:
            raise ValueError('lambda_prior must be (nu0 > K - 1, W0 K x K)')
        self._declare_hyper('lambda_prior', HyperVectorParam('lambda_prior', 1 + K * (K + 1) // 2,
                                                             val=np.concatenate([[float(nu0)], sym_to_vech(W0)])))

    nu0 = property(lambda self: float(self._hyper_vec('lambda_prior')[0]))
    W0 = property(lambda self: vech_to_sym(self._hyper_vec('lambda_prior')[1:]))

    # ---- closed forms and free coordinates ----------------------------------------------------------------------------------------
    def _closed(self, eta, want_grad=True, want_hess=True, want_border=True):
        d = self._data(eta, want_grad, want_hess, want_border)
        if not (want_grad or want_hess):
            d = dict(value=d['value'])
        return glmm_corr_closed_forms(self.P, self.K, self.G, eta, d, self.tau_beta, self.mu0, self.kappa0, self.nu0, self.W0,
                                      want_hess=want_hess)

    def _dense_block(self, eta):
        """(first coordinate, J, H2) of the log-Cholesky map of V at the point `par` holds (set by `_eta`)."""
        free_v = np.asarray(self.par[self._names[2]]['v'].get_free(), dtype=np.float64)
        return 2 * self.P + 2 * self.K + 1, pos_def_matrix_free_to_vector_jac(free_v), pos_def_matrix_free_to_vector_hess(free_v)

    def _global_jac_T(self, C, eta):
        lo, J, _ = self._dense_block(eta)
        out = np.array(super()._global_jac_T(C, eta))
        out[lo:lo + J.shape[0]] = J.T @ out[lo:lo + J.shape[0]]
        return out

    def _arrow_to_free(self, cf, eta):
        j1, j2 = self._jac(eta)
        return block_arrow_to_free(cf, j1, j2, self.n_global, self.G, self.K, dense=self._dense_block(eta))

    # ---- the coupled layout ---------------------------------------------------------------------------------------------------------
    def _coupled_rows(self):
        return corr_coupled_rows(self.P, self.K)

    def _coupled_scaling(self, eta):
        """Ones on the closed columns: the tables already carry the Jacobian of the free coordinates there."""
        P = self.P
        j1 = self._jac(eta)[0]
        return np.concatenate([j1[:P], -j1[P:2 * P] / eta[P:2 * P] ** 2, np.ones(n_closed(self.K))])

    def _closed_jac(self, eta):
        """d [e_mu | n | vech V] / d their free coordinates (NC x NC): identity, exp above the lower bound, the log-Cholesky map."""
        K, NC = self.K, n_closed(self.K)
        lo, J, _ = self._dense_block(eta)
        Jc = np.eye(NC)
        Jc[K, K] = self._jac(eta)[0][lo - 1]
        Jc[K + 1:, K + 1:] = J
        return Jc

    def _device_schur(self, eta, loc_f):
        """sum_g C_g^T A_g^-1 C_g over [m | v | the closed columns in FREE coordinates] from the resident group sums."""
        K, G, ng = self.K, self.G, self.n_global
        _, _, e_mu, _, n, V, e, ig = self._split(eta)
        r = 1.0 / ig
        A0, A1 = glmm_corr_border_tables(K, n, V, self._closed_jac(eta))
        jl = _to_groups(self._jac(eta)[0][ng:], G, K)[:, :, 0]
        scale = np.concatenate([jl[:, :K], -r * r * jl[:, K:]], axis=1)
        iu = np.triu_indices(2 * K)
        return self.ctx.glmm_arrow_schur(loc_f[:, iu[0], iu[1]], scale, e - e_mu[None, :], A0, A1)

    def _ensure_gctx(self):
        """The global context holds the Schur complement ALREADY in free coordinates (`global_hessian`): its layout is one
        unconstrained block of n_global coordinates, so that its packing step is the identity."""
        if not hasattr(self, '_gctx'):
            ng = self.n_global
            blocks = [dict(kind=_hip.BLOCK_BOX, free_size=ng, vec_size=ng, dim0=ng, dim1=0, lb=-np.inf, ub=np.inf)]
            self._gctx = DeviceContext(blocks, quad_kind=_hip.QUAD_DIAG, device=self.ctx.device)
        return self._gctx

    @_hip.host_blas
    def global_hessian(self, free_val, want_host=True):
        """H_S = H_gg - H_gl H_ll^-1 H_lg in FREE coordinates, as the independent-effects classes give it.  The global block is
        taken to free coordinates on the host (its Jacobian has a dense block and n_global <= 147); the elimination runs on the
        device (lrvb_glmm_arrow_schur) from tables that carry the free Jacobian of the closed columns.  The result stays
        resident on the global context for `chol_factor_last`."""
        fv = _hip.as_f64(free_val).ravel()
        ng = self.n_global
        self._push_state()
        self._dev_factor_key = None
        eta = self._eta(fv, True)
        cf = self._closed(eta, want_border=False)    # the group sums of the point stay resident; the border is not copied back
        g, Hgg, rows, Hx, loc_f = self._arrow_to_free(cf, eta)
        if self._external_stats is None:
            s = self._coupled_scaling(eta)
            M = self._device_schur(eta, loc_f) * s[:, None] * s[None, :]
        else:
            M = block_arrow_schur_term(rows, Hx, loc_f)
        Hgg = Hgg.copy()
        Hgg[np.ix_(rows, rows)] -= M
        gc = self._ensure_gctx()
        gc.hvec_begin()
        gc.hvec_add_block(Hgg, 0, 0)
        out = gc.hvec_finish(fv[:ng], g[:ng], True, want_host=want_host)      # an identity packing: see `_ensure_gctx`
        self._schur_key = self._resident_key(fv)
        return out

    def _solve_entries(self):
        NC = n_closed(self.K)
        return (lambda Rl: self.ctx.glmm_arrow_solve_forward(Rl, NC)), (lambda xc: self.ctx.glmm_arrow_solve_back(xc, self.G, self.K, NC))

    def _group_cov_phases(self, s):
        P, K, G, NC = self.P, self.K, self.G, n_closed(self.K)
        return block_arrow_group_cov_by_phases(self.n_global, self._coupled_rows(), P, K, s, self._ensure_gctx().chol_solve,
                                               lambda W, sc: self.ctx.glmm_arrow_group_cov(W, sc, G, K, NC), n_closed=NC)

    def _host_group_cov(self, x):
        _, Hgg, rows, Hx, loc = self._arrow(x, True)
        return block_arrow_group_cov(Hgg, rows, Hx, loc, self.P, self.K, population=True, mu=2 * self.P + np.arange(self.K))

    # ---- hyper-parameters -----------------------------------------------------------------------------------------------------------
    def _prior_hyper(self, kind, eta_g, want):
        """lambda_prior = [nu0 | vech W0]: the KL is linear in it, -1/2 nu0 E log|Lambda| + 1/2 n tr(W0 V) + const."""
        if kind != 'lambda_prior':
            return super()._prior_hyper(kind, eta_g, want)
        P, K, ng = self.P, self.K, self.n_global
        o = 2 * P + 2 * K
        n, V = float(eta_g[o]), vech_to_sym(eta_g[o + 1:ng])
        ra, rb = np.tril_indices(K)
        fac = np.where(ra == rb, 0.5, 1.0)
        if want == 'grad':
            return np.concatenate([[-0.5 * expfam.e_log_det_wishart(n, V)], n * V[ra, rb] * fac])
        C = np.zeros((ng, 1 + ra.size))
        C[o, 0] = -0.25 * _mv_polygamma(1, 0.5 * n, K)
        C[o + 1:, 0] = -0.5 * vech_dupT(np.linalg.inv(V))
        C[o, 1:] = V[ra, rb] * fac
        C[o + 1 + np.arange(ra.size), 1 + np.arange(ra.size)] = n * fac
        return C

    def ranef_cov(self, x, is_free=True):
        """(E Lambda^-1 = V^-1 / (n - K - 1), its correlation matrix): the fitted covariance of the random effects."""
        _, _, _, _, n, V, _, _ = self._split(self._eta(x, is_free))
        if not n > self.K + 1:
            raise ValueError('E Lambda^-1 needs n > K + 1 (n = {})'.format(n))
        C = np.linalg.inv(V) / (n - self.K - 1.0)
        sd = np.sqrt(np.diag(C))
        return C, C / sd[:, None] / sd[None, :]


class LogisticGLMMCorrObjective(_CorrelatedArrow, LogisticGLMMSlopesObjective):
    def __init__(self, par, x, y, z, groups, n_groups, beta_prior_info=1.0, mu_prior=(0.0, 1.0), lambda_prior=None, gh_deg=20,
                 names=('beta', 'mu', 'lam', 'u'), weights=None, device=0):
        """names: the parameters of q(beta), q(mu), q(Lambda) (a WishartParam of size K) and q(u).  lambda_prior = (nu0, W0),
        default (K + 1, I)."""
        LogisticGLMMSlopesObjective.__init__(self, par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, lambda_prior, gh_deg, names,
                                             weights, device)

    def _row_psi_derivs(self, rho, s):
        """(psi_rho, psi_s) by the rule the kernels use (Stein's identity on the nodes: psi_rho = E sigma(t), psi_s =
        E sigma'(t) / 2, as `BinomialGLMMObjective` has it), so that the dense weight cross Hessian is the derivative of the
        same function as the streamed rows at ANY point.  The inherited form differentiates the quadrature sum in sqrt(s)
        instead, which agrees only where the variances are small (1.9e-5 relative apart at s of order one, 20 nodes)."""
        t = rho[:, None] + np.sqrt(np.maximum(s, 0.0))[:, None] * (np.sqrt(2.0) * self.gh_x)[None, :]
        sg = special.expit(t)
        wk = self.gh_w / np.sqrt(np.pi)
        return sg @ wk, 0.5 * ((sg * (1.0 - sg)) @ wk)


class PoissonGLMMCorrObjective(_CorrelatedArrow, PoissonGLMMObjective):
    def __init__(self, par, x, y, z, groups, n_groups, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0), lambda_prior=None,
                 names=('beta', 'mu', 'lam', 'u'), weights=None, device=0):
        """As `PoissonGLMMObjective` with the Wishart precision of `LogisticGLMMCorrObjective`."""
        PoissonGLMMObjective.__init__(self, par, x, y, z, groups, n_groups, offset, beta_prior_info, mu_prior, lambda_prior, names, weights,
                                      device)

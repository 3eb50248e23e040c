"""Logistic mixed model with K <= 4 independent random effects per group -- random slopes:

    y_n ~ Bernoulli(sigma(x_n . beta + z_n . u_{g(n)})),   z_n in R^K,   u_gk ~ N(mu_k, 1 / tau_k) independently over k

with beta_j ~ N(0, 1 / tau_beta), mu_k ~ N(mu0, 1 / kappa0), tau_k ~ Gamma(a0, b0) (the K components share the hyper-parameters)
and q(beta) = UVNParamVector(P), q(mu) = UVNParamVector(K), q(tau_k) = K GammaParams, q(u) = UVNParamArray (G, K), pushed in this
order.  `z` is its own N x K array: a column of ones for an intercept, `x[:, cols]` for slopes.  Vector coordinates

    eta = [m (P) | i_beta (P) | e_mu (K) | i_mu (K) | a_0, b_0, .., a_{K-1}, b_{K-1} | e (G K, group-major) | i (G K)]

n_global = 2 P + 4 K, D = 2 P + 4 K + 2 G K (the order the parameter classes themselves give: ArrayParam flattens in C order).

    KL(eta) =  sum_n w_n [ psi(rho_n, s_n) - y_n rho_n ]     rho_n = x_n . m + z_n . e_g,  s_n = (x_n o x_n) . v + (z_n o z_n) . r_g
             + sum_k { 1/2 E tau_k ( sum_g [(e_gk - e_mu_k)^2 + 1 / i_gk] + G / i_mu_k ) - 1/2 G E log tau_k
                       + 1/2 kappa0 ((e_mu_k - mu0)^2 + 1 / i_mu_k) - (a0 - 1) E log tau_k + b0 E tau_k
                       + 1/2 log i_mu_k + 1/2 sum_g log i_gk - gamma_entropy(a_k, b_k) }
             + 1/2 tau_beta sum_j (m_j^2 + 1 / i_beta_j) + 1/2 sum_j log i_beta_j            (v = 1 / i_beta, r = 1 / i)

The O(N) work is `lrvb_glmm_slopes_terms` (csrc/k_glmm_slopes.hip); everything N-independent is `glmm_slopes_closed_forms`
below, plain numpy on the data pieces.  The Hessian is a block arrow: a dense global block, G local 2 K x 2 K blocks in the
coordinates [e_g0 .. e_g,K-1 | i_g0 .. i_g,K-1] and a border of R = 2 P + 3 K coupled global rows
[m | i_beta | e_mu_0, a_0, b_0, .., e_mu_{K-1}, a_{K-1}, b_{K-1}] (the i_mu_k do not couple).  At K = 1 with z = 1 the model is
`LogisticGLMMObjective`.  The observation weights are the hyper-parameter `weights_par` (the constructor's `weights=` is its
initial value); `obs_influence`, `group_influence` and `ParametricSensitivityLinearApproximation(..., stream_hyper=True)` stream
the sensitivity of any moment to them (`lrvb_glmm_slopes_obs_influence`, `lrvb_glmm_slopes_group_influence`).
`solve`, `lrvb_cov` and the two influence methods take `on_device=True`: the block-arrow solve then runs on the factors the
elimination left on the device (`block_arrow_solve_by_phases`) and the border never reaches the host.

The host algebra of the block arrow is `block_arrow.py` (re-exported here); everything of the objective that is not a device
entry is `_LogisticMixedModel`, which `LogisticGLMMObjective` (glmm.py) instantiates at K = 1.
What the K-effect models share whatever their likelihood -- the layout, the Schur entry, the device-resident solve -- is `_SlopesArrow`,
which `PoissonGLMMObjective` (glmm_poisson.py) inherits as well.  The coupled layout itself sits behind
four hooks of `_SlopesArrow` (`_coupled_rows`, `_coupled_scaling`, `_solve_entries`, `_group_cov_phases`), which `_CorrelatedArrow`
(glmm_corr.py, DESIGN.md section 34: correlated effects, a dense closed border) replaces.
"""
import numpy as np
from scipy import special

from . import _hip
from .block_arrow import (block_arrow_to_free, block_arrow_matvec, block_arrow_dense, block_arrow_sparse,    # noqa: F401 (re-exported)
                          block_arrow_schur_term, block_arrow_local_solve, block_arrow_solve, block_arrow_solve_by_phases,
                          block_arrow_group_cov, block_arrow_group_cov_by_phases, unpack_group_cov, predict_rows,
                          _to_groups, _from_groups, _local_index, _local_chol)
from .models import DeviceContext, DeviceModel
from .packing import HyperVectorParam
from .quadform import gamma_prior_hyper_grad, gamma_prior_hyper_cross
from .hierarchical import _gamma_block, _gamma_entropy


def group_sums_ncol(P, K):
    """(scalar columns, all columns) of one group's sums (include/lrvb_hip.h, lrvb_glmm_slopes_terms)."""
    nsc = 2 * K + K * (2 * K + 1)
    return nsc, nsc + 4 * K * P


def unpack_group_sums(gs, P, K):
    """The G x ncol (or G x nsc, without the border) group sums of the device as the data pieces of `glmm_slopes_closed_forms`:
    (g_loc G x 2 K, loc G x 2 K x 2 K symmetric, border G x 4 K x P or None)."""
    gs = np.asarray(gs, dtype=np.float64)
    G = gs.shape[0]
    K2 = 2 * K
    nsc, ncol = group_sums_ncol(P, K)
    iu = np.triu_indices(K2)
    loc = np.zeros((G, K2, K2))
    loc[:, iu[0], iu[1]] = gs[:, K2:nsc]
    loc[:, iu[1], iu[0]] = gs[:, K2:nsc]
    border = gs[:, nsc:].reshape(G, 4 * K, P) if gs.shape[1] == ncol else None
    return gs[:, :K2], loc, border


def pack_group_sums(g_loc, loc, border):
    """Inverse of `unpack_group_sums` (with the border)."""
    G, K2 = g_loc.shape
    iu = np.triu_indices(K2)
    return np.hstack([g_loc, loc[:, iu[0], iu[1]], np.asarray(border).reshape(G, -1)])


def coupled_rows(P, K):
    """The R = 2 P + 3 K global coordinates the border couples to: [m | i_beta | e_mu_k, a_k, b_k per k]."""
    iem, ia = 2 * P + np.arange(K), 2 * P + 2 * K + 2 * np.arange(K)
    return np.concatenate([np.arange(2 * P), np.stack([iem, ia, ia + 1], axis=1).ravel()])


def _split_eta(eta, P, K, G):
    ng = 2 * P + 4 * K
    m, ib = eta[:P], eta[P:2 * P]
    e_mu, i_mu = eta[2 * P:2 * P + K], eta[2 * P + K:2 * P + 2 * K]
    a, b = eta[2 * P + 2 * K:ng:2], eta[2 * P + 2 * K + 1:ng:2]
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    return m, ib, e_mu, i_mu, a, b, e, ig


def glmm_slopes_closed_forms(P, K, G, eta, data, tau_beta, mu0, kappa0, a0, b0, want_hess=True):
    """The N-independent part of the model, in VECTOR coordinates, from the data-dependent pieces.

    data: dict of the data term in the coordinates (m, v = 1 / i_beta, e, r = 1 / i): 'value', 'g_glob' (2 P: d/dm, d/dv),
    'g_loc' (G x 2 K: [sum a1 z | sum a2 z o z]), and for the Hessian 'Hb' (3 x P x P: mm, mv, vv), 'loc' (G x 2 K x 2 K: the
    blocks sum c q q^T, q = [z | z o z]) and 'border' (G x 4 K x P, row b K + k: sum c11 z_k x | sum c12 z_k^2 x |
    sum c12 z_k x o x | sum c22 z_k^2 x o x for b = 0..3; None where it stayed on the device).

    Returns dict: 'value', 'grad' (D), and with want_hess 'Hgg' (n_global x n_global), 'rows' (the R = 2 P + 3 K coupled global
    coordinates, [m | i_beta | e_mu_k, a_k, b_k per k]), 'Hx' (R x 2 G K, columns in the order of eta's local part; None without
    the border) and 'loc' (G x 2 K x 2 K, coordinates [e_g. | i_g.])."""
    eta = np.asarray(eta, dtype=np.float64)
    ng, GK = 2 * P + 4 * K, G * K
    m, ib, e_mu, i_mu, a, b, e, ig = _split_eta(eta, P, K, G)
    v, r = 1.0 / ib, 1.0 / ig
    Et, EL = a / b, special.digamma(a) - np.log(b)
    d = e - e_mu[None, :]
    Am = np.sum(d * d + r, axis=0) + G / i_mu                  # (K)
    value = (data['value'] + np.sum(0.5 * Et * Am - 0.5 * G * EL + 0.5 * kappa0 * ((e_mu - mu0) ** 2 + 1.0 / i_mu)
                                    - (a0 - 1.0) * EL + b0 * Et + 0.5 * np.log(i_mu) - _gamma_entropy(a, b))
             + 0.5 * np.sum(np.log(ig)) + 0.5 * tau_beta * (np.sum(m * m) + np.sum(v)) + 0.5 * np.sum(np.log(ib)))
    out = dict(value=float(value))
    if data.get('g_glob') is None:
        return out
    gd, gl = np.asarray(data['g_glob']), np.asarray(data['g_loc'])
    dv, dr = -v * v, -r * r                                    # d v / d i_beta, d r / d i
    g_v = gd[P:] + 0.5 * tau_beta
    g_r = gl[:, K:] + 0.5 * Et[None, :]
    dsum = np.sum(d, axis=0)
    iem, iim = 2 * P + np.arange(K), 2 * P + K + np.arange(K)
    ia = 2 * P + 2 * K + 2 * np.arange(K)
    ibb = ia + 1
    g = np.empty(ng + 2 * GK)
    g[:P] = gd[:P] + tau_beta * m
    g[P:2 * P] = g_v * dv + 0.5 / ib
    g[iem] = -Et * dsum + kappa0 * (e_mu - mu0)
    g[iim] = -0.5 * (Et * G + kappa0) / i_mu ** 2 + 0.5 / i_mu
    Hab = []
    for k in range(K):
        gab, H2 = _gamma_block(a[k], b[k], 0.5 * Am[k] + b0, -0.5 * G - (a0 - 1.0))
        g[ia[k]], g[ibb[k]] = gab
        Hab.append(H2)
    g[ng:ng + GK] = (gl[:, :K] + Et[None, :] * d).ravel()
    g[ng + GK:] = (g_r * dr + 0.5 / ig).ravel()
    out['grad'] = g
    if not want_hess:
        return out
    Hb, B, L = np.asarray(data['Hb']), data.get('border'), np.asarray(data['loc'])
    ta, tb = 1.0 / b, -a / b ** 2                              # d E tau / d a, d E tau / d b
    Hgg = np.zeros((ng, ng))
    Hgg[:P, :P] = Hb[0] + tau_beta * np.eye(P)
    Hgg[:P, P:2 * P] = Hb[1] * dv[None, :]
    Hgg[P:2 * P, :P] = Hgg[:P, P:2 * P].T
    Hgg[P:2 * P, P:2 * P] = Hb[2] * dv[:, None] * dv[None, :] + np.diag(g_v * 2.0 * v ** 3 - 0.5 / ib ** 2)
    for k in range(K):
        em, im, ka, kb = iem[k], iim[k], ia[k], ibb[k]
        Hgg[em, em] = Et[k] * G + kappa0
        Hgg[em, ka] = Hgg[ka, em] = -dsum[k] * ta[k]
        Hgg[em, kb] = Hgg[kb, em] = -dsum[k] * tb[k]
        Hgg[im, im] = (Et[k] * G + kappa0) / i_mu[k] ** 3 - 0.5 / i_mu[k] ** 2
        Hgg[im, ka] = Hgg[ka, im] = -0.5 * G / i_mu[k] ** 2 * ta[k]
        Hgg[im, kb] = Hgg[kb, im] = -0.5 * G / i_mu[k] ** 2 * tb[k]
        Hgg[ka:kb + 1, ka:kb + 1] = Hab[k]
    rows = coupled_rows(P, K)
    jl = np.concatenate([np.ones((G, K)), dr], axis=1)          # chain of the local coordinates [e | r(i)]
    loc = L * jl[:, :, None] * jl[:, None, :]
    kk = np.arange(K)
    loc[:, kk, kk] += Et[None, :]
    loc[:, K + kk, K + kk] += g_r * 2.0 * r ** 3 - 0.5 / ig ** 2
    out.update(Hgg=Hgg, rows=rows, Hx=None, loc=loc)
    if B is None:                                              # the border stayed on the device (global_hessian)
        return out
    B = np.asarray(B).reshape(G, 4, K, P)
    R = 2 * P + 3 * K
    Hx = np.zeros((R, 2, G, K))                                 # [row, e or i, g, k]
    Hx[:P, 0] = B[:, 0].transpose(2, 0, 1)
    Hx[:P, 1] = B[:, 1].transpose(2, 0, 1) * dr[None]
    Hx[P:2 * P, 0] = B[:, 2].transpose(2, 0, 1) * dv[:, None, None]
    Hx[P:2 * P, 1] = B[:, 3].transpose(2, 0, 1) * dv[:, None, None] * dr[None]
    for k in range(K):
        o = 2 * P + 3 * k
        Hx[o, 0, :, k] = -Et[k]
        Hx[o + 1, 0, :, k] = d[:, k] * ta[k]
        Hx[o + 2, 0, :, k] = d[:, k] * tb[k]
        Hx[o + 1, 1, :, k] = 0.5 * ta[k] * dr[:, k]
        Hx[o + 2, 1, :, k] = 0.5 * tb[k] * dr[:, k]
    out['Hx'] = Hx.reshape(R, 2 * GK)
    return out


def split_influence_operand(A, P, K, G):
    """The operand A (Q x (2 P + 2 G K), columns [A_m | A_v | A_e (G K, group-major) | A_r (G K)]) of the influence entries in
    their two layouts (include/lrvb_hip.h): A_global (Q x 2 P) and A_local (G x 2 K x Q: group g holds the Q-vectors of
    [e_g0 .. e_g,K-1 | r_g0 .. r_g,K-1])."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    Q, GK = A.shape[0], G * K
    if A.ndim != 2 or A.shape[1] != 2 * P + 2 * GK:
        raise ValueError('A must have {} columns [A_m | A_v | A_e | A_r]'.format(2 * P + 2 * GK))
    Al = A[:, 2 * P:].reshape(Q, 2, G, K).transpose(2, 1, 3, 0)            # [g, e or r, k, q]: one pass over the operand
    return np.ascontiguousarray(A[:, :2 * P]), np.ascontiguousarray(Al).reshape(G, 2 * K, Q)


class _LogisticMixedModel(DeviceModel):
    """What the logistic mixed models share -- everything but the parameter layout and the device entries, for K effects per
    group.  A model gives `_layout` and the four device hooks `_terms`, `_schur`, `_obs_influence` and `_group_influence`, which
    speak the K-generic layouts of include/lrvb_hip.h (group sums G x ncol, closed-form entries G x 2 K x 3, e and r as G x K);
    `_solve_on_device` where it has a device-resident block-arrow solve."""
    _stats_at_point = True
    _loss = 'logistic'                               # the loss the device context is created with
    _minus_y = True                                  # `cross_hessian` subtracts y from `_row_psi_derivs`' first value (False: a1' comes whole)

    def __init__(self, par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device):
        """z: the N x K group design, or None for one effect per group with the unit design (nothing is sent to the device).
        gh_deg=None: a likelihood whose psi is closed-form builds no Gauss-Hermite nodes."""
        self.par = par
        x = _hip.as_f64(x)
        self.n_obs, self.P = x.shape
        if z is not None:
            z = _hip.as_f64(z)
            if z.ndim != 2 or z.shape[0] != self.n_obs or not 1 <= z.shape[1] <= 4:
                raise ValueError('z must be N x K with 1 <= K <= 4')
        self.K = 1 if z is None else z.shape[1]
        self.G = int(n_groups)
        self._names = tuple(names)
        self._index(par, names)
        self.gh_x, self.gh_w = (None, None) if gh_deg is None else np.polynomial.hermite.hermgauss(int(gh_deg))
        self._declare_hyper('beta_prior_info', HyperVectorParam('beta_prior_info', 1, lb=0.0, val=np.array([float(beta_prior_info)])))
        self._declare_hyper('mu_prior', HyperVectorParam('mu_prior', 2, val=np.array(list(map(float, mu_prior)))))
        self._declare_effect_prior(tau_prior)
        self.ctx = DeviceContext(par.layout_blocks(), loss=self._loss, n_obs=self.n_obs, n_cols=self.P, device=device)
        self.ctx.set_data(_hip.SLOT_X, x)
        self._y = _hip.as_f64(y).ravel().copy()
        self.ctx.set_data(_hip.SLOT_Y, self._y)
        self._groups = np.ascontiguousarray(np.asarray(groups).ravel(), dtype=np.int32)
        self.ctx.set_groups(self._groups, self.G)
        if z is not None:
            self.ctx.set_group_design(z)
        self._declare_weights(self.n_obs, weights)
        self._x, self._z = x, z
        self._dev_factor_key = None                  # what the factors of solve(on_device=True) were built at
        self._gcov = None                            # (that key, cov_beta) while the group covariance of `group_cov` is resident
        self._push_state()                           # the initial weights on the device: direct calls on `ctx` see them from the start

    tau_beta = property(lambda self: float(self._hyper_vec('beta_prior_info')[0]))
    mu0 = property(lambda self: float(self._hyper_vec('mu_prior')[0]))
    kappa0 = property(lambda self: float(self._hyper_vec('mu_prior')[1]))
    a0 = property(lambda self: float(self._hyper_vec('tau_prior')[0]))
    b0 = property(lambda self: float(self._hyper_vec('tau_prior')[1]))

    def _declare_effect_prior(self, tau_prior):
        """The hyper-parameter of the prior on the effects' precision: Gamma(a0, b0) on every tau_k."""
        self._declare_hyper('tau_prior', HyperVectorParam('tau_prior', 2, lb=0.0, val=np.array(list(map(float, tau_prior)))))

    def _n_global(self):
        return 2 * self.P + 4 * self.K

    def _split(self, eta):
        """eta as (m, i_beta, e_mu, i_mu, the two pieces of q(precision), e G x K, i G x K)."""
        return _split_eta(eta, self.P, self.K, self.G)

    def _index(self, par, names):
        """The layout must be the canonical one, in vector and in free coordinates, every coordinate packed element-wise
        (identity, or lb + exp).  `_layout` gives it: the (parameter, field, first, last coordinate) of every block, the message
        for a layout that differs, and the message for a parameter that holds more than these blocks."""
        self.n_global = ng = self._n_global()
        D = ng + 2 * self.G * self.K
        vi, fi = par.vector_indices_dict, par.free_indices_dict
        want, msg, msg_more = self._layout(par, names)
        for name, field, lo, hi in want:
            sub = par[name]
            for top, inner in ((vi, sub.vector_indices_dict), (fi, sub.free_indices_dict)):
                if top[name].start + inner[field].start != lo or top[name].start + inner[field].stop != hi:
                    raise ValueError(msg)
        if par.vector_size() != D or par.free_size() != D:
            raise ValueError(msg_more)
        self._index_packing(par)

    def _index_packing(self, par):
        lb = []
        for blk in par.layout_blocks():
            if blk['kind'] != _hip.BLOCK_BOX or np.isfinite(blk['ub']) or blk['free_size'] != blk['vec_size']:
                raise ValueError('every coordinate must be unconstrained or bounded below only')
            lb.extend([blk['lb']] * blk['vec_size'])
        self._lb = np.asarray(lb, dtype=np.float64)
        self._bounded = np.isfinite(self._lb)

    # ---- the point --------------------------------------------------------------------------------------------------
    def _eta(self, x, is_free):
        """Vector coordinates of x; `par` holds the evaluation point afterwards (the side-effect contract of the functors)."""
        x = _hip.as_f64(x).ravel()
        if is_free:
            self.par.set_free(x)
            return np.asarray(self.par.get_vector(), dtype=np.float64).ravel()
        self.par.set_vector(x)
        return x

    def _jac(self, eta):
        """Element-wise packing: d eta / d theta and d2 eta / d theta2."""
        j1 = np.where(self._bounded, eta - np.where(self._bounded, self._lb, 0.0), 1.0)
        return j1, np.where(self._bounded, j1, 0.0)

    def _global_jac_T(self, C, eta):
        """J_g^T C for the n_global leading rows C of a gradient or a cross Hessian (J_g = d eta_global / d theta_global)."""
        jg = self._jac(eta)[0][:self.n_global]
        return C * (jg if np.ndim(C) == 1 else jg[:, None])

    def _grad_to_free(self, g, eta):
        ng = self.n_global
        return np.concatenate([self._global_jac_T(g[:ng], eta), g[ng:] * self._jac(eta)[0][ng:]])

    def _arrow_to_free(self, cf, eta):
        """(grad, Hgg, rows, Hx, loc) of the closed forms `cf` in free coordinates."""
        j1, j2 = self._jac(eta)
        return block_arrow_to_free(cf, j1, j2, self.n_global, self.G, self.K)

    # ---- data pieces (GPU) ------------------------------------------------------------------------------------------
    def _pieces_of(self, val, gg, Hb, gs):
        if gs is None:
            return dict(value=val, g_glob=None)
        gl, loc, border = unpack_group_sums(gs, self.P, self.K)
        return dict(value=val, g_glob=gg, g_loc=gl, Hb=Hb, loc=loc, border=border)

    def _point(self, eta):
        """The arguments of the terms entry at eta, the weights pushed: (m, v, e, r: G x K, nodes, weights)."""
        _, ib, _, _, _, _, e, ig = self._split(eta)
        self._push_state()
        self._dev_factor_key = None                  # the terms entry drops the factor on the device
        return eta[:self.P], 1.0 / ib, e, 1.0 / ig, self.gh_x, self.gh_w

    def _group_sums(self, eta, want_grad=True, want_hess=True, want_border=True):
        """(value, global gradient, H blocks, group sums G x ncol) of this process's rows, as the terms entry gives them."""
        return self._terms(*self._point(eta), want_grad=want_grad or want_hess, want_hess=want_hess, want_border=want_border)

    def _device_terms(self, eta, want_grad, want_hess, want_border=True):
        return self._pieces_of(*self._group_sums(eta, want_grad, want_hess, want_border))

    def stats_size(self):
        return 1 + 2 * self.P + 3 * self.P ** 2 + self.G * group_sums_ncol(self.P, self.K)[1]

    def local_stats(self, eta):
        """[value | global gradient (2 P) | H blocks (3 P^2) | group sums (G x ncol)] of THIS process's rows in the coordinates
        (m, v, e, r) at the vector-coordinate point eta: the buffer of one host-side sum over shards (a group may straddle
        shards: its sums add).  With a reduce hook on the context it is already the sum over the ranks."""
        val, gg, Hb, gs = self._group_sums(_hip.as_f64(eta).ravel())
        return np.concatenate([[val], gg, Hb.ravel(), gs.ravel()])

    def set_reduced_stats(self, flat, eta=None):
        """Install statistics summed over all shards for the point eta (None = use this process's own rows again)."""
        self._install_reduced_stats(flat, self.stats_size(), eta)

    def _data(self, eta, want_grad, want_hess, want_border=True):
        f = self._installed_stats(eta)
        if f is None:
            return self._device_terms(eta, want_grad, want_hess, want_border)
        P, G = self.P, self.G
        o = 1 + 2 * P
        return self._pieces_of(float(f[0]), f[1:o], f[o:o + 3 * P * P].reshape(3, P, P), f[o + 3 * P * P:].reshape(G, -1))

    def _closed(self, eta, want_grad=True, want_hess=True, want_border=True):
        d = self._data(eta, want_grad, want_hess, want_border)
        if not (want_grad or want_hess):
            d = dict(value=d['value'])
        return glmm_slopes_closed_forms(self.P, self.K, self.G, eta, d, self.tau_beta, self.mu0, self.kappa0, self.a0, self.b0,
                                        want_hess=want_hess)

    def _arrow(self, x, is_free):
        """(grad, Hgg, rows, Hx, loc) at x in its own coordinates, cached per point and `_data_key`."""
        eta = self._eta(x, is_free)                  # on a hit too: `par` holds the point afterwards

        def make():
            cf = self._closed(eta)
            return self._arrow_to_free(cf, eta) if is_free else (cf['grad'], cf['Hgg'], cf['rows'], cf['Hx'], cf['loc'])
        self._pieces = self._at_point('arrow', x, is_free, make)
        return self._pieces

    # ---- functor protocol -------------------------------------------------------------------------------------------
    @_hip.host_blas
    def value(self, x, is_free=True):
        return self._closed(self._eta(x, is_free), False, False)['value']

    @_hip.host_blas
    def grad(self, x, is_free=True):
        eta = self._eta(x, is_free)
        g = self._closed(eta, True, False)['grad']
        return self._grad_to_free(g, eta) if is_free else g

    jacobian = grad

    @_hip.host_blas
    def hessian(self, x, is_free=True):
        if self.par.vector_size() > 8192:
            raise MemoryError('dense Hessian of {} parameters: use global_hessian() (Schur complement) or hvp()'.format(self.par.vector_size()))
        return block_arrow_dense(*self._arrow(x, is_free)[1:])

    @_hip.host_blas
    def hvp(self, x, v, is_free=True):
        return block_arrow_matvec(*self._arrow(x, is_free)[1:], v)

    @_hip.host_blas
    def sparse_hessian(self, free_val):
        """The free-coordinate Hessian as a scipy CSR block arrow: global block, border and 2 K x 2 K local blocks."""
        return block_arrow_sparse(*self._arrow(free_val, True)[1:])

    # ---- Schur complement onto the global block -----------------------------------------------------------------------
    def _ensure_gctx(self):
        if not hasattr(self, '_gctx'):
            blocks, size = [], 0
            for b in self.par.layout_blocks():
                if size >= self.n_global:
                    break
                blocks.append(b)
                size += b['vec_size']
            assert size == self.n_global
            self._gctx = DeviceContext(blocks, quad_kind=_hip.QUAD_DIAG, device=self.ctx.device)
        return self._gctx

    @_hip.host_blas
    def global_hessian(self, free_val, want_host=True):
        """H_S = H_gg - H_gl H_ll^-1 H_lg in FREE coordinates (n_global x n_global): its inverse is the linear-response
        covariance of the global parameters.  Device route: the border formed by the terms entry stays on the GPU and the Schur
        entry (lrvb_glmm_slopes_schur, lrvb_glmm_schur) eliminates the 2 G K local parameters there; the host adds the
        N-independent terms to the G local blocks (free coordinates) and sends their upper triangles with the chain factors and
        the closed-form border entries.  The result stays resident on the global context for `chol_factor_last`."""
        fv = _hip.as_f64(free_val).ravel()
        P, K, G, ng = self.P, self.K, self.G, self.n_global
        self._push_state()
        self._dev_factor_key = None
        eta = self._eta(fv, True)
        j1, j2 = self._jac(eta)
        cf = self._closed(eta, want_border=False)    # the group sums of the point stay resident; the border is not copied back
        g, Hgg, rows = cf['grad'], cf['Hgg'].copy(), cf['rows']
        loc_f = block_arrow_to_free(cf, j1, j2, ng, G, K)[4]
        if self._external_stats is None:
            _, ib, e_mu, _, a, b, e, ig = self._split(eta)
            r = 1.0 / ig
            d = e - e_mu[None, :]
            ta, tb = 1.0 / b, -a / b ** 2
            closed = np.zeros((G, 2 * K, 3))
            closed[:, :K, 0], closed[:, :K, 1], closed[:, :K, 2] = -(a / b)[None, :], d * ta[None, :], d * tb[None, :]
            closed[:, K:, 1], closed[:, K:, 2] = 0.5 * ta[None, :], 0.5 * tb[None, :]
            jl = _to_groups(j1[ng:], G, K)[:, :, 0]
            scale = np.concatenate([jl[:, :K], -r * r * jl[:, K:]], axis=1)
            iu = np.triu_indices(2 * K)
            M = self._schur(loc_f[:, iu[0], iu[1]], scale, closed)                    # coordinates [m | v | e_mu_k, a_k, b_k]
            dv = np.concatenate([np.ones(P), -1.0 / ib ** 2, np.ones(3 * K)])
            M = M * dv[:, None] * dv[None, :]
        else:
            M = block_arrow_schur_term(rows, cf['Hx'] * j1[ng:][None, :], loc_f)
        Hgg[np.ix_(rows, rows)] -= M
        gc = self._ensure_gctx()
        gc.hvec_begin()
        gc.hvec_add_block(Hgg, 0, 0)
        out = gc.hvec_finish(fv[:ng], g[:ng], True, want_host=want_host)
        self._schur_key = self._resident_key(fv)
        return out

    def _resident_key(self, fv):
        """What the Schur complement resident on the global context was built at: the point and `_data_key`."""
        return (np.asarray(fv, dtype=np.float64).tobytes(), self._data_key())

    # ---- the whole arrow: solve, covariance of any moment, weight influence --------------------------------------------------
    def _solve_on_device(self, x, R, is_free):
        raise ValueError('on_device=True: this model has no block-arrow solve resident on the device')

    @_hip.host_blas
    def solve(self, x, R, is_free=True, resident_factor=False, on_device=False):
        """H^-1 R at x (R: D x Q or a D-vector, local rows allowed) by `block_arrow_solve`.  resident_factor=True solves the
        Schur complement with the factor on the global context: call `global_hessian(x, want_host=False)` and
        `_ensure_gctx().chol_factor_last()` at the same point first (free coordinates); a factor built at another point, or
        under other weights or hyper-parameters, is refused with a ValueError.
        on_device=True (the models with K effects per group, `_SlopesArrow`; free coordinates, this process's own rows): the local blocks and the border stay
        on the device (`block_arrow_solve_by_phases` around lrvb_glmm_slopes_solve_forward / _back); the
        factors are built here when they are not those of this point and reused otherwise."""
        if on_device:
            return self._solve_on_device(x, R, is_free)
        _, Hgg, rows, Hx, loc = self._arrow(x, is_free)
        if resident_factor and (not is_free or getattr(self, '_schur_key', None) != self._resident_key(_hip.as_f64(x).ravel())):
            raise ValueError('resident_factor=True needs global_hessian(x, want_host=False) and chol_factor_last() at this point, '
                             'with these weights and hyper-parameters, in free coordinates')
        schur_solve = self._ensure_gctx().chol_solve if resident_factor else None
        return block_arrow_solve(Hgg, rows, Hx, loc, R, schur_solve=schur_solve)

    def _moment_jac(self, moment_jac):
        M = np.atleast_2d(_hip.as_f64(moment_jac))
        D = self.n_global + 2 * self.G * self.K
        if M.ndim != 2 or M.shape[1] not in (D, self.n_global):
            raise ValueError('moment Jacobian must have {} (all parameters) or {} (global parameters) columns'.format(D, self.n_global))
        if M.shape[1] != D:
            M = np.hstack([M, np.zeros((M.shape[0], D - M.shape[1]))])
        return M

    def lrvb_cov(self, x, moment_jac, is_free=True, on_device=False):
        """M H^-1 M^T (Q x Q): the linear-response covariance of the moments M theta, M = moment_jac being Q x D (columns of the
        group effects allowed) or Q x n_global (zero-padded).  on_device: as `solve`."""
        M = self._moment_jac(moment_jac)
        return M @ self.solve(x, np.ascontiguousarray(M.T), is_free, on_device=on_device)

    def _influence_operand(self, x, moment_jac, is_free, chol, on_device=False):
        """A = -M H^-1 J (Q x (2 P + 2 G K)) in the coordinates (m, v, e, r) of the device entries -- the element-wise chain from
        eta's (m, i_beta, e, i), the columns of mu and tau dropped -- and the point in those coordinates."""
        self._push_state()
        M = self._moment_jac(moment_jac)
        P, K, G, ng = self.P, self.K, self.G, self.n_global
        GK = G * K
        if on_device and chol is not None:
            raise ValueError('on_device=True does not use a dense factor: pass one of the two')
        if chol is None:
            S = self.solve(x, np.ascontiguousarray(M.T), is_free, on_device=on_device)
        else:
            S = np.asarray(chol.solve(np.ascontiguousarray(M.T))).reshape(ng + 2 * GK, -1)
        eta = self._eta(x, is_free)
        j1 = self._jac(eta)[0] if is_free else np.ones(eta.size)
        _, ib, _, _, _, _, e, ig = self._split(eta)
        v, r = 1.0 / ib, 1.0 / ig
        chain = np.concatenate([j1[:P], -v * v * j1[P:2 * P], j1[ng:ng + GK], -(r * r).ravel() * j1[ng + GK:]])
        keep = np.concatenate([np.arange(2 * P), np.arange(ng, ng + 2 * GK)])
        A = -(S[keep] * chain[:, None]).T
        return np.ascontiguousarray(A), (eta[:P], v, e, r, self.gh_x, self.gh_w)

    def obs_influence(self, x, moment_jac, n0=0, n1=None, is_free=True, chol=None, on_device=False):
        """Rows n0..n1 of (moment_jac @ d par / d w)^T ((n1 - n0) x Q), streamed over the observations on the device
        (lrvb_glmm_slopes_obs_influence, lrvb_glmm_obs_influence); the N x D cross Hessian is never formed.  A = -moment_jac H^-1 J
        comes from the dense factor `chol` where one is given (ParametricSensitivityLinearApproximation holds it), otherwise from
        `block_arrow_solve` -- the route for large G, where no dense factor exists; with on_device=True from the device-resident
        solve (`solve`), so that no N- or G-sized host arithmetic lies between the fit and the streamed rows.  Per unit weight: a
        row of weight zero gets the influence of adding it."""
        A, pt = self._influence_operand(x, moment_jac, is_free, chol, on_device)
        return self._obs_influence(*pt, A, n0=n0, n1=n1)

    def group_influence(self, x, moment_jac, is_free=True, chol=None, on_device=False):
        """G x Q: row g is the derivative of the moments with respect to a common multiplier on the weights of group g's rows,
        sum_{n in g} w_n * (row n of `obs_influence`) -- minus it is the linear prediction of leaving the cluster out.  The
        group's own prior terms on u_g stay in the model and are not part of it.  Fixed summation order on the device
        (lrvb_glmm_slopes_group_influence, lrvb_glmm_group_influence); an empty group gives a zero row.  on_device: as
        `obs_influence`."""
        A, pt = self._influence_operand(x, moment_jac, is_free, chol, on_device)
        return self._group_influence(*pt, A)

    # ---- hyper-parameters ---------------------------------------------------------------------------------------------
    def _prior_hyper(self, kind, eta_g, want):
        P, K, ng = self.P, self.K, self.n_global
        m, ib = eta_g[:P], eta_g[P:2 * P]
        e_mu, i_mu = eta_g[2 * P:2 * P + K], eta_g[2 * P + K:2 * P + 2 * K]
        if kind == 'beta_prior_info':
            if want == 'grad':
                return np.array([0.5 * (np.sum(m * m) + np.sum(1.0 / ib))])
            C = np.zeros((ng, 1))
            C[:P, 0], C[P:2 * P, 0] = m, -0.5 / ib ** 2
            return C
        if kind == 'mu_prior':
            if want == 'grad':
                return np.array([-self.kappa0 * np.sum(e_mu - self.mu0), 0.5 * np.sum((e_mu - self.mu0) ** 2 + 1.0 / i_mu)])
            C = np.zeros((ng, 2))
            C[2 * P:2 * P + K, 0], C[2 * P:2 * P + K, 1] = -self.kappa0, e_mu - self.mu0
            C[2 * P + K:2 * P + 2 * K, 1] = -0.5 / i_mu ** 2
            return C
        if kind != 'tau_prior':
            raise NotImplementedError(kind)
        out = np.zeros(2) if want == 'grad' else np.zeros((ng, 2))
        for k in range(K):
            ia = 2 * P + 2 * K + 2 * k
            a, b = eta_g[ia], eta_g[ia + 1]
            out = out + (gamma_prior_hyper_grad(a, b, special) if want == 'grad' else gamma_prior_hyper_cross(ng, ia, ia + 1, a, b, special))
        return out

    def hyper_grad(self, hyper_par, val1, val1_is_free):
        kind = self.hyper_kind(hyper_par)
        if kind == 'weights':
            raise NotImplementedError('d f / d weights is not declared')
        return self._prior_hyper(kind, self._eta(val1, val1_is_free)[:self.n_global], 'grad')

    def global_cross_hessian(self, hyper_par, val, is_free=True):
        """The n_global rows of the cross Hessian with a PRIOR hyper-parameter (its 2 G K local rows are zero)."""
        kind = self.hyper_kind(hyper_par)
        if kind == 'weights':
            raise NotImplementedError('the weight cross Hessian has local rows: use cross_hessian')
        eta = self._eta(val, is_free)
        C = self._prior_hyper(kind, eta[:self.n_global], 'cross')
        return self._global_jac_T(C, eta) if is_free else C

    @_hip.host_blas
    def cross_hessian(self, hyper_par, val1, val1_is_free):
        """d2 f / d par d hyper^T, all rows (dense protocol: small N and G).  Weights: column n is the gradient of row n's term
        per unit weight, [(psi_rho - y) x_n | psi_s x_n o x_n chained to i_beta | 0 | at g(n): (psi_rho - y) z_n, psi_s z_n o z_n
        chained to i_g.] -- its local rows are NOT zero.  Priors: the local rows are zero."""
        kind = self.hyper_kind(hyper_par)
        val1 = _hip.as_f64(val1).ravel()
        if kind != 'weights':
            Cg = self.global_cross_hessian(hyper_par, val1, is_free=val1_is_free)
            return np.vstack([Cg, np.zeros((val1.size - self.n_global, Cg.shape[1]))])
        eta = self._eta(val1, val1_is_free)
        P, K, G, ng, N = self.P, self.K, self.G, self.n_global, self.n_obs
        GK = G * K
        x, gid = self._x, self._groups
        z = np.ones((N, 1)) if self._z is None else self._z
        _, ib, _, _, _, _, e, ig = self._split(eta)
        v, r = 1.0 / ib, 1.0 / ig
        rho = x @ eta[:P] + np.sum(z * e[gid], axis=1)
        s = (x * x) @ v + np.sum(z * z * r[gid], axis=1)
        p_rho, p_s = self._row_psi_derivs(rho, s)
        if self._minus_y:
            p_rho = p_rho - self._y
        C = np.zeros((N, ng + 2 * GK))
        C[:, :P] = p_rho[:, None] * x
        C[:, P:2 * P] = p_s[:, None] * (x * x) * (-v * v)[None, :]
        n = np.arange(N)[:, None]
        cols = gid[:, None] * K + np.arange(K)[None, :]
        C[n, ng + cols] = p_rho[:, None] * z
        C[n, ng + GK + cols] = p_s[:, None] * z * z * (-r * r)[gid]
        if val1_is_free:
            C = C * self._jac(eta)[0][None, :]
        return np.ascontiguousarray(C.T)

    def _row_psi_derivs(self, rho, s):
        """(psi_rho, psi_s) of every row, on the host path of the dense weight cross Hessian."""
        sd = np.sqrt(s)
        _, d1, _ = self.ctx.gh_logistic(rho, sd, self.gh_x, self.gh_w, order=2)
        return d1[:, 0], 0.5 * d1[:, 1] / sd                  # s_n > 0 wherever a row has a non-zero x or z

    def global_sensitivity(self, hyper_par, free_val):
        """d theta_global / d hyper^T = -H_S^-1 C_g (n_global x Ph) for a prior hyper-parameter: its cross Hessian has no local
        rows, so the local parameters enter through the Schur complement only."""
        Cg = self.global_cross_hessian(hyper_par, free_val)
        gc = self._ensure_gctx()
        self.global_hessian(free_val, want_host=False)
        gc.chol_factor_last()
        return -gc.chol_solve(Cg)


class _SlopesArrow:
    """What the models with K effects per group share on top of `_LogisticMixedModel`, whatever their likelihood: the parameter
    layout of DESIGN.md section 18, the Schur entry on the resident group sums and the block-arrow solve resident on the device
    (`LogisticGLMMSlopesObjective`, `PoissonGLMMObjective`, `BinomialGLMMObjective` and its negative-binomial subclass)."""

    def _layout(self, par, names):
        P, K, G = self.P, self.K, self.G
        ng, GK = 2 * P + 4 * K, G * K
        want = [(names[0], 'mean', 0, P), (names[0], 'info', P, 2 * P), (names[1], 'mean', 2 * P, 2 * P + K),
                (names[1], 'info', 2 * P + K, 2 * P + 2 * K)]
        for k in range(K):
            o = 2 * P + 2 * K + 2 * k
            want += [(names[2] + str(k), 'shape', o, o + 1), (names[2] + str(k), 'rate', o + 1, o + 2)]
        want += [(names[3], 'mean', ng, ng + GK), (names[3], 'info', ng + GK, ng + 2 * GK)]
        msg = ('the parameter must be [UVNParamVector {} ({}) | UVNParamVector {} ({}) | GammaParam {}0 .. {}{} | UVNParamArray {} ({}, {})] '
               'in this order, the group effects pushed last'.format(names[0], P, names[1], K, names[2], names[2], K - 1, names[3], G, K))
        if any(name not in par.vector_indices_dict for name, _, _, _ in want):
            raise ValueError(msg)
        return want, msg, 'the parameter holds more than the blocks of the model'

    def _schur(self, local_blocks, border_scale, closed_rows):
        return self.ctx.glmm_slopes_schur(local_blocks, border_scale, closed_rows)

    # ---- the coupled layout of the device factor: what `_CorrelatedArrow` (glmm_corr.py) replaces -------------------------------
    def _coupled_rows(self):
        return coupled_rows(self.P, self.K)

    def _coupled_scaling(self, eta):
        """s: the border in free coordinates is Hx[r, l] = s_r C_g[l, r] for the device's C_g."""
        dv = np.concatenate([np.ones(self.P), -1.0 / eta[self.P:2 * self.P] ** 2, np.ones(3 * self.K)])
        return self._jac(eta)[0][self._coupled_rows()] * dv

    def _solve_entries(self):
        """(forward, back) of `block_arrow_solve_by_phases` on the resident factor."""
        return self.ctx.glmm_slopes_solve_forward, lambda xc: self.ctx.glmm_slopes_solve_back(xc, self.G, self.K)

    def _group_cov_phases(self, s):
        """`block_arrow_group_cov_by_phases` on the resident factor: (cov_beta, the (G + 1)-row buffer)."""
        P, K, G = self.P, self.K, self.G
        return block_arrow_group_cov_by_phases(self.n_global, self._coupled_rows(), P, K, s, self._ensure_gctx().chol_solve,
                                               lambda W, sc: self.ctx.glmm_slopes_group_cov(W, sc, G, K))

    def _host_group_cov(self, x):
        _, Hgg, rows, Hx, loc = self._arrow(x, True)
        return block_arrow_group_cov(Hgg, rows, Hx, loc, self.P, self.K, population=True)

    # ---- the block-arrow solve resident on the device ------------------------------------------------------------------------
    def _device_factors(self, x, is_free):
        """on_device=True: the Schur factor on the global context and the local factor (L_g, U_g) on `ctx` at the free point x,
        built here (`global_hessian(x, want_host=False)`, `chol_factor_last()`: the border never reaches the host) unless both
        are those of this point, weights and hyper-parameters.  Returns the scaling s of the coupled rows: the border in free
        coordinates is Hx[r, l] = s_r C_g[l, r] for the device's C_g."""
        if not is_free:
            raise ValueError('on_device=True solves in free coordinates')
        if self._external_stats is not None:
            raise ValueError('on_device=True uses the group sums resident on this device, not installed statistics')
        fv = _hip.as_f64(x).ravel()
        self._push_state()
        key = self._resident_key(fv)
        if getattr(self, '_schur_key', None) != key or self._dev_factor_key != key:
            self.global_hessian(fv, want_host=False)
            self._ensure_gctx().chol_factor_last()
            self._dev_factor_key = key
            self._gcov = None                        # the group covariance went with the old factor
        return self._coupled_scaling(self._eta(fv, True))

    def _solve_on_device(self, x, R, is_free):
        s = self._device_factors(x, is_free)
        D = self.n_global + 2 * self.G * self.K
        if np.shape(R)[0] != D:
            raise ValueError('R must have {} rows'.format(D))
        forward, back = self._solve_entries()
        return block_arrow_solve_by_phases(R, self.n_global, self._coupled_rows(), s, forward, self._ensure_gctx().chol_solve, back)


    # ---- group blocks of H^-1, fitted values and predictions --------------------------------------------
    def _group_cov(self, x, is_free, on_device):
        """(cov_beta, cov_u (G + 1) x K x K, cov_beta_u (G + 1) x P x K), the pseudo-group of a population-level row last.  With
        on_device the buffer stays resident on `ctx` for the predict entry and only cov_beta is kept here."""
        if not is_free:
            raise ValueError('the linear-response covariance of the means is taken in free coordinates')
        P, K, G = self.P, self.K, self.G
        if not on_device:
            return self._host_group_cov(x)
        s = self._device_factors(x, True)
        key = self._dev_factor_key
        if self._gcov is not None and self._gcov[0] == key:
            return self._gcov[1], None, None
        self._gcov = None
        cov_beta, buf = self._group_cov_phases(s)
        self._gcov = (key, cov_beta)
        return (cov_beta,) + unpack_group_cov(buf, P, K)

    @_hip.host_blas
    def group_cov(self, x, is_free=True, on_device=False):
        """(cov_beta P x P, cov_u G x K x K, cov_beta_u G x P x K): the linear-response covariance of the means of beta, of every
        group's effects, and between the two -- the blocks of H^-1 in free coordinates, in which E beta = m and E u_gk = e_gk
        are coordinates themselves (lme4's `condVar` is cov_u).  Host route: `block_arrow_group_cov`.  on_device=True: one more
        pass over the factor `solve(on_device=True)` leaves resident (lrvb_glmm_slopes_group_cov); a factor already at this
        point is reused, but the blocks themselves are formed again on every call (the `chol_solve` of R columns, the upload, the
        kernel and the copy of G + 1 rows: the host copy is not kept; `predict` does keep the resident buffer of a cached point);
        vector coordinates and installed statistics are refused, as there."""
        if on_device and self._gcov is not None:
            self._gcov = None                        # the caller asks for the blocks themselves: form them again
        cb, cu, cbu = self._group_cov(x, is_free, on_device)
        return cb, cu[:self.G], cbu[:self.G]

    def ranef_se(self, x, is_free=True, on_device=False):
        """(linear-response, mean-field) standard errors of the group effects, G x K each: sqrt diag Sigma_uu next to 1 / sqrt i."""
        cu = self.group_cov(x, is_free, on_device)[1]
        eta = self._eta(x, is_free)
        ig = self._split(eta)[7]
        return np.sqrt(np.diagonal(cu, axis1=1, axis2=2)), 1.0 / np.sqrt(ig)

    def _predict_rows_of(self, newdata, n0, n1):
        """(x, z, groups with -1 -> G, offset, trials) of the rows to predict; newdata=None: the window of the model's own rows."""
        G, N = self.G, self.n_obs
        if newdata is None:
            n0 = int(n0)
            n1 = N if n1 is None else int(n1)
            if n0 < 0 or n1 > N or n0 > n1:
                raise ValueError('row range [{}, {}) outside [0, {})'.format(n0, n1, N))
            sl = slice(n0, n1)
            off, tr = self._predict_offset(), getattr(self, '_trials', None)
            return self._x[sl], self._z[sl], self._groups[sl], None if off is None else off[sl], None if tr is None else tr[sl]
        unknown = set(newdata) - {'x', 'z', 'groups', 'offset', 'trials'}
        if unknown:
            raise ValueError('newdata has the keys x, z, groups, offset, trials (got {})'.format(sorted(unknown)))
        x = _hip.as_f64(newdata['x'])
        n = x.shape[0]
        z = np.ones((n, 1)) if newdata.get('z') is None else _hip.as_f64(newdata['z'])
        gid = np.asarray(newdata['groups']).ravel()
        if x.ndim != 2 or x.shape[1] != self.P or z.shape != (n, self.K) or gid.size != n:
            raise ValueError('newdata: x must be n x {}, z n x {} and groups of length n'.format(self.P, self.K))
        if np.any(gid != np.round(gid)) or np.any(gid < -1) or np.any(gid >= G):
            raise ValueError('newdata: groups must lie in [0, {}) or be -1 (population level)'.format(G))
        gid = np.where(gid < 0, G, gid).astype(np.int32)
        extra = []
        for name in ('offset', 'trials'):
            a = newdata.get(name)
            if a is not None:
                a = _hip.as_f64(a).ravel()
                if a.size != n or not np.all(np.isfinite(a)):
                    raise ValueError('newdata: {} must hold {} finite values'.format(name, n))
            extra.append(a)
        return x, z, gid, extra[0], extra[1]

    def _predict_offset(self):
        return getattr(self, '_offset', None)

    @_hip.host_blas
    def predict(self, x, newdata=None, n0=0, n1=None, is_free=True, on_device=False):
        """Fitted values (newdata=None: rows n0..n1 of the model's data) or predictions for new rows
        `newdata = dict(x=, z=, groups=, offset=, trials=)`, as a dict of five arrays of one value per row:

            rho        o + x . m + z . e_g             the linear predictor at the variational means
            var_mf     (x o x) . v + (z o z) . r_g     its mean-field variance
            var_lrvb   c^T H^-1 c, c = (x at m, z at e_g): its linear-response variance (the N x D matrix of the c is never formed)
            mean_mf, mean_lrvb   the response-scale mean E g(t), t ~ N(rho, var), under either variance

        groups may hold -1: the row is predicted at the population level, as if its effect u equalled mu (e_mu, 1 / i_mu and
        the blocks of mu in H^-1 stand in for the group's); any other value outside [0, G) is a ValueError.  This is not the
        predictive distribution of a new group, which would add 1 / tau.  on_device=True: the group blocks stay on the device
        (`group_cov`) and the rows are streamed there (lrvb_glmm_slopes_predict and its siblings); free coordinates only."""
        rows = self._predict_rows_of(newdata, n0, n1)
        cb, cu, cbu = self._group_cov(x, is_free, on_device)
        eta = self._eta(x, True)
        P, K, G = self.P, self.K, self.G
        m, ib, e_mu, i_mu, _, _, e, ig = self._split(eta)
        v, e2, r2 = 1.0 / ib, np.vstack([e, e_mu[None, :]]), np.vstack([1.0 / ig, 1.0 / i_mu[None, :]])
        if on_device:
            out = self._predict_entry((m, v, e2, r2, self.gh_x, self.gh_w), cb, None if newdata is not None else (int(n0), n1), rows)
        else:
            rho, s_mf, v_lr = predict_rows(rows[0], rows[1], rows[2], rows[3], m, v, e2, r2, cb, cu, cbu)
            out = rho, s_mf, v_lr, self._response_mean(rho, s_mf, rows[4]), self._response_mean(rho, v_lr, rows[4])
        return dict(zip(('rho', 'var_mf', 'var_lrvb', 'mean_mf', 'mean_lrvb'), out))

    def _response_mean(self, rho, s, trials):
        """E sigma(t), t ~ N(rho, s), by the Gauss-Hermite rule of the kernels; times the trials where the model has them."""
        from scipy.special import expit
        t = rho[:, None] + np.sqrt(np.maximum(s, 0.0))[:, None] * (np.sqrt(2.0) * self.gh_x)[None, :]
        p = (expit(t) * (self.gh_w / np.sqrt(np.pi))[None, :]).sum(1)
        return p if trials is None else trials * p


class LogisticGLMMSlopesObjective(_SlopesArrow, _LogisticMixedModel):
    def __init__(self, par, x, y, z, groups, n_groups, beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20,
                 names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """names: the parameters of q(beta), q(mu), q(tau_k) -- named names[2] + str(k), k = 0..K-1 -- and q(u)."""
        if z is None:
            raise ValueError('z must be N x K with 1 <= K <= 4')
        super().__init__(par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)

    # ---- the device entries -------------------------------------------------------------------------------------------------
    def _terms(self, *point, **want):
        return self.ctx.glmm_slopes_terms(*point, **want)

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_slopes_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_slopes_group_influence(*point_and_operand)

    def _predict_entry(self, point, cov_beta, window, rows):
        if window is not None:
            return self.ctx.glmm_slopes_predict(*point, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_slopes_predict(*point, cov_beta, new=rows[:3])

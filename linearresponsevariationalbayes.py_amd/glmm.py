"""Logistic mixed model with a random intercept:

    y_n ~ Bernoulli(sigma(x_n . beta + u_{g(n)})),   u_g ~ N(mu, 1 / tau),   n = 1..N,  g = 0..G-1

with q(beta) = UVNParamVector(P), q(mu) = UVNParam, q(tau) = GammaParam, q(u) = UVNParamVector(G), the group effects pushed
last.  Vector coordinates eta = [m (P) | i_beta (P) | e_mu, i_mu | a, b | e (G) | i (G)], n_global = 2 P + 4.

    KL(eta) =  sum_n w_n [ psi(rho_n, s_n) - y_n rho_n ]        rho_n = x_n . m + e_g(n),  s_n = (x_n o x_n) . (1 / i_beta) + 1 / i_g(n)
             + 1/2 E tau ( sum_g [(e_g - e_mu)^2 + 1 / i_g] + G / i_mu ) - 1/2 G E log tau
             + 1/2 tau_beta sum_j (m_j^2 + 1 / i_beta_j)
             + 1/2 kappa0 ((e_mu - mu0)^2 + 1 / i_mu)
             - (a0 - 1) E log tau + b0 E tau
             + 1/2 sum_j log i_beta_j + 1/2 log i_mu + 1/2 sum_g log i_g - gamma_entropy(a, b)

(the Gaussian entropies up to their additive constants, as `LogitNormalRegressionObjective` keeps them).  The O(N) work --
the quadrature per row, the per-group segmented sums of the arrow's border and local blocks, the three weighted products of
the global block -- is `lrvb_glmm_terms` (csrc/k_glmm.hip); everything N-independent is `glmm_closed_forms` below, plain
numpy on the data pieces, so it is testable without a GPU.  The Hessian is an arrow: a dense global block, G local 2 x 2
blocks (NOT diagonal: psi_rho_s couples e_g and i_g) and a border of 2 P + 3 coupled global rows (i_mu does not couple).
"""
import numpy as np
from scipy import special
from scipy import sparse as sp_sparse
from scipy import linalg as sp_linalg

from . import _hip
from .models import DeviceContext, DeclaredHypers, refuse_double_reduction
from .packing import HyperVectorParam, ResidentVector
from .quadform import gamma_prior_hyper_grad, gamma_prior_hyper_cross
from .hierarchical import _gamma_block, _gamma_entropy


def glmm_closed_forms(P, G, eta, data, tau_beta, mu0, kappa0, a0, b0, want_hess=True):
    """The N-independent part of the model, in VECTOR coordinates, from the data-dependent pieces.

    eta: [m | i_beta | e_mu, i_mu | a, b | e | i].  data: dict of the data term in the coordinates (m, v = 1 / i_beta, e,
    r = 1 / i): 'value', 'g_glob' (2 P: d/dm, d/dv), 'g_loc' (G x 2: sum_g a1, sum_g a2), and for the Hessian 'Hb' (3 x P x P:
    mm, mv, vv), 'border' (G x 4 P: sum c11 x | sum c12 x | sum c12 x o x | sum c22 x o x) and 'loc' (G x 3: sum c11, c12, c22).

    Returns dict: 'value', 'grad' (V), and with want_hess 'Hgg' (n_global x n_global), 'rows' (the 2 P + 3 coupled global
    coordinates), 'Hx' ((2 P + 3) x 2 G, columns [e_0..e_G-1 | i_0..i_G-1]) and 'loc' (G x 3: ee, ei, ii of each local block).
    """
    eta = np.asarray(eta, dtype=np.float64)
    ng = 2 * P + 4
    m, ib = eta[:P], eta[P:2 * P]
    e_mu, i_mu, a, b = eta[2 * P], eta[2 * P + 1], eta[2 * P + 2], eta[2 * P + 3]
    e, ig = eta[ng:ng + G], eta[ng + G:]
    v, r = 1.0 / ib, 1.0 / ig
    Et, EL = a / b, special.digamma(a) - np.log(b)
    d = e - e_mu
    Am = np.sum(d * d + r) + G / i_mu
    value = (data['value'] + 0.5 * Et * Am - 0.5 * G * EL + 0.5 * tau_beta * (np.sum(m * m) + np.sum(v))
             + 0.5 * kappa0 * ((e_mu - mu0) ** 2 + 1.0 / i_mu) - (a0 - 1.0) * EL + b0 * Et
             + 0.5 * np.sum(np.log(ib)) + 0.5 * np.log(i_mu) + 0.5 * np.sum(np.log(ig)) - _gamma_entropy(a, b))
    out = dict(value=float(value))
    if data.get('g_glob') is None:
        return out
    gd, gl = np.asarray(data['g_glob']), np.asarray(data['g_loc'])
    dv, dr = -v * v, -r * r                                   # d v / d i_beta, d r / d i
    g_v = gd[P:] + 0.5 * tau_beta
    g_r = gl[:, 1] + 0.5 * Et
    dsum = np.sum(d)
    gab, Hab = _gamma_block(a, b, 0.5 * Am + b0, -0.5 * G - (a0 - 1.0))
    g = np.empty(ng + 2 * G)
    g[:P] = gd[:P] + tau_beta * m
    g[P:2 * P] = g_v * dv + 0.5 / ib
    g[2 * P] = -Et * dsum + kappa0 * (e_mu - mu0)
    g[2 * P + 1] = -0.5 * (Et * G + kappa0) / i_mu ** 2 + 0.5 / i_mu
    g[2 * P + 2:ng] = gab
    g[ng:ng + G] = gl[:, 0] + Et * d
    g[ng + G:] = g_r * dr + 0.5 / ig
    out['grad'] = g
    if not want_hess:
        return out
    Hb, B, L = np.asarray(data['Hb']), data.get('border'), np.asarray(data['loc'])
    ta, tb = 1.0 / b, -a / b ** 2                             # d E tau / d a, d E tau / d b
    Hgg = np.zeros((ng, ng))
    Hgg[:P, :P] = Hb[0] + tau_beta * np.eye(P)
    Hgg[:P, P:2 * P] = Hb[1] * dv[None, :]
    Hgg[P:2 * P, :P] = Hgg[:P, P:2 * P].T
    Hgg[P:2 * P, P:2 * P] = Hb[2] * dv[:, None] * dv[None, :] + np.diag(g_v * 2.0 * v ** 3 - 0.5 / ib ** 2)
    iem, iim, ia, ibb = 2 * P, 2 * P + 1, 2 * P + 2, 2 * P + 3
    Hgg[iem, iem] = Et * G + kappa0
    Hgg[iem, ia] = Hgg[ia, iem] = -dsum * ta
    Hgg[iem, ibb] = Hgg[ibb, iem] = -dsum * tb
    Hgg[iim, iim] = (Et * G + kappa0) / i_mu ** 3 - 0.5 / i_mu ** 2
    Hgg[iim, ia] = Hgg[ia, iim] = -0.5 * G / i_mu ** 2 * ta
    Hgg[iim, ibb] = Hgg[ibb, iim] = -0.5 * G / i_mu ** 2 * tb
    Hgg[ia:ibb + 1, ia:ibb + 1] = Hab
    rows = np.concatenate([np.arange(2 * P), [iem, ia, ibb]])
    loc = np.stack([L[:, 0] + Et, L[:, 1] * dr, L[:, 2] * dr * dr + g_r * 2.0 * r ** 3 - 0.5 / ig ** 2], axis=1)
    out.update(Hgg=Hgg, rows=rows, Hx=None, loc=loc)
    if B is None:                                             # the border stayed on the device (global_hessian)
        return out
    B = np.asarray(B)
    Hx = np.empty((2 * P + 3, 2 * G))
    Hx[:P, :G] = B[:, :P].T
    Hx[:P, G:] = B[:, P:2 * P].T * dr[None, :]
    Hx[P:2 * P, :G] = B[:, 2 * P:3 * P].T * dv[:, None]
    Hx[P:2 * P, G:] = B[:, 3 * P:].T * dv[:, None] * dr[None, :]
    Hx[2 * P, :G] = -Et
    Hx[2 * P, G:] = 0.0
    Hx[2 * P + 1, :G] = d * ta
    Hx[2 * P + 2, :G] = d * tb
    Hx[2 * P + 1, G:] = 0.5 * ta * dr
    Hx[2 * P + 2, G:] = 0.5 * tb * dr
    out['Hx'] = Hx
    return out


def arrow_to_free(cf, j1, j2, n_global, G):
    """The pieces of `glmm_closed_forms` in FREE coordinates for an element-wise packing (j1 = d eta / d theta, j2 = its second
    derivative, both V-vectors): (grad, Hgg, rows, Hx, loc)."""
    g = cf['grad']
    ng = n_global
    jg, je, ji = j1[:ng], j1[ng:ng + G], j1[ng + G:]
    Hgg = cf['Hgg'] * jg[:, None] * jg[None, :] + np.diag(g[:ng] * j2[:ng])
    rows = cf['rows']
    Hx = None if cf['Hx'] is None else cf['Hx'] * jg[rows][:, None] * np.concatenate([je, ji])[None, :]
    L = cf['loc']
    loc = np.stack([L[:, 0] * je * je + g[ng:ng + G] * j2[ng:ng + G], L[:, 1] * je * ji,
                    L[:, 2] * ji * ji + g[ng + G:] * j2[ng + G:]], axis=1)
    return g * j1, Hgg, rows, Hx, loc


def arrow_matvec(Hgg, rows, Hx, loc, v):
    """H v for the arrow (global block, border rows, G local 2 x 2 blocks): O(n_global^2 + P G)."""
    ng, G = Hgg.shape[0], loc.shape[0]
    v = np.asarray(v, dtype=np.float64).ravel()
    vg, ve, vi = v[:ng], v[ng:ng + G], v[ng + G:]
    out = np.empty(ng + 2 * G)
    og = Hgg @ vg
    og[rows] += Hx @ v[ng:]
    out[:ng] = og
    t = Hx.T @ vg[rows]
    out[ng:ng + G] = t[:G] + loc[:, 0] * ve + loc[:, 1] * vi
    out[ng + G:] = t[G:] + loc[:, 1] * ve + loc[:, 2] * vi
    return out


def arrow_dense(Hgg, rows, Hx, loc):
    ng, G = Hgg.shape[0], loc.shape[0]
    V = ng + 2 * G
    H = np.zeros((V, V))
    H[:ng, :ng] = Hgg
    H[rows, ng:] = Hx
    H[ng:, rows] = Hx.T
    ie, ii = np.arange(ng, ng + G), np.arange(ng + G, V)
    H[ie, ie], H[ie, ii], H[ii, ie], H[ii, ii] = loc[:, 0], loc[:, 1], loc[:, 1], loc[:, 2]
    return H


def arrow_schur_term(rows, Hx, loc):
    """M = sum_g C_g A_g^-1 C_g^T on the coupled rows (host route; the device route is lrvb_glmm_schur)."""
    G = loc.shape[0]
    det = loc[:, 0] * loc[:, 2] - loc[:, 1] ** 2
    if not (np.all(loc[:, 0] > 0) and np.all(det > 0)):
        raise np.linalg.LinAlgError('a 2 x 2 local block is not positive definite')
    Ce, Ci = Hx[:, :G], Hx[:, G:]
    return ((Ce * (loc[:, 2] / det)) @ Ce.T + (Ci * (loc[:, 0] / det)) @ Ci.T
            - (Ce * (loc[:, 1] / det)) @ Ci.T - (Ci * (loc[:, 1] / det)) @ Ce.T)


def arrow_local_solve(loc, be, bi):
    """A_g^-1 [be_g; bi_g] for every group."""
    det = loc[:, 0] * loc[:, 2] - loc[:, 1] ** 2
    return (loc[:, 2] * be - loc[:, 1] * bi) / det, (loc[:, 0] * bi - loc[:, 1] * be) / det


def arrow_solve(Hgg, rows, Hx, loc, R, schur_solve=None):
    """H^-1 R for the arrow (R: D x Q or a D-vector, D = n_global + 2 G) without the dense matrix: the G local 2 x 2 blocks are
    solved, the result is reduced onto the coupled global rows, the Schur complement Hgg - `arrow_schur_term` is factored and
    solved, and the local parameters are back-substituted -- O(P G Q + n_global^3).  `schur_solve` (n_global x Q -> n_global x Q)
    replaces the host factorisation of the Schur complement, e.g. by the factor resident on the global context after
    `global_hessian(..., want_host=False)` + `chol_factor_last`.  A local block or a Schur complement that is not positive
    definite raises `np.linalg.LinAlgError`."""
    ng, G = Hgg.shape[0], loc.shape[0]
    R = np.asarray(R, dtype=np.float64)
    vec = R.ndim == 1
    R2 = R.reshape(ng + 2 * G, -1)
    det = loc[:, 0] * loc[:, 2] - loc[:, 1] ** 2
    if not (np.all(loc[:, 0] > 0) and np.all(det > 0)):
        raise np.linalg.LinAlgError('a 2 x 2 local block is not positive definite')
    i11, i12, i22 = (loc[:, 2] / det)[:, None], (-loc[:, 1] / det)[:, None], (loc[:, 0] / det)[:, None]
    Rg, Re, Ri = R2[:ng], R2[ng:ng + G], R2[ng + G:]
    te, ti = i11 * Re + i12 * Ri, i12 * Re + i22 * Ri                    # H_ll^-1 R_l
    rhs = Rg.copy()
    rhs[rows] -= Hx[:, :G] @ te + Hx[:, G:] @ ti
    if schur_solve is None:
        S = Hgg.copy()
        S[np.ix_(rows, rows)] -= arrow_schur_term(rows, Hx, loc)
        L = np.linalg.cholesky(0.5 * (S + S.T))                          # LinAlgError where it is not positive definite
        xg = sp_linalg.cho_solve((L, True), rhs)
    else:
        xg = np.asarray(schur_solve(np.ascontiguousarray(rhs)), dtype=np.float64).reshape(ng, -1)
    ce, ci = Hx[:, :G].T @ xg[rows], Hx[:, G:].T @ xg[rows]              # H_lg x_g
    out = np.vstack([xg, te - (i11 * ce + i12 * ci), ti - (i12 * ce + i22 * ci)])
    return out.ravel() if vec else out


class LogisticGLMMObjective(DeclaredHypers):
    _lrvb_device_functor = True

    def __init__(self, par, x, y, groups, n_groups, beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20,
                 names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        self.par = par
        x = _hip.as_f64(x)
        self.n_obs, self.P = x.shape
        self.G = int(n_groups)
        P, G = self.P, self.G
        self._names = tuple(names)
        self._index(par, names)
        self.gh_x, self.gh_w = np.polynomial.hermite.hermgauss(int(gh_deg))
        self._declare_hyper('beta_prior_info', HyperVectorParam('beta_prior_info', 1, lb=0.0, val=np.array([float(beta_prior_info)])))
        self._declare_hyper('mu_prior', HyperVectorParam('mu_prior', 2, val=np.array(list(map(float, mu_prior)))))
        self._declare_hyper('tau_prior', HyperVectorParam('tau_prior', 2, lb=0.0, val=np.array(list(map(float, tau_prior)))))
        self.ctx = DeviceContext(par.layout_blocks(), loss='logistic', n_obs=self.n_obs, n_cols=P, device=device)
        self.ctx.set_data(_hip.SLOT_X, x)
        self._y = _hip.as_f64(y).ravel().copy()
        self.ctx.set_data(_hip.SLOT_Y, self._y)
        self._groups = np.ascontiguousarray(np.asarray(groups).ravel(), dtype=np.int32)
        self.ctx.set_groups(self._groups, G)
        w0 = np.ones(self.n_obs) if weights is None else _hip.as_f64(weights).ravel().copy()
        self._declare_hyper('weights', HyperVectorParam('weights', self.n_obs, val=w0))
        self.tilt_par = None
        self._w_res = ResidentVector()
        self._x = x
        self._external = None
        self._point_key = None

    tau_beta = property(lambda self: float(self._hyper_vec('beta_prior_info')[0]))
    mu0 = property(lambda self: float(self._hyper_vec('mu_prior')[0]))
    kappa0 = property(lambda self: float(self._hyper_vec('mu_prior')[1]))
    a0 = property(lambda self: float(self._hyper_vec('tau_prior')[0]))
    b0 = property(lambda self: float(self._hyper_vec('tau_prior')[1]))

    def _index(self, par, names):
        """The layout must be the canonical one: [beta (mean, info) | mu (mean, info) | tau (shape, rate) | u (mean, info)] in
        both vector and free coordinates, every coordinate packed element-wise (identity, or lb + exp)."""
        P, G = self.P, self.G
        self.n_global = ng = 2 * P + 4
        vi, fi = par.vector_indices_dict, par.free_indices_dict
        want = [(names[0], 'mean', 0, P), (names[0], 'info', P, 2 * P), (names[1], 'mean', 2 * P, 2 * P + 1),
                (names[1], 'info', 2 * P + 1, 2 * P + 2), (names[2], 'shape', 2 * P + 2, 2 * P + 3),
                (names[2], 'rate', 2 * P + 3, ng), (names[3], 'mean', ng, ng + G), (names[3], 'info', ng + G, ng + 2 * G)]
        for name, field, lo, hi in want:
            sub = par[name]
            for top, inner in ((vi, sub.vector_indices_dict), (fi, sub.free_indices_dict)):
                if top[name].start + inner[field].start != lo or top[name].start + inner[field].stop != hi:
                    raise ValueError('the parameter must be [UVNParamVector {} ({}) | UVNParam {} | GammaParam {} | UVNParamVector {} ({})] '
                                     'in this order, the group effects pushed last'.format(names[0], P, names[1], names[2], names[3], G))
        if par.vector_size() != ng + 2 * G or par.free_size() != ng + 2 * G:
            raise ValueError('the parameter holds more than the four blocks of the model')
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

    def _push_state(self):
        w = self._w_res.changed(self.weights_par)
        if w is not None:
            self.ctx.set_weights(w)
            self._point_key = None

    # ---- data pieces (GPU) ------------------------------------------------------------------------------------------
    def _device_terms(self, eta, want_grad, want_hess, want_border=True):
        P, G, ng = self.P, self.G, self.n_global
        self._push_state()
        val, gg, gl, Hb, B, L = self.ctx.glmm_terms(eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:], self.gh_x, self.gh_w,
                                                    want_grad=want_grad or want_hess, want_hess=want_hess, want_border=want_border)
        return dict(value=val, g_glob=gg, g_loc=gl, Hb=Hb, border=B, loc=L)

    def local_stats(self, eta):
        """[value | global gradient (2 P) | H blocks (3 P^2) | group sums (G x (5 + 4 P))] of THIS process's rows in the coordinates
        (m, v, e, r) at the vector-coordinate point eta: the buffer of one host-side sum over shards (a group may straddle
        shards: its sums add).  With a reduce hook on the context it is already the sum over the ranks."""
        eta = _hip.as_f64(eta).ravel()
        d = self._device_terms(eta, True, True)
        gs = np.hstack([d['g_loc'], d['loc'], d['border']])
        return np.concatenate([[d['value']], d['g_glob'], d['Hb'].ravel(), gs.ravel()])

    def set_reduced_stats(self, flat, eta=None):
        """Install statistics summed over all shards for the point eta (None = use this process's own rows again)."""
        refuse_double_reduction(getattr(self, 'ctx', None), flat)
        self._point_key = None
        if flat is None:
            self._external = None
            return
        P, G = self.P, self.G
        flat = np.asarray(flat, dtype=np.float64).ravel()
        n = 1 + 2 * P + 3 * P * P + G * (5 + 4 * P)
        if flat.size != n or eta is None:
            raise ValueError('expected {} statistics and the point they were formed at'.format(n))
        self._external = (np.asarray(eta, dtype=np.float64).copy(), flat.copy())

    def _data(self, eta, want_grad, want_hess, want_border=True):
        if self._external is None:
            return self._device_terms(eta, want_grad, want_hess, want_border)
        if not np.array_equal(self._external[0], eta):
            raise ValueError('the installed statistics were formed at another point')
        P, G = self.P, self.G
        f = self._external[1]
        o = 1 + 2 * P
        gs = f[o + 3 * P * P:].reshape(G, 5 + 4 * P)
        return dict(value=float(f[0]), g_glob=f[1:o], Hb=f[o:o + 3 * P * P].reshape(3, P, P), g_loc=gs[:, :2], loc=gs[:, 2:5],
                    border=gs[:, 5:])

    def _closed(self, eta, want_grad=True, want_hess=True, want_border=True):
        d = self._data(eta, want_grad, want_hess, want_border)
        if not (want_grad or want_hess):
            d = dict(value=d['value'])
        return glmm_closed_forms(self.P, self.G, eta, d, self.tau_beta, self.mu0, self.kappa0, self.a0, self.b0, want_hess=want_hess)

    def _arrow(self, x, is_free):
        """(grad, Hgg, rows, Hx, loc) at x in its own coordinates, cached per point, weights and hyper-parameters."""
        self._push_state()
        key = (bool(is_free), np.asarray(x, dtype=np.float64).tobytes(), self._w_res.key, self._hyper_state_key(),
               None if self._external is None else id(self._external))
        if self._point_key != key:
            eta = self._eta(x, is_free)
            cf = self._closed(eta)
            if is_free:
                j1, j2 = self._jac(eta)
                self._pieces = arrow_to_free(cf, j1, j2, self.n_global, self.G)
            else:
                self._pieces = (cf['grad'], cf['Hgg'], cf['rows'], cf['Hx'], cf['loc'])
            self._point_key = key
        else:
            self._eta(x, is_free)
        return self._pieces

    # ---- functor protocol -------------------------------------------------------------------------------------------
    def __call__(self):
        return self.value(np.asarray(self.par.get_free(), dtype=np.float64), True)

    @_hip.host_blas
    def value(self, x, is_free=True):
        return self._closed(self._eta(x, is_free), False, False)['value']

    @_hip.host_blas
    def grad(self, x, is_free=True):
        eta = self._eta(x, is_free)
        g = self._closed(eta, True, False)['grad']
        return g * self._jac(eta)[0] if is_free else g

    jacobian = grad

    @_hip.host_blas
    def hessian(self, x, is_free=True):
        if self.par.vector_size() > 8192:
            raise MemoryError('dense Hessian of {} parameters: use global_hessian() (Schur complement) or hvp()'.format(self.par.vector_size()))
        _, Hgg, rows, Hx, loc = self._arrow(x, is_free)
        return arrow_dense(Hgg, rows, Hx, loc)

    @_hip.host_blas
    def hvp(self, x, v, is_free=True):
        _, Hgg, rows, Hx, loc = self._arrow(x, is_free)
        return arrow_matvec(Hgg, rows, Hx, loc, v)

    @_hip.host_blas
    def sparse_hessian(self, free_val):
        """The free-coordinate Hessian as a scipy CSR arrow: global block, border and 2 x 2 local blocks."""
        from .objectives import get_sparse_sub_hessian, get_sparse_sub_matrix
        _, Hgg, rows, Hx, loc = self._arrow(free_val, True)
        ng, G = self.n_global, self.G
        D = ng + 2 * G
        gi, li = np.arange(ng), np.arange(ng, D)
        H = get_sparse_sub_hessian(Hgg, gi, D)
        H = H + get_sparse_sub_matrix(Hx, rows, li, D, D) + get_sparse_sub_matrix(Hx.T, li, rows, D, D)
        ie, ii = li[:G], li[G:]
        H = H + sp_sparse.coo_matrix((np.concatenate([loc[:, 0], loc[:, 2], loc[:, 1], loc[:, 1]]),
                                      (np.concatenate([ie, ii, ie, ii]), np.concatenate([ie, ii, ii, ie]))), shape=(D, D))
        return H.tocsr()

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
        covariance of the global parameters.  Device route: the border formed by `lrvb_glmm_terms` stays on the GPU and
        `lrvb_glmm_schur` eliminates the 2 G local parameters there; the host adds the N-independent terms to the G local 2 x 2
        blocks (free coordinates) and sends them with the chain factors.  The result stays resident for `chol_factor_last`."""
        fv = _hip.as_f64(free_val).ravel()
        P, G, ng = self.P, self.G, self.n_global
        self._push_state()
        eta = self._eta(fv, True)
        j1, j2 = self._jac(eta)
        cf = self._closed(eta, want_border=False)    # the group sums of the point stay resident; the border is not copied back
        g, Hgg, rows = cf['grad'], cf['Hgg'].copy(), cf['rows']
        if self._external is None:
            _, _, _, _, loc_f = arrow_to_free(cf, j1, j2, ng, G)
            r = 1.0 / eta[ng + G:]
            a, b = eta[2 * P + 2], eta[2 * P + 3]
            d = eta[ng:ng + G] - eta[2 * P]
            ta, tb = 1.0 / b, -a / b ** 2
            closed = np.empty((G, 6))
            closed[:, 0], closed[:, 1], closed[:, 2] = -a / b, d * ta, d * tb
            closed[:, 3], closed[:, 4], closed[:, 5] = 0.0, 0.5 * ta, 0.5 * tb
            scale = np.stack([j1[ng:ng + G], -r * r * j1[ng + G:]], axis=1)
            M = self.ctx.glmm_schur(loc_f, scale, closed)            # coordinates [m | v | e_mu, a, b]
            dv = np.concatenate([np.ones(P), -1.0 / eta[P:2 * P] ** 2, np.ones(3)])
            M = M * dv[:, None] * dv[None, :]
        else:
            jl = np.concatenate([j1[ng:ng + G], j1[ng + G:]])
            _, _, _, _, loc_f = arrow_to_free(cf, j1, j2, ng, G)
            M = arrow_schur_term(rows, cf['Hx'] * jl[None, :], loc_f)
        Hgg[np.ix_(rows, rows)] -= M
        gc = self._ensure_gctx()
        gc.hvec_begin()
        gc.hvec_add_block(Hgg, 0, 0)
        out = gc.hvec_finish(fv[:ng], g[:ng], True, want_host=want_host)
        self._schur_key = self._resident_key(fv)
        return out

    def _resident_key(self, fv):
        """What the Schur complement resident on the global context was built at: point, weights, hyper-parameters."""
        return (np.asarray(fv, dtype=np.float64).tobytes(), self._w_res.key, self._hyper_state_key(),
                None if self._external is None else id(self._external))

    # ---- the whole arrow: solve, covariance of any moment, weight influence --------------------------------------------------
    @_hip.host_blas
    def solve(self, x, R, is_free=True, resident_factor=False):
        """H^-1 R at x (R: D x Q or a D-vector, local rows allowed) by `arrow_solve`.  resident_factor=True solves the Schur
        complement with the factor on the global context: call `global_hessian(x, want_host=False)` and
        `_ensure_gctx().chol_factor_last()` at the same point first (free coordinates).  A factor built at another point,
        or under other weights or hyper-parameters, is refused with a ValueError."""
        _, Hgg, rows, Hx, loc = self._arrow(x, is_free)
        if resident_factor and (not is_free or getattr(self, '_schur_key', None) != self._resident_key(_hip.as_f64(x).ravel())):
            raise ValueError('resident_factor=True needs global_hessian(x, want_host=False) and chol_factor_last() at this point, '
                             'with these weights and hyper-parameters, in free coordinates')
        schur_solve = self._ensure_gctx().chol_solve if resident_factor else None
        return arrow_solve(Hgg, rows, Hx, loc, R, schur_solve=schur_solve)

    def _moment_jac(self, moment_jac):
        M = np.atleast_2d(_hip.as_f64(moment_jac))
        D = self.n_global + 2 * self.G
        if M.ndim != 2 or M.shape[1] not in (D, self.n_global):
            raise ValueError('moment Jacobian must have {} (all parameters) or {} (global parameters) columns'.format(D, self.n_global))
        if M.shape[1] != D:
            M = np.hstack([M, np.zeros((M.shape[0], D - M.shape[1]))])
        return M

    def lrvb_cov(self, x, moment_jac, is_free=True):
        """M H^-1 M^T (Q x Q): the linear-response covariance of the moments M theta, M = moment_jac being Q x D (columns of the
        group effects allowed) or Q x n_global (zero-padded)."""
        M = self._moment_jac(moment_jac)
        return M @ self.solve(x, np.ascontiguousarray(M.T), is_free)

    def _influence_operand(self, x, moment_jac, is_free, chol):
        """A = -M H^-1 J (Q x (2 P + 2 G)) in the coordinates (m, v, e, r) of the device entries, and the point in them."""
        self._push_state()
        M = self._moment_jac(moment_jac)
        P, G, ng = self.P, self.G, self.n_global
        if chol is None:
            S = self.solve(x, np.ascontiguousarray(M.T), is_free)
        else:
            S = np.asarray(chol.solve(np.ascontiguousarray(M.T))).reshape(ng + 2 * G, -1)
        eta = self._eta(x, is_free)
        j1 = self._jac(eta)[0] if is_free else np.ones(eta.size)
        v, r = 1.0 / eta[P:2 * P], 1.0 / eta[ng + G:]
        chain = np.concatenate([j1[:P], -v * v * j1[P:2 * P], j1[ng:ng + G], -r * r * j1[ng + G:]])
        keep = np.concatenate([np.arange(2 * P), np.arange(ng, ng + 2 * G)])
        A = -(S[keep] * chain[:, None]).T
        return np.ascontiguousarray(A), (eta[:P], v, eta[ng:ng + G], r, self.gh_x, self.gh_w)

    def obs_influence(self, x, moment_jac, n0=0, n1=None, is_free=True, chol=None):
        """Rows n0..n1 of (moment_jac @ d par / d w)^T ((n1 - n0) x Q), streamed over the observations on the device
        (`lrvb_glmm_obs_influence`); the N x D cross Hessian is never formed.  A = -moment_jac H^-1 J comes from the dense factor
        `chol` where one is given (ParametricSensitivityLinearApproximation holds it), otherwise from `arrow_solve` -- the route
        for large G, where no dense factor exists.  Per unit weight: a row of weight zero gets the influence of adding it."""
        A, pt = self._influence_operand(x, moment_jac, is_free, chol)
        return self.ctx.glmm_obs_influence(*pt, A, n0=n0, n1=n1)

    def group_influence(self, x, moment_jac, is_free=True, chol=None):
        """G x Q: row g is the derivative of the moments with respect to a common multiplier on the weights of group g's rows,
        sum_{n in g} w_n * (row n of `obs_influence`) -- minus it is the linear prediction of leaving the cluster out.  The
        group's own prior term on u_g stays in the model and is not part of it.  Fixed summation order on the device
        (`lrvb_glmm_group_influence`); an empty group gives a zero row."""
        A, pt = self._influence_operand(x, moment_jac, is_free, chol)
        return self.ctx.glmm_group_influence(*pt, A)

    # ---- hyper-parameters ---------------------------------------------------------------------------------------------
    def _prior_hyper(self, kind, eta_g, want):
        P, ng = self.P, self.n_global
        m, ib = eta_g[:P], eta_g[P:2 * P]
        e_mu, i_mu, a, b = eta_g[2 * P:ng]
        if kind == 'beta_prior_info':
            if want == 'grad':
                return np.array([0.5 * (np.sum(m * m) + np.sum(1.0 / ib))])
            C = np.zeros((ng, 1))
            C[:P, 0], C[P:2 * P, 0] = m, -0.5 / ib ** 2
            return C
        if kind == 'mu_prior':
            if want == 'grad':
                return np.array([-self.kappa0 * (e_mu - self.mu0), 0.5 * ((e_mu - self.mu0) ** 2 + 1.0 / i_mu)])
            C = np.zeros((ng, 2))
            C[2 * P, 0], C[2 * P, 1], C[2 * P + 1, 1] = -self.kappa0, e_mu - self.mu0, -0.5 / i_mu ** 2
            return C
        if kind != 'tau_prior':
            raise NotImplementedError(kind)
        if want == 'grad':
            return gamma_prior_hyper_grad(a, b, special)
        return gamma_prior_hyper_cross(ng, 2 * P + 2, 2 * P + 3, a, b, special)

    def hyper_grad(self, hyper_par, val1, val1_is_free):
        kind = self.hyper_kind(hyper_par)
        if kind == 'weights':
            raise NotImplementedError('d f / d weights is not declared')
        return self._prior_hyper(kind, self._eta(val1, val1_is_free)[:self.n_global], 'grad')

    def global_cross_hessian(self, hyper_par, val, is_free=True):
        """The n_global rows of the cross Hessian with a PRIOR hyper-parameter (its 2 G local rows are zero)."""
        kind = self.hyper_kind(hyper_par)
        if kind == 'weights':
            raise NotImplementedError('the weight cross Hessian has local rows: use cross_hessian')
        eta = self._eta(val, is_free)
        C = self._prior_hyper(kind, eta[:self.n_global], 'cross')
        return C * self._jac(eta)[0][:self.n_global, None] if is_free else C

    @_hip.host_blas
    def cross_hessian(self, hyper_par, val1, val1_is_free):
        """d2 f / d par1 d hyper^T, all rows (dense protocol: small N and G).  Weights: column n is the gradient of row n's
        term per unit weight, [(psi_rho - y) x_n | psi_s x_n o x_n chained to i_beta | 0 | at g(n): psi_rho - y, psi_s chained
        to i_g] -- its local rows are NOT zero.  Priors: the local rows are zero."""
        kind = self.hyper_kind(hyper_par)
        val1 = _hip.as_f64(val1).ravel()
        if kind != 'weights':
            Cg = self.global_cross_hessian(hyper_par, val1, is_free=val1_is_free)
            return np.vstack([Cg, np.zeros((val1.size - self.n_global, Cg.shape[1]))])
        eta = self._eta(val1, val1_is_free)
        P, G, ng, N = self.P, self.G, self.n_global, self.n_obs
        x, gid = self._x, self._groups
        v, r = 1.0 / eta[P:2 * P], 1.0 / eta[ng + G:]
        rho = x @ eta[:P] + eta[ng:ng + G][gid]
        s = (x * x) @ v + r[gid]
        sd = np.sqrt(s)
        _, d1, _ = self.ctx.gh_logistic(rho, sd, self.gh_x, self.gh_w, order=2)
        p_rho = d1[:, 0] - self._y
        p_s = 0.5 * d1[:, 1] / sd                            # s_n >= 1 / i_g > 0
        C = np.zeros((N, ng + 2 * G))
        C[:, :P] = p_rho[:, None] * x
        C[:, P:2 * P] = p_s[:, None] * (x * x) * (-v * v)[None, :]
        n = np.arange(N)
        C[n, ng + gid] = p_rho
        C[n, ng + G + gid] = p_s * (-r * r)[gid]
        if val1_is_free:
            C = C * self._jac(eta)[0][None, :]
        return np.ascontiguousarray(C.T)

    def global_sensitivity(self, hyper_par, free_val):
        """d theta_global / d hyper^T = -H_S^-1 C_g (n_global x Ph) for a prior hyper-parameter: its cross Hessian has no local
        rows, so the local parameters enter through the Schur complement only."""
        Cg = self.global_cross_hessian(hyper_par, free_val)
        gc = self._ensure_gctx()
        self.global_hessian(free_val, want_host=False)
        gc.chol_factor_last()
        return -gc.chol_solve(Cg)

"""Logistic regression with a full-covariance Gaussian variational posterior: q(beta) = N(m, Lambda^-1), an `MVNParam`
(LRVB/NormalParams.py:6-23) whose information matrix is a log-Cholesky `PosDefMatrixParam`.

    mu_n = x_n . m,  s_n = x_n^T Sigma x_n,  Sigma = Lambda^-1
    KL(eta) = sum_n w_n ( psi(mu_n, s_n) - y_n mu_n )            psi(mu, s) = E log(1 + e^z), z ~ N(mu, s)  (Gauss-Hermite)
            + 1/2 prior_info (m^T m + tr Sigma)                   (beta ~ N(0, I / prior_info))
            + 1/2 log det Lambda                                  (minus the entropy, up to a constant)

Vector coordinates eta = [m | vech Lambda] (row-major lower triangle).  The O(N) work runs on the GPU in the coordinates
(m, vech Sigma) (`lrvb_logitnormal_mvn_terms`: the Sigma-Sigma block is the packed-triangle Kronecker SYRK); the chain to
vech Lambda is N-independent and runs on the device too (`lrvb_logitnormal_mvn_chain`).  The Hessian-vector product is
matrix-free (`lrvb_logitnormal_mvn_hvp`) with the P x P chain pieces on the host.  Derivatives in the variance s use Stein's
identity on the quadrature nodes (d_s psi = E g'' / 2, ...): they equal the derivatives of the quadrature value to within the
quadrature error, exactly where psi is resolved, and a zero design row (s = 0) is regular.
"""
import numpy as np

from . import _hip
from .models import DeviceContext, DeviceModel

MAX_P = 64


def _delta(P):
    """Duplication weights of vech coordinates: 1 on the diagonal, 2 off it."""
    r, c = np.tril_indices(P)
    return np.where(r == c, 1.0, 2.0)


def _unvech_sym(v, P):
    """Symmetric matrix whose lower triangle is the vech vector v (an off-diagonal entry fills both places)."""
    A = np.zeros((P, P))
    A[np.tril_indices(P)] = v
    return A + np.tril(A, -1).T


def _vech(A):
    return A[np.tril_indices(A.shape[0])]


def chain_grad(P, Sigma, m, g_sig, tau):
    """Gradient in (m, vech Lambda) of data term + prior + entropy from the data-term gradient g_sig in (m, vech Sigma).
    Returns (gradient, M = Sigma G Sigma, G) with G the symmetric matrix gradient in Sigma (prior included)."""
    d = _delta(P)
    G = _unvech_sym(g_sig[P:] / d, P) + 0.5 * tau * np.eye(P)
    M = Sigma @ G @ Sigma
    g = np.concatenate([g_sig[:P] + tau * m, -d * _vech(M) + 0.5 * d * _vech(Sigma)])
    return g, M, G


def chain_hvp(P, Sigma, M, v_lam, hv_sig_fn):
    """Product of the (m, vech Lambda) Hessian with v_lam = [v_m | v_Lambda], given hv_sig_fn, the data-term product in
    (m, vech Sigma).  dSigma = -Sigma dLambda Sigma on the way in; on the way out J^T, the second order of Lambda -> Lambda^-1
    (2 symkron(M, Sigma)) and the log-det term (-1/2 symkron(Sigma, Sigma)), all as P x P matrix products."""
    d = _delta(P)
    dL = _unvech_sym(v_lam[P:], P)
    Vs = -Sigma @ dL @ Sigma
    hv = hv_sig_fn(np.concatenate([v_lam[:P], _vech(Vs)]))
    R = _unvech_sym(hv[P:] / d, P)
    Q = -Sigma @ R @ Sigma + Sigma @ dL @ M + M @ dL @ Sigma - 0.5 * Sigma @ dL @ Sigma
    return np.concatenate([hv[:P], d * _vech(Q)])


def psd_free_jvp(free_l, u_l, P):
    """d vech(Lambda) along the free direction u_l, Lambda = L L^T (+ diag_lb I), L = lower triangle of free_l with exp diagonal."""
    L = _unvech_lower(free_l, P)
    np.fill_diagonal(L, np.exp(np.diag(L)))
    dL = _unvech_lower(u_l, P)
    np.fill_diagonal(dL, np.diag(dL) * np.diag(L))
    return _vech(dL @ L.T + L @ dL.T)


def psd_free_vjp_hvp(free_l, u_l, r, g, P):
    """J^T r + (sum_k g_k d2 vech(Lambda)_k / d free^2) u_l for the log-Cholesky block (r, g: vector-coordinate covectors)."""
    L = _unvech_lower(free_l, P)
    np.fill_diagonal(L, np.exp(np.diag(L)))
    kap = np.where(np.eye(P) > 0, np.diag(L)[:, None] * np.ones((1, P)), 1.0)
    d = _delta(P)
    Rm = _unvech_sym(r / d, P)
    Gm = _unvech_sym(g / d, P)
    dLu = _unvech_lower(u_l, P) * kap
    out = 2.0 * (Rm @ L) * kap + 2.0 * (Gm @ dLu) * kap
    out[np.diag_indices(P)] += 2.0 * np.diag(Gm @ L) * np.diag(L) * np.diag(_unvech_lower(u_l, P))
    return out[np.tril_indices(P)]


def _unvech_lower(v, P):
    A = np.zeros((P, P))
    A[np.tril_indices(P)] = v
    return A


class LogitNormalMVNRegressionObjective(DeviceModel):
    _stats_at_point = True

    def __init__(self, par, x, y, beta_name='beta', prior_info=1.0, gh_deg=20, weights=None, device=0):
        self.par = par
        x = _hip.as_f64(x)
        if x.ndim != 2:
            raise ValueError('x must be an N x P matrix')
        self.n_obs, self.P = x.shape
        P = self.P
        self.Pv = P * (P + 1) // 2
        beta = par[beta_name]
        try:
            ok = beta['mean'].free_size() == P and beta['info'].free_size() == self.Pv and len(beta['info'].get()) == P
        except (KeyError, AttributeError, TypeError):
            ok = False
        if not ok:
            raise ValueError('`{}` must be an MVNParam of dimension {}'.format(beta_name, P))
        if par.vector_size() != P + self.Pv:
            raise ValueError('the parameter must hold the MVNParam and nothing else')
        if P > MAX_P:
            raise NotImplementedError('full-covariance logistic regression needs P <= {} (got {}): the Sigma-Sigma Hessian block '
                                      'is the packed-triangle Kronecker SYRK, whose on-chip stage holds 64 columns'.format(MAX_P, P))
        gh_deg = int(gh_deg)
        if not 1 <= gh_deg <= 128:
            raise ValueError('1 to 128 Gauss-Hermite nodes (got {})'.format(gh_deg))
        yv = _hip.as_f64(y).ravel().copy()
        if yv.size != self.n_obs:
            raise ValueError('y has {} entries for {} rows of x'.format(yv.size, self.n_obs))
        self.prior_info = float(prior_info)
        self.gh_x, self.gh_w = np.polynomial.hermite.hermgauss(gh_deg)
        self.ctx = DeviceContext(par.layout_blocks(), loss='logistic', n_obs=self.n_obs, n_cols=P, device=device)
        if self.ctx.D != par.free_size() or self.ctx.V != par.vector_size():
            raise ValueError('layout_blocks() of the parameter disagrees with its free/vector sizes')
        self.ctx.set_data(_hip.SLOT_X, x)
        self._y = yv
        self.ctx.set_data(_hip.SLOT_Y, self._y)
        self._declare_weights(self.n_obs, weights)
        self._x = x
        self.n_dense_builds = 0            # data-term Hessians formed (the matrix-free product never adds to it)
        self._lib = _hip.load()

    def _point(self, eta):
        P = self.P
        Lam = _unvech_sym(eta[P:], P)
        C = np.linalg.cholesky(Lam)
        Ci = np.linalg.solve(C, np.eye(P))
        Sigma = Ci.T @ Ci
        return eta[:P].copy(), np.ascontiguousarray(0.5 * (Sigma + Sigma.T)), 2.0 * np.sum(np.log(np.diag(C)))

    # ---- device calls in (m, vech Sigma) ------------------------------------------------------------------------
    def mvn_terms(self, mean, cov, want_grad=True, want_hess=True):
        """Data term in (m, vech Sigma): value, gradient (D) and Hessian (D x D) (lrvb_logitnormal_mvn_terms)."""
        m, S = _hip.as_f64(mean).ravel(), _hip.as_f64(cov)
        D = self.P + self.Pv
        val = np.empty(1)
        g = np.empty(D) if want_grad else None
        H = np.empty((D, D)) if want_hess else None
        self._push_state()
        self.ctx._check(self._lib.lrvb_logitnormal_mvn_terms(self.ctx._h, _hip.ptr(m), _hip.ptr(S), m.size, _hip.ptr(self.gh_x),
                                                             _hip.ptr(self.gh_w), self.gh_x.size, _hip.ptr(val), _hip.ptr(g), _hip.ptr(H)))
        if want_hess:
            self.n_dense_builds += 1
        return float(val[0]), g, H

    def mvn_hvp(self, mean, cov, v):
        """Data-term Hessian times v in (m, vech Sigma), matrix-free (lrvb_logitnormal_mvn_hvp)."""
        m, S, v = _hip.as_f64(mean).ravel(), _hip.as_f64(cov), _hip.as_f64(v).ravel()
        out = np.empty(self.P + self.Pv)
        self._push_state()
        self.ctx._check(self._lib.lrvb_logitnormal_mvn_hvp(self.ctx._h, _hip.ptr(m), _hip.ptr(S), m.size, _hip.ptr(self.gh_x),
                                                           _hip.ptr(self.gh_w), self.gh_x.size, _hip.ptr(v), _hip.ptr(out)))
        return out

    def _chain_hessian(self, Sigma, M, H_sig):
        D = self.P + self.Pv
        out = np.empty((D, D))
        self.ctx._check(self._lib.lrvb_logitnormal_mvn_chain(self.ctx._h, self.P, _hip.ptr(Sigma), _hip.ptr(_hip.as_f64(M)),
                                                             _hip.ptr(_hip.as_f64(H_sig)), _hip.ptr(out)))
        return out

    # ---- observations sharded over GPUs: the data term is a sum over rows --------------------------------------
    def local_stats(self, eta):
        """[value | gradient (D) | Hessian (D^2)] of THIS process's rows in (m, vech Sigma) at the vector-coordinate point eta:
        the buffer of the one sum all-reduce per evaluation; prior, entropy and the chain to vech Lambda follow it."""
        eta = _hip.as_f64(eta).ravel()
        m, S, _ = self._point(eta)
        val, g, H = self.mvn_terms(m, S)
        return np.concatenate([[val], g, H.ravel()])

    def set_reduced_stats(self, flat, eta=None):
        """Install statistics summed over all shards for the point eta (None = use this process's own rows again)."""
        D = self.P + self.Pv
        self._install_reduced_stats(flat, 1 + D + D * D, eta)

    def _data_terms(self, eta, m, S, want_grad, want_hess):
        D = self.P + self.Pv
        f = self._installed_stats(eta)
        if f is not None:
            return float(f[0]), f[1:1 + D], f[1 + D:].reshape(D, D)
        return self.mvn_terms(m, S, want_grad=want_grad, want_hess=want_hess)

    # ---- vector coordinates (m, vech Lambda) ------------------------------------------------------------------
    def _terms(self, eta, want_grad=True, want_hess=True):
        P, tau = self.P, self.prior_info
        m, Sigma, logdet_lam = self._point(eta)
        val, g_sig, H_sig = self._data_terms(eta, m, Sigma, want_grad or want_hess, want_hess)
        val += 0.5 * tau * (m @ m + np.trace(Sigma)) + 0.5 * logdet_lam
        if not (want_grad or want_hess):
            return val, None, None
        g, M, _ = chain_grad(P, Sigma, m, g_sig, tau)
        if not want_hess:
            return val, g, None
        H = self._chain_hessian(Sigma, M, H_sig)
        H[:P, :P] += tau * np.eye(P)
        return val, g, H

    # ---- functor protocol ------------------------------------------------------------------------------------
    def value(self, x, is_free=True):
        return float(self._terms(self._eta(x, is_free), False, False)[0])

    def grad(self, x, is_free=True):
        g = self._terms(self._eta(x, is_free), True, False)[1]
        if not is_free:
            return g
        # J^T g through the log-Cholesky map as P x P products (the mean block is the identity)
        P, xf = self.P, _hip.as_f64(x).ravel()
        z = np.zeros(self.Pv)
        return np.concatenate([g[:P], psd_free_vjp_hvp(xf[P:], z, g[P:], z, P)])

    jacobian = grad

    def hessian(self, x, is_free=True):
        _, g, H = self._terms(self._eta(x, is_free))
        return self.ctx.free_hessian_from_vector(x, g, H) if is_free else H

    def hvp(self, x, v, is_free=True):
        """Hessian times v without forming a D x D matrix: the data term by `lrvb_logitnormal_mvn_hvp`, the chain to
        vech Lambda and (for free coordinates) through the log-Cholesky map as P x P matrix products."""
        P, tau = self.P, self.prior_info
        v = _hip.as_f64(v).ravel()
        eta = self._eta(x, is_free)
        if self._external_stats is not None:
            H = self.hessian(x, is_free)
            return H @ v
        m, Sigma, _ = self._point(eta)
        if is_free:
            xf = _hip.as_f64(x).ravel()
            v_lam = np.concatenate([v[:P], psd_free_jvp(xf[P:], v[P:], P)])
        else:
            v_lam = v
        _, g_sig, _ = self.mvn_terms(m, Sigma, want_grad=True, want_hess=False)
        g, M, _ = chain_grad(P, Sigma, m, g_sig, tau)
        hv = chain_hvp(P, Sigma, M, v_lam, lambda u: self.mvn_hvp(m, Sigma, u))
        hv[:P] += tau * v_lam[:P]
        if not is_free:
            return hv
        return np.concatenate([hv[:P], psd_free_vjp_hvp(xf[P:], v[P:], hv[P:], g[P:], P)])

    # ---- weight sensitivity ------------------------------------------------------------------------------------
    def cross_hessian(self, hyper_par, val1, val1_is_free):
        """d2 f / d par1 d w^T (D x N).  Row n of the per-observation gradient matrix in (m, vech Lambda) is
        [(psi_mu - y_n) x_n | -psi_s delta o vech(z_n z_n^T)], z_n = Sigma x_n, chained to free coordinates if asked."""
        self.hyper_kind(hyper_par)
        P, D = self.P, self.P + self.Pv
        if self.n_obs * D > 2 ** 28:
            raise MemoryError('the dense cross Hessian would hold {} x {} doubles; shard the observations'.format(D, self.n_obs))
        eta = self._eta(val1, val1_is_free)
        m, Sigma, _ = self._point(eta)
        x = self._x
        z = x @ Sigma
        mu, s = x @ m, np.maximum(np.einsum('ij,ij->i', x, z), 0.0)
        _, d1, d2 = self.ctx.gh_logistic(mu, np.sqrt(s), self.gh_x, self.gh_w, order=2)
        r, c = np.tril_indices(P)
        d = _delta(P)
        G = np.hstack([(d1[:, 0] - self._y)[:, None] * x, (-0.5 * d2[:, 0])[:, None] * z[:, r] * z[:, c] * d[None, :]])
        if val1_is_free:
            G = G @ self.ctx.free_to_vector_jac(val1)
        return np.ascontiguousarray(G.T)

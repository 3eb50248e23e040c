"""Multinomial (softmax) logistic regression: the MAP / delta-q objective whose Hessian is the LRVB / Laplace precision.

    K classes, labels y_n in {0 .. K-1}, class 0 the reference (as in `SimplexParam`); beta = (K-1) x P, row a = class a + 1
    z_na = x_n . beta_a,  z_n0 = 0,  p_n = softmax(z_n)
    f(beta) = sum_n w_n [ log sum_k e^{z_nk} - z_{n, y_n} ]  +  1/2 (eta - m)^T diag(tau) (eta - m),   eta = vec(beta)

The O(N) work runs on the GPU (`lrvb_softmax_*`, k_softmax.hip): one fused pass over X for value, gradient
and the class probabilities, one for each matrix-free Hessian-vector product, and K(K-1)/2 weighted SYRKs for the Hessian.
The prior, the free-coordinate conversion (device) and the bookkeeping follow on the host.  Same functor protocol as the
other model classes, so `Objective`, `get_lrvb_cov`, `ParametricSensitivityLinearApproximation` (hyper-parameter = the
observation weights, rows streamed by `obs_influence`), `ConjugateGradientSolver` and trust-ncg apply.  K = 2 is the
logistic GLM (`GLMObjective(loss='logistic')`).
"""
import numpy as np
import scipy.sparse.linalg

from . import _hip
from .models import DeviceContext, DeviceModel
from .packing import ArrayParam, _box_d1_d2

MAX_CLASSES = 17
MAX_COLS = 1024


class SoftmaxRegressionObjective(DeviceModel):

    def __init__(self, par, x, y, n_classes, beta_name='beta', prior_info=1.0, prior_mean=None, weights=None, device=0):
        K = int(n_classes)
        if K != n_classes or K < 2 or K > MAX_CLASSES:
            raise ValueError('n_classes must be an integer in [2, {}] (got {})'.format(MAX_CLASSES, n_classes))
        x = _hip.as_f64(x)
        if x.ndim != 2:
            raise ValueError('x must be an N x P matrix')
        N, P = x.shape
        if P < 1 or P > MAX_COLS:
            raise ValueError('softmax regression is built for 1 <= P <= {} columns (got {})'.format(MAX_COLS, P))
        y = np.asarray(y).ravel()
        if y.size != N:
            raise ValueError('y must have {} labels (got {})'.format(N, y.size))
        if y.dtype == bool or not (np.issubdtype(y.dtype, np.integer) or np.issubdtype(y.dtype, np.floating)):
            raise ValueError('labels must be integers in [0, {})'.format(K))
        if np.issubdtype(y.dtype, np.floating) and not (np.all(np.isfinite(y)) and np.all(y == np.round(y))):
            raise ValueError('labels must be integers in [0, {})'.format(K))
        if y.size and (y.min() < 0 or y.max() >= K):
            raise ValueError('labels must be integers in [0, {}) (found {} .. {})'.format(K, y.min(), y.max()))
        try:
            beta = par[beta_name]
        except (KeyError, TypeError):
            raise ValueError('the parameter has no entry `{}`'.format(beta_name))
        if not isinstance(beta, ArrayParam) or tuple(beta.shape()) != (K - 1, P):
            raise ValueError('`{}` must be an ArrayParam of shape ({}, {}) = (n_classes - 1, n_cols)'.format(beta_name, K - 1, P))
        D = (K - 1) * P
        if par.vector_size() != D or par.free_size() != D:
            raise ValueError('the parameter must hold the ArrayParam `{}` and nothing else'.format(beta_name))
        self.par, self.n_obs, self.P, self.K, self.D = par, N, P, K, D
        tau = np.broadcast_to(_hip.as_f64(prior_info).ravel() if np.ndim(prior_info) else float(prior_info), (D,))
        self.prior_info = np.array(tau, dtype=np.float64)
        m = np.zeros(D) if prior_mean is None else _hip.as_f64(prior_mean).ravel()
        if m.size != D:
            raise ValueError('prior_mean must have (n_classes - 1) * n_cols = {} entries'.format(D))
        self.prior_mean = m.copy()
        self.ctx = DeviceContext(par.layout_blocks(), loss='data_only', n_obs=N, n_cols=P, device=device)
        if self.ctx.D != D or self.ctx.V != D:
            raise ValueError('layout_blocks() of the parameter disagrees with its free/vector sizes')
        self.ctx.set_data(_hip.SLOT_X, x)
        self._y = y.astype(np.int32)
        self.ctx.softmax_set_labels(self._y, K)
        self._declare_weights(N, weights)
        self._x = x
        self._lb, self._ub = beta._lb, beta._ub
        self._identity_map = bool(np.all(np.isneginf(self._lb)) and np.all(np.isposinf(self._ub)))     # free = vector coordinates

    # ---- vector coordinates --------------------------------------------------------------------------------------
    def _terms(self, eta, want_grad=True, want_hess=True):
        self._push_state()
        val, g, H = self.ctx.softmax_terms(eta, self.K, want_grad=want_grad or want_hess, want_hess=want_hess)
        d = eta - self.prior_mean
        val += 0.5 * float(np.dot(d, self.prior_info * d))
        if g is not None:
            g = g + self.prior_info * d
        if H is not None:
            H[np.diag_indices(self.D)] += self.prior_info
        return val, g, H

    # per point: the diagonal Jacobian of the box map and the diagonal second-order term of the free conversion
    def _point(self, x, is_free):
        def make():
            eta = self._eta(x, is_free)
            g = self._terms(eta, True, False)[1]
            if not is_free:
                return eta, np.ones(self.D), np.zeros(self.D)
            d1, d2 = self._box_diag(x)
            return eta, d1, g * d2
        return self._at_point('point', x, is_free, make)

    def _box_diag(self, x):
        """First and second derivatives of the (element-wise) box map vector = constrain(free): the diagonal of the free-to-vector
        Jacobian and of the second-order term of the free conversion, O(D) instead of the dense D x D matrices."""
        if self._identity_map:
            return np.ones(self.D), np.zeros(self.D)
        return _box_d1_d2(_hip.as_f64(x).ravel(), self._lb, self._ub)

    # ---- functor protocol ------------------------------------------------------------------------------------------
    def value(self, x, is_free=True):
        return float(self._terms(self._eta(x, is_free), False, False)[0])

    def grad(self, x, is_free=True):
        g = self._terms(self._eta(x, is_free), True, False)[1]
        return self._box_diag(x)[0] * g if is_free else g

    jacobian = grad

    def hessian(self, x, is_free=True):
        _, g, H = self._terms(self._eta(x, is_free))
        return self.ctx.free_hessian_from_vector(x, g, H) if (is_free and not self._identity_map) else H

    def hvp(self, x, v, is_free=True):
        """Matrix-free: one fused pass over X per product (`lrvb_softmax_hvp`)."""
        eta, jd, td = self._point(x, is_free)
        u = jd * _hip.as_f64(v).ravel()
        hu = self.ctx.softmax_hvp(eta, self.K, u) + self.prior_info * u
        return jd * hu + td * _hip.as_f64(v).ravel()

    def cg_solve(self, free_val, b, x0=None, Minv=None, tol=1e-8, maxiter=0):
        """H^-1 b by conjugate gradients on the matrix-free products; returns (x, info, iterations)."""
        D = self.D
        count = [0]

        def mv(v):
            count[0] += 1
            return self.hvp(free_val, v, True)
        op = scipy.sparse.linalg.LinearOperator((D, D), matvec=mv)
        M = None if Minv is None else np.asarray(Minv, dtype=np.float64)
        sol, info = scipy.sparse.linalg.cg(op, _hip.as_f64(b).ravel(), x0=x0, rtol=tol, atol=0.0, M=M,
                                           maxiter=(maxiter if maxiter else None))
        return sol, int(info), count[0]

    # ---- weight sensitivity --------------------------------------------------------------------------------------
    def _logits(self, eta):
        z = np.zeros((self.n_obs, self.K))
        z[:, 1:] = self._x @ eta.reshape(self.K - 1, self.P).T
        return z

    def hyper_grad(self, hyper_par, val1, val1_is_free):
        """d f / d w_n = log sum_k e^{z_nk} - z_{n, y_n} (N)."""
        self.hyper_kind(hyper_par)
        z = self._logits(self._eta(val1, val1_is_free))
        m = np.maximum(z.max(axis=1), 0.0)
        lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
        return lse - z[np.arange(self.n_obs), self._y]

    def cross_hessian(self, hyper_par, val1, val1_is_free):
        """d2 f / d par1 d w^T (D x N), column n = vec((p_n - e_{y_n}) x_n^T) chained to free coordinates if asked.
        Dense: for small N (the streamed rows are `obs_influence`)."""
        self.hyper_kind(hyper_par)
        self._push_state()
        eta = self._eta(val1, val1_is_free)
        C = self.ctx.softmax_obs_influence(eta, self.K, np.eye(self.D)).T
        if val1_is_free:
            C = self._box_diag(val1)[0][:, None] * C
        return np.ascontiguousarray(C)

    def obs_influence(self, x, moment_jac, n0=0, n1=None, is_free=True, chol=None):
        """Rows n0..n1 of (moment_jac @ d par / d w)^T ((n1 - n0) x Q), streamed over the observations on the device:
        A = -moment_jac H^-1 J^T (Q x D, from the factor `chol`), then row n = A d2 f / d beta d w_n."""
        if chol is None:
            raise ValueError('obs_influence needs the factor of the Hessian at x (ParametricSensitivityLinearApproximation holds it)')
        self._push_state()
        M = np.atleast_2d(_hip.as_f64(moment_jac))
        if M.shape[1] != self.D:
            raise ValueError('moment Jacobian must have {} columns'.format(self.D))
        S = chol.solve(np.ascontiguousarray(M.T))
        S = np.asarray(S).reshape(self.D, -1)
        jd = self._box_diag(x)[0] if is_free else np.ones(self.D)
        A = -(jd[:, None] * S).T
        return self.ctx.softmax_obs_influence(self._eta(x, is_free), self.K, A, n0=n0, n1=n1)

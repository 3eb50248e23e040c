"""Ordinal mixed model with a cumulative logit link and K <= 4 independent random effects per group: an
ordered categorical response -- Likert items, severity grades, ratings -- `ordinal::clmm`, `MASS::polr` plus random effects,
`brms(family = cumulative)`:

    y_n in {0 .. J - 1},   P(y_n <= j | t_n) = sigma(alpha_{j+1} - t_n),   t_n = o_n + x_n . beta + z_n . u_{g(n)},

with T = J - 1 cut points alpha_1 < .. < alpha_T, 2 <= J <= 16.  Priors, variational families, parameter layout, vector and free
coordinates, n_global = 2 P + 4 K and the coupled rows are those of `LogisticGLMMSlopesObjective` (glmm_slopes.py, DESIGN.md
section 18).  With -inf = alpha_0 and alpha_{T+1} = +inf, lo = alpha_y, hi = alpha_{y+1} and D = hi - lo the row's term is

    h(t) = -log[sigma(hi - t) - sigma(lo - t)] = softplus(t - hi) + softplus(lo - t) - log(1 - e^-D)

whole: nothing is dropped, `log_norm_const()` is 0.0 (the last term depends on the thresholds).  The difference of the two sigmoids
loses every digit in the right tail; the sum on the right has no cancellation anywhere, and a missing cut point of an end category is
a sentinel +-inf at which the logistic node expressions are exact zeros.  The data term is sum_n w_n E h(t), t ~ N(rho_n, s_n), on the
Gauss-Hermite nodes of the logistic model; J = 2 is that model with the offset o - alpha_1.

The thresholds are ONE declared hyper-parameter of T entries, `threshold_par`: alpha in vector coordinates, (alpha_1, gamma_1 ..
gamma_{T-1}) with alpha_{j+1} = alpha_j + e^{gamma_j} in free coordinates.  The device only sees alpha (T doubles per change, nothing of
length N); the chain rule to the free coordinates is host work.  `threshold_terms`, `threshold_sensitivity`, `threshold_profile` and
`fit_thresholds` (`_Thresholds` below) mirror the log-dispersion of DESIGN.md section 41 for a vector.  A common shift of all
thresholds is not identified against the mean of a random intercept, so estimation holds alpha_1 fixed by default.

`ordinal_expected_h`, `ordinal_row_derivs`, `ordinal_threshold_moments` and `ordinal_category_probs` are the host forms of what the
kernels compute per row (the policy OrdinalLik of csrc/k_glmm_walk.h, glmm_thr_rows_kernel of csrc/k_glmm_slopes.hip); none of them
needs a device.
"""
import numpy as np
from scipy.sparse import coo_matrix

from . import _hip
from .block_arrow import predict_rows
from .glmm_binomial import _logistic_nodes, _nodes, _row_vector
from .glmm_slopes import _LogisticMixedModel, _SlopesArrow
from .packing import HyperVectorParam, ResidentVector

MAX_THRESHOLDS = 15
LOG2 = 0.6931471805599453                                               # where -log(1 - e^-D) changes form (OrdinalLik::delta_term)


def _fourth(x):
    """softplus, sigma, sigma', sigma'', sigma''' at x from e = exp(-|x|), as LogisticLik::moments forms them; exact zeros at -inf."""
    sp, sg, g2, g3 = _logistic_nodes(x)
    return sp, sg, g2, g3, g2 * (1.0 - 6.0 * g2)


def _delta_term(D):
    """-log(1 - e^-D), D > 0: through log1p past log 2 (1 - e^-D rounds to 1 from D = 37 on); 0 at D = +inf."""
    D = np.asarray(D, dtype=np.float64)
    with np.errstate(divide='ignore'):
        return np.where(D > LOG2, -np.log1p(-np.exp(-D)), -np.log(-np.expm1(-np.minimum(D, LOG2))))


def _delta_derivs(D):
    """(r, c) = (1 / expm1(D), e^-D / expm1(-D)^2): minus the first and plus the second derivative of `_delta_term`; both 0 at +inf."""
    D = np.asarray(D, dtype=np.float64)
    with np.errstate(over='ignore'):
        dm = np.expm1(-D)
        return 1.0 / np.expm1(D), np.exp(-D) / (dm * dm)


def _bounds(lo, hi, rho):
    return np.broadcast_arrays(np.asarray(rho, dtype=np.float64), np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))


def ordinal_expected_h(rho, s, lo, hi, gh_x, gh_w, delta=None):
    """E h^(k), k = 0..4 (a 5 x ... array), t ~ N(rho, s), by the rule of the kernels: the logistic node expressions at t - hi and at
    lo - t (odd orders of the lo term negated), plus -log(1 - e^-D) in the value.  lo, hi: the row's two cut points on the scale of
    rho -- with an offset either rho includes it, or lo and hi are the folds alpha - o that the device stages; -inf / +inf on an end
    category.  delta: D where it should not be formed as hi - lo (the device takes it from the table of cut points, not from the
    folds).  The value of a row is w times row 0, a1 = w row 1, a2 = w row 2 / 2, c11 = w row 2, c12 = w row 3 / 2, c22 = w row 4 / 4."""
    rho, lo, hi = _bounds(lo, hi, rho)
    t, wk = _nodes(rho, np.broadcast_to(np.asarray(s, dtype=np.float64), rho.shape), gh_x, gh_w)
    with np.errstate(invalid='ignore', over='ignore'):
        ga, gb = _fourth(t - hi[..., None]), _fourth(lo[..., None] - t)
        e = [((a - b if k & 1 else a + b) * wk).sum(-1) for k, (a, b) in enumerate(zip(ga, gb))]
        e[0] = e[0] + _delta_term(hi - lo if delta is None else delta)
    return np.stack(e)


def ordinal_row_derivs(rho, s, lo, hi, gh_x, gh_w):
    """(a1', a2') per unit weight of the streamed influence rows: a1' = E h' (there is no "- y"), a2' = E h'' / 2."""
    e = ordinal_expected_h(rho, s, lo, hi, gh_x, gh_w)
    return e[1], 0.5 * e[2]


def ordinal_threshold_moments(rho, s, lo, hi, gh_x, gh_w, delta=None):
    """The nine per-row quantities of the threshold pass, per unit weight (a 9 x ... array), by the rule of glmm_thr_rows_kernel:
        0..3   d1_hi = -E sigma'(t - hi),  d2_hi = -E sigma''(t - hi) / 2,  d1_lo = -E sigma'(lo - t),  d2_lo = +E sigma''(lo - t) / 2
               (the derivatives in rho and in s of the two gradient entries below),
        4, 5   g_hi = -E sigma(t - hi) - r,   g_lo = E sigma(lo - t) + r,                 r = 1 / expm1(D),
        6..8   H_hi,hi = E sigma'(t - hi) + c,  H_lo,lo = E sigma'(lo - t) + c,  H_lo,hi = -c,   c = e^-D / expm1(-D)^2.
    An entry that belongs to a sentinel (hi of the last category, lo of the first) is an exact zero."""
    rho, lo, hi = _bounds(lo, hi, rho)
    t, wk = _nodes(rho, np.broadcast_to(np.asarray(s, dtype=np.float64), rho.shape), gh_x, gh_w)
    with np.errstate(invalid='ignore', over='ignore'):
        a = [(g * wk).sum(-1) for g in _logistic_nodes(t - hi[..., None])[1:]]
        b = [(g * wk).sum(-1) for g in _logistic_nodes(lo[..., None] - t)[1:]]
        r, c = _delta_derivs(hi - lo if delta is None else delta)
    return np.stack([-a[1], -0.5 * a[2], -b[1], 0.5 * b[2], -a[0] - r, b[0] + r, a[1] + c, b[1] + c, -c])


def ordinal_category_probs(rho, s, thresholds, gh_x, gh_w):
    """(cumprob: ... x T, prob: ... x J) with cumprob[.., j] = P(y <= j) = 1 - E sigma(t - alpha_{j+1}), t ~ N(rho, s) (rho including the
    offset), and prob the differences of [0, cumprob, 1]: the rows of prob sum to 1 by telescoping."""
    rho = np.asarray(rho, dtype=np.float64)
    al = np.asarray(thresholds, dtype=np.float64).ravel()
    t, wk = _nodes(rho[..., None] - al, np.asarray(s, dtype=np.float64)[..., None] + np.zeros(al.size), gh_x, gh_w)
    cum = 1.0 - (_logistic_nodes(t)[1] * wk).sum(-1)
    return cum, _probs_of(cum)


def _probs_of(cum):
    edge = np.concatenate([np.zeros(cum.shape[:-1] + (1,)), cum, np.ones(cum.shape[:-1] + (1,))], axis=-1)
    return np.diff(edge, axis=-1)


def check_thresholds(alpha):
    a = _hip.as_f64(alpha).ravel().copy()
    if not 1 <= a.size <= MAX_THRESHOLDS:
        raise ValueError('thresholds must hold 1 to {} values (2 to {} ordered categories), got {}'.format(MAX_THRESHOLDS, MAX_THRESHOLDS + 1, a.size))
    if not np.all(np.isfinite(a)) or np.any(np.diff(a) <= 0.0):
        raise ValueError('thresholds must be finite and strictly increasing')
    return a


class ThresholdParam(HyperVectorParam):
    """The T cut points as a hyper-parameter: alpha in vector coordinates, (alpha_1, gamma_1 .. gamma_{T-1}) with
    alpha_{j+1} = alpha_j + e^{gamma_j} in free coordinates, so that every free value is an increasing vector."""

    def __init__(self, name, val):
        val = check_thresholds(val)
        super().__init__(name, val.size, val=val)

    def set_free(self, free_val):
        f = np.asarray(free_val, dtype=np.float64).ravel()
        if f.size != self.size():
            raise ValueError('Wrong size for vector ' + self.name)
        self.set(f[0] + np.concatenate([[0.0], np.cumsum(np.exp(f[1:]))]))

    def get_free(self):
        a = np.asarray(self._val, dtype=np.float64)
        return np.concatenate([a[:1], np.log(np.diff(a))])

    def free_to_vector_jac(self, free_val):
        """d alpha / d free, T x T: a column of ones, and e^{gamma_i} in the rows below i."""
        f = np.asarray(free_val, dtype=np.float64).ravel()
        T = f.size
        A = np.zeros((T, T))
        A[:, 0] = 1.0
        for i in range(1, T):
            A[i:, i] = np.exp(f[i])
        return coo_matrix(A)

    def free_to_vector_hess(self, free_val):
        """d2 alpha_j / d free2, one T x T matrix per j: e^{gamma_i} at (i, i) for i <= j."""
        f = np.asarray(free_val, dtype=np.float64).ravel()
        T = f.size
        out = []
        for j in range(T):
            d = np.zeros(T)
            d[1:j + 1] = np.exp(f[1:j + 1])
            out.append(coo_matrix(np.diag(d)))
        return out


class _Thresholds:
    """The cut points of an ordinal mixed model as an estimated VECTOR hyper-parameter, the sibling of
    `_LogDispersion` for T entries: `threshold_par` holds alpha, and the objective that depends on it is F(theta, alpha) = value(theta)
    (nothing is dropped from the value; priors and KL terms do not depend on alpha).  A class lists this one FIRST among its bases."""

    def _declare_thresholds(self, alpha):
        self._declare_hyper('threshold', ThresholdParam('threshold', alpha))
        self._thr_res = ResidentVector()
        self._thr_res.changed(self.threshold_par)                           # the constructor sent these cut points already

    def _push_state(self):
        super()._push_state()
        res = self.__dict__.get('_thr_res')
        if res is None:                                                      # the base constructor's own push: nothing declared yet
            return
        a = res.changed(self.threshold_par)
        if a is not None:
            try:
                self._alpha = check_thresholds(a)
            except ValueError:
                res.key = res._val = None                                    # not resident: the next evaluation meets the same refusal
                raise
            self.ctx.set_thresholds(self._alpha)
            self._dev_factor_key = None                                      # the context dropped its sums and factor with the old cut points
            self._gcov = None

    thresholds = property(lambda self: self._hyper_vec('threshold').copy())

    # ---- derivatives in the thresholds --------------------------------------------------------------------------------------------
    def _threshold_jac(self):
        par = self.threshold_par
        f = par.get_free()
        return np.asarray(par.free_to_vector_jac(f).todense()), [np.asarray(h.todense()) for h in par.free_to_vector_hess(f)]

    @_hip.host_blas
    def threshold_terms(self, x, is_free=True, free_thresholds=False):
        """dict(g = F_alpha (T), H = F_alpha,alpha (T x T, tridiagonal in alpha), cross = d2 F / d theta d alpha (D x T)) at x, in the
        coordinates of x (free: chained through the packing as a gradient is; its mu and tau rows are zero) and in the vector
        coordinates alpha of `threshold_par`, or with free_thresholds=True in its free coordinates (alpha_1, gamma): A^T g,
        A^T H A + sum_j g_j d2 alpha_j and cross A with A = d alpha / d free.  One pass over the rows on the device
        (lrvb_glmm_ordinal_threshold_terms), which leaves the resident sums and factors of the context alone."""
        if self._external_stats is not None:
            raise ValueError('threshold_terms uses the rows resident on this device, not installed statistics')
        eta = self._eta(x, is_free)
        _, ib, _, _, _, _, e, ig = self._split(eta)
        self._push_state()
        P, K, G, ng = self.P, self.K, self.G, self.n_global
        GK, T = G * K, self.threshold_par.size()
        v, r = 1.0 / ib, 1.0 / ig
        g, hd, ho, cg, cl = self.ctx.glmm_ordinal_threshold_terms(eta[:P], v, e, r, self.gh_x, self.gh_w)
        H = np.diag(hd) + np.diag(ho, 1) + np.diag(ho, -1)
        J = np.zeros((ng + 2 * GK, T))
        J[:P], J[P:2 * P] = cg[:, :P].T, (cg[:, P:] * (-v * v)).T
        J[ng:ng + GK] = cl[:, :, :K].transpose(0, 2, 1).reshape(GK, T)
        J[ng + GK:] = (cl[:, :, K:].transpose(0, 2, 1) * (-r * r)[:, :, None]).reshape(GK, T)
        if is_free:
            J = np.stack([self._grad_to_free(J[:, j], eta) for j in range(T)], axis=1)
        if free_thresholds:
            A, A2 = self._threshold_jac()
            H = A.T @ H @ A + sum(gj * hj for gj, hj in zip(g, A2))
            g, J = A.T @ g, J @ A
        return dict(g=g, H=H, cross=J)

    def threshold_sensitivity(self, x, moment_jac=None, is_free=True, on_device=False):
        """d theta / d alpha = -H^-1 J at a fitted x: T right-hand sides through `solve` (on_device as there), D x T; with a moment
        Jacobian M (Q x D or Q x n_global) the Q x T matrix M d theta / d alpha."""
        J = self.threshold_terms(x, is_free)['cross']
        dth = -np.asarray(self.solve(x, J, is_free, on_device=on_device))
        return dth if moment_jac is None else self._moment_jac(moment_jac) @ dth

    def _estimated(self, fix_first):
        return slice(1, None) if fix_first else slice(None)

    def threshold_profile(self, x, is_free=True, on_device=False, fix_first=True):
        """(slope, S): gradient and Hessian S = F_ff - J^T H^-1 J of the PROFILED objective min_theta F(theta, alpha) at a fitted x, in
        the estimated free coordinates of `threshold_par` -- (gamma_1 .. gamma_{T-1}), or with fix_first=False (alpha_1, gamma)."""
        t = self.threshold_terms(x, is_free, free_thresholds=True)
        sel = self._estimated(fix_first)
        J = t['cross'][:, sel]
        if J.shape[1] == 0:
            return np.zeros(0), np.zeros((0, 0))
        return t['g'][sel], t['H'][sel, sel] - J.T @ np.asarray(self.solve(x, J, is_free, on_device=on_device))

    def fit_thresholds(self, fit, theta0, fix_first=True, max_iter=20, tol=1e-8):
        """Profile Newton on the estimated free coordinates of the thresholds (alpha_1 held fixed unless fix_first=False: a common
        shift is not identified against the mean of a random intercept, so fix_first=False is for a `z` without a constant column).
        fit(fun, theta_start) -> theta is the caller's optimiser of theta at the current thresholds (free coordinates).  Each step is
        -S^-1 slope, scaled back to 1 in the max norm; where S is not positive definite, a step of 0.5 against the sign of the
        slope.  The next inner fit starts at theta + d theta.  Stops when max |step| <= tol or max |slope| <= tol (max |F_ff| + 1).
        Returns dict(thresholds, theta, slope, curvature, iterations), slope and curvature (S) being those at the returned point;
        `threshold_par` holds the thresholds."""
        par = self.threshold_par
        sel = self._estimated(fix_first)
        theta = np.asarray(fit(self, _hip.as_f64(theta0).ravel()), dtype=np.float64).ravel()
        it = 0
        while True:
            t = self.threshold_terms(theta, True, free_thresholds=True)
            g, Hf, J = t['g'][sel], t['H'][sel, sel], t['cross'][:, sel]
            if g.size == 0:
                return dict(thresholds=self.thresholds, theta=theta, slope=g, curvature=Hf, iterations=0)
            dth = -np.asarray(self.solve(theta, J, True))
            S = Hf + J.T @ dth
            if it >= max_iter or np.max(np.abs(g)) <= tol * (np.max(np.abs(Hf)) + 1.0):
                break
            try:
                np.linalg.cholesky(S)
                step = -np.linalg.solve(S, g)
            except np.linalg.LinAlgError:
                step = -0.5 * np.sign(g)
            step = step / max(1.0, float(np.max(np.abs(step))))
            if np.max(np.abs(step)) <= tol:
                break
            f = np.array(par.get_free(), dtype=np.float64)
            f[sel] += step
            par.set_free(f)
            theta = np.asarray(fit(self, theta + dth @ step), dtype=np.float64).ravel()
            it += 1
        return dict(thresholds=self.thresholds, theta=theta, slope=g, curvature=S, iterations=it)

    # ---- the hyper-parameter protocol -----------------------------------------------------------------------------------------
    def hyper_grad(self, hyper_par, val1, val1_is_free):
        """threshold: d value / d alpha (T)."""
        if self.hyper_kind(hyper_par) != 'threshold':
            return super().hyper_grad(hyper_par, val1, val1_is_free)
        return self.threshold_terms(val1, val1_is_free)['g']

    def cross_hessian(self, hyper_par, val1, val1_is_free):
        """threshold: the D x T block d2 F / d theta d alpha.  Its local rows are NOT zero, as the weights' are not."""
        if self.hyper_kind(hyper_par) != 'threshold':
            return super().cross_hessian(hyper_par, val1, val1_is_free)
        return self.threshold_terms(val1, val1_is_free)['cross']

    def global_cross_hessian(self, hyper_par, val, is_free=True):
        if self.hyper_kind(hyper_par) == 'threshold':
            raise NotImplementedError('the threshold cross Hessian has local rows: use cross_hessian or threshold_sensitivity')
        return super().global_cross_hessian(hyper_par, val, is_free)

    def global_sensitivity(self, hyper_par, free_val):
        if self.hyper_kind(hyper_par) == 'threshold':
            raise NotImplementedError('the threshold cross Hessian has local rows: use threshold_sensitivity')
        return super().global_sensitivity(hyper_par, free_val)


class OrdinalGLMMObjective(_Thresholds, _SlopesArrow, _LogisticMixedModel):
    _loss = 'logistic'
    _minus_y = False

    def __init__(self, par, x, y, z, groups, n_groups, thresholds, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0),
                 tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: the categories, integers 0 .. J - 1 with J = len(thresholds) + 1 (a category that no row has is fine).  thresholds: the
        T = J - 1 strictly increasing finite start values of the cut points, 1 <= T <= 15; `threshold_par` holds them afterwards.
        z: the N x K group design, or None for one effect per group with the unit design.  offset: the N offsets o_n, or None for
        zero.  `value` is the whole -ELBO: `log_norm_const()` is 0.0.  All checks run before the device context is created."""
        alpha = check_thresholds(thresholds)
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n:
            raise ValueError('y must hold {} values'.format(n))
        if not np.all(np.isfinite(y)) or np.any(y != np.round(y)):
            raise ValueError('y must hold integer categories: {} of {} rows do not'.format(int(np.count_nonzero(~(y == np.round(y)))), n))
        if np.any(y < 0) or np.any(y > alpha.size):
            raise ValueError('y must lie in 0 .. {} ({} thresholds make {} categories): found {} .. {}'.format(
                alpha.size, alpha.size, alpha.size + 1, int(y.min()), int(y.max())))
        if offset is not None:
            offset = _row_vector(offset, n, 'offset')
        if z is None:
            z = np.ones((n, 1))
        super().__init__(par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)
        self._offset, self._alpha = offset, alpha
        self._cat = y.astype(np.int64)
        self.ctx.set_offset(offset)
        self.ctx.set_thresholds(alpha)
        self._declare_thresholds(alpha)

    n_categories = property(lambda self: self.threshold_par.size() + 1)

    # ---- the device entries -------------------------------------------------------------------------------------------------
    def _terms(self, *point, **want):
        return self.ctx.glmm_ordinal_terms(*point, **want)

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_ordinal_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_ordinal_group_influence(*point_and_operand)

    def row_bounds(self):
        """(lo - o, hi - o, D) per row at the current thresholds: the two folds the device stages and D = hi - lo from the table."""
        tab = np.concatenate([[-np.inf], self.thresholds, [np.inf]])
        o = 0.0 if self._offset is None else self._offset
        with np.errstate(invalid='ignore'):
            return tab[self._cat] - o, tab[self._cat + 1] - o, tab[self._cat + 1] - tab[self._cat]

    def _row_psi_derivs(self, rho, s):
        """(E h', E h'' / 2) by the rule the kernels use: a1' whole (`_minus_y` is False, the category is no response to subtract)."""
        lo, hi, _ = self.row_bounds()
        return ordinal_row_derivs(rho, s, lo, hi, self.gh_x, self.gh_w)

    def log_norm_const(self):
        """0.0: the value drops nothing (the term -log(1 - e^-D) depends on the thresholds and stays in it)."""
        return 0.0

    # ---- predictions: P(y <= j) = 1 - E sigma(t - alpha_{j+1}) is the binomial logit entry at the offset o - alpha_{j+1}, one trial ----
    def _predict_rows_of(self, newdata, n0, n1):
        if newdata is not None:
            for key in ('trials', 'thresholds'):
                if key in newdata:
                    raise ValueError('newdata has the keys x, z, groups, offset (got {}): the category probabilities are predicted at '
                                     'the thresholds of the model, and a row has no trials'.format(key))
        return super()._predict_rows_of(newdata, n0, n1)

    @_hip.host_blas
    def predict(self, x, newdata=None, n0=0, n1=None, is_free=True, on_device=False):
        """Fitted values (newdata=None: rows n0..n1 of the model's data) or predictions for new rows
        `newdata = dict(x=, z=, groups=, offset=)` (groups may hold -1: the population level), as a dict:

            rho, var_mf, var_lrvb        the linear predictor o + x . m + z . e_g and its two variances, as every mixed model returns them
            cumprob_mf, cumprob_lrvb     rows x T, P(y <= j) = 1 - E sigma(t - alpha_{j+1}), t ~ N(rho, var), under either variance
            prob_mf, prob_lrvb           rows x J, the differences of [0, cumprob, 1]: every row sums to 1

        on_device=True: the rows go to the binomial logit predict entry as NEW rows, once per threshold at the offset o - alpha_j
        with one trial (and once at o for rho): no kernel of its own, and the resident state of the model is not touched."""
        rows = self._predict_rows_of(newdata, n0, n1)
        xr, zr, gid, off = rows[:4]
        cb, cu, cbu = self._group_cov(x, is_free, on_device)
        eta = self._eta(x, True)
        m, ib, e_mu, i_mu, _, _, e, ig = self._split(eta)
        v, e2, r2 = 1.0 / ib, np.vstack([e, e_mu[None, :]]), np.vstack([1.0 / ig, 1.0 / i_mu[None, :]])
        alpha = self.thresholds
        if on_device:
            o = np.zeros(np.shape(xr)[0]) if off is None else off
            point = (m, v, e2, r2, self.gh_x, self.gh_w)
            rho, s_mf, v_lr = self.ctx.glmm_binomial_predict(*point, cb, new=(xr, zr, gid, o, None))[:3]
            surv = [self.ctx.glmm_binomial_predict(*point, cb, new=(xr, zr, gid, o - a, None))[3:5] for a in alpha]
            cum_mf, cum_lr = (1.0 - np.stack([sv[i] for sv in surv], axis=1) for i in (0, 1))
        else:
            rho, s_mf, v_lr = predict_rows(xr, zr, gid, off, m, v, e2, r2, cb, cu, cbu)
            cum_mf = ordinal_category_probs(rho, s_mf, alpha, self.gh_x, self.gh_w)[0]
            cum_lr = ordinal_category_probs(rho, v_lr, alpha, self.gh_x, self.gh_w)[0]
        return dict(rho=rho, var_mf=s_mf, var_lrvb=v_lr, cumprob_mf=cum_mf, cumprob_lrvb=cum_lr, prob_mf=_probs_of(cum_mf),
                    prob_lrvb=_probs_of(cum_lr))

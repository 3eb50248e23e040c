"""Binomial and negative-binomial mixed models with K <= 4 independent random effects per group:

    y_n ~ Binomial(m_n, sigma(o_n + x_n . beta + z_n . u_{g(n)})),   z_n in R^K,   u_gk ~ N(mu_k, 1 / tau_k) independently over k

with a trial count m_n and an offset o_n per row -- the `cbind(successes, failures)` form of aggregated binary data; m = 1, o = 0
is `LogisticGLMMSlopesObjective`.  Priors, variational families, parameter layout, vector and free coordinates, n_global = 2 P + 4 K
and the coupled rows are that class's (glmm_slopes.py).  Only the data term differs:

    sum_n w_n [ m_n psi(rho_n, s_n) - y_n rho_n ],   rho_n = o_n + x_n . m + z_n . e_g,   s_n = (x_n o x_n) . v + (z_n o z_n) . r_g,
    psi = E softplus(t),  t ~ N(rho_n, s_n)          -- the Gauss-Hermite rule and Stein-rule derivatives of the logistic model.

The constant sum_n w_n log C(m_n, y_n) of the binomial log-likelihood does not depend on the parameters and is DROPPED from the
value.

Negative binomial (NB2: mean e^eta, variance e^eta + e^2eta / phi, KNOWN dispersion phi): the parameter-dependent part of -log p is
(y + phi) softplus(eta - log phi) - y (eta - log phi), i.e. the binomial term with "trials" y + phi (real, not integer) and the
offset o - log phi.  `NegBinomialGLMMObjective` is that construction; its phi is phi0 e^lambda with the constructor's phi0 and ONE
declared hyper-parameter lambda = `log_dispersion_par` (0 at construction), which `fit_dispersion` estimates and whose linear
response `dispersion_sensitivity` gives (`_LogDispersion` below).

Links: `link='probit'` (p = Phi(t)) and `link='cloglog'` (p = 1 - exp(-e^t)) replace the data term by

    sum_n w_n E [ y_n h1(t) + (m_n - y_n) h0(t) ],   h1 = -log p,  h0 = -log(1 - p),  t ~ N(rho_n, s_n)

on the same nodes (cloglog: E h0 = exp(rho + s / 2) in closed form).  `link_h`, `link_row_derivs` and `link_response_mean` below are
the host forms of what the kernels compute per node and per row; they need no device.

The O(N) work is `lrvb_glmm_binomial_terms` (csrc/k_glmm_slopes.hip, the policy BinomialLik of csrc/k_glmm_walk.h); everything
after the per-row coefficients is the shared layer, unchanged.
"""
import numpy as np
from scipy.special import erfc, erfcx, expit, gammaln, ndtr

from . import _hip
from .glmm_slopes import _LogisticMixedModel, _SlopesArrow


def _row_vector(a, n, what):
    a = _hip.as_f64(a).ravel().copy()
    if a.size != n or not np.all(np.isfinite(a)):
        raise ValueError('{} must hold {} finite values'.format(what, n))
    return a


LINKS = {'logit': 0, 'probit': 1, 'cloglog': 2}                         # LRVB_LINK_* of the C ABI
PROBIT_CF_BELOW, PROBIT_CF_TERMS = -5.0, 24                           # BinomialLinkLik<PROBIT>::h1: the continued fraction of t + lambda
LOG2 = 0.6931471805599453                                               # where the cloglog value changes form (BinomialLinkLik::h1)


def _h1_probit(t, order):
    """-log Phi(t) and its derivatives through the inverse Mills ratio lambda = sqrt(2 / pi) / erfcx(-t / sqrt 2)."""
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        ex = erfcx(-t / np.sqrt(2.0))
        lam = np.sqrt(2.0 / np.pi) / ex
        d = t + lam
        # Below t = PROBIT_CF_BELOW, d = t + lambda cancels to -1 / t and carries t^2 times the error of erfcx.  There it comes from the
        # continued fraction sqrt(2 / pi) / erfcx(x) = sqrt 2 (x + K(x)), K = (1/2) / (x + (2/2) / (x + (3/2) / (x + ..))), x = -t / sqrt 2:
        # d = sqrt 2 K(x) with no cancellation, lambda = d - t.  PROBIT_CF_TERMS terms (5e-16 of K at x = 3.5), evaluated from the tail
        # as one ratio N / D; past x = 1e8, where D would overflow, K = 1 / (2 x) to the last bit.
        far = t < PROBIT_CF_BELOW
        x0 = -0.7071067811865476 * t
        x = np.where(far, np.minimum(x0, 1e8), 6.0)
        N, D = np.full_like(x, 0.5 * PROBIT_CF_TERMS), x.copy()
        for k in range(PROBIT_CF_TERMS - 1, 0, -1):
            N, D = 0.5 * k * D, x * D + N
        d = np.where(far, 1.4142135623730951 * np.where(x0 > 1e8, 0.5 / np.where(far, x0, 1.0), N / D), d)
        lam = np.where(far, d - t, lam)
        w = lam * d
        w1 = lam * (1.0 - w) - w * d
        h = [np.where(t < 0.0, 0.5 * t * t - np.log(0.5 * ex), -np.log1p(-0.5 * erfc(np.maximum(t, 0.0) / np.sqrt(2.0)))),
             -lam, w, w1, -w1 * (d + lam) - 2.0 * w * (1.0 - w)]
    return h[:order + 1]


def _h1_cloglog(t, order):
    """-log(1 - exp(-u)), u = e^t, and its derivatives in t through r = u / expm1(u): r' = r (1 - u - r).  The value is
    -log(-expm1(-u)) up to u = log 2 and -log1p(-exp(-u)) past it: 1 - e^-u rounds to 1 from u = 37 on, and -log of it loses e^-u."""
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        u = np.exp(t)
        uc = np.minimum(u, 700.0)
        r = np.where(u > 700.0, 0.0, uc / np.expm1(uc))
        q = 1.0 - uc - r
        r1 = r * q
        q1 = -uc - r1
        r2 = r1 * q + r * q1
        q2 = -uc - r2
        h = [np.where(u > LOG2, -np.log1p(-np.exp(-u)), -np.log(-np.expm1(-np.minimum(u, LOG2)))), -r, -r1, -r2,
             -(r2 * q + 2.0 * r1 * q1 + r * q2)]
    return h[:order + 1]


def link_h(link, t, order=4):
    """([h1, h1', .., h1^(order)], [h0, .., h0^(order)]) at t, order <= 4: the per-trial terms h1 = -log p, h0 = -log(1 - p) of
    the probit or cloglog link by the formulas of the kernels (k_glmm_walk.h, BinomialLinkLik)."""
    t = np.asarray(t, dtype=np.float64)
    if link == 'probit':
        h0 = _h1_probit(-t, order)
        return _h1_probit(t, order), [(-a if k & 1 else a) for k, a in enumerate(h0)]
    if link == 'cloglog':
        return _h1_cloglog(t, order), [np.exp(t)] * (order + 1)
    raise ValueError("link_h: link must be 'probit' or 'cloglog'")


def _nodes(rho, s, gh_x, gh_w):
    rho, s = np.asarray(rho, dtype=np.float64), np.asarray(s, dtype=np.float64)
    t = rho[..., None] + np.sqrt(np.maximum(s, 0.0))[..., None] * (np.sqrt(2.0) * np.asarray(gh_x, dtype=np.float64))
    return t, np.asarray(gh_w, dtype=np.float64) / np.sqrt(np.pi)


def link_expected_h(link, rho, s, y, trials, gh_x, gh_w):
    """E H^(k), k = 0..4, H = y h1 + (trials - y) h0, t ~ N(rho, s) (rho including the offset) by the kernels' rule: h1 on the
    nodes, probit h0 on the nodes at -t, cloglog h0 = exp(rho + s / 2) in closed form.  A 5 x ... array."""
    t, wk = _nodes(rho, s, gh_x, gh_w)
    h1, h0 = link_h(link, t, 4)
    y, f = np.asarray(y, dtype=np.float64), np.asarray(trials, dtype=np.float64) - np.asarray(y, dtype=np.float64)
    e1 = np.stack([(a * wk).sum(-1) for a in h1])
    if link == 'cloglog':
        with np.errstate(over='ignore'):
            e0 = np.stack([np.exp(np.asarray(rho, dtype=np.float64) + 0.5 * np.asarray(s, dtype=np.float64))] * 5)
    else:
        e0 = np.stack([(a * wk).sum(-1) for a in h0])
    with np.errstate(invalid='ignore'):
        return y * e1 + f * e0


def link_row_derivs(link, rho, s, y, trials, gh_x, gh_w):
    """(a1', a2') per unit weight of the streamed influence rows: a1' = E H' (there is no "- y"), a2' = E H'' / 2."""
    e = link_expected_h(link, rho, s, y, trials, gh_x, gh_w)
    return e[1], 0.5 * e[2]


def link_response_mean(link, rho, s, trials, gh_x, gh_w):
    """trials E p(t), t ~ N(rho, s): probit in closed form, Phi(rho / sqrt(1 + s)); cloglog on the nodes, E [-expm1(-e^t)]."""
    if link == 'probit':
        p = ndtr(np.asarray(rho, dtype=np.float64) / np.sqrt(1.0 + np.maximum(np.asarray(s, dtype=np.float64), 0.0)))
    elif link == 'cloglog':
        t, wk = _nodes(rho, s, gh_x, gh_w)
        with np.errstate(over='ignore'):
            p = (-np.expm1(-np.exp(t)) * wk).sum(-1)
    else:
        raise ValueError("link_response_mean: link must be 'probit' or 'cloglog'")
    return p if trials is None else np.asarray(trials, dtype=np.float64) * p


# ---- the NB2 term differentiated in the log-dispersion (the policy NegBinDispLik of csrc/k_glmm_walk.h) ------
def negbin_h_dispersion(t, phi, y):
    """[h_l, d_t h_l, d_t^2 h_l, h_ll] at the linear predictor t (eta = t - log phi is formed here): the NB2 row term
    h = (y + phi) softplus(eta) - y eta differentiated in lambda, phi = e^lambda phi0, at fixed t (d/d lambda = phi d/d phi), by
    the formulas of the kernels:  h_l = phi sp - m sg + y,  h_ll = phi sp - 2 phi sg + m sg',  d_t h_l = phi sg - m sg',
    d_t^2 h_l = phi sg' - m sg'',  m = y + phi, sp, sg, sg', sg'' the softplus, the sigmoid and its derivatives at eta."""
    t, phi, y = np.broadcast_arrays(np.asarray(t, dtype=np.float64), np.asarray(phi, dtype=np.float64), np.asarray(y, dtype=np.float64))
    sp, sg, g2, g3 = _logistic_nodes(t - np.log(phi))
    m = y + phi
    return [(phi * sp - m * sg) + y, phi * sg - m * g2, phi * g2 - m * g3, phi * (sp - 2.0 * sg) + m * g2]


def _logistic_nodes(eta):
    """softplus, sigmoid, sigmoid', sigmoid'' at eta from e = exp(-|eta|), as LogisticLik::moments forms them."""
    e = np.exp(-np.abs(eta))
    ie = 1.0 / (1.0 + e)
    pos = eta >= 0.0
    g2 = e * ie * ie
    om = (1.0 - e) * ie
    return np.maximum(eta, 0.0) + np.log1p(e), np.where(pos, ie, e * ie), g2, np.where(pos, -g2 * om, g2 * om)


def negbin_expected_h_dispersion(rho, s, y, phi, gh_x, gh_w):
    """(E h_l, E d_t h_l, E d_t^2 h_l, E h_ll), a 4 x ... array, t ~ N(rho, s) with rho including the RAW offset o: the E sums of
    softplus, sigmoid, sigmoid', sigmoid'' over the Gauss-Hermite nodes at rho - log phi, combined with phi, y + phi and y behind
    the sums as the kernel combines them.  d1 = w times row 1 and d2 = w times row 2 / 2 are the coefficient rows of the device."""
    rho, phi, y = np.asarray(rho, dtype=np.float64), np.asarray(phi, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t, wk = _nodes(rho - np.log(phi), s, gh_x, gh_w)
    v, e1, e2, e3 = [(a * wk).sum(-1) for a in _logistic_nodes(t)]
    m = y + phi
    return np.stack([(phi * v - m * e1) + y, phi * e1 - m * e2, phi * e2 - m * e3, phi * (v - 2.0 * e1) + m * e2])


NEGBIN_SUM_BELOW = 256      # integer counts below this: psi(y + phi) - psi(phi) as the finite sum of 1 / (phi + j)
NEGBIN_SERIES_FROM = 10.0   # phi from here on: the difference of the two asymptotic series, term by term


def digamma_difference(y, phi):
    """(psi(y + phi) - psi(phi), psi'(y + phi) - psi'(phi)) without the cancellation of the plain difference, which at phi >> y
    keeps only eps phi / y of its digits.  Integer y < NEGBIN_SUM_BELOW: sum_{j<y} 1 / (phi + j) and -sum_{j<y} 1 / (phi + j)^2,
    every term of one sign.  Otherwise, for phi >= NEGBIN_SERIES_FROM, the two Stirling series subtracted TERM BY TERM with
    u = log1p(y / phi):  u + y / (2 phi (phi + y)) - sum_k B_2k / (2k) phi^-2k expm1(-2k u)  and its analogue for psi' (to B_16: the
    first term left out is below 1e-17).  What is left (phi < 10 and a non-integer or large y) has y / phi large enough for
    `scipy.special` differences to keep their digits."""
    from scipy.special import digamma, polygamma
    y, phi = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    d0, d1 = np.zeros(y.shape), np.zeros(y.shape)
    small = (y == np.round(y)) & (y < NEGBIN_SUM_BELOW)
    if np.any(small):
        ys, ps = y[small], phi[small]
        a0, a1 = np.zeros(ys.shape), np.zeros(ys.shape)
        for j in range(int(ys.max()) - 1, -1, -1):                          # the small terms first
            r = np.where(j < ys, 1.0 / (ps + j), 0.0)
            a0 += r; a1 -= r * r
        d0[small], d1[small] = a0, a1
    series = ~small & (phi >= NEGBIN_SERIES_FROM)
    if np.any(series):
        ys, ps = y[series], phi[series]
        u = np.log1p(ys / ps)
        w2 = 1.0 / (ps * ps)
        k = np.arange(1, 9)
        b = np.array((1.0 / 6.0, -1.0 / 30.0, 1.0 / 42.0, -1.0 / 30.0, 5.0 / 66.0, -691.0 / 2730.0, 7.0 / 6.0, -3617.0 / 510.0))
        t0, t1 = np.zeros(ys.shape), np.zeros(ys.shape)
        for kk, bk in zip(k[::-1], b[::-1]):
            t0 += bk / (2.0 * kk) * w2 ** kk * np.expm1(-2.0 * kk * u)
            t1 += bk * w2 ** kk / ps * np.expm1(-(2.0 * kk + 1.0) * u)
        q = ys / (ps * (ps + ys))
        d0[series] = u + 0.5 * q - t0
        # psi'(x) = 1 / x + 1 / (2 x^2) + sum_k B_2k x^-(2k+1):  1 / (phi + y) - 1 / phi = -q,  (phi + y)^-2 - phi^-2 = phi^-2 expm1(-2 u)
        d1[series] = -q + 0.5 * w2 * np.expm1(-2.0 * u) + t1
    rest = ~small & ~series
    if np.any(rest):
        ys, ps = y[rest], phi[rest]
        d0[rest], d1[rest] = digamma(ys + ps) - digamma(ps), polygamma(1, ys + ps) - polygamma(1, ps)
    return d0, d1


class _LogDispersion:
    """The dispersion of a mixed model as an estimated hyper-parameter: phi_n = e^lambda phi0_n with ONE
    scalar lambda = `log_dispersion_par` (0 at construction: phi is the constructor's phi0 exactly, and nothing is pushed that was
    not pushed before).  The objective that depends on lambda is F(theta, lambda) = value(theta) - log_norm_const(); priors and KL
    terms do not.  A class gives `_push_dispersion(phi)` (what the device context is told), `_dispersion_entry(point)` (its
    lrvb_glmm_*_dispersion_terms entry) and `log_norm_const_dispersion()`; it lists this class FIRST among its bases."""

    def _declare_dispersion(self, phi0):
        from .packing import HyperVectorParam, ResidentVector
        self._phi0 = np.array(phi0, dtype=np.float64)
        self._declare_hyper('log_dispersion', HyperVectorParam('log_dispersion', 1, val=np.zeros(1)))
        self._lam_res = ResidentVector()
        self._lam_res.changed(self.log_dispersion_par)                      # phi0 itself is on the device already

    def _push_state(self):
        super()._push_state()
        res = self.__dict__.get('_lam_res')
        if res is None:                                                      # the base constructor's own push: phi0 is not declared yet
            return
        lam = res.changed(self.log_dispersion_par)
        if lam is not None:
            lam = float(np.asarray(lam, dtype=np.float64).ravel()[0])
            if not np.isfinite(lam):
                raise ValueError('log_dispersion must be finite')
            self._phi = self._phi0.copy() if lam == 0.0 else np.exp(lam) * self._phi0
            self._push_dispersion(self._phi)
            self._dev_factor_key = None                                      # the context dropped its sums and factor with the old phi
            self._gcov = None

    log_dispersion = property(lambda self: float(self._hyper_vec('log_dispersion')[0]))

    # ---- derivatives in lambda ------------------------------------------------------------------------------------------------
    @_hip.host_blas
    def dispersion_terms(self, x, is_free=True):
        """dict(d1 = F_lambda, d2 = F_lambda,lambda, cross = J_lambda) at x: the first and second derivative of
        F = value - log_norm_const() in lambda at fixed theta, and J_lambda = d2 F / d theta d lambda, a D-vector in the coordinates
        of x (free: chained through the packing as a gradient is; its mu and tau entries are zero).  One pass over the rows on the
        device (lrvb_glmm_*_dispersion_terms), which leaves the resident sums and factors of the context alone."""
        if self._external_stats is not None:
            raise ValueError('dispersion_terms uses the rows resident on this device, not installed statistics')
        eta = self._eta(x, is_free)
        _, ib, _, _, _, _, e, ig = self._split(eta)
        self._push_state()
        P, K, G, ng = self.P, self.K, self.G, self.n_global
        GK = G * K
        v, r = 1.0 / ib, 1.0 / ig
        d, cg, cl = self._dispersion_entry((eta[:P], v, e, r, self.gh_x, self.gh_w))
        J = np.zeros(ng + 2 * GK)
        J[:P], J[P:2 * P] = cg[:P], cg[P:] * (-v * v)
        J[ng:ng + GK], J[ng + GK:] = cl[:, :K].ravel(), (cl[:, K:] * (-r * r)).ravel()
        c1, c2 = self.log_norm_const_dispersion()
        return dict(d1=float(d[0]) - c1, d2=float(d[1]) - c2, cross=self._grad_to_free(J, eta) if is_free else J)

    def dispersion_sensitivity(self, x, moment_jac=None, is_free=True, on_device=False):
        """d theta / d lambda = -H^-1 J_lambda at a fitted x through `solve` (on_device as there), a D-vector; with a moment
        Jacobian M (Q x D or Q x n_global) the Q-vector M d theta / d lambda."""
        J = self.dispersion_terms(x, is_free)['cross']
        dth = -np.asarray(self.solve(x, J[:, None], is_free, on_device=on_device)).ravel()
        return dth if moment_jac is None else self._moment_jac(moment_jac) @ dth

    def dispersion_profile(self, x, is_free=True, on_device=False):
        """(F_lambda, F_lambda,lambda - J^T H^-1 J): slope and curvature in lambda of the PROFILED objective
        min_theta F(theta, lambda) at a fitted x."""
        t = self.dispersion_terms(x, is_free)
        J = t['cross']
        return t['d1'], t['d2'] - float(J @ np.asarray(self.solve(x, J[:, None], is_free, on_device=on_device)).ravel())

    def fit_dispersion(self, fit, theta0, max_iter=20, tol=1e-8):
        """Profile Newton on lambda.  fit(fun, theta_start) -> theta is the caller's optimiser of theta at the current lambda (free
        coordinates).  Each step is -slope / curvature of the profiled objective, |step| <= 1; where the curvature is not positive,
        a step of 0.5 against the slope.  The next inner fit starts at theta + step d theta / d lambda.  Stops when
        |step| <= tol or |slope| <= tol (|F_ll| + 1).  Returns dict(lam, phi_scale, theta, slope, curvature, iterations), slope
        and curvature being those at the returned (theta, lam); `log_dispersion_par` holds lam."""
        par = self.log_dispersion_par
        lam = self.log_dispersion
        theta = np.asarray(fit(self, _hip.as_f64(theta0).ravel()), dtype=np.float64).ravel()
        it = 0
        while True:
            t = self.dispersion_terms(theta, True)
            dth = -np.asarray(self.solve(theta, t['cross'][:, None], True)).ravel()
            slope, curv = t['d1'], t['d2'] + float(t['cross'] @ dth)
            if it >= max_iter or abs(slope) <= tol * (abs(t['d2']) + 1.0):
                break
            step = -slope / curv if curv > 0.0 else -0.5 * np.sign(slope)
            step = float(np.clip(step, -1.0, 1.0))
            if abs(step) <= tol:
                break
            lam += step
            par.set_vector(np.array([lam]))
            theta = np.asarray(fit(self, theta + step * dth), dtype=np.float64).ravel()
            it += 1
        return dict(lam=lam, phi_scale=float(np.exp(lam)), theta=theta, slope=slope, curvature=curv, iterations=it)

    # ---- the hyper-parameter protocol -----------------------------------------------------------------------------------------
    def hyper_grad(self, hyper_par, val1, val1_is_free):
        """log_dispersion: d value / d lambda, the data term alone (`value` drops log_norm_const; F_lambda is `dispersion_terms`)."""
        if self.hyper_kind(hyper_par) != 'log_dispersion':
            return super().hyper_grad(hyper_par, val1, val1_is_free)
        return np.array([self.dispersion_terms(val1, val1_is_free)['d1'] + self.log_norm_const_dispersion()[0]])

    def cross_hessian(self, hyper_par, val1, val1_is_free):
        """log_dispersion: the D x 1 column J_lambda.  Its local rows are NOT zero, as the weights' are not."""
        if self.hyper_kind(hyper_par) != 'log_dispersion':
            return super().cross_hessian(hyper_par, val1, val1_is_free)
        return self.dispersion_terms(val1, val1_is_free)['cross'][:, None]

    def global_cross_hessian(self, hyper_par, val, is_free=True):
        if self.hyper_kind(hyper_par) == 'log_dispersion':
            raise NotImplementedError('the log-dispersion cross Hessian has local rows: use cross_hessian or dispersion_sensitivity')
        return super().global_cross_hessian(hyper_par, val, is_free)

    def global_sensitivity(self, hyper_par, free_val):
        if self.hyper_kind(hyper_par) == 'log_dispersion':
            raise NotImplementedError('the log-dispersion cross Hessian has local rows: use dispersion_sensitivity')
        return super().global_sensitivity(hyper_par, free_val)


class BinomialGLMMObjective(_SlopesArrow, _LogisticMixedModel):
    _loss = 'logistic'

    def __init__(self, par, x, y, z, groups, n_groups, trials=None, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0),
                 tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0, link='logit'):
        """y: successes, 0 <= y_n <= trials_n (log C(m, y) is dropped from the value).  trials: the N trial counts m_n >= 0 (real
        values are accepted: the negative-binomial subclass sends y + phi), or None for one trial per row.  offset: the N offsets
        o_n, or None for zero.  z: the N x K group design, or None for one effect per group with the unit design (a column of
        ones is sent).  names: as `LogisticGLMMSlopesObjective`.  link: 'logit' (the default), 'probit' or 'cloglog'.  All checks run
        before the device context is created."""
        if link not in LINKS:
            raise ValueError("link must be 'logit', 'probit' or 'cloglog' (got {!r})".format(link))
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n or not np.all(np.isfinite(y)):
            raise ValueError('y must hold {} finite values'.format(n))
        if trials is not None:
            trials = _row_vector(trials, n, 'trials')
            if np.any(trials < 0.0):
                raise ValueError('trials must be >= 0')
        if np.any(y < 0.0) or np.any(y > (1.0 if trials is None else trials)):
            raise ValueError('y must satisfy 0 <= y <= trials')
        if offset is not None:
            offset = _row_vector(offset, n, 'offset')
        if z is None:
            z = np.ones((n, 1))
        super().__init__(par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)
        self._trials, self._offset, self.link = trials, offset, link
        self.ctx.set_link(LINKS[link])
        self.ctx.set_trials(trials)
        self.ctx.set_offset(offset)

    # ---- the device entries -------------------------------------------------------------------------------------------------
    def _terms(self, *point, **want):
        return self.ctx.glmm_binomial_terms(*point, **want)

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_binomial_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_binomial_group_influence(*point_and_operand)

    def _predict_entry(self, point, cov_beta, window, rows):
        if window is not None:
            return self.ctx.glmm_binomial_predict(*point, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_binomial_predict(*point, cov_beta, new=rows)

    def _row_psi_derivs(self, rho, s):
        """The logistic derivatives at rho + o, times m, by the rule the kernels use (Stein's identity on the nodes:
        psi_rho = E sigma(t), psi_s = E sigma'(t) / 2), so that the dense weight cross Hessian is the derivative of the same
        function as the streamed rows.  N x nodes on the host: the dense protocol is the small-N one."""
        if self._offset is not None:
            rho = rho + self._offset
        if self.link != 'logit':
            # `cross_hessian` of the base class subtracts y from the first value; a1' of these links has no such term, so y is
            # ADDED here (met by what is returned, not by an override: (a1' + y) - y differs from a1' by an ulp of |y| at most)
            a1, a2 = link_row_derivs(self.link, rho, s, self._y, 1.0 if self._trials is None else self._trials, self.gh_x, self.gh_w)
            return a1 + self._y, a2
        t = rho[:, None] + np.sqrt(np.maximum(s, 0.0))[:, None] * (np.sqrt(2.0) * self.gh_x)[None, :]
        sg = expit(t)
        wk = self.gh_w / np.sqrt(np.pi)
        p_rho, p_s = (sg * wk).sum(1), 0.5 * (sg * (1.0 - sg) * wk).sum(1)
        return (p_rho, p_s) if self._trials is None else (self._trials * p_rho, self._trials * p_s)


    def _response_mean(self, rho, s, trials):
        if self.link == 'logit':
            return super()._response_mean(rho, s, trials)
        return link_response_mean(self.link, rho, s, trials, self.gh_x, self.gh_w)


class NegBinomialGLMMObjective(_LogDispersion, BinomialGLMMObjective):
    def __init__(self, par, x, y, z, groups, n_groups, dispersion, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0),
                 tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: counts (finite, >= 0).  dispersion: phi > 0, a scalar or N values -- Var y = mu + mu^2 / phi, so phi -> infinity is
        the Poisson model; it is phi0 of phi = e^lambda phi0, lambda = `log_dispersion_par` being 0 until it is set or estimated
        (`fit_dispersion`).  offset: the N log exposures, or None.  The model is the binomial one with
        trials y + phi and offset o - log phi; `value` is -ELBO up to the constant `log_norm_const()`."""
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n or not np.all(np.isfinite(y)) or np.any(y < 0.0):
            raise ValueError('y must hold {} finite counts >= 0'.format(n))
        phi = _hip.as_f64(dispersion).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        phi = np.full(n, phi[0]) if phi.size == 1 else phi.copy()
        o = np.zeros(n) if offset is None else _row_vector(offset, n, 'offset')
        super().__init__(par, x, y, z, groups, n_groups, y + phi, o - np.log(phi), beta_prior_info, mu_prior, tau_prior, gh_deg, names,
                         weights, device)
        self._phi = phi
        self._raw_offset = o
        self.ctx.set_dispersion(phi)                 # read by the dispersion entry alone: the binomial entries are unchanged by it
        self._declare_dispersion(phi)

    # ---- the dispersion as a hyper-parameter ---------------------------------------------------------------
    def _push_dispersion(self, phi):
        self._trials, self._offset = self._y + phi, self._raw_offset - np.log(phi)
        self.ctx.set_trials(self._trials)
        self.ctx.set_offset(self._offset)
        self.ctx.set_dispersion(phi)

    def _dispersion_entry(self, point):
        return self.ctx.glmm_negbin_dispersion_terms(*point)

    def log_norm_const_dispersion(self):
        """(C_lambda, C_lambda,lambda) of C = `log_norm_const()` at the current weights and dispersion:
        C_l = sum w phi [psi(y + phi) - psi(phi)], C_ll = C_l + sum w phi^2 [psi'(y + phi) - psi'(phi)], the two differences by
        `digamma_difference` (no digits lost at phi >> y)."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        d0, d1 = digamma_difference(self._y, self._phi)
        c1 = float(np.sum(w * self._phi * d0))
        return c1, c1 + float(np.sum(w * self._phi * self._phi * d1))

    # ---- predictions: the NB mean exp(o + rho + s / 2) is the Poisson policy's, at the RAW offset (the binomial e1 is not the NB mean) ----
    def _predict_offset(self):
        return self._raw_offset

    def _predict_rows_of(self, newdata, n0, n1):
        x, z, gid, off, _ = super()._predict_rows_of(newdata, n0, n1)
        return x, z, gid, off, None

    def _predict_entry(self, point, cov_beta, window, rows):
        """The rows go to the Poisson entry as new rows: the offset resident on the context is o - log phi."""
        m, v, e, r = point[:4]
        return self.ctx.glmm_poisson_predict(m, v, e, r, cov_beta, new=rows[:4])

    def _response_mean(self, rho, s, trials):
        return np.exp(rho + 0.5 * s)

    def log_norm_const(self):
        """C(y, phi) = sum_n w_n [log Gamma(y_n + phi_n) - log Gamma(phi_n) - log Gamma(y_n + 1)] at the current weights:
        -ELBO(phi) = value - C + KL terms that do not depend on phi, so two dispersions are compared by value - log_norm_const()."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        return float(np.sum(w * (gammaln(self._y + self._phi) - gammaln(self._phi) - gammaln(self._y + 1.0))))

"""Beta mixed model with K <= 4 independent random effects per group: continuous proportions strictly
inside (0, 1) -- rates, shares, cover fractions -- glmmTMB's `beta_family(link = "logit")`:

    y_n ~ Beta(mu_n phi_n, (1 - mu_n) phi_n),   mu_n = sigma(t_n),   t_n = o_n + x_n . beta + z_n . u_{g(n)}

with a precision phi_n = e^lambda phi0_n > 0 (phi0 a scalar or one value per row, Var y = mu (1 - mu) / (1 + phi)); lambda is ONE
declared hyper-parameter, `log_dispersion_par`, 0 at construction, estimated by `fit_dispersion`.
Priors, variational families, parameter layout, vector and free coordinates, n_global = 2 P + 4 K and the coupled rows are those of
`LogisticGLMMSlopesObjective` (glmm_slopes.py).  With l = logit(y) the row's term is, constants dropped,

    h(t) = lgamma(phi sigma(t)) + lgamma(phi sigma(-t)) - phi l sigma(t),
    -log p(y | t) = h(t) - [lgamma(phi) + (phi - 1) log(1 - y) - log y]

and the data term is sum_n w_n E h(t), t ~ N(rho_n, s_n); the bracket, summed with the weights, is `log_norm_const()`.  The
likelihood is not canonical (the response sits inside h), so there is no "- y rho" anywhere.

h is evaluated in the SHIFTED form lgamma(x) = lgamma(1 + x) - log x on both arguments,

    h(t) = softplus(t) + softplus(-t) - 2 log phi + G(mu),   G(mu) = lgamma(1 + phi mu) + lgamma(1 + phi (1 - mu)) - phi l mu

because the chain rule on lgamma(phi sigma(t)) itself loses every digit of h'', h''' and h'''' in the tails (psi^(j)(phi mu) grows
like (phi mu)^-(j+1) while mu'^j falls like mu^j).  G is smooth and its polygamma arguments are >= 1.  `beta_h`, `beta_expected_h`,
`beta_row_derivs` and `beta_response_mean` below are the host forms of what the kernels compute per node and per row (the policy
BetaLik of csrc/k_glmm_walk.h), `polygamma_ge1` the host mirror of its lgamma / polygamma evaluator; they need no device.

The O(N) work is `lrvb_glmm_beta_terms` (csrc/k_glmm_slopes.hip); everything after the per-row coefficients is the shared layer,
unchanged.  The fitted mean E sigma(t) does not depend on phi: predictions go through the binomial predict entry with one trial.
"""
import numpy as np
from scipy.special import digamma, gammaln, polygamma

from . import _hip
from .glmm_binomial import _LogDispersion, _nodes, _row_vector
from .glmm_slopes import _LogisticMixedModel, _SlopesArrow

# Stirling / Bernoulli series of BetaLik::polygamma at z >= 10, in w^2 = 1 / z^2, k = 1 .. 8
_B2K = (1.0 / 6.0, -1.0 / 30.0, 1.0 / 42.0, -1.0 / 30.0, 5.0 / 66.0, -691.0 / 2730.0, 7.0 / 6.0, -3617.0 / 510.0)
POLYGAMMA_SHIFT_TO, POLYGAMMA_SHIFT_STEPS = 10.0, 9


def _horner(c, w2):
    acc = np.zeros_like(w2) + c[-1]
    for a in c[-2::-1]:
        acc = a + w2 * acc
    return acc


def polygamma_ge1(x, order=4):
    """[lgamma(x), psi(x), psi'(x), psi''(x), psi'''(x)][:order + 1] at x >= 1 by the rule of the kernels: nine steps of the
    recurrence f(x) = f(x + 1) + .. wherever the argument is still below 10 (selects), then the asymptotic series to B_16."""
    z = np.array(x, dtype=np.float64, copy=True)
    prod, s = np.ones_like(z), [np.zeros_like(z) for _ in range(4)]
    for _ in range(POLYGAMMA_SHIFT_STEPS):
        lo = z < POLYGAMMA_SHIFT_TO
        r = np.where(lo, 1.0 / z, 0.0)
        r2 = r * r
        s[0] += r; s[1] += r2; s[2] += r2 * r; s[3] += r2 * r2
        prod *= np.where(lo, z, 1.0)
        z = np.where(lo, z + 1.0, z)
    w = 1.0 / z
    w2, lz = w * w, np.log(z)
    k = np.arange(1, 9)
    b = np.asarray(_B2K)
    out = [(z - 0.5) * lz - z + 0.9189385332046727 - np.log(prod) + w * _horner(b / (2 * k * (2 * k - 1)), w2),
           lz - 0.5 * w - s[0] - w2 * _horner(b / (2 * k), w2),
           s[1] + w * (1.0 + 0.5 * w + w2 * _horner(b, w2)),
           -2.0 * s[2] - w2 * (1.0 + w + w2 * _horner(b * (2 * k + 1), w2)),
           6.0 * s[3] + w2 * w * (2.0 + 3.0 * w + w2 * _horner(b * (2 * k + 1) * (2 * k + 2), w2))]
    return out[:order + 1]


def beta_h(t, phi, logit_y, order=4):
    """[h, h', .., h^(order)] at t, order <= 4: h(t) = lgamma(phi sigma(t)) + lgamma(phi sigma(-t)) - phi l sigma(t) and its
    derivatives in t by the formulas of the kernels (k_glmm_walk.h, BetaLik): the shifted form, Faa di Bruno on G."""
    t, phi, l = np.broadcast_arrays(np.asarray(t, dtype=np.float64), np.asarray(phi, dtype=np.float64),
                                    np.asarray(logit_y, dtype=np.float64))
    e = np.exp(-np.abs(t))
    ie = 1.0 / (1.0 + e)
    pos = t >= 0.0
    mu, nu = np.where(pos, ie, e * ie), np.where(pos, e * ie, ie)
    g2 = e * ie * ie
    om = (1.0 - e) * ie
    d = np.where(pos, -om, om)
    pa, pb = polygamma_ge1(1.0 + phi * mu), polygamma_ge1(1.0 + phi * nu)
    G1, G2 = phi * ((pa[1] - pb[1]) - l), phi * phi * (pa[2] + pb[2])
    p3 = phi * phi * phi
    G3, G4 = p3 * (pa[3] - pb[3]), p3 * phi * (pa[4] + pb[4])
    g3, g4 = g2 * d, g2 * (1.0 - 6.0 * g2)
    m1, m2, m3, m4 = g2, g2 * d, g4, g2 * d * (1.0 - 12.0 * g2)
    h = [np.abs(t) + 2.0 * np.log1p(e) + pa[0] + pb[0] - phi * l * mu - 2.0 * np.log(phi),
         -d + G1 * m1,
         2.0 * g2 + G2 * m1 * m1 + G1 * m2,
         2.0 * g3 + G3 * m1 * m1 * m1 + 3.0 * G2 * m1 * m2 + G1 * m3,
         2.0 * g4 + G4 * (m1 * m1) * (m1 * m1) + 6.0 * G3 * m1 * m1 * m2 + G2 * (3.0 * m2 * m2 + 4.0 * m1 * m3) + G1 * m4]
    return h[:order + 1]


def beta_expected_h(rho, s, logit_y, phi, gh_x, gh_w):
    """E h^(k), k = 0..4 (a 5 x ... array), t ~ N(rho, s) (rho including the offset), summed over the Gauss-Hermite nodes as the
    kernels do.  The value of a row is w times row 0, a1 = w times row 1 (there is no "- y")."""
    t, wk = _nodes(rho, s, gh_x, gh_w)
    phi, l = np.asarray(phi, dtype=np.float64), np.asarray(logit_y, dtype=np.float64)
    return np.stack([(a * wk).sum(-1) for a in beta_h(t, phi[..., None], l[..., None], 4)])


def beta_row_derivs(rho, s, logit_y, phi, gh_x, gh_w):
    """(a1', a2') per unit weight of the streamed influence rows: a1' = E h', a2' = E h'' / 2."""
    e = beta_expected_h(rho, s, logit_y, phi, gh_x, gh_w)
    return e[1], 0.5 * e[2]


def beta_response_mean(rho, s, gh_x, gh_w):
    """E sigma(t), t ~ N(rho, s): the mean of the proportion, the logistic one whatever phi, on the nodes as LogisticLik::infl."""
    t, wk = _nodes(rho, s, gh_x, gh_w)
    e = np.exp(-np.abs(t))
    ie = 1.0 / (1.0 + e)
    return (np.where(t >= 0.0, ie, e * ie) * wk).sum(-1)


def beta_h_dispersion(t, phi, logit_y):
    """[h_l, d_t h_l, d_t^2 h_l, h_ll] at t: the row term h of `beta_h` differentiated in lambda, phi = e^lambda phi0, at fixed t
    (d/d lambda = phi d/d phi), by the formulas of the kernels (k_glmm_walk.h, BetaDispLik) on the shifted form: with a = phi mu,
    b = phi (1 - mu), v = mu (1 - mu), d = 1 - 2 mu,
        h_l = a psi(1 + a) + b psi(1 + b) - l a - 2,   h_ll = h_l + 2 + a^2 psi'(1 + a) + b^2 psi'(1 + b),
        K1 = phi [psi(1 + a) + a psi'(1 + a) - psi(1 + b) - b psi'(1 + b) - l],
        K2 = phi^2 [2 psi'(1 + a) + a psi''(1 + a) + 2 psi'(1 + b) + b psi''(1 + b)],   d_t h_l = K1 v,   d_t^2 h_l = K2 v^2 + K1 v d."""
    t, phi, l = np.broadcast_arrays(np.asarray(t, dtype=np.float64), np.asarray(phi, dtype=np.float64),
                                    np.asarray(logit_y, dtype=np.float64))
    e = np.exp(-np.abs(t))
    ie = 1.0 / (1.0 + e)
    pos = t >= 0.0
    mu, nu = np.where(pos, ie, e * ie), np.where(pos, e * ie, ie)
    g2 = e * ie * ie
    om = (1.0 - e) * ie
    d = np.where(pos, -om, om)
    a, b = phi * mu, phi * nu
    pa, pb = polygamma_ge1(1.0 + a, 3), polygamma_ge1(1.0 + b, 3)
    first = a * pa[1] + b * pb[1] - l * a
    ta, tb = a * pa[2], b * pb[2]
    K1 = phi * (((pa[1] + ta) - (pb[1] + tb)) - l)
    K2 = phi * phi * ((2.0 * pa[2] + a * pa[3]) + (2.0 * pb[2] + b * pb[3]))
    K1v = K1 * g2
    return [first - 2.0, K1v, K2 * g2 * g2 + K1v * d, first + a * ta + b * tb]


def beta_expected_h_dispersion(rho, s, logit_y, phi, gh_x, gh_w):
    """(E h_l, E d_t h_l, E d_t^2 h_l, E h_ll), a 4 x ... array, t ~ N(rho, s) (rho including the offset), summed over the
    Gauss-Hermite nodes as the kernels do.  d1 = w times row 1 and d2 = w times row 2 / 2 are the coefficient rows of the device."""
    t, wk = _nodes(rho, s, gh_x, gh_w)
    phi, l = np.asarray(phi, dtype=np.float64), np.asarray(logit_y, dtype=np.float64)
    return np.stack([(a * wk).sum(-1) for a in beta_h_dispersion(t, phi[..., None], l[..., None])])


class BetaGLMMObjective(_LogDispersion, _SlopesArrow, _LogisticMixedModel):
    _loss = 'logistic'

    def __init__(self, par, x, y, z, groups, n_groups, dispersion, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0),
                 tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: proportions, finite and STRICTLY inside (0, 1); exact zeros or ones are refused, not clipped.  dispersion: the
        precision phi > 0, a scalar or N values, as in `NegBinomialGLMMObjective`: phi0 of phi = e^lambda phi0, lambda = `log_dispersion_par`.  z: the N x K group
        design, or None for one effect per group with the unit design.  offset: the N offsets o_n on the logit scale, or None for
        zero.  `value` is -ELBO up to the constant `log_norm_const()`.  All checks run before the device context is created."""
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n:
            raise ValueError('y must hold {} values'.format(n))
        bad = int(np.count_nonzero(~((y > 0.0) & (y < 1.0))))               # NaN compares false
        if bad:
            raise ValueError('y must lie strictly inside (0, 1): {} of {} rows do not (zeros and ones are not clipped)'.format(bad, n))
        phi = _hip.as_f64(dispersion).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        phi = np.full(n, phi[0]) if phi.size == 1 else phi.copy()
        if offset is not None:
            offset = _row_vector(offset, n, 'offset')
        if z is None:
            z = np.ones((n, 1))
        logit_y = np.log(y) - np.log1p(-y)
        # the context's y is logit(y): `_y` of the base class holds it, `_y01` the proportions themselves
        super().__init__(par, x, logit_y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)
        self._y01, self._phi, self._offset = y.copy(), phi, offset
        self.ctx.set_offset(offset)
        self.ctx.set_dispersion(phi)
        self._declare_dispersion(phi)

    # ---- the precision as a hyper-parameter ----------------------------------------------------------------
    def _push_dispersion(self, phi):
        self.ctx.set_dispersion(phi)

    def _dispersion_entry(self, point):
        return self.ctx.glmm_beta_dispersion_terms(*point)

    def log_norm_const_dispersion(self):
        """(first, second) derivative in lambda of `log_norm_const()` at the current weights and precision:
        sum w [phi psi(phi) + phi log(1 - y)], and that plus sum w phi^2 psi'(phi)."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        phi = self._phi
        c1 = float(np.sum(w * (phi * digamma(phi) + phi * np.log1p(-self._y01))))
        return c1, c1 + float(np.sum(w * phi * phi * polygamma(1, phi)))

    # ---- the device entries -------------------------------------------------------------------------------------------------
    def _terms(self, *point, **want):
        return self.ctx.glmm_beta_terms(*point, **want)

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_beta_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_beta_group_influence(*point_and_operand)

    def _row_psi_derivs(self, rho, s):
        """(E h', E h'' / 2) at rho + o by the rule the kernels use.  `cross_hessian` of the base class subtracts its `_y` -- here
        logit(y) -- from the first value; a1' of this model has no such term, so it is ADDED here, as the probit and cloglog
        links do ((a1' + l) - l differs from a1' by an ulp of |l| at most)."""
        if self._offset is not None:
            rho = rho + self._offset
        a1, a2 = beta_row_derivs(rho, s, self._y, self._phi, self.gh_x, self.gh_w)
        return a1 + self._y, a2

    # ---- predictions: E sigma(t) is the logit-binomial mean with one trial; this context never sets trials or a link ----------
    def _predict_rows_of(self, newdata, n0, n1):
        if newdata is not None:
            if 'trials' in newdata:
                raise ValueError('newdata has the keys x, z, groups, offset, dispersion (got trials)')
            newdata = {k: a for k, a in newdata.items() if k != 'dispersion'}    # accepted and not needed: the mean does not use it
        return super()._predict_rows_of(newdata, n0, n1)

    def _predict_entry(self, point, cov_beta, window, rows):
        if window is not None:
            return self.ctx.glmm_binomial_predict(*point, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_binomial_predict(*point, cov_beta, new=rows)

    def _response_mean(self, rho, s, trials):
        return beta_response_mean(rho, s, self.gh_x, self.gh_w)

    def log_norm_const(self):
        """sum_n w_n [lgamma(phi_n) + (phi_n - 1) log(1 - y_n) - log y_n] at the current weights, the part of the Beta
        log-density that the value drops: -ELBO(phi) = value - log_norm_const() + KL terms that do not depend on phi, so two
        precisions are compared by value - log_norm_const()."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        return float(np.sum(w * (gammaln(self._phi) + (self._phi - 1.0) * np.log1p(-self._y01) - np.log(self._y01))))

"""Gamma mixed model with a log link and K <= 4 independent random effects per group: right-skewed positive
responses -- costs, durations, concentrations, claim sizes -- `glmer(family = Gamma(link = "log"))`:

    y_n ~ Gamma(shape phi_n, mean mu_n),   mu_n = exp(t_n),   t_n = o_n + x_n . beta + z_n . u_{g(n)}

with a shape phi_n = e^lambda phi0_n > 0 (phi0 a scalar or one value per row, Var y = mu^2 / phi); lambda is ONE declared
hyper-parameter, `log_dispersion_par`, 0 at construction, estimated by `fit_dispersion`.  Priors,
variational families, parameter layout, vector and free coordinates, n_global = 2 P + 4 K and the coupled rows are those of
`LogisticGLMMSlopesObjective` (glmm_slopes.py).  The row's term is

    h(t) = phi (y e^{-t} + t),    -log p(y | t) = h(t) - [phi log phi - lgamma(phi) + (phi - 1) log y]

and the data term is sum_n w_n E h(t), t ~ N(rho_n, s_n); the bracket, summed with the weights, is `log_norm_const()`.  The
expectation is closed form, as for the Poisson model: with rho including the offset,

    E h = g + phi rho,   g = phi exp((log y - rho) + s / 2),
    a1 = phi - g,  a2 = g / 2,  c11 = g,  c12 = -g / 2,  c22 = g / 4       (times w)

-- one exp per row, no quadrature.  The likelihood is not canonical in the walk's sense (the response sits inside g), so there is no
"- y rho" anywhere.  h is linear in phi: the derivative of the data term in lambda is the data term, and the cross Hessian its
gradient.  `gamma_expected_h`, `gamma_row_derivs` and `gamma_response_mean` below are the host forms of what the kernels compute per
row (the policy GammaLik of csrc/k_glmm_walk.h); `gamma_shape_terms` holds the two phi-only pieces of the lambda-derivatives of
`log_norm_const()`.  None of them needs a device.

The O(N) work is `lrvb_glmm_gamma_terms` (csrc/k_glmm_slopes.hip); everything after the per-row coefficients is the shared layer,
unchanged.  The fitted mean E e^t = exp(rho + s / 2) does not depend on phi: predictions go through the Poisson predict entry.
`HurdleGammaGLMM` is the two-part composite for semicontinuous data (zeros plus positive amounts), a host composite without
kernels of its own.
"""
import numpy as np
from scipy.special import gammaln

from . import _hip
from .glmm_binomial import _LogDispersion, _row_vector
from .glmm_hurdle import _HurdleGLMM
from .glmm_slopes import _LogisticMixedModel, _SlopesArrow


def gamma_expected_h(rho, s, log_y, phi):
    """E h^(k), k = 0..4 (a 5 x ... array), h(t) = phi (y e^{-t} + t), t ~ N(rho, s) (rho including the offset), by the rule of
    the kernels: g = phi exp((log y - rho) + s / 2) and [g + phi rho, phi - g, g, -g, g].  The value of a row is w times row 0,
    a1 = w times row 1, a2 = w row 2 / 2, c11 = w row 2, c12 = w row 3 / 2, c22 = w row 4 / 4.  Where g overflows it is inf."""
    rho, s, ly, phi = np.broadcast_arrays(np.asarray(rho, dtype=np.float64), np.asarray(s, dtype=np.float64),
                                          np.asarray(log_y, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    with np.errstate(over='ignore', invalid='ignore'):
        g = phi * np.exp((ly - rho) + 0.5 * s)
        return np.stack([g + phi * rho, phi - g, g, -g, g])


def gamma_row_derivs(rho, s, log_y, phi):
    """(a1', a2') per unit weight of the streamed influence rows: a1' = phi - g, a2' = g / 2."""
    e = gamma_expected_h(rho, s, log_y, phi)
    return e[1], 0.5 * e[2]


def gamma_response_mean(rho, s):
    """E e^t = exp(rho + s / 2), t ~ N(rho, s): the mean of the response, whatever phi."""
    with np.errstate(over='ignore'):
        return np.exp(np.asarray(rho, dtype=np.float64) + 0.5 * np.asarray(s, dtype=np.float64))


# `gamma_shape_terms` switches from the defining forms to the asymptotic series at this phi
SHAPE_SERIES_FROM = 16.0
# B_2k / (2 k) and B_2k, k = 1 .. 9: log z - psi(z) = 1 / (2 z) + sum_k B_2k / (2 k z^2k),  z psi'(z) = 1 + 1 / (2 z) + sum_k B_2k / z^2k
_B2K = (1.0 / 6.0, -1.0 / 30.0, 1.0 / 42.0, -1.0 / 30.0, 5.0 / 66.0, -691.0 / 2730.0, 7.0 / 6.0, -3617.0 / 510.0, 43867.0 / 798.0)


def _shape_series(z):
    """(z (log z - psi(z)), z (1 - z psi'(z))) by the asymptotic series to B_18, for z >= SHAPE_SERIES_FROM (the first term left out
    is below 1e-19 of the result there)."""
    w = 1.0 / z
    w2 = w * w
    k = np.arange(1, len(_B2K) + 1)
    c1, c2 = np.asarray(_B2K) / (2 * k), np.asarray(_B2K)
    a1, a2 = np.zeros_like(z) + c1[-1], np.zeros_like(z) + c2[-1]
    for i in range(len(_B2K) - 2, -1, -1):
        a1, a2 = c1[i] + w2 * a1, c2[i] + w2 * a2
    return 0.5 + w * a1, -0.5 - w * a2


def _u_minus_log1p(u):
    """u - log1p(u) for u > 0: as written above u = 1 / 4 (no small difference there), below it by the alternating series
    u^2 / 2 - u^3 / 3 + .. to u^32 (the first term left out is below 2e-19 of the result)."""
    us = np.minimum(u, 0.25)
    ser = np.full_like(us, 1.0 / 32.0)
    for m in range(31, 1, -1):
        ser = (1.0 / m if m % 2 == 0 else -1.0 / m) + us * ser
    return np.where(u > 0.25, u - np.log1p(u), ser * us * us)


def gamma_shape_terms(phi):
    """(T1, T2) = (phi (log phi - psi(phi)), phi (1 - phi psi'(phi))): the two pieces of the lambda-derivatives of
    `log_norm_const()` that depend on phi alone,
        C_l = sum w [T1 + phi + phi log y],   C_ll = sum w [T1 + T2 + phi + phi log y].
    Formed as written both lose accuracy as phi grows (log phi - psi(phi) ~ 1 / (2 phi) is a difference of two numbers of size
    log phi, and 1 - phi psi'(phi) ~ -1 / (2 phi) one of two numbers near 1).  From phi = SHAPE_SERIES_FROM = 16 on the asymptotic
    series 1 / (2 phi) + 1 / (12 phi^2) - .. and -1 / (2 phi) - 1 / (6 phi^2) + .. (to B_18) are used.  Below the threshold the
    argument is first SHIFTED up to z = phi + n >= 16 by the recurrences of psi and psi', and what the shift adds is written as
    sums of terms of ONE sign, x_j = phi + j, j = 0 .. n - 1:
        log phi - psi(phi)   = [log z - psi(z)] + sum_j [1 / x_j - log1p(1 / x_j)],
        psi'(phi) - 1 / phi  = [psi'(z) - 1 / z] + sum_j 1 / (x_j^2 (x_j + 1))       (1 / phi - 1 / z = sum_j 1 / (x_j (x_j + 1))),
    so that no digits cancel at any phi.  Relative error below 1e-14 on [1e-3, 1e12] against mpmath
    (tests/test_glmm_gamma_host_math.py)."""
    phi = np.asarray(phi, dtype=np.float64)
    p = phi.ravel()
    n = np.maximum(np.ceil(SHAPE_SERIES_FROM - p), 0.0)                     # steps of the shift: 0 from phi = 16 on
    z = p + n
    s1, s2 = _shape_series(z)                                              # z (log z - psi z), z (1 - z psi' z)
    d1, d2 = np.zeros_like(p), np.zeros_like(p)
    for j in range(int(n.max()) if p.size else 0):
        on = j < n
        x = np.where(on, p + j, 1.0)
        u = 1.0 / x
        d1 += np.where(on, _u_minus_log1p(u), 0.0)
        d2 += np.where(on, u * u / (x + 1.0), 0.0)
    t1 = p * (s1 / z + d1)
    t2 = p * p * (s2 / (z * z) - d2)
    return t1.reshape(phi.shape), t2.reshape(phi.shape)


class GammaGLMMObjective(_LogDispersion, _SlopesArrow, _LogisticMixedModel):
    _loss = 'poisson'

    def __init__(self, par, x, y, z, groups, n_groups, dispersion, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0),
                 tau_prior=(1.0, 1.0), names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: responses, finite and STRICTLY positive; a zero is refused, not clipped (zeros plus positive amounts are the two-part
        composite `HurdleGammaGLMM`).  dispersion: the shape phi > 0, a scalar or N values, as in `BetaGLMMObjective`: phi0 of
        phi = e^lambda phi0, lambda = `log_dispersion_par`.  z: the N x K group design, or None for one effect per group with the
        unit design.  offset: the N offsets o_n on the log scale, or None for zero.  `value` is -ELBO up to the constant
        `log_norm_const()`.  All checks run before the device context is created."""
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n:
            raise ValueError('y must hold {} values'.format(n))
        bad = int(np.count_nonzero(~((y > 0.0) & np.isfinite(y))))            # NaN compares false
        if bad:
            raise ValueError('y must be finite and strictly positive: {} of {} rows are not (zeros are not clipped: zeros plus '
                             'positive amounts are the two-part composite HurdleGammaGLMM)'.format(bad, n))
        phi = _hip.as_f64(dispersion).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        phi = np.full(n, phi[0]) if phi.size == 1 else phi.copy()
        if offset is not None:
            offset = _row_vector(offset, n, 'offset')
        if z is None:
            z = np.ones((n, 1))
        # the context's y is log(y): `_y` of the base class holds it, `_ypos` the responses themselves
        super().__init__(par, x, np.log(y), z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, None, names, weights, device)
        self._ypos, self._phi, self._offset = y.copy(), phi, offset
        self.ctx.set_offset(offset)
        self.ctx.set_dispersion(phi)
        self._declare_dispersion(phi)

    # ---- the shape as a hyper-parameter ------------------------------------------------------------------
    def _push_dispersion(self, phi):
        self.ctx.set_dispersion(phi)

    def _dispersion_entry(self, point):
        return self.ctx.glmm_gamma_dispersion_terms(*point[:4])

    def log_norm_const_dispersion(self):
        """(first, second) derivative in lambda of `log_norm_const()` at the current weights and shape:
        sum w [T1 + phi + phi log y] and sum w [T1 + T2 + phi + phi log y], (T1, T2) = `gamma_shape_terms(phi)`."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        phi = self._phi
        t1, t2 = gamma_shape_terms(phi)
        c1 = float(np.sum(w * (t1 + phi * (1.0 + self._y))))
        return c1, c1 + float(np.sum(w * t2))

    # ---- the device entries (the point carries the two unused quadrature slots of the shared layer) ---------------------------
    def _terms(self, m, v, e, r, gh_x, gh_w, **want):
        return self.ctx.glmm_gamma_terms(m, v, e, r, **want)

    def _obs_influence(self, m, v, e, r, gh_x, gh_w, A, **window):
        return self.ctx.glmm_gamma_obs_influence(m, v, e, r, A, **window)

    def _group_influence(self, m, v, e, r, gh_x, gh_w, A):
        return self.ctx.glmm_gamma_group_influence(m, v, e, r, A)

    def _row_psi_derivs(self, rho, s):
        """(phi - g, g / 2) at rho + o by the rule the kernels use.  `cross_hessian` of the base class subtracts its `_y` -- here
        log(y) -- from the first value; a1' of this model has no such term, so it is ADDED here, as the Beta model does
        ((a1' + l) - l differs from a1' by an ulp of |l| at most)."""
        if self._offset is not None:
            rho = rho + self._offset
        a1, a2 = gamma_row_derivs(rho, s, self._y, self._phi)
        return a1 + self._y, a2

    # ---- predictions: E e^t is the Poisson mean; the Poisson entry reads the resident offset and never y ----------------------
    def _predict_rows_of(self, newdata, n0, n1):
        if newdata is not None:
            if 'trials' in newdata:
                raise ValueError('newdata has the keys x, z, groups, offset, dispersion (got trials)')
            newdata = {k: a for k, a in newdata.items() if k != 'dispersion'}    # accepted and not needed: the mean does not use it
        return super()._predict_rows_of(newdata, n0, n1)

    def _predict_entry(self, point, cov_beta, window, rows):
        m, v, e, r = point[:4]
        if window is not None:
            return self.ctx.glmm_poisson_predict(m, v, e, r, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_poisson_predict(m, v, e, r, cov_beta, new=rows[:4])

    def _response_mean(self, rho, s, trials):
        return gamma_response_mean(rho, s)

    def log_norm_const(self):
        """sum_n w_n [phi_n log phi_n - lgamma(phi_n) + (phi_n - 1) log y_n] at the current weights, the part of the Gamma
        log-density that the value drops: -ELBO(phi) = value - log_norm_const() + KL terms that do not depend on phi, so two
        shapes are compared by value - log_norm_const()."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        phi = self._phi
        return float(np.sum(w * (phi * np.log(phi) - gammaln(phi) + (phi - 1.0) * self._y)))


class HurdleGammaGLMM(_HurdleGLMM):
    """The two-part model for semicontinuous data, zeros plus positive amounts, as the pair of its two independent parts:

        zero             `BinomialGLMMObjective` on 1[y > 0] over all N rows under `zero_link`
        count            `GammaGLMMObjective` on the rows with y > 0 (`positive_rows`), with the same G groups: a group without a
                         positive row is an empty group of that model

    y >= 0, finite.  dispersion: the shape phi > 0, a scalar or N values (one per row of the whole data, zeros included; subset to
    the positive rows here, as `HurdleNegBinomialGLMM` does).  `offset` belongs to the Gamma part and `zero_offset` to the zero
    part.  `predict` returns p_pos = P(y > 0), mean_count = E [y | y > 0] and mean = their product under both variances; newdata may
    hold `dispersion`, which the mean does not use."""
    _count_keys = ('dispersion',)

    def __init__(self, par_zero, par_pos, x, y, z, groups, n_groups, dispersion, offset=None, zero_link='logit', zero_offset=None,
                 beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'),
                 weights=None, device=0):
        n = np.shape(x)[0]
        phi = _hip.as_f64(dispersion).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        self._phi = phi.copy()
        super().__init__(par_zero, par_pos, x, y, z, groups, n_groups, offset, zero_link, zero_offset, beta_prior_info, mu_prior,
                         tau_prior, gh_deg, names, weights, device)

    def _check_y(self, y, n):
        if y.size != n or not np.all(np.isfinite(y)) or np.any(y < 0.0):
            raise ValueError('y must hold {} finite values >= 0'.format(n))

    def _make_count(self, par_pos, x, y, z, groups, kw):
        phi = self._phi if self._phi.size == 1 else self._phi[self.positive_rows]
        kw = {k: a for k, a in kw.items() if k != 'gh_deg'}                  # the Gamma part has no quadrature
        return GammaGLMMObjective(par_pos, x, y, z, groups, self.G, phi, **kw)

    def _own_rows(self, sl):
        return {} if self._phi.size == 1 else dict(dispersion=self._phi[sl])

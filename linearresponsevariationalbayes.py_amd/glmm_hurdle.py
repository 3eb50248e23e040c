"""Hurdle count models with K <= 4 independent random effects per group: counts with more zeros, or fewer,
than a Poisson model allows.  The hurdle likelihood

    P(y = 0) = 1 - p,    P(y = k) = p Poisson(k; lambda) / (1 - exp(-lambda)),  k >= 1

factorises EXACTLY into two independent mixed models: a Bernoulli model on 1[y > 0] (`BinomialGLMMObjective`, any link) and a
zero-truncated Poisson model on the rows with y > 0, `TruncatedPoissonGLMMObjective`:

    y_n in {1, 2, ..},  P(y_n | t_n) = e^{y_n t_n - u_n} / (y_n! (1 - e^{-u_n})),  u_n = e^{t_n},  t_n = o_n + x_n . beta + z_n . u_{g(n)}

Priors, variational families, parameter layout, vector and free coordinates, n_global = 2 P + 4 K and the coupled rows are those of
`LogisticGLMMSlopesObjective` (glmm_slopes.py).  The likelihood is canonical in t with the log-partition

    A(t) = log(e^u - 1) = u + log(-expm1(-u)),   A' = u + r = lambda / (1 - e^{-lambda}) (the response mean),  r = u / expm1(u),
    A^(k) = u + r^(k-1), k >= 1       (r' = r q, q = 1 - u - r, q' = -u - r': the recurrences of the cloglog link; A = e^t - h1^cloglog)

and the data term is sum_n w_n [E A(t) - y_n rho_n], t ~ N(rho_n, s_n); the constant sum_n w_n log y_n! is DROPPED from the value
(`log_norm_const`).  The e^t part of every E A^(k) is exp(rho + s / 2) in closed form; log(-expm1(-u)) and r^(k-1) go on the
Gauss-Hermite nodes.  `ztp_A`, `ztp_expected_A`, `ztp_row_derivs` and `ztp_response_mean` below are the host forms of what the
kernels compute per node and per row; they need no device.

The O(N) work is `lrvb_glmm_ztpoisson_terms` (csrc/k_glmm_slopes.hip, the policy TruncPoissonLik of csrc/k_glmm_walk.h); everything
after the per-row coefficients is the shared layer, unchanged.  `HurdlePoissonGLMM` is a host composite of the two models and has
no kernels of its own.

Over-dispersed positive counts: `TruncatedNegBinomialGLMMObjective` is the zero-truncated NB2 model with a
KNOWN dispersion phi_n > 0 (mean mu = e^t, variance mu + mu^2 / phi before truncation), glmmTMB's `truncated_nbinom2`.  With
eta = t - log phi, sp = softplus and v = phi sp(eta), P(y = 0) = (1 + e^eta)^-phi = exp(-v), and the row's term is

    H(eta) = (y + phi) sp(eta) - y eta + g(eta),   g = log(1 - exp(-v))

-- the NB2 term of `NegBinomialGLMMObjective` plus the log of 1 - P(0).  The data term is sum_n w_n E H(eta), eta ~ N(rho_n, s_n),
rho_n including the SHIFTED offset o_n - log phi_n; sum_n w_n [lgamma(y + phi) - lgamma(phi) - log y!] is dropped
(`log_norm_const`).  `ztnb_g`, `ztnb_expected_H`, `ztnb_row_derivs` and `ztnb_response_mean` are the host forms of the policy
TruncNegBinLik; `HurdleNegBinomialGLMM` is `HurdlePoissonGLMM` with this count part.
"""
import numpy as np
from scipy.special import gammaln

from . import _hip
from .glmm_binomial import BinomialGLMMObjective, LINKS, _nodes, _row_vector
from .glmm_slopes import _LogisticMixedModel, _SlopesArrow


def _ztp_node(t, order):
    """[log(-expm1(-u)), r, r', r'', r'''][:order + 1] at t, u = e^t, r = u / expm1(u): what the kernels sum over the nodes."""
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        u = np.exp(t)
        uc = np.minimum(u, 700.0)
        r = np.where(u > 700.0, 0.0, uc / np.expm1(uc))
        q = 1.0 - uc - r
        r1 = r * q
        q1 = -uc - r1
        r2 = r1 * q + r * q1
        q2 = -uc - r2
        g = [np.log(-np.expm1(-u)), r, r1, r2, r2 * q + 2.0 * r1 * q1 + r * q2]
    return g[:order + 1]


def ztp_A(t, order=4):
    """[A, A', .., A^(order)] at t, order <= 4: the log-partition A(t) = log(exp(e^t) - 1) of the zero-truncated Poisson likelihood
    and its derivatives in t by the formulas of the kernels (k_glmm_walk.h, TruncPoissonLik): e^t plus the node part."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(over='ignore'):
        u = np.exp(t)
    return [u + g for g in _ztp_node(t, order)]


def ztp_expected_A(rho, s, gh_x, gh_w):
    """E A^(k), k = 0..4, t ~ N(rho, s) (rho including the offset) by the kernels' rule: exp(rho + s / 2) in closed form plus the
    Gauss-Hermite sum of log(-expm1(-u)) and of r^(k-1).  A 5 x ... array."""
    t, wk = _nodes(rho, s, gh_x, gh_w)
    with np.errstate(over='ignore', invalid='ignore'):
        eu = np.exp(np.asarray(rho, dtype=np.float64) + 0.5 * np.asarray(s, dtype=np.float64))
        return np.stack([(g * wk).sum(-1) + eu for g in _ztp_node(t, 4)])


def ztp_row_derivs(rho, s, gh_x, gh_w):
    """(E A', E A'' / 2): the streamed influence rows use a1' = E A' - y and a2' = E A'' / 2 per unit weight."""
    e = ztp_expected_A(rho, s, gh_x, gh_w)
    return e[1], 0.5 * e[2]


def ztp_response_mean(rho, s, gh_x, gh_w):
    """E [lambda / (1 - exp(-lambda))], lambda = e^t, t ~ N(rho, s): the mean of the truncated count, E A' = exp(rho + s / 2) + E r."""
    return ztp_expected_A(rho, s, gh_x, gh_w)[1]


def _logistic_node(t):
    """softplus and sigma, sigma', sigma'', sigma''' at t as LogisticLik::moments forms them."""
    e = np.exp(-np.abs(t))
    ie = 1.0 / (1.0 + e)
    sp = np.maximum(t, 0.0) + np.log1p(e)
    sg = np.where(t >= 0.0, ie, e * ie)
    g2 = e * ie * ie
    om = (1.0 - e) * ie
    g3 = np.where(t >= 0.0, -g2 * om, g2 * om)
    return sp, sg, g2, g3, g2 * (1.0 - 6.0 * g2)


def _recip_expm1(v):
    """R = 1 / expm1(v), 0 past v = 700 by a select; 1 / 0 = inf where v underflowed to 0 (a refusal, not a clamp)."""
    return np.where(v > 700.0, 0.0, 1.0 / np.expm1(np.minimum(v, 700.0)))


def ztnb_g(eta, phi, order=4):
    """[g, g', .., g^(order)] at eta, order <= 4: g = log(1 - exp(-v)), v = phi softplus(eta), the log of 1 - P(y = 0) of the NB2
    law, and its derivatives in eta by the formulas of the kernels (k_glmm_walk.h, TruncNegBinLik): the chain rule in its factored
    form, a = v' R, b = v'' R, d = v''' R, c = v' + a, every intermediate O(1)."""
    eta, phi = np.broadcast_arrays(np.asarray(eta, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        sp, sg, g2, g3, g4 = _logistic_node(eta)
        v = phi * sp
        R = _recip_expm1(v)
        v1, v2, v3 = phi * sg, phi * g2, phi * g3
        a, b, d = v1 * R, v2 * R, v3 * R
        c = v1 + a
        gg2 = b - a * c
        b1, c1 = d - a * (v2 + b), v2 + gg2
        gg3 = b1 - gg2 * c - a * c1
        d1 = phi * g4 * R - a * (v3 + d)
        b2 = d1 - gg2 * (v2 + b) - a * (v3 + b1)
        gg4 = b2 - gg3 * c - 2.0 * gg2 * c1 - a * (v3 + gg3)
        # the corner e^eta < 1e-3 and v < 0.01, where the derivatives of order 2 to 4 are O(e^eta) differences of O(1) terms
        x = np.exp(np.minimum(eta, 0.0))
        m2, m3, m4 = _ztnb_small_m(x)
        lp, lpp, lppp = -0.5 + v * (1.0 / 12.0 - v * v * (1.0 / 720.0)), 1.0 / 12.0 - v * v * (1.0 / 240.0), v * (-1.0 / 120.0)
        v4 = phi * g4
        small = (eta < ZTNB_ETA_SMALL) & (v < ZTNB_V_SMALL)
        gg2 = np.where(small, m2 + lpp * v1 * v1 + lp * v2, gg2)
        gg3 = np.where(small, m3 + lppp * v1 * v1 * v1 + 3.0 * lpp * v1 * v2 + lp * v3, gg3)
        gg4 = np.where(small, m4 - (1.0 / 120.0) * (v1 * v1) * (v1 * v1) + 6.0 * lppp * v1 * v1 * v2 + lpp * (3.0 * v2 * v2 + 4.0 * v1 * v3)
                       + lp * v4, gg4)
        g = [np.log(-np.expm1(-v)), a, gg2, gg3, gg4]
    return g[:order + 1]


# The corner of `ztnb_g` (and of TruncNegBinLik::node): eta < log(1e-3) and v = phi softplus(eta) < 0.01.  There
#   g = log phi + eta + M(eta) + L(v),   M = log(softplus(eta) / e^eta) = sum_k c_k x^k with x = e^eta,
#   L = log((1 - e^-v) / v) = -v / 2 + v^2 / 24 - v^4 / 2880,
# and every term of g^(2) = M^(2) + L^(2) v_1^2 + L^(1) v_2, .. has the sign and the size of the result: no cancellation.  What the two
# series leave out is below 2e-13 (x^6) and 1e-15 (v^6) of the result.
ZTNB_ETA_SMALL, ZTNB_V_SMALL = -6.907755278982137, 0.01
_ZTNB_M = (-1.0 / 2.0, 5.0 / 24.0, -1.0 / 8.0, 251.0 / 2880.0, -19.0 / 288.0)


def _ztnb_small_m(x):
    """The derivatives of order 2, 3, 4 in eta of M = sum_k c_k x^k, x = e^eta: sum_k c_k k^j x^k, by Horner."""
    c = _ZTNB_M
    return tuple(x * (c[0] + x * (2.0 ** j * c[1] + x * (3.0 ** j * c[2] + x * (4.0 ** j * c[3] + x * (5.0 ** j * c[4])))))
                 for j in (2, 3, 4))


def ztnb_expected_H(rho, s, y, phi, gh_x, gh_w):
    """E [H + y eta], E [H' + y], E H'', E H''', E H'''' (a 5 x ... array), H = (y + phi) softplus - y eta + g, eta ~ N(rho, s)
    (rho including the shifted offset o - log phi), by the kernels' rule: (y + phi) sp^(k) + g^(k) summed over the Gauss-Hermite
    nodes.  The value of a row is w (row 0 - y rho), a1 = w (row 1 - y)."""
    t, wk = _nodes(rho, s, gh_x, gh_w)
    y, phi = np.asarray(y, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    m = (y + phi)[..., None]
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        lg = _logistic_node(t)
        g = ztnb_g(t, phi[..., None], 4)
        return np.stack([((m * a + b) * wk).sum(-1) for a, b in zip(lg, g)])


def ztnb_row_derivs(rho, s, y, phi, gh_x, gh_w):
    """((y + phi) E sigma + E g', E H'' / 2): the streamed influence rows use a1' = the first - y and a2' = the second per unit weight."""
    e = ztnb_expected_H(rho, s, y, phi, gh_x, gh_w)
    return e[1], 0.5 * e[2]


def ztnb_response_mean(rho, s, phi, gh_x, gh_w):
    """E [mu / (1 - P0)] = E [e^t (1 + R(v))], e^t = phi e^eta, eta ~ N(rho, s) (rho on the SHIFTED scale, t - log phi): the mean
    of the truncated count.  The e^t part is phi exp(rho + s / 2) in closed form and not clamped; e^t R(v) goes on the nodes."""
    phi = np.asarray(phi, dtype=np.float64)
    with np.errstate(over='ignore'):
        return phi * np.exp(np.asarray(rho, dtype=np.float64) + 0.5 * np.asarray(s, dtype=np.float64)) + _ztnb_mean_nodes(rho, s, phi, gh_x, gh_w)


def _ztnb_mean_nodes(rho, s, phi, gh_x, gh_w):
    """The node part of `ztnb_response_mean`: the Gauss-Hermite sum of e^t R(v), 0 past v = 700 by the select of the derivatives."""
    t, wk = _nodes(rho, s, gh_x, gh_w)
    phi = np.asarray(phi, dtype=np.float64)
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        v = phi[..., None] * _logistic_node(t)[0]
        return (np.where(v > 700.0, 0.0, phi[..., None] * np.exp(t) * _recip_expm1(v)) * wk).sum(-1)


class TruncatedPoissonGLMMObjective(_SlopesArrow, _LogisticMixedModel):
    _loss = 'poisson'

    def __init__(self, par, x, y, z, groups, n_groups, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0),
                 gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: positive counts (finite, >= 1; log y! is dropped from the value).  z: the N x K group design, or None for one effect
        per group with the unit design (a column of ones is sent).  offset: the N log exposures o_n, or None for zero.  names: as
        `LogisticGLMMSlopesObjective`.  All checks run before the device context is created."""
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n or not np.all(np.isfinite(y)) or np.any(y < 1.0):
            raise ValueError('y must hold {} finite counts >= 1 (the zero-truncated model has no zeros)'.format(n))
        if offset is not None:
            offset = _row_vector(offset, n, 'offset')
        if z is None:
            z = np.ones((n, 1))
        super().__init__(par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)
        self._offset = offset
        self.ctx.set_offset(offset)

    # ---- the device entries -------------------------------------------------------------------------------------------------
    def _terms(self, *point, **want):
        return self.ctx.glmm_ztpoisson_terms(*point, **want)

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_ztpoisson_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_ztpoisson_group_influence(*point_and_operand)

    def _predict_entry(self, point, cov_beta, window, rows):
        if window is not None:
            return self.ctx.glmm_ztpoisson_predict(*point, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_ztpoisson_predict(*point, cov_beta, new=rows[:4])

    def _response_mean(self, rho, s, trials):
        return ztp_response_mean(rho, s, self.gh_x, self.gh_w)

    def _row_psi_derivs(self, rho, s):
        """(E A', E A'' / 2) at rho + o by the rule the kernels use, so that the dense weight cross Hessian is the derivative of
        the same function as the streamed rows; `cross_hessian` of the base class subtracts y from the first."""
        if self._offset is not None:
            rho = rho + self._offset
        return ztp_row_derivs(rho, s, self.gh_x, self.gh_w)

    def log_norm_const(self):
        """-sum_n w_n log y_n! at the current weights, the constant the value drops: -ELBO = value - log_norm_const() + the KL
        terms, so that models of the same counts are compared by value - log_norm_const()."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        return float(-np.sum(w * gammaln(self._y + 1.0)))


class TruncatedNegBinomialGLMMObjective(_SlopesArrow, _LogisticMixedModel):
    _loss = 'logistic'

    def __init__(self, par, x, y, z, groups, n_groups, dispersion, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0),
                 tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: positive counts (finite, >= 1).  dispersion: phi > 0, a scalar or N values, as in `NegBinomialGLMMObjective` -- fixed
        data, not estimated.  z: the N x K group design, or None for one effect per group with the unit design.  offset: the N log
        exposures o_n, or None for zero.  `value` is -ELBO up to the constant `log_norm_const()`.  All checks run before the
        device context is created."""
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n or not np.all(np.isfinite(y)) or np.any(y < 1.0):
            raise ValueError('y must hold {} finite counts >= 1 (the zero-truncated model has no zeros)'.format(n))
        phi = _hip.as_f64(dispersion).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        self._scalar_phi = float(phi[0]) if phi.size == 1 else None
        phi = np.full(n, phi[0]) if phi.size == 1 else phi.copy()
        o = np.zeros(n) if offset is None else _row_vector(offset, n, 'offset')
        if z is None:
            z = np.ones((n, 1))
        super().__init__(par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)
        # the kernels work on eta = t - log phi: `_offset` is the shifted offset.  The raw one is kept: `predict` reports rho on
        # its scale, where the closed-form part of the mean reads exp(rho_raw + s / 2) = phi exp(rho + s / 2)
        self._phi, self._raw_offset, self._offset = phi, o, o - np.log(phi)
        self.ctx.set_offset(self._offset)
        self.ctx.set_dispersion(phi)

    # ---- the device entries -------------------------------------------------------------------------------------------------
    def _terms(self, *point, **want):
        return self.ctx.glmm_ztnegbin_terms(*point, **want)

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_ztnegbin_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_ztnegbin_group_influence(*point_and_operand)

    def _row_psi_derivs(self, rho, s):
        """((y + phi) E sigma + E g', E H'' / 2) at rho + the shifted offset by the rule the kernels use; `cross_hessian` of the
        base class subtracts y from the first."""
        return ztnb_row_derivs(rho + self._offset, s, self._y, self._phi, self.gh_x, self.gh_w)

    # ---- predictions: the rows carry the shifted offset and phi (in the slot of the trials) ------------------------------------
    def _predict_rows_of(self, newdata, n0, n1):
        if newdata is None:
            x, z, gid, off, _ = super()._predict_rows_of(None, n0, n1)
            return x, z, gid, off, self._phi[int(n0):self.n_obs if n1 is None else int(n1)]
        if 'trials' in newdata:
            raise ValueError('newdata has the keys x, z, groups, offset, dispersion (got trials)')
        x, z, gid, off, _ = super()._predict_rows_of({k: a for k, a in newdata.items() if k != 'dispersion'}, n0, n1)
        n = x.shape[0]
        phi = newdata.get('dispersion')
        if phi is None:
            if self._scalar_phi is None:
                raise ValueError('newdata: dispersion is required, the model was given one dispersion per row')
            phi = self._scalar_phi
        phi = _hip.as_f64(phi).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('newdata: dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        phi = np.full(n, phi[0]) if phi.size == 1 else phi.copy()
        return x, z, gid, (np.zeros(n) if off is None else off) - np.log(phi), phi

    def _predict_entry(self, point, cov_beta, window, rows):
        if window is not None:
            return self.ctx.glmm_ztnegbin_predict(*point, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_ztnegbin_predict(*point, cov_beta, new=rows)

    def _response_mean(self, rho, s, phi):
        return ztnb_response_mean(rho, s, phi, self.gh_x, self.gh_w)

    def predict(self, x, newdata=None, n0=0, n1=None, is_free=True, on_device=False):
        """`predict` of the shared layer; `rho` is the linear predictor t = o + x . m + z . e_g on the log-mean scale (the raw
        offset), and the means are those of the TRUNCATED count.  newdata may hold `dispersion` (a scalar or one value per row),
        required when the model was given one dispersion per row.  A mean that overflows is a ValueError."""
        out = super().predict(x, newdata=newdata, n0=n0, n1=n1, is_free=is_free, on_device=on_device)
        out['rho'] = np.asarray(out['rho']) + np.log(self._predict_rows_of(newdata, n0, n1)[4])
        if not (np.all(np.isfinite(out['mean_mf'])) and np.all(np.isfinite(out['mean_lrvb']))):
            raise ValueError('the mean of the truncated count is not finite for some row: exp(rho + var / 2) overflows (it is not clamped)')
        return out

    def log_norm_const(self):
        """C(y, phi) = sum_n w_n [log Gamma(y_n + phi_n) - log Gamma(phi_n) - log Gamma(y_n + 1)] at the current weights, the
        constant of the NB2 law that the value drops (`NegBinomialGLMMObjective.log_norm_const`)."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        return float(np.sum(w * (gammaln(self._y + self._phi) - gammaln(self._phi) - gammaln(self._y + 1.0))))


class _HurdleGLMM:
    """What the hurdle composites share: the zero part, the rows with y > 0, `value`, `predict`.  A subclass builds its count part
    in `_make_count` and names in `_count_keys` what its count part takes from newdata beyond x, z, groups and offset."""
    _count_keys = ()

    def __init__(self, par_zero, par_count, x, y, z, groups, n_groups, offset=None, zero_link='logit', zero_offset=None,
                 beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'),
                 weights=None, device=0):
        if zero_link not in LINKS:
            raise ValueError("zero_link must be 'logit', 'probit' or 'cloglog' (got {!r})".format(zero_link))
        x = _hip.as_f64(x)
        n = x.shape[0]
        y = _hip.as_f64(y).ravel()
        self._check_y(y, n)
        z = np.ones((n, 1)) if z is None else _hip.as_f64(z)
        groups = np.asarray(groups).ravel()
        if offset is not None:
            offset = _row_vector(offset, n, 'offset')
        w = None if weights is None else _row_vector(weights, n, 'weights')
        pos = np.flatnonzero(y > 0.0)
        if pos.size == 0:
            raise ValueError('the count part needs at least one row with y > 0')
        kw = dict(beta_prior_info=beta_prior_info, mu_prior=mu_prior, tau_prior=tau_prior, gh_deg=gh_deg, names=names, device=device)
        self.positive_rows = pos
        self.n_obs, self.G = n, int(n_groups)
        self._x, self._z, self._groups, self._offset = x, z, groups, offset
        self._zero_offset = None if zero_offset is None else _row_vector(zero_offset, n, 'zero_offset')
        self.zero = BinomialGLMMObjective(par_zero, x, (y > 0.0).astype(np.float64), z, groups, n_groups, offset=self._zero_offset,
                                          weights=w, link=zero_link, **kw)
        self.count = self._make_count(par_count, x[pos], y[pos], z[pos], groups[pos],
                                      dict(kw, offset=None if offset is None else offset[pos], weights=None if w is None else w[pos]))

    def _check_y(self, y, n):
        """The responses of the composite (a subclass with a continuous positive part accepts what lies between 0 and 1)."""
        if y.size != n or not np.all(np.isfinite(y)) or np.any(y < 0.0) or np.any((y > 0.0) & (y < 1.0)):
            raise ValueError('y must hold {} finite counts: 0, or >= 1'.format(n))

    def value(self, x_zero, x_count, is_free=True):
        """The sum of the two parts' values: -ELBO of the hurdle model up to `log_norm_const()`."""
        return self.zero.value(x_zero, is_free) + self.count.value(x_count, is_free)

    def log_norm_const(self):
        return self.count.log_norm_const()

    def _rows(self, newdata, n0, n1):
        """newdata of the two parts: (zero, count).  None: the window [n0, n1) of the model's own N rows, which the count part
        holds only where y > 0 and is therefore handed as new rows."""
        if newdata is None:
            n0 = int(n0)
            n1 = self.n_obs if n1 is None else int(n1)
            if n0 < 0 or n1 > self.n_obs or n0 > n1:
                raise ValueError('row range [{}, {}) outside [0, {})'.format(n0, n1, self.n_obs))
            sl = slice(n0, n1)
            newdata = dict(x=self._x[sl], z=self._z[sl], groups=self._groups[sl],
                           offset=None if self._offset is None else self._offset[sl],
                           zero_offset=None if self._zero_offset is None else self._zero_offset[sl], **self._own_rows(sl))
        keys = ('x', 'z', 'groups', 'offset', 'zero_offset') + self._count_keys
        unknown = set(newdata) - set(keys)
        if unknown:
            raise ValueError('newdata has the keys {} (got {})'.format(', '.join(keys), sorted(unknown)))
        shared = {k: newdata.get(k) for k in ('x', 'z', 'groups')}
        count = dict(shared, offset=newdata.get('offset'), **{k: newdata[k] for k in self._count_keys if newdata.get(k) is not None})
        return dict(shared, offset=newdata.get('zero_offset')), count

    def _own_rows(self, sl):
        """What the count part needs of the model's own rows `sl` beyond x, z, groups and offset."""
        return {}

    def predict(self, x_zero, x_count, newdata=None, n0=0, n1=None, on_device=False):
        """Fitted values (newdata=None: rows n0..n1 of the data, zeros included) or predictions for new rows
        `newdata = dict(x=, z=, groups=, offset=, zero_offset=)`, groups -1 being the population level, at the free points of
        the two parts.  A dict of one value per row under the mean-field (`_mf`) and the linear-response (`_lrvb`) variance:
        p_pos = P(y > 0), mean_count = E [y | y > 0] and mean = p_pos mean_count = E y; `zero` and `count` hold the two parts'
        own `predict` results."""
        nd_zero, nd_count = self._rows(newdata, n0, n1)
        pz = self.zero.predict(x_zero, newdata=nd_zero, on_device=on_device)
        pc = self.count.predict(x_count, newdata=nd_count, on_device=on_device)
        out = dict(zero=pz, count=pc)
        for v in ('mf', 'lrvb'):
            out['p_pos_' + v], out['mean_count_' + v] = pz['mean_' + v], pc['mean_' + v]
            out['mean_' + v] = pz['mean_' + v] * pc['mean_' + v]
        return out


class HurdlePoissonGLMM(_HurdleGLMM):
    """The hurdle Poisson mixed model as the pair of its two independent parts, fitted and queried separately:

        zero             `BinomialGLMMObjective` on 1[y > 0] over all N rows under `zero_link`
        count            `TruncatedPoissonGLMMObjective` on the rows with y > 0 (`positive_rows`), with the same G groups: a group
                         without a positive row is an empty group of that model

    Both parts share x, z and the groups; `offset` (the log exposure) belongs to the count part and `zero_offset` to the zero
    part.  par_zero and par_count are two parameters of the layout of `LogisticGLMMSlopesObjective`.  The variational posteriors
    of the two parts are independent, so E [p lambda / (1 - e^{-lambda})] is the product of the two expectations."""

    def _make_count(self, par_count, x, y, z, groups, kw):
        return TruncatedPoissonGLMMObjective(par_count, x, y, z, groups, self.G, **kw)


class HurdleNegBinomialGLMM(_HurdleGLMM):
    """The hurdle NB2 mixed model (glmmTMB's `truncated_nbinom2` with a binomial zero part): `HurdlePoissonGLMM` with
    `TruncatedNegBinomialGLMMObjective` as the count part.  dispersion: phi > 0, a scalar or N values (one per row of the whole
    data, zeros included; subset to the positive rows here); newdata of `predict` may hold `dispersion`, required when phi was
    given per row.  At phi = 1 and zero_link='logit' with equal linear predictors the model is the plain NB2 one."""
    _count_keys = ('dispersion',)

    def __init__(self, par_zero, par_count, x, y, z, groups, n_groups, dispersion, offset=None, zero_link='logit', zero_offset=None,
                 beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'),
                 weights=None, device=0):
        n = np.shape(x)[0]
        phi = _hip.as_f64(dispersion).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        self._phi = phi.copy()
        super().__init__(par_zero, par_count, x, y, z, groups, n_groups, offset, zero_link, zero_offset, beta_prior_info, mu_prior,
                         tau_prior, gh_deg, names, weights, device)

    def _make_count(self, par_count, x, y, z, groups, kw):
        phi = self._phi if self._phi.size == 1 else self._phi[self.positive_rows]
        return TruncatedNegBinomialGLMMObjective(par_count, x, y, z, groups, self.G, phi, **kw)

    def _own_rows(self, sl):
        return {} if self._phi.size == 1 else dict(dispersion=self._phi[sl])

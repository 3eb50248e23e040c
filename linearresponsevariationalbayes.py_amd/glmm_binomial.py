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
offset o - log phi.  `NegBinomialGLMMObjective` is that construction and nothing else; phi is fixed data, not a hyper-parameter,
and is not estimated.

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


def _h1_probit(t, order):
    """-log Phi(t) and its derivatives through the inverse Mills ratio lambda = sqrt(2 / pi) / erfcx(-t / sqrt 2)."""
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        ex = erfcx(-t / np.sqrt(2.0))
        lam = np.sqrt(2.0 / np.pi) / ex
        d = t + lam
        w = lam * d
        w1 = lam * (1.0 - w) - w * d
        h = [np.where(t < 0.0, 0.5 * t * t - np.log(0.5 * ex), -np.log1p(-0.5 * erfc(np.maximum(t, 0.0) / np.sqrt(2.0)))),
             -lam, w, w1, -w1 * (d + lam) - 2.0 * w * (1.0 - w)]
    return h[:order + 1]


def _h1_cloglog(t, order):
    """-log(1 - exp(-u)), u = e^t, and its derivatives in t through r = u / expm1(u): r' = r (1 - u - r)."""
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        u = np.exp(t)
        uc = np.minimum(u, 700.0)
        r = np.where(u > 700.0, 0.0, uc / np.expm1(uc))
        q = 1.0 - uc - r
        r1 = r * q
        q1 = -uc - r1
        r2 = r1 * q + r * q1
        q2 = -uc - r2
        h = [-np.log(-np.expm1(-u)), -r, -r1, -r2, -(r2 * q + 2.0 * r1 * q1 + r * q2)]
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


class NegBinomialGLMMObjective(BinomialGLMMObjective):
    def __init__(self, par, x, y, z, groups, n_groups, dispersion, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0),
                 tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: counts (finite, >= 0).  dispersion: phi > 0, a scalar or N values -- Var y = mu + mu^2 / phi, so phi -> infinity is
        the Poisson model; fixed data, not estimated.  offset: the N log exposures, or None.  The model is the binomial one with
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

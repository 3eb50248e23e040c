"""Poisson mixed model with K <= 4 independent random effects per group -- count regression with a log link, an exposure offset
and random slopes:

    y_n ~ Poisson(exp(o_n + x_n . beta + z_n . u_{g(n)})),   z_n in R^K,   u_gk ~ N(mu_k, 1 / tau_k) independently over k

Priors, variational families, parameter layout, vector and free coordinates, n_global = 2 P + 4 K and the coupled rows are those
of `LogisticGLMMSlopesObjective` (glmm_slopes.py).  Only the data term differs:

    sum_n w_n [ psi_n - y_n rho_n ],   rho_n = o_n + x_n . m + z_n . e_g,   s_n = (x_n o x_n) . v + (z_n o z_n) . r_g,
    psi_n = E exp(t) = exp(rho_n + s_n / 2),  t ~ N(rho_n, s_n)             -- exact, no quadrature.

The constant sum_n w_n log y_n! of the Poisson log-likelihood does not depend on the parameters and is DROPPED from the value.
The O(N) work is `lrvb_glmm_poisson_terms` (csrc/k_glmm_slopes.hip); everything after the per-row coefficients -- the group
sums, `glmm_slopes_closed_forms`, `block_arrow.py`, the Schur entry and the device-resident solve -- is the shared layer, unchanged.
"""
import numpy as np

from . import _hip
from .glmm_slopes import _LogisticMixedModel, _SlopesArrow


class PoissonGLMMObjective(_SlopesArrow, _LogisticMixedModel):
    _loss = 'poisson'

    def __init__(self, par, x, y, z, groups, n_groups, offset=None, beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0),
                 names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: counts (finite, >= 0; log y! is dropped from the value).  z: the N x K group design, or None for one effect per
        group with the unit design (a column of ones is sent: there is no separate K = 1 kernel).  offset: the N log exposures
        o_n, or None for zero.  names: the parameters of q(beta), q(mu), q(tau_k) -- named names[2] + str(k), k = 0..K-1 -- and
        q(u)."""
        y = _hip.as_f64(y).ravel()
        if not np.all(np.isfinite(y)) or np.any(y < 0.0):
            raise ValueError('y must hold finite counts >= 0')
        n = np.shape(x)[0]
        if z is None:
            z = np.ones((n, 1))
        if offset is not None:
            offset = _hip.as_f64(offset).ravel().copy()
            if offset.size != n or not np.all(np.isfinite(offset)):
                raise ValueError('offset must hold {} finite values'.format(n))
        super().__init__(par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, None, names, weights, device)
        self._offset = offset
        self.ctx.set_offset(offset)

    # ---- the device entries (the point carries the two unused quadrature slots of the shared layer) ---------------------------
    def _terms(self, m, v, e, r, gh_x, gh_w, **want):
        return self.ctx.glmm_poisson_terms(m, v, e, r, **want)

    def _obs_influence(self, m, v, e, r, gh_x, gh_w, A, **window):
        return self.ctx.glmm_poisson_obs_influence(m, v, e, r, A, **window)

    def _group_influence(self, m, v, e, r, gh_x, gh_w, A):
        return self.ctx.glmm_poisson_group_influence(m, v, e, r, A)

    def _predict_entry(self, point, cov_beta, window, rows):
        m, v, e, r = point[:4]
        if window is not None:
            return self.ctx.glmm_poisson_predict(m, v, e, r, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_poisson_predict(m, v, e, r, cov_beta, new=rows[:4])

    def _response_mean(self, rho, s, trials):
        return np.exp(rho + 0.5 * s)

    def _row_psi_derivs(self, rho, s):
        psi = np.exp(rho + (0.0 if self._offset is None else self._offset) + 0.5 * s)
        return psi, 0.5 * psi

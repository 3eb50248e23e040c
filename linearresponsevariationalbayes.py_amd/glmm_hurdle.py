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


class HurdlePoissonGLMM:
    """The hurdle Poisson mixed model as the pair of its two independent parts, fitted and queried separately:

        zero             `BinomialGLMMObjective` on 1[y > 0] over all N rows under `zero_link`
        count            `TruncatedPoissonGLMMObjective` on the rows with y > 0 (`positive_rows`), with the same G groups: a group
                         without a positive row is an empty group of that model

    Both parts share x, z and the groups; `offset` (the log exposure) belongs to the count part and `zero_offset` to the zero
    part.  par_zero and par_count are two parameters of the layout of `LogisticGLMMSlopesObjective`.  The variational posteriors
    of the two parts are independent, so E [p lambda / (1 - e^{-lambda})] is the product of the two expectations."""

    def __init__(self, par_zero, par_count, x, y, z, groups, n_groups, offset=None, zero_link='logit', zero_offset=None,
                 beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'),
                 weights=None, device=0):
        if zero_link not in LINKS:
            raise ValueError("zero_link must be 'logit', 'probit' or 'cloglog' (got {!r})".format(zero_link))
        x = _hip.as_f64(x)
        n = x.shape[0]
        y = _hip.as_f64(y).ravel()
        if y.size != n or not np.all(np.isfinite(y)) or np.any(y < 0.0) or np.any((y > 0.0) & (y < 1.0)):
            raise ValueError('y must hold {} finite counts: 0, or >= 1'.format(n))
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
        self.count = TruncatedPoissonGLMMObjective(par_count, x[pos], y[pos], z[pos], groups[pos], n_groups,
                                                   offset=None if offset is None else offset[pos],
                                                   weights=None if w is None else w[pos], **kw)

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
                           zero_offset=None if self._zero_offset is None else self._zero_offset[sl])
        unknown = set(newdata) - {'x', 'z', 'groups', 'offset', 'zero_offset'}
        if unknown:
            raise ValueError('newdata has the keys x, z, groups, offset, zero_offset (got {})'.format(sorted(unknown)))
        shared = {k: newdata.get(k) for k in ('x', 'z', 'groups')}
        return dict(shared, offset=newdata.get('zero_offset')), dict(shared, offset=newdata.get('offset'))

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

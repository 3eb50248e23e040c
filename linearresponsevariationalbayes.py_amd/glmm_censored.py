"""Censored Gaussian (Tobit) mixed model with K <= 4 independent random effects per group: a Gaussian
response of which some rows are only known to lie above or below a value -- a study that ends before the event, an assay with a
detection limit -- `censReg`, `lmec`, `brms(y | cens(c) ~ ..)`; on log-times the log-normal accelerated-failure-time model with
shared frailties, `survreg(dist = "lognormal") + frailty`:

    y*_n ~ N(t_n, 1 / phi_n),   t_n = o_n + x_n . beta + z_n . u_{g(n)},   status delta_n in {0, +1, -1}:
    delta = 0: y_n = y*_n is observed;   delta = +1: right-censored, y*_n > y_n;   delta = -1: left-censored, y*_n < y_n

with a precision phi_n = e^lambda phi0_n = 1 / sigma_n^2 > 0 (phi0 a scalar or one value per row); lambda is ONE declared
hyper-parameter, `log_dispersion_par`, 0 at construction, estimated by `fit_dispersion`.  Priors, variational
families, parameter layout, vector and free coordinates, n_global = 2 P + 4 K and the coupled rows are those of
`LogisticGLMMSlopesObjective` (glmm_slopes.py).  With r = sqrt(phi) the row's term is

    observed   h(t) = phi (y - t)^2 / 2,           -log p(y | t) = h(t) - [log(phi) / 2 - log(2 pi) / 2]
    censored   h(t) = -log Phi(a),  a = delta r (t - y),  which is -log P(y* > y | t) or -log P(y* < y | t) whole

and the data term is sum_n w_n E h(t), t ~ N(rho_n, s_n); the bracket, summed with the weights over the OBSERVED rows only, is
`log_norm_const()`.  An observed row is closed form,

    E h = phi ((y - rho)^2 + s) / 2,   E h' = -phi (y - rho),   E h'' = phi,   E h''' = E h'''' = 0,

a censored one goes on the Gauss-Hermite nodes with d_t^k h = (delta r)^k H^(k)(a), H = -log Phi evaluated through the inverse
Mills ratio exactly as the probit link evaluates it (glmm_binomial._h1_probit, BinomialLinkLik<PROBIT>::h1 on the device).  The
likelihood is not canonical in the walk's sense (the response sits inside h), so there is no "- y rho" anywhere.
`censnormal_expected_h`, `censnormal_row_derivs`, `censnormal_response_mean` and `censnormal_dispersion_moments` below are the host
forms of what the kernels compute per row (the policies CensNormalLik and CensNormalDispLik of csrc/k_glmm_walk.h); none of them
needs a device.

The O(N) work is `lrvb_glmm_censnormal_terms` (csrc/k_glmm_slopes.hip); everything after the per-row coefficients is the shared
layer, unchanged.  `predict` returns the LATENT mean E y* = rho under both variances, whatever phi.
"""
import numpy as np

from . import _hip
from .glmm_binomial import _LogDispersion, _h1_probit, _nodes, _row_vector
from .glmm_slopes import _LogisticMixedModel, _SlopesArrow


def _rows(rho, s, y, phi, status):
    rho, s, y, phi, st = np.broadcast_arrays(np.asarray(rho, dtype=np.float64), np.asarray(s, dtype=np.float64),
                                             np.asarray(y, dtype=np.float64), np.asarray(phi, dtype=np.float64),
                                             np.asarray(status, dtype=np.float64))
    return rho, s, y, phi, st


def _censored_nodes(rho, s, y, phi, st, gh_x, gh_w):
    """(a, w_k, delta r): the argument a = delta r (t_k - y) of -log Phi on the nodes, formed as the kernels form it -- the fold
    u = rho - y first, then u + sqrt(s) x_k, then ONE product with delta r.  a = 0 on observed rows (their node sums are not read)."""
    tu, wk = _nodes(rho - y, s, gh_x, gh_w)
    dr = st * np.sqrt(phi)
    return dr[..., None] * tu, wk, dr


def censnormal_expected_h(rho, s, y, phi, status, gh_x, gh_w):
    """E h^(k), k = 0..4 (a 5 x ... array), t ~ N(rho, s) (rho including the offset), by the rule of the kernels: observed rows
    (status 0) in closed form, [phi ((rho - y)^2 + s) / 2, phi (rho - y), phi, 0, 0]; censored rows (status +-1) summed over the
    Gauss-Hermite nodes, (delta r)^k sum_k w_k H^(k)(a_k).  The value of a row is w times row 0, a1 = w times row 1 (there is no
    "- y"), a2 = w row 2 / 2, c11 = w row 2, c12 = w row 3 / 2, c22 = w row 4 / 4.  Where a sum overflows it is inf."""
    rho, s, y, phi, st = _rows(rho, s, y, phi, status)
    a, wk, dr = _censored_nodes(rho, s, y, phi, st, gh_x, gh_w)
    with np.errstate(over='ignore', invalid='ignore'):
        H = [(h * wk).sum(-1) for h in _h1_probit(a, 4)]
        cens = [H[0], H[1] * dr, H[2] * phi, H[3] * (dr * phi), H[4] * (phi * phi)]
        u = rho - y
        zero = np.zeros_like(u)
        obs = [0.5 * (phi * (u * u + s)), phi * u, phi + zero, zero, zero]
        return np.stack([np.where(st != 0.0, c, o) for c, o in zip(cens, obs)])


def censnormal_row_derivs(rho, s, y, phi, status, gh_x, gh_w):
    """(a1', a2') per unit weight of the streamed influence rows: a1' = E h', a2' = E h'' / 2."""
    e = censnormal_expected_h(rho, s, y, phi, status, gh_x, gh_w)
    return e[1], 0.5 * e[2]


def censnormal_response_mean(rho, s=None):
    """E y* = E t = rho, t ~ N(rho, s) (rho including the offset): the latent mean, whatever phi and whatever s."""
    return np.array(rho, dtype=np.float64, copy=True)


def censnormal_dispersion_moments(rho, s, y, phi, status, gh_x, gh_w):
    """(E h_l, E d_t h_l, E d_t^2 h_l, E h_ll), a 4 x ... array: the row term differentiated in lambda, phi = e^lambda phi0, at fixed t
    (d a / d lambda = a / 2), by the rule of the kernels (CensNormalDispLik).  Observed rows are linear in phi, as the Gamma term:
    (E h, E h', E h'', E h).  Censored rows, on the nodes:
        h_l = a H' / 2,   d_t h_l = delta r (a H'' + H') / 2,   d_t^2 h_l = phi (a H''' + 2 H'') / 2,   h_ll = a (a H'' + H') / 4.
    d1 = w times row 1 and d2 = w times row 2 / 2 are the coefficient rows of the device."""
    rho, s, y, phi, st = _rows(rho, s, y, phi, status)
    a, wk, dr = _censored_nodes(rho, s, y, phi, st, gh_x, gh_w)
    with np.errstate(over='ignore', invalid='ignore'):
        H = _h1_probit(a, 3)
        b1 = a * H[2] + H[1]
        cens = [0.5 * ((a * H[1]) * wk).sum(-1), (0.5 * dr) * (b1 * wk).sum(-1), (0.5 * phi) * ((a * H[3] + 2.0 * H[2]) * wk).sum(-1),
                0.25 * ((a * b1) * wk).sum(-1)]
        u = rho - y
        eh = 0.5 * (phi * (u * u + s))
        obs = [eh, phi * u, phi + np.zeros_like(u), eh]
        return np.stack([np.where(st != 0.0, c, o) for c, o in zip(cens, obs)])


class CensoredNormalGLMMObjective(_LogDispersion, _SlopesArrow, _LogisticMixedModel):
    _loss = 'logistic'

    def __init__(self, par, x, y, z, groups, n_groups, dispersion, censoring=None, offset=None, beta_prior_info=1.0,
                 mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20, names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        """y: the responses, finite; on a censored row the value the latent response is known to lie above or below.  dispersion: the
        precision phi = 1 / sigma^2 > 0, a scalar or N values, as in `GammaGLMMObjective`: phi0 of phi = e^lambda phi0,
        lambda = `log_dispersion_par`.  censoring: None (every row observed) or N integers in {-1, 0, 1}: -1 left-censored (y* < y),
        0 observed, +1 right-censored (y* > y).  z: the N x K group design, or None for one effect per group with the unit design.
        offset: the N offsets o_n, or None for zero.  `value` is -ELBO up to the constant `log_norm_const()`.  All checks run
        before the device context is created."""
        y = _hip.as_f64(y).ravel()
        n = np.shape(x)[0]
        if y.size != n:
            raise ValueError('y must hold {} values'.format(n))
        bad = int(np.count_nonzero(~np.isfinite(y)))
        if bad:
            raise ValueError('y must be finite: {} of {} rows are not (an open-ended row is a censored one: give its bound and '
                             'censoring = +1 or -1)'.format(bad, n))
        phi = _hip.as_f64(dispersion).ravel()
        if phi.size not in (1, n) or not np.all(np.isfinite(phi)) or np.any(phi <= 0.0):
            raise ValueError('dispersion must be a finite positive scalar or {} finite positive values'.format(n))
        phi = np.full(n, phi[0]) if phi.size == 1 else phi.copy()
        if censoring is None:
            status = np.zeros(n, dtype=np.int32)
        else:
            c = np.asarray(censoring).ravel()
            if c.size != n or not np.all(np.isin(c, (-1, 0, 1))):
                raise ValueError('censoring must be None or {} values in (-1, 0, 1): -1 left-censored, 0 observed, +1 right-censored'.format(n))
            status = c.astype(np.int32)
        if offset is not None:
            offset = _row_vector(offset, n, 'offset')
        if z is None:
            z = np.ones((n, 1))
        super().__init__(par, x, y, z, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)
        self._phi, self._offset, self._status = phi, offset, status
        self._observed = status == 0
        self.ctx.set_offset(offset)
        self.ctx.set_dispersion(phi)
        self.ctx.set_censoring(status)
        self._declare_dispersion(phi)

    censoring = property(lambda self: self._status.copy())

    # ---- the precision as a hyper-parameter ----------------------------------------------------------------
    def _push_dispersion(self, phi):
        self.ctx.set_dispersion(phi)

    def _dispersion_entry(self, point):
        return self.ctx.glmm_censnormal_dispersion_terms(*point)

    def log_norm_const_dispersion(self):
        """(first, second) derivative in lambda of `log_norm_const()` at the current weights: (sum over the observed rows of w / 2, 0)."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        return 0.5 * float(np.sum(w[self._observed])), 0.0

    # ---- the device entries -------------------------------------------------------------------------------------------------
    def _terms(self, *point, **want):
        return self.ctx.glmm_censnormal_terms(*point, **want)

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_censnormal_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_censnormal_group_influence(*point_and_operand)

    def _row_psi_derivs(self, rho, s):
        """(E h', E h'' / 2) at rho + o by the rule the kernels use.  `cross_hessian` of the base class subtracts its `_y` from the
        first value; a1' of this model has no such term, so y is ADDED here, as the probit and cloglog links do ((a1' + y) - y
        differs from a1' by an ulp of |y| at most)."""
        if self._offset is not None:
            rho = rho + self._offset
        a1, a2 = censnormal_row_derivs(rho, s, self._y, self._phi, self._status, self.gh_x, self.gh_w)
        return a1 + self._y, a2

    # ---- predictions: the latent mean, which needs neither trials nor a status nor the precision ----------------------------
    def _predict_rows_of(self, newdata, n0, n1):
        if newdata is not None:
            for key in ('trials', 'censoring'):
                if key in newdata:
                    raise ValueError('newdata has the keys x, z, groups, offset, dispersion (got {}): the latent mean is predicted, '
                                     'which has neither trials nor a status'.format(key))
            newdata = {k: a for k, a in newdata.items() if k != 'dispersion'}    # accepted and not needed: the mean does not use it
        return super()._predict_rows_of(newdata, n0, n1)

    def _predict_entry(self, point, cov_beta, window, rows):
        if window is not None:
            return self.ctx.glmm_censnormal_predict(*point, cov_beta, n0=window[0], n1=window[1])
        return self.ctx.glmm_censnormal_predict(*point, cov_beta, new=rows[:4])

    def _response_mean(self, rho, s, trials):
        return censnormal_response_mean(rho, s)

    def log_norm_const(self):
        """sum over the OBSERVED rows of w_n [log(phi_n) / 2 - log(2 pi) / 2] at the current weights, the part of the Gaussian
        log-density that the value drops (a censored row's term is its log-probability whole): -ELBO(phi) = value -
        log_norm_const() + KL terms that do not depend on phi, so two precisions are compared by value - log_norm_const()."""
        w = np.asarray(self.weights_par.get_vector(), dtype=np.float64).ravel()
        o = self._observed
        return float(np.sum(w[o] * (0.5 * np.log(self._phi[o]) - 0.9189385332046727)))

"""Independent fp64 torch reference of `TruncatedNegBinomialGLMMObjective`, shared by the CPU and GPU tests,
in the style of tests/glmm_ztpoisson_reference.py.

The prior and entropy terms are `glmm_slopes_reference.kl_vec` with zero weights.  With eta = t - log phi the data term is

    sum_n w_n [ (y_n + phi_n) E softplus(eta) - y_n rho_n + E g(eta) ],   eta ~ N(rho_n, s_n),
    rho_n = o_n - log phi_n + x_n . m + z_n . e_g(n),        g(eta) = log(1 - exp(-phi softplus(eta)))  (the log of 1 - P(y = 0))

The first two terms are `glmm_binomial_reference`'s binomial term with trials y + phi and the offset o - log phi (its `psi`); E g is
the `deg`-node Gauss-Hermite sum of `torch.log(-torch.expm1(-phi * softplus(eta)))`, and its derivatives are defined by Stein's
identity on the same nodes (`_EG`), g^(k) being taken by k nested autograd passes -- no chain-rule recurrences anywhere.

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import math

import numpy as np
import torch

import glmm_binomial_reference as bref
import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)
from glmm_ztpoisson_reference import dk, _rule
from lmvn_reference import psi

GH_DEG = 20


def softplus(t):
    """log(1 + e^t) without the linear branch of torch.nn.functional.softplus past t = 20 (whose second derivative is 0, not 2e-9)."""
    return torch.logaddexp(torch.zeros_like(t), t)


LOG_X_SMALL, V_SMALL = math.log(1e-4), 0.01
_M = (-1.0 / 2.0, 5.0 / 24.0, -1.0 / 8.0, 251.0 / 2880.0, -19.0 / 288.0, 19087.0 / 362880.0)


def g_of(phi):
    """g(.; phi) as a function of eta: log(1 - exp(-phi softplus(eta))).  Nested autograd of the plain expression sums terms of order
    1 to a result of order e^eta and loses relative accuracy as eta -> -inf (1e-2 in the fourth derivative at eta = -30, measured
    against mpmath; 9e-11 at eta = -12).  Where x = e^eta < 1e-4 and v = phi softplus(eta) < 0.01 the reference therefore differentiates
        log phi + eta + log(log1p(x) / x) + log((1 - e^-v) / v)
      = log phi + eta + (-x / 2 + 5 x^2 / 24 - x^3 / 8 + 251 x^4 / 2880 - 19 x^5 / 288 + 19087 x^6 / 362880)
                      + (-v / 2 + v^2 / 24 - v^4 / 2880 + v^6 / 181440 - v^8 / 9676800)
    -- two polynomials without cancellation; the next terms are below 1e-17 of the result.  The polynomials are evaluated on the corner's own elements and scattered
    into the plain expression, which is finite there (its values and derivatives at those elements are dropped)."""
    def g(t):
        big = torch.log(-torch.expm1(-phi * softplus(t)))
        with torch.no_grad():
            corner = (t < LOG_X_SMALL) & (phi * softplus(t) < V_SMALL)
        if not bool(corner.any()):
            return big
        ph = phi * torch.ones_like(t)
        # the polynomials on the corner's own elements only: nested autograd pays for every operation four times over
        tc, pc = t[corner], ph[corner]
        x = torch.exp(tc)
        v = pc * torch.log1p(x)
        q = v * v
        m = x * (_M[0] + x * (_M[1] + x * (_M[2] + x * (_M[3] + x * (_M[4] + x * _M[5])))))
        el = v * (-0.5 + v * (1.0 / 24.0 + q * (-1.0 / 2880.0 + q * (1.0 / 181440.0 - q / 9676800.0))))
        return big.masked_scatter(corner, torch.log(pc) + tc + m + el)
    return g


def expected_g(mu, s, phi, k, deg=GH_DEG):
    """E g^(k) at eta ~ N(mu, s) on the nodes; phi one value per row."""
    t, wts = _rule(mu, s, deg)
    return (dk(g_of(phi[:, None]), t, k) * wts[None, :]).sum(1)


def expected_sp(mu, s, k, deg=GH_DEG):
    """E softplus^(k) on the same nodes, by nested autograd."""
    t, wts = _rule(mu, s, deg)
    return (dk(softplus, t, k) * wts[None, :]).sum(1)


class _EG(torch.autograd.Function):
    """E g^(k), differentiated in (mu, s) by Stein's identity on the same nodes, to any order."""
    @staticmethod
    def forward(ctx, mu, s, phi, deg, k):
        ctx.save_for_backward(mu, s, phi)
        ctx.deg, ctx.k = deg, k
        return expected_g(mu, s, phi, k, deg)

    @staticmethod
    def backward(ctx, go):
        mu, s, phi = ctx.saved_tensors
        return go * _EG.apply(mu, s, phi, ctx.deg, ctx.k + 1), go * 0.5 * _EG.apply(mu, s, phi, ctx.deg, ctx.k + 2), None, None, None


def data(eta, x, y, z, w, o, phi, gid, G, deg=GH_DEG):
    rho, s = bref._rho_s(eta, x, z, o - torch.log(phi), gid, G)
    return (w * ((y + phi) * psi(rho, s, deg) - y * rho + _EG.apply(rho, s, phi, deg, 0))).sum()


def _priors(eta, x, y, z, w, gid, G, hyp):
    return sref.kl_vec(eta, x, y, z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_vec(eta, x, y, z, w, o, phi, gid, G, hyp, deg=GH_DEG):
    return data(eta, x, y, z, w, o, phi, gid, G, deg) + _priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, phi, gid, G, hyp, deg=GH_DEG):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, phi, gid, G, hyp, deg)


def targs(x, y, z, w, o, phi, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """The arguments of `kl_vec` / `kl_free` behind the point; o is the RAW offset."""
    return bref.targs(x, y, z, w, o, phi, gid, G, hyp) + (deg,)


def ztnb_draw(rng, mu, phi):
    """Zero-truncated NB2 draws with mean mu and dispersion phi (numpy) by inversion of the untruncated CDF on (P(0), 1)."""
    from scipy.stats import nbinom
    mu, phi = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    pr = phi / (phi + mu)
    p0 = pr ** phi
    u = np.minimum(p0 + rng.uniform(size=mu.shape) * (1.0 - p0), 1.0 - 1e-12)
    return np.maximum(nbinom.ppf(u, phi, pr), 1.0)


def problem(N, P, K, G, seed, phi=1.7, zero_weights=False, **kw):
    """x, z, w, gid, o and the point of `glmm_poisson_reference.problem`; phi a scalar, or 'vector' for one value per row,
    log-uniform on [0.05, 1e3] with phi[0] = 0.05 and phi[1] = 1e3 (N >= 4); y >= 1 drawn from the zero-truncated NB2 law at
    o + x beta + z . u.  With N >= 4: y[0] = y[1] = 1 and y[2] = 57, a large count.  zero_weights: every fifth weight is 0.
    Returns (x, y, z, w, gid, o, phi (N), free)."""
    import glmm_poisson_reference as pref
    x, _, z, w, gid, o, free = pref.problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 6])
    if isinstance(phi, str):
        ph = np.exp(rng.uniform(np.log(0.05), np.log(1e3), size=N))
        if N >= 4:
            ph[0], ph[1] = 0.05, 1e3
    else:
        ph = np.full(N, float(phi))
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    y = ztnb_draw(rng, np.exp(o + x @ beta + (z * u[gid]).sum(1)), ph)
    if N >= 4:
        y[0], y[1], y[2] = 1.0, 1.0, 57.0
    else:
        y[0] = 1.0
    if zero_weights:
        w = w.copy()
        w[::5] = 0.0
    return x, y, z, w, gid, o, ph, free


def _t(a):
    return torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)))


def eh_coefs(rho, s, y, phi, deg=GH_DEG):
    """E [H + y eta], E [H' + y], E H'', E H''', E H'''' (5 x n, numpy) by the reference's rule, rho on the shifted scale: the
    moments (y + phi) E sp^(k) + E g^(k)."""
    rho, s, y, phi = (_t(a) for a in np.broadcast_arrays(rho, s, y, phi))
    return np.stack([((y + phi) * expected_sp(rho, s, k, deg) + expected_g(rho, s, phi, k, deg)).numpy() for k in range(5)])


def nb_coefs(rho, s, y, phi, deg=GH_DEG):
    """The NB2 moments alone, (y + phi) E sp^(k), k = 0..4 (5 x n, numpy)."""
    rho, s, y, phi = (_t(a) for a in np.broadcast_arrays(rho, s, y, phi))
    return np.stack([((y + phi) * expected_sp(rho, s, k, deg)).numpy() for k in range(5)])


def response_mean(rho, s, phi, deg=GH_DEG, closed=True):
    """E [mu / (1 - P0)], mu = e^t = phi e^eta, eta ~ N(rho, s): phi exp(rho + s / 2) plus the node sum of mu exp(-v) / (1 - exp(-v))
    (numpy).  closed=False takes the e^t part on the nodes too (what the model does NOT do); closed=None returns the node sum alone."""
    rho, s, phi = (_t(a) for a in np.broadcast_arrays(rho, s, phi))
    t, wts = _rule(rho, s, deg)
    v = phi[:, None] * softplus(t)
    mu = phi[:, None] * torch.exp(t)
    node = torch.where(v > 700.0, torch.zeros_like(v), mu * torch.exp(-v) / -torch.expm1(-v))
    if closed is None:
        return (node * wts[None, :]).sum(1).numpy()
    if not closed:
        return ((mu + node) * wts[None, :]).sum(1).numpy()
    return (phi * torch.exp(rho + 0.5 * s) + (node * wts[None, :]).sum(1)).numpy()

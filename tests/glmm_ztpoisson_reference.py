"""Independent fp64 torch reference of `TruncatedPoissonGLMMObjective`, shared by the CPU and GPU tests, in
the style of tests/glmm_link_reference.py.

The prior and entropy terms are `glmm_slopes_reference.kl_vec` with zero weights.  The data term is

    sum_n w_n [ E A(t) - y_n rho_n ],  t ~ N(rho_n, s_n),  rho_n = o_n + x_n . m + z_n . e_g(n),
    A(t) = log(exp(e^t) - 1) = e^t + B(t),   B(t) = log(-expm1(-exp(t)))

with E e^t = exp(rho + s / 2) and E B by the `deg`-node Gauss-Hermite sum.  Derivatives are defined by Stein's identity on the same
nodes (`_EA`: d_rho E A^(k) = E A^(k+1), d_s E A^(k) = E A^(k+2) / 2), B^(k) being taken by k nested autograd passes of
torch.log / torch.expm1 / torch.exp -- no r = u / expm1(u) recurrences anywhere.

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import math

import numpy as np
import torch

import glmm_poisson_reference as pref
import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)

GH_DEG = 20


U_SMALL = 0.05


def B(t):
    """The part of A that goes on the nodes: log(1 - exp(-e^t)), u = e^t.  Nested autograd of the plain expression sums terms of
    order 1 to a result of order u and loses relative accuracy as u -> 0 (2.7e-10 in B'''' at t = -12, measured against mpmath:
    above the 1e-10 the CPU test allows the reference).  Below U_SMALL the reference therefore differentiates
    t + log((1 - e^-u) / u) = t - u / 2 + u^2 / 24 - u^4 / 2880 + u^6 / 181440 - u^8 / 9676800, the series of -u / 2 +
    log(sinh(u / 2) / (u / 2)) -- a polynomial in u without cancellation; the next term is below 2e-22 there.  Both branches see a
    clamped argument, so that the branch not taken stays finite in every derivative."""
    u = torch.exp(t)
    us, ub = torch.clamp(u, max=U_SMALL), torch.clamp(u, min=U_SMALL)
    q = us * us
    small = t + us * (-0.5 + us * (1.0 / 24.0 + q * (-1.0 / 2880.0 + q * (1.0 / 181440.0 - q / 9676800.0))))
    return torch.where(u < U_SMALL, small, torch.log(-torch.expm1(-ub)))


def A(t):
    return torch.exp(t) + B(t)


def dk(fn, t, k):
    """k-th derivative of fn at t by k nested autograd passes."""
    with torch.enable_grad():
        tt = t.detach().requires_grad_(True)
        h = fn(tt)
        for _ in range(k):
            h, = torch.autograd.grad(h.sum(), tt, create_graph=True)
    return h.detach()


def _rule(mu, s, deg):
    gx, gw = np.polynomial.hermite.hermgauss(deg)
    nodes = torch.tensor(math.sqrt(2.0) * gx, dtype=torch.float64)
    wts = torch.tensor(gw / math.sqrt(math.pi), dtype=torch.float64)
    return mu[:, None] + torch.sqrt(torch.clamp(s, min=0.0))[:, None] * nodes[None, :], wts


def expected_dk(mu, s, k, deg=GH_DEG, closed=True):
    """E A^(k) at t ~ N(mu, s): exp(mu + s / 2) plus E B^(k) on the nodes.  closed=False takes the e^t part on the nodes too (what
    the model does NOT do; the tests use it to show that an input tells the two apart)."""
    t, wts = _rule(mu, s, deg)
    if not closed:
        return (dk(A, t, k) * wts[None, :]).sum(1)
    return torch.exp(mu + 0.5 * s) + (dk(B, t, k) * wts[None, :]).sum(1)


class _EA(torch.autograd.Function):
    """E A^(k), differentiated in (mu, s) by Stein's identity on the same nodes, to any order."""
    @staticmethod
    def forward(ctx, mu, s, deg, k):
        ctx.save_for_backward(mu, s)
        ctx.deg, ctx.k = deg, k
        return expected_dk(mu, s, k, deg)

    @staticmethod
    def backward(ctx, go):
        mu, s = ctx.saved_tensors
        return go * _EA.apply(mu, s, ctx.deg, ctx.k + 1), go * 0.5 * _EA.apply(mu, s, ctx.deg, ctx.k + 2), None, None


def data(eta, x, y, z, w, o, gid, G, deg=GH_DEG):
    rho, s = pref._rho_s(eta, x, z, o, gid, G)
    return (w * (_EA.apply(rho, s, deg, 0) - y * rho)).sum()


def _priors(eta, x, y, z, w, gid, G, hyp):
    return sref.kl_vec(eta, x, y, z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_vec(eta, x, y, z, w, o, gid, G, hyp, deg=GH_DEG):
    return data(eta, x, y, z, w, o, gid, G, deg) + _priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, gid, G, hyp, deg=GH_DEG):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, gid, G, hyp, deg)


def targs(x, y, z, w, o, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """The arguments of `kl_vec` / `kl_free` behind the point."""
    return pref.targs(x, y, z, w, o, gid, G, hyp) + (deg,)


def ztp_draw(rng, lam):
    """Zero-truncated Poisson draws with rate lam (numpy) by inversion of the untruncated CDF on (P(0), 1)."""
    from scipy.stats import poisson
    lam = np.asarray(lam, dtype=np.float64)
    p0 = np.exp(-lam)
    return np.maximum(poisson.ppf(p0 + rng.uniform(size=lam.shape) * (1.0 - p0), lam), 1.0)


def problem(N, P, K, G, seed, zero_weights=False, **kw):
    """x, z, w, gid, o and the point of `glmm_poisson_reference.problem`, y >= 1 drawn from the zero-truncated Poisson law at
    o + x beta + z . u.  With N >= 4: y[0] = y[1] = 1 and y[2] = 57, a large count.  zero_weights: every fifth weight is 0.
    Returns (x, y, z, w, gid, o, free)."""
    x, _, z, w, gid, o, free = pref.problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 5])
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    y = ztp_draw(rng, np.exp(o + x @ beta + (z * u[gid]).sum(1)))
    if N >= 4:
        y[0], y[1], y[2] = 1.0, 1.0, 57.0
    else:
        y[0] = 1.0
    if zero_weights:
        w = w.copy()
        w[::5] = 0.0
    return x, y, z, w, gid, o, free


def ea_coefs(rho, s, deg=GH_DEG, closed=True):
    """E A^(k), k = 0..4 (5 x n, numpy) by the reference's rule."""
    t = lambda a: torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)))
    return np.stack([expected_dk(t(rho), t(s), k, deg, closed).numpy() for k in range(5)])


def response_mean(rho, s, deg=GH_DEG):
    """E [lambda / (1 - exp(-lambda))], lambda = e^t: exp(rho + s / 2) plus the node sum of u / expm1(u) (numpy)."""
    rho, s = (torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))) for a in (rho, s))
    t, wts = _rule(rho, s, deg)
    u = torch.exp(t)
    return (torch.exp(rho + 0.5 * s) + ((u / torch.expm1(u)) * wts[None, :]).sum(1)).numpy()

"""Independent fp64 torch reference of `BetaGLMMObjective`, shared by the CPU and GPU tests, in the style of
tests/glmm_ztnegbin_reference.py.

The prior and entropy terms are `glmm_slopes_reference.kl_vec` with zero weights.  With l = logit(y) the data term is

    sum_n w_n E h(t),   t ~ N(rho_n, s_n),   rho_n = o_n + x_n . m + z_n . e_g(n),
    h(t) = lgamma(phi sigma(t)) + lgamma(phi sigma(-t)) - phi l sigma(t)

on the `deg`-node Gauss-Hermite rule, and its derivatives are defined by Stein's identity on the same nodes (`_EH`), h^(k) being
taken by k nested autograd passes -- no Faa di Bruno and no polygamma series anywhere.

How h is WRITTEN matters (measured against mpmath in tests/test_glmm_beta_host_math.py).  Nested autograd of the expression above
loses every digit of h'', h''', h'''' in the tails (it returns h'' = -1.7e-12 at t = -30), and so does any form that goes through
`torch.sigmoid`, whose backward is y (1 - y) on a saturated y.  The reference differentiates

    h(t) = softplus(t) + softplus(-t) - 2 log phi + lgamma(1 + phi mu) + lgamma(1 + phi nu) - phi l mu,
    mu = exp(-softplus(-t)),   nu = 1 - mu = exp(-softplus(t)),   softplus = logaddexp(0, .)

(lgamma(x) = lgamma(1 + x) - log x on both arguments).  One more thing was measured: autograd's second derivative of `torch.lgamma`
is torch's trigamma, polygamma(1, .), which is good to 5e-10 only (six recurrence steps and a series cut at B_6), while lgamma,
digamma, polygamma(n >= 2) and the Hurwitz zeta function are good to 1e-14 or better.  With it h'' .. h'''' were off by 1e-9 to 4e-7
in the BULK.  `lgamma` below is therefore `torch.lgamma` with its derivative chain spelled out -- digamma, then
psi^(n) = (-1)^(n+1) n! zeta(n + 1, .) from `torch.special.zeta` -- and nothing else changes: the derivatives of h are still taken by
nested autograd.  Against mpmath the reference then meets the 1e-10 cap on the whole grid of tests/test_glmm_beta_host_math.py; the
GPU data sets stay at |rho| <= 12 all the same, and the far tails are pinned on the CPU against mpmath, not through torch.

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import math

import numpy as np
import torch

import glmm_binomial_reference as bref
import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)
from glmm_ztpoisson_reference import dk, _rule
from glmm_ztnegbin_reference import softplus

GH_DEG = 20


def logit(y):
    return torch.log(y) - torch.log1p(-y)


class _LGamma(torch.autograd.Function):
    """lgamma (n = 0), digamma (n = 1) and psi^(n-1) = (-1)^n (n - 1)! zeta(n, x) (n >= 2), each the derivative of the one before."""
    @staticmethod
    def forward(ctx, x, n):
        ctx.save_for_backward(x)
        ctx.n = n
        if n == 0:
            return torch.lgamma(x)
        if n == 1:
            return torch.digamma(x)
        return (-1.0) ** n * math.factorial(n - 1) * torch.special.zeta(torch.tensor(float(n), dtype=x.dtype), x)

    @staticmethod
    def backward(ctx, go):
        x, = ctx.saved_tensors
        return go * _LGamma.apply(x, ctx.n + 1), None


def lgamma(x):
    return _LGamma.apply(x, 0)


def h_of(phi, l):
    """h(.; phi, l) as a function of t, in the shifted form of the module docstring."""
    def h(t):
        mu, nu = torch.exp(-softplus(-t)), torch.exp(-softplus(t))
        return (softplus(t) + softplus(-t) - 2.0 * torch.log(phi) + lgamma(1.0 + phi * mu) + lgamma(1.0 + phi * nu)
                - phi * l * mu)
    return h


def expected_h(mu, s, phi, l, k, deg=GH_DEG):
    """E h^(k) at t ~ N(mu, s) on the nodes; phi and l one value per row."""
    t, wts = _rule(mu, s, deg)
    return (dk(h_of(phi[:, None], l[:, None]), t, k) * wts[None, :]).sum(1)


class _EH(torch.autograd.Function):
    """E h^(k), differentiated in (mu, s) by Stein's identity on the same nodes, to any order."""
    @staticmethod
    def forward(ctx, mu, s, phi, l, deg, k):
        ctx.save_for_backward(mu, s, phi, l)
        ctx.deg, ctx.k = deg, k
        return expected_h(mu, s, phi, l, k, deg)

    @staticmethod
    def backward(ctx, go):
        mu, s, phi, l = ctx.saved_tensors
        return (go * _EH.apply(mu, s, phi, l, ctx.deg, ctx.k + 1), go * 0.5 * _EH.apply(mu, s, phi, l, ctx.deg, ctx.k + 2),
                None, None, None, None)


def data(eta, x, y, z, w, o, phi, gid, G, deg=GH_DEG):
    """y: the proportions themselves, strictly inside (0, 1)."""
    rho, s = bref._rho_s(eta, x, z, o, gid, G)
    return (w * _EH.apply(rho, s, phi, logit(y), deg, 0)).sum()


def _priors(eta, x, y, z, w, gid, G, hyp):
    return sref.kl_vec(eta, x, y, z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_vec(eta, x, y, z, w, o, phi, gid, G, hyp, deg=GH_DEG):
    return data(eta, x, y, z, w, o, phi, gid, G, deg) + _priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, phi, gid, G, hyp, deg=GH_DEG):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, phi, gid, G, hyp, deg)


def targs(x, y, z, w, o, phi, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """The arguments of `kl_vec` / `kl_free` behind the point; o is the offset on the logit scale."""
    return bref.targs(x, y, z, w, o, phi, gid, G, hyp) + (deg,)


def log_norm_const(y, phi, w):
    """sum w [lgamma(phi) + (phi - 1) log(1 - y) - log y] (numpy), what the value drops."""
    from scipy.special import gammaln
    return float(np.sum(w * (gammaln(phi) + (phi - 1.0) * np.log1p(-y) - np.log(y))))


PROBES = (1e-12, 1.0 - 1e-12, 0.5)


def problem(N, P, K, G, seed, phi=7.5, zero_weights=False, **kw):
    """x, z, w, gid, o and the point of `glmm_binomial_reference.problem`; phi a scalar (>= 0.5: smaller values put Beta draws at
    exactly 0 or 1 in fp64), or 'vector' for one value per row, log-uniform on [0.5, 1e3] with phi[3] = 0.5 and phi[4] = 1e3
    (N >= 5: the two ends sit behind the probe rows, whose own phi stays a draw); y drawn from Beta(mu phi, (1 - mu) phi) at mu = sigma(o + x beta + z . u), every draw strictly interior.  Then three
    probe rows (N >= 4): y[0] = 1e-12, y[1] = 1 - 1e-12, y[2] = 0.5.  zero_weights: every fifth weight
    is 0.  Returns (x, y, z, w, gid, o, phi (N), free)."""
    x, _, z, w, gid, o, _, free = bref.problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 7])
    if isinstance(phi, str):
        ph = np.exp(rng.uniform(np.log(0.5), np.log(1e3), size=N))
        if N >= 5:
            ph[3], ph[4] = 0.5, 1e3
    else:
        ph = np.full(N, float(phi))
    assert ph.min() >= 0.5
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    mu = 1.0 / (1.0 + np.exp(-(o + x @ beta + (z * u[gid]).sum(1))))
    y = rng.beta(mu * ph, (1.0 - mu) * ph)
    assert np.all((y > 0.0) & (y < 1.0)), 'a Beta draw is not strictly interior'
    if N >= 4:
        y[0], y[1], y[2] = PROBES
    if zero_weights:
        w = w.copy()
        w[::5] = 0.0
    return x, y, z, w, gid, o, ph, free


def _t(a):
    return torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)))


def eh_coefs(rho, s, l, phi, deg=GH_DEG):
    """E h^(k), k = 0..4 (5 x n, numpy) by the reference's rule; l = logit(y)."""
    rho, s, l, phi = (_t(a) for a in np.broadcast_arrays(rho, s, l, phi))
    return np.stack([expected_h(rho, s, phi, l, k, deg).numpy() for k in range(5)])


def h_derivs(t, phi, l):
    """h^(k)(t), k = 0..4 (5 x n, numpy) by nested autograd of the reference's h."""
    t, phi, l = (_t(a) for a in np.broadcast_arrays(t, phi, l))
    return np.stack([dk(h_of(phi, l), t, k).numpy() for k in range(5)])


def response_mean(rho, s, deg=GH_DEG):
    """E sigma(t), t ~ N(rho, s), on the nodes (numpy)."""
    rho, s = (_t(a) for a in np.broadcast_arrays(rho, s))
    t, wts = _rule(rho, s, deg)
    return (torch.exp(-softplus(-t)) * wts[None, :]).sum(1).numpy()

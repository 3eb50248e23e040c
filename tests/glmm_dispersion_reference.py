"""Independent fp64 torch reference (CPU) of the log-dispersion derivatives of `BetaGLMMObjective` and `NegBinomialGLMMObjective`
(DESIGN.md section 41), shared by tests/test_glmm_dispersion_host_math.py and tests/test_gpu_glmm_dispersion.py.

The dispersion is phi_n = exp(lambda) phi0_n and the objective that depends on lambda is

    F(theta, lambda) = sum_n w_n E h(t; phi_n) - lnc(phi) + (priors and entropy, free of phi),   t ~ N(rho_n, s_n),

with the row terms of tests/glmm_beta_reference.py (`h_of`, the shifted form, its own `lgamma` chain -- not `torch.lgamma`, whose
trigamma is good to 5e-10 only) and of tests/glmm_binomial_reference.py (the NB2 term in the form the model evaluates,
(y + phi) softplus(t - log phi) - y (t - log phi): it differs from that file's (y + phi) logaddexp(log phi, t) - y t by
sum w phi log phi, which depends on phi and belongs to neither `value` nor `log_norm_const`).  The expectations of those files are
custom autograd functions closed in phi (`_EH`, `_ENB`); here E is the PLAIN Gauss-Hermite sum on the same nodes, with phi a tensor
that requires grad: one lambda PER ROW (all equal), so that a single backward pass gives the per-row derivative.

The model defines its gradient in (rho, s) by Stein's identity on the nodes, d_rho E h = E h', d_s E h = E h'' / 2, h^(k) by nested
autograd here; J_lambda is the derivative in lambda of THAT gradient:  per row a1 = d_lambda E h', a2 = d_lambda E h'' / 2, chained to
theta through rho_n(theta) and s_n(theta) by autograd.  Nothing here uses a closed formula of the package."""
import math

import numpy as np
import torch

import glmm_beta_reference as beta_ref
import glmm_binomial_reference as bref
from glmm_reference import value_grad_hess
from glmm_slopes_reference import free_to_vec
from glmm_ztnegbin_reference import softplus
from glmm_ztpoisson_reference import _rule, dk

GH_DEG = 20


def beta_h(lphi, l, y):
    """h(.; phi, l) of the Beta model at phi = exp(lphi); y is not used (l = logit y)."""
    return beta_ref.h_of(torch.exp(lphi), l)


def negbin_h(lphi, l, y):
    """The NB2 row term as the model evaluates it, at phi = exp(lphi); l is not used.  eta = t - lphi is LINEAR in lambda: formed as
    t - log(exp(lambda) phi0) its second derivative in lambda is (1 / phi^2) phi phi - (1 / phi) phi, an ulp instead of 0, and that ulp
    times y = 400 is all of h_ll at eta = -38 (measured against mpmath: tests/test_glmm_dispersion_host_math.py)."""
    def h(t):
        eta = t - lphi
        return (y + torch.exp(lphi)) * softplus(eta) - y * eta
    return h


def beta_lnc(phi, y, w):
    return (w * (beta_ref.lgamma(phi) + (phi - 1.0) * torch.log1p(-y) - torch.log(y))).sum()


def negbin_lnc(phi, y, w):
    return (w * (beta_ref.lgamma(y + phi) - beta_ref.lgamma(phi) - beta_ref.lgamma(y + 1.0))).sum()


FAMILY = {'beta': (beta_h, beta_lnc), 'negbin': (negbin_h, negbin_lnc)}


def _dt(fn, t, k):
    """k-th derivative of fn in t by k nested autograd passes, the graph KEPT (the result is differentiated in lambda next)."""
    tt = t.detach().requires_grad_(True)
    h = fn(tt)
    for _ in range(k):
        h, = torch.autograd.grad(h.sum(), tt, create_graph=True)
    return h


def _t(a):
    return torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)))


def row_pieces(family, rho, s, y, phi0, lam=0.0, deg=GH_DEG):
    """Per row (numpy, 5 x n): E h_l, E d_t h_l, E d_t^2 h_l, E h_ll and E h itself at phi = exp(lam) phi0, t ~ N(rho, s): the plain
    Gauss-Hermite sums of h, h', h'' differentiated in a per-row lambda by autograd."""
    rho, s, y, phi0 = (_t(a) for a in np.broadcast_arrays(rho, s, y, phi0))
    h_of = FAMILY[family][0]
    lam_n = torch.full_like(rho, float(lam)).requires_grad_(True)
    lphi = lam_n + torch.log(phi0)
    l = torch.log(y) - torch.log1p(-y) if family == 'beta' else y
    t, wts = _rule(rho, s, deg)
    fn = h_of(lphi[:, None], l[:, None], y[:, None])
    E = [(_dt(fn, t, k) * wts[None, :]).sum(1) for k in range(3)]
    d0, = torch.autograd.grad(E[0].sum(), lam_n, create_graph=True)
    d00, = torch.autograd.grad(d0.sum(), lam_n, retain_graph=True)
    d1, = torch.autograd.grad(E[1].sum(), lam_n, retain_graph=True)
    d2, = torch.autograd.grad(E[2].sum(), lam_n, retain_graph=True)
    return np.stack([a.detach().numpy() for a in (d0, d1, d2, d00, E[0])])


def lnc_derivs(family, y, phi0, w, lam=0.0):
    """(lnc, lnc_l, lnc_ll) at phi = exp(lam) phi0 by autograd through the reference's own lgamma chain."""
    y, phi0, w = (_t(a) for a in np.broadcast_arrays(y, phi0, w))
    lt = torch.tensor(float(lam), dtype=torch.float64, requires_grad=True)
    c = FAMILY[family][1](torch.exp(lt) * phi0, y, w)
    c1, = torch.autograd.grad(c, lt, create_graph=True)
    c2, = torch.autograd.grad(c1, lt)
    return float(c.detach()), float(c1.detach()), float(c2)


def dispersion_terms(family, x, y, z, w, o, phi0, gid, G, point, lam=0.0, is_free=True, deg=GH_DEG):
    """dict(F (without priors), d1 = F_l, d2 = F_ll, cross = J_l in the coordinates of `point`, scale = sum w |E h_l| + |lnc_l|) of
    the reference; o is the RAW offset."""
    P, K = x.shape[1], z.shape[1]
    tx, tz, to = torch.tensor(x), torch.tensor(z), torch.tensor(np.asarray(o, dtype=np.float64))
    tg = torch.tensor(np.asarray(gid, dtype=np.int64))
    p = torch.tensor(np.asarray(point, dtype=np.float64), requires_grad=True)
    eta = free_to_vec(p, P, K, G) if is_free else p
    rho, s = bref._rho_s(eta, tx, tz, to, tg, G)
    rp = row_pieces(family, rho.detach().numpy(), s.detach().numpy(), y, phi0, lam, deg)
    tw = torch.tensor(np.asarray(w, dtype=np.float64))
    lin = (tw * (torch.tensor(rp[1]) * rho + 0.5 * torch.tensor(rp[2]) * s)).sum()
    J, = torch.autograd.grad(lin, p)
    c, c1, c2 = lnc_derivs(family, y, phi0, w, lam)
    return dict(F=float(np.sum(w * rp[4])) - c, d1=float(np.sum(w * rp[0])) - c1, d2=float(np.sum(w * rp[3])) - c2, cross=J.numpy(),
                scale=float(np.sum(np.abs(w * rp[0]))) + abs(c1), scale2=float(np.sum(np.abs(w * rp[3]))) + abs(c2))


class _ENB(torch.autograd.Function):
    """`glmm_binomial_reference._ENB` on a rule of `deg` nodes: E d^k/dt^k logaddexp(log phi, t), differentiated in (mu, s) by
    Stein's identity on the same nodes."""
    @staticmethod
    def forward(ctx, mu, s, lphi, k, deg):
        ctx.save_for_backward(mu, s, lphi)
        ctx.k, ctx.deg = k, deg
        t, wts = _rule(mu, s, deg)
        return (dk(lambda tt: torch.logaddexp(lphi[:, None].expand_as(tt), tt), t, k) * wts[None, :]).sum(1)

    @staticmethod
    def backward(ctx, go):
        mu, s, lphi = ctx.saved_tensors
        return go * _ENB.apply(mu, s, lphi, ctx.k + 1, ctx.deg), go * 0.5 * _ENB.apply(mu, s, lphi, ctx.k + 2, ctx.deg), None, None, None


def _nb_kl_free(free, x, y, z, w, o, phi, gid, G, hyp, deg):
    eta = free_to_vec(free, x.shape[1], z.shape[1], G)
    rho, s = bref._rho_s(eta, x, z, o, gid, G)
    return (w * ((y + phi) * _ENB.apply(rho, s, torch.log(phi), 0, deg) - y * rho)).sum() + bref._priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(family, free, x, y, z, w, o, phi, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """(value, gradient, dense Hessian) of the model's whole objective (priors and entropy included; the NB2 value carries the
    constant sum w phi log phi of glmm_binomial_reference, which no derivative in theta sees) at phi, by the reference files' own
    functions; for the dense Hessian of the profile."""
    if family == 'beta':
        return value_grad_hess(beta_ref.kl_free, free, beta_ref.targs(x, y, z, w, o, phi, gid, G, hyp, deg))
    return value_grad_hess(_nb_kl_free, free, bref.targs(x, y, z, w, o, phi, gid, G, hyp) + (deg,))


def profile(family, x, y, z, w, o, phi0, gid, G, free, lam=0.0, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """(slope, curvature, d theta / d lambda, dense free Hessian) of the profiled objective at the free point: F_l,
    F_ll - J^T H^-1 J and -H^-1 J with the reference's dense Hessian (the NB2 reference runs on 20 nodes only)."""
    t = dispersion_terms(family, x, y, z, w, o, phi0, gid, G, free, lam, True, deg)
    H = kl_free(family, free, x, y, z, w, o, math.exp(lam) * np.asarray(phi0, dtype=np.float64), gid, G, hyp, deg)[2]
    dth = -np.linalg.solve(H, t['cross'])
    return t['d1'], t['d2'] + float(t['cross'] @ dth), dth, H


def simulate(family, N, P, K, G, seed, phi_true):
    """Data drawn from the model at a KNOWN dispersion, for the fits: x ~ N(0, 1 / P), z = [1 | 0.5 N(0, 1)], groups uniform, unit
    weights, no offset; Beta: y ~ Beta(mu phi, (1 - mu) phi) at mu = sigma(t); NB2: y ~ Poisson(Gamma(phi, mu / phi)) at
    mu = exp(1 + t); t = x beta + z u.  Returns (x, y, z, w, gid, o)."""
    rng = np.random.default_rng([seed, 41])
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), 0.5 * rng.normal(size=(N, K - 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    t = x @ (0.8 * rng.normal(size=P)) + (z * (0.5 * rng.normal(size=(G, K)))[gid]).sum(1)
    if family == 'beta':
        mu = 1.0 / (1.0 + np.exp(-t))
        y = rng.beta(mu * phi_true, (1.0 - mu) * phi_true)
        assert np.all((y > 0.0) & (y < 1.0))
    else:
        mu = np.exp(1.0 + t)
        y = rng.poisson(rng.gamma(phi_true, mu / phi_true)).astype(np.float64)
    return x, y, z, np.ones(N), gid, np.zeros(N)


def profile_optimum(family, x, y, z, w, o, phi0, gid, G, lam=0.0, free=None, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), tol=1e-9, log=None):
    """The reference's OWN profile optimum (lambda, theta): Newton on theta with the dense reference Hessian inside Newton on lambda
    with the profile slope and curvature (|step| <= 1), from the start (lam, free) -- plain Newton steps, so start near (a fitted
    point of the model under test is a fair start: the stationary point found is the reference's).  CPU, a minute per Hessian at
    N = 2000: for choosing a seed, not for the suite."""
    P, K = x.shape[1], z.shape[1]
    free = np.zeros(2 * P + 4 * K + 2 * G * K) if free is None else np.array(free, dtype=np.float64)
    phi0 = np.asarray(phi0, dtype=np.float64) * np.ones(x.shape[0])
    for _ in range(30):
        for _ in range(40):
            _, g, H = kl_free(family, free, x, y, z, w, o, math.exp(lam) * phi0, gid, G, hyp)
            if np.max(np.abs(g)) < 1e-8:
                break
            free = free - np.linalg.solve(H, g)
        t = dispersion_terms(family, x, y, z, w, o, phi0, gid, G, free, lam, True)
        dth = -np.linalg.solve(H, t['cross'])
        slope, curv = t['d1'], t['d2'] + float(t['cross'] @ dth)
        step = float(np.clip(-slope / curv if curv > 0 else -0.5 * np.sign(slope), -1.0, 1.0))
        if log:
            log(lam, slope, curv, step)
        if abs(step) < tol:
            break
        lam += step
        free = free + step * dth
    return lam, free

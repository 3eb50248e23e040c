"""Independent fp64 torch reference of `BinomialGLMMObjective(link='probit' | 'cloglog')`, shared by the CPU
and GPU tests, in the style of tests/glmm_binomial_reference.py.

The prior and entropy terms are `glmm_slopes_reference.kl_vec` with zero weights.  The data term is

    sum_n w_n E [ y_n h1(t) + (m_n - y_n) h0(t) ],  t ~ N(rho_n, s_n),  rho_n = o_n + x_n . m + z_n . e_g(n),
    probit:  h1 = -log_ndtr(t),  h0 = -log_ndtr(-t);      cloglog:  h1 = -log(-expm1(-exp(t))),  h0 = exp(t)

by the GH_DEG-node Gauss-Hermite sum of h1 (and of the probit h0); the cloglog E h0 is exp(rho + s / 2).  Derivatives are defined
by Stein's identity on the same nodes (`_EH`: d_rho E h^(k) = E h^(k+1), d_s E h^(k) = E h^(k+2) / 2), h^(k) being taken by k nested
autograd passes of torch.special.log_ndtr / torch.expm1 -- no closed Mills-ratio or r = u / expm1(u) formulas anywhere.

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import math

import numpy as np
import torch

import glmm_binomial_reference as bref
import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)

GH_DEG = bref.GH_DEG
LINKS = ('probit', 'cloglog')


def h1(link, t):
    return -torch.special.log_ndtr(t) if link == 'probit' else -torch.log(-torch.expm1(-torch.exp(t)))


def h0(link, t):
    return -torch.special.log_ndtr(-t) if link == 'probit' else torch.exp(t)


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


def expected_dk(link, which, mu, s, k, deg=GH_DEG):
    """E h1^(k) (which = 1) or E h0^(k) (which = 0) at t ~ N(mu, s): on the nodes, except the cloglog h0, exp(mu + s / 2)."""
    if which == 0 and link == 'cloglog':
        return torch.exp(mu + 0.5 * s)
    t, wts = _rule(mu, s, deg)
    fn = (lambda a: h1(link, a)) if which == 1 else (lambda a: h0(link, a))
    return (dk(fn, t, k) * wts[None, :]).sum(1)


class _EH(torch.autograd.Function):
    """y E h1^(k) + f E h0^(k), differentiated in (mu, s) by Stein's identity on the same nodes, to any order."""
    @staticmethod
    def forward(ctx, mu, s, y, f, link, k):
        ctx.save_for_backward(mu, s, y, f)
        ctx.link, ctx.k = link, k
        return y * expected_dk(link, 1, mu, s, k) + f * expected_dk(link, 0, mu, s, k)

    @staticmethod
    def backward(ctx, go):
        mu, s, y, f = ctx.saved_tensors
        return (go * _EH.apply(mu, s, y, f, ctx.link, ctx.k + 1), go * 0.5 * _EH.apply(mu, s, y, f, ctx.link, ctx.k + 2),
                None, None, None, None)


def data(eta, x, y, z, w, o, mt, gid, G, link):
    rho, s = bref._rho_s(eta, x, z, o, gid, G)
    return (w * _EH.apply(rho, s, y, mt - y, link, 0)).sum()


def kl_vec(eta, x, y, z, w, o, mt, gid, G, hyp, link):
    return data(eta, x, y, z, w, o, mt, gid, G, link) + bref._priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, mt, gid, G, hyp, link):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, mt, gid, G, hyp, link)


def targs(x, y, z, w, o, mt, gid, G, link, hyp=(1.0, 0.0, 1.0, 1.0, 1.0)):
    """The arguments of `kl_vec` / `kl_free` behind the point."""
    return bref.targs(x, y, z, w, o, mt, gid, G, hyp) + (link,)


def prob(link, t):
    """p(t) of the link, numpy."""
    from scipy.special import ndtr
    t = np.asarray(t, dtype=np.float64)
    return ndtr(t) if link == 'probit' else -np.expm1(-np.exp(t))


def problem(N, P, K, G, seed, link, **kw):
    """`glmm_binomial_reference.problem` with y ~ Binomial(m, p(o + x beta + z . u)) drawn under the link; with N >= 4 the rows 2
    and 3 get at least two trials, y[2] = 0 and y[3] = m[3] (next to m[0] = 0 and the Bernoulli row 1 of that problem).
    Returns (x, y, z, w, gid, o, m, free)."""
    x, _, z, w, gid, o, m, free = bref.problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 4])
    if N >= 4:
        m[2], m[3] = max(m[2], 2.0), max(m[3], 2.0)
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    y = rng.binomial(m.astype(np.int64), prob(link, o + x @ beta + (z * u[gid]).sum(1))).astype(np.float64)
    if N >= 4:
        y[2], y[3] = 0.0, m[3]
    return x, y, z, w, gid, o, m, free


def eh_coefs(link, rho, s, y, mt):
    """E H^(k), k = 0..4 (5 x n, numpy), H = y h1 + (m - y) h0, by the reference's rule."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    rho, s, y, mt = t(rho), t(s), t(y), t(mt)
    return np.stack([_EH.apply(rho, s, y, mt - y, link, k).numpy() for k in range(5)])


def response_mean(link, rho, s, mt, deg=GH_DEG):
    """m E p(t) on the nodes (numpy); the probit mean in closed form is `prob('probit', rho / sqrt(1 + s))`."""
    t, wts = _rule(torch.tensor(np.asarray(rho, dtype=np.float64)), torch.tensor(np.asarray(s, dtype=np.float64)), deg)
    p = torch.exp(torch.special.log_ndtr(t)) if link == 'probit' else -torch.expm1(-torch.exp(t))
    return np.asarray(mt, dtype=np.float64) * (p * wts[None, :]).sum(1).numpy()


def row_coefs(x, y, z, w, o, mt, gid, G, eta, link):
    """Per-row value and the five coefficients a1 = w E H', a2 = w E H'' / 2, c11 = w E H'', c12 = w E H''' / 2, c22 = w E H'''' / 4."""
    rho, s = bref._rho_s(np.asarray(eta, dtype=np.float64), x, z, o, gid, G)
    e = eh_coefs(link, rho, s, y, mt)
    return dict(value=w * e[0], a1=w * e[1], a2=w * 0.5 * e[2], c11=w * e[2], c12=w * 0.5 * e[3], c22=w * 0.25 * e[4])


def data_pieces(x, y, z, w, o, mt, gid, G, eta, link):
    """The data-dependent inputs of `glmm_slopes_closed_forms` in numpy, from `row_coefs` (as the binomial helper's)."""
    c = row_coefs(x, y, z, w, o, mt, gid, G, eta, link)
    x2, z2 = x * x, z * z

    def gsum(v):
        out = np.zeros((G,) + v.shape[1:])
        np.add.at(out, gid, v)
        return out
    outer = lambda cc, p, q: gsum(cc[:, None, None] * p[:, :, None] * q[:, None, :])
    K = z.shape[1]
    loc = np.zeros((G, 2 * K, 2 * K))
    loc[:, :K, :K] = outer(c['c11'], z, z)
    loc[:, :K, K:] = outer(c['c12'], z, z2)
    loc[:, K:, :K] = loc[:, :K, K:].transpose(0, 2, 1)
    loc[:, K:, K:] = outer(c['c22'], z2, z2)
    border = np.concatenate([outer(c['c11'], z, x), outer(c['c12'], z2, x), outer(c['c12'], z, x2), outer(c['c22'], z2, x2)], axis=1)
    return dict(value=float(np.sum(c['value'])), g_glob=np.concatenate([x.T @ c['a1'], x2.T @ c['a2']]),
                g_loc=np.hstack([gsum(c['a1'][:, None] * z), gsum(c['a2'][:, None] * z2)]),
                Hb=np.stack([x.T @ (c['c11'][:, None] * x), x.T @ (c['c12'][:, None] * x2), x2.T @ (c['c22'][:, None] * x2)]),
                border=border, loc=loc)

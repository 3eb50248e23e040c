"""Independent fp64 torch references of `BinomialGLMMObjective` and `NegBinomialGLMMObjective` (shared by the CPU and GPU tests).

Binomial: the KL of tests/glmm_slopes_reference.py with the data term replaced by

    sum_n w_n [ m_n psi(rho_n, s_n) - y_n rho_n ],   rho_n = o_n + x_n . m + z_n . e_g(n),
                                                     s_n = (x_n o x_n) . (1 / i_beta) + (z_n o z_n) . (1 / i_g(n))

psi = E softplus(t), t ~ N(rho, s), being `glmm_slopes_reference`'s (tests/lmvn_reference.py); the constant log C(m, y) is dropped.
The prior and entropy terms are literally those of `glmm_slopes_reference.kl_vec`: it is called with zero weights, which removes its
own data term and nothing else.

Negative binomial (`nb_kl_vec`), written separately -- it does NOT go through the binomial formula: the data term

    sum_n w_n [ (y_n + phi_n) E logaddexp(log phi_n, t) - y_n rho_n ],   t ~ N(rho_n, s_n),  rho_n = o_n + x_n . m + z_n . e_g(n)

by the 20-node Gauss-Hermite sum of logaddexp(log phi, .) itself, under the same rule as the model: its derivatives are defined by
Stein's identity on the same nodes, the derivatives of logaddexp in t being taken by nested autograd (`_ENB`).

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import math

import numpy as np
import torch

import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)
from lmvn_reference import psi

GH_DEG = 20


def _rho_s(eta, x, z, o, gid, G):
    P, K = x.shape[1], z.shape[1]
    ng = 2 * P + 4 * K
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    rho = o + x @ eta[:P] + (z * e[gid]).sum(1)
    s = (x * x) @ (1.0 / eta[P:2 * P]) + (z * z * (1.0 / ig)[gid]).sum(1)
    return rho, s


def _priors(eta, x, y, z, w, gid, G, hyp):
    return sref.kl_vec(eta, x, y, z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_vec(eta, x, y, z, w, o, mt, gid, G, hyp):
    """hyp = [tau_beta, mu0, kappa0, a0, b0] (a tensor, so that the priors can be differentiated); mt: the trials."""
    rho, s = _rho_s(eta, x, z, o, gid, G)
    data = (w * (mt * psi(rho, s, GH_DEG) - y * rho)).sum()
    return data + _priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, mt, gid, G, hyp):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, mt, gid, G, hyp)


def _dk_logaddexp(lphi, t, k):
    """k-th derivative in t of logaddexp(log phi, t), by k nested autograd passes (no closed sigmoid formulas)."""
    with torch.enable_grad():
        tt = t.detach().requires_grad_(True)
        h = torch.logaddexp(lphi.expand_as(tt), tt)
        for _ in range(k):
            h, = torch.autograd.grad(h.sum(), tt, create_graph=True)
    return h.detach()


class _ENB(torch.autograd.Function):
    """E d^k/dt^k logaddexp(log phi, t), t ~ N(mu, s), by Gauss-Hermite, differentiated by the rule the model uses (Stein's
    identity on the same nodes: d_mu E h^(k) = E h^(k+1), d_s E h^(k) = E h^(k+2) / 2), to any order."""
    @staticmethod
    def forward(ctx, mu, s, lphi, k):
        ctx.save_for_backward(mu, s, lphi)
        ctx.k = k
        gx, gw = np.polynomial.hermite.hermgauss(GH_DEG)
        nodes = torch.tensor(math.sqrt(2.0) * gx, dtype=torch.float64)
        wts = torch.tensor(gw / math.sqrt(math.pi), dtype=torch.float64)
        t = mu[:, None] + torch.sqrt(torch.clamp(s, min=0.0))[:, None] * nodes[None, :]
        return (_dk_logaddexp(lphi[:, None], t, k) * wts[None, :]).sum(1)

    @staticmethod
    def backward(ctx, go):
        mu, s, lphi = ctx.saved_tensors
        return go * _ENB.apply(mu, s, lphi, ctx.k + 1), go * 0.5 * _ENB.apply(mu, s, lphi, ctx.k + 2), None, None


def nb_data(eta, x, y, z, w, o, phi, gid, G):
    rho, s = _rho_s(eta, x, z, o, gid, G)
    return (w * ((y + phi) * _ENB.apply(rho, s, torch.log(phi), 0) - y * rho)).sum()


def nb_kl_vec(eta, x, y, z, w, o, phi, gid, G, hyp):
    return nb_data(eta, x, y, z, w, o, phi, gid, G) + _priors(eta, x, y, z, w, gid, G, hyp)


def nb_kl_free(free, x, y, z, w, o, phi, gid, G, hyp):
    return nb_kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, phi, gid, G, hyp)


def tensors(x, y, z, w, o, mt, gid, hyp=(1.0, 0.0, 1.0, 1.0, 1.0)):
    """The argument tuple of `kl_vec` / `kl_free` (or, with phi for mt, of `nb_kl_vec` / `nb_kl_free`) behind the point,
    without G: (x, y, z, w, o, mt, gid, hyp)."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return t(x), t(y), t(z), t(w), t(o), t(mt), torch.tensor(np.asarray(gid, dtype=np.int64)), t(hyp)


def targs(x, y, z, w, o, mt, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0)):
    t = tensors(x, y, z, w, o, mt, gid, hyp)
    return t[:7] + (G, t[7])


def problem(N, P, K, G, seed, **kw):
    """x, z, w, gid and the point (free coordinates) of `glmm_slopes_reference.problem`; then the non-intercept columns of z are
    halved, o ~ 0.3 N(0, 1), integer trials in 0..12 (m[0] = 0 and m[1] = 1 when N >= 4: a row without trials and a Bernoulli
    row) and y ~ Binomial(m, sigma(o + x beta + z . u)) with beta and u the means of the point.
    Returns (x, y, z, w, gid, o, m, free)."""
    x, _, z, w, gid, free = sref.problem(N, P, K, G, seed, **kw)
    z = z.copy()
    z[:, 1:] *= 0.5
    rng = np.random.default_rng([seed, 2])
    o = 0.3 * rng.normal(size=N)
    m = rng.integers(0, 13, size=N).astype(np.float64)
    if N >= 4:
        m[0], m[1] = 0.0, 1.0
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    pr = 1.0 / (1.0 + np.exp(-(o + x @ beta + (z * u[gid]).sum(1))))
    y = rng.binomial(m.astype(np.int64), pr).astype(np.float64)
    return x, y, z, w, gid, o, m, free


def nb_problem(N, P, K, G, seed, phi=1.7, **kw):
    """The x, z, w, gid, o and point of `problem`, y ~ Poisson(3) and the dispersion phi (scalar, or 'vector' for
    phi_n ~ U(0.5, 4)).  Returns (x, y, z, w, gid, o, phi (N), free)."""
    x, _, z, w, gid, o, _, free = problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 3])
    y = rng.poisson(3.0, size=N).astype(np.float64)
    ph = rng.uniform(0.5, 4.0, size=N) if isinstance(phi, str) else np.full(N, float(phi))
    return x, y, z, w, gid, o, ph, free


def psi_coefs(rho, s, mt):
    """m psi and its derivatives (value, d_rho, d_s, d_rhorho, d_rhos, d_ss) by autograd of the reference's psi."""
    tr = torch.tensor(np.asarray(rho, dtype=np.float64), requires_grad=True)
    ts = torch.tensor(np.asarray(s, dtype=np.float64), requires_grad=True)
    val = torch.tensor(np.asarray(mt, dtype=np.float64)) * psi(tr, ts, GH_DEG)
    p_r, p_s = torch.autograd.grad(val.sum(), (tr, ts), create_graph=True)
    p_rr, p_rs = torch.autograd.grad(p_r.sum(), (tr, ts), retain_graph=True)
    p_ss, = torch.autograd.grad(p_s.sum(), ts)
    return tuple(t.detach().numpy() for t in (val, p_r, p_s, p_rr, p_rs, p_ss))


def row_coefs(x, y, z, w, o, mt, gid, G, eta):
    """Per-row value and the five coefficients a1 = w (m psi_rho - y), a2 = w m psi_s, c11 = w m psi_rhorho, c12 = w m psi_rhos,
    c22 = w m psi_ss by autograd of psi."""
    rho, s = _rho_s(np.asarray(eta, dtype=np.float64), x, z, o, gid, G)
    val, p_r, p_s, p_rr, p_rs, p_ss = psi_coefs(rho, s, mt)
    return dict(value=w * (val - y * rho), a1=w * (p_r - y), a2=w * p_s, c11=w * p_rr, c12=w * p_rs, c22=w * p_ss)


def data_pieces(x, y, z, w, o, mt, gid, G, eta):
    """The data-dependent inputs of `glmm_slopes_closed_forms` in numpy, from `row_coefs`."""
    c = row_coefs(x, y, z, w, o, mt, gid, G, eta)
    K = z.shape[1]
    x2, z2 = x * x, z * z

    def gsum(v):
        out = np.zeros((G,) + v.shape[1:])
        np.add.at(out, gid, v)
        return out
    outer = lambda cc, p, q: gsum(cc[:, None, None] * p[:, :, None] * q[:, None, :])
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

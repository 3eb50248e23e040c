"""Independent fp64 torch reference of the Poisson mixed model `PoissonGLMMObjective` (shared by the CPU and GPU tests): the KL of
tests/glmm_slopes_reference.py with the data term replaced by

    sum_n w_n [ exp(rho_n + s_n / 2) - y_n rho_n ],   rho_n = o_n + x_n . m + z_n . e_g(n),
                                                      s_n = (x_n o x_n) . (1 / i_beta) + (z_n o z_n) . (1 / i_g(n))

(E exp(t) for t ~ N(rho, s) is exact; the constant log y! is dropped).  The prior and entropy terms are literally those of
`glmm_slopes_reference.kl_vec`: it is called with zero weights, which removes its own data term and nothing else.  Coordinates,
`positive_mask`, `free_to_vec` and `value_grad_hess` are that module's."""
import numpy as np
import torch

import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)


def _rho_s(eta, x, z, o, gid, G):
    P, K = x.shape[1], z.shape[1]
    ng = 2 * P + 4 * K
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    rho = o + x @ eta[:P] + (z * e[gid]).sum(1)
    s = (x * x) @ (1.0 / eta[P:2 * P]) + (z * z * (1.0 / ig)[gid]).sum(1)
    return rho, s


def kl_vec(eta, x, y, z, w, o, gid, G, hyp):
    """hyp = [tau_beta, mu0, kappa0, a0, b0] (a tensor, so that the priors can be differentiated)."""
    rho, s = _rho_s(eta, x, z, o, gid, G)
    data = (w * (torch.exp(rho + 0.5 * s) - y * rho)).sum()
    return data + sref.kl_vec(eta, x, y, z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_free(free, x, y, z, w, o, gid, G, hyp):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, gid, G, hyp)


def tensors(x, y, z, w, o, gid, hyp=(1.0, 0.0, 1.0, 1.0, 1.0)):
    """The argument tuple of `kl_vec` / `kl_free` behind the point, without G: (x, y, z, w, o, gid, hyp)."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return t(x), t(y), t(z), t(w), t(o), torch.tensor(np.asarray(gid, dtype=np.int64)), t(hyp)


def targs(x, y, z, w, o, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0)):
    t = tensors(x, y, z, w, o, gid, hyp)
    return t[:6] + (G, t[6])


def problem(N, P, K, G, seed, **kw):
    """x, z, w, gid and the point (free coordinates) of `glmm_slopes_reference.problem`; then the non-intercept columns of z
    are halved, o = log U(0.5, 2) and y ~ Poisson(exp(o + x beta + z . u)) with beta and u the means of the point.
    Returns (x, y, z, w, gid, o, free)."""
    x, _, z, w, gid, free = sref.problem(N, P, K, G, seed, **kw)
    z = z.copy()
    z[:, 1:] *= 0.5
    rng = np.random.default_rng([seed, 1])
    o = np.log(rng.uniform(0.5, 2.0, size=N))
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    y = rng.poisson(np.exp(o + x @ beta + (z * u[gid]).sum(1))).astype(np.float64)
    return x, y, z, w, gid, o, free


def psi_coefs(rho, s):
    """psi and its derivatives (psi, psi_rho, psi_s, psi_rhorho, psi_rhos, psi_ss) by autograd of psi = exp(rho + s / 2)."""
    tr = torch.tensor(np.asarray(rho, dtype=np.float64), requires_grad=True)
    ts = torch.tensor(np.asarray(s, dtype=np.float64), requires_grad=True)
    val = torch.exp(tr + 0.5 * ts)
    p_r, p_s = torch.autograd.grad(val.sum(), (tr, ts), create_graph=True)
    p_rr, p_rs = torch.autograd.grad(p_r.sum(), (tr, ts), retain_graph=True)
    p_ss, = torch.autograd.grad(p_s.sum(), ts)
    return tuple(t.detach().numpy() for t in (val, p_r, p_s, p_rr, p_rs, p_ss))


def row_coefs(x, y, z, w, o, gid, G, eta):
    """Per-row value and the five coefficients a1 = w (psi_rho - y), a2 = w psi_s, c11 = w psi_rhorho, c12 = w psi_rhos,
    c22 = w psi_ss by autograd of psi."""
    rho, s = _rho_s(np.asarray(eta, dtype=np.float64), x, z, o, gid, G)
    val, p_r, p_s, p_rr, p_rs, p_ss = psi_coefs(rho, s)
    return dict(value=w * (val - y * rho), a1=w * (p_r - y), a2=w * p_s, c11=w * p_rr, c12=w * p_rs, c22=w * p_ss)


def data_pieces(x, y, z, w, o, gid, G, eta):
    """The data-dependent inputs of `glmm_slopes_closed_forms` in numpy, from `row_coefs`."""
    c = row_coefs(x, y, z, w, o, gid, G, eta)
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

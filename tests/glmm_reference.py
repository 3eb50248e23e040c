"""Independent fp64 torch reference of the logistic mixed model `LogisticGLMMObjective` (shared by the CPU and GPU tests).

    KL =  sum_n w_n [ psi(rho_n, s_n) - y_n rho_n ]     rho_n = x_n . m + e_g(n),  s_n = (x_n o x_n) . (1 / i_beta) + 1 / i_g(n)
        + 1/2 E tau ( sum_g [(e_g - e_mu)^2 + 1 / i_g] + G / i_mu ) - 1/2 G E log tau
        + 1/2 tau_beta sum_j (m_j^2 + 1 / i_beta_j) + 1/2 kappa0 ((e_mu - mu0)^2 + 1 / i_mu)
        - (a0 - 1) E log tau + b0 E tau
        + 1/2 sum_j log i_beta_j + 1/2 log i_mu + 1/2 sum_g log i_g - gamma_entropy(a, b)

psi and its Stein-rule derivatives come from tests/lmvn_reference.py.  Vector coordinates
eta = [m | i_beta | e_mu, i_mu | a, b | e | i]; free coordinates take the logarithm of every positive entry (lower bound 0).
`_EG` does not go through torch.func: differentiate with torch.autograd.grad / torch.autograd.functional.hessian."""
import numpy as np
import torch

from lmvn_reference import psi


class _PolyGamma(torch.autograd.Function):
    """polygamma(k, a) through scipy, differentiable to any order (d/da polygamma(k) = polygamma(k + 1)).  torch's own fp64
    trigamma is accurate to about 1e-9 only (0.7: 1.2e-9, 2.0: 2.4e-10 against scipy), which is above the gradient tolerance."""
    @staticmethod
    def forward(ctx, a, k):
        from scipy import special
        ctx.save_for_backward(a)
        ctx.k = k
        return torch.tensor(special.polygamma(k, a.detach().numpy()), dtype=torch.float64)

    @staticmethod
    def backward(ctx, go):
        a, = ctx.saved_tensors
        return go * _PolyGamma.apply(a, ctx.k + 1), None


def digamma(a):
    return _PolyGamma.apply(a, 0)


def positive_mask(P, G):
    mask = np.zeros(2 * P + 4 + 2 * G, dtype=bool)
    mask[P:2 * P] = True
    mask[2 * P + 1:2 * P + 4] = True
    mask[2 * P + 4 + G:] = True
    return mask


def free_to_vec(free, P, G):
    mask = torch.tensor(positive_mask(P, G))
    return torch.where(mask, torch.exp(free), free)


def kl_vec(eta, x, y, w, gid, G, hyp, gh_deg=20):
    """hyp = [tau_beta, mu0, kappa0, a0, b0] (a tensor, so that the priors can be differentiated)."""
    P = x.shape[1]
    ng = 2 * P + 4
    m, ib = eta[:P], eta[P:2 * P]
    e_mu, i_mu, a, b = eta[2 * P], eta[2 * P + 1], eta[2 * P + 2], eta[2 * P + 3]
    e, ig = eta[ng:ng + G], eta[ng + G:]
    tau_beta, mu0, kappa0, a0, b0 = hyp[0], hyp[1], hyp[2], hyp[3], hyp[4]
    rho = x @ m + e[gid]
    s = (x * x) @ (1.0 / ib) + (1.0 / ig)[gid]
    data = (w * (psi(rho, s, gh_deg) - y * rho)).sum()
    Et, EL = a / b, digamma(a) - torch.log(b)
    ent = a - torch.log(b) + torch.lgamma(a) + (1.0 - a) * digamma(a)
    return (data + 0.5 * Et * (((e - e_mu) ** 2 + 1.0 / ig).sum() + G / i_mu) - 0.5 * G * EL
            + 0.5 * tau_beta * ((m ** 2).sum() + (1.0 / ib).sum()) + 0.5 * kappa0 * ((e_mu - mu0) ** 2 + 1.0 / i_mu)
            - (a0 - 1.0) * EL + b0 * Et
            + 0.5 * torch.log(ib).sum() + 0.5 * torch.log(i_mu) + 0.5 * torch.log(ig).sum() - ent)


def kl_free(free, x, y, w, gid, G, hyp, gh_deg=20):
    return kl_vec(free_to_vec(free, x.shape[1], G), x, y, w, gid, G, hyp, gh_deg)


def tensors(x, y, w, gid, hyp=(1.0, 0.0, 1.0, 1.0, 1.0)):
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return t(x), t(y), t(w), torch.tensor(np.asarray(gid, dtype=np.int64)), t(hyp)


def value_grad_hess(fun, point, args, want_hess=True):
    """fun(point, *args) -> value, gradient and dense Hessian (numpy)."""
    p = torch.tensor(np.asarray(point, dtype=np.float64), requires_grad=True)
    val = fun(p, *args)
    g, = torch.autograd.grad(val, p)
    H = None
    if want_hess:
        H = torch.autograd.functional.hessian(lambda q: fun(q, *args), p.detach()).numpy()
        H = 0.5 * (H + H.T)
    return float(val.detach()), g.numpy(), H


def problem(N, P, G, seed, big_group=True, empty_group=True):
    """Data, group ids and a point (free coordinates) with logits of order one.  With G >= 3: the last group is empty and group 0
    holds more than half of the rows; the other rows fall on the remaining groups at random."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    w = rng.uniform(0.5, 1.5, size=N)
    n_used = G - 1 if (empty_group and G >= 3) else G
    gid = rng.integers(0, n_used, size=N)
    if big_group and G >= 3:
        gid[rng.uniform(size=N) < 0.55] = 0
    u = rng.normal(size=G) * 0.7
    beta = rng.normal(size=P) * 0.8
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + u[gid] + 0.3)))).astype(np.float64)
    free = np.concatenate([beta + 0.1 * rng.normal(size=P), rng.normal(size=P) * 0.3 + 2.0,     # m, log i_beta
                           [0.2, 1.0], [0.7, 0.4],                                              # e_mu, log i_mu, log a, log b
                           u + 0.1 * rng.normal(size=G), rng.normal(size=G) * 0.3 + 1.0])       # e, log i
    return x, y, w, gid.astype(np.int32), free


def row_coefs(x, y, w, gid, G, eta, gh_deg=20):
    """Per-row value and the five coefficients a1 = w (psi_rho - y), a2 = w psi_s, c11 = w psi_rhorho, c12 = w psi_rhos,
    c22 = w psi_ss by autograd of the reference's psi (rows are independent: derivatives of the sum over rows)."""
    P = x.shape[1]
    ng = 2 * P + 4
    rho = x @ eta[:P] + eta[ng:ng + G][gid]
    s = (x * x) @ (1.0 / eta[P:2 * P]) + (1.0 / eta[ng + G:])[gid]
    tr = torch.tensor(rho, requires_grad=True)
    ts = torch.tensor(s, requires_grad=True)
    val = psi(tr, ts, gh_deg)
    p_r, p_s = torch.autograd.grad(val.sum(), (tr, ts), create_graph=True)
    p_rr, p_rs = torch.autograd.grad(p_r.sum(), (tr, ts), retain_graph=True)
    p_ss, = torch.autograd.grad(p_s.sum(), ts)
    n = lambda t: t.detach().numpy()
    return dict(value=w * (n(val) - y * rho), a1=w * (n(p_r) - y), a2=w * n(p_s), c11=w * n(p_rr), c12=w * n(p_rs), c22=w * n(p_ss))


def data_pieces(x, y, w, gid, G, eta, gh_deg=20):
    """The data-dependent inputs of `glmm_closed_forms` in numpy, from `row_coefs`."""
    c = row_coefs(x, y, w, gid, G, eta, gh_deg)
    P = x.shape[1]
    x2 = x * x

    def gsum(v):
        out = np.zeros((G,) + v.shape[1:])
        np.add.at(out, gid, v)
        return out
    border = np.hstack([gsum(c['c11'][:, None] * x), gsum(c['c12'][:, None] * x), gsum(c['c12'][:, None] * x2), gsum(c['c22'][:, None] * x2)])
    return dict(value=float(np.sum(c['value'])), g_glob=np.concatenate([x.T @ c['a1'], x2.T @ c['a2']]),
                g_loc=np.stack([gsum(c['a1']), gsum(c['a2'])], axis=1),
                Hb=np.stack([x.T @ (c['c11'][:, None] * x), x.T @ (c['c12'][:, None] * x2), x2.T @ (c['c22'][:, None] * x2)]),
                border=border, loc=np.stack([gsum(c['c11']), gsum(c['c12']), gsum(c['c22'])], axis=1))

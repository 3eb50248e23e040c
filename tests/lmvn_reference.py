"""Independent fp64 torch reference of the full-covariance logistic regression objective (free coordinates, log-Cholesky
map written here), shared by the CPU and GPU tests of `LogitNormalMVNRegressionObjective`.

psi(mu, s) = E g(z), z ~ N(mu, s), g = log(1 + e^t), by Gauss-Hermite; its derivatives are defined by Stein's identity on the
same nodes, d_mu E g^(k) = E g^(k+1) and d_s E g^(k) = E g^(k+2) / 2, which is what the model differentiates (a zero design
row, s = 0, stays regular).  `_EG` carries that rule through autograd to any order."""
import math

import numpy as np
import torch


def _gk(t, k):
    """k-th derivative of log(1 + e^t), overflow-free."""
    if k == 0:
        return torch.logaddexp(torch.zeros_like(t), t)
    s = torch.sigmoid(t)
    g2 = s * (1 - s)
    if k == 1:
        return s
    if k == 2:
        return g2
    g3 = g2 * (1 - 2 * s)
    if k == 3:
        return g3
    g4 = g2 * (1 - 6 * g2)
    if k == 4:
        return g4
    if k == 5:
        return g3 * (1 - 12 * g2)
    if k == 6:
        return g4 * (1 - 12 * g2) - 12 * g3 * g3
    raise ValueError(k)


class _EG(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, s, k, nodes, weights):
        ctx.save_for_backward(mu, s)
        ctx.k, ctx.nodes, ctx.weights = k, nodes, weights
        t = mu[:, None] + torch.sqrt(torch.clamp(s, min=0.0))[:, None] * nodes[None, :]
        return (_gk(t, k) * weights[None, :]).sum(1)

    @staticmethod
    def backward(ctx, go):
        mu, s = ctx.saved_tensors
        k, n, w = ctx.k, ctx.nodes, ctx.weights
        return go * _EG.apply(mu, s, k + 1, n, w), go * 0.5 * _EG.apply(mu, s, k + 2, n, w), None, None, None


def psi(mu, s, gh_deg):
    gx, gw = np.polynomial.hermite.hermgauss(gh_deg)
    nodes = torch.tensor(math.sqrt(2.0) * gx, dtype=torch.float64)
    weights = torch.tensor(gw / math.sqrt(math.pi), dtype=torch.float64)
    return _EG.apply(mu, s, 0, nodes, weights)


def chol_from_free(fl, P):
    r, c = np.tril_indices(P)
    L = torch.zeros((P, P), dtype=torch.float64)
    L = L.index_put((torch.tensor(r), torch.tensor(c)), fl)
    return torch.tril(L, -1) + torch.diag(torch.exp(torch.diagonal(L)))


def kl_free(free, x, y, w, tau, gh_deg):
    """KL in free coordinates [m | log-Cholesky of Lambda] (torch tensors in, scalar out)."""
    P = x.shape[1]
    m = free[:P]
    L = chol_from_free(free[P:], P)
    Lam = L @ L.T
    Sigma = torch.cholesky_inverse(L)
    mu = x @ m
    s = torch.einsum('ni,ij,nj->n', x, Sigma, x)
    data = (w * (psi(mu, s, gh_deg) - y * mu)).sum()
    return data + 0.5 * tau * (m @ m + torch.trace(Sigma)) + torch.log(torch.diagonal(L)).sum()


def kl_vec(eta, x, y, w, tau, gh_deg):
    """KL in vector coordinates [m | vech Lambda]."""
    P = x.shape[1]
    r, c = np.tril_indices(P)
    A = torch.zeros((P, P), dtype=torch.float64).index_put((torch.tensor(r), torch.tensor(c)), eta[P:])
    Lam = A + torch.tril(A, -1).T
    Sigma = torch.linalg.inv(Lam)
    m = eta[:P]
    mu = x @ m
    s = torch.einsum('ni,ij,nj->n', x, Sigma, x)
    data = (w * (psi(mu, s, gh_deg) - y * mu)).sum()
    return data + 0.5 * tau * (m @ m + torch.trace(Sigma)) + 0.5 * torch.logdet(Lam)


def problem(N, P, seed, with_extremes=True):
    """Data and a point (free coordinates) with s_n of order 0.1: one all-zero row, one row with |mu| ~ 300."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    y = (rng.uniform(size=N) < 0.5).astype(np.float64)
    w = rng.uniform(0.5, 1.5, size=N)
    m = rng.normal(size=P) * 0.5
    A = rng.normal(size=(P, P)) / np.sqrt(P)
    Lam = 4.0 * np.eye(P) + A @ A.T
    if with_extremes:
        x[0] = 0.0                       # s = 0 and mu = 0
        if P >= 2:                       # column 0 is zero except in row 1: mu_1 = 300 at a small s_1
            x[:, 0] = 0.0
            x[1, 0] = 3.0
            m[0] = 100.0
            Lam[0, 0] += 100.0
    L = np.linalg.cholesky(Lam)
    fl = L[np.tril_indices(P)].copy()
    r, c = np.tril_indices(P)
    fl[r == c] = np.log(np.diag(L))
    return x, y, w, np.concatenate([m, fl]), Lam

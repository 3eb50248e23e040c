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


# ---- per-observation coefficients, independent of the kernels' formulas -------------------------------------------------
# For row n with mu_n = x_n . m, s_n = x_n^T Sigma x_n and the nodes t_k = mu_n + sqrt(s_n) z_k (z_k, p_k: the Gauss-Hermite
# rule for N(0, 1)):  value_n = w_n (E g - y_n mu_n), a1 = w (E g' - y), a2 = w E g'' / 2, c11 = w E g'', c12 = w E g''' / 2,
# c22 = w E g'''' / 4, the derivatives in (mu, s) by Stein's identity (the lmvn_coef_kernel header).

def std_nodes(deg):
    """Gauss-Hermite nodes and weights for E f(z), z ~ N(0, 1)."""
    gx, gw = np.polynomial.hermite.hermgauss(deg)
    return math.sqrt(2.0) * gx, gw / math.sqrt(math.pi)


def coefs_f64(x, y, w, m, S, nodes, weights):
    """fp64 coefficients by scipy.special.expit and np.logaddexp: dict of value, a1, a2, c11, c12, c22 (one entry per row)."""
    from scipy.special import expit
    mu = x @ m
    s = np.maximum(np.einsum('ni,ij,nj->n', x, S, x), 0.0)
    t = mu[:, None] + np.sqrt(s)[:, None] * nodes[None, :]
    p, q = expit(t), expit(-t)                     # sigma(t), 1 - sigma(t), each without cancellation
    g2 = p * q
    g3 = g2 * (q - p)
    g4 = g2 * (1.0 - 6.0 * g2)
    E = lambda a: a @ weights
    return dict(value=w * (E(np.logaddexp(0.0, t)) - y * mu), a1=w * (E(p) - y), a2=w * 0.5 * E(g2), c11=w * E(g2),
                c12=w * 0.5 * E(g3), c22=w * 0.25 * E(g4))


def coefs_mp(mu, s, y, w, nodes, weights, dps=40):
    """The same six numbers for one observation given (mu, s) directly, in mpmath at `dps` digits (inputs taken exactly)."""
    import mpmath as mp
    with mp.workdps(dps):
        mu, s, y, w = mp.mpf(mu), mp.mpf(s), mp.mpf(y), mp.mpf(w)
        sd = mp.sqrt(s)
        v = e1 = e2 = e3 = e4 = mp.mpf(0)
        for zk, pk in zip(nodes, weights):
            t = mu + sd * mp.mpf(zk)
            pk = mp.mpf(pk)
            sg = 1 / (1 + mp.exp(-t))
            g2 = sg * (1 - sg)
            v += pk * mp.log1p(mp.exp(t))
            e1 += pk * sg
            e2 += pk * g2
            e3 += pk * g2 * (1 - 2 * sg)
            e4 += pk * g2 * (1 - 6 * g2)
        out = dict(value=w * (v - y * mu), a1=w * (e1 - y), a2=w * e2 / 2, c11=w * e2, c12=w * e3 / 2, c22=w * e4 / 4)
        return {k: float(val) for k, val in out.items()}


def terms_from_coefs(x, c):
    """Value, gradient and Hessian of the data term in (m, vech Sigma) from per-row coefficients, with the explicit
    U (N x Pv, row n = packed lower triangle of x_n x_n^T) and the duplication weights delta of vech coordinates."""
    P = x.shape[1]
    r, cc = np.tril_indices(P)
    d = np.where(r == cc, 1.0, 2.0)
    U = x[:, r] * x[:, cc]
    g = np.concatenate([x.T @ c['a1'], d * (U.T @ c['a2'])])
    Hms = (x.T @ (c['c12'][:, None] * U)) * d[None, :]
    H = np.block([[x.T @ (c['c11'][:, None] * x), Hms], [Hms.T, d[:, None] * (U.T @ (c['c22'][:, None] * U)) * d[None, :]]])
    return float(np.sum(c['value'])), g, H


# ---- the mean-field model (q(beta_j) = N(mean_j, 1 / info_j)) as the model defines it -----------------------------------

def kl_mean_field(eta, x, y, w, tau, gh_deg):
    """KL of `LogitNormalRegressionObjective` in vector coordinates [mean | info] (torch in, scalar out): the quadrature
    sum phi(mu, sd) = sum_k p_k log(1 + exp(mu + sd z_k)) differentiated as it stands, sd = sqrt(v).  Where v = 0 (an
    all-zero design row) sd is held at 0 with a finite derivative: v does not move there, so the row adds exactly zero
    to every derivative in (mean, info)."""
    nodes, weights = (torch.tensor(a, dtype=torch.float64) for a in std_nodes(gh_deg))
    P = x.shape[1]
    mean, info = eta[:P], eta[P:]
    var = 1.0 / info
    mu, v = x @ mean, (x * x) @ var
    pos = v > 0
    sd = torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))
    t = mu[:, None] + sd[:, None] * nodes[None, :]
    phi = (torch.logaddexp(torch.zeros_like(t), t) * weights[None, :]).sum(1)
    return (w * (phi - y * mu)).sum() + 0.5 * tau * ((mean ** 2).sum() + var.sum()) + 0.5 * torch.log(info).sum()

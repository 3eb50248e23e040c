"""Independent fp64 torch reference of the logistic mixed model with random slopes `LogisticGLMMSlopesObjective` (shared by the
CPU and GPU tests).  K independent effects per group, design z (N x K):

    KL =  sum_n w_n [ psi(rho_n, s_n) - y_n rho_n ]     rho_n = x_n . m + z_n . e_g(n),  s_n = (x_n o x_n) . (1 / i_beta) + (z_n o z_n) . (1 / i_g(n))
        + sum_k { 1/2 E tau_k ( sum_g [(e_gk - e_mu_k)^2 + 1 / i_gk] + G / i_mu_k ) - 1/2 G E log tau_k
                  + 1/2 kappa0 ((e_mu_k - mu0)^2 + 1 / i_mu_k) - (a0 - 1) E log tau_k + b0 E tau_k
                  + 1/2 log i_mu_k + 1/2 sum_g log i_gk - gamma_entropy(a_k, b_k) }
        + 1/2 tau_beta sum_j (m_j^2 + 1 / i_beta_j) + 1/2 sum_j log i_beta_j

psi and its Stein-rule derivatives come from tests/lmvn_reference.py, digamma through scipy (tests/glmm_reference.py).  Vector
coordinates eta = [m | i_beta | e_mu (K) | i_mu (K) | a_0, b_0, .. | e (G K, group-major) | i (G K)]; free coordinates take the
logarithm of every positive entry (lower bound 0)."""
import numpy as np
import torch

from lmvn_reference import psi
from glmm_reference import digamma, value_grad_hess          # noqa: F401  (value_grad_hess is re-exported for the tests)


def positive_mask(P, K, G):
    ng = 2 * P + 4 * K
    mask = np.zeros(ng + 2 * G * K, dtype=bool)
    mask[P:2 * P] = True
    mask[2 * P + K:ng] = True
    mask[ng + G * K:] = True
    return mask


def free_to_vec(free, P, K, G):
    mask = torch.tensor(positive_mask(P, K, G))
    return torch.where(mask, torch.exp(free), free)


def kl_vec(eta, x, y, z, w, gid, G, hyp, gh_deg=20):
    """hyp = [tau_beta, mu0, kappa0, a0, b0] (a tensor, so that the priors can be differentiated)."""
    P, K = x.shape[1], z.shape[1]
    ng = 2 * P + 4 * K
    m, ib = eta[:P], eta[P:2 * P]
    e_mu, i_mu = eta[2 * P:2 * P + K], eta[2 * P + K:2 * P + 2 * K]
    ab = eta[2 * P + 2 * K:ng].reshape(K, 2)
    a, b = ab[:, 0], ab[:, 1]
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    tau_beta, mu0, kappa0, a0, b0 = hyp[0], hyp[1], hyp[2], hyp[3], hyp[4]
    rho = x @ m + (z * e[gid]).sum(1)
    s = (x * x) @ (1.0 / ib) + (z * z * (1.0 / ig)[gid]).sum(1)
    data = (w * (psi(rho, s, gh_deg) - y * rho)).sum()
    Et, EL = a / b, digamma(a) - torch.log(b)
    ent = a - torch.log(b) + torch.lgamma(a) + (1.0 - a) * digamma(a)
    per_k = (0.5 * Et * (((e - e_mu[None, :]) ** 2 + 1.0 / ig).sum(0) + G / i_mu) - 0.5 * G * EL
             + 0.5 * kappa0 * ((e_mu - mu0) ** 2 + 1.0 / i_mu) - (a0 - 1.0) * EL + b0 * Et
             + 0.5 * torch.log(i_mu) + 0.5 * torch.log(ig).sum(0) - ent)
    return data + per_k.sum() + 0.5 * tau_beta * ((m ** 2).sum() + (1.0 / ib).sum()) + 0.5 * torch.log(ib).sum()


def kl_free(free, x, y, z, w, gid, G, hyp, gh_deg=20):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, gid, G, hyp, gh_deg)


def tensors(x, y, z, w, gid, hyp=(1.0, 0.0, 1.0, 1.0, 1.0)):
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return t(x), t(y), t(z), t(w), torch.tensor(np.asarray(gid, dtype=np.int64)), t(hyp)


def problem(N, P, K, G, seed, big_group=True, empty_group=True):
    """Data, design z (first column ones, the others N(0, 1)), group ids and a point (free coordinates) with the scales of
    glmm_reference.problem.  With G >= 3: the last group is empty and group 0 holds more than half of the rows."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), rng.normal(size=(N, K - 1))], axis=1)
    w = rng.uniform(0.5, 1.5, size=N)
    n_used = G - 1 if (empty_group and G >= 3) else G
    gid = rng.integers(0, n_used, size=N)
    if big_group and G >= 3:
        gid[rng.uniform(size=N) < 0.55] = 0
    u = rng.normal(size=(G, K)) * 0.7
    beta = rng.normal(size=P) * 0.8
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid]).sum(1) + 0.3)))).astype(np.float64)
    free = np.concatenate([beta + 0.1 * rng.normal(size=P), rng.normal(size=P) * 0.3 + 2.0,                 # m, log i_beta
                           0.2 + 0.1 * rng.normal(size=K), 1.0 + 0.1 * rng.normal(size=K),                  # e_mu, log i_mu
                           (np.array([0.7, 0.4])[None, :] + 0.1 * rng.normal(size=(K, 2))).ravel(),         # log a_k, log b_k
                           (u + 0.1 * rng.normal(size=(G, K))).ravel(), rng.normal(size=G * K) * 0.3 + 1.0])   # e, log i
    return x, y, z, w, gid.astype(np.int32), free


def row_coefs(x, y, z, w, gid, G, eta, gh_deg=20):
    """Per-row value and the five coefficients a1 = w (psi_rho - y), a2 = w psi_s, c11 = w psi_rhorho, c12 = w psi_rhos,
    c22 = w psi_ss by autograd of the reference's psi."""
    P, K = x.shape[1], z.shape[1]
    ng = 2 * P + 4 * K
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    rho = x @ eta[:P] + (z * e[gid]).sum(1)
    s = (x * x) @ (1.0 / eta[P:2 * P]) + (z * z * (1.0 / ig)[gid]).sum(1)
    tr = torch.tensor(rho, requires_grad=True)
    ts = torch.tensor(s, requires_grad=True)
    val = psi(tr, ts, gh_deg)
    p_r, p_s = torch.autograd.grad(val.sum(), (tr, ts), create_graph=True)
    p_rr, p_rs = torch.autograd.grad(p_r.sum(), (tr, ts), retain_graph=True)
    p_ss, = torch.autograd.grad(p_s.sum(), ts)
    n = lambda t: t.detach().numpy()
    return dict(value=w * (n(val) - y * rho), a1=w * (n(p_r) - y), a2=w * n(p_s), c11=w * n(p_rr), c12=w * n(p_rs), c22=w * n(p_ss))


def data_pieces(x, y, z, w, gid, G, eta, gh_deg=20):
    """The data-dependent inputs of `glmm_slopes_closed_forms` in numpy, from `row_coefs`."""
    c = row_coefs(x, y, z, w, gid, G, eta, gh_deg)
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

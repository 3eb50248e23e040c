"""Independent fp64 torch reference of the mixed models with CORRELATED random effects, `LogisticGLMMCorrObjective` and
`PoissonGLMMCorrObjective` (shared by the CPU and GPU tests).  u_g ~ N(mu, Lambda^-1), Lambda ~ Wishart(nu0, W0^-1), q(Lambda) =
Wishart(n, V), q(u_g) mean-field:

    KL =  sum_n w_n [ psi_n - y_n rho_n ]     rho_n = o_n + x_n . m + z_n . e_g(n),  s_n = (x_n o x_n) . (1 / i_beta) + (z_n o z_n) . (1 / i_g(n))
        + 1/2 sum_g [ d_g^T (n V) d_g + sum_k n V_kk (1 / i_gk + 1 / i_mu_k) ] - 1/2 (G + nu0 - K - 1) E log|Lambda| + 1/2 n tr(W0 V)
        - wishart_entropy(n, V) + sum_k [ 1/2 kappa0 ((e_mu_k - mu0)^2 + 1 / i_mu_k) + 1/2 log i_mu_k ] + 1/2 sum_gk log i_gk
        + 1/2 tau_beta sum_j (m_j^2 + 1 / i_beta_j) + 1/2 sum_j log i_beta_j

d_g = e_g - e_mu, E log|Lambda| = psi_K(n / 2) + K log 2 + log|V|, psi_n the Gauss-Hermite E log(1 + exp t) of tests/lmvn_reference.py
(logistic) or exp(rho_n + s_n / 2) (Poisson).  Written with torch.mvlgamma, a digamma and its own log-Cholesky map; every
derivative is autograd's.  The digamma is `glmm_reference.digamma` (scipy's polygamma behind an autograd Function) and not
torch.digamma: the derivative of the latter is torch's fp64 trigamma, which is accurate to 1e-10 .. 5e-10 only (measured
against scipy at 1.3 .. 4.4), above the 1e-10 asked of the gradient -- the other mixed-model references made the same choice.
torch.mvlgamma stays: its first derivative is torch's digamma (accurate to rounding), its second enters one Hessian entry only.  Vector coordinates eta = [m | i_beta | e_mu (K) | i_mu (K) | n | vech V (row-major lower triangle) |
e (G K, group-major) | i (G K)]; free coordinates: log of the positive entries, n = K - 1 + exp(.), V = L L^T with L the lower
triangle of the free entries, its diagonal exponentiated."""
import numpy as np
import torch

from lmvn_reference import psi
from glmm_reference import digamma, value_grad_hess          # noqa: F401  (value_grad_hess is re-exported for the tests)
import glmm_slopes_reference as sref
import glmm_poisson_reference as pref


def sizes(P, K, G):
    Kv = K * (K + 1) // 2
    ng = 2 * P + 2 * K + 1 + Kv
    return Kv, ng, ng + 2 * G * K


def coupled_rows(P, K):
    Kv, ng, _ = sizes(P, K, 0)
    return np.concatenate([np.arange(2 * P + K), np.arange(2 * P + 2 * K, ng)])


def _tril(K):
    r, c = np.tril_indices(K)
    return torch.tensor(r), torch.tensor(c)


def vech_to_mat(vech, K):
    r, c = _tril(K)
    L = torch.zeros((K, K), dtype=vech.dtype)
    L = L.index_put((r, c), vech)
    return L + L.T - torch.diag(torch.diagonal(L))


def free_to_vec(free, P, K, G):
    Kv, ng, D = sizes(P, K, G)
    o = 2 * P + 2 * K
    r, c = _tril(K)
    L = torch.zeros((K, K), dtype=free.dtype).index_put((r, c), free[o + 1:ng])
    L = torch.tril(L, -1) + torch.diag(torch.exp(torch.diagonal(L)))
    V = L @ L.T
    return torch.cat([free[:P], torch.exp(free[P:2 * P]), free[2 * P:2 * P + K], torch.exp(free[2 * P + K:o]),
                      (K - 1.0 + torch.exp(free[o])).reshape(1), V[r, c], free[ng:ng + G * K], torch.exp(free[ng + G * K:])])


def kl_vec(eta, x, y, z, w, o, gid, G, hyp, lik='logistic', gh_deg=20):
    """hyp = [tau_beta, mu0, kappa0, nu0 | vech W0] (a tensor, so that the priors can be differentiated); o: the offsets (N)."""
    P, K = x.shape[1], z.shape[1]
    Kv, ng, D = sizes(P, K, G)
    m, ib = eta[:P], eta[P:2 * P]
    e_mu, i_mu = eta[2 * P:2 * P + K], eta[2 * P + K:2 * P + 2 * K]
    n, V = eta[2 * P + 2 * K], vech_to_mat(eta[2 * P + 2 * K + 1:ng], K)
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    tau_beta, mu0, kappa0, nu0, W0 = hyp[0], hyp[1], hyp[2], hyp[3], vech_to_mat(hyp[4:], K)
    rho = o + x @ m + (z * e[gid]).sum(1)
    s = (x * x) @ (1.0 / ib) + (z * z * (1.0 / ig)[gid]).sum(1)
    psi_n = psi(rho, s, gh_deg) if lik == 'logistic' else torch.exp(rho + 0.5 * s)
    data = (w * (psi_n - y * rho)).sum()
    EL = n * V
    half = 0.5 * n - 0.5 * torch.arange(K, dtype=eta.dtype)
    mvdg = digamma(half).sum()
    logdet = torch.logdet(V)
    e_logdet = mvdg + K * np.log(2.0) + logdet
    entropy = 0.5 * (K + 1) * logdet + 0.5 * K * (K + 1) * np.log(2.0) + torch.mvlgamma(0.5 * n, K) - 0.5 * (n - K - 1.0) * mvdg + 0.5 * n * K
    d = e - e_mu[None, :]
    quad = 0.5 * ((d @ EL) * d).sum() + 0.5 * (torch.diagonal(EL)[None, :] * (1.0 / ig + (1.0 / i_mu)[None, :])).sum()
    return (data + quad - 0.5 * G * e_logdet - 0.5 * (nu0 - K - 1.0) * e_logdet + 0.5 * (W0 * EL).sum() - entropy
            + (0.5 * kappa0 * ((e_mu - mu0) ** 2 + 1.0 / i_mu) + 0.5 * torch.log(i_mu)).sum() + 0.5 * torch.log(ig).sum()
            + 0.5 * tau_beta * ((m ** 2).sum() + (1.0 / ib).sum()) + 0.5 * torch.log(ib).sum())


def kl_free(free, x, y, z, w, o, gid, G, hyp, lik='logistic', gh_deg=20):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, gid, G, hyp, lik, gh_deg)


def default_hyp(K, tau_beta=1.0, mu0=0.0, kappa0=1.0, nu0=None, W0=None):
    W0 = np.eye(K) if W0 is None else np.asarray(W0, dtype=np.float64)
    r, c = np.tril_indices(K)
    return np.concatenate([[tau_beta, mu0, kappa0, K + 1.0 if nu0 is None else nu0], W0[r, c]])


def other_hyp(K):
    """A prior away from the defaults: nu0 = K + 2.5, W0 a full positive definite matrix."""
    A = 0.3 * np.arange(1, K * K + 1, dtype=np.float64).reshape(K, K) / K
    return default_hyp(K, 1.3, 0.2, 0.7, K + 2.5, np.eye(K) * 1.4 + 0.1 * (A @ A.T))


def targs(x, y, z, w, o, gid, G, hyp, lik='logistic'):
    """The argument tuple of `kl_vec` / `kl_free` behind the point."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return t(x), t(y), t(z), t(w), t(o), torch.tensor(np.asarray(gid, dtype=np.int64)), G, t(hyp), lik


def problem(N, P, K, G, seed, lik='logistic', hyp=None, **kw):
    """Data of `glmm_slopes_reference.problem` (logistic, o = 0) or `glmm_poisson_reference.problem`, and a point in the free
    coordinates of this model: (m, i_beta, e_mu, i_mu, e, i) are that module's, and q(Lambda) sits near its conjugate update
    given them under the prior of `hyp` (default `other_hyp(K)`) -- n = G + nu0, V = (W0 + S)^-1 with
    S = sum_g d_g d_g^T + diag(sum_g 1 / i_gk + G / i_mu_k) -- with the log-Cholesky entries of V moved by N(0, 0.05^2) and
    log(n - K + 1) by N(0, 0.1^2): at a random (n, V) the Hessian is indefinite at every seed tried for the wide shapes.
    Returns (x, y, z, w, gid, o, free)."""
    if lik == 'logistic':
        x, y, z, w, gid, f0 = sref.problem(N, P, K, G, seed, **kw)
        o = np.zeros(N)
    else:
        x, y, z, w, gid, o, f0 = pref.problem(N, P, K, G, seed, **kw)
    hyp = other_hyp(K) if hyp is None else np.asarray(hyp, dtype=np.float64)
    rng = np.random.default_rng([seed, 7])
    r, c = np.tril_indices(K)
    ng0 = 2 * P + 4 * K
    e_mu, i_mu = f0[2 * P:2 * P + K], np.exp(f0[2 * P + K:2 * P + 2 * K])
    e, ig = f0[ng0:ng0 + G * K].reshape(G, K), np.exp(f0[ng0 + G * K:]).reshape(G, K)
    d = e - e_mu[None, :]
    W0 = np.zeros((K, K))
    W0[r, c] = hyp[4:]
    W0 = W0 + W0.T - np.diag(np.diag(W0))
    L = np.linalg.cholesky(np.linalg.inv(W0 + d.T @ d + np.diag((1.0 / ig).sum(0) + G / i_mu)))
    chol = np.where(r == c, np.log(L[r, r]), L[r, c]) + 0.05 * rng.normal(size=r.size)
    free = np.concatenate([f0[:2 * P + 2 * K], [np.log(G + hyp[3] - (K - 1.0)) + 0.1 * rng.normal()], chol, f0[ng0:]])
    return x, y, z, w, gid, o, free


def data_pieces(x, y, z, w, o, gid, G, eta, lik='logistic'):
    """The data-dependent inputs of `glmm_corr_closed_forms` (those of `glmm_slopes_closed_forms`) from the per-row autograd
    derivatives of the two references this one shares its data term with."""
    P, K = x.shape[1], z.shape[1]
    _, ng, _ = sizes(P, K, G)
    eta = np.asarray(eta, dtype=np.float64)
    eta_s = np.concatenate([eta[:2 * P], np.ones(4 * K), eta[ng:]])          # the layout those modules read (m, i_beta, e, i) from
    if lik == 'logistic':
        return sref.data_pieces(x, y, z, w, gid, G, eta_s)
    return pref.data_pieces(x, y, z, w, o, gid, G, eta_s)

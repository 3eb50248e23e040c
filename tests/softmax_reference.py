"""Plain numpy fp64 reference of the multinomial (softmax) regression data term (no device, no torch).

beta is (K - 1) x P (row a = class a + 1, class 0 the reference), eta = vec(beta) row-major, w the observation weights:
    f = sum_n w_n [ log sum_k e^{z_nk} - z_{n, y_n} ],   z_n0 = 0,  z_na = x_n . beta_a
"""
import numpy as np


def logits(x, beta):
    z = np.zeros((x.shape[0], beta.shape[0] + 1))
    z[:, 1:] = x @ beta.T
    return z


def probs(x, beta):
    z = logits(x, beta)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    return (e / e.sum(axis=1, keepdims=True))[:, 1:]


def value(x, y, w, beta):
    z = logits(x, beta)
    m = np.maximum(z.max(axis=1), 0.0)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    return float(np.sum(w * (lse - z[np.arange(len(y)), y])))


def residuals(x, y, w, beta):
    """r_na = w_n (p_na - [y_n = a + 1]), N x (K - 1)."""
    p = probs(x, beta)
    e = np.zeros_like(p)
    rows = np.nonzero(y > 0)[0]
    e[rows, y[rows] - 1] = 1.0
    return w[:, None] * (p - e)


def grad(x, y, w, beta):
    return (residuals(x, y, w, beta).T @ x).ravel()


def hess_block(x, w, beta, a, b):
    p = probs(x, beta)
    c = w * p[:, a] * ((1.0 if a == b else 0.0) - p[:, b])
    return x.T @ (c[:, None] * x)


def hessian(x, w, beta):
    Km, P = beta.shape
    H = np.empty((Km * P, Km * P))
    for a in range(Km):
        for b in range(Km):
            H[a * P:(a + 1) * P, b * P:(b + 1) * P] = hess_block(x, w, beta, a, b)
    return H


def hvp(x, w, beta, v):
    p = probs(x, beta)
    t = x @ v.reshape(beta.shape).T
    u = w[:, None] * p * (t - (p * t).sum(axis=1, keepdims=True))
    return (u.T @ x).ravel()


def cross_hessian(x, y, beta):
    """d2 f / d eta d w_n: D x N, column n = vec((p_n - e_{y_n}) x_n^T)."""
    r = residuals(x, y, np.ones(x.shape[0]), beta)
    return np.einsum('na,np->apn', r, x).reshape(-1, x.shape[0])

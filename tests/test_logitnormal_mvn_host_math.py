"""Host pieces of `LogitNormalMVNRegressionObjective` (no GPU): the chain from (m, vech Sigma) to (m, vech Lambda) -- gradient,
Hessian (the formula the device chain evaluates) and the matrix-free product -- and the log-Cholesky product pieces, each
against torch fp64 autograd of the KL (tests/lmvn_reference.py).  Also the refusals that need no device."""
import numpy as np
import pytest
import torch

from lmvn_reference import coefs_f64, coefs_mp, kl_free, kl_mean_field, kl_vec, problem, psi, std_nodes, terms_from_coefs


def _import():
    import lrvb_amd.logitnormal_mvn as lm
    return lm


def _sig_derivs(x, y, w, m, Sigma, deg):
    """Data term's gradient and Hessian in (m, vech Sigma) by autograd (symmetric fill of the off-diagonal coordinate)."""
    P = x.shape[1]
    r, c = np.tril_indices(P)
    xt, yt, wt = (torch.tensor(a) for a in (x, y, w))

    def data(z):
        A = torch.zeros((P, P), dtype=torch.float64).index_put((torch.tensor(r), torch.tensor(c)), z[P:])
        S = A + torch.tril(A, -1).T
        mu = xt @ z[:P]
        s = torch.einsum('ni,ij,nj->n', xt, S, xt)
        return (wt * (psi(mu, s, deg) - yt * mu)).sum()

    z = torch.tensor(np.concatenate([m, Sigma[r, c]]), requires_grad=True)
    g = torch.autograd.grad(data(z), z)[0].numpy()
    H = torch.autograd.functional.hessian(data, z.detach()).numpy()
    return g, H


def _symkron(A, B):
    """tr(A E_r B E_c) over vech coordinates r, c (E = symmetric unit matrices)."""
    P = A.shape[0]
    r, c = np.tril_indices(P)
    i, j = r[:, None], c[:, None]
    p, q = r[None, :], c[None, :]
    v = A[i, p] * B[j, q]
    v = v + np.where(i != j, A[j, p] * B[i, q], 0.0)
    v = v + np.where(p != q, A[i, q] * B[j, p], 0.0)
    v = v + np.where((i != j) & (p != q), A[j, q] * B[i, p], 0.0)
    return v


@pytest.mark.parametrize('P', [1, 2, 5])
def test_chain_to_vech_lambda_matches_autograd(P):
    lm = _import()
    tau, deg = 0.7, 12
    x, y, w, free, Lam = problem(60, P, seed=P)
    Sigma = np.linalg.inv(Lam)
    m = free[:P]
    g_sig, H_sig = _sig_derivs(x, y, w, m, Sigma, deg)
    eta = torch.tensor(np.concatenate([m, Lam[np.tril_indices(P)]]), requires_grad=True)
    args = (torch.tensor(x), torch.tensor(y), torch.tensor(w), tau, deg)
    g_ref = torch.autograd.grad(kl_vec(eta, *args), eta)[0].numpy()
    H_ref = torch.autograd.functional.hessian(lambda e: kl_vec(e, *args), eta.detach()).numpy()
    g, M, _ = lm.chain_grad(P, Sigma, m, g_sig, tau)
    assert np.max(np.abs(g - g_ref)) <= 1e-10 * np.max(np.abs(g_ref))
    # the Hessian formula of lrvb_logitnormal_mvn_chain: J^T H J + 2 symkron(M, Sigma) - 1/2 symkron(Sigma, Sigma)
    Pv = P * (P + 1) // 2
    S = _symkron(Sigma, Sigma)
    d = lm._delta(P)
    J = np.eye(P + Pv)
    J[P:, P:] = -S / d[:, None]
    H = J.T @ H_sig @ J
    H[P:, P:] += 2.0 * _symkron(M, Sigma) - 0.5 * S
    H[:P, :P] += tau * np.eye(P)
    assert np.max(np.abs(H - H_ref)) <= 1e-9 * np.max(np.abs(H_ref))
    # the matrix-free product, vector coordinates
    rng = np.random.default_rng(1)
    for _ in range(3):
        v = rng.normal(size=P + Pv)
        hv = lm.chain_hvp(P, Sigma, M, v, lambda u: H_sig @ u)
        hv[:P] += tau * v[:P]
        assert np.max(np.abs(hv - H_ref @ v)) <= 1e-10 * np.max(np.abs(H_ref @ v))


@pytest.mark.parametrize('P', [1, 3])
def test_free_coordinate_product_pieces_match_autograd(P):
    lm = _import()
    tau, deg = 0.5, 10
    x, y, w, free, Lam = problem(40, P, seed=10 + P)
    args = (torch.tensor(x), torch.tensor(y), torch.tensor(w), tau, deg)
    Pv = P * (P + 1) // 2
    H_ref = torch.autograd.functional.hessian(lambda f: kl_free(f, *args), torch.tensor(free)).numpy()
    Sigma = np.linalg.inv(Lam)
    m = free[:P]
    g_sig, H_sig = _sig_derivs(x, y, w, m, Sigma, deg)
    g_vec, M, _ = lm.chain_grad(P, Sigma, m, g_sig, tau)
    rng = np.random.default_rng(2)
    for _ in range(3):
        u = rng.normal(size=P + Pv)
        v_lam = np.concatenate([u[:P], lm.psd_free_jvp(free[P:], u[P:], P)])
        hv = lm.chain_hvp(P, Sigma, M, v_lam, lambda z: H_sig @ z)
        hv[:P] += tau * v_lam[:P]
        out = np.concatenate([hv[:P], lm.psd_free_vjp_hvp(free[P:], u[P:], hv[P:], g_vec[P:], P)])
        ref = H_ref @ u
        assert np.max(np.abs(out - ref)) <= 1e-10 * np.max(np.abs(ref))


@pytest.mark.parametrize('P', [1, 3])
def test_edge_references_agree_with_autograd(P):
    """The per-row coefficients of tests/lmvn_reference.py (fp64, assembled with an explicit U) against autograd of the data
    term, and against mpmath row by row, at a point with an all-zero row and a row with |mu| ~ 300."""
    x, y, w, free, Lam = problem(40, P, seed=P)
    y[3] = 0.3
    m, S = free[:P], np.linalg.inv(Lam)
    S = 0.5 * (S + S.T)
    nodes, weights = std_nodes(20)
    c = coefs_f64(x, y, w, m, S, nodes, weights)
    _, g, H = terms_from_coefs(x, c)
    g_ref, H_ref = _sig_derivs(x, y, w, m, S, 20)
    assert np.max(np.abs(g - g_ref)) <= 1e-13 * np.max(np.abs(g_ref))
    assert np.max(np.abs(H - H_ref)) <= 1e-13 * np.max(np.abs(H_ref))
    mu, s = x @ m, np.einsum('ni,ij,nj->n', x, S, x)
    for n in range(0, 40, 7):
        cm = coefs_mp(mu[n], max(s[n], 0.0), y[n], w[n], nodes, weights)
        for k, v in cm.items():
            assert abs(c[k][n] - v) <= 1e-15 * w[n] * (1 + abs(mu[n])) + 1e-13 * abs(v)


def test_mean_field_reference_matches_oracle():
    """kl_mean_field (the mean-field model's KL for the GPU edge tests) against the numpy oracle of the model."""
    from oracle import logitnormal as ol
    from test_logitnormal_host_math import problem as mf_problem
    x, y, w, eta = mf_problem(50, 4, seed=1)
    gx, gw = np.polynomial.hermite.hermgauss(20)
    o_val, o_g, o_H = ol.kl_terms(eta, x, y, w, 0.7, gx, gw)
    args = (torch.tensor(x), torch.tensor(y), torch.tensor(w), 0.7, 20)
    et = torch.tensor(eta, requires_grad=True)
    val = kl_mean_field(et, *args)
    g = torch.autograd.grad(val, et)[0].numpy()
    H = torch.autograd.functional.hessian(lambda t: kl_mean_field(t, *args), torch.tensor(eta)).numpy()
    assert abs(val.item() - o_val) <= 1e-13 * abs(o_val)
    assert np.max(np.abs(g - o_g)) <= 1e-13 * np.max(np.abs(o_g))
    assert np.max(np.abs(H - o_H)) <= 1e-13 * np.max(np.abs(o_H))


def test_refusals_before_any_device_call():
    import lrvb_amd as vb
    par = vb.ModelParamsDict('p')
    par.push_param(vb.MVNParam('beta', dim=65))
    with pytest.raises(NotImplementedError, match='P <= 64'):
        vb.LogitNormalMVNRegressionObjective(par, np.zeros((4, 65)), np.zeros(4))
    par = vb.ModelParamsDict('p')
    par.push_param(vb.MVNParam('beta', dim=3))
    with pytest.raises(ValueError, match='y has'):
        vb.LogitNormalMVNRegressionObjective(par, np.zeros((4, 3)), np.zeros(5))
    with pytest.raises(ValueError, match='nodes'):
        vb.LogitNormalMVNRegressionObjective(par, np.zeros((4, 3)), np.zeros(4), gh_deg=129)
    par2 = vb.ModelParamsDict('p')
    par2.push_param(vb.UVNParamVector('beta', length=3))
    with pytest.raises(ValueError, match='MVNParam'):
        vb.LogitNormalMVNRegressionObjective(par2, np.zeros((4, 3)), np.zeros(4))

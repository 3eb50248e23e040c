"""Edges of the full-covariance logistic regression kernels (`LogitNormalMVNRegressionObjective`) and the weight cross
Hessians of both logit-normal classes, against references that share no formula with the kernels (tests/lmvn_reference.py):
per-row coefficients by scipy / np.logaddexp in fp64 or mpmath at 40 digits, assembled with an explicit U, and torch fp64
autograd of the KL.

Kernel edges and the cases that reach them:
  lmvn_rowpass_kernel, 32-row tiles: N < 32 (one partial tile), N = 31 / 32 / 33
  lmvn_cross_kernel, 16-row stages, splits of >= 256 rows: N < 256 (one split), N = 15 / 16 / 17, 255 / 256 / 257, 4095 / 4097
  lmvn_cross_kernel, 64-column slices of the packed triangle: P = 11, 19, 37 (Pv = 66, 190, 703) and P = 64 (Pv = 2080)
  wsyrk_kron_kernel, at least 8 splits: N < 256 leaves splits empty, every P from 1 to 64 in the sweep
  lmvn_coef_kernel, 128-node LDS table: K = 1, 2, 3, 63, 64, 65, 127, 128
  exp(-|t|) underflow (|t| > 745): mu = +-800 and s = 1e4
Tolerances as in test_gpu_logitnormal_mvn.py: value 1e-11, gradient 1e-10, Hessian 1e-9 relative, symmetry 1e-12."""
import numpy as np
import pytest
import torch

from lmvn_reference import (coefs_f64, coefs_mp, kl_free, kl_mean_field, kl_vec, problem, std_nodes, terms_from_coefs)

pytestmark = pytest.mark.gpu

N_GRID = [1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4097, 65539]
P_GRID = [1, 2, 3, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64]
ALWAYS = [(1, 64), (17, 64), (257, 63), (4097, 1), (33, 11), (4095, 11), (255, 19), (257, 19), (16, 37), (4097, 37)]


def _sweep():
    """About 40 seeded (N, P) pairs of the grid whose host reference (N Pv^2 multiply-adds) stays small, plus ALWAYS."""
    rng = np.random.default_rng(2024)
    pairs = [(N, P) for N in N_GRID for P in P_GRID if N * (P * (P + 1) // 2) ** 2 <= 4e9]
    pick = [pairs[i] for i in rng.choice(len(pairs), size=30, replace=False)]
    return sorted(set(pick) | set(ALWAYS))


SWEEP = _sweep()


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _model(vb, x, y, w, tau=0.7, deg=20):
    par = vb.ModelParamsDict('params')
    par.push_param(vb.MVNParam('beta', dim=x.shape[1]))
    return par, vb.LogitNormalMVNRegressionObjective(par, x, y, prior_info=tau, gh_deg=deg, weights=w)


def _model_mf(vb, x, y, w, tau=0.7, deg=20):
    par = vb.ModelParamsDict('mf')
    par.push_param(vb.UVNParamVector('beta', length=x.shape[1]))
    return par, vb.LogitNormalRegressionObjective(par, x, y, prior_info=tau, gh_deg=deg, weights=w)


def _data(N, P, seed):
    """lmvn_reference.problem (one all-zero row, one row with |mu| ~ 300) once there are rows to spare, plain rows below."""
    x, y, w, free, Lam = problem(N, P, seed, with_extremes=N >= 8)
    S = np.linalg.inv(Lam)
    return x, y, w, free, free[:P].copy(), 0.5 * (S + S.T)


def _check_terms(fun, x, y, w, m, S, nodes, weights):
    val, g, H = fun.mvn_terms(m, S)
    v_ref, g_ref, H_ref = terms_from_coefs(x, coefs_f64(x, y, w, m, S, nodes, weights))
    assert abs(val - v_ref) <= 1e-11 * max(abs(v_ref), 1e-300)
    assert rel(g, g_ref) <= 1e-10
    assert rel(H, H_ref) <= 1e-9
    assert rel(H, H.T) <= 1e-12
    return H_ref


# ---- 2 and 5: shape sweep through the tile and split geometry ------------------------------------------------------------
@pytest.mark.parametrize('N,P', SWEEP)
def test_shape_sweep_terms_and_hvp_match_reference(vb, N, P):
    x, y, w, free, m, S = _data(N, P, seed=7 * N + P)
    par, fun = _model(vb, x, y, w)
    H_ref = _check_terms(fun, x, y, w, m, S, *std_nodes(20))
    rng = np.random.default_rng(N + 100 * P)
    for kind in ('mean', 'sigma', 'both'):
        v = rng.normal(size=H_ref.shape[0])
        if kind == 'mean':
            v[P:] = 0.0
        elif kind == 'sigma':
            v[:P] = 0.0
        ref = H_ref @ v
        assert rel(fun.mvn_hvp(m, S, v), ref) <= 1e-10, kind


# ---- 3: quadrature degrees at the edges of the node table ---------------------------------------------------------------
def test_quadrature_degrees_match_reference(vb):
    N, P = 257, 17
    x, y, w, free, m, S = _data(N, P, seed=3)
    par, fun = _model(vb, x, y, w)
    for K in (1, 2, 3, 63, 64, 65, 127, 128):
        fun.gh_x, fun.gh_w = np.polynomial.hermite.hermgauss(K)
        _check_terms(fun, x, y, w, m, S, *std_nodes(K))


def test_free_coordinates_at_128_nodes_match_autograd(vb):
    N, P, tau, K = 301, 3, 0.7, 128
    x, y, w, free, _ = problem(N, P, seed=128)
    par, fun = _model(vb, x, y, w, tau, K)
    args = (torch.tensor(x), torch.tensor(y), torch.tensor(w), tau, K)
    ft = torch.tensor(free, requires_grad=True)
    val = kl_free(ft, *args)
    g_ref = torch.autograd.grad(val, ft)[0].numpy()
    H_ref = torch.autograd.functional.hessian(lambda f: kl_free(f, *args), torch.tensor(free)).numpy()
    assert abs(fun.value(free) - val.item()) <= 1e-11 * abs(val.item())
    assert rel(fun.grad(free), g_ref) <= 1e-10
    assert rel(fun.hessian(free), H_ref) <= 1e-9


# ---- 4: coefficient regimes, one observation against mpmath -----------------------------------------------------------
MUS = [0.0, 1e-8, -1e-8, 30.0, -30.0, 300.0, -300.0, 800.0, -800.0]
SS = [0.0, 1e-300, 1e-6, 1.0, 1e4]
WS = [0.0, 1e-300, 1.0, 1e6]


@pytest.mark.parametrize('y', [0.0, 1.0, 0.3])
def test_coefficient_regimes_match_mpmath(vb, y):
    """P = 1, x = 1: the gradient in (m, Sigma) is (a1, a2) and the Hessian [[c11, c12], [c12, c22]], so every coefficient is
    read directly.  Bounds |dev - ref| <= atol + 1e-12 |ref|, atol = 2e-15 w (1e-15 w (1 + |mu| + 10 sqrt(s)) for the value):
    a few ulps of the O(1) per-node terms, scaled by the weight, so w = 0 must give exact zeros."""
    nodes, weights = std_nodes(20)
    par, fun = _model(vb, np.ones((1, 1)), np.array([y]), np.ones(1))
    for w in WS:
        fun.weights_par.set_vector(np.array([w]))
        for mu in MUS:
            for s in SS:
                val, g, H = fun.mvn_terms(np.array([mu]), np.array([[s]]))
                got = dict(value=val, a1=g[0], a2=g[1], c11=H[0, 0], c12=H[0, 1], c22=H[1, 1])
                assert np.all(np.isfinite(g)) and np.all(np.isfinite(H)) and np.isfinite(val)
                assert H[0, 1] == H[1, 0]
                ref = coefs_mp(mu, s, y, w, nodes, weights)
                for k, r in ref.items():
                    atol = w * (1e-15 * (1 + abs(mu) + 10 * np.sqrt(s)) if k == 'value' else 2e-15)
                    assert abs(got[k] - r) <= atol + 1e-12 * abs(r), (k, mu, s, y, w, got[k], r)


# ---- 5: the free-coordinate matrix-free product against autograd ------------------------------------------------------
@pytest.mark.parametrize('P', [1, 7, 64])
def test_free_hvp_matches_autograd(vb, P):
    N, tau = 1001, 0.7
    x, y, w, free, _ = problem(N, P, seed=40 + P)
    par, fun = _model(vb, x, y, w, tau)
    args = (torch.tensor(x), torch.tensor(y), torch.tensor(w), tau, 20)
    rng = np.random.default_rng(P)
    for _ in range(2):
        u = rng.normal(size=free.size)
        _, hv = torch.autograd.functional.hvp(lambda f: kl_free(f, *args), torch.tensor(free), torch.tensor(u))
        assert rel(fun.hvp(free, u), hv.numpy()) <= 1e-10


# ---- 6: weight cross Hessians of both logit-normal classes ------------------------------------------------------------
def _cross_ref(kl, theta, w):
    """d2 KL / d theta d w^T (D x N) by torch fp64 autograd: the Jacobian in w of the gradient in theta, and the Hessian."""
    th = torch.tensor(theta)
    grad = lambda wt: torch.autograd.functional.jacobian(lambda t: kl(t, wt), th, create_graph=True)
    G = torch.autograd.functional.jacobian(grad, torch.tensor(w)).numpy()
    H = torch.autograd.functional.hessian(lambda t: kl(t, torch.tensor(w)), th).numpy()
    return G, H


def _mf_problem(N, P, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    y = (rng.uniform(size=N) < 0.5).astype(float)
    y[3] = 0.3                                           # a fractional response
    w = rng.uniform(0.5, 1.5, size=N)
    mean, info = rng.normal(size=P) * 0.5, rng.uniform(1.0, 4.0, size=P)
    x[0] = 0.0                                           # v = 0, mu = 0
    x[:, 0] = 0.0
    x[1, 0] = 3.0                                        # mu_1 ~ 300
    mean[0], info[0] = 100.0, 100.0
    return x, y, w, np.concatenate([mean, info])


def _sensitivity_matches(vb, fun, par, theta, H_ref, G_ref):
    sens = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, theta, fun.weights_par.get_vector().copy())
    assert rel(sens.get_dinput_dhyper(), -np.linalg.solve(H_ref, G_ref)) <= 1e-9


@pytest.mark.parametrize('is_free', [True, False])
def test_mvn_weight_cross_hessian_matches_autograd(vb, is_free):
    N, P, tau = 40, 4, 0.7
    x, y, w, free, _ = problem(N, P, seed=6)
    y[3] = 0.3
    par, fun = _model(vb, x, y, w, tau)
    xt, yt = torch.tensor(x), torch.tensor(y)
    if is_free:
        theta = free
        kl = lambda t, wt: kl_free(t, xt, yt, wt, tau, 20)
    else:
        theta = fun.ctx.constrain(free)
        kl = lambda t, wt: kl_vec(t, xt, yt, wt, tau, 20)
    G_ref, H_ref = _cross_ref(kl, theta, w)
    G = fun.cross_hessian(fun.weights_par, theta, is_free)
    assert G.shape == G_ref.shape and np.all(np.isfinite(G))
    assert rel(G, G_ref) <= 1e-10
    if is_free:
        _sensitivity_matches(vb, fun, par, theta, H_ref, G_ref)


@pytest.mark.parametrize('is_free', [True, False])
def test_mean_field_weight_cross_hessian_matches_autograd(vb, is_free):
    """The all-zero row (v = 0) has an exactly zero column: the weight does not reach the gradient through x_n = 0."""
    N, P, tau = 40, 4, 0.7
    x, y, w, eta = _mf_problem(N, P, seed=8)
    par, fun = _model_mf(vb, x, y, w, tau)
    xt, yt = torch.tensor(x), torch.tensor(y)
    theta = np.concatenate([eta[:P], np.log(eta[P:])]) if is_free else eta
    if is_free:
        kl = lambda t, wt: kl_mean_field(torch.cat([t[:P], torch.exp(t[P:])]), xt, yt, wt, tau, 20)
    else:
        kl = lambda t, wt: kl_mean_field(t, xt, yt, wt, tau, 20)
    G_ref, H_ref = _cross_ref(kl, theta, w)
    assert np.all(G_ref[:, 0] == 0.0)
    G = fun.cross_hessian(fun.weights_par, theta, is_free)
    assert G.shape == G_ref.shape
    assert np.all(np.isfinite(G)), 'non-finite columns: {}'.format(np.where(~np.all(np.isfinite(G), axis=0))[0])
    assert rel(G, G_ref) <= 1e-10
    assert rel(fun.hessian(theta, is_free), H_ref) <= 1e-9
    if is_free:
        _sensitivity_matches(vb, fun, par, theta, H_ref, G_ref)


# ---- 7: sharding and call order ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('cuts', [(1,), (17,), (100, 433)], ids=['1+rest', '17+rest', 'three'])
def test_ragged_shards_sum_to_the_whole(vb, cuts):
    N, P = 1001, 6
    x, y, w, free, _ = problem(N, P, seed=17)
    par, whole = _model(vb, x, y, w)
    eta = whole.ctx.constrain(free)
    s_all = whole.local_stats(eta)
    edges = [0, *cuts, N]
    parts = [_model(vb, x[a:b], y[a:b], w[a:b])[1].local_stats(eta) for a, b in zip(edges[:-1], edges[1:])]
    assert rel(np.sum(parts, axis=0), s_all) <= 1e-12


def _residual(z, H, b):
    return np.linalg.norm(H @ z - b) / np.linalg.norm(b)


def test_call_order_value_hessian_hvp_weights_hessian(vb):
    """The row pass, the cross kernel and the Kronecker SYRK share the context's scratch buffers (c->lmvn, c->tile_part,
    c->Hfree; the chain reuses Hfree and Heta): every result of this sequence must match the reference of its own inputs."""
    N, P, tau = 301, 5, 0.7
    x, y, w, free_a, _ = problem(N, P, seed=77)
    free_b = free_a + 0.05 * np.random.default_rng(1).normal(size=free_a.size)
    par, fun = _model(vb, x, y, w, tau)
    xt, yt = torch.tensor(x), torch.tensor(y)
    kl = lambda f, wv: kl_free(f, xt, yt, torch.tensor(wv), tau, 20)
    hess = lambda f, wv: torch.autograd.functional.hessian(lambda t: kl(t, wv), torch.tensor(f)).numpy()
    b = np.random.default_rng(2).normal(size=free_a.size)

    v_ref = kl(torch.tensor(free_a), w).item()
    assert abs(fun.value(free_a) - v_ref) <= 1e-11 * abs(v_ref)                              # 1. value
    H_a = hess(free_a, w)
    assert rel(fun.hessian(free_a), H_a) <= 1e-9                                             # 2. Hessian at A
    assert _residual(fun.cg_solve(free_a, b, tol=1e-12)[0], H_a, b) <= 1e-10
    u = np.random.default_rng(3).normal(size=free_a.size)
    assert rel(fun.hvp(free_b, u), hess(free_b, w) @ u) <= 1e-10                             # 3. HVP at B
    w2 = w.copy()
    w2[::3] *= 2.5
    w2[5] = 0.0
    fun.weights_par.set_vector(w2)                                                           # 4. weights change
    H_a2 = hess(free_a, w2)
    assert rel(fun.hessian(free_a), H_a2) <= 1e-9                                            # 5. Hessian at A again
    assert _residual(fun.cg_solve(free_a, b, tol=1e-12)[0], H_a2, b) <= 1e-10               # (and the cached one)

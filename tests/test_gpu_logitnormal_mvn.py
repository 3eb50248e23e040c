"""Logistic regression with a full-covariance Gaussian posterior on the GPU (`LogitNormalMVNRegressionObjective`).
Reference: torch fp64 autograd of the KL in free coordinates (tests/lmvn_reference.py) and numpy with an explicit
U (rows = packed lower triangle of x_n x_n^T).  Tolerances: value 1e-11, gradient 1e-10, Hessian 1e-9 relative."""
import numpy as np
import pytest
import scipy.optimize
import torch

from lmvn_reference import kl_free, problem

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize('P', [1, 2, 7, 16, 31, 33, 63, 64])
def test_value_gradient_hessian_match_autograd(vb, P):
    N, tau, deg = 2000, 0.7, 20
    x, y, w, free, _ = problem(N, P, seed=P)
    par, fun = _model(vb, x, y, w, tau, deg)
    args = (torch.tensor(x), torch.tensor(y), torch.tensor(w), tau, deg)
    ft = torch.tensor(free, requires_grad=True)
    val = kl_free(ft, *args)
    g_ref = torch.autograd.grad(val, ft)[0].numpy()
    assert abs(fun.value(free) - val.item()) <= 1e-11 * abs(val.item())
    assert rel(fun.grad(free), g_ref) <= 1e-10
    if P <= 7:
        H_ref = torch.autograd.functional.hessian(lambda f: kl_free(f, *args), torch.tensor(free)).numpy()
        assert rel(fun.hessian(free), H_ref) <= 1e-9
    else:
        # Hessian columns by forward-over-reverse products instead of the full AD Hessian
        rng = np.random.default_rng(P)
        H = fun.hessian(free)
        for _ in range(2):
            u = torch.tensor(rng.normal(size=free.size))
            _, hv = torch.autograd.functional.hvp(lambda f: kl_free(f, *args), torch.tensor(free), u)
            assert rel(H @ u.numpy(), hv.numpy()) <= 1e-9


def _host_coefs(x, y, w, m, S, deg):
    gx, gw = np.polynomial.hermite.hermgauss(deg)
    xk, wk = np.sqrt(2) * gx, gw / np.sqrt(np.pi)
    mu = x @ m
    s = np.maximum(np.einsum('ni,ij,nj->n', x, S, x), 0.0)
    t = mu[:, None] + np.sqrt(s)[:, None] * xk[None, :]
    sg = 1 / (1 + np.exp(-t))
    g2 = sg * (1 - sg)
    g3 = g2 * (1 - 2 * sg)
    g4 = g2 * (1 - 6 * g2)
    E = lambda a: a @ wk
    return dict(a1=w * (E(sg) - y), a2=w * 0.5 * E(g2), c11=w * E(g2), c12=w * 0.5 * E(g3), c22=w * 0.25 * E(g4))


def test_vector_blocks_match_explicit_U_at_P64(vb):
    N, P = 8000, 64
    x, y, w, free, Lam = problem(N, P, seed=3)
    par, fun = _model(vb, x, y, w)
    m, S = free[:P], np.linalg.inv(Lam)
    S = 0.5 * (S + S.T)
    val, g, H = fun.mvn_terms(m, S)
    c = _host_coefs(x, y, w, m, S, 20)
    r, cc = np.tril_indices(P)
    d = np.where(r == cc, 1.0, 2.0)
    U = x[:, r] * x[:, cc]
    g_ref = np.concatenate([x.T @ c['a1'], d * (U.T @ c['a2'])])
    H_ref = np.block([[x.T @ (c['c11'][:, None] * x), (x.T @ (c['c12'][:, None] * U)) * d[None, :]],
                      [((x.T @ (c['c12'][:, None] * U)) * d[None, :]).T, d[:, None] * (U.T @ (c['c22'][:, None] * U)) * d[None, :]]])
    assert rel(g, g_ref) <= 1e-10
    assert rel(H, H_ref) <= 1e-9
    assert rel(H, H.T) <= 1e-12


def test_diagonal_lambda_matches_mean_field(vb):
    N, P = 3000, 9
    rng = np.random.default_rng(5)
    x = rng.normal(size=(N, P)) / 3.0
    x[0] = 0.0
    y = (rng.uniform(size=N) < 0.5).astype(float)
    w = rng.uniform(0.5, 1.5, size=N)
    m, info = rng.normal(size=P) * 0.4, rng.uniform(2.0, 5.0, size=P)
    par, fun = _model(vb, x, y, w)
    parm = vb.ModelParamsDict('mf')
    parm.push_param(vb.UVNParamVector('beta', length=P))
    mf = vb.LogitNormalRegressionObjective(parm, x, y, prior_info=0.7, gh_deg=20, weights=w)
    Lam = np.diag(info)
    eta = np.concatenate([m, Lam[np.tril_indices(P)]])
    eta_mf = np.concatenate([m, info])
    assert abs(fun.value(eta, False) - mf.value(eta_mf, False)) <= 1e-12 * abs(mf.value(eta_mf, False))
    assert rel(fun.grad(eta, False)[:P], mf.grad(eta_mf, False)[:P]) <= 1e-12


@pytest.mark.parametrize('P', [5, 33])
def test_matrix_free_hvp(vb, P):
    x, y, w, free, _ = problem(2500, P, seed=20 + P)
    par, fun = _model(vb, x, y, w)
    D = free.size
    rng = np.random.default_rng(P)
    eta = fun.ctx.constrain(free)
    # device-side evidence: every sum over observations of the C entry points passes the (single-rank, identity) reduce hook,
    # which records its length
    sizes = []
    fun.ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))
    for is_free, pt in ((True, free), (False, eta)):
        H = fun.hessian(pt, is_free)
        assert max(sizes) == D * D + D + 1                   # the build reduces [H | g | value] once
        del sizes[:]
        for _ in range(3):
            v = rng.normal(size=D)
            assert rel(fun.hvp(pt, v, is_free), H @ v) <= 1e-10
        assert max(sizes) <= D + 1                           # the products never reduce (so never form) a D x D block
    fun.ctx.set_reduce_hook(None)


def _fit(vb, objective, D, x0=None):
    x0 = np.zeros(D) if x0 is None else x0
    return scipy.optimize.minimize(objective.fun_free, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp, x0=x0,
                                   method='trust-ncg', options={'gtol': 1e-8, 'maxiter': 200})


@pytest.mark.parametrize('P', [8, 64])
def test_fit_lrvb_covariance_and_weight_sensitivity(vb, P):
    N = 4000 if P == 8 else 6000
    rng = np.random.default_rng(P)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    beta = rng.normal(size=P) * 1.5
    y = (rng.uniform(size=N) < 1 / (1 + np.exp(-x @ beta))).astype(float)
    par, fun = _model(vb, x, y, None, tau=0.5)
    objective = vb.Objective(par, fun)
    D = P + P * (P + 1) // 2
    opt = _fit(vb, objective, D)
    theta = opt.x
    assert np.linalg.norm(objective.fun_free_grad(theta)) < 1e-6
    H = objective.fun_free_hessian(theta)
    fun.ctx.chol_factor(H)
    Msel = np.eye(D)[:P]
    cov = fun.ctx.lrvb_cov(Msel)
    np.testing.assert_allclose(cov, Msel @ np.linalg.solve(H, Msel.T), rtol=1e-6, atol=0)
    if P != 8:
        return
    sens = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, theta, np.ones(N))
    dth = sens.get_dinput_dhyper()
    n = int(np.argmax(np.abs(dth[:P]).sum(axis=0)))
    errs = []
    for dw in (-0.5, -0.25):                              # halve, then quarter the cut of one observation's weight
        wv = np.ones(N); wv[n] = 1.0 + dw
        fun.weights_par.set_vector(wv)
        th2 = _fit(vb, objective, D, theta).x
        pred = dw * dth[:, n]
        errs.append(np.max(np.abs(th2 - theta - pred)))
        assert errs[-1] <= 0.02 * np.max(np.abs(pred))
    fun.weights_par.set_vector(np.ones(N))
    assert 3.0 <= errs[0] / errs[1] <= 5.5                # the residual of the linear prediction is second order: x 4


def test_sharded_stats_sum_to_the_whole(vb):
    x, y, w, free, _ = problem(3000, 6, seed=11)
    P = 6
    par, whole = _model(vb, x, y, w)
    _, a = _model(vb, x[:1400], y[:1400], w[:1400])
    _, b = _model(vb, x[1400:], y[1400:], w[1400:])
    eta = whole.ctx.constrain(free)
    s_all, s_a, s_b = whole.local_stats(eta), a.local_stats(eta), b.local_stats(eta)
    assert rel(s_a + s_b, s_all) <= 1e-12
    a.set_reduced_stats(s_a + s_b, eta)
    assert rel(a.hessian(free), whole.hessian(free)) <= 1e-11
    assert rel(a.grad(free), whole.grad(free)) <= 1e-11


def test_refusals(vb):
    import lrvb_amd._hip as h
    rng = np.random.default_rng(0)
    x = rng.normal(size=(50, 65))
    ctx = vb.DeviceContext([dict(kind=0, free_size=65, vec_size=65, dim0=65, dim1=0, lb=-np.inf, ub=np.inf)],
                           loss='logistic', n_obs=50, n_cols=65)
    ctx.set_data(h.SLOT_X, x)
    ctx.set_data(h.SLOT_Y, np.zeros(50))
    gx, gw = np.polynomial.hermite.hermgauss(5)
    val = np.empty(1)
    st = h.load().lrvb_logitnormal_mvn_terms(ctx._h, h.ptr(np.zeros(65)), h.ptr(np.eye(65)), 65, h.ptr(gx), h.ptr(gw), 5,
                                               h.ptr(val), None, None)
    assert st == h.ERR_UNSUPPORTED and 'P <= 64' in h.last_error()
    x, y, w, free, _ = problem(100, 3, seed=1)
    par, fun = _model(vb, x, y, w)
    gx, gw = np.polynomial.hermite.hermgauss(129)
    fun.gh_x, fun.gh_w = gx, gw
    with pytest.raises(NotImplementedError, match='quadrature nodes'):
        fun.value(free)


def test_full_size_hessian_symmetric_pd_rows_match_host(vb):
    N, P = 1_000_000, 64
    rng = np.random.default_rng(64)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    beta = rng.normal(size=P)
    y = (rng.uniform(size=N) < 1 / (1 + np.exp(-x @ beta))).astype(float)
    par, fun = _model(vb, x, y, None, tau=1.0)
    D = P + P * (P + 1) // 2
    # Newton from the Laplace-like start: converges in a few steps at this N
    Lam0 = np.eye(P) + 0.25 * (x.T @ x)
    L0 = np.linalg.cholesky(Lam0)
    fl = L0[np.tril_indices(P)].copy()
    r, c = np.tril_indices(P)
    fl[r == c] = np.log(np.diag(L0))
    theta = np.concatenate([np.zeros(P), fl])
    for _ in range(8):
        g = fun.grad(theta)
        if np.linalg.norm(g) < 1e-6:
            break
        H = fun.hessian(theta)
        theta = theta - np.linalg.solve(H, g)
    H = fun.hessian(theta)
    assert np.linalg.norm(fun.grad(theta)) < 1e-5
    assert rel(H, H.T) <= 1e-12
    np.linalg.cholesky(0.5 * (H + H.T))
    # rows of the data-term Hessian in (m, vech Sigma) against the host, in chunks of rows
    eta = fun.ctx.constrain(theta)
    m, S, _ = fun._point(eta)
    _, _, Hs = fun.mvn_terms(m, S)
    d = np.where(r == c, 1.0, 2.0)
    rows = np.sort(rng.choice(D, size=6, replace=False))
    acc = np.zeros((rows.size, D))
    for n0 in range(0, N, 50_000):
        xb = x[n0:n0 + 50_000]
        cf = _host_coefs(xb, y[n0:n0 + 50_000], np.ones(len(xb)), m, S, 20)
        U = xb[:, r] * xb[:, c] * d[None, :]
        for k, row in enumerate(rows):
            t = xb[:, row] if row < P else U[:, row - P]
            ca, cb = (cf['c11'], cf['c12']) if row < P else (cf['c12'], cf['c22'])
            acc[k, :P] += xb.T @ (t * ca)
            acc[k, P:] += U.T @ (t * cb)
    assert rel(Hs[rows], acc) <= 1e-9

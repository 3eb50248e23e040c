"""Multinomial (softmax) regression on the GPU (k_softmax.hip): value, gradient, Hessian and the matrix-free
product against torch fp64 autograd and the numpy reference (tests/softmax_reference.py, itself pinned by autograd in
tests/test_softmax_host_math.py); K = 2 against the logistic GLM (a second device route); extreme logits; fit, LRVB covariance,
CG; weight sensitivity (dense and streamed rows, and a refit); the full-size Hessian and gradient against torch on the GPU;
the reduce-hook contract; the C ABI refusals."""
import ctypes

import numpy as np
import pytest
import scipy.optimize
import torch

import softmax_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if b.size else 0.0


def _problem(rng, N, P, K, scale=1.0):
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    y = rng.integers(0, K, size=N)
    w = rng.uniform(0.2, 2.0, size=N)
    w[1::4] = 0.0                                   # zero weights (row 0 keeps a positive one)
    beta = rng.normal(size=(K - 1, P)) * scale
    return x, y, w, beta


def _model(vb, x, y, w, K, tau=0.5, lb=-np.inf, ub=np.inf):
    par = vb.ModelParamsDict('par')
    par.push_param(vb.ArrayParam('beta', shape=(K - 1, x.shape[1]), lb=lb, ub=ub))
    fun = vb.SoftmaxRegressionObjective(par, x, y, K, prior_info=tau, weights=w)
    return par, fun, vb.Objective(par, fun)


def _torch_f(x, y, w, K, tau, lb=None, ub=None):
    X, W = torch.as_tensor(x), torch.as_tensor(w)
    Y = torch.as_tensor(y, dtype=torch.long)

    def f(theta):
        eta = theta if lb is None else lb + (ub - lb) / (1.0 + torch.exp(-theta))
        z = torch.cat([torch.zeros(X.shape[0], 1, dtype=torch.float64), X @ eta.reshape(K - 1, -1).T], dim=1)
        return (W * (torch.logsumexp(z, dim=1) - z[torch.arange(X.shape[0]), Y])).sum() + 0.5 * tau * (eta * eta).sum()
    return f


def _autograd(f, theta, v):
    t = torch.tensor(theta, requires_grad=True)
    val = f(t)
    g, = torch.autograd.grad(val, t, create_graph=True)
    hv, = torch.autograd.grad(g @ torch.as_tensor(v), t)
    return val.item(), g.detach().numpy(), hv.numpy()


@pytest.mark.parametrize('N', [1, 9, 2000])
@pytest.mark.parametrize('P', [1, 7, 33, 128, 129, 257, 1024])
@pytest.mark.parametrize('K', [2, 3, 5, 17])
def test_terms_against_autograd(vb, K, P, N):
    rng = np.random.default_rng(1000 * K + 10 * P + N)
    x, y, w, beta = _problem(rng, N, P, K)
    tau = 0.5
    par, fun, objective = _model(vb, x, y, w, K, tau)
    theta = beta.ravel()
    v = rng.normal(size=theta.size)
    val, g, hv = _autograd(_torch_f(x, y, w, K, tau), theta, v)
    assert abs(objective.fun_free(theta) - val) <= 1e-12 * abs(val)
    assert _rel(objective.fun_free_grad(theta), g) <= 1e-11
    assert _rel(objective.fun_free_hvp(theta, v), hv) <= 1e-11
    assert _rel(objective.fun_vector_hvp(theta, v), hv) <= 1e-11
    assert _rel(objective.fun_vector_grad(theta), g) <= 1e-11
    if theta.size <= 1100:
        H = sr.hessian(x, w, beta) + tau * np.eye(theta.size)
        assert _rel(objective.fun_free_hessian(theta), H) <= 1e-11
        assert _rel(objective.fun_vector_hessian(theta), H) <= 1e-11
        assert _rel(H @ v, hv) <= 1e-11


@pytest.mark.parametrize('K,P', [(3, 7), (5, 33)])
def test_box_bounded_free_coordinates_against_autograd(vb, K, P):
    rng = np.random.default_rng(K + P)
    N, lb, ub, tau = 500, -1.5, 2.5, 0.3
    x, y, w, _ = _problem(rng, N, P, K)
    par, fun, objective = _model(vb, x, y, w, K, tau, lb=lb, ub=ub)
    theta = rng.normal(size=(K - 1) * P) * 0.7
    v = rng.normal(size=theta.size)
    f = _torch_f(x, y, w, K, tau, lb, ub)
    val, g, hv = _autograd(f, theta, v)
    H = torch.autograd.functional.hessian(f, torch.tensor(theta)).numpy()
    assert abs(objective.fun_free(theta) - val) <= 1e-12 * abs(val)
    assert _rel(objective.fun_free_grad(theta), g) <= 1e-11
    assert _rel(objective.fun_free_hessian(theta), H) <= 1e-11
    assert _rel(objective.fun_free_hvp(theta, v), hv) <= 1e-11


@pytest.mark.parametrize('K,P', [(17, 66), (5, 130)])
def test_hessian_against_autograd_on_the_batched_syrk_path(vb, K, P):
    """Many blocks (136 at K = 17) on the LDS-DMA SYRK path (even P > 64), in batched launches, negative off-diagonal weight
    columns included: the free-coordinate Hessian against torch autograd."""
    rng = np.random.default_rng(K * P)
    N, tau = 300, 0.4
    x, y, w, beta = _problem(rng, N, P, K, scale=2.0)
    _, _, objective = _model(vb, x, y, w, K, tau)
    theta = beta.ravel()
    H = torch.autograd.functional.hessian(_torch_f(x, y, w, K, tau), torch.tensor(theta), vectorize=True).numpy()
    assert _rel(objective.fun_free_hessian(theta), H) <= 1e-11


def test_unaligned_design_takes_the_four_byte_staging(vb):
    """An even-P design whose base is not 16-byte aligned (an offset view handed over by pointer) is staged 4 bytes at a time:
    value, gradient, product, Hessian and influence rows against the reference."""
    rng = np.random.default_rng(61)
    N, P, K = 777, 130, 4
    x, y, w, beta = _problem(rng, N, P, K)
    D = (K - 1) * P
    store = torch.empty(N * P + 1, dtype=torch.float64, device='cuda:0')
    X = store[1:].view(N, P)
    X.copy_(torch.as_tensor(x))
    assert X.data_ptr() % 16 != 0
    ctx = vb.DeviceContext([dict(kind=vb._hip.BLOCK_BOX, free_size=D, vec_size=D, dim0=D, dim1=0, lb=-np.inf, ub=np.inf)],
                           loss='data_only', n_obs=N, n_cols=P)
    torch.cuda.synchronize()
    ctx.set_data_dev(vb._hip.SLOT_X, X.data_ptr(), N, P)
    ctx.set_weights(w)
    ctx.softmax_set_labels(y, K)
    b = beta.ravel()
    v = rng.normal(size=D)
    A = rng.normal(size=(3, D))
    val, g, H = ctx.softmax_terms(b, K)
    assert abs(val - sr.value(x, y, w, beta)) <= 1e-12 * abs(val)
    assert _rel(g, sr.grad(x, y, w, beta)) <= 1e-11
    assert _rel(H, sr.hessian(x, w, beta)) <= 1e-11
    assert _rel(ctx.softmax_hvp(b, K, v), sr.hvp(x, w, beta, v)) <= 1e-11
    rows = ctx.softmax_obs_influence(b, K, A, 5, 700)
    assert _rel(rows, (A @ sr.cross_hessian(x, y, beta))[:, 5:700].T) <= 1e-11
    ctx.close()


@pytest.mark.parametrize('P', [5, 64, 130])
def test_two_classes_is_the_logistic_glm(vb, P):
    rng = np.random.default_rng(P)
    N, tau = 3000, 0.8
    x, y, w, beta = _problem(rng, N, P, 2)
    _, _, soft = _model(vb, x, y, w, 2, tau)
    gpar = vb.ModelParamsDict('par')
    gpar.push_param(vb.VectorParam('beta', P))
    glm = vb.Objective(gpar, vb.GLMObjective(gpar, x, y.astype(np.float64), loss='logistic', prior_info=tau, weights=w))
    theta = beta.ravel()
    v = rng.normal(size=P)
    assert abs(soft.fun_free(theta) - glm.fun_free(theta)) <= 1e-12 * abs(glm.fun_free(theta))
    assert _rel(soft.fun_free_grad(theta), glm.fun_free_grad(theta)) <= 1e-12
    assert _rel(soft.fun_free_hessian(theta), glm.fun_free_hessian(theta)) <= 1e-12
    assert _rel(soft.fun_free_hvp(theta, v), glm.fun_free_hvp(theta, v)) <= 1e-12


@pytest.mark.parametrize('P', [3, 130])
def test_extreme_logits(vb, P):
    rng = np.random.default_rng(7)
    N, K = 400, 4
    x = rng.normal(size=(N, P))
    beta = rng.normal(size=(K - 1, P)) * 2e3 / np.sqrt(P)
    y = np.argmax(sr.logits(x, beta), axis=1)                 # separable: every row labelled by its largest logit
    y[::7] = (y[::7] + 1) % K                                  # ... but a few are not
    w = np.ones(N)
    assert np.abs(sr.logits(x, beta)).max() >= 1e3
    _, fun, objective = _model(vb, x, y, w, K, tau=0.0)
    theta = beta.ravel()
    v = rng.normal(size=theta.size)
    val = objective.fun_free(theta)
    g = objective.fun_free_grad(theta)
    H = objective.fun_free_hessian(theta)
    hv = objective.fun_free_hvp(theta, v)
    assert np.isfinite(val) and np.all(np.isfinite(g)) and np.all(np.isfinite(H)) and np.all(np.isfinite(hv))
    ref = sr.value(x, y, w, beta)
    assert abs(val - ref) <= 1e-12 * abs(ref)
    assert _rel(g, sr.grad(x, y, w, beta)) <= 1e-11
    Hr = sr.hessian(x, w, beta)
    assert np.max(np.abs(H - Hr)) <= 1e-11 * max(np.max(np.abs(Hr)), 1.0)
    assert np.max(np.abs(hv - Hr @ v)) <= 1e-11 * max(np.max(np.abs(Hr @ v)), 1.0)


def _fit(objective, D, x0=None):
    """trust-ncg on the matrix-free products, then Newton steps (H^-1 g by CG on the same products).  Near the optimum the
    value, a sum over N rows, resolves decreases only down to ~1e-16 of itself: trust-ncg's ratio test stalls there
    (|g| ~ 1e-7 at N = 4000), and the value-free Newton steps finish the job quadratically."""
    x = np.zeros(D) if x0 is None else x0
    x = scipy.optimize.minimize(objective.fun_free, x, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp,
                                method='trust-ncg', options={'gtol': 1e-9, 'maxiter': 200}).x
    fun = objective.fun
    for _ in range(4):
        g = objective.fun_free_grad(x)
        if np.max(np.abs(g)) <= 1e-10:
            break
        x = x - fun.cg_solve(x, g, tol=1e-12)[0]
    return x


def test_fit_trust_ncg_with_newton_polish_covariance_and_cg(vb):
    """The 1e-8 gradient is reached by trust-ncg followed by the Newton-CG polish of _fit (see there)."""
    rng = np.random.default_rng(21)
    K, P, N, tau = 5, 50, 4000, 1.0
    x = rng.normal(size=(N, P))
    btrue = rng.normal(size=(K - 1, P)) * 0.3
    p = np.hstack([1.0 - sr.probs(x, btrue).sum(axis=1, keepdims=True), sr.probs(x, btrue)])
    y = np.array([rng.choice(K, p=pi / pi.sum()) for pi in p])
    w = rng.uniform(0.5, 1.5, size=N)
    par, fun, objective = _model(vb, x, y, w, K, tau)
    D = (K - 1) * P
    opt = _fit(objective, D)
    assert np.max(np.abs(objective.fun_free_grad(opt))) <= 1e-8
    H = torch.autograd.functional.hessian(_torch_f(x, y, w, K, tau), torch.tensor(opt)).numpy()
    M = np.eye(D)[::17]
    cov = vb.ModelSensitivity.get_lrvb_cov(objective, opt, M)
    ref = M @ np.linalg.solve(H, M.T)
    assert _rel(cov, ref) <= 1e-8
    b = rng.normal(size=D)
    cg = vb.ConjugateGradientSolver(objective.fun_free_hvp, opt)
    cg.tol = 1e-12
    hinv_b, info = cg.get_hinv_vec(b)
    assert info == 0
    assert _rel(hinv_b, np.linalg.solve(H, b)) <= 1e-8


def test_weight_sensitivity(vb):
    rng = np.random.default_rng(33)
    K, P, N, tau = 3, 4, 600, 1.0
    x = rng.normal(size=(N, P))
    btrue = rng.normal(size=(K - 1, P)) * 0.5
    p = np.hstack([1.0 - sr.probs(x, btrue).sum(axis=1, keepdims=True), sr.probs(x, btrue)])
    y = np.array([rng.choice(K, p=pi / pi.sum()) for pi in p])
    w = np.ones(N)
    par, fun, objective = _model(vb, x, y, w, K, tau)
    D = (K - 1) * P
    opt = _fit(objective, D)
    sens = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, opt, w.copy(),
                                                       input_is_free=True, hyper_is_free=False)
    # torch: d theta / d w = -H^-1 d2 f / d theta d w
    f = _torch_f(x, y, w, K, tau)
    H = torch.autograd.functional.hessian(f, torch.tensor(opt)).numpy()

    def grad_w(wt):
        t = torch.tensor(opt, requires_grad=True)
        X, Y = torch.as_tensor(x), torch.as_tensor(y, dtype=torch.long)
        z = torch.cat([torch.zeros(N, 1, dtype=torch.float64), X @ t.reshape(K - 1, P).T], dim=1)
        fv = (wt * (torch.logsumexp(z, dim=1) - z[torch.arange(N), Y])).sum() + 0.5 * tau * (t * t).sum()
        return torch.autograd.grad(fv, t, create_graph=True)[0]
    C = torch.autograd.functional.jacobian(grad_w, torch.as_tensor(w)).numpy()
    ref = -np.linalg.solve(H, C)
    dense = sens.get_dinput_dhyper()
    assert _rel(dense, ref) <= 1e-9
    M = rng.normal(size=(3, D))
    rows = sens.get_doutput_dhyper_rows(M, 50, 450)
    assert rows.shape == (400, 3)
    assert _rel(rows, (M @ dense)[:, 50:450].T) <= 1e-10
    # perturb 1 % of the weights: the predicted refit is within second order of the actual refit
    w2 = w.copy()
    idx = rng.choice(N, N // 100, replace=False)
    w2[idx] = 0.0
    pred = sens.predict_input_par_from_hyperparameters(w2)
    fun.weights_par.set_vector(w2)
    actual = _fit(objective, D, opt)
    first = np.linalg.norm(actual - opt)
    assert first > 1e-3
    assert np.linalg.norm(pred - actual) <= 0.1 * first


def _full_size(vb, N, P, K, chunk):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(N + P + K)
    X = torch.randn(N, P, generator=g, device=dev, dtype=torch.float64) / P ** 0.5
    y = torch.randint(0, K, (N,), generator=g, device=dev)
    w = torch.rand(N, generator=g, device=dev, dtype=torch.float64) * 2.0
    beta = torch.randn(K - 1, P, generator=g, device=dev, dtype=torch.float64)
    D = (K - 1) * P
    ctx = vb.DeviceContext([dict(kind=vb._hip.BLOCK_BOX, free_size=D, vec_size=D, dim0=D, dim1=0, lb=-np.inf, ub=np.inf)],
                           loss='data_only', n_obs=N, n_cols=P)
    torch.cuda.synchronize()
    ctx.set_data_dev(vb._hip.SLOT_X, X.data_ptr(), N, P)
    ctx.set_weights(w.cpu().numpy())
    ctx.softmax_set_labels(y.cpu().numpy(), K)
    val, gd, Hd = ctx.softmax_terms(beta.cpu().numpy().ravel(), K)
    H = torch.zeros(D, D, device=dev, dtype=torch.float64)
    G = torch.zeros(K - 1, P, device=dev, dtype=torch.float64)
    for n0 in range(0, N, chunk):
        Xc = X[n0:n0 + chunk]
        z = torch.cat([torch.zeros(Xc.shape[0], 1, device=dev, dtype=torch.float64), Xc @ beta.T], dim=1)
        p = torch.softmax(z, dim=1)[:, 1:]
        e = torch.nn.functional.one_hot(y[n0:n0 + chunk], K)[:, 1:].to(torch.float64)
        wc = w[n0:n0 + chunk]
        G += (wc[:, None] * (p - e)).T @ Xc
        for a in range(K - 1):
            for b in range(a, K - 1):
                c = wc * p[:, a] * ((1.0 if a == b else 0.0) - p[:, b])
                H[a * P:(a + 1) * P, b * P:(b + 1) * P] += Xc.T @ (c[:, None] * Xc)
    for a in range(K - 1):
        for b in range(a + 1, K - 1):
            H[b * P:(b + 1) * P, a * P:(a + 1) * P] = H[a * P:(a + 1) * P, b * P:(b + 1) * P]
    Hr, Gr = H.cpu().numpy(), G.cpu().numpy().ravel()
    ctx.close()
    del X
    torch.cuda.empty_cache()
    return _rel(Hd, Hr), _rel(gd, Gr)


@pytest.mark.parametrize('N,P,K', [(1_000_000, 256, 10), (1_000_000, 1024, 4)])
def test_full_size_hessian_and_gradient(vb, N, P, K):
    eh, eg = _full_size(vb, N, P, K, 125_000)
    assert eh <= 1e-12 and eg <= 1e-12, (eh, eg)


def test_reduce_hook_contract(vb):
    rng = np.random.default_rng(41)
    K, P, N = 4, 9, 300
    x, y, w, beta = _problem(rng, N, P, K)
    _, fun, _ = _model(vb, x, y, w, K)
    ctx, b = fun.ctx, beta.ravel()
    D = b.size
    v = rng.normal(size=D)
    A = rng.normal(size=(5, D))
    base = (ctx.softmax_terms(b, K), ctx.softmax_terms(b, K, want_hess=False), ctx.softmax_hvp(b, K, v),
            ctx.softmax_obs_influence(b, K, A, 10, 200))
    sizes = []
    ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))
    out = [ctx.softmax_terms(b, K)]
    assert sizes == [D * D + D + 1]
    out.append(ctx.softmax_terms(b, K, want_hess=False))
    assert sizes[1:] == [D + 1]
    out.append(ctx.softmax_hvp(b, K, v))
    assert sizes[2:] == [D]
    out.append(ctx.softmax_obs_influence(b, K, A, 10, 200))
    assert sizes[3:] == []                          # per-row results: no sum over observations
    ctx.set_reduce_hook(None)
    for (v0, g0, H0), (v1, g1, H1) in zip(base[:2], out[:2]):
        assert v0 == v1 and np.array_equal(g0, g1) and (H0 is None or np.array_equal(H0, H1))
    assert np.array_equal(base[2], out[2]) and np.array_equal(base[3], out[3])


def test_abi_refusals(vb):
    rng = np.random.default_rng(43)
    N, P = 20, 3
    x = rng.normal(size=(N, P))
    blocks = [dict(kind=vb._hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
    ctx = vb.DeviceContext(blocks, loss='data_only', n_obs=N, n_cols=P)
    ctx.set_data(vb._hip.SLOT_X, x)
    lib, h = ctx._lib, ctx._h
    beta = np.zeros(2 * P)
    val = np.empty(1)
    bp = beta.ctypes.data
    assert lib.lrvb_softmax_terms(h, bp, 3, P, val.ctypes.data, None, None, 0) == vb._hip.ERR_STATE
    assert lib.lrvb_softmax_hvp(h, bp, 3, P, bp, np.empty(2 * P).ctypes.data) == vb._hip.ERR_STATE
    bad = np.zeros(N, dtype=np.int32)
    bad[4] = 3
    assert lib.lrvb_softmax_set_labels(h, bad.ctypes.data, N, 3) == vb._hip.ERR_INVALID
    bad[4] = -1
    assert lib.lrvb_softmax_set_labels(h, bad.ctypes.data, N, 3) == vb._hip.ERR_INVALID
    good = rng.integers(0, 3, size=N).astype(np.int32)
    assert lib.lrvb_softmax_set_labels(h, good.ctypes.data, N, 18) == vb._hip.ERR_UNSUPPORTED
    assert lib.lrvb_softmax_set_labels(h, good.ctypes.data, N, 3) == vb._hip.OK
    assert lib.lrvb_softmax_terms(h, bp, 18, P, val.ctypes.data, None, None, 0) == vb._hip.ERR_UNSUPPORTED
    assert lib.lrvb_softmax_terms(h, bp, 3, P, val.ctypes.data, None, None, 0) == vb._hip.OK
    ctx.close()
    wide = 1025
    blocks = [dict(kind=vb._hip.BLOCK_BOX, free_size=2 * wide, vec_size=2 * wide, dim0=2 * wide, dim1=0, lb=-np.inf, ub=np.inf)]
    ctx = vb.DeviceContext(blocks, loss='data_only', n_obs=4, n_cols=wide)
    ctx.set_data(vb._hip.SLOT_X, np.ones((4, wide)))
    lab = np.zeros(4, dtype=np.int32)
    assert ctx._lib.lrvb_softmax_set_labels(ctx._h, lab.ctypes.data, 4, 3) == vb._hip.ERR_UNSUPPORTED
    b2 = np.zeros(2 * wide)
    assert ctx._lib.lrvb_softmax_terms(ctx._h, b2.ctypes.data, 3, wide, val.ctypes.data, None, None, 0) == vb._hip.ERR_UNSUPPORTED
    ctx.close()

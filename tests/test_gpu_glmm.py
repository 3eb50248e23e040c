"""`LogisticGLMMObjective` (random-intercept logistic regression, arrow Hessian) on the GPU against the torch reference
tests/glmm_reference.py.  Tolerances are the project's for this kind of quantity (tests/test_gpu_logitnormal.py,
tests/test_gpu_lmm.py, BASELINE.json): value 1e-11, gradient 1e-10, Hessian and products 1e-9 relative; LRVB covariance rtol 1e-6."""
import time

import numpy as np
import pytest
import scipy.optimize
import torch

import glmm_reference as ref
from helpers import rel_err

pytestmark = pytest.mark.gpu

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _model(vb, x, y, w, gid, G, hyp=HYP, deg=20):
    P = x.shape[1]
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParam('mu'))
    par.push_param(vb.GammaParam('tau'))
    par.push_param(vb.UVNParamVector('u', length=G))
    fun = vb.LogisticGLMMObjective(par, x, y, gid, G, beta_prior_info=hyp[0], mu_prior=hyp[1:3], tau_prior=hyp[3:5], gh_deg=deg, weights=w)
    fun._push_state()                                    # the weights on the device before any direct call on fun.ctx
    return par, fun


def _targs(x, y, w, gid, G, hyp=HYP):
    t = ref.tensors(x, y, w, gid, hyp)
    return (t[0], t[1], t[2], t[3], G, t[4])


def _eta(free, P, G):
    mask = ref.positive_mask(P, G)
    return np.where(mask, np.exp(free), free)


def _schur(H, ng):
    return H[:ng, :ng] - H[:ng, ng:] @ np.linalg.solve(H[ng:, ng:], H[ng:, :ng])


@pytest.mark.parametrize('N,P,G', [(1, 1, 1), (37, 3, 5), (500, 8, 40), (1999, 17, 3), (4096, 64, 300), (20011, 30, 1000)])
def test_value_grad_hessian_products_and_schur(vb, N, P, G):
    x, y, w, gid, free = ref.problem(N, P, G, seed=N + P)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2      # an empty group, one with more than half the rows
    par, fun = _model(vb, x, y, w, gid, G)
    targs = _targs(x, y, w, gid, G)
    ng = 2 * P + 4
    eta = _eta(free, P, G)
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    e = [abs(fun.value(eta, False) - val) / abs(val), rel_err(fun.grad(eta, False), g), rel_err(fun.hessian(eta, False), H)]
    print('vector', N, P, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    assert np.allclose(par['u']['mean'].get(), eta[ng:ng + G])           # the side-effect contract: par holds the evaluation point
    valf, gf, Hf = ref.value_grad_hess(ref.kl_free, free, targs)
    Hd = fun.hessian(free, True)
    e = [abs(fun.value(free, True) - valf) / abs(valf), rel_err(fun.grad(free, True), gf), rel_err(Hd, Hf)]
    print('free', N, P, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    assert np.allclose(par['beta']['mean'].get(), free[:P])
    # products, Schur complement, LRVB covariance, sparse export
    objective = vb.Objective(par, fun)
    rng = np.random.default_rng(3)
    v = rng.normal(size=free.size)
    assert rel_err(objective.fun_free_hvp(free, v), Hf @ v) < 1e-9
    HS = fun.global_hessian(free)
    e_s = rel_err(HS, _schur(Hf, ng))
    print('schur', e_s)
    assert e_s < 1e-9
    gc = fun._ensure_gctx()
    fun.global_hessian(free, want_host=False)
    gc.chol_factor_last()
    M = np.eye(ng)[:P]
    cov = gc.lrvb_cov(M)
    assert np.allclose(cov, np.linalg.inv(Hf)[:P, :P], rtol=1e-6, atol=0)
    assert rel_err(fun.sparse_hessian(free).toarray(), Hd) < 1e-14


def test_terms_are_bitwise_reproducible_and_order_independent(vb):
    N, P, G = 3001, 7, 23
    x, y, w, gid, free = ref.problem(N, P, G, seed=5)
    eta = _eta(free, P, G)
    ng = 2 * P + 4
    par, fun = _model(vb, x, y, w, gid, G)
    gx, gw = fun.gh_x, fun.gh_w
    pt = (eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:], gx, gw)
    a, b = fun.ctx.glmm_terms(*pt), fun.ctx.glmm_terms(*pt)
    assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    # another row order: the same sums, to rounding
    perm = np.random.default_rng(6).permutation(N)
    _, fun2 = _model(vb, x[perm], y[perm], w[perm], gid[perm], G)
    c = fun2.ctx.glmm_terms(*pt)
    assert abs(c[0] - a[0]) < 1e-11 * abs(a[0])
    assert rel_err(c[1], a[1]) < 1e-10 and rel_err(c[2], a[2]) < 1e-10
    assert all(rel_err(p, q) < 1e-9 for p, q in zip(c[3:], a[3:]))
    # a zero weight equals deleting the row
    w0 = w.copy()
    drop = np.array([0, 17, N - 1])
    w0[drop] = 0.0
    keep = np.setdiff1d(np.arange(N), drop)
    _, fun3 = _model(vb, x, y, w0, gid, G)
    _, fun4 = _model(vb, x[keep], y[keep], w[keep], gid[keep], G)
    c, d = fun3.ctx.glmm_terms(*pt), fun4.ctx.glmm_terms(*pt)
    assert abs(c[0] - d[0]) < 1e-11 * abs(d[0])
    assert rel_err(c[1], d[1]) < 1e-10 and rel_err(c[2], d[2]) < 1e-10
    assert all(rel_err(p, q) < 1e-9 for p, q in zip(c[3:], d[3:]))


def _fit(objective, theta0):
    opt = scipy.optimize.minimize(objective.fun_free, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp, x0=theta0,
                                  method='trust-ncg', options={'gtol': 1e-7, 'maxiter': 200})
    th = opt.x
    for _ in range(8):                                   # Newton polish where the ratio test stalls at the rounding of f
        g = objective.fun_free_grad(th)
        if np.max(np.abs(g)) < 1e-8:
            break
        th = th - np.linalg.solve(objective.fun_free_hessian(th), g)
    return th


def test_fit_lrvb_and_sensitivities(vb):
    N, P, G = 3000, 4, 30
    x, y, w, gid, free0 = ref.problem(N, P, G, seed=77, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, w, gid, G)
    ng = 2 * P + 4
    objective = vb.Objective(par, fun)
    th = _fit(objective, np.zeros(free0.size))
    assert np.max(np.abs(objective.fun_free_grad(th))) < 1e-6
    targs = _targs(x, y, w, gid, G)
    _, _, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    H = objective.fun_free_hessian(th)
    assert rel_err(H, H_ad) < 1e-9
    assert np.min(np.linalg.eigvalsh(0.5 * (H + H.T))) > 0
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    cov = gc.lrvb_cov(np.eye(ng)[:P])
    Hinv = np.linalg.inv(H_ad)
    assert np.allclose(cov, Hinv[:P, :P], rtol=1e-6, atol=0)
    par.set_free(th)
    assert np.all(np.diag(cov) > 1.0 / par['beta']['info'].get())
    # prior sensitivity of the global parameters against -H^-1 C by AD of the reference
    tt = torch.tensor(th)

    def cross_ad(index):
        hyp = torch.tensor(np.asarray(HYP), requires_grad=True)
        p = tt.clone().requires_grad_(True)
        g, = torch.autograd.grad(ref.kl_free(p, targs[0], targs[1], targs[2], targs[3], G, hyp), p, create_graph=True)
        rows = [torch.autograd.grad(g[k], hyp, retain_graph=True)[0].numpy() for k in range(g.numel())]
        return np.stack(rows)[:, index]
    for hp, index in ((fun.tau_prior_par, [3, 4]), (fun.mu_prior_par, [1, 2]), (fun.beta_prior_info_par, [0])):
        C = cross_ad(index)
        assert np.all(C[ng:] == 0.0)                                      # prior rows of the local block are zero
        assert rel_err(fun.cross_hessian(hp, th, True), C) < 1e-9
        sens = fun.global_sensitivity(hp, th)
        assert np.allclose(sens, -(Hinv @ C)[:ng], rtol=1e-6, atol=1e-12)
    # weight cross Hessian against AD (its local rows are not zero)
    wt = targs[2].clone().requires_grad_(True)
    p = tt.clone().requires_grad_(True)
    g, = torch.autograd.grad(ref.kl_free(p, targs[0], targs[1], wt, targs[3], G, targs[5]), p, create_graph=True)
    Cw = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())])
    two = vb.TwoParameterObjective(par, fun.weights_par, fun)
    Cw_dev = two.fun_hessian_free1_vector2(th, w)
    assert rel_err(Cw_dev, Cw) < 1e-9
    assert np.max(np.abs(Cw[ng:])) > 0
    # leaving one observation out: linear prediction against the refit
    sens = -np.linalg.solve(H, Cw_dev)
    w2 = w.copy(); w2[11] = 0.0
    fun.weights_par.set_vector(w2)
    th2 = _fit(objective, th)
    pred = th + sens @ (w2 - w)
    assert np.max(np.abs(pred - th2)) < 0.05 * np.max(np.abs(th2 - th)) + 1e-8


def test_reduce_hook_contract_and_shards(vb):
    N, P, G = 2001, 6, 11
    x, y, w, gid, free = ref.problem(N, P, G, seed=9)
    order = np.argsort(gid, kind='stable')                               # sorted rows: the cut below goes through group 0
    x, y, w, gid = x[order], y[order], w[order], gid[order]
    eta = _eta(free, P, G)
    ng = 2 * P + 4
    _, full = _model(vb, x, y, w, gid, G)
    pt = (eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:], full.gh_x, full.gh_w)
    ctx = full.ctx
    base = (ctx.glmm_terms(*pt), ctx.glmm_terms(*pt, want_hess=False))
    sizes = []
    ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))
    out = [ctx.glmm_terms(*pt)]
    assert sizes == [3 * P * P + G * (5 + 4 * P) + 2 * P + 1]
    out.append(ctx.glmm_terms(*pt, want_hess=False))
    assert sizes[1:] == [G * (5 + 4 * P) + 2 * P + 1]
    ctx.set_reduce_hook(None)
    for p, q in zip(base, out):
        assert p[0] == q[0] and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(p[1:], q[1:]))
    # two half-shards, a group straddling the cut
    n1 = 700
    assert gid[n1 - 1] == gid[n1]
    _, f1 = _model(vb, x[:n1], y[:n1], w[:n1], gid[:n1], G)
    _, f2 = _model(vb, x[n1:], y[n1:], w[n1:], gid[n1:], G)
    s_sum = f1.local_stats(eta) + f2.local_stats(eta)
    assert rel_err(s_sum, full.local_stats(eta)) < 1e-11
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, _targs(x, y, w, gid, G))
    f1.set_reduced_stats(s_sum, eta)
    assert abs(f1.value(eta, False) - val) < 1e-11 * abs(val)
    assert rel_err(f1.grad(eta, False), g) < 1e-10 and rel_err(f1.hessian(eta, False), H) < 1e-9
    _, _, Hf = ref.value_grad_hess(ref.kl_free, free, _targs(x, y, w, gid, G))
    f1.set_reduced_stats(s_sum, eta)
    assert rel_err(f1.global_hessian(free), _schur(Hf, ng)) < 1e-9
    with pytest.raises(ValueError):
        f1.value(eta * 1.01, False)
    f1.set_reduced_stats(None)
    assert abs(f1.value(eta, False) - val) > 1e-3 * abs(val)


def test_refusals_by_error_code(vb):
    hip = vb._hip
    rng = np.random.default_rng(43)

    def context(N, P, with_y=True):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)))
        if with_y:
            ctx.set_data(hip.SLOT_Y, (rng.uniform(size=N) < 0.5).astype(np.float64))
        return ctx

    def call(ctx, P, G, var=None, r=None, nodes=20):
        m = np.zeros(P)
        v = np.ones(P) if var is None else var
        e = np.zeros(G)
        rr = np.ones(G) if r is None else r
        gx, gw = np.zeros(max(nodes, 1)), np.ones(max(nodes, 1))
        val = np.empty(1)
        return ctx._lib.lrvb_glmm_terms(ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, gx.ctypes.data,
                                        gw.ctypes.data, nodes, val.ctypes.data, None, None, None, None, None)
    N, G = 20, 3
    gid = np.arange(N) % G
    wide = context(N, 65)
    assert call(wide, 65, G) == hip.ERR_UNSUPPORTED                       # P > 64
    ctx = context(N, 3)
    assert call(ctx, 3, G) == hip.ERR_STATE                               # no groups
    noy = context(N, 3, with_y=False)
    noy.set_groups(gid, G)
    assert call(noy, 3, G) == hip.ERR_STATE                               # no responses
    ctx.set_groups(gid, G)
    loc, sc, cl, M = np.ones((G, 3)), np.ones((G, 2)), np.zeros((G, 6)), np.empty((9, 9))
    schur = lambda: ctx._lib.lrvb_glmm_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, M.ctypes.data)
    assert schur() == hip.ERR_STATE                                       # no group sums resident
    assert call(ctx, 3, G, var=np.array([1.0, 0.0, 1.0])) == hip.ERR_INVALID
    assert call(ctx, 3, G, r=np.array([1.0, 1.0, -1.0])) == hip.ERR_INVALID
    assert call(ctx, 3, G, nodes=129) == hip.ERR_UNSUPPORTED
    assert call(ctx, 3, G) == hip.OK
    assert schur() == hip.ERR_NOT_POSDEF                                  # [1 1; 1 1] is singular
    loc[:, 2] = 2.0
    assert schur() == hip.OK


def test_full_size_arrow(vb):
    """N = 1e6, P = 64, G = 1e4: finite, the arrow product consistent with the Schur complement
    (H_S x_g = global part of H [x_g; -H_ll^-1 H_lg x_g]) to 1e-9, and H_S factors."""
    from lrvb_amd import glmm
    N, P, G = 1000000, 64, 10000
    rng = np.random.default_rng(1)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    u = rng.normal(size=G) * 0.7
    beta = rng.normal(size=P) * 0.8
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + u[gid])))).astype(np.float64)
    free = np.concatenate([beta, np.full(P, 6.0), [0.0, 3.0], [np.log(G / 2.0), np.log(G / 4.0)], u, np.full(G, 3.0)])
    par, fun = _model(vb, x, y, None, gid, G)
    ng = 2 * P + 4
    t0 = time.perf_counter()
    HS = fun.global_hessian(free)
    t1 = time.perf_counter()
    assert np.all(np.isfinite(HS))
    fun._ensure_gctx().chol_factor_last()
    xg = rng.normal(size=ng)
    lo = fun.hvp(free, np.concatenate([xg, np.zeros(2 * G)]), True)[ng:]
    t2 = time.perf_counter()
    loc = fun._pieces[4]
    se, si = glmm.arrow_local_solve(loc, lo[:G], lo[G:])
    out = fun.hvp(free, np.concatenate([xg, -se, -si]), True)
    t3 = time.perf_counter()
    print('global_hessian %.3f s, first hvp (arrow build) %.3f s, cached hvp %.4f s' % (t1 - t0, t2 - t1, t3 - t2))
    assert np.all(np.isfinite(out))
    assert rel_err(out[:ng], HS @ xg) < 1e-9
    assert np.max(np.abs(out[ng:])) < 1e-9 * np.max(np.abs(lo))

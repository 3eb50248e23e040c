"""Streamed weight influence of `PoissonGLMMObjective`: the row entry `lrvb_glmm_poisson_obs_influence`, the
group entry `lrvb_glmm_poisson_group_influence` and the routes behind `obs_influence` / `group_influence`, against torch autograd
of tests/glmm_poisson_reference.py.  Tolerances are those of tests/test_gpu_glmm_slopes_influence.py for the same quantities:
influence rows 1e-9 relative, group sums against the weighted sums of the rows 1e-10, quantities behind an H^-1 rtol 1e-6 with
atol 1e-12."""
import numpy as np
import pytest
import torch

import glmm_poisson_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _eta, _point, _fit
from test_gpu_glmm_poisson import SHAPES, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def rows_autograd(x, y, z, w, o, gid, G, eta, A):
    """N x Q: column q is the derivative with respect to the weights of A[q] . (gradient of the reference in (m, v, e, r))."""
    P, K = x.shape[1], z.shape[1]
    ng, GK = 2 * P + 4 * K, G * K
    t = ref.tensors(x, y, z, w, o, gid, HYP)
    c = torch.tensor(np.concatenate([eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + GK], 1.0 / eta[ng + GK:]]), requires_grad=True)
    wt = t[3].clone().requires_grad_(True)
    et = torch.cat([c[:P], 1.0 / c[P:2 * P], torch.tensor(eta[2 * P:ng]), c[2 * P:2 * P + GK], 1.0 / c[2 * P + GK:]])
    g, = torch.autograd.grad(ref.kl_vec(et, t[0], t[1], t[2], wt, t[4], t[5], G, t[6]), c, create_graph=True)
    return np.stack([torch.autograd.grad(g @ torch.tensor(A[q]), wt, retain_graph=True)[0].numpy() for q in range(A.shape[0])], axis=1)


def _segment_sum(gid, G, v):
    out = np.zeros((G,) + v.shape[1:])
    np.add.at(out, gid, v)
    return out


@pytest.mark.parametrize('N,P,K,G', [SHAPES[0]] + SHAPES[3:])
def test_rows_against_autograd_and_windows(vb, N, P, K, G):
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=N + P + K)
    par, fun = _model(vb, x, y, z, w, o, gid, G)
    eta = _eta(free, P, K, G)
    pt = _point(eta, P, K, G)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want = rows_autograd(x, y, z, w, o, gid, G, eta, A)
    for Q in (1, 5, 16, 21):                                             # 21 crosses the 16-column MFMA block
        got = fun.ctx.glmm_poisson_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        for n0, n1 in ((5, 700), (N // 3, N // 3 + 1), (63, 129), (N, N), (0, 0)):      # windows no tile boundary aligns with
            n0, n1 = min(n0, N), min(n1, N)
            win = fun.ctx.glmm_poisson_obs_influence(*pt, A[:Q], n0=n0, n1=n1)
            assert win.shape == (n1 - n0, Q) and np.array_equal(win, got[n0:n1])


def test_rows_do_not_depend_on_the_weights(vb):
    N, P, K, G = 3001, 7, 3, 23
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=5)
    eta = _eta(free, P, K, G)
    pt = _point(eta, P, K, G)
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G * K))
    _, f1 = _model(vb, x, y, z, np.ones(N), o, gid, G)
    w0 = w.copy()
    zero = np.array([0, 17, 64, 1500, N - 1])
    w0[zero] = 0.0
    _, f0 = _model(vb, x, y, z, w0, o, gid, G)
    a = f1.ctx.glmm_poisson_obs_influence(*pt, A)
    b = f0.ctx.glmm_poisson_obs_influence(*pt, A)
    assert np.all(np.abs(a[zero]) > 0)
    assert np.array_equal(a, b)                                           # a left-out row still gets the influence of adding it


@pytest.mark.parametrize('N,P,K,G,Q', [(3001, 7, 3, 23, 5), (4096, 64, 4, 150, 16), (1, 1, 1, 1, 1), (130, 64, 4, 2, 21)])
def test_group_sums(vb, N, P, K, G, Q):
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=N + P + K)
    eta = _eta(free, P, K, G)
    A = np.random.default_rng(7).normal(size=(Q, 2 * P + 2 * G * K))
    _, fun = _model(vb, x, y, z, w, o, gid, G)
    pt = _point(eta, P, K, G)
    rows = fun.ctx.glmm_poisson_obs_influence(*pt, A)
    want = _segment_sum(gid, G, w[:, None] * rows)
    a, b = fun.ctx.glmm_poisson_group_influence(*pt, A), fun.ctx.glmm_poisson_group_influence(*pt, A)
    e = rel_err(a, want)
    print('group sums', N, P, K, G, Q, e)
    assert a.shape == (G, Q) and e < 1e-10
    assert np.array_equal(a, b)                                           # bitwise reproducible
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)      # the empty group


@pytest.fixture(scope='module')
def fitted(vb):
    """N = 3000, P = 5, K = 2, G = 25 at its optimum (unit weights), with the dense Hessian and the weight cross Hessian of the
    reference by torch autograd."""
    N, P, K, G = 3000, 5, 2, 25
    x, y, z, w, gid, o, free0 = ref.problem(N, P, K, G, seed=78, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, o, gid, G)
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = ref.targs(x, y, z, w, o, gid, G, HYP)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    assert np.max(np.abs(g_ad)) < 1e-6                                   # stationary by the REFERENCE gradient
    assert np.min(np.linalg.eigvalsh(H_ad)) > 0                          # ... whose Hessian is positive definite there
    wt = targs[3].clone().requires_grad_(True)
    p = torch.tensor(th).requires_grad_(True)
    g, = torch.autograd.grad(ref.kl_free(p, targs[0], targs[1], targs[2], wt, targs[4], targs[5], G, targs[7]), p, create_graph=True)
    Cw = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())])
    return dict(N=N, P=P, K=K, G=G, x=x, y=y, z=z, o=o, gid=gid, w=w, par=par, fun=fun, objective=objective, th=th, H_ad=H_ad, Cw=Cw)


def test_routes_at_a_fitted_point(vb, fitted):
    f = fitted
    fun, par, th, P, K, G = f['fun'], f['par'], f['th'], f['P'], f['K'], f['G']
    ng = 2 * P + 4 * K
    D = ng + 2 * G * K
    want = -np.linalg.solve(f['H_ad'], f['Cw']).T                        # N x D
    rows = fun.obs_influence(th, np.eye(D))
    print('arrow route', rel_err(rows, want))
    assert np.allclose(rows, want, rtol=1e-6, atol=1e-12)
    # the device route: the block-arrow solve on the factors resident on the device
    rows_dev = fun.obs_influence(th, np.eye(D), on_device=True)
    assert np.allclose(rows_dev, rows, rtol=1e-6, atol=1e-12)
    gi = fun.group_influence(th, np.eye(D))
    assert np.allclose(fun.group_influence(th, np.eye(D), on_device=True), gi, rtol=1e-6, atol=1e-12)
    assert np.allclose(gi, _segment_sum(f['gid'], G, f['w'][:, None] * rows), rtol=1e-6, atol=1e-12)
    # streamed rows through the sensitivity class (dense factor route)
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, th, f['w'], stream_hyper=True)
    dense = lin.get_doutput_dhyper_rows(np.eye(D))
    print('dense factor route against the arrow route', rel_err(dense, rows))
    assert np.allclose(dense, rows, rtol=1e-6, atol=1e-12)
    win = lin.get_doutput_dhyper_rows(np.eye(D)[:3], n0=100, n1=333)
    assert np.allclose(win, rows[100:333, :3], rtol=1e-6, atol=1e-12)
    # the dense weight cross Hessian (small-N protocol) takes psi from the Poisson likelihood, offset included
    C = fun.cross_hessian(fun.weights_par, th, True)
    assert C.shape == (D, f['N']) and rel_err(C, f['Cw']) < 1e-9


def test_leave_one_group_out(vb, fitted):
    """The criterion of tests/test_gpu_glmm_slopes_influence.py::test_leave_one_group_out: the streamed prediction
    theta - group_influence[g] lands as close to the refit without group g as the dense torch-AD prediction does."""
    f = fitted
    fun, th, P, K, G, gid, w = f['fun'], f['th'], f['P'], f['K'], f['G'], f['gid'], f['w']
    D = 2 * P + 4 * K + 2 * G * K
    gi = fun.group_influence(th, np.eye(D))
    assert gi.shape == (G, D)
    g = int(np.argmax(np.max(np.abs(gi), axis=1)))
    w2 = w.copy()
    w2[gid == g] = 0.0
    pred = th - gi[g]                                                    # the multiplier on the group's weights goes from 1 to 0
    pred_ad = th - np.linalg.solve(f['H_ad'], f['Cw']) @ (w2 - w)
    fun.weights_par.set_vector(w2)
    try:
        th2 = _fit(vb, f['objective'], th)
    finally:
        fun.weights_par.set_vector(w)
    d, d_ad, step = np.max(np.abs(pred - th2)), np.max(np.abs(pred_ad - th2)), np.max(np.abs(th2 - th))
    print('leave group {} out: |pred - refit| {:.3e}, AD prediction {:.3e}, |refit - theta| {:.3e}'.format(g, d, d_ad, step))
    assert step > 0
    assert d <= d_ad + 1e-6 * step

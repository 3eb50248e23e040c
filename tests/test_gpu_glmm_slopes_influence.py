"""Streamed weight influence of `LogisticGLMMSlopesObjective`: the row entry
`lrvb_glmm_slopes_obs_influence`, the group entry `lrvb_glmm_slopes_group_influence`, `weights_par` and the routes behind
`obs_influence` / `group_influence`, against torch autograd of tests/glmm_slopes_reference.py.  Tolerances are those of
tests/test_gpu_glmm_influence.py for the same quantities: influence rows 1e-9 relative, sums in another order 1e-10 / 1e-9,
quantities behind an H^-1 rtol 1e-6 with atol 1e-12, agreement of the two classes at K = 1 1e-12."""
import time

import numpy as np
import pytest
import torch

import glmm_reference as ref1
import glmm_slopes_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, SHAPES, _model, _targs, _eta, _point, _fit
from test_glmm_slopes_influence_host_math import rows_autograd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _pt(fun, eta, P, K, G):
    return _point(eta, P, K, G) + (fun.gh_x, fun.gh_w)


def _segment_sum(gid, G, v):
    out = np.zeros((G,) + v.shape[1:])
    np.add.at(out, gid, v)
    return out


@pytest.mark.parametrize('N,P,K,G,seed', SHAPES)
def test_rows_against_autograd_and_windows(vb, N, P, K, G, seed):
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=seed)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2      # an empty group, one with more than half the rows
    par, fun = _model(vb, x, y, z, w, gid, G)
    eta = _eta(free, P, K, G)
    pt = _pt(fun, eta, P, K, G)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want = rows_autograd(x, y, z, w, gid, G, eta, A)
    for Q in (1, 5, 16, 21):
        got = fun.ctx.glmm_slopes_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        for n0, n1 in ((5, 700), (N // 3, N // 3 + 1), (63, 129), (N, N), (0, 0)):
            n0, n1 = min(n0, N), min(n1, N)
            win = fun.ctx.glmm_slopes_obs_influence(*pt, A[:Q], n0=n0, n1=n1)
            assert win.shape == (n1 - n0, Q) and np.array_equal(win, got[n0:n1])


def test_rows_do_not_depend_on_the_weights(vb):
    N, P, K, G = 3001, 7, 3, 23
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=5)
    eta = _eta(free, P, K, G)
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G * K))
    _, f1 = _model(vb, x, y, z, np.ones(N), gid, G)
    w0 = w.copy()
    zero = np.array([0, 17, 64, 1500, N - 1])
    w0[zero] = 0.0
    _, f0 = _model(vb, x, y, z, w0, gid, G)
    a = f1.ctx.glmm_slopes_obs_influence(*_pt(f1, eta, P, K, G), A)
    b = f0.ctx.glmm_slopes_obs_influence(*_pt(f0, eta, P, K, G), A)
    assert np.all(np.abs(a[zero]) > 0)
    assert np.array_equal(a, b)                                           # a left-out row still gets the influence of adding it


@pytest.mark.parametrize('N,P,K,G,Q', [(3001, 7, 3, 23, 5), (4096, 64, 4, 150, 16), (1, 1, 1, 1, 1), (130, 64, 4, 2, 21)])
def test_group_sums(vb, N, P, K, G, Q):
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=N + P + K)
    eta = _eta(free, P, K, G)
    A = np.random.default_rng(7).normal(size=(Q, 2 * P + 2 * G * K))
    _, fun = _model(vb, x, y, z, w, gid, G)
    pt = _pt(fun, eta, P, K, G)
    rows = fun.ctx.glmm_slopes_obs_influence(*pt, A)
    want = _segment_sum(gid, G, w[:, None] * rows)
    a, b = fun.ctx.glmm_slopes_group_influence(*pt, A), fun.ctx.glmm_slopes_group_influence(*pt, A)
    e = rel_err(a, want)
    print('group sums', N, P, K, G, Q, e)
    assert a.shape == (G, Q) and e < 1e-10
    assert np.array_equal(a, b)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)      # the empty group
    perm = np.random.default_rng(6).permutation(N)
    _, fun2 = _model(vb, x[perm], y[perm], z[perm], w[perm], gid[perm], G)
    assert rel_err(fun2.ctx.glmm_slopes_group_influence(*pt, A), a) < 1e-9


@pytest.mark.parametrize('N,P,G', [(37, 3, 5), (2500, 9, 30)])
def test_one_effect_with_unit_design_equals_the_intercept_class(vb, N, P, G):
    x, y, w, gid, free = ref1.problem(N, P, G, seed=N + P)
    par1 = vb.ModelParamsDict('params')
    par1.push_param(vb.UVNParamVector('beta', length=P))
    par1.push_param(vb.UVNParam('mu'))
    par1.push_param(vb.GammaParam('tau'))
    par1.push_param(vb.UVNParamVector('u', length=G))
    old = vb.LogisticGLMMObjective(par1, x, y, gid, G, beta_prior_info=HYP[0], mu_prior=HYP[1:3], tau_prior=HYP[3:5], weights=w)
    old._push_state()                                                    # the weights on the device before a direct call on old.ctx
    _, new = _model(vb, x, y, np.ones((N, 1)), w, gid, G)
    eta = _eta(free, P, 1, G)
    ng = 2 * P + 4
    A = np.random.default_rng(3).normal(size=(21, 2 * P + 2 * G))
    pt1 = (eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:], old.gh_x, old.gh_w)
    ptk = _pt(new, eta, P, 1, G)
    assert rel_err(new.ctx.glmm_slopes_obs_influence(*ptk, A), old.ctx.glmm_obs_influence(*pt1, A)) < 1e-12
    assert rel_err(new.ctx.glmm_slopes_obs_influence(*ptk, A[:3], n0=11, n1=30), old.ctx.glmm_obs_influence(*pt1, A[:3], n0=11, n1=30)) < 1e-12
    assert rel_err(new.ctx.glmm_slopes_group_influence(*ptk, A), old.ctx.glmm_group_influence(*pt1, A)) < 1e-12


def test_reduce_hook_contract_and_shards(vb):
    N, P, K, G, Q = 2001, 6, 2, 11, 5
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=9)
    order = np.argsort(gid, kind='stable')                               # sorted rows: the cut below goes through group 0
    x, y, z, w, gid = x[order], y[order], z[order], w[order], gid[order]
    eta = _eta(free, P, K, G)
    A = np.random.default_rng(8).normal(size=(Q, 2 * P + 2 * G * K))
    _, full = _model(vb, x, y, z, w, gid, G)
    pt = _pt(full, eta, P, K, G)
    ctx = full.ctx
    base_g, base_r = ctx.glmm_slopes_group_influence(*pt, A), ctx.glmm_slopes_obs_influence(*pt, A)
    sizes = []
    ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))
    rows = ctx.glmm_slopes_obs_influence(*pt, A)
    assert sizes == []                                                   # per-observation rows stay rank-local
    grp = ctx.glmm_slopes_group_influence(*pt, A)
    assert sizes == [G * Q]
    ctx.set_reduce_hook(None)
    assert np.array_equal(rows, base_r) and np.array_equal(grp, base_g)
    n1 = 700
    assert gid[n1 - 1] == gid[n1]                                        # a group straddling the cut
    _, f1 = _model(vb, x[:n1], y[:n1], z[:n1], w[:n1], gid[:n1], G)
    _, f2 = _model(vb, x[n1:], y[n1:], z[n1:], w[n1:], gid[n1:], G)
    s = f1.ctx.glmm_slopes_group_influence(*pt, A) + f2.ctx.glmm_slopes_group_influence(*pt, A)
    assert rel_err(s, base_g) < 1e-10
    assert np.array_equal(np.vstack([f1.ctx.glmm_slopes_obs_influence(*pt, A), f2.ctx.glmm_slopes_obs_influence(*pt, A)]), base_r)


@pytest.fixture(scope='module')
def fitted(vb):
    """The N = 4000, P = 6, K = 2, G = 60 problem of tests/test_gpu_glmm_slopes.py::test_fit_covariance_and_tau_prior_sensitivity at
    its optimum (unit weights), with the dense Hessian and the weight cross Hessian of the reference by torch autograd."""
    N, P, K, G = 4000, 6, 2, 60
    x, y, z, w, gid, free0 = ref.problem(N, P, K, G, seed=77, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, gid, G)
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = _targs(x, y, z, w, gid, G)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    assert np.max(np.abs(g_ad)) < 1e-6                                   # stationary by the REFERENCE gradient
    assert np.min(np.linalg.eigvalsh(H_ad)) > 0                          # ... whose Hessian is positive definite there
    wt = targs[3].clone().requires_grad_(True)
    p = torch.tensor(th).requires_grad_(True)
    g, = torch.autograd.grad(ref.kl_free(p, targs[0], targs[1], targs[2], wt, targs[4], G, targs[6]), p, create_graph=True)
    Cw = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())])
    return dict(N=N, P=P, K=K, G=G, x=x, y=y, z=z, gid=gid, w=w, par=par, fun=fun, objective=objective, th=th, H_ad=H_ad, Cw=Cw)


def test_end_to_end_at_a_fitted_point(vb, fitted):
    f = fitted
    fun, par, th, P, K, G = f['fun'], f['par'], f['th'], f['P'], f['K'], f['G']
    ng = 2 * P + 4 * K
    D = ng + 2 * G * K
    want = -np.linalg.solve(f['H_ad'], f['Cw']).T                        # N x D
    rows = fun.obs_influence(th, np.eye(D))
    print('arrow route', rel_err(rows, want), np.max(np.abs((rows - want) / np.where(want == 0, 1, want))))
    assert np.allclose(rows, want, rtol=1e-6, atol=1e-12)
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, th, f['w'], stream_hyper=True)
    dense = lin.get_doutput_dhyper_rows(np.eye(D))
    print('dense factor route against the arrow route', rel_err(dense, rows))
    assert np.allclose(dense, rows, rtol=1e-6, atol=1e-12)
    win = lin.get_doutput_dhyper_rows(np.eye(D)[:3], n0=100, n1=333)
    assert np.allclose(win, rows[100:333, :3], rtol=1e-6, atol=1e-12)
    # a Q x n_global moment Jacobian is zero-padded
    assert np.array_equal(fun.obs_influence(th, np.eye(ng)[:2], n0=7, n1=90), fun.obs_influence(th, np.eye(D)[:2], n0=7, n1=90))
    # the dense weight cross Hessian (small-N protocol)
    C = fun.cross_hessian(fun.weights_par, th, True)
    e = rel_err(C, f['Cw'])
    print('cross Hessian', e)
    assert C.shape == (D, f['N']) and e < 1e-9
    with pytest.raises(NotImplementedError):
        fun.hyper_grad(fun.weights_par, th, True)
    with pytest.raises(NotImplementedError):
        fun.global_cross_hessian(fun.weights_par, th)


def test_leave_one_group_out(vb, fitted):
    """The streamed prediction theta - group_influence[g] lands as close to the refit without group g as the dense torch-AD
    prediction does (a test of the kernel, not of the quality of the linear approximation)."""
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


def test_changed_weights_reach_the_device_and_invalidate_the_factor(vb, fitted):
    f = fitted
    fun, th, G = f['fun'], f['th'], f['G']
    R = np.random.default_rng(4).normal(size=(th.size, 2))
    fun.global_hessian(th, want_host=False)
    fun._ensure_gctx().chol_factor_last()
    base = fun.solve(th, R, resident_factor=True)
    assert np.allclose(base, np.linalg.solve(f['H_ad'], R), rtol=1e-6, atol=1e-12)
    w2 = np.random.default_rng(5).uniform(0.5, 1.5, size=f['N'])
    fun.weights_par.set_vector(w2)
    try:
        val, g_ad, _ = ref.value_grad_hess(ref.kl_free, th, _targs(f['x'], f['y'], f['z'], w2, f['gid'], G), want_hess=False)
        e_v, e_g = abs(fun.value(th, True) - val) / abs(val), rel_err(fun.grad(th, True), g_ad)
        print('value and gradient under new weights', e_v, e_g)
        assert e_v < 1e-11 and e_g < 1e-10
        with pytest.raises(ValueError):                                  # the resident factor was built under the old weights
            fun.solve(th, R, resident_factor=True)
    finally:
        fun.weights_par.set_vector(f['w'])
    assert np.allclose(fun.solve(th, R), base, rtol=1e-6, atol=1e-12)


def test_refusals_by_error_code(vb):
    hip = vb._hip
    rng = np.random.default_rng(43)

    def context(N, P, with_y=True, with_x=True):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=P)
        if with_x:
            ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)))
        if with_y:
            ctx.set_data(hip.SLOT_Y, (rng.uniform(size=N) < 0.5).astype(np.float64))
        return ctx

    def call(ctx, P, G, K, var=None, r=None, nodes=20, n0=0, n1=None, group=False, Q=2, G_arg=None):
        N = ctx.n_obs
        Kc = min(max(K, 1), 5)
        m = np.zeros(P)
        v = np.ones(P) if var is None else var
        e = np.zeros(G * Kc)
        rr = np.ones(G * Kc) if r is None else r
        gx, gw = np.zeros(max(nodes, 1)), np.ones(max(nodes, 1))
        Ag, Al = np.ones((Q, 2 * P)), np.ones((G, 2 * Kc, Q))
        out = np.empty((max(N, G), Q))
        head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G if G_arg is None else G_arg, K,
                gx.ctypes.data, gw.ctypes.data, nodes, Ag.ctypes.data, Al.ctypes.data, Q)
        if group:
            return ctx._lib.lrvb_glmm_slopes_group_influence(*head, out.ctypes.data)
        return ctx._lib.lrvb_glmm_slopes_obs_influence(*head, n0, N if n1 is None else n1, out.ctypes.data)
    N, G, K = 20, 3, 2
    gid = np.arange(N) % G
    for group in (False, True):
        wide = context(N, 65)
        assert call(wide, 65, G, K, group=group) == hip.ERR_UNSUPPORTED    # P > 64
        ctx = context(N, 3)
        assert call(ctx, 3, G, 0, group=group) == hip.ERR_UNSUPPORTED and call(ctx, 3, G, 5, group=group) == hip.ERR_UNSUPPORTED
        assert call(ctx, 3, G, K, nodes=129, group=group) == hip.ERR_UNSUPPORTED
        assert call(ctx, 3, G, K, group=group) == hip.ERR_STATE            # no groups
        ctx.set_groups(gid, G)
        assert call(ctx, 3, G, K, group=group) == hip.ERR_STATE            # no group design
        noy = context(N, 3, with_y=False)
        noy.set_groups(gid, G)
        noy.set_group_design(np.ones((N, K)))
        assert call(noy, 3, G, K, group=group) == hip.ERR_STATE            # no responses
        nox = context(N, 3, with_x=False)
        nox.set_groups(gid, G)
        nox.set_group_design(np.ones((N, K)))
        assert call(nox, 3, G, K, group=group) == hip.ERR_STATE            # no design matrix
        ctx.set_group_design(np.ones((N + 1, K)))
        assert call(ctx, 3, G, K, group=group) == hip.ERR_STATE            # z with another row count
        ctx.set_group_design(np.ones((N, K)))
        assert call(ctx, 3, G, 1, group=group) == hip.ERR_STATE            # z has another K
        assert call(ctx, 3, G, K, var=np.array([1.0, 0.0, 1.0]), group=group) == hip.ERR_INVALID
        bad_r = np.ones(G * K)
        bad_r[G * K - 1] = -1.0
        assert call(ctx, 3, G, K, r=bad_r, group=group) == hip.ERR_INVALID
        assert call(ctx, 3, G, K, G_arg=G + 1, group=group) == hip.ERR_SIZE
        assert call(ctx, 3, G, K, group=group) == hip.OK
    # a bad row range: the code lrvb_glmm_obs_influence returns for the same mistake
    assert call(ctx, 3, G, K, n0=5, n1=4) == hip.ERR_INVALID
    assert call(ctx, 3, G, K, n0=0, n1=N + 1) == hip.ERR_INVALID
    assert call(ctx, 3, G, K, n0=N, n1=N) == hip.OK
    pt = (np.zeros(3), np.ones(3), np.zeros((G, K)), np.ones((G, K)), np.zeros(20), np.ones(20))
    with pytest.raises(ValueError):
        ctx.glmm_slopes_obs_influence(*pt, np.ones((2, 2 * 3 + 2 * G * K + 1)))
    with pytest.raises(ValueError):
        ctx.glmm_slopes_group_influence(*pt, np.ones((2, 2 * 3)))
    with pytest.raises(ValueError):                                      # LRVB_ERR_INVALID surfaces as ValueError
        ctx.glmm_slopes_obs_influence(*pt, np.ones((2, 2 * 3 + 2 * G * K)), n0=3, n1=2)


def _psi_derivs(rho, s, deg=20):
    """psi_rho and psi_s by Gauss-Hermite in plain numpy (Stein's identity for the derivative in s)."""
    gx, gw = np.polynomial.hermite.hermgauss(deg)
    t = rho[:, None] + np.sqrt(2.0 * s)[:, None] * gx[None, :]
    sg = 1.0 / (1.0 + np.exp(-t))
    wk = gw / np.sqrt(np.pi)
    return sg @ wk, 0.5 * ((sg * (1.0 - sg)) @ wk)


def test_full_size_rows_and_groups(vb):
    """N = 1e6, P = 64, K = 4, G = 1e4, Q = 16: a 4096-row window that no tile boundary aligns with and 50 groups against a numpy
    restatement to 1e-9; wall times (host call, copies included) are printed, none is asserted."""
    N, P, K, G, Q = 1000000, 64, 4, 10000, 16
    rng = np.random.default_rng(1)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), rng.standard_normal((N, K - 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    u = rng.normal(size=(G, K)) * 0.7
    beta = rng.normal(size=P) * 0.8
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid]).sum(1))))).astype(np.float64)
    w = rng.uniform(0.5, 1.5, size=N)
    _, fun = _model(vb, x, y, z, w, gid, G)
    m, v, e, r = beta, np.full(P, np.exp(-6.0)), u, np.full((G, K), np.exp(-3.0))
    pt = (m, v, e, r, fun.gh_x, fun.gh_w)
    A = rng.normal(size=(Q, 2 * P + 2 * G * K))
    Ae, Ar = A[:, 2 * P:2 * P + G * K].reshape(Q, G, K), A[:, 2 * P + G * K:].reshape(Q, G, K)

    def rows_np(idx):
        xs, zs, gs = x[idx], z[idx], gid[idx]
        p_rho, p_s = _psi_derivs(xs @ m + (zs * e[gs]).sum(1), (xs * xs) @ v + (zs * zs * r[gs]).sum(1))
        a1, a2 = p_rho - y[idx], p_s
        return (a1[:, None] * (xs @ A[:, :P].T + np.einsum('nk,qnk->nq', zs, Ae[:, gs]))
                + a2[:, None] * ((xs * xs) @ A[:, P:2 * P].T + np.einsum('nk,qnk->nq', zs * zs, Ar[:, gs])))
    n0 = 500001
    win = fun.ctx.glmm_slopes_obs_influence(*pt, A, n0=n0, n1=n0 + 4096)
    e_w = rel_err(win, rows_np(np.arange(n0, n0 + 4096)))
    print('window', e_w)
    assert e_w < 1e-9
    t0 = time.perf_counter()
    full = fun.ctx.glmm_slopes_obs_influence(*pt, A)
    t1 = time.perf_counter()
    grp = fun.ctx.glmm_slopes_group_influence(*pt, A)
    t2 = time.perf_counter()
    print('rows N x 16: %.4f s, group influence G x 16: %.4f s (wall)' % (t1 - t0, t2 - t1))
    assert np.all(np.isfinite(full)) and np.array_equal(full[n0:n0 + 4096], win)
    some = rng.choice(G, size=50, replace=False)
    want = np.stack([(w[np.flatnonzero(gid == g), None] * rows_np(np.flatnonzero(gid == g))).sum(axis=0) for g in some])
    e_g = rel_err(grp[some], want)
    print('groups', e_g)
    assert e_g < 1e-9

"""Streamed weight influence of `LogisticGLMMObjective`: the row entry `lrvb_glmm_obs_influence`, the group entry
`lrvb_glmm_group_influence`, the arrow solve behind `obs_influence(..., chol=None)` and `lrvb_cov`, against torch autograd of
tests/glmm_reference.py.  Tolerances are the project's for the same kind of quantity: products and influence rows 1e-9 relative
(tests/test_gpu_glmm.py, tests/test_gpu_influence.py), sums in another order 1e-10 / 1e-9, quantities behind an H^-1 rtol 1e-6
(with the atol = 1e-12 of the sensitivities of tests/test_gpu_glmm.py where entries pass through zero)."""
import time

import numpy as np
import pytest
import torch

import glmm_reference as ref
from helpers import rel_err
from test_gpu_glmm import HYP, _model, _targs, _eta, _fit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _point(fun, eta, P, G):
    ng = 2 * P + 4
    return (eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:], fun.gh_x, fun.gh_w)


def _rows_ad(x, y, w, gid, G, eta, A):
    """A @ C (transposed: N x Q), C = d2 KL / d (m, v, e, r) d w^T by torch autograd of the reference: row q is the derivative
    with respect to the weights of A[q] . (gradient in (m, v, e, r))."""
    P = x.shape[1]
    ng = 2 * P + 4
    t = ref.tensors(x, y, w, gid, HYP)
    z = torch.tensor(np.concatenate([eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:]]), requires_grad=True)
    wt = t[2].clone().requires_grad_(True)
    et = torch.cat([z[:P], 1.0 / z[P:2 * P], torch.tensor(eta[2 * P:ng]), z[2 * P:2 * P + G], 1.0 / z[2 * P + G:]])
    g, = torch.autograd.grad(ref.kl_vec(et, t[0], t[1], wt, t[3], G, t[4]), z, create_graph=True)
    return np.stack([torch.autograd.grad(g @ torch.tensor(A[q]), wt, retain_graph=True)[0].numpy() for q in range(A.shape[0])], axis=1)


def _segment_sum(gid, G, v):
    out = np.zeros((G,) + v.shape[1:])
    np.add.at(out, gid, v)
    return out


@pytest.mark.parametrize('N,P,G', [(1, 1, 1), (37, 3, 5), (500, 8, 40), (1999, 17, 3), (4096, 64, 300), (20011, 30, 1000)])
def test_rows_against_autograd_and_windows(vb, N, P, G):
    x, y, w, gid, free = ref.problem(N, P, G, seed=N + P)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2      # an empty group, one with more than half the rows
    par, fun = _model(vb, x, y, w, gid, G)
    eta = _eta(free, P, G)
    pt = _point(fun, eta, P, G)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G))
    want = _rows_ad(x, y, w, gid, G, eta, A)
    for Q in (1, 5, 16, 21):
        got = fun.ctx.glmm_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', N, P, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        for n0, n1 in ((5, 700), (N // 3, N // 3 + 1), (63, 129), (N, N), (0, 0)):
            n0, n1 = min(n0, N), min(n1, N)
            win = fun.ctx.glmm_obs_influence(*pt, A[:Q], n0=n0, n1=n1)
            assert win.shape == (n1 - n0, Q) and np.array_equal(win, got[n0:n1])
            if n1 > n0:
                assert rel_err(win, want[n0:n1, :Q]) < 1e-9


def test_rows_do_not_depend_on_the_weights(vb):
    N, P, G = 3001, 7, 23
    x, y, w, gid, free = ref.problem(N, P, G, seed=5)
    eta = _eta(free, P, G)
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G))
    _, f1 = _model(vb, x, y, np.ones(N), gid, G)
    w0 = w.copy()
    zero = np.array([0, 17, 64, 1500, N - 1])
    w0[zero] = 0.0
    _, f0 = _model(vb, x, y, w0, gid, G)
    a, b = f1.ctx.glmm_obs_influence(*_point(f1, eta, P, G), A), f0.ctx.glmm_obs_influence(*_point(f0, eta, P, G), A)
    assert np.all(np.abs(a[zero]) > 0)
    assert np.array_equal(a, b)                                           # a left-out row still gets the influence of adding it


@pytest.mark.parametrize('N,P,G,Q', [(3001, 7, 23, 5), (20011, 30, 1000, 21), (1, 1, 1, 1), (4096, 64, 300, 16)])
def test_group_sums(vb, N, P, G, Q):
    x, y, w, gid, free = ref.problem(N, P, G, seed=N + P)
    eta = _eta(free, P, G)
    A = np.random.default_rng(7).normal(size=(Q, 2 * P + 2 * G))
    _, fun = _model(vb, x, y, w, gid, G)
    pt = _point(fun, eta, P, G)
    rows = fun.ctx.glmm_obs_influence(*pt, A)
    want = _segment_sum(gid, G, w[:, None] * rows)
    a, b = fun.ctx.glmm_group_influence(*pt, A), fun.ctx.glmm_group_influence(*pt, A)
    e = rel_err(a, want)
    print('group sums', N, P, G, Q, e)
    assert a.shape == (G, Q) and e < 1e-10
    assert np.array_equal(a, b)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)      # the empty group
    perm = np.random.default_rng(6).permutation(N)
    _, fun2 = _model(vb, x[perm], y[perm], w[perm], gid[perm], G)
    assert rel_err(fun2.ctx.glmm_group_influence(*pt, A), a) < 1e-9


def test_reduce_hook_contract_and_shards(vb):
    N, P, G, Q = 2001, 6, 11, 5
    x, y, w, gid, free = ref.problem(N, P, G, seed=9)
    order = np.argsort(gid, kind='stable')                               # sorted rows: the cut below goes through group 0
    x, y, w, gid = x[order], y[order], w[order], gid[order]
    eta = _eta(free, P, G)
    A = np.random.default_rng(8).normal(size=(Q, 2 * P + 2 * G))
    _, full = _model(vb, x, y, w, gid, G)
    pt = _point(full, eta, P, G)
    ctx = full.ctx
    base_g, base_r = ctx.glmm_group_influence(*pt, A), ctx.glmm_obs_influence(*pt, A)
    sizes = []
    ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))
    rows = ctx.glmm_obs_influence(*pt, A)
    assert sizes == []                                                   # per-observation rows stay rank-local
    grp = ctx.glmm_group_influence(*pt, A)
    assert sizes == [G * Q]
    ctx.set_reduce_hook(None)
    assert np.array_equal(rows, base_r) and np.array_equal(grp, base_g)
    n1 = 700
    assert gid[n1 - 1] == gid[n1]                                        # a group straddling the cut
    _, f1 = _model(vb, x[:n1], y[:n1], w[:n1], gid[:n1], G)
    _, f2 = _model(vb, x[n1:], y[n1:], w[n1:], gid[n1:], G)
    s = f1.ctx.glmm_group_influence(*pt, A) + f2.ctx.glmm_group_influence(*pt, A)
    assert rel_err(s, base_g) < 1e-10
    assert np.array_equal(np.vstack([f1.ctx.glmm_obs_influence(*pt, A), f2.ctx.glmm_obs_influence(*pt, A)]), base_r)


@pytest.fixture(scope='module')
def fitted(vb):
    """The N = 3000, P = 4, G = 30 problem of tests/test_gpu_glmm.py::test_fit_lrvb_and_sensitivities at its optimum, with the
    dense Hessian and the weight cross Hessian of the reference by torch autograd."""
    N, P, G = 3000, 4, 30
    x, y, w, gid, free0 = ref.problem(N, P, G, seed=77, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, w, gid, G)
    objective = vb.Objective(par, fun)
    th = _fit(objective, np.zeros(free0.size))
    assert np.max(np.abs(objective.fun_free_grad(th))) < 1e-6
    targs = _targs(x, y, w, gid, G)
    _, _, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    wt = targs[2].clone().requires_grad_(True)
    p = torch.tensor(th).requires_grad_(True)
    g, = torch.autograd.grad(ref.kl_free(p, targs[0], targs[1], wt, targs[3], G, targs[5]), p, create_graph=True)
    Cw = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())])
    return dict(N=N, P=P, G=G, gid=gid, w=w, par=par, fun=fun, objective=objective, th=th, H_ad=H_ad, Cw=Cw)


def test_end_to_end_at_a_fitted_point(vb, fitted):
    f = fitted
    fun, par, th, P, G = f['fun'], f['par'], f['th'], f['P'], f['G']
    ng = 2 * P + 4
    D = ng + 2 * G
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
    # the solve itself, with local rows on the right-hand side, on the host and with the factor resident on the global context
    R = np.random.default_rng(4).normal(size=(D, 3))
    Hinv = np.linalg.inv(f['H_ad'])
    assert np.allclose(fun.solve(th, R), Hinv @ R, rtol=1e-6, atol=1e-12)
    fun.global_hessian(th, want_host=False)
    fun._ensure_gctx().chol_factor_last()
    assert np.allclose(fun.solve(th, R, resident_factor=True), Hinv @ R, rtol=1e-6, atol=1e-12)
    with pytest.raises(ValueError):                                      # the resident factor belongs to another point
        fun.solve(th + 1e-3, R, resident_factor=True)
    # LRVB covariance of beta and three group effects: a block that needs the whole arrow
    idx = np.concatenate([np.arange(P), ng + np.array([0, 11, G - 1])])
    M = np.eye(D)[idx]
    cov = fun.lrvb_cov(th, M)
    assert np.allclose(cov, Hinv[np.ix_(idx, idx)], rtol=1e-6, atol=0)
    assert np.allclose(fun.lrvb_cov(th, np.eye(ng)[:P]), Hinv[:P, :P], rtol=1e-6, atol=0)


def test_leave_one_group_out(vb, fitted):
    """The streamed prediction theta - group_influence[g] lands as close to the refit without group g as the dense torch-AD
    prediction does (a test of the kernel, not of the quality of the linear approximation)."""
    f = fitted
    fun, th, P, G, gid, w = f['fun'], f['th'], f['P'], f['G'], f['gid'], f['w']
    D = 2 * P + 4 + 2 * G
    gi = fun.group_influence(th, np.eye(D))
    assert gi.shape == (G, D)
    g = int(np.argmax(np.max(np.abs(gi), axis=1)))
    w2 = w.copy()
    w2[gid == g] = 0.0
    pred = th - gi[g]                                                    # the multiplier on the group's weights goes from 1 to 0
    pred_ad = th - np.linalg.solve(f['H_ad'], f['Cw']) @ (w2 - w)
    fun.weights_par.set_vector(w2)
    try:
        th2 = _fit(f['objective'], th)
    finally:
        fun.weights_par.set_vector(w)
    d, d_ad, step = np.max(np.abs(pred - th2)), np.max(np.abs(pred_ad - th2)), np.max(np.abs(th2 - th))
    print('leave group {} out: |pred - refit| {:.3e}, AD prediction {:.3e}, |refit - theta| {:.3e}'.format(g, d, d_ad, step))
    assert step > 0
    assert d <= d_ad + 1e-6 * step


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

    def call(ctx, P, G, var=None, r=None, nodes=20, n0=0, n1=None, group=False, Q=2):
        N = ctx.n_obs
        m = np.zeros(P)
        v = np.ones(P) if var is None else var
        e = np.zeros(G)
        rr = np.ones(G) if r is None else r
        gx, gw = np.zeros(max(nodes, 1)), np.ones(max(nodes, 1))
        Ag, Al = np.ones((Q, 2 * P)), np.ones((G, 2 * Q))
        out = np.empty((max(N, G), Q))
        head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, gx.ctypes.data, gw.ctypes.data, nodes,
                Ag.ctypes.data, Al.ctypes.data, Q)
        if group:
            return ctx._lib.lrvb_glmm_group_influence(*head, out.ctypes.data)
        return ctx._lib.lrvb_glmm_obs_influence(*head, n0, N if n1 is None else n1, out.ctypes.data)
    N, G = 20, 3
    gid = np.arange(N) % G
    for group in (False, True):
        wide = context(N, 65)
        assert call(wide, 65, G, group=group) == hip.ERR_UNSUPPORTED       # P > 64
        ctx = context(N, 3)
        assert call(ctx, 3, G, group=group) == hip.ERR_STATE               # no groups
        noy = context(N, 3, with_y=False)
        noy.set_groups(gid, G)
        assert call(noy, 3, G, group=group) == hip.ERR_STATE               # no responses
        nox = context(N, 3, with_x=False)
        nox.set_groups(gid, G)
        assert call(nox, 3, G, group=group) == hip.ERR_STATE               # no design matrix (responses and groups are set)
        ctx.set_groups(gid, G)
        assert call(ctx, 3, G, var=np.array([1.0, 0.0, 1.0]), group=group) == hip.ERR_INVALID
        assert call(ctx, 3, G, r=np.array([1.0, 1.0, -1.0]), group=group) == hip.ERR_INVALID
        assert call(ctx, 3, G, nodes=129, group=group) == hip.ERR_UNSUPPORTED
        assert call(ctx, 3, G, group=group) == hip.OK
    # a bad row range: the code lrvb_obs_influence returns for the same mistake
    assert call(ctx, 3, G, n0=5, n1=4) == hip.ERR_INVALID
    assert call(ctx, 3, G, n0=0, n1=N + 1) == hip.ERR_INVALID
    assert call(ctx, 3, G, n0=N, n1=N) == hip.OK
    pt = (np.zeros(3), np.ones(3), np.zeros(G), np.ones(G), np.zeros(20), np.ones(20))
    with pytest.raises(ValueError):
        ctx.glmm_obs_influence(*pt, np.ones((2, 2 * 3 + 2 * G + 1)))
    with pytest.raises(ValueError):
        ctx.glmm_group_influence(*pt, np.ones((2, 2 * 3)))
    with pytest.raises(ValueError):                                      # LRVB_ERR_INVALID surfaces as ValueError
        ctx.glmm_obs_influence(*pt, np.ones((2, 2 * 3 + 2 * G)), n0=3, n1=2)


def _psi_derivs(rho, s, deg=20):
    """psi_rho and psi_s by Gauss-Hermite in plain numpy (Stein's identity for the derivative in s)."""
    gx, gw = np.polynomial.hermite.hermgauss(deg)
    t = rho[:, None] + np.sqrt(2.0 * s)[:, None] * gx[None, :]
    sg = 1.0 / (1.0 + np.exp(-t))
    wk = gw / np.sqrt(np.pi)
    return sg @ wk, 0.5 * ((sg * (1.0 - sg)) @ wk)


def test_full_size_rows_and_groups(vb):
    """N = 1e6, P = 64, G = 1e4, Q = 16: a 4096-row window that no tile boundary aligns with and 50 groups against the numpy
    restatement to 1e-9; wall times (host call, copies included) are printed, best of 3."""
    N, P, G, Q = 1000000, 64, 10000, 16
    rng = np.random.default_rng(1)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    u = rng.normal(size=G) * 0.7
    beta = rng.normal(size=P) * 0.8
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + u[gid])))).astype(np.float64)
    w = rng.uniform(0.5, 1.5, size=N)
    _, fun = _model(vb, x, y, w, gid, G)
    m, v, e, r = beta, np.full(P, np.exp(-6.0)), u, np.full(G, np.exp(-3.0))
    pt = (m, v, e, r, fun.gh_x, fun.gh_w)
    A = rng.normal(size=(Q, 2 * P + 2 * G))

    def rows_np(idx):
        xs, gs = x[idx], gid[idx]
        p_rho, p_s = _psi_derivs(xs @ m + e[gs], (xs * xs) @ v + r[gs])
        a1, a2 = p_rho - y[idx], p_s
        return (a1[:, None] * (xs @ A[:, :P].T + A[:, 2 * P + gs].T)
                + a2[:, None] * ((xs * xs) @ A[:, P:2 * P].T + A[:, 2 * P + G + gs].T))
    n0 = 500001
    win = fun.ctx.glmm_obs_influence(*pt, A, n0=n0, n1=n0 + 4096)
    e_w = rel_err(win, rows_np(np.arange(n0, n0 + 4096)))
    print('window', e_w)
    assert e_w < 1e-9
    t_rows, t_grp = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        full = fun.ctx.glmm_obs_influence(*pt, A)
        t1 = time.perf_counter()
        grp = fun.ctx.glmm_group_influence(*pt, A)
        t2 = time.perf_counter()
        t_rows.append(t1 - t0); t_grp.append(t2 - t1)
    print('rows N x 16: %.4f s, group influence G x 16: %.4f s (wall, best of 3)' % (min(t_rows), min(t_grp)))
    assert np.all(np.isfinite(full)) and np.array_equal(full[n0:n0 + 4096], win)
    some = rng.choice(G, size=50, replace=False)
    want = np.stack([(w[np.flatnonzero(gid == g), None] * rows_np(np.flatnonzero(gid == g))).sum(axis=0) for g in some])
    e_g = rel_err(grp[some], want)
    print('groups', e_g)
    assert e_g < 1e-9

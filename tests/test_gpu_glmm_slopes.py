"""`LogisticGLMMSlopesObjective` (logistic mixed model with K <= 4 random effects per group, block-arrow Hessian) on the GPU against
the torch reference tests/glmm_slopes_reference.py.  Tolerances are the project's for this kind of quantity
(tests/test_gpu_glmm.py): value 1e-11, gradient 1e-10, Hessian, products and Schur complement 1e-9 relative; LRVB covariance
rtol 1e-6."""
import time

import numpy as np
import pytest

import glmm_reference as ref1
import glmm_slopes_reference as ref
from helpers import rel_err

pytestmark = pytest.mark.gpu

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _par(vb, P, K, G):
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    return par


def _model(vb, x, y, z, w, gid, G, hyp=HYP, deg=20):
    par = _par(vb, x.shape[1], z.shape[1], G)
    fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, beta_prior_info=hyp[0], mu_prior=hyp[1:3], tau_prior=hyp[3:5],
                                         gh_deg=deg, weights=w)
    return par, fun


def _targs(x, y, z, w, gid, G, hyp=HYP):
    t = ref.tensors(x, y, z, w, gid, hyp)
    return (t[0], t[1], t[2], t[3], t[4], G, t[5])


def _eta(free, P, K, G):
    return np.where(ref.positive_mask(P, K, G), np.exp(free), free)


def _schur(H, ng):
    return H[:ng, :ng] - H[:ng, ng:] @ np.linalg.solve(H[ng:, ng:], H[ng:, :ng])


def _assert_local_blocks_posdef(Hf, ng, G, K):
    """On the REFERENCE Hessian: every local 2 K x 2 K block is positive definite, so a NOT_POSDEF from the device is a finding
    about the kernel, not about the inputs."""
    gk = np.arange(G * K).reshape(G, K)
    li = ng + np.concatenate([gk, G * K + gk], axis=1)
    blocks = Hf[li[:, :, None], li[:, None, :]]
    assert np.all(np.linalg.eigvalsh(blocks) > 0)


def _point(eta, P, K, G):
    ng = 2 * P + 4 * K
    return (eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G * K].reshape(G, K), 1.0 / eta[ng + G * K:].reshape(G, K))


def _check_against_reference(vb, x, y, z, w, gid, G, free, deg=20, schur=True):
    N, P = x.shape
    K = z.shape[1]
    par, fun = _model(vb, x, y, z, w, gid, G, deg=deg)
    targs = _targs(x, y, z, w, gid, G) + (deg,)
    ng = 2 * P + 4 * K
    eta = _eta(free, P, K, G)
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    e = [abs(fun.value(eta, False) - val) / abs(val), rel_err(fun.grad(eta, False), g), rel_err(fun.hessian(eta, False), H)]
    print('vector', N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    assert np.allclose(par['u']['mean'].get(), eta[ng:ng + G * K].reshape(G, K))     # par holds the evaluation point
    valf, gf, Hf = ref.value_grad_hess(ref.kl_free, free, targs)
    Hd = fun.hessian(free, True)
    e = [abs(fun.value(free, True) - valf) / abs(valf), rel_err(fun.grad(free, True), gf), rel_err(Hd, Hf)]
    print('free', N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    assert np.allclose(par['beta']['mean'].get(), free[:P])
    objective = vb.Objective(par, fun)
    v = np.random.default_rng(3).normal(size=free.size)
    assert rel_err(objective.fun_free_hvp(free, v), Hf @ v) < 1e-9
    assert rel_err(fun.sparse_hessian(free).toarray(), Hd) < 1e-14
    if not schur:
        return fun, Hf
    _assert_local_blocks_posdef(Hf, ng, G, K)
    HS = fun.global_hessian(free)
    e_s = rel_err(HS, _schur(Hf, ng))
    print('schur', e_s)
    assert e_s < 1e-9
    return fun, Hf


# seeds: the first of N + P + K, N + P + K + 1, .. at which the reference Hessian (free coordinates) is positive definite at the
# point of `problem` -- found on the CPU; every local block and the Schur complement are then positive definite too.  At
# (500, 8, 3, 40) -- about six rows per group and component triple -- no seed from 511 to 536 gives a positive definite Hessian at
# that point (smallest eigenvalue -0.1 to -0.6), while every local block is positive definite (smallest eigenvalue 0.09 to 0.2):
# there the Schur complement is checked as everywhere, its inverse is no covariance, and the device factorisation must refuse it.
SHAPES = [(1, 1, 1, 1, 3), (37, 3, 2, 5, 43), (500, 8, 3, 40, 511), (1999, 17, 4, 3, 2020), (4096, 64, 4, 150, 4164), (130, 64, 4, 2, 198)]


@pytest.mark.parametrize('N,P,K,G,seed', SHAPES)
def test_value_grad_hessian_products_schur_and_covariance(vb, N, P, K, G, seed):
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=seed)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2      # an empty group, one with more than half the rows
    fun, Hf = _check_against_reference(vb, x, y, z, w, gid, G, free)
    ng = 2 * P + 4 * K
    gc = fun._ensure_gctx()
    fun.global_hessian(free, want_host=False)
    if np.min(np.linalg.eigvalsh(Hf)) <= 0:
        assert (N, P, K, G) == (500, 8, 3, 40)
        with pytest.raises(np.linalg.LinAlgError):
            gc.chol_factor_last()
        return
    gc.chol_factor_last()
    Hinv = np.linalg.inv(Hf)
    assert np.allclose(gc.lrvb_cov(np.eye(ng)[:P]), Hinv[:P, :P], rtol=1e-6, atol=0)
    # the whole arrow, a moment with local columns, the Schur complement solved by the resident factor
    M = np.zeros((2, free.size))
    M[0, 0], M[1, ng + (G * K) // 2] = 1.0, 1.0
    idx = [0, ng + (G * K) // 2]
    assert np.allclose(fun.lrvb_cov(free, M), Hinv[np.ix_(idx, idx)], rtol=1e-6, atol=1e-12)
    S = fun.solve(free, np.ascontiguousarray(M.T), resident_factor=True)
    assert np.allclose(M @ S, Hinv[np.ix_(idx, idx)], rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize('N,P,G', [(37, 3, 5), (2500, 9, 30)])
def test_one_effect_with_unit_design_equals_the_intercept_class(vb, N, P, G):
    x, y, w, gid, free = ref1.problem(N, P, G, seed=N + P)
    par1 = vb.ModelParamsDict('params')
    par1.push_param(vb.UVNParamVector('beta', length=P))
    par1.push_param(vb.UVNParam('mu'))
    par1.push_param(vb.GammaParam('tau'))
    par1.push_param(vb.UVNParamVector('u', length=G))
    old = vb.LogisticGLMMObjective(par1, x, y, gid, G, beta_prior_info=HYP[0], mu_prior=HYP[1:3], tau_prior=HYP[3:5], weights=w)
    _, new = _model(vb, x, y, np.ones((N, 1)), w, gid, G)
    v0, v1 = old.value(free, True), new.value(free, True)
    assert abs(v1 - v0) < 1e-12 * abs(v0)
    assert rel_err(new.grad(free, True), old.grad(free, True)) < 1e-12
    assert rel_err(new.hessian(free, True), old.hessian(free, True)) < 1e-12
    _, _, Hf = ref1.value_grad_hess(ref1.kl_free, free, (lambda t: (t[0], t[1], t[2], t[3], G, t[4]))(ref1.tensors(x, y, w, gid, HYP)))
    _assert_local_blocks_posdef(Hf, 2 * P + 4, G, 1)
    assert rel_err(new.global_hessian(free), old.global_hessian(free)) < 1e-12


def test_terms_are_bitwise_reproducible_and_order_independent(vb):
    N, P, K, G = 3001, 7, 2, 23
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=5)
    eta = _eta(free, P, K, G)
    _, fun = _model(vb, x, y, z, w, gid, G)
    pt = _point(eta, P, K, G) + (fun.gh_x, fun.gh_w)
    a, b = fun.ctx.glmm_slopes_terms(*pt), fun.ctx.glmm_slopes_terms(*pt)
    assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    perm = np.random.default_rng(6).permutation(N)
    _, fun2 = _model(vb, x[perm], y[perm], z[perm], w[perm], gid[perm], G)
    c = fun2.ctx.glmm_slopes_terms(*pt)
    assert abs(c[0] - a[0]) < 1e-12 * abs(a[0])
    assert all(rel_err(p, q) < 1e-12 for p, q in zip(c[1:], a[1:]))


def test_edge_inputs_against_reference(vb):
    N, P, K, G = 300, 5, 3, 7
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=11, empty_group=False)
    # zero weights on a whole group
    w0 = w.copy()
    w0[gid == 2] = 0.0
    assert np.any(gid == 2)
    _check_against_reference(vb, x, y, z, w0, gid, G, free, schur=False)
    # a group of one row
    gid1 = gid.copy()
    gid1[gid1 == 4] = 3
    gid1[17] = 4
    assert np.sum(gid1 == 4) == 1
    _check_against_reference(vb, x, y, z, w, gid1, G, free, schur=False)
    # a component whose design column is identically zero: its local rows are prior-only
    z0 = z.copy()
    z0[:, 1] = 0.0
    fun, Hf = _check_against_reference(vb, x, y, z0, w, gid, G, free, schur=False)
    ng = 2 * P + 4 * K
    e_g1 = ng + np.arange(G) * K + 1
    assert np.all(Hf[np.ix_(np.arange(2 * P), e_g1)] == 0.0)
    # the extremes of the quadrature
    _check_against_reference(vb, x, y, z, w, gid, G, free, deg=1, schur=False)
    _check_against_reference(vb, x, y, z, w, gid, G, free, deg=128, schur=False)


def _fit(vb, objective, theta0):
    th, _ = vb.OptimizationUtils.minimize_objective_trust_ncg(objective, theta0, False, maxiter=200, gtol=1e-7, disp=False)
    th = np.asarray(th, dtype=np.float64)
    for _ in range(8):                                   # Newton polish where the ratio test stalls at the rounding of f
        g = objective.fun_free_grad(th)
        if np.max(np.abs(g)) < 1e-8:
            break
        th = th - objective.fun.solve(th, g)
    return th


def test_fit_covariance_and_tau_prior_sensitivity(vb):
    N, P, K, G = 4000, 6, 2, 60
    x, y, z, w, gid, free0 = ref.problem(N, P, K, G, seed=77, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, gid, G)
    ng = 2 * P + 4 * K
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = _targs(x, y, z, w, gid, G)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    assert np.max(np.abs(g_ad)) < 1e-6                                   # stationary by the REFERENCE gradient
    assert np.min(np.linalg.eigvalsh(H_ad)) > 0
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    cov = gc.lrvb_cov(np.eye(ng)[:P])
    assert np.allclose(cov, np.linalg.inv(H_ad)[:P, :P], rtol=1e-6, atol=0)
    par.set_free(th)
    assert np.all(np.diag(cov) > 1.0 / par['beta']['info'].get())
    # the tau prior: the linear prediction of the global parameters against a central difference of refits, to the tolerance of
    # the leave-one-out check of tests/test_gpu_glmm.py::test_fit_lrvb_and_sensitivities (5 % of the change + 1e-8)
    sens = fun.global_sensitivity(fun.tau_prior_par, th)
    h = np.array([0.05, -0.03])
    base = np.asarray(fun.tau_prior_par.get_vector(), dtype=np.float64).copy()
    fun.tau_prior_par.set_vector(base + h)
    th_p = _fit(vb, objective, th)
    fun.tau_prior_par.set_vector(base - h)
    th_m = _fit(vb, objective, th)
    fun.tau_prior_par.set_vector(base)
    diff = 0.5 * (th_p - th_m)[:ng]
    assert np.max(np.abs(sens @ h - diff)) < 0.05 * np.max(np.abs(diff)) + 1e-8


def test_reduce_hook_contract_and_shards(vb):
    N, P, K, G = 2001, 6, 2, 11
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=9)
    order = np.argsort(gid, kind='stable')                               # sorted rows: the cut below goes through group 0
    x, y, z, w, gid = x[order], y[order], z[order], w[order], gid[order]
    eta = _eta(free, P, K, G)
    ng = 2 * P + 4 * K
    _, full = _model(vb, x, y, z, w, gid, G)
    pt = _point(eta, P, K, G) + (full.gh_x, full.gh_w)
    ctx = full.ctx
    ncol = 2 * K + K * (2 * K + 1) + 4 * K * P
    base = (ctx.glmm_slopes_terms(*pt), ctx.glmm_slopes_terms(*pt, want_hess=False))
    sizes = []
    ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))
    out = [ctx.glmm_slopes_terms(*pt)]
    assert sizes == [3 * P * P + G * ncol + 2 * P + 1]
    out.append(ctx.glmm_slopes_terms(*pt, want_hess=False))
    assert sizes[1:] == [G * ncol + 2 * P + 1]
    ctx.set_reduce_hook(None)
    for p, q in zip(base, out):
        assert p[0] == q[0] and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(p[1:], q[1:]))
    # two shards, a group straddling the cut
    n1 = 700
    assert gid[n1 - 1] == gid[n1]
    _, f1 = _model(vb, x[:n1], y[:n1], z[:n1], w[:n1], gid[:n1], G)
    _, f2 = _model(vb, x[n1:], y[n1:], z[n1:], w[n1:], gid[n1:], G)
    s_sum = f1.local_stats(eta) + f2.local_stats(eta)
    assert s_sum.size == f1.stats_size()
    assert rel_err(s_sum, full.local_stats(eta)) < 1e-11
    targs = _targs(x, y, z, w, gid, G)
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    f1.set_reduced_stats(s_sum, eta)
    assert abs(f1.value(eta, False) - val) < 1e-11 * abs(val)
    assert rel_err(f1.grad(eta, False), g) < 1e-10 and rel_err(f1.hessian(eta, False), H) < 1e-9
    _, _, Hf = ref.value_grad_hess(ref.kl_free, free, targs)
    _assert_local_blocks_posdef(Hf, ng, G, K)
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

    def call(ctx, P, G, K, nodes=20):
        m, v = np.zeros(P), np.ones(P)
        e, rr = np.zeros(max(G * K, 1)), np.ones(max(G * K, 1))
        gx, gw = np.zeros(max(nodes, 1)), np.ones(max(nodes, 1))
        val = np.empty(1)
        return ctx._lib.lrvb_glmm_slopes_terms(ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, K,
                                               gx.ctypes.data, gw.ctypes.data, nodes, val.ctypes.data, None, None, None, 0)

    def design(ctx, n, K):
        zz = np.ones((n, max(K, 1)))
        return ctx._lib.lrvb_set_group_design(ctx._h, zz.ctypes.data, n, K)
    N, G = 20, 3
    gid = np.arange(N) % G
    wide = context(N, 65)
    assert call(wide, 65, G, 2) == hip.ERR_UNSUPPORTED                    # P > 64
    ctx = context(N, 3)
    assert design(ctx, N, 0) == hip.ERR_UNSUPPORTED and design(ctx, N, 5) == hip.ERR_UNSUPPORTED
    assert call(ctx, 3, G, 0) == hip.ERR_UNSUPPORTED and call(ctx, 3, G, 5) == hip.ERR_UNSUPPORTED
    assert call(ctx, 3, G, 2, nodes=129) == hip.ERR_UNSUPPORTED
    assert call(ctx, 3, G, 2) == hip.ERR_STATE                            # no groups
    ctx.set_groups(gid, G)
    assert call(ctx, 3, G, 2) == hip.ERR_STATE                            # no group design
    noy = context(N, 3, with_y=False)
    noy.set_groups(gid, G)
    assert design(noy, N, 2) == hip.OK
    assert call(noy, 3, G, 2) == hip.ERR_STATE                            # no responses
    assert design(ctx, N + 1, 2) == hip.OK
    assert call(ctx, 3, G, 2) == hip.ERR_STATE                            # z with another row count
    ctx.set_groups(gid, G)                                                # ... which the next lrvb_set_groups drops
    assert call(ctx, 3, G, 2) == hip.ERR_STATE
    assert design(ctx, N, 2) == hip.OK
    assert call(ctx, 3, G, 1) == hip.ERR_STATE                            # z has another K
    K = 2
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((6 + 3 * K, 6 + 3 * K))
    schur = lambda k=K: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, k, M.ctypes.data)
    assert schur() == hip.ERR_STATE                                       # no group sums resident
    assert schur(5) == hip.ERR_UNSUPPORTED
    assert call(ctx, 3, G, 2) == hip.OK
    assert schur() == hip.OK
    loc[1, 2 * K] = -1.0                                                  # entry (1, 1) of group 1's block
    assert schur() == hip.ERR_NOT_POSDEF
    ctx.set_groups(gid, G)
    assert schur() == hip.ERR_STATE                                       # lrvb_set_groups drops the resident sums


def test_full_size(vb):
    """N = 1e6, P = 64, K = 4, G = 1e4: build, Schur step and one hvp; value and gradient against the reference on the rows of
    50 groups.  The times are printed, none is asserted."""
    N, P, K, G = 1000000, 64, 4, 10000
    rng = np.random.default_rng(1)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), rng.standard_normal((N, K - 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    u = rng.normal(size=(G, K)) * 0.7
    beta = rng.normal(size=P) * 0.8
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid]).sum(1))))).astype(np.float64)
    free = np.concatenate([beta, np.full(P, 6.0), np.zeros(K), np.full(K, 3.0), np.tile([np.log(G / 2.0), np.log(G / 4.0)], K),
                           u.ravel(), np.full(G * K, 3.0)])
    par, fun = _model(vb, x, y, z, None, gid, G)
    ng = 2 * P + 4 * K
    t0 = time.perf_counter()
    HS = fun.global_hessian(free)
    t1 = time.perf_counter()
    assert np.all(np.isfinite(HS))
    fun._ensure_gctx().chol_factor_last()
    xg = rng.normal(size=ng)
    out = fun.hvp(free, np.concatenate([xg, np.zeros(2 * G * K)]), True)
    t2 = time.perf_counter()
    out2 = fun.hvp(free, np.concatenate([xg, np.zeros(2 * G * K)]), True)
    t3 = time.perf_counter()
    print('global_hessian %.3f s, first hvp (arrow build) %.3f s, cached hvp %.4f s' % (t1 - t0, t2 - t1, t3 - t2))
    assert np.all(np.isfinite(out)) and np.array_equal(out, out2)
    # the arrow product is consistent with the Schur complement: H_S x_g = global part of H [x_g; -H_ll^-1 H_lg x_g]
    from lrvb_amd import glmm_slopes as gs
    loc = fun._pieces[4]
    lo = gs._to_groups(out[ng:], G, K)[:, :, 0]
    sol = gs._from_groups(gs.block_arrow_local_solve(loc, lo)[:, :, None], G, K)[:, 0]
    back = fun.hvp(free, np.concatenate([xg, -sol]), True)
    assert rel_err(back[:ng], HS @ xg) < 1e-9
    # value and gradient of the data term on the rows of 50 groups, against the reference
    sub = np.flatnonzero(gid < 50)
    Gs = 50
    eta = _eta(free, P, K, G)
    eta_s = np.concatenate([eta[:ng], eta[ng:ng + Gs * K], eta[ng + G * K:ng + G * K + Gs * K]])
    free_s = np.concatenate([free[:ng], free[ng:ng + Gs * K], free[ng + G * K:ng + G * K + Gs * K]])
    _, fsub = _model(vb, x[sub], y[sub], z[sub], None, gid[sub], Gs)
    targs = _targs(x[sub], y[sub], z[sub], np.ones(sub.size), gid[sub], Gs)
    val, g, _ = ref.value_grad_hess(ref.kl_vec, eta_s, targs, want_hess=False)
    assert abs(fsub.value(eta_s, False) - val) < 1e-11 * abs(val)
    assert rel_err(fsub.grad(eta_s, False), g) < 1e-10
    # ... and the same group sums from the full-size pass (the rows of a group are the same rows, in the same order)
    pt = _point(eta, P, K, G) + (fun.gh_x, fun.gh_w)
    gs_full = fun.ctx.glmm_slopes_terms(*pt, want_hess=False)[3]
    pts = _point(eta_s, P, K, Gs) + (fun.gh_x, fun.gh_w)
    gs_sub = fsub.ctx.glmm_slopes_terms(*pts, want_hess=False)[3]
    assert rel_err(gs_full[:Gs], gs_sub) < 1e-12

"""`PoissonGLMMObjective` (Poisson mixed model with K <= 4 random effects per group, exposure offset, block-arrow Hessian;
DESIGN.md section 26) on the GPU against the torch reference tests/glmm_poisson_reference.py.  Tolerances are those of the
sibling model (tests/test_gpu_glmm_slopes.py): value 1e-11, gradient 1e-10, Hessian, products and Schur complement 1e-9
relative; LRVB covariance and solves rtol 1e-6.  The arithmetic behind the per-row coefficients is the same and the coefficient
is one exp.  At all six shapes the reference Hessian and every local block are positive definite at the point of `problem`
(checked on the CPU: smallest eigenvalue 0.086 to 0.28, local blocks >= 0.155), so no covariance or solve check is skipped."""
import numpy as np
import pytest

import glmm_poisson_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _schur, _assert_local_blocks_posdef, _point, _fit

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (37, 3, 2, 5), (500, 8, 3, 40), (1999, 17, 4, 3), (4096, 64, 4, 150), (130, 64, 4, 2)]


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _model(vb, x, y, z, w, o, gid, G, hyp=HYP):
    K = 1 if z is None else z.shape[1]
    par = _par(vb, x.shape[1], K, G)
    fun = vb.PoissonGLMMObjective(par, x, y, z, gid, G, offset=o, beta_prior_info=hyp[0], mu_prior=hyp[1:3], tau_prior=hyp[3:5],
                                  weights=w)
    return par, fun


def _check_against_reference(vb, x, y, z, w, o, gid, G, free, solves=True):
    """Value, gradient, Hessian (vector and free coordinates), products, sparse Hessian, Schur complement; with `solves` the
    covariance and the solve of a moment with a local column, by the host route and on the device."""
    N, P = x.shape
    K = z.shape[1]
    par, fun = _model(vb, x, y, z, w, o, gid, G)
    targs = ref.targs(x, y, z, w, o, gid, G, HYP)
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
    _assert_local_blocks_posdef(Hf, ng, G, K)
    e_s = rel_err(fun.global_hessian(free), _schur(Hf, ng))
    print('schur', e_s)
    assert e_s < 1e-9
    if not solves:
        return fun, Hf
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    Hinv = np.linalg.inv(Hf)
    M = np.zeros((2, free.size))
    idx = [0, ng + (G * K) // 2]
    M[0, idx[0]], M[1, idx[1]] = 1.0, 1.0
    want = Hinv[np.ix_(idx, idx)]
    for on_device in (False, True):
        assert np.allclose(fun.lrvb_cov(free, M, on_device=on_device), want, rtol=1e-6, atol=1e-12)
        S = fun.solve(free, np.ascontiguousarray(M.T), on_device=on_device)
        assert S.shape == (free.size, 2) and np.allclose(M @ S, want, rtol=1e-6, atol=1e-12)
        assert np.allclose(S, Hinv[:, idx], rtol=1e-6, atol=1e-12)
        assert np.allclose(par['beta']['mean'].get(), free[:P])         # par holds the evaluation point afterwards
        assert np.allclose(par['u']['mean'].get(), free[ng:ng + G * K].reshape(G, K))
    return fun, Hf


@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G):
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=N + P + K)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2      # an empty group, one with more than half the rows
    _check_against_reference(vb, x, y, z, w, o, gid, G, free)


@pytest.mark.parametrize('N', [64, 65])
def test_tile_edges(vb, N):
    P, K, G = 5, 2, 3
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=N + P + K)
    _check_against_reference(vb, x, y, z, w, o, gid, G, free)


def _terms(fun, eta):
    P, K, G = fun.P, fun.K, fun.G
    return fun.ctx.glmm_poisson_terms(*_point(eta, P, K, G))


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))


def test_offset(vb):
    N, P, K, G = 300, 5, 2, 7
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=21)
    eta = _eta(free, P, K, G)
    _, f_none = _model(vb, x, y, z, w, None, gid, G)
    _, f_zero = _model(vb, x, y, z, w, np.zeros(N), gid, G)
    assert _same(_terms(f_none, eta), _terms(f_zero, eta))
    # a constant added to the offset and taken from the coefficient of a ones column of x leaves gradient and Hessian unchanged
    x1 = x.copy()
    x1[:, 0] = 1.0
    c = 0.37
    eta_c = eta.copy()
    eta_c[0] -= c
    _, f_a = _model(vb, x1, y, z, w, o, gid, G)
    _, f_b = _model(vb, x1, y, z, w, o + c, gid, G)
    assert np.any(o != 0.0)
    ta, tb = _terms(f_a, eta), _terms(f_b, eta_c)                        # the data term: gradient, H blocks, group sums
    assert all(rel_err(q, p) < 1e-12 for p, q in zip(ta[1:], tb[1:]))
    # the whole objective: the prior 1/2 tau_beta m_0^2 sees the moved coefficient, in the gradient's entry 0 and nowhere else
    ga, gb = f_a.grad(eta, False), f_b.grad(eta_c, False)
    gb[0] += HYP[0] * c
    assert rel_err(gb, ga) < 1e-12
    assert rel_err(f_b.hessian(eta_c, False), f_a.hessian(eta, False)) < 1e-12


def test_unit_design(vb):
    N, P, G = 300, 4, 6
    x, y, z, w, gid, o, free = ref.problem(N, P, 1, G, seed=22)
    eta = _eta(free, P, 1, G)
    _, f_none = _model(vb, x, y, None, w, o, gid, G)
    _, f_ones = _model(vb, x, y, np.ones((N, 1)), w, o, gid, G)
    assert f_none.K == 1 and _same(_terms(f_none, eta), _terms(f_ones, eta))
    assert f_none.value(eta, False) == f_ones.value(eta, False)
    assert np.array_equal(f_none.hessian(eta, False), f_ones.hessian(eta, False))


def test_terms_are_bitwise_reproducible_and_order_independent(vb):
    N, P, K, G = 3001, 7, 2, 23
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=5)
    eta = _eta(free, P, K, G)
    _, fun = _model(vb, x, y, z, w, o, gid, G)
    a, b = _terms(fun, eta), _terms(fun, eta)
    assert _same(a, b)
    perm = np.random.default_rng(6).permutation(N)
    _, fun2 = _model(vb, x[perm], y[perm], z[perm], w[perm], o[perm], gid[perm], G)
    c = _terms(fun2, eta)
    assert abs(c[0] - a[0]) < 1e-12 * abs(a[0])
    assert all(rel_err(p, q) < 1e-12 for p, q in zip(c[1:], a[1:]))


def test_edge_inputs_against_reference(vb):
    N, P, K, G = 300, 5, 3, 7
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=11, empty_group=False)
    # all y = 0
    _check_against_reference(vb, x, np.zeros(N), z, w, o, gid, G, free)
    # some w = 0: a whole group and scattered rows
    w0 = w.copy()
    w0[gid == 2] = 0.0
    w0[[0, 17, 64, N - 1]] = 0.0
    assert np.any(gid == 2)
    _check_against_reference(vb, x, y, z, w0, o, gid, G, free)
    # one group holding every row (the others are empty).  At this point -- no optimum -- the reference Hessian has the
    # eigenvalue -0.21 (found on the CPU; the Poisson Hessian does not depend on y, the six prior-only groups decide it), so its
    # inverse is no covariance: everything up to the Schur complement is checked, every local block being positive definite
    _check_against_reference(vb, x, y, z, w, o, np.full(N, 3, dtype=np.int32), G, free, solves=False)
    # G = 1
    x, y, z, w, gid, o, free = ref.problem(N, P, K, 1, seed=12)
    assert np.all(gid == 0)
    _check_against_reference(vb, x, y, z, w, o, gid, 1, free)


def test_fit_covariance_and_tau_prior_sensitivity(vb):
    N, P, K, G = 2000, 4, 2, 30
    x, y, z, w, gid, o, free0 = ref.problem(N, P, K, G, seed=77, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, o, gid, G)
    ng = 2 * P + 4 * K
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = ref.targs(x, y, z, w, o, gid, G, HYP)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    print('reference gradient at the fit', np.max(np.abs(g_ad)))
    assert np.max(np.abs(g_ad)) < 1e-6                                   # stationary by the REFERENCE gradient
    assert np.min(np.linalg.eigvalsh(H_ad)) > 0
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    cov = gc.lrvb_cov(np.eye(ng)[:P])
    assert np.allclose(cov, np.linalg.inv(H_ad)[:P, :P], rtol=1e-6, atol=0)
    par.set_free(th)
    assert np.all(np.diag(cov) > 1.0 / par['beta']['info'].get())
    # the tau prior: the bound of tests/test_gpu_glmm_slopes.py::test_fit_covariance_and_tau_prior_sensitivity (5 % of the
    # change + 1e-8) against a central difference of refits
    sens = fun.global_sensitivity(fun.tau_prior_par, th)
    h = np.array([0.05, -0.03])
    base = np.asarray(fun.tau_prior_par.get_vector(), dtype=np.float64).copy()
    fun.tau_prior_par.set_vector(base + h)
    th_p = _fit(vb, objective, th)
    fun.tau_prior_par.set_vector(base - h)
    th_m = _fit(vb, objective, th)
    fun.tau_prior_par.set_vector(base)
    diff = 0.5 * (th_p - th_m)[:ng]
    print('tau prior sensitivity', np.max(np.abs(sens @ h - diff)), np.max(np.abs(diff)))
    assert np.max(np.abs(sens @ h - diff)) < 0.05 * np.max(np.abs(diff)) + 1e-8


def test_reduce_hook_contract_and_shards(vb):
    N, P, K, G = 2001, 6, 2, 11
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=9)
    order = np.argsort(gid, kind='stable')                               # sorted rows: the cut below goes through group 0
    x, y, z, w, gid, o = x[order], y[order], z[order], w[order], gid[order], o[order]
    eta = _eta(free, P, K, G)
    ng = 2 * P + 4 * K
    _, full = _model(vb, x, y, z, w, o, gid, G)
    pt = _point(eta, P, K, G)
    ctx = full.ctx
    ncol = 2 * K + K * (2 * K + 1) + 4 * K * P
    base = (ctx.glmm_poisson_terms(*pt), ctx.glmm_poisson_terms(*pt, want_hess=False))
    sizes = []
    ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))
    out = [ctx.glmm_poisson_terms(*pt)]
    assert sizes == [3 * P * P + G * ncol + 2 * P + 1]                   # exactly one hook call per terms call
    out.append(ctx.glmm_poisson_terms(*pt, want_hess=False))
    assert sizes[1:] == [G * ncol + 2 * P + 1]
    A = np.random.default_rng(8).normal(size=(5, 2 * P + 2 * G * K))
    ctx.glmm_poisson_obs_influence(*pt, A)
    assert len(sizes) == 2                                               # per-observation rows stay rank-local
    ctx.glmm_poisson_group_influence(*pt, A)
    assert sizes[2:] == [G * 5]                                          # exactly one per group-influence call
    ctx.set_reduce_hook(None)
    for p, q in zip(base, out):
        assert p[0] == q[0] and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(p[1:], q[1:]))
    # two shards, a group straddling the cut
    n1 = 700
    assert gid[n1 - 1] == gid[n1]
    _, f1 = _model(vb, x[:n1], y[:n1], z[:n1], w[:n1], o[:n1], gid[:n1], G)
    _, f2 = _model(vb, x[n1:], y[n1:], z[n1:], w[n1:], o[n1:], gid[n1:], G)
    s_sum = f1.local_stats(eta) + f2.local_stats(eta)
    assert s_sum.size == f1.stats_size()
    targs = ref.targs(x, y, z, w, o, gid, G, HYP)
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    f1.set_reduced_stats(s_sum, eta)
    assert abs(f1.value(eta, False) - val) < 1e-11 * abs(val)
    assert rel_err(f1.grad(eta, False), g) < 1e-10 and rel_err(f1.hessian(eta, False), H) < 1e-9
    assert abs(f1.value(eta, False) - full.value(eta, False)) < 1e-11 * abs(val)
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
        ctx = vb.DeviceContext(blocks, loss='poisson', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)) / np.sqrt(P))
        if with_y:
            ctx.set_data(hip.SLOT_Y, rng.poisson(2.0, size=N).astype(np.float64))
        return ctx

    def call(ctx, P, G, K, var=None, r=None, G_arg=None, kind='terms'):
        Kc = min(max(K, 1), 5)
        m = np.zeros(P)
        v = np.ones(P) if var is None else var
        e = np.zeros(max(G * Kc, 1))
        rr = np.ones(max(G * Kc, 1)) if r is None else r
        head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G if G_arg is None else G_arg, K)
        if kind == 'terms':
            val = np.empty(1)
            return ctx._lib.lrvb_glmm_poisson_terms(*head, val.ctypes.data, None, None, None, 0)
        Q = 2
        Ag, Al = np.ones((Q, 2 * P)), np.ones((max(G, 1), 2 * Kc, Q))
        out = np.empty((max(ctx.n_obs, G), Q))
        if kind == 'group':
            return ctx._lib.lrvb_glmm_poisson_group_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, out.ctypes.data)
        return ctx._lib.lrvb_glmm_poisson_obs_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, 0, ctx.n_obs, out.ctypes.data)

    N, G, K = 20, 3, 2
    gid = np.arange(N) % G
    for kind in ('terms', 'rows', 'group'):
        wide = context(N, 65)
        assert call(wide, 65, G, K, kind=kind) == hip.ERR_UNSUPPORTED    # P = 65
        ctx = context(N, 3)
        assert call(ctx, 3, G, 5, kind=kind) == hip.ERR_UNSUPPORTED      # K = 5
        assert call(ctx, 3, G, 0, kind=kind) == hip.ERR_UNSUPPORTED
        assert call(ctx, 3, G, K, kind=kind) == hip.ERR_STATE            # no groups
        ctx.set_groups(gid, G)
        assert call(ctx, 3, G, K, kind=kind) == hip.ERR_STATE            # no group design
        ctx.set_group_design(np.ones((N, K)))
        assert call(ctx, 3, G, 1, kind=kind) == hip.ERR_STATE            # a design of another K
        noy = context(N, 3, with_y=False)
        noy.set_groups(gid, G)
        noy.set_group_design(np.ones((N, K)))
        assert call(noy, 3, G, K, kind=kind) == hip.ERR_STATE            # no responses
        ctx.set_offset(np.zeros(N + 1))
        assert call(ctx, 3, G, K, kind=kind) == hip.ERR_STATE            # an offset of the wrong length
        ctx.set_offset(None)
        assert call(ctx, 3, G, K, kind=kind) == hip.OK                   # NULL clears it
        ctx.set_offset(np.zeros(N))
        assert call(ctx, 3, G, K, var=np.array([1.0, 0.0, 1.0]), kind=kind) == hip.ERR_INVALID
        bad_r = np.ones(G * K)
        bad_r[G * K - 1] = -1.0
        assert call(ctx, 3, G, K, r=bad_r, kind=kind) == hip.ERR_INVALID
        assert call(ctx, 3, G, K, G_arg=G + 1, kind=kind) == hip.ERR_SIZE   # a wrong G
        assert call(ctx, 3, G, K, kind=kind) == hip.OK
    # lrvb_glmm_slopes_schur after Poisson terms of another K
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((6 + 3 * K, 6 + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    assert call(ctx, 3, G, K) == hip.OK and schur() == hip.OK            # the Poisson sums are what the Schur entry works on
    ctx.set_group_design(np.ones((N, 1)))
    assert call(ctx, 3, G, 1) == hip.OK
    assert schur() == hip.ERR_STATE
    ctx.set_group_design(np.ones((N, K)))
    assert call(ctx, 3, G, K) == hip.OK and schur() == hip.OK
    ctx.set_offset(np.zeros(N))
    assert schur() == hip.ERR_STATE                                      # lrvb_set_offset drops the resident sums


def test_python_layer_refusals_and_overflow(vb):
    N, P, K, G = 60, 3, 2, 4
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=31, empty_group=False)
    eta = _eta(free, P, K, G)
    for bad in (-1.0, np.nan, np.inf):
        yb = y.copy()
        yb[7] = bad
        with pytest.raises(ValueError):
            _model(vb, x, yb, z, w, o, gid, G)
    with pytest.raises(ValueError):
        _model(vb, x, y, z, w, o[:-1], gid, G)
    ob = o.copy()
    ob[3] = np.nan
    with pytest.raises(ValueError):
        _model(vb, x, y, z, w, ob, gid, G)
    # one row's offset at 800: exp overflows in fp64, the value is not finite and the entry says so (no fault, no clamp)
    ob = o.copy()
    ob[3] = 800.0
    _, fun = _model(vb, x, y, z, w, ob, gid, G)
    with pytest.raises(ValueError, match='not finite'):
        fun.value(eta, False)
    with pytest.raises(ValueError, match='not finite'):
        fun.hessian(eta, False)
    _, ok = _model(vb, x, y, z, w, o, gid, G)
    assert np.isfinite(ok.value(eta, False))


def test_coexistence_with_the_logistic_entries(vb):
    """Poisson terms, logistic slopes terms, Poisson terms on ONE context: the first and third bitwise equal, the logistic
    result bitwise that of a fresh logistic-only context (the offset does not leak, nor does anything else)."""
    N, P, K, G = 700, 6, 3, 9
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=41)
    y = np.minimum(y, 1.0)                                               # responses both likelihoods accept
    eta = _eta(free, P, K, G)
    pt = _point(eta, P, K, G)
    _, fun = _model(vb, x, y, z, w, o, gid, G)
    par2 = _par(vb, P, K, G)
    logi = vb.LogisticGLMMSlopesObjective(par2, x, y, z, gid, G, weights=w)
    gh = (logi.gh_x, logi.gh_w)
    a = fun.ctx.glmm_poisson_terms(*pt)
    mid = fun.ctx.glmm_slopes_terms(*pt, *gh)
    b = fun.ctx.glmm_poisson_terms(*pt)
    assert _same(a, b)
    assert _same(mid, logi.ctx.glmm_slopes_terms(*pt, *gh))
    A = np.random.default_rng(1).normal(size=(5, 2 * P + 2 * G * K))
    assert np.array_equal(fun.ctx.glmm_slopes_group_influence(*pt, *gh, A), logi.ctx.glmm_slopes_group_influence(*pt, *gh, A))
    assert np.array_equal(fun.ctx.glmm_slopes_obs_influence(*pt, *gh, A), logi.ctx.glmm_slopes_obs_influence(*pt, *gh, A))
    assert _same(fun.ctx.glmm_poisson_terms(*pt), a)

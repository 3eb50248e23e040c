"""`BinomialGLMMObjective` and `NegBinomialGLMMObjective` on the GPU: the BinomialLik instantiation of the
shared tile walk bit for bit against the pinned logistic one, against the torch references tests/glmm_binomial_reference.py, the
aggregation and offset identities, the state contract of lrvb_set_trials / lrvb_set_offset and a fit.  Tolerances are those of
the sibling models (tests/test_gpu_glmm_slopes.py, tests/test_gpu_glmm_poisson.py): value 1e-11, gradient 1e-10, Hessian,
products and Schur complement 1e-9 relative; LRVB covariance and solves rtol 1e-6 -- the arithmetic is the logistic one times
m <= 12.

Positive definiteness of the reference free Hessian at the off-optimum point of `problem`, checked on the CPU for exactly these
draws: binomial 0.082 to 0.20 at the five smaller shapes (local blocks >= 0.209), -0.147 at (500, 8, 3, 40) (local blocks 0.159);
negative binomial (phi = 1.7 | vector) 0.098 to 0.19 at the five solve shapes with seed 23 at (37, 3, 2, 5) (-0.033 at its
default seed), -0.142 | -0.120 at (500, 8, 3, 40) (local blocks 0.150).  That one shape runs without the covariance and solve
checks; the other five assert positive definiteness and skip nothing."""
import numpy as np
import pytest

import glmm_binomial_reference as ref
import glmm_slopes_reference as sref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _schur, _assert_local_blocks_posdef, _point, _fit

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (37, 3, 2, 5), (65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7), (500, 8, 3, 40)]
NO_SOLVES = (500, 8, 3, 40)                                              # indefinite at the point of `problem` (module docstring)
BITWISE_SHAPES = [(65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7)]


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _prior_kw(hyp):
    return dict(beta_prior_info=hyp[0], mu_prior=hyp[1:3], tau_prior=hyp[3:5])


def _model(vb, x, y, z, w, o, mt, gid, G, hyp=HYP):
    K = 1 if z is None else z.shape[1]
    par = _par(vb, x.shape[1], K, G)
    return par, vb.BinomialGLMMObjective(par, x, y, z, gid, G, trials=mt, offset=o, weights=w, **_prior_kw(hyp))


def _nb_model(vb, x, y, z, w, o, phi, gid, G, hyp=HYP):
    par = _par(vb, x.shape[1], z.shape[1], G)
    return par, vb.NegBinomialGLMMObjective(par, x, y, z, gid, G, phi, offset=o, weights=w, **_prior_kw(hyp))


def _logistic(vb, x, y, z, w, gid, G, hyp=HYP):
    par = _par(vb, x.shape[1], z.shape[1], G)
    return par, vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, weights=w, **_prior_kw(hyp))


def _check_against_reference(par, fun, kl_vec, kl_free, targs, free, G, K, solves=True, value_shift=0.0):
    """The body of tests/test_gpu_glmm_poisson.py::_check_against_reference: value, gradient, Hessian (vector and free
    coordinates), products, sparse Hessian, Schur complement; with `solves` the covariance and the solve of a moment with a
    local column, by the host route and on the device.  `value_shift`: a constant the reference carries and the model drops."""
    N, P = fun.n_obs, fun.P
    ng = 2 * P + 4 * K
    eta = _eta(free, P, K, G)
    val, g, H = ref.value_grad_hess(kl_vec, eta, targs)
    val -= value_shift
    e = [abs(fun.value(eta, False) - val) / abs(val), rel_err(fun.grad(eta, False), g), rel_err(fun.hessian(eta, False), H)]
    print('vector', N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    assert np.allclose(par['u']['mean'].get(), eta[ng:ng + G * K].reshape(G, K))     # par holds the evaluation point
    valf, gf, Hf = ref.value_grad_hess(kl_free, free, targs)
    valf -= value_shift
    Hd = fun.hessian(free, True)
    e = [abs(fun.value(free, True) - valf) / abs(valf), rel_err(fun.grad(free, True), gf), rel_err(Hd, Hf)]
    print('free', N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    assert np.allclose(par['beta']['mean'].get(), free[:P])
    import lrvb_amd as vb
    objective = vb.Objective(par, fun)
    v = np.random.default_rng(3).normal(size=free.size)
    e_p = rel_err(objective.fun_free_hvp(free, v), Hf @ v)
    assert e_p < 1e-9
    assert rel_err(fun.sparse_hessian(free).toarray(), Hd) < 1e-14
    _assert_local_blocks_posdef(Hf, ng, G, K)
    e_s = rel_err(fun.global_hessian(free), _schur(Hf, ng))
    print('product', e_p, 'schur', e_s)
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


def _same(a, b):
    return a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))


# ---- A: bit for bit the logistic instantiation ------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', BITWISE_SHAPES)
def test_one_trial_no_offset_is_the_logistic_instantiation_bitwise(vb, N, P, K, G):
    """No tolerance: the walk, the flushes and the partial-row fixup of the BinomialLik instantiation against the pinned
    LogisticLik one -- once with no buffers (null pointers) and once with explicit ones and zeros (the staged path)."""
    x, y, z, w, gid, free = sref.problem(N, P, K, G, seed=N + P + K)
    eta = _eta(free, P, K, G)
    pt = _point(eta, P, K, G)
    _, logi = _logistic(vb, x, y, z, w, gid, G)
    gh = (logi.gh_x, logi.gh_w)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want_terms = logi.ctx.glmm_slopes_terms(*pt, *gh)
    assert want_terms[3].shape == (G, 2 * K + K * (2 * K + 1) + 4 * K * P)            # the full group sums, border included
    want_rows = {Q: logi.ctx.glmm_slopes_obs_influence(*pt, *gh, A[:Q], n0=3, n1=N - 2) for Q in (5, 21)}
    want_group = logi.ctx.glmm_slopes_group_influence(*pt, *gh, A)
    for mt, o in ((None, None), (np.ones(N), np.zeros(N))):
        _, fun = _model(vb, x, y, z, w, o, mt, gid, G)
        assert np.array_equal(fun.gh_x, gh[0]) and np.array_equal(fun.gh_w, gh[1])
        assert _same(fun.ctx.glmm_binomial_terms(*pt, *gh), want_terms)
        for Q in (5, 21):
            got = fun.ctx.glmm_binomial_obs_influence(*pt, *gh, A[:Q], n0=3, n1=N - 2)
            assert got.shape == (N - 5, Q) and np.array_equal(got, want_rows[Q])
        assert np.array_equal(fun.ctx.glmm_binomial_group_influence(*pt, *gh, A), want_group)


# ---- B: the binomial reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G):
    x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, seed=N + P + K)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2      # an empty group, one with more than half the rows
    par, fun = _model(vb, x, y, z, w, o, mt, gid, G)
    targs = ref.targs(x, y, z, w, o, mt, gid, G, HYP)
    _check_against_reference(par, fun, ref.kl_vec, ref.kl_free, targs, free, G, K, solves=(N, P, K, G) != NO_SOLVES)


# ---- C: the negative binomial reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G,phi', [s + (1.7,) for s in SHAPES] + [(65, 5, 2, 3, 'vector')])
def test_negative_binomial_reference_parity(vb, N, P, K, G, phi):
    seed = 23 if (N, P, K, G) == (37, 3, 2, 5) else N + P + K            # positive definite there (module docstring)
    x, y, z, w, gid, o, ph, free = ref.nb_problem(N, P, K, G, seed=seed, phi=phi)
    par, fun = _nb_model(vb, x, y, z, w, o, 1.7 if phi == 1.7 else ph, gid, G)
    targs = ref.targs(x, y, z, w, o, ph, gid, G, HYP)
    # the reference's (y + phi) logaddexp(log phi, t) carries phi log phi per row, which the model's form does not have
    shift = float(np.sum(w * ph * np.log(ph)))
    _check_against_reference(par, fun, ref.nb_kl_vec, ref.nb_kl_free, targs, free, G, K, solves=(N, P, K, G) != NO_SOLVES,
                             value_shift=shift)
    from scipy.special import gammaln
    assert abs(fun.log_norm_const() - np.sum(w * (gammaln(y + ph) - gammaln(ph) - gammaln(y + 1.0)))) < 1e-9


# ---- D: aggregation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 64, 4, 2)])
def test_aggregated_rows_equal_the_expanded_bernoulli_rows(vb, N, P, K, G):
    """y successes out of m trials with weight w = a row (y = 1, weight w y) and a row (y = 0, weight w (m - y)) of the
    logistic class, x and z duplicated, no offset."""
    x, y, z, w, gid, _, mt, free = ref.problem(N, P, K, G, seed=N + P + K)
    eta = _eta(free, P, K, G)
    _, fun = _model(vb, x, y, z, w, None, mt, gid, G)
    x2, z2, g2 = np.vstack([x, x]), np.vstack([z, z]), np.concatenate([gid, gid])
    y2 = np.concatenate([np.ones(N), np.zeros(N)])
    w2 = np.concatenate([w * y, w * (mt - y)])
    _, logi = _logistic(vb, x2, y2, z2, w2, g2, G)
    val = logi.value(eta, False)
    e = [abs(fun.value(eta, False) - val) / abs(val), rel_err(fun.grad(eta, False), logi.grad(eta, False)),
         rel_err(fun.hessian(eta, False), logi.hessian(eta, False))]
    print('aggregation', N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9


# ---- E: offset -------------------------------------------------------------------------------------------------------------
def test_offset(vb):
    N, P, K, G = 300, 5, 2, 7
    x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, seed=21)
    eta = _eta(free, P, K, G)
    terms = lambda f, at: f.ctx.glmm_binomial_terms(*_point(at, P, K, G), f.gh_x, f.gh_w)
    _, f_none = _model(vb, x, y, z, w, None, mt, gid, G)
    _, f_zero = _model(vb, x, y, z, w, np.zeros(N), mt, gid, G)
    assert _same(terms(f_none, eta), terms(f_zero, eta))
    # a constant added to the offset and taken from the coefficient of a ones column of x leaves gradient and Hessian unchanged
    x1 = x.copy()
    x1[:, 0] = 1.0
    c = 0.37
    eta_c = eta.copy()
    eta_c[0] -= c
    _, f_a = _model(vb, x1, y, z, w, o, mt, gid, G)
    _, f_b = _model(vb, x1, y, z, w, o + c, mt, gid, G)
    assert np.any(o != 0.0)
    ta, tb = terms(f_a, eta), terms(f_b, eta_c)                          # the data term: value, gradient, H blocks, group sums
    assert abs(ta[0] - tb[0]) < 1e-12 * abs(ta[0])                       # rho itself is unchanged, so is the y rho term
    assert all(rel_err(q, p) < 1e-12 for p, q in zip(ta[1:], tb[1:]))
    # the whole objective: the prior 1/2 tau_beta m_0^2 sees the moved coefficient, in the gradient's entry 0 and nowhere else
    ga, gb = f_a.grad(eta, False), f_b.grad(eta_c, False)
    gb[0] += HYP[0] * c
    assert rel_err(gb, ga) < 1e-12
    assert rel_err(f_b.hessian(eta_c, False), f_a.hessian(eta, False)) < 1e-12


# ---- F: state --------------------------------------------------------------------------------------------------------------
def test_trials_and_offset_state(vb):
    hip = vb._hip
    N, P, K, G = 130, 4, 2, 5
    x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, seed=31, empty_group=False)
    eta = _eta(free, P, K, G)
    pt = _point(eta, P, K, G)
    _, fun = _model(vb, x, y, z, w, o, mt, gid, G)
    ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
    m, v, e, r = [np.ascontiguousarray(a, dtype=np.float64) for a in pt]
    gx, gw = np.ascontiguousarray(gh[0]), np.ascontiguousarray(gh[1])
    head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, r.ctypes.data, G, K, gx.ctypes.data, gw.ctypes.data, gx.size)
    Q = 2
    Ag, Al, out = np.ones((Q, 2 * P)), np.ones((G, 2 * K, Q)), np.empty((max(N, G), Q))
    val = np.empty(1)
    entries = (lambda: ctx._lib.lrvb_glmm_binomial_terms(*head, val.ctypes.data, None, None, None, 0),
               lambda: ctx._lib.lrvb_glmm_binomial_obs_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, 0, N, out.ctypes.data),
               lambda: ctx._lib.lrvb_glmm_binomial_group_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, out.ctypes.data))
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    # the binomial sums are what the Schur entry works on; either setter drops them
    assert entries[0]() == hip.OK and schur() == hip.OK
    ctx.set_trials(mt)
    assert schur() == hip.ERR_STATE
    assert entries[0]() == hip.OK and schur() == hip.OK
    ctx.set_offset(o)
    assert schur() == hip.ERR_STATE
    # a buffer of the wrong length is found when an entry runs; NULL clears it
    for setter, good in ((ctx.set_trials, mt), (ctx.set_offset, o)):
        setter(np.ones(N + 1))
        assert [f() for f in entries] == [hip.ERR_STATE] * 3
        setter(None)
        assert [f() for f in entries] == [hip.OK] * 3
        setter(good)
        assert [f() for f in entries] == [hip.OK] * 3
    # cleared trials and offset are one trial and zero: the logistic result, bitwise
    ctx.set_trials(None)
    ctx.set_offset(None)
    assert _same(ctx.glmm_binomial_terms(*pt, *gh), ctx.glmm_slopes_terms(*pt, *gh))


def test_coexistence_with_the_logistic_entries(vb):
    """Binomial terms, logistic slopes terms, binomial terms on ONE context with trials and offset set: the first and third
    bitwise equal, the logistic results bitwise those of a logistic-only context (neither buffer leaks into them)."""
    N, P, K, G = 700, 6, 3, 9
    x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, seed=41)
    y = np.minimum(y, 1.0)                                               # responses both likelihoods accept
    mt = np.maximum(mt, 1.0)
    eta = _eta(free, P, K, G)
    pt = _point(eta, P, K, G)
    _, fun = _model(vb, x, y, z, w, o, mt, gid, G)
    _, logi = _logistic(vb, x, y, z, w, gid, G)
    gh = (logi.gh_x, logi.gh_w)
    a = fun.ctx.glmm_binomial_terms(*pt, *gh)
    mid = fun.ctx.glmm_slopes_terms(*pt, *gh)
    b = fun.ctx.glmm_binomial_terms(*pt, *gh)
    assert _same(a, b)
    want = logi.ctx.glmm_slopes_terms(*pt, *gh)
    assert _same(mid, want) and not _same(a, want)
    A = np.random.default_rng(1).normal(size=(5, 2 * P + 2 * G * K))
    assert np.array_equal(fun.ctx.glmm_slopes_group_influence(*pt, *gh, A), logi.ctx.glmm_slopes_group_influence(*pt, *gh, A))
    assert np.array_equal(fun.ctx.glmm_slopes_obs_influence(*pt, *gh, A), logi.ctx.glmm_slopes_obs_influence(*pt, *gh, A))
    assert _same(fun.ctx.glmm_binomial_terms(*pt, *gh), a)


# ---- G: fit ----------------------------------------------------------------------------------------------------------------
def test_fit_covariance_and_tau_prior_sensitivity(vb):
    """The thresholds of tests/test_gpu_glmm_poisson.py::test_fit_covariance_and_tau_prior_sensitivity; a solve with many
    groups at a point where the Hessian is positive definite by construction."""
    N, P, K, G = 2000, 4, 2, 30
    x, y, z, w, gid, o, mt, free0 = ref.problem(N, P, K, G, seed=77, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, o, mt, gid, G)
    ng = 2 * P + 4 * K
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = ref.targs(x, y, z, w, o, mt, gid, G, HYP)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    print('reference gradient at the fit', np.max(np.abs(g_ad)))
    assert np.max(np.abs(g_ad)) < 1e-6                                   # stationary by the REFERENCE gradient
    assert np.min(np.linalg.eigvalsh(H_ad)) > 0
    Hinv = np.linalg.inv(H_ad)
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    cov = gc.lrvb_cov(np.eye(ng)[:P])
    assert np.allclose(cov, Hinv[:P, :P], rtol=1e-6, atol=0)
    M = np.zeros((2, th.size))
    idx = [0, ng + (G * K) // 2]
    M[0, idx[0]], M[1, idx[1]] = 1.0, 1.0
    for on_device in (False, True):
        assert np.allclose(fun.lrvb_cov(th, M, on_device=on_device), Hinv[np.ix_(idx, idx)], rtol=1e-6, atol=1e-12)
    par.set_free(th)
    assert np.all(np.diag(cov) > 1.0 / par['beta']['info'].get())
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

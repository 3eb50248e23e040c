"""The device-resident block-arrow solve of `LogisticGLMMSlopesObjective` (`on_device=True`: lrvb_glmm_slopes_solve_forward /
lrvb_glmm_slopes_solve_back around the Schur factor on the global context) against the host route
`block_arrow_solve` at the same point.

Both routes solve the same matrix, so they are compared by what a solver can promise: the backward error
    eta(X) = ||R - H X||_F / (||H||_F ||X||_F + ||R||_F)
in `np.longdouble` with the dense H = fun.hessian(theta), required to be eta_dev <= 8 eta_host + D 2^-53 (8: the blocked GEMM sums
the groups in another order than `einsum`; the floor is one unit of backward error of a D-dimensional solve, for an eta_host that
is accidentally tiny), and the first-order forward bound, doubled: ||X_dev - X_host||_F <= 2 kappa_2(H) (eta_dev + eta_host)
||X_host||_F.  Seeds: the first of N + P + K, N + P + K + 1, .. at which the reference Hessian is positive definite at the point of
`problem` (found on the CPU, as in tests/test_gpu_glmm_slopes.py)."""
import numpy as np
import pytest

import glmm_slopes_reference as ref

pytestmark = pytest.mark.gpu

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0
#        N,    P, K,  G,   Q, seed
PARITY = [(130, 64, 4, 2, 21, 198),                                      # every group cut by a tile, Q no multiple of 16
          (4096, 64, 4, 150, 16, 4164),
          (600, 3, 1, 40, 1, 604),                                       # K = 1, vector right-hand side
          (300, 1, 3, 7, 5, 304),                                        # P = 1, empty last group
          (500, 5, 2, 60, 300, 11440)]                                   # Q above one workgroup of columns


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _model(vb, N, P, K, G, seed, **kw):
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=seed, **kw)
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, beta_prior_info=HYP[0], mu_prior=HYP[1:3], tau_prior=HYP[3:5], weights=w)
    return fun, free, (x, y, z, w, gid)


def _fro(a):
    return np.sqrt(np.sum(np.square(np.asarray(a, dtype=np.longdouble))))


def _backward_error(H, X, R):
    Hl, Xl, Rl = (np.asarray(a, dtype=np.longdouble).reshape(a.shape[0], -1) for a in (H, X, R))
    return float(_fro(Rl - Hl @ Xl) / (_fro(Hl) * _fro(Xl) + _fro(Rl)))


def _both_routes(fun, free, R):
    """(H, X_dev, X_host, eta_dev, eta_host, kappa) at one point."""
    H = fun.hessian(free)
    Xh = fun.solve(free, R, on_device=False)
    Xd = fun.solve(free, R, on_device=True)
    assert Xd.shape == Xh.shape == np.shape(R)
    return H, Xd, Xh, _backward_error(H, Xd, R), _backward_error(H, Xh, R), float(np.linalg.cond(H))


def _assert_forward_bound(dev, host, bound, what):
    diff, scale = float(_fro(np.asarray(dev) - np.asarray(host))), float(_fro(host))
    print('%s: ||dev - host|| / ||host|| = %.3e, bound %.3e' % (what, diff / scale, bound))
    assert diff <= bound * scale


@pytest.mark.parametrize('N,P,K,G,Q,seed', PARITY)
def test_parity_with_the_host_route(vb, N, P, K, G, Q, seed):
    fun, free, (_, _, _, _, gid) = _model(vb, N, P, K, G, seed)
    if (N, P, K, G) == (300, 1, 3, 7):
        assert not np.any(gid == G - 1)
    D = free.size
    rng = np.random.default_rng(seed)
    R = rng.normal(size=D) if Q == 1 else rng.normal(size=(D, Q))
    assert np.all(R.reshape(D, -1)[2 * P + 4 * K:] != 0.0)                # local rows in the right-hand side
    H, Xd, Xh, e_dev, e_host, kappa = _both_routes(fun, free, R)
    print('(N, P, K, G, Q) = %s: eta_dev %.3e, eta_host %.3e, kappa_2(H) %.4e' % ((N, P, K, G, Q), e_dev, e_host, kappa))
    assert e_dev <= 8.0 * e_host + D * 2.0 ** -53
    _assert_forward_bound(Xd, Xh, 2.0 * kappa * (e_dev + e_host), 'X')


def test_bitwise_reproducible_and_vector_equals_first_column(vb):
    N, P, K, G, Q, seed = PARITY[4]
    fun, free, _ = _model(vb, N, P, K, G, seed)
    R = np.random.default_rng(5).normal(size=(free.size, 19))
    X1 = fun.solve(free, R, on_device=True)
    X2 = fun.solve(free, R, on_device=True)
    assert np.array_equal(X1, X2)
    fun.value(free)                                                       # drops the factor: the next solve rebuilds everything
    assert np.array_equal(fun.solve(free, R, on_device=True), X1)
    xv = fun.solve(free, R[:, 0].copy(), on_device=True)
    xc = fun.solve(free, np.ascontiguousarray(R[:, :1]), on_device=True)
    assert xv.shape == (free.size,) and xc.shape == (free.size, 1)
    assert np.array_equal(xv, xc[:, 0])


def test_downstream_covariance_and_influence(vb):
    N, P, K, G, Q = 3001, 7, 3, 23, 5
    fun, free, _ = _model(vb, N, P, K, G, 3011)
    D, ng = free.size, 2 * P + 4 * K
    M = np.random.default_rng(9).normal(size=(Q, D))
    assert np.all(M[:, ng:] != 0.0)                                       # the moments include group-effect columns
    Rm = np.ascontiguousarray(M.T)
    H, Xd, Xh, e_dev, e_host, kappa = _both_routes(fun, free, Rm)
    bound = 2.0 * kappa * (e_dev + e_host)
    print('downstream: eta_dev %.3e, eta_host %.3e, kappa_2(H) %.4e' % (e_dev, e_host, kappa))
    _assert_forward_bound(Xd, Xh, bound, 'X')
    _assert_forward_bound(fun.lrvb_cov(free, M, on_device=True), fun.lrvb_cov(free, M), bound, 'lrvb_cov')
    _assert_forward_bound(fun.obs_influence(free, M, on_device=True), fun.obs_influence(free, M), bound, 'obs_influence')
    _assert_forward_bound(fun.obs_influence(free, M, n0=100, n1=1000, on_device=True), fun.obs_influence(free, M, n0=100, n1=1000),
                          bound, 'obs_influence window')
    _assert_forward_bound(fun.group_influence(free, M, on_device=True), fun.group_influence(free, M), bound, 'group_influence')


def _record(fun):
    """Wrap the terms and Schur calls of `fun`: lists of the want_border arguments and of the Schur builds."""
    terms, schur = [], []
    dt, sc = fun._device_terms, fun.ctx.glmm_slopes_schur

    def device_terms(eta, want_grad, want_hess, want_border=True):
        terms.append(bool(want_border))
        return dt(eta, want_grad, want_hess, want_border)

    def glmm_slopes_schur(*a):
        schur.append(1)
        return sc(*a)
    fun._device_terms, fun.ctx.glmm_slopes_schur = device_terms, glmm_slopes_schur
    return terms, schur


def test_no_border_copy_and_reuse_of_the_factor(vb):
    N, P, K, G, Q, seed = PARITY[3]
    fun, free, _ = _model(vb, N, P, K, G, seed)
    terms, schur = _record(fun)
    R = np.random.default_rng(2).normal(size=(free.size, 3))
    X = fun.solve(free, R, on_device=True)
    assert terms == [False] and len(schur) == 1                           # a fresh point: one terms call, the border stays
    X2 = fun.solve(free, 2.0 * R, on_device=True)
    assert terms == [False] and len(schur) == 1                           # the same point: nothing is rebuilt
    assert np.allclose(X2, 2.0 * X, rtol=1e-12, atol=0)
    fun.lrvb_cov(free, R.T, on_device=True)
    fun.group_influence(free, R.T, on_device=True)
    assert terms == [False] and len(schur) == 1


def test_invalidation_by_weights_and_hyper_parameters(vb):
    N, P, K, G, Q, seed = PARITY[2]
    fun, free, (_, _, _, w, _) = _model(vb, N, P, K, G, seed)
    terms, schur = _record(fun)
    R = np.random.default_rng(3).normal(size=(free.size, 4))
    X0 = fun.solve(free, R, on_device=True)
    assert len(schur) == 1
    for step, change in enumerate((lambda: fun.weights_par.set_vector(w * np.linspace(0.8, 1.2, N)),
                                   lambda: fun.tau_prior_par.set_vector(np.array([2.5, 1.7])))):
        built = len(schur)
        change()
        Xd = fun.solve(free, R, on_device=True)
        assert len(schur) == built + 1                                    # rebuilt at the new state
        assert not np.array_equal(Xd, X0)
        H, Xd2, Xh, e_dev, e_host, kappa = _both_routes(fun, free, R)
        assert np.array_equal(Xd2, Xd)
        assert e_dev <= 8.0 * e_host + free.size * 2.0 ** -53
        _assert_forward_bound(Xd, Xh, 2.0 * kappa * (e_dev + e_host), 'X after change %d' % step)
        X0 = Xd


def _status(ctx, method, *args):
    """The status code the C entry behind a context method returned."""
    seen = []
    ctx._check = seen.append
    try:
        method(*args)
    finally:
        del ctx._check
    assert len(seen) == 1
    return seen[0]


def test_refusals(vb):
    hip = vb._hip
    N, P, K, G, Q, seed = PARITY[3]
    fun, free, _ = _model(vb, N, P, K, G, seed)
    ctx, R = fun.ctx, 2 * P + 3 * K
    Rl, xc = np.ones((G, 2 * K, 3)), np.ones((R, 3))
    fwd = lambda a=Rl: _status(ctx, ctx.glmm_slopes_solve_forward, a)
    back = lambda a=xc, g=G, k=K: _status(ctx, ctx.glmm_slopes_solve_back, a, g, k)
    assert fwd() == hip.ERR_STATE and back() == hip.ERR_STATE             # no Schur yet
    fun.value(free)
    assert fwd() == hip.ERR_STATE                                         # group sums, but no factor
    fun.global_hessian(free, want_host=False)
    assert back() == hip.ERR_STATE                                        # back without a forward
    assert fwd() == hip.OK
    assert back(np.ones((R, 2))) == hip.ERR_SIZE                          # another Q than the forward before it
    assert back() == hip.OK
    assert fwd(np.ones((G + 1, 2 * K, 3))) == hip.ERR_SIZE and back(g=G - 1) == hip.ERR_SIZE
    assert fwd(np.ones((G, 10, 3))) == hip.ERR_UNSUPPORTED                # K = 5
    assert back(np.ones((2 * P + 15, 3)), k=5) == hip.ERR_UNSUPPORTED
    assert fwd(np.ones((G, 2 * K, 0))) == hip.ERR_INVALID and back(np.ones((R, 0))) == hip.ERR_INVALID    # Q = 0
    assert fwd() == hip.OK
    fun.global_hessian(free, want_host=False)
    assert back() == hip.ERR_STATE                                        # a new factor: the old forward pass is gone
    assert fwd() == hip.OK
    fun.value(free)                                                       # a later lrvb_glmm_slopes_terms drops the factor
    assert fwd() == hip.ERR_STATE and back() == hip.ERR_STATE
    # the keyword
    Rhs = np.ones(free.size)
    eta = np.where(ref.positive_mask(P, K, G), np.exp(free), free)
    with pytest.raises(ValueError):
        fun.solve(eta, Rhs, is_free=False, on_device=True)
    fun.set_reduced_stats(fun.local_stats(eta), eta)
    with pytest.raises(ValueError):
        fun.solve(free, Rhs, on_device=True)
    fun.set_reduced_stats(None)
    assert np.all(np.isfinite(fun.solve(free, Rhs, on_device=True)))


def test_local_block_not_positive_definite(vb):
    """Group 0 with e = 6 and log i = -4: its local block is indefinite on the REFERENCE Hessian (smallest eigenvalue about -350),
    so both routes must refuse the point."""
    N, P, K, G = 60, 2, 2, 3
    fun, free, (x, y, z, w, gid) = _model(vb, N, P, K, G, 5, big_group=False, empty_group=False)
    ng = 2 * P + 4 * K
    free = free.copy()
    free[ng:ng + K], free[ng + G * K:ng + G * K + K] = 6.0, -4.0
    t = ref.tensors(x, y, z, w, gid, HYP)
    _, _, Hf = ref.value_grad_hess(ref.kl_free, free, (t[0], t[1], t[2], t[3], t[4], G, t[5]))
    li = ng + np.concatenate([np.arange(K), G * K + np.arange(K)])
    assert np.min(np.linalg.eigvalsh(Hf[np.ix_(li, li)])) < -1.0
    Rhs = np.ones(free.size)
    with pytest.raises(np.linalg.LinAlgError):
        fun.solve(free, Rhs, on_device=False)
    with pytest.raises(np.linalg.LinAlgError):
        fun.solve(free, Rhs, on_device=True)
    with pytest.raises(np.linalg.LinAlgError):
        fun.lrvb_cov(free, np.eye(free.size)[:2], on_device=True)

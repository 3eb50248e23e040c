"""The estimated dispersion of `BetaGLMMObjective` and `NegBinomialGLMMObjective` on the GPU: the
BetaDispLik / NegBinDispLik instantiations of glmm_disp_rows_kernel and the host layer on top of them against the torch reference
tests/glmm_dispersion_reference.py (itself checked against mpmath in tests/test_glmm_dispersion_host_math.py), the entry-level
contract, finite differences of the device itself, state and side effects, refusals, the sensitivity against refits and the
profile-Newton fit.

Shapes (N, P, K, G), both families: (1, 1, 1, 1); (37, 3, 1, 5) bare (z=None, offset=None, a scalar phi0); (65, 5, 2, 3) with 5
nodes -- a second tile of one row, a cut group and an empty group; (130, 64, 4, 2) -- G = 2 cuts a group at both tile boundaries;
(300, 17, 4, 7) with every fifth weight zero.  phi0 is a scalar at the first three (Beta 7.5, NB2 1.7) and one value per row,
log-uniform on [0.5, 1e3] with both ends present, at the last two.  The point is the off-optimum one of the reference files'
`problem`.  lambda = 0 at every shape and lambda = 0.7 at (65, 5, 2, 3) and (300, 17, 4, 7): the push path.

Bounds (tests/test_gpu_glmm_beta.py): d1 and d2 1e-11, the value bound, relative to sum w |E h_l| + |lnc_l| (and the same with
h_ll), because the data part and the constant's part cancel at large phi; `cross` 1e-10, the gradient bound, in vector and free
coordinates; sensitivity and profile rtol 1e-6 on both routes, the solve bound; the identity with the host forms 1e-12 of the
largest magnitude; finite differences of the device's own F at delta = 1e-4 to 1e-6 relative.  The Beta Hessian at lambda = 0.7 is
positive definite at these points too (smallest reference eigenvalues printed by the parity test)."""
import numpy as np
import pytest

import glmm_beta_reference as beta_ref
import glmm_binomial_reference as bref
import glmm_dispersion_reference as dref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _point, _fit
from test_gpu_glmm_binomial import _prior_kw
from test_gpu_glmm_link import _segment_sum
from test_gpu_glmm_ztnegbin import _largest

pytestmark = pytest.mark.gpu

FAMILIES = ['beta', 'negbin']
SHAPES = [(1, 1, 1, 1), (37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7)]
PARITY = [(s, 0.0) for s in SHAPES] + [((65, 5, 2, 3), 0.7), ((300, 17, 4, 7), 0.7)]
DEG = {(65, 5, 2, 3): 5}
SCALAR_PHI = {'beta': 7.5, 'negbin': 1.7}
IDENT = 1e-12


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _data(family, N, P, K, G):
    """(x, y, z, w, gid, o, phi0 (N), free, deg, bare) of a shape."""
    bare = (N, P, K, G) == (37, 3, 1, 5)
    if family == 'beta':
        x, y, z, w, gid, o, ph, free = beta_ref.problem(N, P, K, G, N + P + K, phi='vector' if N >= 130 else 7.5, zero_weights=(N == 300))
    else:
        x, y, z, w, gid, o, ph, free = bref.nb_problem(N, P, K, G, N + P + K, phi=1.7)
        if N >= 130:
            ph = np.exp(np.random.default_rng([N, 11]).uniform(np.log(0.5), np.log(1e3), size=N))
            ph[3], ph[4] = 0.5, 1e3
        if N == 300:
            w = w.copy()
            w[::5] = 0.0
    if bare:
        o = np.zeros(N)
        assert np.array_equal(z, np.ones((N, 1)))
    if N >= 130:
        assert ph.min() == 0.5 and ph.max() == 1e3
    return x, y, z, w, gid, o, ph, free, DEG.get((N, P, K, G), dref.GH_DEG), bare


def _model(vb, family, x, y, z, w, o, phi, gid, G, deg=dref.GH_DEG, K=None, hyp=HYP):
    par = _par(vb, x.shape[1], K if z is None else z.shape[1], G)
    cls = vb.BetaGLMMObjective if family == 'beta' else vb.NegBinomialGLMMObjective
    return par, cls(par, x, y, z, gid, G, phi, offset=o, weights=w, gh_deg=deg, **_prior_kw(hyp))


_cache = {}


def _case(vb, family, shape):
    key = (family,) + shape
    if key not in _cache:
        N, P, K, G = shape
        x, y, z, w, gid, o, ph, free, deg, bare = _data(family, N, P, K, G)
        par, fun = _model(vb, family, x, y, None if bare else z, w, None if bare else o, SCALAR_PHI[family] if bare else ph, gid, G, deg, K=K)
        _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, o=o, ph=ph, free=free, deg=deg, eta=_eta(free, P, K, G), par=par, fun=fun, bare=bare)
    return _cache[key]


def _fresh(vb, family, c, G, K):
    """A model of its own on the data of a case: the entries are called directly on its context."""
    bare = c['bare']
    return _model(vb, family, c['x'], c['y'], None if bare else c['z'], c['w'], None if bare else c['o'],
                  SCALAR_PHI[family] if bare else c['ph'], c['gid'], G, c['deg'], K=K)[1]


def _entry(fun, family):
    return fun.ctx.glmm_beta_dispersion_terms if family == 'beta' else fun.ctx.glmm_negbin_dispersion_terms


def _set_lam(fun, lam):
    fun.log_dispersion_par.set_vector(np.array([float(lam)]))


def _ref_args(c, G):
    return c['x'], c['y'], c['z'], c['w'], c['o'], c['ph'], c['gid'], G


# ---- A: the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape,lam', PARITY)
def test_reference_parity(vb, family, shape, lam):
    N, P, K, G = shape
    c = _case(vb, family, shape)
    fun, free, eta, deg = c['fun'], c['free'], c['eta'], c['deg']
    assert fun.log_dispersion_par is fun.hyper_pars['log_dispersion'] and fun.log_dispersion_par.get_vector().size == 1
    _set_lam(fun, lam)
    try:
        for point, is_free in ((free, True), (eta, False)):
            got = fun.dispersion_terms(point, is_free)
            want = dref.dispersion_terms(family, *_ref_args(c, G), point, lam, is_free, deg)
            e = [abs(got['d1'] - want['d1']) / want['scale'], abs(got['d2'] - want['d2']) / want['scale2'], rel_err(got['cross'], want['cross'])]
            print(family, shape, 'lambda', lam, 'free' if is_free else 'vector', 'd1, d2 over their scales, cross:', e,
                  'd1', want['d1'], 'scale', want['scale'])
            assert e[0] <= 1e-11 and e[1] <= 1e-11 and e[2] <= 1e-10
            ng = 2 * P + 4 * K
            assert np.all(got['cross'][2 * P:ng] == 0.0)                     # the mu and tau entries
            assert np.array_equal(np.exp(lam) * c['ph'] if lam else c['ph'], fun._phi)
        slope, curv, dth, Hf = dref.profile(family, *_ref_args(c, G), free, lam, HYP, deg)
        print(family, shape, 'lambda', lam, 'smallest eigenvalue of the reference free Hessian', float(np.min(np.linalg.eigvalsh(Hf))),
              'profile slope and curvature', slope, curv)
        assert np.min(np.linalg.eigvalsh(Hf)) > 0
        M = np.zeros((2, free.size))
        M[0, 0], M[1, free.size - 1] = 1.0, 1.0
        for on_device in (False, True):
            s = fun.dispersion_sensitivity(free, on_device=on_device)
            assert np.allclose(s, dth, rtol=1e-6, atol=1e-12 * np.max(np.abs(dth)))
            assert np.allclose(fun.dispersion_sensitivity(free, M, on_device=on_device), M @ dth, rtol=1e-6, atol=1e-12 * np.max(np.abs(dth)))
            ps, pc = fun.dispersion_profile(free, on_device=on_device)
            assert abs(ps - slope) <= 1e-11 * want['scale'] or abs(ps - slope) <= 1e-6 * abs(slope)
            assert abs(pc - curv) <= 1e-6 * abs(curv)
    finally:
        _set_lam(fun, 0.0)


# ---- B: the entries themselves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', SHAPES)
def test_entry_contract_and_host_identity(vb, family, shape):
    """Two calls at one point are bitwise equal; an empty group's local row is exactly zero; the outputs equal the host sum of the
    per-row `*_expected_h_dispersion` terms (the mirror of what the kernel forms per row) to 1e-12 of the largest magnitude."""
    from lrvb_amd.glmm_beta import beta_expected_h_dispersion
    from lrvb_amd.glmm_binomial import negbin_expected_h_dispersion
    N, P, K, G = shape
    c = _case(vb, family, shape)
    fun = _fresh(vb, family, c, G, K)
    x, y, z, w, gid, o, ph = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'ph'))
    pt = _point(c['eta'], P, K, G)
    gh = (fun.gh_x, fun.gh_w)
    entry = _entry(fun, family)
    a, b = entry(*pt, *gh), entry(*pt, *gh)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    d, cg, cl = a
    assert d.shape == (2,) and cg.shape == (2 * P,) and cl.shape == (G, 2 * K)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(cl[G - 1] == 0.0)         # the empty group keeps exact zeros
    m, v, e, r = pt
    rho, s = o + x @ m + np.sum(z * e[gid], axis=1), (x * x) @ v + np.sum(z * z * r[gid], axis=1)
    if family == 'beta':
        E = beta_expected_h_dispersion(rho, s, np.log(y) - np.log1p(-y), ph, *gh)
    else:
        E = negbin_expected_h_dispersion(rho, s, y, ph, *gh)
    d1, d2 = w * E[1], w * 0.5 * E[2]
    want_cl = np.hstack([_segment_sum(gid, G, d1[:, None] * z), _segment_sum(gid, G, d2[:, None] * z * z)])
    errs = [_largest(d, [np.sum(w * E[0]), np.sum(w * E[3])]), _largest(cg, np.concatenate([x.T @ d1, (x * x).T @ d2])), _largest(cl, want_cl)]
    print(family, shape, 'entry against the host forms', errs)
    assert max(errs) <= IDENT


@pytest.mark.parametrize('family', FAMILIES)
def test_weight_zero_rows_contribute_exact_zeros(vb, family):
    """(300, 17, 4, 7), every fifth weight zero: a second model whose zero-weight rows hold OTHER responses and dispersions gives
    the same bits -- w x = 0 exactly for every finite x, and adding a zero changes no sum."""
    shape = (300, 17, 4, 7)
    N, P, K, G = shape
    c = _case(vb, family, shape)
    zero = c['w'] == 0.0
    assert zero.sum() == 60
    y2, ph2 = c['y'].copy(), c['ph'].copy()
    y2[zero] = 0.37 if family == 'beta' else 11.0
    ph2[zero] = 3.3
    A = _fresh(vb, family, c, G, K)
    B = _model(vb, family, c['x'], y2, c['z'], c['w'], c['o'], ph2, c['gid'], G, c['deg'])[1]
    pt = _point(c['eta'], P, K, G)
    a, b = _entry(A, family)(*pt, A.gh_x, A.gh_w), _entry(B, family)(*pt, B.gh_x, B.gh_w)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    w1 = np.where(zero, 1.0, c['w'])                                         # and with a weight there the rows do count
    C = _model(vb, family, c['x'], c['y'], c['z'], w1, c['o'], c['ph'], c['gid'], G, c['deg'])[1]
    assert not np.array_equal(_entry(C, family)(*pt, C.gh_x, C.gh_w)[1], a[1])


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('shape', [(65, 5, 2, 3), (300, 17, 4, 7)])
def test_finite_differences_of_the_device(vb, family, shape):
    """(F(theta, lambda + delta) - F(theta, lambda - delta)) / (2 delta) of the device's own F = value - log_norm_const() against d1,
    delta = 1e-4, 1e-6 relative: a reference and a kernel that shared one mistake would still miss this."""
    N, P, K, G = shape
    c = _case(vb, family, shape)
    fun, free = c['fun'], c['free']
    delta = 1e-4
    F = {}
    try:
        for lam in (delta, -delta, 0.0):
            _set_lam(fun, lam)
            F[lam] = fun.value(free) - fun.log_norm_const()
        t = fun.dispersion_terms(free)
    finally:
        _set_lam(fun, 0.0)
    fd1 = (F[delta] - F[-delta]) / (2.0 * delta)
    fd2 = (F[delta] - 2.0 * F[0.0] + F[-delta]) / delta ** 2
    print(family, shape, 'd1', t['d1'], 'central difference', fd1, 'd2', t['d2'], 'second difference', fd2)
    assert abs(fd1 - t['d1']) <= 1e-6 * abs(t['d1'])


# ---- C: state and side effects -------------------------------------------------------------------------------------------------
def _everything(fun, free, n1):
    p = fun.predict(free, n0=1, n1=n1)
    return [np.array([fun.value(free)]), fun.grad(free), fun.hessian(free)] + [p[k] for k in sorted(p)]


@pytest.mark.parametrize('family', FAMILIES)
def test_lambda_zero_is_bitwise_the_untouched_model(vb, family):
    shape = (65, 5, 2, 3)
    N, P, K, G = shape
    c = _case(vb, family, shape)
    free = c['free']
    A, B = _fresh(vb, family, c, G, K), _fresh(vb, family, c, G, K)           # B never touches the new parameter
    base = _everything(B, free, N - 2)
    first = _everything(A, free, N - 2)
    assert all(np.array_equal(p, q) for p, q in zip(first, base))
    R = np.eye(free.size)[:, [0, free.size - 1]]
    sol = A.solve(free, R, on_device=True)
    key = A._dev_factor_key
    assert key is not None
    _set_lam(A, 0.7)
    moved = _everything(A, free, N - 2)
    assert A._dev_factor_key is None                                         # the resident factor went with the old phi
    assert not np.array_equal(moved[0], base[0]) and not np.array_equal(moved[2], base[2])      # the memos were not served
    assert np.array_equal(A._phi, np.exp(0.7) * c['ph'])
    assert not np.array_equal(A.solve(free, R, on_device=True), sol)
    _set_lam(A, 0.0)
    back = _everything(A, free, N - 2)
    assert all(np.array_equal(p, q) for p, q in zip(back, base))             # and back: the first values bitwise
    assert np.array_equal(A.solve(free, R, on_device=True), sol)
    assert np.array_equal(A._phi, c['ph'])


def test_negbin_results_are_bitwise_unchanged_by_set_dispersion(vb):
    """The binomial entries never read the dispersion buffer: the NB2 class now fills it, and nothing of what it computed before moves."""
    shape = (130, 64, 4, 2)
    N, P, K, G = shape
    c = _case(vb, 'negbin', shape)
    fun = _fresh(vb, 'negbin', c, G, K)
    ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
    pt = _point(c['eta'], P, K, G)
    A = np.random.default_rng(2).normal(size=(3, 2 * P + 2 * G * K))
    both = lambda: (ctx.glmm_binomial_terms(*pt, *gh), ctx.glmm_binomial_obs_influence(*pt, *gh, A), ctx.glmm_binomial_group_influence(*pt, *gh, A))
    same = lambda p, q: (p[0][0] == q[0][0] and all(np.array_equal(u, v) for u, v in zip(p[0][1:], q[0][1:]))
                         and np.array_equal(p[1], q[1]) and np.array_equal(p[2], q[2]))
    base = both()
    first = ctx.glmm_negbin_dispersion_terms(*pt, *gh)                       # the class itself has filled the buffer
    for disp in (None, np.full(N, 3.0), c['ph'][::-1].copy(), c['ph']):
        ctx.set_dispersion(disp)
        assert same(both(), base)
    assert all(np.array_equal(p, q) for p, q in zip(ctx.glmm_negbin_dispersion_terms(*pt, *gh), first))     # with phi0 back, the same bits
    # and a plain binomial model that never set one
    par = _par(vb, P, K, G)
    bino = vb.BinomialGLMMObjective(par, c['x'], c['y'], c['z'], c['gid'], G, trials=c['y'] + c['ph'], offset=c['o'] - np.log(c['ph']),
                                    weights=c['w'], **_prior_kw(HYP))
    assert same((bino.ctx.glmm_binomial_terms(*pt, *gh), bino.ctx.glmm_binomial_obs_influence(*pt, *gh, A),
                 bino.ctx.glmm_binomial_group_influence(*pt, *gh, A)), base)


@pytest.mark.parametrize('family', FAMILIES)
def test_entries_leave_the_resident_state_alone(vb, family):
    """After `dispersion_terms` a `solve(on_device=True)` rebuilds nothing and returns the same bits; on the context, the Schur entry
    still finds the group sums of the last terms entry."""
    shape = (65, 5, 2, 3)
    N, P, K, G = shape
    c = _case(vb, family, shape)
    fun, free = _fresh(vb, family, c, G, K), c['free']
    R = np.random.default_rng(4).normal(size=(free.size, 3))
    first = fun.solve(free, R, on_device=True)
    key = fun._dev_factor_key
    built = []
    orig = fun.global_hessian
    fun.global_hessian = lambda *a, **k: (built.append(1), orig(*a, **k))[1]
    t = fun.dispersion_terms(free)
    assert fun._dev_factor_key == key and key is not None
    again = fun.solve(free, R, on_device=True)
    assert built == [] and np.array_equal(first, again)
    assert np.array_equal(fun.dispersion_sensitivity(free, on_device=True), -fun.solve(free, t['cross'][:, None], on_device=True).ravel())
    assert built == []
    # on the context: group sums, then the new entry, then the Schur entry on the SAME sums
    hip = vb._hip
    other = _fresh(vb, family, c, G, K)
    ctx, gh = other.ctx, (other.gh_x, other.gh_w)
    pt = _point(c['eta'], P, K, G)
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3))
    M1, M2 = np.empty((2 * P + 3 * K, 2 * P + 3 * K)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda M: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    terms = ctx.glmm_beta_terms if family == 'beta' else ctx.glmm_binomial_terms
    terms(*pt, *gh)
    assert schur(M1) == hip.OK
    terms(*pt, *gh)
    _entry(other, family)(*pt, *gh)
    assert schur(M2) == hip.OK and np.array_equal(M1, M2)


# ---- D: refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', FAMILIES)
def test_refusals_by_error_code_and_text(vb, family):
    hip = vb._hip
    rng = np.random.default_rng(47)
    name = 'lrvb_glmm_beta_dispersion_terms' if family == 'beta' else 'lrvb_glmm_negbin_dispersion_terms'

    def context(N, P):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)) / np.sqrt(P))
        ctx.set_data(hip.SLOT_Y, rng.normal(size=N) if family == 'beta' else rng.poisson(3.0, size=N).astype(np.float64))
        ctx.set_trials(np.full(N, 5.5))
        ctx.set_dispersion(rng.uniform(0.5, 40.0, size=N))
        return ctx

    def call(ctx, P, G, K, nq=20, mean=None):
        Kc = min(max(K, 1), 5)
        m, v, e, rr = np.zeros(P) if mean is None else mean, np.ones(P), np.zeros(max(G * Kc, 1)), np.ones(max(G * Kc, 1))
        gx, gw = np.polynomial.hermite.hermgauss(min(nq, 128))
        gx, gw = np.resize(gx, nq), np.resize(gw, nq)
        d, cg, cl = np.empty(2), np.empty(2 * P), np.empty((max(G, 1), 2 * Kc))
        return getattr(ctx._lib, name)(ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, K, gx.ctypes.data,
                                       gw.ctypes.data, nq, d.ctypes.data, cg.ctypes.data, cl.ctypes.data)

    N, G, K = 20, 3, 2
    gid = np.arange(N) % G
    assert call(context(N, 65), 65, G, K) == hip.ERR_UNSUPPORTED              # P = 65
    ctx = context(N, 3)
    ctx.set_groups(gid, G)
    ctx.set_group_design(np.ones((N, K)))
    assert call(ctx, 3, G, 5) == hip.ERR_UNSUPPORTED                          # K = 5
    assert call(ctx, 3, G, 0) == hip.ERR_UNSUPPORTED                          # K = 0
    assert call(ctx, 3, G, K, nq=129) == hip.ERR_UNSUPPORTED                  # 129 nodes
    ctx.set_dispersion(np.ones(N + 1))
    assert call(ctx, 3, G, K) == hip.ERR_STATE                                # a dispersion of the wrong length
    ctx.set_dispersion(None)
    assert call(ctx, 3, G, K) == hip.ERR_STATE                                # no dispersion
    m, v, e, r = np.zeros(3), np.ones(3), np.zeros((G, K)), np.ones((G, K))
    gx, gw = np.polynomial.hermite.hermgauss(20)
    entry = ctx.glmm_beta_dispersion_terms if family == 'beta' else ctx.glmm_negbin_dispersion_terms
    with pytest.raises(Exception, match='no dispersion'):
        entry(m, v, e, r, gx, gw)
    ctx.set_dispersion(np.ones(N + 1))
    with pytest.raises(Exception, match='the dispersion has 21 entries'):
        entry(m, v, e, r, gx, gw)
    ctx.set_dispersion(np.full(N, 2.5))
    assert call(ctx, 3, G, K) == hip.OK
    assert call(ctx, 3, G, K, nq=128) == hip.OK and call(ctx, 3, G, K, nq=1) == hip.OK
    assert call(ctx, 3, G, K, mean=np.array([0.0, np.nan, 0.0])) == hip.ERR_INVALID      # a NaN point
    with pytest.raises(ValueError, match='not finite'):
        entry(np.array([0.0, np.nan, 0.0]), v, e, r, gx, gw)
    assert call(ctx, 3, G, K) == hip.OK                                       # and the context goes on working
    if family == 'negbin':
        ctx.set_link(1)
        assert call(ctx, 3, G, K) == hip.ERR_UNSUPPORTED                      # the NB2 term is the logit one
        ctx.set_link(0)
        ctx.set_trials(None)
        assert call(ctx, 3, G, K) == hip.ERR_STATE                            # no trials
    assert vb._hip.load().lrvb_version() == 1


@pytest.mark.parametrize('family', FAMILIES)
def test_global_routes_refuse_the_new_parameter(vb, family):
    c = _case(vb, family, (37, 3, 1, 5))
    fun, free = c['fun'], c['free']
    with pytest.raises(NotImplementedError, match='dispersion_sensitivity'):
        fun.global_sensitivity(fun.log_dispersion_par, free)
    with pytest.raises(NotImplementedError, match='dispersion_sensitivity'):
        fun.global_cross_hessian(fun.log_dispersion_par, free)
    C = fun.cross_hessian(fun.log_dispersion_par, free, True)
    assert C.shape == (free.size, 1) and np.array_equal(C[:, 0], fun.dispersion_terms(free)['cross'])
    g = fun.hyper_grad(fun.log_dispersion_par, free, True)
    assert g.shape == (1,) and abs(g[0] - (fun.dispersion_terms(free)['d1'] + fun.log_norm_const_dispersion()[0])) <= 1e-12 * abs(g[0])
    assert np.array_equal(fun.global_cross_hessian(fun.tau_prior_par, free), fun.cross_hessian(fun.tau_prior_par, free, True)[:fun.n_global])


# ---- E: sensitivity against refits, and the fit ------------------------------------------------------------------------------------
FIT_SHAPE = (2000, 4, 1, 30)
PHI_TRUE = {'beta': 20.0, 'negbin': 3.0}
FIT_SEED = {'beta': 7, 'negbin': 7}
FIT_HYP = (1.0, 0.0, 1.0, 1.0, 1.0)                                      # the priors `profile_optimum` of the reference ran with


def _fit_model(vb, family):
    N, P, K, G = FIT_SHAPE
    x, y, z, w, gid, o = dref.simulate(family, N, P, K, G, FIT_SEED[family], PHI_TRUE[family])
    par, fun = _model(vb, family, x, y, z, w, o, PHI_TRUE[family] / 4.0, gid, G, hyp=FIT_HYP)
    return par, fun, (x, y, z, w, gid, o)


@pytest.mark.parametrize('family', FAMILIES)
def test_sensitivity_against_refits(vb, family):
    """Refits at lambda = +-0.05: the moments of beta and mu predicted by `dispersion_sensitivity` (both routes) and by
    `ParametricSensitivityLinearApproximation` with the dense cross Hessian agree with the refit differences within the project's
    refit margin, 5 % of the largest change."""
    N, P, K, G = FIT_SHAPE
    par, fun, _ = _fit_model(vb, family)
    objective = vb.Objective(par, fun)
    D = 2 * P + 4 * K + 2 * G * K
    th = _fit(vb, objective, np.zeros(D))
    idx = np.concatenate([np.arange(P), 2 * P + np.arange(K)])               # the means of beta and mu
    M = np.eye(D)[idx]
    pred = [fun.dispersion_sensitivity(th, M, on_device=dev) for dev in (False, True)]
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.log_dispersion_par, th, np.zeros(1))
    pred.append((M @ lin.get_dinput_dhyper())[:, 0])
    h = 0.05
    _set_lam(fun, h)
    th_p = _fit(vb, objective, th + h * fun.dispersion_sensitivity(th))
    _set_lam(fun, -h)
    th_m = _fit(vb, objective, th - h * fun.dispersion_sensitivity(th))
    _set_lam(fun, 0.0)
    diff = 0.5 * (th_p - th_m)[idx]
    for p in pred:
        print(family, 'predicted against refit', np.max(np.abs(p * h - diff)), 'largest change', np.max(np.abs(diff)))
        assert np.max(np.abs(p * h - diff)) < 0.05 * np.max(np.abs(diff)) + 1e-8


@pytest.mark.parametrize('family', FAMILIES)
def test_fit_dispersion(vb, family):
    """From phi0 = phi_true / 4.  The reference's own profile optimum for these seeds, computed on the CPU
    (glmm_dispersion_reference.profile_optimum): see REFERENCE_OPTIMUM below; both lie inside the gross-error band."""
    N, P, K, G = FIT_SHAPE
    par, fun, _ = _fit_model(vb, family)
    objective = vb.Objective(par, fun)
    D = 2 * P + 4 * K + 2 * G * K
    out = fun.fit_dispersion(lambda f, start: _fit(vb, objective, start), np.zeros(D))
    lam, th = out['lam'], out['theta']
    t = fun.dispersion_terms(th)
    print(family, 'fit_dispersion', {k: out[k] for k in ('lam', 'phi_scale', 'slope', 'curvature', 'iterations')}, 'F_ll', t['d2'],
          'phi_hat', out['phi_scale'] * PHI_TRUE[family] / 4.0, 'reference optimum', REFERENCE_OPTIMUM[family])
    assert fun.log_dispersion == lam and out['iterations'] <= 20
    assert abs(out['slope']) < 1e-6 * (abs(t['d2']) + 1.0)
    assert out['curvature'] > 0
    F = lambda theta: fun.value(theta) - fun.log_norm_const()
    F_hat = F(th)
    dth = fun.dispersion_sensitivity(th)
    for step in (0.1, -0.1):
        _set_lam(fun, lam + step)
        assert F(_fit(vb, objective, th + step * dth)) > F_hat
    _set_lam(fun, lam)
    phi_hat = out['phi_scale'] * PHI_TRUE[family] / 4.0
    assert PHI_TRUE[family] / 2.0 <= phi_hat <= 2.0 * PHI_TRUE[family]        # a gross-error band, not a measurement
    # the reference's own optimum: either side stops its inner fits at a gradient of 1e-8 and its Newton iteration on lambda at a step
    # of 1e-8 or 1e-9, and the two objectives agree to 1e-11, so the two optima cannot be 1e-5 apart
    assert abs(lam - REFERENCE_OPTIMUM[family]) < 1e-5


# lambda-hat of the reference's own profile optimum for FIT_SEED, FIT_HYP and phi0 = phi_true / 4, computed once on the CPU by
# glmm_dispersion_reference.profile_optimum (dense reference Hessian, Newton to a step below 1e-9): phi-hat = 19.6604 for the
# simulated 20 (Beta) and 3.04997 for the simulated 3 (NB2), both inside [phi_true / 2, 2 phi_true]
REFERENCE_OPTIMUM = {'beta': 1.3691677420916015, 'negbin': 1.4028122483037813}

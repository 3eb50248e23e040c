"""`CensoredNormalGLMMObjective` on the GPU: the CensNormalLik and CensNormalDispLik instantiations of the shared
tile walk against the torch reference tests/glmm_censnormal_reference.py (observed rows on 96 Gauss-Hermite nodes, not the closed form;
censored rows through log_ndtr and nested autograd, not the inverse Mills ratio), the probit identity across models, the shift
identity, the all-observed closed form, the zero-variance known answer, the dispersion identities, predictions, streamed
influence, the state contract, the refusals, and the fits.

Error measure and bounds are those of tests/test_gpu_glmm_gamma.py: value 1e-11, gradient 1e-10, Hessian / products / Schur complement
1e-9 relative; LRVB covariance and solves rtol 1e-6 on both routes; influence rows 1e-9, group sums against the weighted rows 1e-10,
the dense cross Hessian 1e-9, quantities behind an H^-1 rtol 1e-6 with atol 1e-12; identities 1e-12 of the largest magnitude.

Shapes (N, P, K, G): (1, 1, 1, 1); (37, 3, 1, 5) with z=None, offset=None and a scalar phi; (65, 5, 2, 3) -- a second tile of one row,
a cut group and an empty group; (130, 64, 4, 2) -- groups cut by tile boundaries, P and K at their limits; (300, 17, 4, 7) with
every fifth weight zero.  phi = 2 (a scalar) at the first three, one value per row on [0.25, 16] (both ends present) at the last
two.  Every shape runs in three MODES: 'mixed' (about 30 % censored, left and right), 'observed' (censoring=None) and 'censored'
(every row, alternating sides).  Every data set lies inside the grid on which the reference meets its 1e-10 cap against mpmath
(asserted row by row on the CPU in tests/test_glmm_censnormal_host_math.py).  Its reference free Hessian is positive definite with a
condition number below 1e8: asserted here, in `test_reference_parity`, on all fifteen data sets, and on the CPU on eleven of them
(the two large shapes in their 'mixed' mode only); the fifteen values, 3e1 to 3e3, are tabulated in DESIGN.md section 45.  So the
covariance and solve checks run everywhere.

Probit identity.  On an all-censored data set with a scalar phi, r = sqrt(phi), the row term is -log Phi(delta r (t - y)).  The
binomial model B under the probit link with design (r x, r z), offset r (o - y), one trial and response 1[delta = +1] has, at the
SAME point, rho_B = r (rho - y) and s_B = r^2 s: its term is -log Phi(t_B) for a success and -log Phi(-t_B) for a failure -- the
same function.  With phi in {4, 0.25} every product with r is exact, so value, gradient (mean AND variance coordinates), the three
H blocks, every column of the group sums, the influence rows and the group influence are EQUAL to rounding."""
import numpy as np
import pytest
import torch

import glmm_censnormal_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _point, _fit
from test_gpu_glmm_binomial import _prior_kw, _check_against_reference, _same
from test_gpu_glmm_link import _moments, _segment_sum
from test_gpu_glmm_ztnegbin import _largest

pytestmark = pytest.mark.gpu

SHAPES = ref.SHAPES
MODES = ref.MODES
INFL_SHAPES = [(37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2)]
IDENT_SHAPES = [(130, 64, 4, 2), (300, 17, 4, 7)]
IDENT = 1e-12
assert HYP == ref.TEST_HYP                                               # the CPU preconditions were computed under these priors


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _model(vb, x, y, z, w, o, phi, st, gid, G, hyp=HYP, K=None, gh_deg=20):
    par = _par(vb, x.shape[1], K if z is None else z.shape[1], G)
    return par, vb.CensoredNormalGLMMObjective(par, x, y, z, gid, G, phi, censoring=st, offset=o, weights=w, gh_deg=gh_deg, **_prior_kw(hyp))


_cache = {}


def _case(vb, N, P, K, G, mode='mixed'):
    """The model at the point of `problem`, computed once per case and mode.  The bare shape is handed z=None, offset=None and the
    scalar phi; 'observed' is handed censoring=None."""
    key = (N, P, K, G, mode)
    if key not in _cache:
        x, y, z, w, gid, o, ph, st, free = ref.shape_data(N, P, K, G, mode)
        bare = (N, P, K, G) == ref.BARE
        par, fun = _model(vb, x, y, None if bare else z, w, None if bare else o, 2.0 if N < 130 else ph, None if mode == 'observed' else st, gid, G, K=K)
        _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, o=o, ph=ph, st=st, free=free, eta=_eta(free, P, K, G), par=par, fun=fun,
                           targs=ref.targs(x, y, z, w, o, ph, gid, G, st, HYP))
    return _cache[key]


def _fresh(vb, c, G, **kw):
    """A model of the case's data with a context of its own."""
    d = dict(c, **kw)
    return _model(vb, d['x'], d['y'], d['z'], d['w'], d['o'], d['ph'], d['st'], d['gid'], G, gh_deg=d.get('gh_deg', 20))[1]


def _hf(c):
    if 'Hf' not in c:
        c['Hf'] = ref.value_grad_hess(ref.kl_free, c['free'], c['targs'])[2]
    return c['Hf']


def _rho_s(c, pt):
    m, v, e, r = pt
    return c['o'] + c['x'] @ m + np.sum(c['z'] * e[c['gid']], axis=1), (c['x'] * c['x']) @ v + np.sum(c['z'] * c['z'] * r[c['gid']], axis=1)


def _gh(fun):
    return fun.gh_x, fun.gh_w


# ---- A: the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G, mode):
    c = _case(vb, N, P, K, G, mode)
    y, w, gid, ph, st, fun = c['y'], c['w'], c['gid'], c['ph'], c['st'], c['fun']
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2     # an empty group, one with more than half the rows
    if N == 300:
        assert np.sum(w == 0.0) == 60
    if mode == 'mixed' and N >= 30:
        assert 0.15 <= np.mean(st != 0) <= 0.45 and np.any(st == 1) and np.any(st == -1)
    assert np.array_equal(fun.censoring, st) and (mode != 'observed' or not np.any(st))
    _, Hf = _check_against_reference(c['par'], fun, ref.kl_vec, ref.kl_free, c['targs'], c['free'], G, K, solves=True)
    c['Hf'] = Hf
    ev = np.linalg.eigvalsh(Hf)
    print('reference free Hessian', (N, P, K, G), mode, 'smallest eigenvalue', float(ev[0]), 'largest', float(ev[-1]), 'condition {:.1e}'.format(float(ev[-1] / ev[0])))
    assert ev[0] > 0 and ev[-1] / ev[0] < 1e8
    lnc = ref.log_norm_const(ph, w, st)
    assert abs(fun.log_norm_const() - lnc) <= 1e-12 * abs(lnc) + 1e-9
    other = _fresh(vb, c, G)
    pt = _point(c['eta'], P, K, G) + _gh(other)
    assert _same(other.ctx.glmm_censnormal_terms(*pt), other.ctx.glmm_censnormal_terms(*pt))     # two evaluations, equal bits


# ---- B: identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('phi', [4.0, 0.25])
@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_probit_identity_across_models(vb, N, P, K, G, phi):
    """Module docstring: everything EQUALS the probit binomial model B on (r x, r z), offset r (o - y), response 1[delta = +1], at the
    point of `problem` and with every variance times 30.  This pins the new policy to a kernel that has golden files."""
    c = _case(vb, N, P, K, G, 'censored')
    x, y, z, w, gid, o, st = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'st'))
    r = np.sqrt(phi)
    assert r * r == phi and np.all(st != 0)
    A = _model(vb, x, y, z, w, o, phi, st, gid, G)[1]
    B = vb.BinomialGLMMObjective(_par(vb, P, K, G), r * x, (st == 1).astype(np.float64), r * z, gid, G, offset=r * (o - y), weights=w,
                                 link='probit', gh_deg=20, **_prior_kw(HYP))
    m, v, e, rr = _point(c['eta'], P, K, G)
    gh = _gh(A)
    Aop = np.random.default_rng(N).normal(size=(5, 2 * P + 2 * G * K))
    # B's columns are r times A's: an operand row for A's coordinates acts on B's gradient through the same numbers
    for widen in (1.0, 30.0):
        pt = (m, v * widen, e, rr * widen)
        ta, tb = A.ctx.glmm_censnormal_terms(*pt, *gh), B.ctx.glmm_binomial_terms(*pt, *gh)
        errs = [abs(tb[0] - ta[0]) / abs(ta[0])] + [_largest(ta[i], tb[i]) for i in (1, 2, 3)]
        print('probit identity', (N, P, K, G), 'phi', phi, 'variances x', widen, errs)
        assert max(errs) <= IDENT
        assert ta[3].shape == (G, 2 * K + K * (2 * K + 1) + 4 * K * P) and np.any(ta[2][1] != 0.0)
        ra, rb = A.ctx.glmm_censnormal_obs_influence(*pt, *gh, Aop), B.ctx.glmm_binomial_obs_influence(*pt, *gh, Aop)
        ga, gb = A.ctx.glmm_censnormal_group_influence(*pt, *gh, Aop), B.ctx.glmm_binomial_group_influence(*pt, *gh, Aop)
        errs = [_largest(ra, rb), _largest(ga, gb)]
        print('probit identity, influence', errs)
        assert max(errs) <= IDENT


@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_shift_identity(vb, N, P, K, G):
    """(y + c, o + c) gives the same value, gradient and Hessian, for c = 37.5 and -1e6 (y and o are multiples of 2^-20, so the
    shifted values are exact)."""
    c = _case(vb, N, P, K, G, 'mixed')
    A = _fresh(vb, c, G)
    pt = _point(c['eta'], P, K, G) + _gh(A)
    ta = A.ctx.glmm_censnormal_terms(*pt)
    for shift in (37.5, -1e6):
        ys, os_ = c['y'] + shift, c['o'] + shift
        assert np.array_equal(ys - shift, c['y']) and np.array_equal(os_ - shift, c['o'])
        S = _fresh(vb, c, G, y=ys, o=os_)
        ts = S.ctx.glmm_censnormal_terms(*pt)
        errs = [abs(ts[0] - ta[0]) / abs(ta[0])] + [_largest(ta[i], ts[i]) for i in (1, 2, 3)]
        d = [_largest(p, q) for p, q in zip(A.ctx.glmm_censnormal_dispersion_terms(*pt), S.ctx.glmm_censnormal_dispersion_terms(*pt))]
        print('shift identity', (N, P, K, G), shift, errs, d)
        assert max(errs + d) <= IDENT


def _dense_gaussian(c, pt):
    """The closed-form Gaussian data term computed densely on the host: value, gradient (2 P), H blocks (3 x P x P) and the first
    2 K group-sum columns."""
    x, z, w, gid, ph, y = (c[k] for k in ('x', 'z', 'w', 'gid', 'ph', 'y'))
    rho, s = _rho_s(c, pt)
    u = rho - y
    val = float(np.sum(w * 0.5 * ph * (u * u + s)))
    a1, a2 = w * ph * u, w * 0.5 * ph
    g = np.concatenate([x.T @ a1, (x * x).T @ a2])
    Hb = np.stack([x.T @ (x * (w * ph)[:, None]), np.zeros((x.shape[1],) * 2), np.zeros((x.shape[1],) * 2)])
    G, K = pt[2].shape
    loc = np.zeros((G, 2 * K))
    np.add.at(loc, gid, np.concatenate([z * a1[:, None], z * z * a2[:, None]], axis=1))
    return val, g, Hb, loc


@pytest.mark.parametrize('N,P,K,G', SHAPES[1:])
def test_all_observed_is_the_closed_form_and_ignores_the_nodes(vb, N, P, K, G):
    """censoring=None: the dense closed-form Gaussian answer to 1e-12 of the largest magnitude, and equal BITS with gh_deg 1 and 20."""
    c = _case(vb, N, P, K, G, 'observed')
    pt = _point(c['eta'], P, K, G)
    f20, f1 = _fresh(vb, c, G, st=None), _fresh(vb, c, G, st=None, gh_deg=1)
    t20, t1 = f20.ctx.glmm_censnormal_terms(*pt, *_gh(f20)), f1.ctx.glmm_censnormal_terms(*pt, *_gh(f1))
    assert f1.gh_x.size == 1 and _same(t20, t1)
    A = np.random.default_rng(N).normal(size=(5, 2 * P + 2 * G * K))
    assert np.array_equal(f20.ctx.glmm_censnormal_obs_influence(*pt, *_gh(f20), A), f1.ctx.glmm_censnormal_obs_influence(*pt, *_gh(f1), A))
    assert all(np.array_equal(p, q) for p, q in zip(f20.ctx.glmm_censnormal_dispersion_terms(*pt, *_gh(f20)), f1.ctx.glmm_censnormal_dispersion_terms(*pt, *_gh(f1))))
    assert np.array_equal(f20.hessian(c['free']), f1.hessian(c['free']))
    val, g, Hb, loc = _dense_gaussian(c, pt)
    errs = [abs(t20[0] - val) / abs(val), _largest(t20[1], g), _largest(t20[2], Hb), _largest(t20[3][:, :2 * K], loc)]
    print('all observed against the dense closed form', (N, P, K, G), errs)
    assert max(errs) <= IDENT
    assert np.all(t20[2][1:] == 0.0)                                     # E h''' = E h'''' = 0: exact zeros in the cross and variance blocks


@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (300, 17, 4, 7)])
def test_zero_variance_known_answer(vb, N, P, K, G):
    """At vanishing variances t = rho: value - log_norm_const - (prior and entropy terms of the reference) = -sum w log p with
    scipy's norm.logpdf on observed rows, logsf on right-censored and logcdf on left-censored ones."""
    from scipy.stats import norm
    c = _case(vb, N, P, K, G, 'mixed')
    y, w, ph, st = (c[k] for k in ('y', 'w', 'ph', 'st'))
    eta = c['eta'].copy()
    ng, GK = 2 * P + 4 * K, G * K
    eta[P:2 * P] = 1e30
    eta[ng + GK:] = 1e30
    fun = _fresh(vb, c, G)
    t = c['targs']
    priors = float(ref._priors(torch.tensor(eta), t[0], t[1], t[2], t[3], t[6], G, t[8]))
    rho, s = _rho_s(c, _point(eta, P, K, G))
    assert np.max(s) < 1e-28
    sd = 1.0 / np.sqrt(ph)
    lp = np.where(st == 0, norm.logpdf(y, rho, sd), np.where(st == 1, norm.logsf(y, rho, sd), norm.logcdf(y, rho, sd)))
    want = -np.sum(w * lp)
    got = fun.value(eta, False) - fun.log_norm_const() - priors
    print('zero variance', (N, P, K, G), got, want, abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-11 * max(abs(want), abs(fun.log_norm_const()))


# ---- C: the dispersion ---------------------------------------------------------------------------------------------------------
def _set_lam(fun, lam):
    fun.log_dispersion_par.set_vector(np.array([lam]))


@pytest.mark.parametrize('N,P,K,G', SHAPES[1:])
def test_dispersion_terms_all_observed_are_the_data_term_and_its_gradient(vb, N, P, K, G):
    """An observed row is linear in phi: d[0] = d[1] = the data-term value and the cross Hessian = the data-term gradient, to 1e-12
    of the largest magnitude -- the rows kernel against the dispersion kernel, two different kernels.  The entry leaves the resident
    sums alone and is bitwise reproducible."""
    c = _case(vb, N, P, K, G, 'observed')
    fun = _fresh(vb, c, G)
    pt = _point(c['eta'], P, K, G) + _gh(fun)
    val, g, Hb, gs = fun.ctx.glmm_censnormal_terms(*pt)
    d, cg, cl = fun.ctx.glmm_censnormal_dispersion_terms(*pt)
    errs = [abs(d[0] - val) / abs(val), abs(d[1] - val) / abs(val), _largest(cg, g), _largest(cl, gs[:, :2 * K])]
    print('dispersion identity', (N, P, K, G), errs)
    assert max(errs) <= IDENT
    assert cl.shape == (G, 2 * K) and (G < 3 or np.all(cl[G - 1] == 0.0))
    a, b = fun.ctx.glmm_censnormal_dispersion_terms(*pt), fun.ctx.glmm_censnormal_dispersion_terms(*pt)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert _same(fun.ctx.glmm_censnormal_terms(*pt), (val, g, Hb, gs))


@pytest.mark.parametrize('mode', ['mixed', 'censored'])
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_dispersion_terms_against_the_reference_autograd(vb, N, P, K, G, mode):
    """F_lambda and F_lambda,lambda at the value bound 1e-11 (relative to |value| + |log_norm_const|) and the cross Hessian at the
    gradient bound 1e-10, against the reference differentiated in lambda by autograd."""
    c = _case(vb, N, P, K, G, mode)
    fun = c['fun']
    t = fun.dispersion_terms(c['free'])
    d1, d2, cross = ref.dispersion_terms(c['free'], c['targs'])
    scale = abs(fun.value(c['free'])) + abs(fun.log_norm_const()) + 1.0
    errs = [abs(t['d1'] - d1) / scale, abs(t['d2'] - d2) / scale, rel_err(t['cross'], cross)]
    print('dispersion terms against autograd', (N, P, K, G), mode, errs)
    assert errs[0] <= 1e-11 and errs[1] <= 1e-11 and errs[2] <= 1e-10
    hyp = fun.hyper_grad(fun.log_dispersion_par, c['free'], True)
    assert abs(hyp[0] - (t['d1'] + fun.log_norm_const_dispersion()[0])) <= 1e-13 * scale


def _everything(fun, free, n1):
    p = fun.predict(free, n0=1, n1=n1)
    return [np.array([fun.value(free)]), fun.grad(free), fun.hessian(free)] + [p[k] for k in sorted(p)]


def test_lambda_zero_is_bitwise_and_log_four_is_a_fresh_model(vb):
    """lambda = 0 is bit for bit the fixed-phi result; after lambda = log 4 the results equal those of a model built with 4 phi0
    (e^{log 4} phi0 and 4 phi0 differ by an ulp, which the inverse behind var_lrvb multiplies by the condition number of this
    shape: 1e-11 of the largest magnitude, the bound of the Gamma test), and back at 0 the first values return bitwise."""
    N, P, K, G = 65, 5, 2, 3
    c = _case(vb, N, P, K, G, 'mixed')
    free = c['free']
    A, B = _fresh(vb, c, G), _fresh(vb, c, G)
    base = _everything(B, free, N - 2)
    first = _everything(A, free, N - 2)
    assert all(np.array_equal(p, q) for p, q in zip(first, base))
    R = np.eye(free.size)[:, [0, free.size - 1]]
    sol = A.solve(free, R, on_device=True)
    assert A._dev_factor_key is not None
    _set_lam(A, np.log(4.0))
    moved = _everything(A, free, N - 2)
    assert A._dev_factor_key is None and not np.array_equal(moved[0], base[0])
    four = _fresh(vb, c, G, ph=4.0 * c['ph'])
    want = _everything(four, free, N - 2)
    errs = [_largest(p, q) for p, q in zip(moved, want)]
    print('lambda = log 4 against a model built with 4 phi0', errs)
    assert max(errs) <= 1e-11
    assert abs((A.log_norm_const() - four.log_norm_const()) / four.log_norm_const()) <= 1e-13
    _set_lam(A, 0.0)
    back = _everything(A, free, N - 2)
    assert all(np.array_equal(p, q) for p, q in zip(back, base))
    assert np.array_equal(A.solve(free, R, on_device=True), sol) and np.array_equal(A._phi, c['ph'])


FIT_SHAPE, PHI_TRUE, BETA_TRUE = (2000, 3, 1, 40), 4.0, np.array([1.0, -0.7, 0.4])


def _simulate(seed=3):
    """About 30 % right-censoring: the censoring point is an independent normal draw, and the row is censored where the latent value
    lies above it."""
    N, P, K, G = FIT_SHAPE
    rng = np.random.default_rng([seed, 45])
    x = rng.normal(size=(N, P))
    z = np.ones((N, 1))
    gid = rng.integers(0, G, size=N).astype(np.int32)
    t = 0.5 + x @ BETA_TRUE + (0.6 * rng.normal(size=(G, K)))[gid, 0]
    ystar = t + rng.normal(size=N) / np.sqrt(PHI_TRUE)
    cut = 0.5 + 1.1 + 1.4 * rng.normal(size=N)
    st = (ystar > cut).astype(np.int32)
    y = np.where(st == 1, cut, ystar)
    return x, y, z, np.ones(N), gid, np.zeros(N), st


def test_dispersion_sensitivity_against_refits_and_fit_dispersion(vb):
    """Simulated data at phi = 4 with about 30 % right-censoring, the model built with phi0 = phi / 4.  Refits at lambda = +-0.05: the
    moments of beta and mu predicted by `dispersion_sensitivity` (both routes) and by `ParametricSensitivityLinearApproximation`
    with `log_dispersion_par` agree with the refit differences within 5 % of the largest change.  Then `fit_dispersion` lands in
    [phi / 2, 2 phi], and beta_1 of the censored fit is closer to the truth than beta_1 of the fit that treats the censored rows as
    observed.  Both statements were confirmed on this seed with the CPU reference alone (L-BFGS on `kl_free`, no device): its figures
    are in DESIGN.md section 45."""
    N, P, K, G = FIT_SHAPE
    x, y, z, w, gid, o, st = _simulate()
    assert 0.2 <= np.mean(st) <= 0.4
    par, fun = _model(vb, x, y, z, w, o, PHI_TRUE / 4.0, st, gid, G)
    objective = vb.Objective(par, fun)
    D = 2 * P + 4 * K + 2 * G * K
    th = _fit(vb, objective, np.zeros(D))
    idx = np.concatenate([np.arange(P), 2 * P + np.arange(K)])
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
        print('predicted against refit', np.max(np.abs(p * h - diff)), 'largest change', np.max(np.abs(diff)))
        assert np.max(np.abs(p * h - diff)) < 0.05 * np.max(np.abs(diff)) + 1e-8
    out = fun.fit_dispersion(lambda f, start: _fit(vb, objective, start), th)
    phi_hat = out['phi_scale'] * PHI_TRUE / 4.0
    print('fit_dispersion', {k: out[k] for k in ('lam', 'phi_scale', 'slope', 'curvature', 'iterations')}, 'phi_hat', phi_hat)
    assert fun.log_dispersion == out['lam'] and out['iterations'] <= 20 and out['curvature'] > 0
    assert PHI_TRUE / 2.0 <= phi_hat <= 2.0 * PHI_TRUE
    b_cens = out['theta'][1]
    par_n, naive = _model(vb, x, y, z, w, o, PHI_TRUE / 4.0, None, gid, G)
    obj_n = vb.Objective(par_n, naive)
    out_n = naive.fit_dispersion(lambda f, start: _fit(vb, obj_n, start), _fit(vb, obj_n, np.zeros(D)))
    b_naive = out_n['theta'][1]
    print('beta_1: truth', BETA_TRUE[1], 'censored fit', b_cens, 'fit that ignores the censoring', b_naive)
    assert abs(b_cens - BETA_TRUE[1]) < abs(b_naive - BETA_TRUE[1])


def test_fit_covariance_and_tau_prior_sensitivity(vb):
    """The body and thresholds of tests/test_gpu_glmm_gamma.py::test_fit_covariance_and_tau_prior_sensitivity, on the simulated
    censored data at the true precision."""
    N, P, K, G = FIT_SHAPE
    x, y, z, w, gid, o, st = _simulate()
    par, fun = _model(vb, x, y, z, w, o, PHI_TRUE, st, gid, G)
    ng = 2 * P + 4 * K
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(ng + 2 * G * K))
    targs = ref.targs(x, y, z, w, o, np.full(N, PHI_TRUE), gid, G, st, HYP)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    print('reference gradient at the fit', np.max(np.abs(g_ad)))
    assert np.max(np.abs(g_ad)) < 1e-6 and np.min(np.linalg.eigvalsh(H_ad)) > 0
    Hinv = np.linalg.inv(H_ad)
    M = np.zeros((2, th.size))
    idx = [0, ng + (G * K) // 2]
    M[0, idx[0]], M[1, idx[1]] = 1.0, 1.0
    for on_device in (False, True):
        assert np.allclose(fun.lrvb_cov(th, M, on_device=on_device), Hinv[np.ix_(idx, idx)], rtol=1e-6, atol=1e-12)
    se_lr, se_mf = fun.ranef_se(th, on_device=True)
    assert np.allclose(se_lr.ravel(), np.sqrt(np.diag(Hinv)[ng + np.arange(G * K)]), rtol=1e-6, atol=0) and se_mf.shape == (G, K)
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


# ---- D: predictions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (130, 64, 4, 2)])
def test_predict_window_and_new_rows(vb, N, P, K, G):
    """Both routes; a window no tile boundary aligns with and new rows, some at the population level (group -1).  The mean is the
    latent one, rho, under both variances."""
    c = _case(vb, N, P, K, G, 'mixed')
    fun, free, x, z, gid = c['fun'], c['free'], c['x'], c['z'], c['gid']
    Hf = _hf(c)
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    Hinv = np.linalg.inv(Hf)
    rng = np.random.default_rng([N, 37])
    n_new = 70
    new = dict(x=rng.normal(size=(n_new, P)) / np.sqrt(P), z=np.concatenate([np.ones((n_new, 1)), 0.5 * rng.normal(size=(n_new, K - 1))], axis=1),
               groups=rng.integers(0, G, size=n_new), offset=0.3 * rng.normal(size=n_new))
    new['groups'][::9] = -1
    n0, n1 = 3, N - 2
    ng = 2 * P + 4 * K
    for what, kw, Cm, off in (('window', dict(n0=n0, n1=n1), _moments(x[n0:n1], z[n0:n1], gid[n0:n1], P, K, G), c['o'][n0:n1]),
                              ('new rows', dict(newdata=new), _moments(new['x'], new['z'], new['groups'], P, K, G), new['offset'])):
        want_var = np.einsum('nd,de,ne->n', Cm, Hinv, Cm)
        want_rho = off + Cm @ free
        outs = [fun.predict(free, on_device=dev, **kw) for dev in (False, True)]
        for route, out in zip(('host', 'device'), outs):
            assert np.allclose(out['rho'], want_rho, rtol=1e-12, atol=1e-12)
            assert np.allclose(out['var_lrvb'], want_var, rtol=1e-6, atol=0)
            assert np.array_equal(out['mean_mf'], out['rho']) and np.array_equal(out['mean_lrvb'], out['rho'])
        assert np.allclose(outs[1]['var_lrvb'], outs[0]['var_lrvb'], rtol=1e-6, atol=0)
    full = fun.predict(free, on_device=True)
    win = fun.predict(free, n0=n0, n1=n1, on_device=True)
    assert all(np.array_equal(win[k], full[k][n0:n1]) for k in full)
    with_phi = fun.predict(free, newdata=dict(new, dispersion=np.full(n_new, 3.0)), on_device=True)
    without = fun.predict(free, newdata=new, on_device=True)
    assert all(np.array_equal(with_phi[k], without[k]) for k in without)
    for key, val in (('trials', np.ones(n_new)), ('censoring', np.zeros(n_new))):
        with pytest.raises(ValueError, match='got {}'.format(key)):
            fun.predict(free, newdata=dict(new, **{key: val}))
    # group_cov and ranef_se on both routes against the dense inverse
    for dev in (False, True):
        se_lr, se_mf = fun.ranef_se(free, on_device=dev)
        assert np.allclose(se_lr.ravel(), np.sqrt(np.diag(Hinv)[ng + np.arange(G * K)]), rtol=1e-6, atol=0) and se_mf.shape == (G, K)
        cb, cu, cbu = fun.group_cov(free, on_device=dev)
        ie = ng + np.arange(G * K).reshape(G, K)
        assert np.allclose(cb, Hinv[:P, :P], rtol=1e-6, atol=1e-12)
        assert cu.shape == (G, K, K) and np.allclose(cu, Hinv[ie[:, :, None], ie[:, None, :]], rtol=1e-6, atol=1e-12)
        assert cbu.shape == (G, P, K) and np.allclose(cbu, Hinv[np.arange(P)[None, :, None], ie[:, None, :]], rtol=1e-6, atol=1e-12)


# ---- E: influence ------------------------------------------------------------------------------------------------------------
_infl = {}


def _infl_case(vb, N, P, K, G):
    """The dense reference of tests/test_gpu_glmm_link.py::_infl_case, computed once."""
    key = (N, P, K, G)
    if key in _infl:
        return _infl[key]
    c = _case(vb, N, P, K, G, 'mixed')
    t, free, eta = c['targs'], c['free'], c['eta']
    ng, GK = 2 * P + 4 * K, G * K
    p = torch.tensor(np.concatenate([eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + GK], 1.0 / eta[ng + GK:]]), requires_grad=True)
    wt = t[3].clone().requires_grad_(True)
    et = torch.cat([p[:P], 1.0 / p[P:2 * P], torch.tensor(eta[2 * P:ng]), p[2 * P:2 * P + GK], 1.0 / p[2 * P + GK:]])
    g, = torch.autograd.grad(ref.kl_vec(et, t[0], t[1], t[2], wt, *t[4:]), p, create_graph=True)
    rows_mv = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())], axis=1)
    wt2 = t[3].clone().requires_grad_(True)
    q = torch.tensor(free).requires_grad_(True)
    gf, = torch.autograd.grad(ref.kl_free(q, t[0], t[1], t[2], wt2, *t[4:]), q, create_graph=True)
    Cw = np.stack([torch.autograd.grad(gf[k], wt2, retain_graph=True)[0].numpy() for k in range(gf.numel())])
    Hf = _hf(c)
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    _infl[key] = dict(c, rows_mv=rows_mv, Cw=Cw, Hf=Hf)
    return _infl[key]


@pytest.mark.parametrize('N,P,K,G', INFL_SHAPES)
def test_influence_rows_windows_and_group_sums_against_autograd(vb, N, P, K, G):
    c = _infl_case(vb, N, P, K, G)
    fun, w, gid = c['fun'], c['w'], c['gid']
    pt = _point(c['eta'], P, K, G) + _gh(fun)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want = c['rows_mv'] @ A.T
    for Q in (5, 21):                                                    # 21 crosses the 16-column MFMA block
        got = fun.ctx.glmm_censnormal_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        win = fun.ctx.glmm_censnormal_obs_influence(*pt, A[:Q], n0=3, n1=N - 2)
        assert win.shape == (N - 5, Q) and np.array_equal(win, got[3:N - 2])
    rows = fun.ctx.glmm_censnormal_obs_influence(*pt, A)
    a, b = fun.ctx.glmm_censnormal_group_influence(*pt, A), fun.ctx.glmm_censnormal_group_influence(*pt, A)
    e = rel_err(a, _segment_sum(gid, G, w[:, None] * rows))
    print('group sums', N, P, K, G, e)
    assert a.shape == (G, 21) and e < 1e-10
    assert rel_err(a, _segment_sum(gid, G, w[:, None] * want)) < 1e-9
    assert np.array_equal(a, b)
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)


@pytest.mark.parametrize('N,P,K,G', INFL_SHAPES)
def test_influence_routes_stream_hyper_and_dense_cross_hessian(vb, N, P, K, G):
    c = _infl_case(vb, N, P, K, G)
    fun, par, free, w, gid = c['fun'], c['par'], c['free'], c['w'], c['gid']
    D = 2 * P + 4 * K + 2 * G * K
    want = -np.linalg.solve(c['Hf'], c['Cw']).T
    rows = fun.obs_influence(free, np.eye(D))
    print('arrow route', rel_err(rows, want))
    assert np.allclose(rows, want, rtol=1e-6, atol=1e-12)
    assert np.allclose(fun.obs_influence(free, np.eye(D), on_device=True), rows, rtol=1e-6, atol=1e-12)
    gi = fun.group_influence(free, np.eye(D))
    assert np.allclose(fun.group_influence(free, np.eye(D), on_device=True), gi, rtol=1e-6, atol=1e-12)
    assert np.allclose(gi, _segment_sum(gid, G, w[:, None] * want), rtol=1e-6, atol=1e-12)
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, free, w, stream_hyper=True)
    assert np.allclose(lin.get_doutput_dhyper_rows(np.eye(D)), want, rtol=1e-6, atol=1e-12)
    C = fun.cross_hessian(fun.weights_par, free, True)                   # the dense weight cross Hessian (small-N protocol)
    assert C.shape == (D, N) and rel_err(C, c['Cw']) < 1e-9
    sens = fun.global_sensitivity(fun.tau_prior_par, free)
    assert sens.shape[0] == 2 * P + 4 * K and np.all(np.isfinite(sens))


# ---- F: state and refusals -----------------------------------------------------------------------------------------------------
def test_state_contract(vb):
    """The new entries read neither lrvb_set_link nor lrvb_set_trials, leave the other likelihoods' entries alone; the status is read
    from the row's own entry; a missing dispersion or status is LRVB_ERR_STATE after which the context goes on working."""
    hip = vb._hip
    N, P, K, G = 130, 4, 2, 5
    x, y, z, w, gid, o, ph, st, free = ref.problem(N, P, K, G, 31, phi='vector', empty_group=False)
    pt = _point(_eta(free, P, K, G), P, K, G)
    _, fun = _model(vb, x, y, z, w, o, ph, st, gid, G)
    ctx = fun.ctx
    gh = np.polynomial.hermite.hermgauss(20)
    ptg = pt + gh
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G * K))
    cens = lambda: (ctx.glmm_censnormal_terms(*ptg), ctx.glmm_censnormal_obs_influence(*ptg, A, n0=3, n1=N - 2),
                    ctx.glmm_censnormal_group_influence(*ptg, A), ctx.glmm_censnormal_dispersion_terms(*ptg))
    same = lambda a, b: _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and all(np.array_equal(p, q) for p, q in zip(a[3], b[3]))
    base = cens()
    assert same(cens(), base)
    trials = np.random.default_rng(3).integers(1, 9, size=N).astype(np.float64)
    for link, tr in ((1, None), (2, trials), (0, trials), (0, None)):
        ctx.set_link(link)
        ctx.set_trials(tr)
        assert same(cens(), base)
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    ctx.glmm_censnormal_terms(*ptg)
    assert schur() == hip.OK
    M0 = M.copy()
    ctx.glmm_censnormal_dispersion_terms(*ptg)
    assert schur() == hip.OK and np.array_equal(M, M0)
    ctx.set_censoring(st)
    assert schur() == hip.ERR_STATE                                      # the setter drops the resident sums
    assert same(cens(), base)
    # the status is read from the row's ORIGINAL index: with a reversed status the value is the HOST sum over the rows in their
    # original order (value bound 1e-11), and not the host sum with the status taken in group-sorted order
    from lrvb_amd.glmm_censored import censnormal_expected_h
    rev_st = st[::-1].copy()
    assert not np.array_equal(rev_st, st)
    ctx.set_censoring(rev_st)
    moved = ctx.glmm_censnormal_terms(*ptg)
    assert not _same(moved, base[0])
    m_, v_, e_, r_ = pt
    rho = o + x @ m_ + np.sum(z * e_[gid], axis=1)
    s_ = (x * x) @ v_ + np.sum(z * z * r_[gid], axis=1)
    host = lambda status: float(np.sum(w * censnormal_expected_h(rho, s_, y, ph, status, *gh)[0]))
    want = host(rev_st)
    order = np.argsort(gid, kind='stable')
    by_sorted = np.empty(N, dtype=rev_st.dtype)
    by_sorted[order] = rev_st[:N]                                        # what a kernel reading the status at the sorted position would use
    print('status from the original index: value', moved[0], 'host', want, 'host with the status at the sorted position', host(by_sorted))
    assert abs(moved[0] - want) <= 1e-11 * abs(want) and abs(moved[0] - host(by_sorted)) > 1e-6 * abs(want)
    ctx.set_censoring(st)
    val = np.empty(1)
    raw = lambda: ctx._lib.lrvb_glmm_censnormal_terms(ctx._h, pt[0].ctypes.data, pt[1].ctypes.data, P, pt[2].ctypes.data, pt[3].ctypes.data, G, K,
                                                      gh[0].ctypes.data, gh[1].ctypes.data, 20, val.ctypes.data, None, None, None, 0)
    calls = (lambda: ctx.glmm_censnormal_terms(*ptg), lambda: ctx.glmm_censnormal_obs_influence(*ptg, A), lambda: ctx.glmm_censnormal_group_influence(*ptg, A),
             lambda: ctx.glmm_censnormal_dispersion_terms(*ptg))
    for clear, restore, none_text, len_text in (
            (ctx.set_dispersion, lambda: ctx.set_dispersion(ph), 'no dispersion: call lrvb_set_dispersion first', 'the dispersion has {} entries, the model has {} observations'),
            (ctx.set_censoring, lambda: ctx.set_censoring(st), 'no censoring status: call lrvb_set_censoring first', 'the censoring status has {} entries, the model has {} observations')):
        clear(None)
        assert raw() == hip.ERR_STATE
        for call in calls:
            with pytest.raises(Exception, match=none_text):
                call()
        clear(np.ones(N + 1))
        assert raw() == hip.ERR_STATE
        with pytest.raises(Exception, match=len_text.format(N + 1, N)):
            ctx.glmm_censnormal_terms(*ptg)
        restore()
        assert same(cens(), base)
    # a status other than -1, 0, +1 is refused at the setter, with the state left as it was
    bad = st.copy()
    bad[7] = 2
    with pytest.raises(ValueError, match=r'censoring\[7\] is 2: the status is -1 \(left-censored\), 0 \(observed\) or \+1 \(right-censored\)'):
        ctx.set_censoring(bad)
    assert same(cens(), base)
    # the other likelihoods' entries give the same bits before and after a call of the new ones
    ctx.set_trials(trials)
    others = lambda: (ctx.glmm_slopes_terms(*ptg), ctx.glmm_poisson_terms(*pt), ctx.glmm_binomial_terms(*ptg), ctx.glmm_beta_terms(*ptg),
                      ctx.glmm_gamma_terms(*pt))
    before = others()
    assert same(cens(), base)
    after = others()
    assert all(_same(a, b) for a, b in zip(after, before)) and all(not _same(b, base[0]) for b in before)
    assert vb._hip.load().lrvb_version() == 1


def test_refusals_by_error_code(vb):
    hip = vb._hip
    rng = np.random.default_rng(47)
    gh = np.polynomial.hermite.hermgauss(20)

    def context(N, P):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)) / np.sqrt(P))
        ctx.set_data(hip.SLOT_Y, rng.normal(size=N))
        ctx.set_dispersion(rng.uniform(0.5, 4.0, size=N))
        ctx.set_censoring(rng.integers(-1, 2, size=N))
        return ctx

    def call(ctx, P, G, K, kind, n0=0, n1=None, nq=20):
        Kc = min(max(K, 1), 5)
        m, v, e, rr = np.zeros(P), np.ones(P), np.zeros(max(G * Kc, 1)), np.ones(max(G * Kc, 1))
        gx, gw = np.zeros(max(nq, 20)), np.ones(max(nq, 20))
        gx[:20], gw[:20] = gh
        head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, K, gx.ctypes.data, gw.ctypes.data, nq)
        lib = ctx._lib
        n1 = ctx.n_obs if n1 is None else n1
        if kind == 'terms':
            val = np.empty(1)
            return lib.lrvb_glmm_censnormal_terms(*head, val.ctypes.data, None, None, None, 0)
        if kind == 'disp':
            d, cg, cl = np.empty(2), np.empty(2 * P), np.empty((max(G, 1), 2 * Kc))
            return lib.lrvb_glmm_censnormal_dispersion_terms(*head, d.ctypes.data, cg.ctypes.data, cl.ctypes.data)
        Q = 2
        Ag, Al = np.ones((Q, 2 * P)), np.ones((max(G, 1), 2 * Kc, Q))
        out = np.empty((5 * max(ctx.n_obs, G), Q))
        if kind == 'group':
            return lib.lrvb_glmm_censnormal_group_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, out.ctypes.data)
        return lib.lrvb_glmm_censnormal_obs_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, n0, n1, out.ctypes.data)

    N, G, K = 20, 3, 2
    gid = np.arange(N) % G
    for kind in ('terms', 'rows', 'group', 'disp'):
        wide = context(N, 65)
        assert call(wide, 65, G, K, kind) == hip.ERR_UNSUPPORTED         # P = 65
        ctx = context(N, 3)
        ctx.set_groups(gid, G)
        ctx.set_group_design(np.ones((N, K)))
        assert call(ctx, 3, G, 5, kind) == hip.ERR_UNSUPPORTED           # K = 5
        assert call(ctx, 3, G, 0, kind) == hip.ERR_UNSUPPORTED           # K = 0
        assert call(ctx, 3, G, K, kind, nq=129) == hip.ERR_UNSUPPORTED   # more than 128 nodes
        ctx.set_offset(np.zeros(N + 1))
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # an offset of the wrong length
        ctx.set_offset(None)
        ctx.set_dispersion(np.ones(N + 1))
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # a dispersion of the wrong length
        ctx.set_dispersion(None)
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # no dispersion
        ctx.set_dispersion(np.full(N, 2.5))
        ctx.set_censoring(np.zeros(N + 1))
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # a status of the wrong length
        ctx.set_censoring(None)
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # no status
        ctx.set_censoring(np.arange(N) % 3 - 1)
        if kind == 'rows':
            assert call(ctx, 3, G, K, kind, n0=5, n1=4) == hip.ERR_INVALID and call(ctx, 3, G, K, kind, n1=N + 1) == hip.ERR_INVALID
        assert call(ctx, 3, G, K, kind) == hip.OK
    st2 = np.zeros(N, dtype=np.int32)
    st2[4] = 2
    assert ctx._lib.lrvb_set_censoring(ctx._h, st2.ctypes.data, N) == hip.ERR_INVALID
    assert call(ctx, 3, G, K, 'terms') == hip.OK                         # the state is left as it was
    wide = context(N, 65)
    with pytest.raises(Exception, match='the censored Gaussian mixed model needs P <= 64'):
        wide.glmm_censnormal_terms(np.zeros(65), np.ones(65), np.zeros((G, K)), np.ones((G, K)), *gh)
    with pytest.raises(Exception, match='1 to 4 random effects per group'):
        ctx.glmm_censnormal_terms(np.zeros(3), np.ones(3), np.zeros((G, 5)), np.ones((G, 5)), *gh)
    # the constructor
    x, z = np.ones((N, 2)), np.ones((N, K))
    for bad in (np.nan, np.inf, -np.inf):
        y = np.full(N, 0.4)
        y[5] = bad
        with pytest.raises(ValueError, match='y must be finite: 1 of 20 rows'):
            vb.CensoredNormalGLMMObjective(_par(vb, 2, K, G), x, y, z, gid, G, 2.0)
    with pytest.raises(ValueError, match='censoring must be None or 20 values'):
        vb.CensoredNormalGLMMObjective(_par(vb, 2, K, G), x, np.full(N, 0.4), z, gid, G, 2.0, censoring=st2)
    for phi in (0.0, -3.0, np.inf, np.ones(N + 1)):
        with pytest.raises(ValueError, match='dispersion'):
            vb.CensoredNormalGLMMObjective(_par(vb, 2, K, G), x, np.full(N, 0.4), z, gid, G, phi)


def test_extreme_points(vb):
    """P = 1 with x = 1.  A mean of 1e200 puts rho = 1e200 on every row: phi (rho - y)^2 overflows on the observed rows (and a^2 / 2 on
    the left-censored ones), the point is refused with a ValueError that names the cause, and no sums stay resident; the context
    goes on working.  On right-censored rows alone the same point is legitimate: -log Phi(+huge) = 0 and every derivative is 0."""
    hip = vb._hip
    N, K, G = 70, 1, 3
    rng = np.random.default_rng(9)
    x = np.ones((N, 1))
    y, ph, w, o = rng.normal(size=N), np.exp(rng.uniform(np.log(0.25), np.log(16.0), size=N)), rng.uniform(0.5, 1.5, size=N), rng.normal(size=N)
    gid = (np.arange(N) % G).astype(np.int32)
    st = (np.arange(N) % 3 - 1).astype(np.int32)
    v, e, r = np.array([0.5]), np.zeros((G, K)), np.full((G, K), 0.7)
    _, fun = _model(vb, x, y, None, w, o, ph, st, gid, G, K=K)
    ctx = fun.ctx
    gh = _gh(fun)
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 + 3 * K, 2 + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    good = (np.array([0.3]), v, e, r)
    base = ctx.glmm_censnormal_terms(*good, *gh)
    assert np.isfinite(base[0]) and schur() == hip.OK
    for m in (1e200, -1e200):
        with pytest.raises(ValueError, match='censored Gaussian data term is not finite.*overflows'):
            ctx.glmm_censnormal_terms(np.array([m]), v, e, r, *gh)
        assert schur() == hip.ERR_STATE                                  # no sums left resident
        with pytest.raises(ValueError, match='not finite'):
            ctx.glmm_censnormal_dispersion_terms(np.array([m]), v, e, r, *gh)
        assert _same(ctx.glmm_censnormal_terms(*good, *gh), base) and schur() == hip.OK
    _, right = _model(vb, x, y, None, w, o, ph, np.ones(N, dtype=np.int32), gid, G, K=K)
    val, gg, Hb, gs = right.ctx.glmm_censnormal_terms(np.array([1e200]), v, e, r, *gh)
    assert val == 0.0 and np.all(gg == 0.0) and np.all(Hb == 0.0) and np.all(gs == 0.0)

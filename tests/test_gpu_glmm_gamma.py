"""`GammaGLMMObjective` and `HurdleGammaGLMM` on the GPU: the GammaLik and GammaDispLik instantiations of the
shared tile walk against the torch reference tests/glmm_gamma_reference.py (96-node Gauss-Hermite, not the closed form), the Poisson
and the scale identity across models, the dispersion identities, predictions, streamed influence, the state contract, the refusals,
extreme points, the two-part composite and the fits.

Error measure and bounds are those of tests/test_gpu_glmm_ztnegbin.py: value 1e-11, gradient 1e-10, Hessian / products / Schur
complement 1e-9 relative; LRVB covariance and solves rtol 1e-6; influence rows 1e-9, group sums against the weighted rows 1e-10,
the dense cross Hessian 1e-9, quantities behind an H^-1 rtol 1e-6 with atol 1e-12; identities 1e-12 of the largest magnitude.

Shapes (N, P, K, G): (1, 1, 1, 1); (37, 3, 1, 5) with z=None, offset=None and a scalar phi; (65, 5, 2, 3) -- a second tile of one row,
a cut group and an empty group; (130, 64, 4, 2); (300, 17, 4, 7) with every fifth weight zero.  phi = 7.5 at the first three, one
value per row on [0.05, 1e4] (both ends present) at the last two.  Every data set with N >= 4 holds the probe rows y[0] = 1e-12,
y[1] = 1e12 and y[2] = 1.

Two variants of every data set.  RAW: the probe rows as they are.  A row with y = 1e12 at a mean of order 1 has g = phi y / mu of
order 1e13: the reference free Hessian is positive definite (the data block is a sum of rank-one terms g c c^T) but its condition
number is 7e13 to 5e15 (smallest eigenvalues 0.248, 0.208, 0.282, 0.198 against largest 1.7e13 .. 1.4e15; computed on the CPU), so an
fp64 inverse of it -- the reference's own included -- carries no six digits and the covariance and solve checks CANNOT run there.
The RAW variant runs value, gradient, Hessian, products and Schur complement against the reference, and the identities.  CENTRED:
the same rows with the probes' log y added to their offsets (o[0] += log 1e-12, o[1] += log 1e12), which by the scale identity
makes them ordinary rows while log y - rho is still formed from two numbers of size 27.6; condition numbers 4e2 to 9e5 (smallest
eigenvalues 0.180, 0.248, 0.207, 0.282, 0.198, printed by the parity test and recorded in DESIGN.md section 43).  Every shape runs
the covariance and solve checks, the influence and the prediction tests on its CENTRED variant.  (37, 3, 1, 5) is handed
offset=None in its RAW variant and the two probe offsets in its CENTRED one.

Every s_n of these data sets is below 2.5 and every |rho_n| below 32; the reference meets its 1e-10 cap against mpmath for s up to
100 whatever rho (tests/test_glmm_gamma_host_math.py).

Poisson identity.  The Gamma row term is E h = g + phi rho, g = phi exp(log y - rho + s / 2), rho = o + x . m + z . e.  The Poisson
model B with design (-x, -z), offset log(phi y) - o and responses y_B = phi has, at the SAME point, rho_B = log(phi y) - rho and
s_B = s, so its row term exp(rho_B + s / 2) - y_B rho_B = g + phi rho - phi log(phi y): value_B = value - sum w phi log(phi y).  Its
coefficients are a1_B = g - phi = -a1, a2_B = a2, c11_B = c11, c12_B = +g / 2 = -c12, c22_B = c22: exactly the odd ones change
sign, and exactly the products with an odd number of design factors (a1 x, a1 z, c12 x (x o x), c12 z z^2, c12 z^2 x, c12 z x^2)
carry one more sign from the negated design, while c11 (-x)(-x), c11 (-z)(-x), a2 x^2, c22 .. keep theirs.  So the gradient (mean AND
variance coordinates), all three H blocks and EVERY column of the group sums are EQUAL between the two models."""
import numpy as np
import pytest
import torch

import glmm_gamma_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _point, _fit
from test_gpu_glmm_binomial import _prior_kw, _check_against_reference, _same
from test_gpu_glmm_link import _moments, _segment_sum
from test_gpu_glmm_ztnegbin import _largest

pytestmark = pytest.mark.gpu

SHAPES = ref.SHAPES
INFL_SHAPES = [(37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2)]
IDENT_SHAPES = [(130, 64, 4, 2), (300, 17, 4, 7)]
IDENT = 1e-12
LOG_PROBES = (np.log(ref.PROBES[0]), np.log(ref.PROBES[1]))
assert HYP == ref.TEST_HYP                                               # the CPU preconditions were computed under these priors


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _data(N, P, K, G, centred):
    """The draws of a shape: (x, y, z, w, gid, o, phi (N), free, bare) -- `bare`: the model is handed z=None and the scalar phi
    (the reference a column of ones and N equal values), and in the RAW variant offset=None (the reference zeros)."""
    bare = (N, P, K, G) == ref.BARE
    x, y, z, w, gid, o, ph, free = ref.shape_data(N, P, K, G, centred)
    return x, y, z, w, gid, o, ph, free, bare


def _model(vb, x, y, z, w, o, phi, gid, G, hyp=HYP, K=None):
    par = _par(vb, x.shape[1], K if z is None else z.shape[1], G)
    return par, vb.GammaGLMMObjective(par, x, y, z, gid, G, phi, offset=o, weights=w, **_prior_kw(hyp))


_cache = {}


def _case(vb, N, P, K, G, centred=True):
    """The model at the point of `problem`, computed once per case and variant."""
    key = (N, P, K, G, centred)
    if key not in _cache:
        x, y, z, w, gid, o, ph, free, bare = _data(N, P, K, G, centred)
        par, fun = _model(vb, x, y, None if bare else z, w, None if bare and not centred else o, 7.5 if bare else ph, gid, G, K=K)
        _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, o=o, ph=ph, free=free, eta=_eta(free, P, K, G), par=par, fun=fun,
                           targs=ref.targs(x, y, z, w, o, ph, gid, G, HYP))
    return _cache[key]


def _fresh(vb, c, G):
    """A model of the case's data with a context of its own."""
    return _model(vb, c['x'], c['y'], c['z'], c['w'], c['o'], c['ph'], c['gid'], G)[1]


def _hf(c):
    """The reference free Hessian of a case, computed once (the parity test leaves its own here)."""
    if 'Hf' not in c:
        c['Hf'] = ref.value_grad_hess(ref.kl_free, c['free'], c['targs'])[2]
    return c['Hf']


def _rho_s(c, pt):
    m, v, e, r = pt
    return c['o'] + c['x'] @ m + np.sum(c['z'] * e[c['gid']], axis=1), (c['x'] * c['x']) @ v + np.sum(c['z'] * c['z'] * r[c['gid']], axis=1)


# ---- A: the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('centred', [True, False])
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G, centred):
    if N < 4 and not centred:
        return                                                           # one row, no probes: the two variants are one
    c = _case(vb, N, P, K, G, centred)
    y, w, gid, ph = c['y'], c['w'], c['gid'], c['ph']
    assert np.all((y > 0.0) & np.isfinite(y))
    if N >= 4:
        assert (y[0], y[1], y[2]) == ref.PROBES
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2     # an empty group, one with more than half the rows
    if N == 300:
        assert np.sum(w == 0.0) == 60
    assert c['fun'].gh_x is None                                         # no quadrature anywhere in the model
    rho, s = _rho_s(c, _point(c['eta'], P, K, G))
    assert np.max(s) < 2.5 and np.max(np.abs(rho)) < 32.0                # where the reference meets its cap against mpmath
    _, Hf = _check_against_reference(c['par'], c['fun'], ref.kl_vec, ref.kl_free, c['targs'], c['free'], G, K, solves=centred)
    c['Hf'] = Hf
    ev = np.linalg.eigvalsh(Hf)
    print('reference free Hessian', (N, P, K, G), 'centred' if centred else 'raw', 'smallest eigenvalue', float(ev[0]), 'largest', float(ev[-1]),
          'covariance and solve checks', 'run' if centred else 'cannot run: condition {:.1e}'.format(float(ev[-1] / ev[0])))
    assert ev[0] > 0
    lnc = ref.log_norm_const(y, ph, w)
    assert abs(c['fun'].log_norm_const() - lnc) <= 1e-12 * abs(lnc) + 1e-9
    # two evaluations at one point are bitwise equal (through a model of its own: a direct call of the terms entry on a shared
    # context would drop the factor the class believes resident)
    other = _fresh(vb, c, G)
    pt = _point(c['eta'], P, K, G)
    assert _same(other.ctx.glmm_gamma_terms(*pt), other.ctx.glmm_gamma_terms(*pt))


# ---- B: identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_poisson_identity_across_models(vb, N, P, K, G):
    """Module docstring: gradient, H blocks and group sums EQUAL those of the Poisson model B, value_B = value - sum w phi log(phi y).
    The RAW variant (the probe rows at full size), at the point of `problem` and with every variance times 30."""
    c = _case(vb, N, P, K, G, centred=False)
    x, y, z, w, gid, o, ph = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'ph'))
    lpy = np.log(ph) + np.log(y)
    par_b = _par(vb, P, K, G)
    B = vb.PoissonGLMMObjective(par_b, -x, ph, -z, gid, G, offset=lpy - o, weights=w, **_prior_kw(HYP))
    A = _fresh(vb, c, G)
    m, v, e, r = _point(c['eta'], P, K, G)
    shift = float(np.sum(w * ph * lpy))
    for widen in (1.0, 30.0):
        pt = (m, v * widen, e, r * widen)
        ta, tb = A.ctx.glmm_gamma_terms(*pt), B.ctx.glmm_poisson_terms(*pt)
        big = max(abs(ta[0]), abs(shift))
        errs = [abs(tb[0] - (ta[0] - shift)) / big] + [_largest(ta[i], tb[i]) for i in (1, 2, 3)]
        print('Poisson identity', (N, P, K, G), 'variances x', widen, errs)
        assert max(errs) <= IDENT
        assert ta[3].shape == (G, 2 * K + K * (2 * K + 1) + 4 * K * P) and np.any(ta[2][1] != 0.0)
        # and the influence rows: a1' x and a1' z carry both signs, a2' neither
        Aop = np.random.default_rng(N).normal(size=(5, 2 * P + 2 * G * K))
        ra, rb = A.ctx.glmm_gamma_obs_influence(*pt, Aop), B.ctx.glmm_poisson_obs_influence(*pt, Aop)
        ga, gb = A.ctx.glmm_gamma_group_influence(*pt, Aop), B.ctx.glmm_poisson_group_influence(*pt, Aop)
        errs = [_largest(ra, rb), _largest(ga, gb)]
        print('Poisson identity, influence', errs)
        assert max(errs) <= IDENT


@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_scale_identity(vb, N, P, K, G):
    """The model (c y, o + log c) has the same gradient and Hessian, and its value - log_norm_const() is shifted by sum w log c."""
    c = _case(vb, N, P, K, G)
    x, y, z, w, gid, o, ph, eta = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'ph', 'eta'))
    A = _fresh(vb, c, G)
    for scale in (37.5, 1e-9):
        _, S = _model(vb, x, scale * y, z, w, o + np.log(scale), ph, gid, G)
        pt = _point(eta, P, K, G)
        ta, ts = A.ctx.glmm_gamma_terms(*pt), S.ctx.glmm_gamma_terms(*pt)
        errs = [_largest(ta[i], ts[i]) for i in (1, 2, 3)]
        fa, fs = A.value(eta, False) - A.log_norm_const(), S.value(eta, False) - S.log_norm_const()
        shift = float(np.sum(w) * np.log(scale))
        big = max(abs(A.value(eta, False)), abs(A.log_norm_const()), abs(shift))
        errs.append(abs(fs - (fa + shift)) / big)
        print('scale identity', (N, P, K, G), scale, errs)
        assert max(errs) <= IDENT


@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (300, 17, 4, 7)])
def test_zero_variance_known_answer(vb, N, P, K, G):
    """At vanishing variances t = rho: value - log_norm_const - (prior and entropy terms of the reference) = -sum w log Gamma(y)
    with scipy's density at shape phi and scale mu / phi.  The variances are 1e-30 (free coordinates are logs of the precisions)."""
    from scipy.stats import gamma as gamma_dist
    c = _case(vb, N, P, K, G)
    x, y, z, w, gid, o, ph = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'ph'))
    eta = c['eta'].copy()
    ng, GK = 2 * P + 4 * K, G * K
    eta[P:2 * P] = 1e30
    eta[ng + GK:] = 1e30
    fun = _fresh(vb, c, G)
    t = c['targs']
    priors = float(ref._priors(torch.tensor(eta), t[0], t[1], t[2], t[3], t[6], G, t[8]))
    rho, s = _rho_s(c, _point(eta, P, K, G))
    assert np.max(s) < 1e-28
    want = -np.sum(w * gamma_dist.logpdf(y, a=ph, scale=np.exp(rho) / ph))
    got = fun.value(eta, False) - fun.log_norm_const() - priors
    print('zero variance', (N, P, K, G), got, want, abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-11 * max(abs(want), abs(fun.log_norm_const()))


# ---- C: the dispersion ---------------------------------------------------------------------------------------------------------
def _set_lam(fun, lam):
    fun.log_dispersion_par.set_vector(np.array([lam]))


@pytest.mark.parametrize('N,P,K,G', SHAPES[1:])
def test_dispersion_terms_are_the_data_term_and_its_gradient(vb, N, P, K, G):
    """h is linear in phi: d[0] = d[1] = the data-term value and the cross Hessian = the data-term gradient, to 1e-12 of the largest
    magnitude -- the rows kernel against the dispersion kernel, two different kernels.  Both variants; and the entry leaves the
    resident sums alone."""
    for centred in (True, False):
        c = _case(vb, N, P, K, G, centred)
        fun = _fresh(vb, c, G)
        pt = _point(c['eta'], P, K, G)
        val, g, Hb, gs = fun.ctx.glmm_gamma_terms(*pt)
        d, cg, cl = fun.ctx.glmm_gamma_dispersion_terms(*pt)
        errs = [abs(d[0] - val) / abs(val), abs(d[1] - val) / abs(val), _largest(cg, g), _largest(cl, gs[:, :2 * K])]
        print('dispersion identity', (N, P, K, G), 'centred' if centred else 'raw', errs)
        assert max(errs) <= IDENT
        assert cl.shape == (G, 2 * K) and (G < 3 or np.all(cl[G - 1] == 0.0))
        a, b = fun.ctx.glmm_gamma_dispersion_terms(*pt), fun.ctx.glmm_gamma_dispersion_terms(*pt)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))           # bitwise reproducible
        assert _same(fun.ctx.glmm_gamma_terms(*pt), (val, g, Hb, gs))
    # F_lambda and F_lambda,lambda of the class against the host forms, and a central difference of F in lambda
    c = _case(vb, N, P, K, G)
    fun = _fresh(vb, c, G)
    t = fun.dispersion_terms(c['free'])
    F = lambda: fun.value(c['free']) - fun.log_norm_const()
    h = 1e-4
    _set_lam(fun, h)
    Fp = F()
    _set_lam(fun, -h)
    Fm = F()
    _set_lam(fun, 0.0)
    F0 = F()
    fd1, fd2 = (Fp - Fm) / (2 * h), (Fp - 2 * F0 + Fm) / (h * h)
    print('F_lambda', t['d1'], fd1, 'F_lambda,lambda', t['d2'], fd2)
    # central differences of a function of size `scale`: rounding 1e-15 scale / h (/ h^2), truncation h^2 times a derivative of that size
    scale = abs(fun.value(c['free'])) + abs(fun.log_norm_const())
    assert abs(t['d1'] - fd1) <= 1e-15 * scale / h + 1e-7 * scale and abs(t['d2'] - fd2) <= 1e-15 * scale / (h * h) + 1e-6 * scale


def _everything(fun, free, n1):
    p = fun.predict(free, n0=1, n1=n1)
    return [np.array([fun.value(free)]), fun.grad(free), fun.hessian(free)] + [p[k] for k in sorted(p)]


def test_lambda_zero_is_bitwise_and_log_four_is_a_fresh_model(vb):
    """lambda = 0 is bit for bit the fixed-phi result; after lambda = log 4 the results equal those of a model built with 4 phi0
    (e^{log 4} phi0 and 4 phi0 differ by an ulp, 2e-16, which the inverse behind var_lrvb multiplies by the condition number of this
    shape, 2.2e3, once per row that moves it: 1e-11 of the largest magnitude), and back at 0 the first values return bitwise."""
    N, P, K, G = 65, 5, 2, 3
    c = _case(vb, N, P, K, G)
    free = c['free']
    A, B = _fresh(vb, c, G), _fresh(vb, c, G)                            # B never touches the parameter
    base = _everything(B, free, N - 2)
    first = _everything(A, free, N - 2)
    assert all(np.array_equal(p, q) for p, q in zip(first, base))
    R = np.eye(free.size)[:, [0, free.size - 1]]
    sol = A.solve(free, R, on_device=True)
    assert A._dev_factor_key is not None
    _set_lam(A, np.log(4.0))
    moved = _everything(A, free, N - 2)
    assert A._dev_factor_key is None                                     # the resident factor went with the old phi
    assert not np.array_equal(moved[0], base[0])
    four = _model(vb, c['x'], c['y'], c['z'], c['w'], c['o'], 4.0 * c['ph'], c['gid'], G)[1]
    want = _everything(four, free, N - 2)
    errs = [_largest(p, q) for p, q in zip(moved, want)]
    print('lambda = log 4 against a model built with 4 phi0', errs)
    assert max(errs) <= 1e-11
    assert abs((A.log_norm_const() - four.log_norm_const()) / four.log_norm_const()) <= 1e-13
    _set_lam(A, 0.0)
    back = _everything(A, free, N - 2)
    assert all(np.array_equal(p, q) for p, q in zip(back, base))
    assert np.array_equal(A.solve(free, R, on_device=True), sol) and np.array_equal(A._phi, c['ph'])


FIT_SHAPE, PHI_TRUE = (2000, 4, 1, 30), 6.0


def _simulate(seed=7):
    N, P, K, G = FIT_SHAPE
    rng = np.random.default_rng([seed, 43])
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    z = np.ones((N, 1))
    gid = rng.integers(0, G, size=N).astype(np.int32)
    t = 1.0 + x @ (0.8 * rng.normal(size=P)) + (z * (0.5 * rng.normal(size=(G, K)))[gid]).sum(1)
    y = rng.gamma(PHI_TRUE, np.exp(t) / PHI_TRUE)
    return x, y, z, np.ones(N), gid, np.zeros(N)


def test_dispersion_sensitivity_against_refits_and_fit_dispersion(vb):
    """Simulated data at phi = 6, the model built with phi0 = phi / 4.  Refits at lambda = +-0.05: the moments of beta and mu
    predicted by `dispersion_sensitivity` (both routes) and by `ParametricSensitivityLinearApproximation` with `log_dispersion_par`
    agree with the refit differences within the project's refit margin, 5 % of the largest change.  Then `fit_dispersion`: a
    stationary point of the profiled objective with positive curvature, F larger at lambda-hat +- 0.1 after refits, and phi-hat
    inside the gross-error band [phi / 2, 2 phi]."""
    N, P, K, G = FIT_SHAPE
    x, y, z, w, gid, o = _simulate()
    par, fun = _model(vb, x, y, z, w, o, PHI_TRUE / 4.0, gid, G)
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
    lam, th = out['lam'], out['theta']
    t = fun.dispersion_terms(th)
    phi_hat = out['phi_scale'] * PHI_TRUE / 4.0
    print('fit_dispersion', {k: out[k] for k in ('lam', 'phi_scale', 'slope', 'curvature', 'iterations')}, 'F_ll', t['d2'], 'phi_hat', phi_hat)
    assert fun.log_dispersion == lam and out['iterations'] <= 20
    assert abs(out['slope']) < 1e-6 * (abs(t['d2']) + 1.0) and out['curvature'] > 0
    F = lambda theta: fun.value(theta) - fun.log_norm_const()
    F_hat = F(th)
    dth = fun.dispersion_sensitivity(th)
    for step in (0.1, -0.1):
        _set_lam(fun, lam + step)
        assert F(_fit(vb, objective, th + step * dth)) > F_hat
    _set_lam(fun, lam)
    assert PHI_TRUE / 2.0 <= phi_hat <= 2.0 * PHI_TRUE                    # a gross-error band, not a measurement


# ---- D: predictions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (130, 64, 4, 2)])
def test_predict_window_and_new_rows(vb, N, P, K, G):
    """Both routes; a window no tile boundary aligns with and new rows, some at the population level (group -1).  The mean is
    E e^t = exp(rho + var / 2) whatever phi; the reference takes it on its 96 nodes."""
    c = _case(vb, N, P, K, G)
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
    for what, kw, Cm, off in (('window', dict(n0=n0, n1=n1), _moments(x[n0:n1], z[n0:n1], gid[n0:n1], P, K, G), c['o'][n0:n1]),
                              ('new rows', dict(newdata=new), _moments(new['x'], new['z'], new['groups'], P, K, G), new['offset'])):
        want_var = np.einsum('nd,de,ne->n', Cm, Hinv, Cm)
        want_rho = off + Cm @ free                                       # the means are free coordinates themselves
        outs = [fun.predict(free, on_device=dev, **kw) for dev in (False, True)]
        for route, out in zip(('host', 'device'), outs):
            assert np.allclose(out['rho'], want_rho, rtol=1e-12, atol=1e-12)
            assert np.allclose(out['var_lrvb'], want_var, rtol=1e-6, atol=0)
            for col, var in (('mean_mf', 'var_mf'), ('mean_lrvb', 'var_lrvb')):
                want = ref.response_mean(out['rho'], out[var])
                err = np.abs(out[col] - want) / want
                print('predict', (N, P, K, G), what, route, col, float(np.max(err)))
                assert out[col].shape == want.shape and np.all(want > 0.0) and np.all(err <= 1e-12)
        assert np.allclose(outs[1]['var_lrvb'], outs[0]['var_lrvb'], rtol=1e-6, atol=0)
    full = fun.predict(free, on_device=True)
    win = fun.predict(free, n0=n0, n1=n1, on_device=True)
    assert all(np.array_equal(win[k], full[k][n0:n1]) for k in full)     # a window equals the same rows of the full result bitwise
    with_phi = fun.predict(free, newdata=dict(new, dispersion=np.full(n_new, 3.0)), on_device=True)
    without = fun.predict(free, newdata=new, on_device=True)
    assert all(np.array_equal(with_phi[k], without[k]) for k in without)
    with pytest.raises(ValueError, match='trials'):
        fun.predict(free, newdata=dict(new, trials=np.ones(n_new)))


# ---- E: influence ------------------------------------------------------------------------------------------------------------
_infl = {}


def _infl_case(vb, N, P, K, G):
    """The dense reference of tests/test_gpu_glmm_link.py::_infl_case, computed once."""
    key = (N, P, K, G)
    if key in _infl:
        return _infl[key]
    c = _case(vb, N, P, K, G)
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
    pt = _point(c['eta'], P, K, G)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want = c['rows_mv'] @ A.T                                            # N x 21
    for Q in (5, 21):                                                    # 21 crosses the 16-column MFMA block
        got = fun.ctx.glmm_gamma_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        win = fun.ctx.glmm_gamma_obs_influence(*pt, A[:Q], n0=3, n1=N - 2)
        assert win.shape == (N - 5, Q) and np.array_equal(win, got[3:N - 2])
    rows = fun.ctx.glmm_gamma_obs_influence(*pt, A)
    a, b = fun.ctx.glmm_gamma_group_influence(*pt, A), fun.ctx.glmm_gamma_group_influence(*pt, A)
    e = rel_err(a, _segment_sum(gid, G, w[:, None] * rows))
    print('group sums', N, P, K, G, e)
    assert a.shape == (G, 21) and e < 1e-10
    assert rel_err(a, _segment_sum(gid, G, w[:, None] * want)) < 1e-9   # and against autograd directly
    assert np.array_equal(a, b)                                           # bitwise reproducible
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)      # the empty group


@pytest.mark.parametrize('N,P,K,G', INFL_SHAPES)
def test_influence_routes_stream_hyper_and_dense_cross_hessian(vb, N, P, K, G):
    c = _infl_case(vb, N, P, K, G)
    fun, par, free, w, gid = c['fun'], c['par'], c['free'], c['w'], c['gid']
    D = 2 * P + 4 * K + 2 * G * K
    want = -np.linalg.solve(c['Hf'], c['Cw']).T                           # N x D
    rows = fun.obs_influence(free, np.eye(D))
    print('arrow route', rel_err(rows, want))
    assert np.allclose(rows, want, rtol=1e-6, atol=1e-12)
    assert np.allclose(fun.obs_influence(free, np.eye(D), on_device=True), rows, rtol=1e-6, atol=1e-12)
    gi = fun.group_influence(free, np.eye(D))
    assert np.allclose(fun.group_influence(free, np.eye(D), on_device=True), gi, rtol=1e-6, atol=1e-12)
    assert np.allclose(gi, _segment_sum(gid, G, w[:, None] * want), rtol=1e-6, atol=1e-12)
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, free, w, stream_hyper=True)
    dense = lin.get_doutput_dhyper_rows(np.eye(D))
    assert np.allclose(dense, want, rtol=1e-6, atol=1e-12)
    n0, n1 = 7, min(N - 1, 100)
    assert np.allclose(lin.get_doutput_dhyper_rows(np.eye(D)[:3], n0=n0, n1=n1), want[n0:n1, :3], rtol=1e-6, atol=1e-12)
    C = fun.cross_hessian(fun.weights_par, free, True)                   # the dense weight cross Hessian (small-N protocol)
    assert C.shape == (D, N) and rel_err(C, c['Cw']) < 1e-9
    # group_cov and ranef_se on both routes against the reference inverse
    Hinv = np.linalg.inv(c['Hf'])
    ng = 2 * P + 4 * K
    for dev in (False, True):
        se_lr, se_mf = fun.ranef_se(free, on_device=dev)
        assert np.allclose(se_lr.ravel(), np.sqrt(np.diag(Hinv)[ng + np.arange(G * K)]), rtol=1e-6, atol=0) and se_mf.shape == (G, K)
    sens = fun.global_sensitivity(fun.tau_prior_par, free)
    assert sens.shape[0] == ng and np.all(np.isfinite(sens))


# ---- F: state and refusals -----------------------------------------------------------------------------------------------------
def test_state_contract(vb):
    """The new entries read neither lrvb_set_link nor lrvb_set_trials, leave the other likelihoods' entries alone, and a missing
    dispersion is LRVB_ERR_STATE after which the context goes on working."""
    hip = vb._hip
    N, P, K, G = 130, 4, 2, 5
    x, y, z, w, gid, o, ph, free = ref.problem(N, P, K, G, 31, phi='vector', empty_group=False)
    o = o.copy()
    o[0] += LOG_PROBES[0]
    o[1] += LOG_PROBES[1]
    pt = _point(_eta(free, P, K, G), P, K, G)
    _, fun = _model(vb, x, y, z, w, o, ph, gid, G)
    ctx = fun.ctx
    gh = np.polynomial.hermite.hermgauss(20)
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G * K))
    gamma = lambda: (ctx.glmm_gamma_terms(*pt), ctx.glmm_gamma_obs_influence(*pt, A, n0=3, n1=N - 2), ctx.glmm_gamma_group_influence(*pt, A),
                     ctx.glmm_gamma_dispersion_terms(*pt))
    same = lambda a, b: _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and all(np.array_equal(p, q) for p, q in zip(a[3], b[3]))
    base = gamma()
    assert same(gamma(), base)                                           # two calls at one point
    trials = np.random.default_rng(3).integers(1, 9, size=N).astype(np.float64)
    for link, tr in ((1, None), (2, trials), (0, trials), (0, None)):
        ctx.set_link(link)
        ctx.set_trials(tr)
        assert same(gamma(), base)
    # the resident sums of the new entry are what the Schur entry works on; the dispersion entry leaves them, lrvb_set_dispersion drops them
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    ctx.glmm_gamma_terms(*pt)
    assert schur() == hip.OK
    M0 = M.copy()
    ctx.glmm_gamma_dispersion_terms(*pt)
    assert schur() == hip.OK and np.array_equal(M, M0)
    ctx.set_dispersion(ph)
    assert schur() == hip.ERR_STATE
    assert same(gamma(), base)
    # phi and log(y) are read from the row's own entry: permuted ones give other numbers
    ctx.set_dispersion(ph[::-1].copy())
    assert not _same(ctx.glmm_gamma_terms(*pt), base[0])
    # no dispersion, one of the wrong length: the error code and the existing texts
    val = np.empty(1)
    raw = lambda: ctx._lib.lrvb_glmm_gamma_terms(ctx._h, pt[0].ctypes.data, pt[1].ctypes.data, P, pt[2].ctypes.data, pt[3].ctypes.data, G, K,
                                                 val.ctypes.data, None, None, None, 0)
    ctx.set_dispersion(None)
    assert raw() == hip.ERR_STATE
    for call in (lambda: ctx.glmm_gamma_terms(*pt), lambda: ctx.glmm_gamma_obs_influence(*pt, A), lambda: ctx.glmm_gamma_group_influence(*pt, A),
                 lambda: ctx.glmm_gamma_dispersion_terms(*pt)):
        with pytest.raises(Exception, match='no dispersion: call lrvb_set_dispersion first'):
            call()
    ctx.set_dispersion(np.ones(N + 1))
    assert raw() == hip.ERR_STATE
    with pytest.raises(Exception, match='the dispersion has {} entries, the model has {} observations'.format(N + 1, N)):
        ctx.glmm_gamma_terms(*pt)
    ctx.set_dispersion(ph)
    assert same(gamma(), base)                                           # and the context goes on working
    # the other likelihoods' entries give the same bits before and after a call of the new ones
    ctx.set_trials(trials)
    others = lambda: (ctx.glmm_slopes_terms(*pt, *gh), ctx.glmm_slopes_obs_influence(*pt, *gh, A), ctx.glmm_slopes_group_influence(*pt, *gh, A),
                      ctx.glmm_poisson_terms(*pt), ctx.glmm_poisson_obs_influence(*pt, A), ctx.glmm_poisson_group_influence(*pt, A),
                      ctx.glmm_binomial_terms(*pt, *gh), ctx.glmm_binomial_obs_influence(*pt, *gh, A), ctx.glmm_binomial_group_influence(*pt, *gh, A),
                      ctx.glmm_beta_terms(*pt, *gh), ctx.glmm_beta_obs_influence(*pt, *gh, A), ctx.glmm_beta_group_influence(*pt, *gh, A))
    before = others()
    assert same(gamma(), base)
    after = others()
    assert all(_same(after[i], before[i]) for i in (0, 3, 6, 9))
    assert all(np.array_equal(after[i], before[i]) for i in (1, 2, 4, 5, 7, 8, 10, 11))
    assert all(not _same(before[i], base[0]) for i in (0, 3, 6, 9))      # and they are other numbers
    assert vb._hip.load().lrvb_version() == 1


def test_refusals_by_error_code(vb):
    hip = vb._hip
    rng = np.random.default_rng(47)

    def context(N, P):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='poisson', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)) / np.sqrt(P))
        ctx.set_data(hip.SLOT_Y, rng.normal(size=N))                     # log(y)
        ctx.set_dispersion(rng.uniform(0.5, 40.0, size=N))
        return ctx

    def call(ctx, P, G, K, kind, n0=0, n1=None):
        Kc = min(max(K, 1), 5)
        m, v, e, rr = np.zeros(P), np.ones(P), np.zeros(max(G * Kc, 1)), np.ones(max(G * Kc, 1))
        head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, K)
        lib = ctx._lib
        n1 = ctx.n_obs if n1 is None else n1
        if kind == 'terms':
            val = np.empty(1)
            return lib.lrvb_glmm_gamma_terms(*head, val.ctypes.data, None, None, None, 0)
        if kind == 'disp':
            d, cg, cl = np.empty(2), np.empty(2 * P), np.empty((max(G, 1), 2 * Kc))
            return lib.lrvb_glmm_gamma_dispersion_terms(*head, d.ctypes.data, cg.ctypes.data, cl.ctypes.data)
        Q = 2
        Ag, Al = np.ones((Q, 2 * P)), np.ones((max(G, 1), 2 * Kc, Q))
        out = np.empty((5 * max(ctx.n_obs, G), Q))
        if kind == 'group':
            return lib.lrvb_glmm_gamma_group_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, out.ctypes.data)
        return lib.lrvb_glmm_gamma_obs_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, n0, n1, out.ctypes.data)

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
        ctx.set_offset(np.zeros(N + 1))
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # an offset of the wrong length
        ctx.set_offset(None)
        ctx.set_dispersion(np.ones(N + 1))
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # a dispersion of the wrong length
        ctx.set_dispersion(None)
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # no dispersion
        ctx.set_dispersion(np.full(N, 2.5))
        if kind == 'rows':
            assert call(ctx, 3, G, K, kind, n0=5, n1=4) == hip.ERR_INVALID and call(ctx, 3, G, K, kind, n1=N + 1) == hip.ERR_INVALID
        assert call(ctx, 3, G, K, kind) == hip.OK
    # the texts, through the wrappers
    wide = context(N, 65)
    with pytest.raises(Exception, match='the Gamma mixed model needs P <= 64'):
        wide.glmm_gamma_terms(np.zeros(65), np.ones(65), np.zeros((G, K)), np.ones((G, K)))
    with pytest.raises(Exception, match='1 to 4 random effects per group'):
        ctx.glmm_gamma_terms(np.zeros(3), np.ones(3), np.zeros((G, 5)), np.ones((G, 5)))
    # the constructor: y <= 0 or not finite is a ValueError that names the rows and points to the two-part composite; so is a bad dispersion
    x, z = np.ones((N, 2)), np.ones((N, K))
    for bad in (0.0, -1.0, np.nan, np.inf):
        y = np.full(N, 0.4)
        y[5] = bad
        with pytest.raises(ValueError, match='1 of 20 rows.*HurdleGammaGLMM'):
            vb.GammaGLMMObjective(_par(vb, 2, K, G), x, y, z, gid, G, 2.0)
    for phi in (0.0, -3.0, np.inf, np.ones(N + 1)):
        with pytest.raises(ValueError, match='dispersion'):
            vb.GammaGLMMObjective(_par(vb, 2, K, G), x, np.full(N, 0.4), z, gid, G, phi)


def test_extreme_points(vb):
    """P = 1 with x = +-1.  A mean of -800 puts rho = -800 + o on the rows with x = 1: g = phi exp(log y + 800 + ..) overflows, the
    point is refused with a ValueError that names the cause, and no sums stay resident.  On data with x = 1 throughout, a mean of
    +800 is accepted: g underflows to 0 on every row, the value is sum w phi rho to rounding and the gradient sum w phi x."""
    hip = vb._hip
    N, K, G = 70, 1, 3
    rng = np.random.default_rng(9)
    x = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None]
    y, ph, w, o = np.exp(rng.normal(size=N)), np.exp(rng.uniform(np.log(0.05), np.log(1e4), size=N)), rng.uniform(0.5, 1.5, size=N), rng.normal(size=N)
    gid = (np.arange(N) % G).astype(np.int32)
    v, e, r = np.array([0.5]), np.zeros((G, K)), np.full((G, K), 0.7)
    _, fun = _model(vb, x, y, None, w, o, ph, gid, G, K=K)
    ctx = fun.ctx
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 + 3 * K, 2 + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    good = (np.array([0.3]), v, e, r)
    base = ctx.glmm_gamma_terms(*good)
    assert np.isfinite(base[0]) and schur() == hip.OK
    for m in (-800.0, 800.0):                                            # either sign overflows on half the rows of this design
        with pytest.raises(ValueError, match='Gamma data term is not finite.*overflows'):
            ctx.glmm_gamma_terms(np.array([m]), v, e, r)
        assert schur() == hip.ERR_STATE                                  # no sums left resident
        with pytest.raises(ValueError, match='not finite'):
            ctx.glmm_gamma_dispersion_terms(np.array([m]), v, e, r)
        assert _same(ctx.glmm_gamma_terms(*good), base) and schur() == hip.OK
    ones = np.ones((N, 1))
    _, up = _model(vb, ones, y, None, w, o, ph, gid, G, K=K)
    m = np.array([800.0])
    rho = o + 800.0
    val, gg, Hb, gs = up.ctx.glmm_gamma_terms(m, v, e, r)
    want, want_g = np.sum(w * ph * rho), np.sum(w * ph)
    print('rho = +800', abs(val - want) / want, abs(gg[0] - want_g) / want_g, gg[1], float(np.max(np.abs(Hb))))
    assert abs(val - want) <= 1e-14 * want and abs(gg[0] - want_g) <= 1e-14 * want_g
    assert gg[1] == 0.0 and np.all(Hb == 0.0) and np.all(gs[:, K:] == 0.0)


# ---- G: the two-part composite -------------------------------------------------------------------------------------------------
def test_hurdle_gamma_parts_are_the_stand_alone_models_and_predict(vb):
    """`HurdleGammaGLMM`: the zero part is `BinomialGLMMObjective` on 1[y > 0] over all rows, the positive part
    `GammaGLMMObjective` on the rows with y > 0 with phi subset to them -- value, gradient and predictions of either part equal a
    stand-alone model on the same rows bit for bit; `predict` returns P(y > 0), E[y | y > 0] and their product under both
    variances, checked against the reference's response means."""
    import glmm_binomial_reference as bref
    N, P, K, G = 130, 5, 2, 4
    x, y, z, w, gid, o, ph, free = ref.problem(N, P, K, G, 53, phi='vector', empty_group=False)
    y = y.copy()
    y[0], y[1] = 0.3, 2.5                                                # amounts between 0 and 1 are amounts, not counts
    y[5::3] = 0.0
    pos = np.flatnonzero(y > 0.0)
    kw = _prior_kw(HYP)
    H = vb.HurdleGammaGLMM(_par(vb, P, K, G), _par(vb, P, K, G), x, y, z, gid, G, ph, offset=o, weights=w, **kw)
    assert np.array_equal(H.positive_rows, pos)
    zero = vb.BinomialGLMMObjective(_par(vb, P, K, G), x, (y > 0.0).astype(np.float64), z, gid, G, weights=w, **kw)
    gam = vb.GammaGLMMObjective(_par(vb, P, K, G), x[pos], y[pos], z[pos], gid[pos], G, ph[pos], offset=o[pos], weights=w[pos], **kw)
    assert H.value(free, free) == zero.value(free) + gam.value(free) and H.log_norm_const() == gam.log_norm_const()
    assert np.array_equal(H.zero.grad(free), zero.grad(free)) and np.array_equal(H.count.grad(free), gam.grad(free))
    assert np.array_equal(H.count.hessian(free), gam.hessian(free))
    rng = np.random.default_rng(5)
    n_new = 40
    new = dict(x=rng.normal(size=(n_new, P)) / np.sqrt(P), z=np.concatenate([np.ones((n_new, 1)), 0.5 * rng.normal(size=(n_new, K - 1))], axis=1),
               groups=rng.integers(-1, G, size=n_new), offset=0.3 * rng.normal(size=n_new))
    for dev in (False, True):
        for kwp in (dict(n0=3, n1=N - 2), dict(newdata=new)):
            out = H.predict(free, free, on_device=dev, **kwp)
            nd = kwp.get('newdata')
            rows = nd if nd else dict(x=x[3:N - 2], z=z[3:N - 2], groups=gid[3:N - 2], offset=o[3:N - 2])
            pz = zero.predict(free, on_device=dev, newdata=dict(rows, offset=None))
            pc = gam.predict(free, on_device=dev, newdata=rows)
            for v in ('mf', 'lrvb'):
                assert np.array_equal(out['p_pos_' + v], pz['mean_' + v]) and np.array_equal(out['mean_count_' + v], pc['mean_' + v])
                want = bref_response(out['zero']['rho'], out['zero']['var_' + v]) * ref.response_mean(out['count']['rho'], out['count']['var_' + v])
                err = np.abs(out['mean_' + v] - want) / want
                print('hurdle predict', 'device' if dev else 'host', 'new rows' if nd else 'window', v, float(np.max(err)))
                assert np.all(err <= 1e-12)
    with pytest.raises(ValueError, match='>= 0'):
        vb.HurdleGammaGLMM(_par(vb, P, K, G), _par(vb, P, K, G), x, -y, z, gid, G, ph, **kw)


def bref_response(rho, s, deg=20):
    """E sigma(t) on the 20 nodes of the binomial model (tests/glmm_beta_reference.py::response_mean)."""
    import glmm_beta_reference as beta_ref
    return beta_ref.response_mean(rho, s, deg)


# ---- H: fit ------------------------------------------------------------------------------------------------------------------
def test_fit_covariance_and_tau_prior_sensitivity(vb):
    """The body and thresholds of tests/test_gpu_glmm_ztnegbin.py::test_fit_covariance_and_tau_prior_sensitivity."""
    N, P, K, G = 2000, 4, 2, 30
    x, y, z, w, gid, o, ph, free0 = ref.problem(N, P, K, G, 77, phi=20.0, big_group=False, empty_group=False)
    y = y.copy()
    y[:3] = np.exp(o[:3])                                                # no probe rows in a fit: ordinary amounts
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, o, 20.0, gid, G)
    ng = 2 * P + 4 * K
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = ref.targs(x, y, z, w, o, ph, gid, G, HYP)
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
    se_lr, se_mf = fun.ranef_se(th, on_device=True)
    ie = ng + np.arange(G * K)
    assert np.allclose(se_lr.ravel(), np.sqrt(np.diag(Hinv)[ie]), rtol=1e-6, atol=0) and se_mf.shape == (G, K)
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

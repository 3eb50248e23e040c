"""The log-dispersion derivatives of the Beta and the NB2 mixed model without a GPU: the package's host forms
(the formulas of the kernels, policies BetaDispLik and NegBinDispLik) and the torch reference tests/glmm_dispersion_reference.py
against mpmath at 60 digits of the UNSHIFTED definitions

    Beta   h(t, phi) = lgamma(phi sigma(t)) + lgamma(phi sigma(-t)) - phi l sigma(t),        l = logit(y)
    NB2    h(t, phi) = (y + phi) log(1 + e^t / phi) - y (t - log phi)

differentiated in lambda (phi = e^lambda phi0, d/d lambda = phi d/d phi) and t.  The exact node terms are the plain chain rule of
those definitions with mpmath's polygamma; `test_exact_terms_are_independent` checks that chain rule against mpmath's numerical
MIXED differentiation (mp.diff in (t, lambda), no formula) at the issue's points and in the tails.

Grids.  Beta: that of tests/test_glmm_beta_host_math.py, rho in {-30 .. 30} x s in {0, 0.5, 3} x phi in {0.3 .. 3000} x l in {-8 .. 3},
540 points.  NB2: the same rho, s and phi x y in {0, 1, 7, 400}; rho is the RAW linear predictor, so eta = rho - log phi runs from
-38 to 31.  The four quantities per family are E h_l, E d_t h_l, E d_t^2 h_l, E h_ll on the 20-node rule, and the per-node terms
themselves on t = -40 .. 40.

Measure.  POINTWISE, cap `CAP` = 1e-10 (the project's), relative to max(|exact|, scale), where the SCALE of a quantity at a point is
the sum over the nodes of w_k times the sum of the ABSOLUTE VALUES of the terms its formula adds at that node:
    Beta   h_l:      |a psi(1 + a)| + |b psi(1 + b)| + |l a| + 2                    (a = phi mu, b = phi (1 - mu), v = mu (1 - mu))
           h_ll:     the first three and a^2 psi'(1 + a) + b^2 psi'(1 + b)
           d_t h_l:  phi v (|psi(1 + a)| + a psi'(1 + a) + |psi(1 + b)| + b psi'(1 + b) + |l|)
           d_t^2:    phi^2 v^2 (2 psi'(1 + a) + a |psi''(1 + a)| + 2 psi'(1 + b) + b |psi''(1 + b)|) + |1 - 2 mu| times the line above
    NB2    h_l:      phi sp + m sg + y;   h_ll: phi sp + 2 phi sg + m sg';   d_t h_l: phi sg + m sg';   d_t^2: phi sg' + m |sg''|
(m = y + phi; sp, sg the softplus and sigmoid at eta).  These quantities are differences of such terms -- h_l of NB2 is
mu - mu (1 + y / phi) + y + O(mu^2 / phi) at large phi -- and a sum of fp64 terms cannot be better than eps times the largest.
The scales are computed here from scipy's digamma / polygamma, not from the package.

`log_norm_const_dispersion`.  Both forms per row against mpmath, phi / y up to 1e8 for NB2 (`digamma_difference`: the finite sum,
the term-by-term series and the scipy branch are all visited), same cap; NB2 relative to the exact value itself (no cancellation
is left in the form), Beta relative to |phi psi(phi)| + |phi log(1 - y)|."""
import numpy as np
import pytest

import glmm_dispersion_reference as dref

CAP = 1e-10
RHO = np.array([-30.0, -12.0, -5.0, -2.0, 0.0, 2.5, 5.0, 12.0, 30.0])
S = np.array([0.0, 0.5, 3.0])
PHI = np.array([0.3, 2.0, 15.0, 200.0, 3000.0])
L = np.array([-8.0, -0.7, 0.4, 3.0])
Y = np.array([0.0, 1.0, 7.0, 400.0])
NAMES = ('E h_l', 'E d_t h_l', 'E d_t^2 h_l', 'E h_ll')


def _points(last):
    return tuple(a.ravel() for a in np.meshgrid(RHO, S, PHI, last, indexing='ij'))


def _gh():
    return np.polynomial.hermite.hermgauss(dref.GH_DEG)


@pytest.fixture(scope='module', autouse=True)
def pkg():
    """The host forms this file pins.  Every test of the file asks for them, the ones on the exact terms and on the reference
    included: without the feature there is nothing for those yardsticks to measure."""
    from lrvb_amd import glmm_beta, glmm_binomial
    assert hasattr(glmm_beta, 'beta_h_dispersion') and hasattr(glmm_binomial, 'negbin_h_dispersion')
    return glmm_beta, glmm_binomial


# ---- exact node terms (mpmath) -------------------------------------------------------------------------------------------------
def _mp_beta(t, phi, l):
    """[h_l, d_t h_l, d_t^2 h_l, h_ll] of the UNSHIFTED Beta h by the plain chain rule."""
    import mpmath as mp
    mu, nu = 1 / (1 + mp.exp(-t)), 1 / (1 + mp.exp(t))
    v, d = mu * nu, nu - mu
    a, b = phi * mu, phi * nu
    pa, pb = [mp.polygamma(j, a) for j in range(3)], [mp.polygamma(j, b) for j in range(3)]
    first = a * pa[0] + b * pb[0] - l * a
    K1 = phi * (pa[0] + a * pa[1] - pb[0] - b * pb[1] - l)
    K2 = phi ** 2 * (2 * pa[1] + a * pa[2] + 2 * pb[1] + b * pb[2])
    return [first, K1 * v, K2 * v ** 2 + K1 * v * d, first + a ** 2 * pa[1] + b ** 2 * pb[1]]


def _mp_negbin(t, phi, y):
    import mpmath as mp
    eta = t - mp.log(phi)
    sg = 1 / (1 + mp.exp(-eta))
    sp = mp.log1p(mp.exp(eta)) if eta < 0 else eta + mp.log1p(mp.exp(-eta))
    g2 = sg * (1 - sg)
    g3 = g2 * (1 - 2 * sg)
    m = y + phi
    return [phi * sp - m * sg + y, phi * sg - m * g2, phi * g2 - m * g3, phi * sp - 2 * phi * sg + m * g2]


def _mp_def(family, l_or_y):
    """The unshifted definition as an mpmath function of (t, lambda) at phi0 = 1 (phi = e^lambda)."""
    import mpmath as mp
    c = mp.mpf(float(l_or_y))
    if family == 'beta':
        return lambda t, lam: (mp.loggamma(mp.exp(lam) / (1 + mp.exp(-t))) + mp.loggamma(mp.exp(lam) / (1 + mp.exp(t)))
                               - mp.exp(lam) * c / (1 + mp.exp(-t)))
    return lambda t, lam: (c + mp.exp(lam)) * mp.log1p(mp.exp(t - lam)) - c * (t - lam)


MP = {'beta': _mp_beta, 'negbin': _mp_negbin}


def test_exact_terms_are_independent():
    """The chain rules above against mp.diff, numerical mixed differentiation of the definitions in (t, lambda): the issue's points
    t = -3, 0.4, 5, phi = 7.5, l = -1.3, y = 3, and a tail point each."""
    import mpmath as mp
    mp.mp.dps = 60
    worst = 0.0
    for family, c, pts in (('beta', -1.3, [(-3.0, 7.5), (0.4, 7.5), (5.0, 7.5), (-25.0, 0.3), (30.0, 3000.0)]),
                           ('negbin', 3.0, [(-3.0, 7.5), (0.4, 7.5), (5.0, 7.5), (-25.0, 0.3), (30.0, 3000.0)])):
        f = _mp_def(family, c)
        for t, phi in pts:
            t, lam = mp.mpf(t), mp.log(mp.mpf(phi))
            got = MP[family](t, mp.mpf(phi), mp.mpf(c))
            for q, order in zip(got, ((0, 1), (1, 1), (2, 1), (0, 2))):
                want = mp.diff(f, (t, lam), order)
                worst = max(worst, float(abs(q - want) / abs(want)))
    print('mpmath chain rules against mp.diff, relative:', worst)
    assert worst <= 1e-25


def _exact_moments(family, rho, s, phi, c):
    import mpmath as mp
    mp.mp.dps = 60
    e = np.zeros((4, rho.size))
    for n in range(rho.size):
        acc = [mp.mpf(0)] * 4
        gx, gw = _gh() if s[n] > 0.0 else ([0.0], [np.sqrt(np.pi)])
        for xk, wk in zip(gx, gw):
            t = mp.mpf(float(rho[n])) + mp.sqrt(mp.mpf(float(s[n]))) * mp.sqrt(2) * mp.mpf(float(xk))
            w = mp.mpf(float(wk)) / mp.sqrt(mp.pi)
            for k, q in enumerate(MP[family](t, mp.mpf(float(phi[n])), mp.mpf(float(c[n])))):
                acc[k] += w * q
        e[:, n] = [float(a) for a in acc]
    return e


# ---- the scales of the module docstring (scipy, per node) ----------------------------------------------------------------------
def _scale_nodes(family, t, phi, c):
    from scipy.special import digamma, polygamma, expit
    if family == 'beta':
        mu, nu = expit(t), expit(-t)
        v = mu * nu
        a, b = phi * mu, phi * nu
        p0a, p0b = np.abs(digamma(1.0 + a)), np.abs(digamma(1.0 + b))
        p1a, p1b = polygamma(1, 1.0 + a), polygamma(1, 1.0 + b)
        p2a, p2b = np.abs(polygamma(2, 1.0 + a)), np.abs(polygamma(2, 1.0 + b))
        first = a * p0a + b * p0b + np.abs(c) * a
        k1 = phi * v * (p0a + a * p1a + p0b + b * p1b + np.abs(c))
        return [first + 2.0, k1, phi * phi * v * v * (2.0 * p1a + a * p2a + 2.0 * p1b + b * p2b) + np.abs(nu - mu) * k1,
                first + a * a * p1a + b * b * p1b]
    eta = t - np.log(phi)
    sp, sg = np.logaddexp(0.0, eta), expit(eta)
    g2 = sg * expit(-eta)
    g3 = np.abs(g2 * (expit(-eta) - sg))
    m = c + phi
    return [phi * sp + m * sg + c, phi * sg + m * g2, phi * g2 + m * g3, phi * sp + 2.0 * phi * sg + m * g2]


def _scale_moments(family, rho, s, phi, c):
    gx, gw = _gh()
    t = rho[:, None] + np.sqrt(s)[:, None] * np.sqrt(2.0) * gx[None, :]
    return np.stack([(q * gw / np.sqrt(np.pi)).sum(-1) for q in _scale_nodes(family, t, phi[:, None], c[:, None])])


CASES = {'beta': L, 'negbin': Y}
_exact_cache = {}


def _grid(family):
    if family not in _exact_cache:
        rho, s, phi, c = _points(CASES[family])
        _exact_cache[family] = (rho, s, phi, c, _exact_moments(family, rho, s, phi, c), _scale_moments(family, rho, s, phi, c))
    return _exact_cache[family]


def _host_moments(pkg, family, rho, s, phi, c):
    gx, gw = _gh()
    if family == 'beta':
        return pkg[0].beta_expected_h_dispersion(rho, s, c, phi, gx, gw)
    return pkg[1].negbin_expected_h_dispersion(rho, s, c, phi, gx, gw)


@pytest.mark.parametrize('family', ['beta', 'negbin'])
def test_expectations_against_mpmath_pointwise(pkg, family):
    rho, s, phi, c, exact, scale = _grid(family)
    assert np.all(scale >= np.abs(exact) * (1.0 - 1e-12))                # the scale is a sum of the magnitudes behind the exact value
    host = _host_moments(pkg, family, rho, s, phi, c)
    err = np.abs(host - exact) / np.maximum(np.abs(exact), scale)
    print(family, 'host', dict(zip(NAMES, err.max(-1))))
    print(family, 'smallest |exact| / scale per quantity', (np.abs(exact) / scale).min(-1))
    assert host.shape == exact.shape and np.all(err <= CAP)
    # s = 0: the expectation is the node function itself
    at0 = s == 0.0
    node = pkg[0].beta_h_dispersion if family == 'beta' else pkg[1].negbin_h_dispersion
    h = np.stack(node(rho[at0], phi[at0], c[at0]))
    assert np.all(np.abs(h - host[:, at0]) <= 1e-13 * scale[:, at0])


@pytest.mark.parametrize('family', ['beta', 'negbin'])
def test_reference_against_mpmath_pointwise(family):
    """The yardstick of the GPU tests on the same grid, same measure."""
    rho, s, phi, c, exact, scale = _grid(family)
    y = 1.0 / (1.0 + np.exp(-c)) if family == 'beta' else c              # the reference takes the proportion itself
    got = dref.row_pieces(family, rho, s, y, phi)[:4]
    err = np.abs(got - exact) / np.maximum(np.abs(exact), scale)
    print(family, 'reference', dict(zip(NAMES, err.max(-1))))
    assert np.all(err <= CAP)


@pytest.mark.parametrize('family', ['beta', 'negbin'])
def test_per_node_terms_against_mpmath(pkg, family):
    import mpmath as mp
    mp.mp.dps = 60
    tt = np.arange(-40.0, 41.0)
    t, phi, c = (a.ravel() for a in np.meshgrid(tt, PHI, CASES[family], indexing='ij'))
    exact = np.array([[float(q) for q in MP[family](mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(float(d)))] for a, b, d in zip(t, phi, c)]).T
    node = pkg[0].beta_h_dispersion if family == 'beta' else pkg[1].negbin_h_dispersion
    host = np.stack(node(t, phi, c))
    scale = np.stack(_scale_nodes(family, t, phi, c))
    err = np.abs(host - exact) / np.maximum(np.abs(exact), scale)
    print(family, 'per node', dict(zip(NAMES, err.max(-1))))
    assert np.all(err <= CAP)


def test_issue_points(pkg):
    """The eight identities at t = -3, 0.4, 5, phi = 7.5, l = -1.3, y = 3, pure relative error."""
    import mpmath as mp
    mp.mp.dps = 60
    for family, c, node in (('beta', -1.3, pkg[0].beta_h_dispersion), ('negbin', 3.0, pkg[1].negbin_h_dispersion)):
        for t in (-3.0, 0.4, 5.0):
            want = np.array([float(q) for q in MP[family](mp.mpf(t), mp.mpf(7.5), mp.mpf(c))])
            got = np.array([float(q) for q in node(t, 7.5, c)])
            assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want)), (family, t, got, want)


# ---- log_norm_const_dispersion ----------------------------------------------------------------------------------------------------
class _Weights:
    def __init__(self, n):
        self._w = np.ones(n)

    def get_vector(self):
        return self._w


def _stub(cls, **attrs):
    """An instance without a device: `log_norm_const_dispersion` reads `_phi`, the responses and the weights only."""
    obj = cls.__new__(cls)
    obj.__dict__.update(attrs)
    return obj


def test_negbin_log_norm_const_dispersion_against_mpmath(pkg):
    import mpmath as mp
    import lrvb_amd
    mp.mp.dps = 60
    gbin = pkg[1]
    y, phi = (a.ravel() for a in np.meshgrid(np.array([0.0, 1.0, 3.0, 7.0, 255.0, 256.0, 400.0, 2.5, 1e4]),
                                             np.array([0.3, 2.0, 9.99, 10.0, 15.0, 3000.0, 1e5, 3e8, 4e10]), indexing='ij'))
    assert (phi[y > 0] / y[y > 0]).max() >= 1e8
    d0, d1 = gbin.digamma_difference(y, phi)
    e0 = np.array([float(mp.digamma(mp.mpf(a) + mp.mpf(b)) - mp.digamma(mp.mpf(b))) for a, b in zip(y, phi)])
    e1 = np.array([float(mp.polygamma(1, mp.mpf(a) + mp.mpf(b)) - mp.polygamma(1, mp.mpf(b))) for a, b in zip(y, phi)])
    pos = y > 0
    assert np.all(d0[~pos] == 0.0) and np.all(d1[~pos] == 0.0)
    r0, r1 = np.abs(d0[pos] - e0[pos]) / np.abs(e0[pos]), np.abs(d1[pos] - e1[pos]) / np.abs(e1[pos])
    print('digamma_difference, pointwise relative: psi', r0.max(), "psi'", r1.max())
    assert r0.max() <= CAP and r1.max() <= CAP
    # the plain scipy difference does lose the digits this form keeps
    from scipy.special import digamma
    plain = np.abs((digamma(y + phi) - digamma(phi))[pos] - e0[pos]) / np.abs(e0[pos])
    print('plain scipy difference, worst relative:', plain.max())
    assert plain.max() > 1e-6
    # the method, per row and summed with weights
    for n in range(y.size):
        fun = _stub(lrvb_amd.NegBinomialGLMMObjective, _y=y[n:n + 1], _phi=phi[n:n + 1], weights_par=_Weights(1))
        c1, c2 = fun.log_norm_const_dispersion()
        w1 = phi[n] * e0[n]
        w2 = w1 + phi[n] ** 2 * e1[n]
        assert abs(c1 - w1) <= CAP * abs(w1) and abs(c2 - w2) <= CAP * max(abs(w2), abs(w1))


def test_beta_log_norm_const_dispersion_against_mpmath(pkg):
    import mpmath as mp
    import lrvb_amd
    mp.mp.dps = 60
    y, phi = (a.ravel() for a in np.meshgrid(np.array([1e-12, 0.03, 0.5, 0.9, 1.0 - 1e-12]), np.array([0.3, 1.4616, 2.0, 15.0, 3000.0, 1e8]),
                                             indexing='ij'))
    worst = 0.0
    for n in range(y.size):
        fun = _stub(lrvb_amd.BetaGLMMObjective, _y01=y[n:n + 1], _phi=phi[n:n + 1], weights_par=_Weights(1))
        c1, c2 = fun.log_norm_const_dispersion()
        p, yy = mp.mpf(float(phi[n])), mp.mpf(float(y[n]))
        t1, t2 = p * mp.digamma(p), p * mp.log1p(-yy)
        w1 = t1 + t2
        w2 = w1 + p ** 2 * mp.polygamma(1, p)
        sc = float(abs(t1) + abs(t2))
        worst = max(worst, abs(c1 - float(w1)) / sc, abs(c2 - float(w2)) / (sc + float(p ** 2 * mp.polygamma(1, p))))
    print('Beta log_norm_const_dispersion, worst over the scale:', worst)
    assert worst <= CAP


def test_log_norm_const_dispersion_is_the_derivative_of_log_norm_const(pkg):
    """Central differences of `log_norm_const()` itself in lambda (both classes, several rows and weights): 1e-6 relative."""
    import lrvb_amd
    rng = np.random.default_rng(5)
    n = 40
    w = _Weights(n)
    w._w = rng.uniform(0.0, 2.0, size=n)
    phi0 = np.exp(rng.uniform(np.log(0.5), np.log(1e3), size=n))
    for cls, attrs in ((lrvb_amd.NegBinomialGLMMObjective, dict(_y=rng.poisson(3.0, size=n).astype(np.float64))),
                       (lrvb_amd.BetaGLMMObjective, dict(_y01=rng.uniform(0.01, 0.99, size=n)))):
        def at(lam):
            return _stub(cls, _phi=np.exp(lam) * phi0, weights_par=w, **attrs)
        c1, c2 = at(0.0).log_norm_const_dispersion()
        d = 1e-4
        f1 = (at(d).log_norm_const() - at(-d).log_norm_const()) / (2 * d)
        f2 = (at(d).log_norm_const_dispersion()[0] - at(-d).log_norm_const_dispersion()[0]) / (2 * d)
        assert abs(f1 - c1) <= 1e-6 * abs(c1) and abs(f2 - c2) <= 1e-6 * abs(c2)

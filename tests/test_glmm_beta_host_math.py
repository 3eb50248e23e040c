"""The Beta likelihood without a GPU: the package's module-level host functions (the formulas of the kernels:
both lgamma arguments shifted by one, Faa di Bruno on G, the x >= 1 lgamma / polygamma evaluator) and the torch reference
tests/glmm_beta_reference.py against mpmath at 60 digits of the UNSHIFTED definition

    h(t) = lgamma(phi sigma(t)) + lgamma(phi sigma(-t)) - phi l sigma(t),     l = logit(y)

so that a wrong shift shows; the mirror identity, the known answer against scipy's Beta density, finite differences, and the
constructor's refusals.

Moments.  E h^(k), k = 0..4, on the 20-node rule.  Grid: rho in {-30, -12, -5, -2, 0, 2.5, 5, 12, 30} x s in {0, 0.5, 3} x phi in
{0.3, 2, 15, 200, 3000} x l in {-8, -0.7, 0.4, 3}: 540 points, the nodes reach |t| = 43.  No point is exactly symmetric (l != 0), so
no E h^(k) is an exact zero; the grid does hold points where E h''' is 2e-4 of E |h'''|.  The measure is POINTWISE: the error of
every E h^(k) over the magnitude of that E h^(k) at that point, and `CAP` = 1e-10 is the cap of tests/test_glmm_ztnegbin_host_math.py.
The exact node terms are mpmath's own polygamma functions at 60 digits in the plain chain rule of the unshifted h -- the form that
is useless in fp64 (it cancels 19 digits at |t| = 43) and exact to 40 digits there.  `test_exact_moments_are_independent` checks that
chain rule against mpmath.taylor (numerical differentiation, no formula) on a sample.
Host functions and reference both meet the cap on the whole grid (measured worsts: DESIGN.md section 40) -- the reference only
since its lgamma carries a derivative chain of its own (torch's trigamma is good to 5e-10: glmm_beta_reference.py).

Per node.  `beta_h` and the reference's h against the same exact terms on t = -40, -39, .., 40 x phi x l in {-8, -0.7, 0, 3}.
h', h''' and (for some phi, l) h'', h'''' cross zero inside the range -- at l = 0, t = 0 the odd ones are exact zeros -- so the error
is taken over max(|exact|, 1) for k = 0, 1 and over max(|exact|, 2 sigma'(t)) for k >= 2: 2 sigma' is the size of the softplus
part of h'' and falls with |t| as every derivative does.  `NODE` = 1e-10 again.

Evaluator.  `polygamma_ge1` (nine select steps to z >= 10, the series to B_16, as the kernels) against mpmath on [1, 1e6]:
relative, `EVAL` = 1e-13 (the issue's stand-in measured 2.6e-14; lgamma crosses zero at x = 1 and 2 and is measured over
max(|exact|, 1))."""
import numpy as np
import pytest

import glmm_beta_reference as ref

CAP, NODE, EVAL, IDENT = 1e-10, 1e-10, 1e-13, 1e-12
RHO = np.array([-30.0, -12.0, -5.0, -2.0, 0.0, 2.5, 5.0, 12.0, 30.0])
S = np.array([0.0, 0.5, 3.0])
PHI = np.array([0.3, 2.0, 15.0, 200.0, 3000.0])
L = np.array([-8.0, -0.7, 0.4, 3.0])


def _points():
    rho, s, phi, l = (a.ravel() for a in np.meshgrid(RHO, S, PHI, L, indexing='ij'))
    return rho, s, phi, l


def _gh(deg=ref.GH_DEG):
    return np.polynomial.hermite.hermgauss(deg)


@pytest.fixture(scope='module')
def gb():
    import lrvb_amd
    from lrvb_amd import glmm_beta
    assert hasattr(glmm_beta, 'beta_h') and hasattr(lrvb_amd, 'BetaGLMMObjective')
    return glmm_beta


def _mp_h(phi, l):
    """The unshifted definition as an mpmath function of t."""
    import mpmath as mp
    phi, l = mp.mpf(float(phi)), mp.mpf(float(l))

    def h(t):
        mu, nu = 1 / (1 + mp.exp(-t)), 1 / (1 + mp.exp(t))
        return mp.loggamma(phi * mu) + mp.loggamma(phi * nu) - phi * l * mu
    return h


def _mp_derivs(t, phi, l):
    """[h, h', .., h''''] at t (mpf) of the unshifted h by the plain chain rule with mpmath's polygamma at the working precision."""
    import mpmath as mp
    phi, l = mp.mpf(float(phi)), mp.mpf(float(l))
    mu, nu = 1 / (1 + mp.exp(-t)), 1 / (1 + mp.exp(t))
    v = mu * nu
    d = nu - mu
    m1, m2, m3, m4 = v, v * d, v * (1 - 6 * v), v * d * (1 - 12 * v)
    a, b = phi * mu, phi * nu
    F = [None] + [phi ** j * (mp.polygamma(j - 1, a) + (-1) ** j * mp.polygamma(j - 1, b)) for j in (1, 2, 3, 4)]
    F[1] -= phi * l
    return [mp.loggamma(a) + mp.loggamma(b) - phi * l * mu,
            F[1] * m1,
            F[2] * m1 ** 2 + F[1] * m2,
            F[3] * m1 ** 3 + 3 * F[2] * m1 * m2 + F[1] * m3,
            F[4] * m1 ** 4 + 6 * F[3] * m1 ** 2 * m2 + F[2] * (3 * m2 ** 2 + 4 * m1 * m3) + F[1] * m4]


@pytest.fixture(scope='module')
def exact():
    """E h^(k), k = 0..4 (5 x n), at the grid on the 20-node rule, every node term from mpmath at 60 digits.  Computed once."""
    import mpmath as mp
    mp.mp.dps = 60
    rho, s, phi, l = _points()
    e = np.zeros((5, rho.size))
    for n in range(rho.size):
        acc = [mp.mpf(0)] * 5
        gx, gw = _gh() if s[n] > 0.0 else ([0.0], [np.sqrt(np.pi)])       # s = 0: every node sits at rho and the weights sum to 1
        for xk, wk in zip(gx, gw):
            t = mp.mpf(float(rho[n])) + mp.sqrt(mp.mpf(float(s[n]))) * mp.sqrt(2) * mp.mpf(float(xk))
            w = mp.mpf(float(wk)) / mp.sqrt(mp.pi)
            for k, c in enumerate(_mp_derivs(t, phi[n], l[n])):
                acc[k] += w * c
        e[:, n] = [float(a) for a in acc]
    return e


def _pointwise(got, want):
    return np.abs(got - want) / np.abs(want)


def test_exact_moments_are_independent():
    """The chain rule of `_mp_derivs` against numerical differentiation (mpmath.taylor) of the definition, at 60 digits."""
    import mpmath as mp
    mp.mp.dps = 60
    worst = 0.0
    for t in (-40.0, -7.5, -0.3, 0.0, 2.0, 19.0, 40.0):
        for phi, l in ((0.3, -8.0), (15.0, 0.4), (3000.0, 3.0)):
            c = mp.taylor(_mp_h(phi, l), mp.mpf(t), 4)
            got = _mp_derivs(mp.mpf(t), phi, l)
            for k in range(5):
                want = c[k] * mp.factorial(k)
                worst = max(worst, float(abs(got[k] - want) / abs(want)))
    print('mpmath chain rule against mpmath.taylor, relative:', worst)
    assert worst <= 1e-25


def test_expectations_against_mpmath_pointwise(gb, exact):
    rho, s, phi, l = _points()
    gx, gw = _gh()
    assert np.all(exact != 0.0)
    host = gb.beta_expected_h(rho, s, l, phi, gx, gw)
    refc = ref.eh_coefs(rho, s, l, phi)
    eh, er = _pointwise(host, exact), _pointwise(refc, exact)
    print('host      E h^(k), k = 0..4, pointwise relative, whole grid:', eh.max(-1))
    print('reference E h^(k), k = 0..4, pointwise relative, whole grid:', er.max(-1))
    # the grid holds points where E h''' is a small remainder of its node terms
    t = rho[:, None] + np.sqrt(s)[:, None] * np.sqrt(2.0) * gx[None, :]
    mag = (np.abs(gb.beta_h(t, phi[:, None], l[:, None])[3]) * gw / np.sqrt(np.pi)).sum(-1)
    print('smallest |E h\'\'\'| / E |h\'\'\'|:', float(np.min(np.abs(exact[3]) / mag)))
    assert np.min(np.abs(exact[3]) / mag) < 1e-3
    assert host.shape == exact.shape and np.all(eh <= CAP)
    assert np.all(er <= CAP)
    a1, a2 = gb.beta_row_derivs(rho, s, l, phi, gx, gw)
    assert np.array_equal(a1, host[1]) and np.array_equal(a2, 0.5 * host[2])
    # s = 0: the expectation is the function itself
    at0 = s == 0.0
    h = np.stack(gb.beta_h(rho[at0], phi[at0], l[at0]))
    assert np.all(np.abs(h - host[:, at0]) <= 1e-14 * np.maximum(1.0, np.abs(h)))


def test_host_per_node_terms_against_mpmath(gb):
    import mpmath as mp
    mp.mp.dps = 60
    t = np.arange(-40.0, 40.5, 1.0)
    worst, worst_ref = np.zeros(5), np.zeros(5)
    for phi in PHI:
        for l in (-8.0, -0.7, 0.0, 3.0):
            got = gb.beta_h(t, phi, l, 4)
            assert len(got) == 5 and len(gb.beta_h(t, phi, l, order=2)) == 3
            rf = ref.h_derivs(t, phi, l)
            for i, ti in enumerate(t):
                want = [float(c) for c in _mp_derivs(mp.mpf(float(ti)), phi, l)]
                e = np.exp(-abs(ti))
                v2 = 2.0 * e / ((1.0 + e) * (1.0 + e))                  # 2 sigma'(t)
                for k in range(5):
                    scale = max(abs(want[k]), 1.0 if k < 2 else v2)
                    worst[k] = max(worst[k], abs(got[k][i] - want[k]) / scale)
                    worst_ref[k] = max(worst_ref[k], abs(rf[k][i] - want[k]) / scale)
    print('per node h^(k), k = 0..4, on [-40, 40], host:', worst, ' reference:', worst_ref)
    assert np.all(worst <= NODE) and np.all(worst_ref <= NODE)


def test_evaluator_against_mpmath(gb):
    import mpmath as mp
    mp.mp.dps = 50
    x = np.concatenate([np.linspace(1.0, 12.0, 221), np.exp(np.linspace(np.log(12.0), np.log(1e6), 80)), [1.0, 2.0, 9.999999, 10.0, 1e6]])
    got = gb.polygamma_ge1(x)
    assert gb.POLYGAMMA_SHIFT_TO == 10.0 and gb.POLYGAMMA_SHIFT_STEPS == 9        # the kernels' constants
    worst = np.zeros(5)
    for i, xi in enumerate(x):
        xm = mp.mpf(float(xi))
        want = [mp.loggamma(xm)] + [mp.polygamma(j, xm) for j in range(4)]
        for k in range(5):
            scale = max(abs(want[k]), 1) if k == 0 else abs(want[k])
            worst[k] = max(worst[k], float(abs(mp.mpf(float(got[k][i])) - want[k]) / scale))
    print('lgamma, psi .. psi\'\'\' on [1, 1e6], relative:', worst)
    assert np.all(worst <= EVAL)
    assert len(gb.polygamma_ge1(x, order=2)) == 3


def test_mirror_identity(gb):
    """h(t; l) = h(-t; -l) - phi l: sigma(t) = 1 - sigma(-t) swaps the two lgamma terms and -phi l sigma(t) = -phi l + phi l sigma(-t).
    Derivatives: h^(k)(t; l) = (-1)^k h^(k)(-t; -l), k >= 1."""
    t = np.linspace(-40.0, 40.0, 161)
    for phi in PHI:
        for l in L:
            a, b = gb.beta_h(t, phi, l), gb.beta_h(-t, phi, -l)
            assert np.all(np.abs(a[0] - (b[0] - phi * l)) <= IDENT * np.maximum(np.abs(a[0]), abs(phi * l)))
            for k in range(1, 5):
                assert np.all(np.abs(a[k] - (-1) ** k * b[k]) <= IDENT * np.max(np.abs(a[k])))
    rho, s, phi, l = _points()
    gx, gw = _gh()
    a, b = gb.beta_expected_h(rho, s, l, phi, gx, gw), gb.beta_expected_h(-rho, s, -l, phi, gx, gw)
    assert np.all(np.abs(a[0] - (b[0] - phi * l)) <= IDENT * np.maximum(np.abs(a[0]), np.abs(phi * l)))
    for k in range(1, 5):
        assert np.all(np.abs(a[k] - (-1) ** k * b[k]) <= IDENT * np.abs(a[k]))


def test_tails_are_finite_and_linear(gb):
    """No finite point is refused: at |t| = 2000, h = |t| + lgamma(1 + phi) - 2 log phi - [t > 0] phi l, h' = +-1 - [..] 0, the rest 0."""
    from scipy.special import gammaln
    for phi, l in ((0.3, -8.0), (15.0, 0.4), (3000.0, 3.0)):
        for t in (-2000.0, 2000.0):
            h = gb.beta_h(np.array([t]), phi, l)
            want = abs(t) + gammaln(1.0 + phi) - 2.0 * np.log(phi) - (phi * l if t > 0 else 0.0)
            assert abs(h[0][0] - want) <= 1e-14 * abs(want) and h[1][0] == np.sign(t) and all(a[0] == 0.0 for a in h[2:])


def test_single_node_known_answer(gb):
    """With one node (gh_deg = 1: t = rho) sum w h(rho) - log_norm_const is minus the weighted Beta log-density."""
    from scipy.stats import beta as beta_dist
    rng = np.random.default_rng(5)
    n = 200
    rho, phi, w = rng.normal(size=n) * 3.0, np.exp(rng.uniform(np.log(0.5), np.log(1e3), size=n)), rng.uniform(0.5, 1.5, size=n)
    mu = 1.0 / (1.0 + np.exp(-rho))
    y = np.clip(rng.beta(mu * phi, (1.0 - mu) * phi), 1e-12, 1.0 - 1e-12)
    gx, gw = _gh(1)
    e = gb.beta_expected_h(rho, np.full(n, 0.7), np.log(y) - np.log1p(-y), phi, gx, gw)
    got = np.sum(w * e[0]) - ref.log_norm_const(y, phi, w)
    want = -np.sum(w * beta_dist.logpdf(y, mu * phi, (1.0 - mu) * phi))
    print('single node known answer', got, want)
    assert abs(got - want) <= 1e-12 * abs(want)


def test_row_derivs_against_finite_differences(gb):
    rho, s, phi, l = _points()
    keep = (np.abs(rho) <= 12.0) & (s > 0.0)
    rho, s, phi, l = rho[keep], s[keep], phi[keep], l[keep]
    gx, gw = _gh()
    f = lambda r, v: gb.beta_expected_h(r, v, l, phi, gx, gw)
    e = f(rho, s)
    a1, a2 = gb.beta_row_derivs(rho, s, l, phi, gx, gw)
    d = 1e-4
    fd_rho = (f(rho + d, s) - f(rho - d, s)) / (2 * d)
    fd_s = (f(rho, s + d) - f(rho, s - d)) / (2 * d)
    # Stein's identity on the nodes: d_rho E h^(k) = E h^(k+1) exactly, d_s E h^(k) = E h^(k+2) / 2 up to the quadrature error
    for k in range(4):
        scale = np.maximum(np.abs(e[k + 1]), np.abs(e[k]))
        assert np.all(np.abs(fd_rho[k] - e[k + 1]) <= 1e-6 * scale + 1e-9)
    assert np.all(np.abs(fd_rho[0] - a1) <= 1e-6 * np.maximum(np.abs(a1), np.abs(e[0])) + 1e-9)
    smooth = s <= 0.5                                                    # where 20 nodes resolve h'' (the rule is exact to degree 39)
    assert np.all(np.abs(fd_s[0] - a2)[smooth] <= 1e-5 * np.maximum(np.abs(a2), 1.0)[smooth])


def test_response_mean(gb):
    rho, s, _, _ = _points()
    gx, gw = _gh()
    got = gb.beta_response_mean(rho, s, gx, gw)
    assert np.all(np.abs(got - ref.response_mean(rho, s)) <= 1e-14 * got) and np.all((got > 0.0) & (got < 1.0))


def test_constructor_refusals(gb):
    """Every check runs before the device context is created, so no GPU is needed."""
    import lrvb_amd as vb
    n = 6
    x, z, gid = np.ones((n, 2)), np.ones((n, 1)), np.zeros(n, dtype=np.int64)
    y = np.full(n, 0.3)
    for bad, count in ((0.0, 1), (1.0, 1), (np.nan, 1), (-0.2, 1), (1.5, 1), (np.inf, 1)):
        yy = y.copy()
        yy[3] = bad
        with pytest.raises(ValueError, match=r'{} of {} rows'.format(count, n)):
            vb.BetaGLMMObjective(None, x, yy, z, gid, 1, 2.0)
    yy = y.copy()
    yy[[0, 4]] = 0.0, 1.0
    with pytest.raises(ValueError, match='2 of 6 rows'):
        vb.BetaGLMMObjective(None, x, yy, z, gid, 1, 2.0)
    for phi in (0.0, -1.0, np.nan, np.inf, np.ones(n - 1), np.r_[np.ones(n - 1), 0.0]):
        with pytest.raises(ValueError, match='dispersion'):
            vb.BetaGLMMObjective(None, x, y, z, gid, 1, phi)
    with pytest.raises(ValueError, match='offset'):
        vb.BetaGLMMObjective(None, x, y, z, gid, 1, 2.0, offset=np.zeros(n + 1))

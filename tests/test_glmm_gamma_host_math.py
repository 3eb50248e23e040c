"""The Gamma mixed model on the CPU: the torch reference tests/glmm_gamma_reference.py and the host forms of
linearresponsevariationalbayes.py_amd/glmm_gamma.py against mpmath, and the preconditions of the GPU parity tests.  No device.

Exact values.  E h^(k), h(t) = phi (y e^{-t} + t), t ~ N(rho, s), is [g + phi rho, phi - g, g, -g, g] with g = phi exp(log y - rho +
s / 2), evaluated by mpmath at 40 digits (`_exact`; the precision is set per function and restored); `test_exact_moments_are_independent` shows by mpmath QUADRATURE of h^(k) against
the Gaussian density that this is the expectation, so that the closed form pinned below is not merely compared with itself.

Error measure.  An error of E h^(k) is taken over the size of its terms: max(g, phi |rho|) for the value, max(phi, g) for
a1 = phi - g (a difference: no method holds it relative to the result where g is next to phi), g for the three others.  `CAP` = 1e-10
is the cap of the other families (tests/test_glmm_beta_host_math.py).

Where the reference meets the cap.  The 96-node rule sums exp(-sqrt(2 s) x) against the Gauss-Hermite weights; the factor
exp(log y - rho) stands outside the sum, so the error depends on s alone.  Measured here on a grid: 1e-14 or better up to s = 100,
for rho in [-40, 40] and log y in [-30, 30]; 3e-8 at s = 200.  The data sets of the GPU tests have s < 2.5 and |rho| < 32, and the
reference is pinned at EVERY one of their rows, in both variants, below."""
import mpmath as mp
import numpy as np
import pytest

import glmm_gamma_reference as ref

CAP, HOST = 1e-10, 1e-13
DPS = 40                                                                 # set per function (mp.workdps): no other test's precision is touched


@pytest.fixture(scope='module')
def gg():
    from lrvb_amd import glmm_gamma
    return glmm_gamma


def _at_dps(fn):
    """Runs a test at DPS digits of mpmath and restores the caller's precision."""
    import functools

    @functools.wraps(fn)
    def run(*a, **k):
        with mp.workdps(DPS):
            return fn(*a, **k)
    return run


@_at_dps
def _exact(rho, s, ly, phi):
    """E h^(k), k = 0..4, and the error scales (5 x n each) by mpmath."""
    out, scale = [], []
    for r, v, l, p in zip(*np.broadcast_arrays(rho, s, ly, phi)):
        r, v, l, p = mp.mpf(float(r)), mp.mpf(float(v)), mp.mpf(float(l)), mp.mpf(float(p))
        g = p * mp.exp(l - r + v / 2)
        out.append([float(a) for a in (g + p * r, p - g, g, -g, g)])
        scale.append([float(a) for a in (max(g, p * abs(r)), max(p, g), g, g, g)])
    return np.array(out).T, np.array(scale).T


def _rows(N, P, K, G, centred):
    """(rho, s, log y, phi) of every row of a GPU test shape at the point of `problem`."""
    x, y, z, w, gid, o, ph, free = ref.shape_data(N, P, K, G, centred)
    eta = ref.free_to_vec(__import__('torch').tensor(free), P, K, G).numpy()
    ng, GK = 2 * P + 4 * K, G * K
    m, v, e, r = eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + GK].reshape(G, K), 1.0 / eta[ng + GK:].reshape(G, K)
    return o + x @ m + np.sum(z * e[gid], axis=1), (x * x) @ v + np.sum(z * z * r[gid], axis=1), np.log(y), ph


@_at_dps
def test_exact_moments_are_independent():
    """mpmath quadrature of h^(k)(t) N(t; rho, s) against the closed form, at points that cover small and large s, both signs of
    rho and the probe responses."""
    for rho, s, ly, phi in ((0.3, 0.5, 0.0, 1.0), (-2.0, 4.0, np.log(1e-12), 7.5), (27.0, 2.0, np.log(1e12), 0.05), (1.5, 30.0, 0.7, 1e4)):
        want, scale = _exact([rho], [s], [ly], [phi])
        r, v, l, p = (mp.mpf(float(a)) for a in (rho, s, ly, phi))
        dens = lambda t: mp.exp(-(t - r) ** 2 / (2 * v)) / mp.sqrt(2 * mp.pi * v)
        hk = [lambda t: p * (mp.exp(l - t) + t), lambda t: p * (1 - mp.exp(l - t)), lambda t: p * mp.exp(l - t),
              lambda t: -p * mp.exp(l - t), lambda t: p * mp.exp(l - t)]
        sd = mp.sqrt(v)
        cuts = [r + j * sd for j in range(-40, 41, 4)]
        for k in range(5):
            got = mp.quad(lambda t: hk[k](t) * dens(t), cuts)
            assert abs(float(got) - want[k, 0]) <= 1e-20 * scale[k, 0] + 1e-15 * scale[k, 0]


@pytest.mark.parametrize('centred', [True, False])
@pytest.mark.parametrize('N,P,K,G', ref.SHAPES)
def test_reference_meets_the_cap_at_every_row_of_the_test_problems(N, P, K, G, centred):
    """Every row of every GPU test shape, both variants: |rho| < 32, s < 2.5 (asserted), the reference's E h^(k) within 1e-10."""
    rho, s, ly, ph = _rows(N, P, K, G, centred)
    assert np.max(np.abs(rho)) < 32.0 and np.max(s) < 2.5
    got = ref.eh_coefs(rho, s, ly, ph)
    want, scale = _exact(rho, s, ly, ph)
    err = np.abs(got - want) / scale
    print('reference against mpmath', (N, P, K, G), 'centred' if centred else 'raw', 'largest |rho|', float(np.max(np.abs(rho))), 'largest s',
          float(np.max(s)), 'errors by order', err.max(axis=1))
    assert got.shape == want.shape and np.all(err <= CAP)


def test_reference_and_host_forms_against_mpmath_on_a_grid(gg):
    """rho in [-40, 40], s in [0, 100], log y in [-30, 30], phi in [1e-3, 1e8]: the reference within CAP (the range stated in the
    module docstring), the host forms within HOST = 1e-13 (one exp of an argument of size up to 120: (|A| + 2) ulp)."""
    rng = np.random.default_rng(5)
    n = 400
    rho, s = rng.uniform(-40.0, 40.0, size=n), np.concatenate([[0.0, 100.0], rng.uniform(0.0, 100.0, size=n - 2)])
    ly, ph = rng.uniform(-30.0, 30.0, size=n), np.exp(rng.uniform(np.log(1e-3), np.log(1e8), size=n))
    want, scale = _exact(rho, s, ly, ph)
    e_ref = np.abs(ref.eh_coefs(rho, s, ly, ph) - want) / scale
    e_host = np.abs(gg.gamma_expected_h(rho, s, ly, ph) - want) / scale
    print('grid: reference', e_ref.max(axis=1), 'host forms', e_host.max(axis=1))
    assert np.all(e_ref <= CAP) and np.all(e_host <= HOST)
    a1, a2 = gg.gamma_row_derivs(rho, s, ly, ph)
    assert np.array_equal(a1, gg.gamma_expected_h(rho, s, ly, ph)[1]) and np.array_equal(a2, 0.5 * gg.gamma_expected_h(rho, s, ly, ph)[2])
    # past s = 100 the reference leaves the cap: it is stated, not hidden
    far = np.abs(ref.eh_coefs([0.3], [200.0], [0.0], [1.0]) - _exact([0.3], [200.0], [0.0], [1.0])[0])[2, 0] / _exact([0.3], [200.0], [0.0], [1.0])[1][2, 0]
    print('reference at s = 200', far)
    assert far > CAP


def test_five_coefficients_against_finite_differences(gg):
    """a1 = d_rho E h, a2 = d_s E h, c11 = d_rho^2, c12 = d_rho d_s, c22 = d_s^2 of the host value, by central differences in mpmath-free
    fp64 at a step of 1e-4 (truncation 1e-8, rounding 1e-12 of the value): 1e-6 of the largest term."""
    rho, s, ly, ph = np.array([0.4, -1.3, 2.0]), np.array([0.7, 1.9, 0.2]), np.array([0.3, -2.0, 1.1]), np.array([2.5, 0.05, 40.0])
    E = lambda r, v: gg.gamma_expected_h(r, v, ly, ph)[0]
    e = gg.gamma_expected_h(rho, s, ly, ph)
    h = 1e-4
    fd = dict(a1=(E(rho + h, s) - E(rho - h, s)) / (2 * h), a2=(E(rho, s + h) - E(rho, s - h)) / (2 * h),
              c11=(E(rho + h, s) - 2 * E(rho, s) + E(rho - h, s)) / (h * h), c22=(E(rho, s + h) - 2 * E(rho, s) + E(rho, s - h)) / (h * h),
              c12=(E(rho + h, s + h) - E(rho + h, s - h) - E(rho - h, s + h) + E(rho - h, s - h)) / (4 * h * h))
    want = dict(a1=e[1], a2=0.5 * e[2], c11=e[2], c12=0.5 * e[3], c22=0.25 * e[4])
    scale = np.maximum(ph, e[2])
    for k in fd:
        assert np.all(np.abs(fd[k] - want[k]) <= 1e-6 * scale), k
    assert np.all(want['c12'] < 0.0)                                     # the sign that sets this model apart from the Poisson one


@_at_dps
def test_shape_terms_against_mpmath(gg):
    """phi (log phi - psi(phi)) and phi (1 - phi psi'(phi)) to 1e-14 relative on [1e-3, 1e12], the threshold and its neighbours
    included; and what the defining forms lose, so that the series is seen to be needed."""
    from scipy.special import digamma, polygamma
    phis = np.concatenate([10.0 ** np.linspace(-3.0, 12.0, 601), [1.0, 2.0, gg.SHAPE_SERIES_FROM, np.nextafter(gg.SHAPE_SERIES_FROM, 0.0),
                                                                 np.nextafter(gg.SHAPE_SERIES_FROM, 100.0), 15.0, 17.0, 1e3, 1e6, 1e9]])
    t1, t2 = gg.gamma_shape_terms(phis)
    worst = [0.0, 0.0]
    for p, a, b in zip(phis, t1, t2):
        P = mp.mpf(float(p))
        e1, e2 = P * (mp.log(P) - mp.digamma(P)), P * (1 - P * mp.polygamma(1, P))
        worst = [max(worst[0], float(abs((mp.mpf(float(a)) - e1) / e1))), max(worst[1], float(abs((mp.mpf(float(b)) - e2) / e2)))]
    print('gamma_shape_terms: largest relative errors', worst)
    assert max(worst) <= 1e-14
    assert gg.gamma_shape_terms(np.array([[2.0, 3.0]]))[0].shape == (1, 2) and np.ndim(gg.gamma_shape_terms(4.0)[0]) == 0
    naive = lambda p: (p * (np.log(p) - digamma(p)), p * (1.0 - p * polygamma(1, p)))
    lost = [abs(naive(p)[0] - float(mp.mpf(p) * (mp.log(p) - mp.digamma(p)))) / 0.5 for p in (1e6, 1e9)]
    print('the defining form of T1 at 1e6, 1e9 loses', lost)
    assert lost[1] > 1e-9


@_at_dps
def test_log_norm_const_derivatives_by_differences(gg):
    """C(lambda) = phi log phi - lgamma(phi) + (phi - 1) log y at phi = e^lambda phi0 in mpmath: C_l = T1 + phi + phi log y and
    C_ll = T1 + T2 + phi + phi log y."""
    for phi0, ly in ((0.3, -2.0), (7.5, 0.4), (2e3, 27.0)):
        C = lambda lam: (lambda p: p * mp.log(p) - mp.loggamma(p) + (p - 1) * mp.mpf(ly))(mp.mpf(phi0) * mp.exp(lam))
        t1, t2 = (float(a) for a in gg.gamma_shape_terms(phi0))
        c1, c2 = t1 + phi0 * (1.0 + ly), t1 + t2 + phi0 * (1.0 + ly)
        assert abs(float(mp.diff(C, 0)) - c1) <= 1e-12 * (abs(c1) + phi0) and abs(float(mp.diff(C, 0, 2)) - c2) <= 1e-10 * (abs(c2) + phi0)


def test_value_minus_constant_is_the_gamma_density(gg):
    """One row: E h - [phi log phi - lgamma(phi) + (phi - 1) log y] = E_q of -scipy.stats.gamma.logpdf(y, a=phi, scale=e^t / phi),
    the expectation on the reference's 96 nodes."""
    from scipy.stats import gamma as gamma_dist
    from scipy.special import gammaln
    gx, gw = np.polynomial.hermite.hermgauss(ref.GH_DEG)
    for rho, s, y, phi in ((0.3, 0.5, 2.2, 3.0), (-1.0, 2.0, 1e-3, 0.4), (4.0, 0.1, 300.0, 55.0)):
        t = rho + np.sqrt(2.0 * s) * gx
        want = np.sum(gw / np.sqrt(np.pi) * -gamma_dist.logpdf(y, a=phi, scale=np.exp(t) / phi))
        got = gg.gamma_expected_h(rho, s, np.log(y), phi)[0] - (phi * np.log(phi) - gammaln(phi) + (phi - 1.0) * np.log(y))
        assert abs(got - want) <= 1e-12 * max(abs(want), phi * abs(rho), 1.0)


def test_response_mean_and_overflow(gg):
    rho, s = np.array([0.3, -5.0, 12.0]), np.array([0.5, 3.0, 1.0])
    assert np.allclose(gg.gamma_response_mean(rho, s), ref.response_mean(rho, s), rtol=1e-13, atol=0)
    e = gg.gamma_expected_h(-800.0, 0.5, 0.0, 2.0)
    assert np.isinf(e[0]) and np.isinf(e[2])                             # the overflow the entry refuses
    e = gg.gamma_expected_h(800.0, 0.5, 0.0, 2.0)
    assert e[0] == 1600.0 and e[1] == 2.0 and e[2] == 0.0                # the underflow it accepts: h -> phi rho


@pytest.mark.parametrize('N,P,K,G', ref.SHAPES)
def test_parity_preconditions(N, P, K, G):
    """The reference free Hessian at each GPU test shape: positive definite in both variants (the data block is a sum of rank-one
    terms g c c^T); the CENTRED variant is what the covariance and solve checks run on, the RAW one is too ill-conditioned for an
    fp64 inverse to six digits (module docstring of tests/test_gpu_glmm_gamma.py).  The eigenvalues are printed and recorded in
    DESIGN.md section 43."""
    for centred in (True, False):
        if N < 4 and not centred:
            continue
        x, y, z, w, gid, o, ph, free = ref.shape_data(N, P, K, G, centred)
        H = ref.value_grad_hess(ref.kl_free, free, ref.targs(x, y, z, w, o, ph, gid, G, ref.TEST_HYP))[2]
        ev = np.linalg.eigvalsh(H)
        print('reference free Hessian', (N, P, K, G), 'centred' if centred else 'raw', 'smallest eigenvalue', float(ev[0]), 'largest', float(ev[-1]),
              'condition', float(ev[-1] / ev[0]))
        assert ev[0] > 0.1
        # centred: an fp64 inverse keeps nine digits or more, three more than the solve checks ask for
        assert (ev[-1] / ev[0] < 1e7) if centred else (ev[-1] / ev[0] > 1e12)


def test_constructor_refusals_need_no_device(gg):
    """All checks run before the device context is created: y <= 0 or not finite, and a bad dispersion, are ValueErrors on a machine
    without a GPU; the text of a zero points to the two-part composite."""
    import lrvb_amd as vb
    N, K, G = 20, 2, 3
    x, z, gid = np.ones((N, 2)), np.ones((N, K)), np.arange(N) % G
    par = lambda: None
    for bad in (0.0, -1.0, np.nan, np.inf):
        y = np.full(N, 0.4)
        y[5] = bad
        with pytest.raises(ValueError, match='1 of 20 rows.*HurdleGammaGLMM'):
            vb.GammaGLMMObjective(par(), x, y, z, gid, G, 2.0)
    for phi in (0.0, -3.0, np.inf, np.ones(N + 1)):
        with pytest.raises(ValueError, match='dispersion'):
            vb.GammaGLMMObjective(par(), x, np.full(N, 0.4), z, gid, G, phi)
    with pytest.raises(ValueError, match='dispersion'):
        vb.HurdleGammaGLMM(par(), par(), x, np.full(N, 0.4), z, gid, G, -1.0)
    with pytest.raises(ValueError, match='>= 0'):
        vb.HurdleGammaGLMM(par(), par(), x, np.full(N, -0.4), z, gid, G, 1.0)
    assert vb.GammaGLMMObjective.__mro__[1].__name__ == '_LogDispersion'

"""The censored Gaussian mixed model on the CPU: the torch reference tests/glmm_censnormal_reference.py and the
host forms of linearresponsevariationalbayes.py_amd/glmm_censored.py against mpmath, and the preconditions of the GPU parity tests.
No device.

Exact values.  Observed rows: E h^(k) of h = phi (y - t)^2 / 2 is [phi ((y - rho)^2 + s) / 2, -phi (y - rho), phi, 0, 0], shown by
mpmath QUADRATURE of h^(k) against the Gaussian density.  Censored rows: h = -log Phi(a), a = delta r (t - y), r = sqrt(phi); its
derivatives in t and in lambda (phi = e^lambda phi0) are evaluated at 60 digits by `_Hk` and `_lam_k`, where the cancellations of
the left tail (a^4 ulp at worst) cost nothing, and `test_exact_forms_are_the_derivatives` shows by `mpmath.diff` of the ONE
expression -log Phi(delta sqrt(phi0 e^lambda) (t - y)) that these are its derivatives, so that the forms pinned below are not merely
compared with themselves.  The model's expectation is their sum over the Gauss-Hermite nodes (the quadrature is part of the model
there, as for the probit link); that the node sum converges to the integral is shown by mpmath quadrature too.

Error measure.  An error of E h^(k) of a censored row is taken over the size of the terms of H^(k) on the nodes (`_Hk`): with
l = phi / Phi the inverse Mills ratio, d = a + l and w = l d these are H, l, w, l + w |d| and (l + w |d|)(|d| + l) + 2 w -- the value and
the first two derivatives are measured relative to themselves, the last two over their terms, which cancel in the left tail where
no method holds them relative to the result.  Observed rows: relative to phi ((y - rho)^2 + s) / 2, phi |y - rho| and phi.
`CAP` = 1e-10 is the cap of the other families (tests/test_glmm_gamma_host_math.py).

Where the reference meets the cap.  Everything about a censored row depends on (r (rho - y), phi s) alone: the argument on node k is
a_k = r (rho - y) + sqrt(phi s) x_k, and the factors (delta r)^k are exact powers.  GRID: |r (rho - y)| <= 16, phi s <= 40, phi in
[0.25, 16], both statuses.  Measured there: 2e-11 at worst (the fourth derivative; nested autograd of log_ndtr loses a^2 ulp per
order in the left tail), the host forms 2e-14.  At phi s = 100 the reference is still at 5e-11; it is not relied on there.  Every row
of every GPU data set is asserted to lie inside GRID below."""
import mpmath as mp
import numpy as np
import pytest
import torch

import glmm_censnormal_reference as ref

CAP, HOST = 1e-10, 1e-13
DPS = 60
GRID = dict(ru=16.0, phis=40.0, phi=(0.25, 16.0))
GX, GW = np.polynomial.hermite.hermgauss(ref.GH_DEG)


@pytest.fixture(scope='module')
def gc():
    import lrvb_amd
    from lrvb_amd import glmm_censored
    assert hasattr(glmm_censored, 'censnormal_expected_h') and hasattr(lrvb_amd, 'CensoredNormalGLMMObjective')
    return glmm_censored


def _at_dps(fn):
    """Runs a test at DPS digits of mpmath and restores the caller's precision."""
    import functools

    @functools.wraps(fn)
    def run(*a, **k):
        with mp.workdps(DPS):
            return fn(*a, **k)
    return run


def _mpf(a):
    return mp.mpf(float(a))


def _H(a):
    """-log Phi(a) at full precision on both sides."""
    return -mp.log(mp.ncdf(a)) if a < 0 else -mp.log1p(-mp.ncdf(-a))


def _Hk(a):
    """([H, H', H'', H''', H''''], the sizes of their terms) at a, H = -log Phi, at the working precision."""
    l = mp.npdf(a) / mp.ncdf(a)
    d = a + l
    w = l * d
    w1 = l * (1 - w) - w * d
    t3 = l + w * abs(d)
    return [_H(a), -l, w, w1, -w1 * (d + l) - 2 * w * (1 - w)], [_H(a), l, w, t3, t3 * (abs(d) + l) + 2 * w]


def _lam_k(a, dr, H):
    """(h_l, d_t h_l, d_t^2 h_l, h_ll) of h = H(a), a = delta r (t - y), r^2 = phi0 e^lambda: d a / d lambda = a / 2."""
    return [a * H[1] / 2, dr * (a * H[2] + H[1]) / 2, dr * dr * (a * H[3] + 2 * H[2]) / 2, a * (a * H[2] + H[1]) / 4]


@_at_dps
def test_exact_forms_are_the_derivatives(gc):
    """`_Hk` and `_lam_k` against mpmath.diff of -log Phi(delta sqrt(phi0 e^lambda) (t - y)) in t and in lambda: both statuses, both
    tails, 1e-25 of the size of the terms (mpmath.diff at 60 digits holds about 30)."""
    for t, yy, p, d in ((0.3, 0.1, 1.0, 1), (-9.0, 0.4, 4.0, 1), (7.0, 0.5, 0.25, 1), (-1.0, 0.8, 16.0, -1), (6.0, -3.0, 9.0, -1), (-25.0, 1.0, 2.0, 1)):
        t, yy, p = _mpf(t), _mpf(yy), _mpf(p)
        f = lambda tt, lam: _H(d * mp.sqrt(p * mp.exp(lam)) * (tt - yy))
        dr = d * mp.sqrt(p)
        a = dr * (t - yy)
        H, T = _Hk(a)
        for k in range(1, 5):
            got = mp.diff(lambda tt: f(tt, mp.mpf(0)), t, k)
            assert abs(got - dr ** k * H[k]) <= mp.mpf(10) ** -25 * abs(dr) ** k * T[k], (t, k)
        sizes = [abs(a) * T[1], abs(dr) * (abs(a) * T[2] + T[1]), p * (abs(a) * T[3] + 2 * T[2]), abs(a) * (abs(a) * T[2] + T[1])]
        for i, order in enumerate(((0, 1), (1, 1), (2, 1), (0, 2))):
            got = mp.diff(f, (t, mp.mpf(0)), order)
            assert abs(got - _lam_k(a, dr, H)[i]) <= mp.mpf(10) ** -25 * sizes[i], (t, order)


@_at_dps
def _exact(rho, s, y, phi, st, gx=GX, gw=GW):
    """E h^(k), k = 0..4, and the error scales (5 x n each): censored rows on the nodes by `_Hk`, observed rows in closed form."""
    out, scale = [], []
    for r, v, yy, p, d in zip(*np.broadcast_arrays(rho, s, y, phi, st)):
        r, v, yy, p = _mpf(r), _mpf(v), _mpf(yy), _mpf(p)
        if d == 0:
            u = r - yy
            out.append([float(a) for a in (p * (u * u + v) / 2, p * u, p, 0, 0)])
            scale.append([float(a) for a in (p * (u * u + v) / 2, max(p * abs(u), p * mp.sqrt(v), mp.mpf(10) ** -300), p, p, p)])
            continue
        dr = int(d) * mp.sqrt(p)
        E, S = [mp.mpf(0)] * 5, [mp.mpf(0)] * 5
        for xk, wk in zip(gx, gw):
            t = r + mp.sqrt(v) * mp.sqrt(2) * _mpf(xk)
            wq = _mpf(wk) / mp.sqrt(mp.pi)
            H, sz = _Hk(dr * (t - yy))
            for k in range(5):
                E[k] += wq * H[k] * dr ** k
                S[k] += wq * sz[k] * abs(dr) ** k
        out.append([float(a) for a in E])
        scale.append([float(a) for a in S])
    return np.array(out).T, np.array(scale).T


@_at_dps
def _exact_dispersion(rho, s, y, phi, st, gx=GX, gw=GW):
    """(E h_l, E d_t h_l, E d_t^2 h_l, E h_ll) and scales (4 x n): `_lam_k` on the nodes, observed rows in closed form."""
    out, scale = [], []
    for r, v, yy, p, d in zip(*np.broadcast_arrays(rho, s, y, phi, st)):
        r, v, yy, p = _mpf(r), _mpf(v), _mpf(yy), _mpf(p)
        if d == 0:
            u = r - yy
            eh = p * (u * u + v) / 2
            out.append([float(a) for a in (eh, p * u, p, eh)])
            scale.append([float(a) for a in (eh, max(p * abs(u), p * mp.sqrt(v), mp.mpf(10) ** -300), p, eh)])
            continue
        E, S = [mp.mpf(0)] * 4, [mp.mpf(0)] * 4
        for xk, wk in zip(gx, gw):
            t = r + mp.sqrt(v) * mp.sqrt(2) * _mpf(xk)
            wq = _mpf(wk) / mp.sqrt(mp.pi)
            dr = int(d) * mp.sqrt(p)
            a = dr * (t - yy)
            H, sz = _Hk(a)
            for i, val in enumerate(_lam_k(a, dr, H)):
                E[i] += wq * val
            rr = mp.sqrt(p)
            for i, val in enumerate((abs(a) * sz[1], rr * (abs(a) * sz[2] + sz[1]), p * (abs(a) * sz[3] + 2 * sz[2]), abs(a) * (abs(a) * sz[2] + sz[1]))):
                S[i] += wq * val
        out.append([float(a) for a in E])
        scale.append([float(a) for a in S])
    return np.array(out).T, np.array(scale).T


def _rows(N, P, K, G, mode):
    """(rho, s, y, phi, st) of every row of a GPU test shape at the point of `problem`."""
    x, y, z, w, gid, o, ph, st, free = ref.shape_data(N, P, K, G, mode)
    eta = ref.free_to_vec(torch.tensor(free), P, K, G).numpy()
    ng, GK = 2 * P + 4 * K, G * K
    m, v, e, r = eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + GK].reshape(G, K), 1.0 / eta[ng + GK:].reshape(G, K)
    return o + x @ m + np.sum(z * e[gid], axis=1), (x * x) @ v + np.sum(z * z * r[gid], axis=1), y, ph, st


def _inside_grid(rho, s, y, ph):
    return (np.max(np.abs(np.sqrt(ph) * (rho - y))) <= GRID['ru'] and np.max(ph * s) <= GRID['phis']
            and ph.min() >= GRID['phi'][0] and ph.max() <= GRID['phi'][1])


@_at_dps
def test_exact_moments_are_independent(gc):
    """mpmath quadrature of h^(k)(t) N(t; rho, s): the observed closed form IS the expectation (1e-15), and the censored node sum
    converges to it -- at 96 nodes to 1e-7 of the size of the terms (-log Phi is not entire: the rule converges algebraically, which is
    why the quadrature is part of the model's definition and the reference runs on the class's own nodes)."""
    gx, gw = np.polynomial.hermite.hermgauss(96)
    for rho, s, y, phi, d in ((0.3, 0.5, 0.1, 1.0, 0), (-2.0, 4.0, 3.0, 7.5, 0), (0.3, 0.5, 0.1, 1.0, 1), (-1.0, 0.8, 0.4, 4.0, -1), (2.0, 0.3, 0.5, 0.25, 1)):
        r, v, yy, p = (_mpf(a) for a in (rho, s, y, phi))
        dens = lambda t: mp.exp(-(t - r) ** 2 / (2 * v)) / mp.sqrt(2 * mp.pi * v)
        if d == 0:
            hk = [lambda t: p * (yy - t) ** 2 / 2, lambda t: -p * (yy - t), lambda t: p, lambda t: mp.mpf(0), lambda t: mp.mpf(0)]
        else:
            dr = d * mp.sqrt(p)
            hk = [(lambda t, k=k: _Hk(dr * (t - yy))[0][k] * dr ** k) for k in range(5)]
        sd = mp.sqrt(v)
        cuts = [r + j * sd for j in range(-40, 41, 4)]
        got = gc.censnormal_expected_h([rho], [s], [y], [phi], [d], gx, gw)[:, 0]
        for k in range(5):
            want = float(mp.quad(lambda t: hk[k](t) * dens(t), cuts))
            assert abs(got[k] - want) <= (1e-15 if d == 0 else 1e-7) * max(abs(want), float(p) ** (k / 2)), (rho, s, y, phi, d, k, got[k], want)


@pytest.mark.parametrize('mode', ref.MODES)
@pytest.mark.parametrize('N,P,K,G', ref.SHAPES)
def test_reference_meets_the_cap_at_every_row_of_the_test_problems(gc, N, P, K, G, mode):
    """Every row of every GPU data set lies inside GRID (asserted), and the reference's E h^(k) is within 1e-10 there."""
    rho, s, y, ph, st = _rows(N, P, K, G, mode)
    assert _inside_grid(rho, s, y, ph)
    if mode == 'mixed' and N >= 30:
        share = np.mean(st != 0)
        assert 0.15 <= share <= 0.45 and np.any(st == 1) and np.any(st == -1)
    if mode == 'censored':
        assert np.all(st != 0)
    if mode == 'observed':
        assert np.all(st == 0)
    got = ref.eh_coefs(rho, s, y, ph, st)
    want, scale = _exact(rho, s, y, ph, st)
    err = np.abs(got - want) / scale
    print('reference against mpmath', (N, P, K, G), mode, 'largest |r (rho - y)|', float(np.max(np.abs(np.sqrt(ph) * (rho - y)))),
          'largest phi s', float(np.max(ph * s)), 'errors by order', err.max(axis=1))
    assert got.shape == want.shape and np.all(err <= CAP)


def test_reference_and_host_forms_against_mpmath_on_the_grid(gc):
    """GRID of the module docstring, corners included: the reference within CAP, the host forms within HOST = 1e-13."""
    rng = np.random.default_rng(5)
    n = 90
    ru, ps = rng.uniform(-GRID['ru'], GRID['ru'], size=n), rng.uniform(0.0, GRID['phis'], size=n)
    ph = np.exp(rng.uniform(np.log(GRID['phi'][0]), np.log(GRID['phi'][1]), size=n))
    st = rng.choice([-1, 0, 1], size=n, p=[0.4, 0.2, 0.4])
    ru[:4], ps[:4], st[:4] = [-16.0, 16.0, -16.0, 16.0], [40.0, 40.0, 0.0, 0.0], [1, 1, -1, -1]
    ph[:2] = GRID['phi']
    y = rng.normal(size=n)
    rho, s = y + ru / np.sqrt(ph), ps / ph
    assert np.max(np.abs(np.sqrt(ph) * (rho - y))) <= GRID['ru'] * (1 + 1e-12) and np.max(ph * s) <= GRID['phis'] * (1 + 1e-12)   # the corners, to rounding
    want, scale = _exact(rho, s, y, ph, st)
    e_ref = np.abs(ref.eh_coefs(rho, s, y, ph, st) - want) / scale
    host = gc.censnormal_expected_h(rho, s, y, ph, st, GX, GW)
    e_host = np.abs(host - want) / scale
    print('grid: reference', e_ref.max(axis=1), 'host forms', e_host.max(axis=1))
    assert np.all(e_ref <= CAP) and np.all(e_host <= HOST)
    a1, a2 = gc.censnormal_row_derivs(rho, s, y, ph, st, GX, GW)
    assert np.array_equal(a1, host[1]) and np.array_equal(a2, 0.5 * host[2])
    assert np.array_equal(gc.censnormal_response_mean(rho, s), rho)      # the latent mean, whatever s and phi


def test_dispersion_moments_against_mpmath_and_central_differences(gc):
    """All four lambda-moments: the host forms against mpmath (1e-12 of the size of their terms), the reference's
    autograd within CAP, and fp64 central differences of the host E h, E h', E h'' in lambda at a step of 1e-4 (truncation 1e-8)."""
    rng = np.random.default_rng(9)
    n = 40
    ru, ps = rng.uniform(-8.0, 8.0, size=n), rng.uniform(0.0, 20.0, size=n)
    ph = np.exp(rng.uniform(np.log(0.25), np.log(16.0), size=n))
    st = rng.choice([-1, 0, 1], size=n, p=[0.4, 0.2, 0.4])
    y = rng.normal(size=n)
    rho, s = y + ru / np.sqrt(ph), ps / ph
    want, scale = _exact_dispersion(rho, s, y, ph, st)
    host = gc.censnormal_dispersion_moments(rho, s, y, ph, st, GX, GW)
    e_host = np.abs(host - want) / scale
    e_ref = np.abs(ref.eh_dispersion(rho, s, y, ph, st) - want) / scale
    print('dispersion moments: host', e_host.max(axis=1), 'reference', e_ref.max(axis=1))
    assert np.all(e_host <= 1e-12) and np.all(e_ref <= CAP)
    h = 1e-4
    E = lambda lam: gc.censnormal_expected_h(rho, s, y, ph * np.exp(lam), st, GX, GW)
    ep, e0, em = E(h), E(0.0), E(-h)
    fd = [(ep[0] - em[0]) / (2 * h), (ep[1] - em[1]) / (2 * h), (ep[2] - em[2]) / (2 * h), (ep[0] - 2 * e0[0] + em[0]) / (h * h)]
    for i in range(4):
        tol = 1e-6 * scale[i] + 1e-15 * np.abs(e0[0]) / (h * h if i == 3 else h)
        assert np.all(np.abs(fd[i] - host[i]) <= tol), i
    # an observed row is linear in phi: h_l = h_ll = h
    o = st == 0
    assert np.array_equal(host[0][o], e0[0][o]) and np.array_equal(host[3][o], e0[0][o]) and np.array_equal(host[1][o], e0[1][o])


def test_five_coefficients_against_finite_differences(gc):
    """a1 = d_rho E h, a2 = d_s E h, c11, c12, c22 of the host value by central differences (96 nodes, so that Stein's identity on
    the nodes is the derivative of the node sum to well below the step's truncation 1e-8): 1e-6 of the largest term."""
    gx, gw = np.polynomial.hermite.hermgauss(96)
    rho, s, y = np.array([0.4, -1.3, 2.0, 0.1, 0.9]), np.array([0.7, 1.9, 0.2, 0.5, 1.1]), np.array([0.3, -2.0, 1.1, 0.6, -0.2])
    ph, st = np.array([2.5, 0.25, 16.0, 1.0, 4.0]), np.array([0, 1, -1, 1, 0])
    E = lambda r, v: gc.censnormal_expected_h(r, v, y, ph, st, gx, gw)[0]
    e = gc.censnormal_expected_h(rho, s, y, ph, st, gx, gw)
    h = 1e-4
    fd = dict(a1=(E(rho + h, s) - E(rho - h, s)) / (2 * h), a2=(E(rho, s + h) - E(rho, s - h)) / (2 * h),
              c11=(E(rho + h, s) - 2 * E(rho, s) + E(rho - h, s)) / (h * h), c22=(E(rho, s + h) - 2 * E(rho, s) + E(rho, s - h)) / (h * h),
              c12=(E(rho + h, s + h) - E(rho + h, s - h) - E(rho - h, s + h) + E(rho - h, s - h)) / (4 * h * h))
    want = dict(a1=e[1], a2=0.5 * e[2], c11=e[2], c12=0.5 * e[3], c22=0.25 * e[4])
    scale = np.maximum(ph * ph, np.abs(e[0]) + 1.0)
    for k in fd:
        assert np.all(np.abs(fd[k] - want[k]) <= 1e-6 * scale), (k, fd[k], want[k])
    assert np.all(want['c12'][st == 0] == 0.0) and np.all(want['c22'][st == 0] == 0.0)
    # the sign of delta in the odd derivatives: a right-censored row pushes t up (a1 < 0), a left-censored one down
    assert np.all(want['a1'][st == 1] < 0.0) and np.all(want['a1'][st == -1] > 0.0)


@pytest.mark.parametrize('N,P,K,G,mode', [s + (m,) for s in ref.SHAPES[:3] for m in ref.MODES] + [s + ('mixed',) for s in ref.SHAPES[3:]])
def test_reference_free_hessian_leaves_six_digits(gc, N, P, K, G, mode):
    """The precondition of the covariance and solve checks of the GPU tests (rtol 1e-6): the reference free Hessian of a data set is
    positive definite with a condition number below 1e8.  All fifteen data sets were computed here once and are tabulated in
    DESIGN.md section 45 (31 to 3.1e3); the two large shapes run in their 'mixed' mode only (the dense autograd Hessian of
    (130, 64, 4, 2) takes most of a minute), and the GPU parity test asserts the same bound on all fifteen."""
    x, y, z, w, gid, o, ph, st, free = ref.shape_data(N, P, K, G, mode)
    t = ref.targs(x, y, z, w, o, ph, gid, G, st, ref.TEST_HYP)
    Hf = ref.value_grad_hess(ref.kl_free, free, t)[2]
    ev = np.linalg.eigvalsh(Hf)
    print('reference free Hessian', (N, P, K, G), mode, 'smallest eigenvalue {:.3g} largest {:.3g} condition {:.2e}'.format(ev[0], ev[-1], ev[-1] / ev[0]))
    assert ev[0] > 0 and ev[-1] / ev[0] < 1e8


def test_constructor_checks_run_before_any_device_context(gc):
    """Everything is validated before the context exists: these refusals need no GPU."""
    import lrvb_amd as vb
    N, P, K, G = 6, 2, 1, 2
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    par.push_param(vb.GammaParam('tau0'))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    x, y, gid = np.ones((N, P)), np.arange(N, dtype=np.float64), np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    make = lambda **kw: vb.CensoredNormalGLMMObjective(par, x, kw.pop('y', y), None, gid, G, kw.pop('dispersion', 1.0), **kw)
    with pytest.raises(ValueError, match='censoring must be None or 6 values in'):
        make(censoring=[0, 1, 2, 0, 0, 0])
    with pytest.raises(ValueError, match='censoring must be None or 6 values in'):
        make(censoring=[0, 1, 0])
    with pytest.raises(ValueError, match='y must be finite'):
        make(y=np.array([0.0, np.inf, 1.0, 2.0, 3.0, 4.0]))
    with pytest.raises(ValueError, match='y must hold 6 values'):
        make(y=np.zeros(5))
    with pytest.raises(ValueError, match='dispersion must be a finite positive scalar or 6'):
        make(dispersion=np.ones(4))
    with pytest.raises(ValueError, match='dispersion must be a finite positive scalar or 6'):
        make(dispersion=0.0)
    with pytest.raises(ValueError, match='offset must hold 6 finite values'):
        make(offset=np.zeros(3))

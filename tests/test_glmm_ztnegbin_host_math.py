"""The zero-truncated NB2 likelihood of the hurdle model without a GPU: the accuracy of the torch reference
tests/glmm_ztnegbin_reference.py against mpmath, the package's module-level host functions (the formulas of the kernels: the
factored chain rule of g = log(1 - exp(-phi softplus))) against both, the phi = 1 identities, and the constructors' refusals.

Moments.  "E H^(k)" below is what the kernels sum on the nodes, (y + phi) E sp^(k) + E g^(k), k = 0..4 (the value and a1 subtract
y rho and y behind it).  Grid: phi in {0.05, 1, 50, 1e3} x rho in {-30, -12, -5, 0.4, 2.5, 5} x s in {0, 0.5, 3, 40}, y = 1 + n mod 7;
the 20 nodes reach eta in [-78, 53].  (rho = 0 is left out: at phi = 1, E H''' = y E sigma'' is exactly 0 there.)

`CAP` = 1e-10 POINTWISE (the error of every E H^(k) over the magnitude of that E H^(k) at that point) is the cap and the measure of
tests/test_glmm_ztpoisson_host_math.py, here on the whole grid.  The factored chain rule alone does not meet it: as eta -> -inf,
H'', H''' and H'''' tend to (y - 1/2 + phi / 2) e^eta while the terms they are formed from stay O(1) (g'' = b - a c with a, b, c -> 1),
so the relative error grows like 1e-16 e^-eta: 3.4e-3, 7.6e-3, 1.7e-2 at orders 2, 3, 4 at rho = -30, s = 0, phi = 0.05 (|exact| =
4.9e-14), and as much in a reference that differentiates log(-expm1(-phi softplus)) by nested autograd.  Kernels and host functions
therefore take g'', g''', g'''' in the corner e^eta < 1e-3, v < 0.01 from two short series (glmm_hurdle.py, `_ztnb_small_m`), and the
reference differentiates two longer polynomials of its own there.  Measured on the whole grid, orders 0..4: host 1.0e-15, 1.0e-15,
1.8e-14, 3.8e-14, 1.2e-13; reference 2.2e-15, 8.3e-16, 1.4e-13, 1.2e-13, 1.1e-11.  `test_expectations_against_mpmath_where_resolvable`
keeps the same cap wherever |exact| >= 1e-5 (now implied) and adds an absolute measure, `ABS` = 3.2e-14 over max(1, |exact|, y + phi)
everywhere -- the g part to 1.6e-14 per node, the (y + phi) sp^(k) part a sum of 20 weighted terms each good to a few ulp of y + phi
(measured 4.8e-16 host, 2.7e-14 reference: k = 4 at phi = 1e3, nested autograd).

Per node.  g^(k) against mpmath.taylor at 50 digits on phi in {0.05, 0.5, 1, 7, 50, 1e3, 1e5} x eta = -36, -35, .., 30, absolute over
max(1, |exact|).  Measured for the committed formulas, k = 0..4: 1.9e-16, 4.3e-16, 4.9e-16, 8.6e-16, 1.2e-15; the bound
`NODE` = 1.2e-14 is ten times the largest.  (The plain recurrence R' = -R (1 + R), .. measures 4.7e-15 at order 4.)"""
import numpy as np
import pytest
import torch

import glmm_ztnegbin_reference as ref

CAP, IDENT, NODE, ABS = 1e-10, 1e-12, 1.2e-14, 3.2e-14
PHI = np.array([0.05, 1.0, 50.0, 1e3])
RHO = np.array([-30.0, -12.0, -5.0, 0.4, 2.5, 5.0])
S = np.array([0.0, 0.5, 3.0, 40.0])


def _points():
    phi, rho, s = np.meshgrid(PHI, RHO, S, indexing='ij')
    phi, rho, s = phi.ravel(), rho.ravel(), s.ravel()
    return phi, rho, s, 1.0 + np.arange(rho.size) % 7.0


def _gh(deg=ref.GH_DEG):
    return np.polynomial.hermite.hermgauss(deg)


@pytest.fixture(scope='module')
def gh():
    import lrvb_amd
    from lrvb_amd import glmm_hurdle
    assert hasattr(glmm_hurdle, 'ztnb_g') and hasattr(lrvb_amd, 'TruncatedNegBinomialGLMMObjective')
    return glmm_hurdle


def _mp_g(phi):
    import mpmath as mp
    return lambda t: mp.log(-mp.expm1(-mp.mpf(float(phi)) * mp.log1p(mp.exp(t))))


@pytest.fixture(scope='module')
def exact():
    """(E H^(k), k = 0..4, 5 x n; the node part E [e^t R(v)] of the response mean, n) at the grid on the 20-node rule, every node
    term from mpmath at 50 digits (mpmath.taylor).  Computed once."""
    import mpmath as mp
    mp.mp.dps = 50
    phi, rho, s, y = _points()
    gx, gw = _gh()
    sp = lambda t: mp.log1p(mp.exp(t))
    e, node = np.zeros((5, rho.size)), np.zeros(rho.size)
    for n in range(rho.size):
        acc, am = [mp.mpf(0)] * 5, mp.mpf(0)
        m = mp.mpf(float(y[n])) + mp.mpf(float(phi[n]))
        for xk, wk in zip(gx, gw):
            t = mp.mpf(float(rho[n])) + mp.sqrt(mp.mpf(float(s[n]))) * mp.sqrt(2) * mp.mpf(float(xk))
            w = mp.mpf(float(wk)) / mp.sqrt(mp.pi)
            c, d = mp.taylor(_mp_g(phi[n]), t, 4), mp.taylor(sp, t, 4)
            for k in range(5):
                acc[k] += w * (m * d[k] + c[k]) * mp.factorial(k)
            am += w * mp.mpf(float(phi[n])) * mp.exp(t) / mp.expm1(mp.mpf(float(phi[n])) * sp(t))
        e[:, n], node[n] = [float(a) for a in acc], float(am)
    return e, node


def _pointwise(got, want):
    """Per derivative order: the largest error over that derivative's own magnitude at the same point."""
    return np.max(np.abs(got - want) / np.abs(want), axis=-1)


def _both(gh):
    phi, rho, s, y = _points()
    gx, gw = _gh()
    return (('reference', ref.eh_coefs(rho, s, y, phi)), ('host', gh.ztnb_expected_H(rho, s, y, phi, gx, gw)))


# ---- accuracy of the reference and of the host functions ---------------------------------------------------------------------
def test_expectations_against_mpmath_pointwise(gh, exact):
    """The cap and measure the model was asked to meet, on the whole grid (module docstring)."""
    for name, got in _both(gh):
        err = _pointwise(got, exact[0])
        print(name, 'E H^(k), k = 0..4, pointwise relative:', err)
    for name, got in _both(gh):
        assert got.shape == exact[0].shape and np.all(_pointwise(got, exact[0]) <= CAP), name


def test_expectations_against_mpmath_where_resolvable(gh, exact):
    e = exact[0]
    phi, rho, s, y = _points()
    assert np.all(e != 0.0)
    big = np.abs(e) >= 1e-5
    assert np.all(big[:2]) and big.sum() > 0.7 * big.size                # orders 0 and 1 everywhere, most of the rest
    for name, got in _both(gh):
        rel = np.where(big, np.abs(got - e) / np.abs(e), 0.0).max(-1)
        ab = (np.abs(got - e) / np.maximum(np.maximum(1.0, y + phi), np.abs(e))).max(-1)
        print(name, 'pointwise where |exact| >= 1e-5:', rel, ' absolute over max(1, |exact|, y + phi):', ab)
        assert np.all(rel <= CAP) and np.all(ab <= ABS)
    gx, gw = _gh()
    a1, a2 = gh.ztnb_row_derivs(rho, s, y, phi, gx, gw)
    got = gh.ztnb_expected_H(rho, s, y, phi, gx, gw)
    assert np.array_equal(a1, got[1]) and np.array_equal(a2, 0.5 * got[2])
    # s = 0: the expectation is the function itself
    at0 = s == 0.0
    sp, sg, g2, g3, g4 = gh._logistic_node(rho[at0])
    g = gh.ztnb_g(rho[at0], phi[at0])
    H = np.stack([(y + phi)[at0] * a + b for a, b in zip((sp, sg, g2, g3, g4), g)])
    assert np.all(np.abs(H - got[:, at0]) <= 1e-14 * np.maximum(1.0, np.abs(H)))


def test_host_per_node_terms_against_mpmath(gh):
    import mpmath as mp
    mp.mp.dps = 50
    eta = np.arange(-36.0, 31.0)
    worst = np.zeros(5)
    for phi in (0.05, 0.5, 1.0, 7.0, 50.0, 1e3, 1e5):
        got = gh.ztnb_g(eta, phi, 4)
        assert len(got) == 5 and len(gh.ztnb_g(eta, phi, order=2)) == 3
        fn = _mp_g(phi)
        for i, t in enumerate(eta):
            c = mp.taylor(fn, mp.mpf(float(t)), 4)
            for k in range(5):
                want = c[k] * mp.factorial(k)
                worst[k] = max(worst[k], float(abs(mp.mpf(float(got[k][i])) - want) / max(1, abs(want))))
    print('per node g^(k), k = 0..4, absolute over max(1, |exact|):', worst)
    assert np.all(worst <= NODE)


def test_host_tails(gh):
    """g -> eta + log phi, g' -> 1 and g'' .. -> 0 as eta -> -inf; exact zeros of every derivative where v is huge; a non-finite
    value (a refusal, not a clamp) where v underflows to 0."""
    g = gh.ztnb_g(np.array([-40.0, -40.0]), np.array([0.05, 50.0]))
    assert np.allclose(g[0], -40.0 + np.log([0.05, 50.0]), rtol=0, atol=1e-14) and np.all(np.abs(g[1] - 1.0) < 1e-15)
    assert all(np.all(np.abs(a) < 1e-15) for a in g[2:])
    far = gh.ztnb_g(np.array([10.0, 800.0, 30.0]), np.array([100.0, 1.0, 1e5]))
    assert all(np.array_equal(a, np.zeros(3)) for a in far)
    with np.errstate(all='ignore'):
        assert all(not np.isfinite(a[0]) for a in gh.ztnb_g(np.array([-800.0]), 1.0)[:2])       # g = log 0 and g' = 0 / 0: the value and a1
        assert not np.isfinite(gh.ztnb_expected_H(np.array([-800.0]), np.array([1.0]), 2.0, 1.0, *_gh())[0, 0])


def test_host_response_mean(gh, exact):
    """The mean of the truncated count: the closed-form part plus the node sum, against mpmath on the same nodes; the node sum
    alone, CAP pointwise, wherever it is not below 1e-290 (past v = 700 it is set to 0 and is below 1e-300); against the true integral by
    mpmath.quad where the 20-node rule is exact to rounding (s <= 0.01, as tests/test_glmm_ztpoisson_host_math.py argues)."""
    import mpmath as mp
    mp.mp.dps = 50
    phi, rho, s, _ = _points()
    gx, gw = _gh()
    closed = phi * np.exp(rho + 0.5 * s)
    want = closed + exact[1]
    seen = exact[1] >= 1e-290
    for name, got, node in (('host', gh.ztnb_response_mean(rho, s, phi, gx, gw), gh._ztnb_mean_nodes(rho, s, phi, gx, gw)),
                            ('reference', ref.response_mean(rho, s, phi), ref.response_mean(rho, s, phi, closed=None))):
        e_full = np.max(np.abs(got - want) / want)
        e_node = np.max(np.abs(node - exact[1])[seen] / exact[1][seen])
        assert np.all(node[~seen] <= 1e-290)
        print('response mean', name, e_full, 'node part', e_node)
        assert e_full <= IDENT and e_node <= CAP and np.all(got >= 1.0 - 1e-15)
    for p0 in (0.05, 1.0, 50.0):
        for r0 in (-6.0, -1.0, 0.7, 3.0):
            for s0 in (0.0, 0.01):
                mean = lambda t: p0 * mp.exp(t) / -mp.expm1(-p0 * mp.log1p(mp.exp(t)))
                if s0 == 0.0:
                    w0 = mean(mp.mpf(r0))
                else:
                    sd = mp.sqrt(mp.mpf(s0))
                    w0 = mp.quad(lambda a: mean(r0 + sd * a) * mp.npdf(a), [-12, -4, 0, 4, 12])
                h = gh.ztnb_response_mean(np.array([r0]), np.array([s0]), np.array([p0]), gx, gw)[0]
                assert abs(h - float(w0)) <= IDENT * float(w0)


def test_closed_form_part_differs_from_the_rule_at_large_variance(gh):
    """What the x 30 variance case of the GPU test rests on: at s = 48 the 20-node sum of e^t is off by more than 1e-2 of
    phi exp(rho + s / 2), so a mean whose e^t part was taken on the nodes cannot pass there; at s = 1.6 the two agree to 1e-12."""
    for phi in (0.05, 1.7, 1e3):
        a, b = ref.response_mean([0.3], [48.0], phi), ref.response_mean([0.3], [48.0], phi, closed=False)
        assert abs(a - b)[0] > 1e-2 * a[0]
        a, b = ref.response_mean([0.3], [1.6], phi), ref.response_mean([0.3], [1.6], phi, closed=False)
        assert abs(a - b)[0] <= IDENT * a[0]
        h = gh.ztnb_response_mean(np.array([0.3]), np.array([48.0]), np.array([phi]), *_gh())
        assert abs(h - ref.response_mean([0.3], [48.0], phi))[0] <= IDENT * h[0]


# ---- the phi = 1 identities --------------------------------------------------------------------------------------------------
def test_phi_one_identities_per_node(gh):
    """At phi = 1: g = eta - sp(eta), so H = y sp - (y - 1) eta (the binomial term with y trials and y - 1 successes), and
    1 - P(y = 0) = sigma(eta) (the zero part of the hurdle is a logit Bernoulli model).  Per node, to 1e-14."""
    eta = np.linspace(-30.0, 30.0, 121)
    sp, sg, g2, g3, g4 = gh._logistic_node(eta)
    g = gh.ztnb_g(eta, 1.0)
    want = [eta - sp, 1.0 - sg, -g2, -g3, -g4]
    for k in range(5):
        assert np.max(np.abs(g[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))) <= 1e-14
    assert np.max(np.abs(-np.expm1(g[0]) - (1.0 - sg))) <= 1e-14           # P(y = 0) = 1 - sigma
    tt = torch.tensor(eta)
    for k in range(5):                                                   # and the reference's g, by its own route
        got = ref.dk(ref.g_of(torch.tensor(1.0)), tt, k).numpy()
        assert np.max(np.abs(got - want[k]) / np.maximum(1.0, np.abs(want[k]))) <= 1e-14
    # the moments: (y + 1) E sp^(k) + E g^(k) = y E sp^(k) + [eta, 1, 0, 0, 0]
    rho, s = np.meshgrid(np.array([-12.0, -2.0, 0.4, 5.0]), np.array([0.0, 0.5, 3.0]), indexing='ij')
    rho, s = rho.ravel(), s.ravel()
    y = 1.0 + np.arange(rho.size) % 7.0
    binom = ref.nb_coefs(rho, s, y - 1.0, 1.0)                           # trials y
    binom[0] += rho
    binom[1] += 1.0
    for got in (ref.eh_coefs(rho, s, y, 1.0), gh.ztnb_expected_H(rho, s, y, np.ones_like(rho), *_gh())):
        assert np.max(np.abs(got - binom) / np.maximum(1.0, np.abs(binom))) <= 1e-14 * 7.0


def test_reference_derivatives_are_steins_rule():
    """`value_grad_hess` of the reference's data term differentiates through `_EG`: its gradient in (rho, s) is (E g', E g'' / 2)."""
    rho = torch.tensor([-3.0, 0.4, 2.0], dtype=torch.float64, requires_grad=True)
    s = torch.tensor([0.2, 1.0, 2.5], dtype=torch.float64, requires_grad=True)
    phi = torch.tensor([0.05, 1.7, 50.0], dtype=torch.float64)
    val = ref._EG.apply(rho, s, phi, ref.GH_DEG, 0)
    g_r, g_s = torch.autograd.grad(val.sum(), (rho, s), create_graph=True)
    e = [ref.expected_g(rho.detach(), s.detach(), phi, k).numpy() for k in range(4)]
    assert np.allclose(g_r.detach().numpy(), e[1], rtol=1e-15) and np.allclose(g_s.detach().numpy(), 0.5 * e[2], rtol=1e-15)
    g_rs, = torch.autograd.grad(g_r.sum(), s)
    assert np.allclose(g_rs.numpy(), 0.5 * e[3], rtol=1e-15)


def test_draws_are_truncated_nb2():
    rng = np.random.default_rng(11)
    y = ref.ztnb_draw(rng, np.full(200000, 1.3), 0.7)
    p0 = (0.7 / 2.0) ** 0.7
    assert y.min() == 1.0 and abs(y.mean() - 1.3 / (1.0 - p0)) < 0.02
    x, y, z, w, gid, o, ph, free = ref.problem(130, 4, 2, 5, 3, phi='vector')
    assert y[0] == y[1] == 1.0 and y[2] == 57.0 and ph[0] == 0.05 and ph[1] == 1e3 and np.all(y >= 1.0)


# ---- the classes' checks that need no device ---------------------------------------------------------------------------------
def test_refusals_before_the_device_context_exists():
    import inspect
    import lrvb_amd as vb
    x, z, gid = np.ones((4, 1)), np.ones((4, 1)), np.zeros(4, dtype=np.int64)
    for bad in (0.0, 0.5, -1.0, np.nan, np.inf):
        y = np.array([1.0, 2.0, bad, 3.0])
        with pytest.raises(ValueError, match='>= 1'):
            vb.TruncatedNegBinomialGLMMObjective(None, x, y, z, gid, 1, 1.5)
    with pytest.raises(ValueError, match='>= 1'):
        vb.TruncatedNegBinomialGLMMObjective(None, x, np.ones(3), z, gid, 1, 1.5)
    y = np.array([1.0, 2.0, 5.0, 3.0])
    for bad in (0.0, -1.0, np.nan, np.inf, np.ones(3), np.array([1.0, 2.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match='dispersion'):
            vb.TruncatedNegBinomialGLMMObjective(None, x, y, z, gid, 1, bad)
        with pytest.raises(ValueError, match='dispersion'):
            vb.HurdleNegBinomialGLMM(None, None, x, y - 1.0, z, gid, 1, bad)
    with pytest.raises(ValueError, match='offset'):
        vb.TruncatedNegBinomialGLMMObjective(None, x, y, z, gid, 1, 1.5, offset=np.array([0.0, np.nan, 0.0, 0.0]))
    with pytest.raises(ValueError, match='zero_link'):
        vb.HurdleNegBinomialGLMM(None, None, x, np.arange(4.0), z, gid, 1, 1.5, zero_link='cauchit')
    for yy in (np.array([0.0, 1.0, 0.5, 2.0]), np.array([0.0, -1.0, 1.0, 2.0]), np.zeros(4)):
        with pytest.raises(ValueError):
            vb.HurdleNegBinomialGLMM(None, None, x, yy, z, gid, 1, 1.5)
    sig = inspect.signature(vb.TruncatedNegBinomialGLMMObjective.__init__)
    assert list(sig.parameters)[1:10] == ['par', 'x', 'y', 'z', 'groups', 'n_groups', 'dispersion', 'offset', 'beta_prior_info']
    assert sig.parameters['gh_deg'].default == 20
    assert issubclass(vb.HurdleNegBinomialGLMM, vb.glmm_hurdle._HurdleGLMM) and issubclass(vb.HurdlePoissonGLMM, vb.glmm_hurdle._HurdleGLMM)
    assert 'predict' not in vars(vb.HurdleNegBinomialGLMM) and 'value' not in vars(vb.HurdleNegBinomialGLMM)     # the body is shared

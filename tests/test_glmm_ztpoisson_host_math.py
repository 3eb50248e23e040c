"""The zero-truncated Poisson likelihood of the hurdle model without a GPU: the accuracy of the torch
reference tests/glmm_ztpoisson_reference.py against mpmath, the package's module-level host functions (the formulas of the
kernels: r = u / expm1(u) and its recurrences, the e^t part in closed form) against both, and the reduction identities.

Points: the grid rho in {-12, -10, -8, -5, -2, 0, 2.5, 5} x s in {0, 0.5, 1.5, 3}, corners and s = 0 included; the 20 nodes then
reach t in about [-25, 18].

Bounds.  `CAP` = 1e-10 is the cap of DESIGN.md section 35, here taken POINTWISE: the error of every E A^(k) over the magnitude of
that E A^(k) at that point (stricter than section 35's "largest error over the vector's largest magnitude").  The loss to expect:
q = 1 - u - r cancels to -u / 2 as u -> 0, so A'', A''' and A'''' (all about u / 2) carry about 2^-53 / (u / 2): 4e-11 relative at
t = -12 per node before the weights average it down.  Measured maxima over the grid, k = 0..4 (printed by the tests):
host 3.6e-16, 2.8e-16, 3.9e-12, 3.9e-12, 3.9e-12; reference 2.4e-16, 1.9e-16, 5.2e-16, 5.2e-15, 1.2e-13 (its small-u series).  The
plain recurrences meet the cap with a factor 25 to spare, so neither the kernels nor the host functions carry a series.
`IDENT` = 1e-12 of the largest magnitude of a coefficient vector over the grid, the measure and the bound of the identities in
tests/test_glmm_link_host_math.py: they compare sums of at most 20 node terms whose parts cancel analytically, each term good to
a few ulp of its own magnitude.  (Pointwise the cloglog link reference, nested autograd without a series, is only good to 2.7e-10
at rho = -12, outside the [-5, 5] it was written for.)

Large mean.  A^(k) - e^t = r^(k-1) decays like u^k e^-u, but the lowest of the 20 nodes sits 5.39 sqrt(2 s) below rho: at rho = 6,
s = 0.5 the node at t = 2.06 (weight 6e-8) still contributes r''' of order 1, 1e-10 of exp(rho + s / 2) -- outside 1e-12.  At
rho >= 10, s <= 0.5 every node has t >= 4.6, u >= 100 and r^(k) < 1e-35: the region used here; the GPU test uses rho >= 12 at its
own s <= 1.7 (lowest node t >= 2.0 at weight 1e-13, u^4 e^-u 1e-13 < 1e-13 exp(12)) and re-checks the reference at its own data."""
import numpy as np
import pytest
import torch

import glmm_link_reference as lref
import glmm_ztpoisson_reference as ref

CAP, IDENT = 1e-10, 1e-12
RHO = np.array([-12.0, -10.0, -8.0, -5.0, -2.0, 0.0, 2.5, 5.0])
S = np.array([0.0, 0.5, 1.5, 3.0])


def _points():
    rho, s = np.meshgrid(RHO, S, indexing='ij')
    return rho.ravel(), s.ravel()


def _gh(deg=ref.GH_DEG):
    return np.polynomial.hermite.hermgauss(deg)


@pytest.fixture(scope='module')
def gh():
    import lrvb_amd
    from lrvb_amd import glmm_hurdle
    return glmm_hurdle


@pytest.fixture(scope='module')
def gb():
    from lrvb_amd import glmm_binomial
    return glmm_binomial


@pytest.fixture(scope='module')
def exact():
    """E A^(k), k = 0..4, at the grid on the 20-node rule: the node part log(1 - exp(-e^t)) and its derivatives from mpmath at 50
    digits (mpmath.taylor), plus exp(rho + s / 2).  Also E r, the node part of the response mean.  Computed once."""
    import mpmath as mp
    mp.mp.dps = 50
    rho, s = _points()
    gx, gw = _gh()
    fn = lambda t: mp.log(-mp.expm1(-mp.exp(t)))
    e = np.zeros((5, rho.size))
    for n in range(rho.size):
        acc = [mp.mpf(0)] * 5
        for xk, wk in zip(gx, gw):
            t = mp.mpf(float(rho[n])) + mp.sqrt(mp.mpf(float(s[n]))) * mp.sqrt(2) * mp.mpf(float(xk))
            c = mp.taylor(fn, t, 4)
            for k in range(5):
                acc[k] += mp.mpf(float(wk)) / mp.sqrt(mp.pi) * c[k] * mp.factorial(k)
        eu = mp.exp(mp.mpf(float(rho[n])) + mp.mpf(float(s[n])) / 2)
        e[:, n] = [float(a + eu) for a in acc]
    return e


def _pointwise(got, want):
    """Per derivative order: the largest error over that derivative's own magnitude at the same point."""
    return np.max(np.abs(got - want) / np.abs(want), axis=-1)


def _worst(got, want):
    """The identities' measure, that of tests/test_glmm_link_host_math.py: per derivative order (a row over the grid) the largest
    error over that row's largest magnitude."""
    return np.max(np.abs(got - want), axis=-1) / np.max(np.abs(want), axis=-1)


# ---- accuracy of the reference and of the host functions ---------------------------------------------------------------------
def test_reference_expectations_against_mpmath(exact):
    rho, s = _points()
    err = _pointwise(ref.ea_coefs(rho, s), exact)
    print('reference E A^(k), k = 0..4, pointwise relative:', err)
    assert np.all(err <= CAP)


def test_host_expectations_against_mpmath_and_reference(gh, exact):
    rho, s = _points()
    gx, gw = _gh()
    got = gh.ztp_expected_A(rho, s, gx, gw)
    err = _pointwise(got, exact)
    print('host E A^(k), k = 0..4, pointwise relative:', err)
    assert got.shape == (5, rho.size) and np.all(err <= CAP)
    assert np.all(_pointwise(got, ref.ea_coefs(rho, s)) <= CAP)
    a1, a2 = gh.ztp_row_derivs(rho, s, gx, gw)
    assert np.array_equal(a1, got[1]) and np.array_equal(a2, 0.5 * got[2])
    assert np.array_equal(gh.ztp_response_mean(rho, s, gx, gw), got[1])
    # s = 0: the expectation is the function itself
    at0 = s == 0.0
    A = np.stack(gh.ztp_A(rho[at0]))
    assert np.all(np.abs(A - got[:, at0]) <= 1e-14 * np.abs(A))


def test_host_per_node_terms(gh):
    """A is convex with A' > 1 (the mean of a count >= 1); the tails: A -> t, A' -> 1, A'' -> 0 as t -> -inf and A^(k) -> e^t as
    t -> +inf, exact zeros of the node part where u = e^t is huge, and NaN (a refusal, not a clamp) where u underflows to 0."""
    import mpmath as mp
    mp.mp.dps = 50
    t = np.array([-30.0, -20.0, -12.0, -5.0, 0.0, 1.0, 3.0, 5.0])
    A = gh.ztp_A(t)
    assert len(A) == 5 and len(gh.ztp_A(t, order=2)) == 3
    assert np.all(A[1] > 1.0 - 1e-15) and np.all(A[2] > 0.0)
    for k in (0, 1):                                                     # good to 2e-16 everywhere
        want = np.array([float(mp.diff(lambda a: mp.log(mp.expm1(mp.exp(a))), mp.mpf(float(v)), k)) for v in t])
        assert np.max(np.abs(A[k] - want) / np.abs(want)) < 1e-15
    for k in (2, 3, 4):                                                  # the absolute error stays at a few 1e-17 for u -> 0
        want = np.array([float(mp.diff(lambda a: mp.log(mp.expm1(mp.exp(a))), mp.mpf(float(v)), k)) for v in t])
        assert np.all(np.abs(A[k] - want) <= 2e-15 * np.maximum(np.abs(want), 1.0))
        assert np.all(np.abs(A[k] - want)[:3] < 1e-15)
    node = gh._ztp_node(np.array([40.0, 700.0, 800.0]), 4)
    assert all(np.array_equal(g, np.zeros(3)) for g in node)
    assert all(np.all(np.isnan(a) | np.isinf(a)) for a in gh.ztp_A(np.array([-800.0])))


def test_host_response_mean(gh, exact):
    """The node sum itself against mpmath on the same nodes (part of `exact`, row 1: E A').  Against the true integral
    E [lambda / (1 - exp(-lambda))] by mpmath.quad only where the 20-node rule is exact to rounding: r(t) is analytic within pi / 2
    of the real axis, and at s <= 0.01 the remainder of the degree-39 rule, s^20 39!! / (pi / 2)^40 = 5e-25, is far below it."""
    import mpmath as mp
    mp.mp.dps = 50
    rho, s = _points()
    gx, gw = _gh()
    got = gh.ztp_response_mean(rho, s, gx, gw)
    assert np.max(np.abs(got - exact[1]) / exact[1]) <= IDENT
    assert np.max(np.abs(got - ref.response_mean(rho, s)) / exact[1]) <= IDENT
    assert np.all(got >= 1.0 - 1e-15)
    for r0 in (-6.0, -1.0, 0.7, 3.0):
        for s0 in (0.0, 0.01):
            mean = lambda t: mp.exp(t) / -mp.expm1(-mp.exp(t))
            if s0 == 0.0:
                want = mean(mp.mpf(r0))
            else:
                sd = mp.sqrt(mp.mpf(s0))
                want = mp.quad(lambda a: mean(r0 + sd * a) * mp.npdf(a), [-12, -4, 0, 4, 12])
            h = gh.ztp_response_mean(np.array([r0]), np.array([s0]), gx, gw)[0]
            assert abs(h - float(want)) <= IDENT * float(want)


# ---- reduction identities ----------------------------------------------------------------------------------------------------
def test_hurdle_decomposition(gh, gb):
    """For any (rho, s, y >= 0) the Poisson term exp(rho + s / 2) - y rho is [y = 0] (cloglog E h0) + [y > 0] (cloglog E h1 + the
    zero-truncated term), in the value and in the derivatives k = 1..4: A = e^t - h1, the node parts cancel.  On the reference
    and on the host functions."""
    rho, s = _points()
    gx, gw = _gh()
    one, zero = np.ones_like(rho), np.zeros_like(rho)
    y = 1.0 + np.arange(rho.size) % 7.0
    pois = np.tile(np.exp(rho + 0.5 * s), (5, 1))
    shift = np.zeros((5, rho.size))
    shift[0], shift[1] = y * rho, y                                      # the "- y rho" of the value and the "- y" of a1
    for name, h1, h0, ea in (('reference', lref.eh_coefs('cloglog', rho, s, one, one), lref.eh_coefs('cloglog', rho, s, zero, one),
                              ref.ea_coefs(rho, s)),
                             ('host', gb.link_expected_h('cloglog', rho, s, one, one, gx, gw),
                              gb.link_expected_h('cloglog', rho, s, zero, one, gx, gw), gh.ztp_expected_A(rho, s, gx, gw))):
        err_pos = np.max(_worst(h1 + (ea - shift), pois - shift))
        err_zero = np.max(_worst(h0, pois))
        print('hurdle decomposition', name, err_pos, err_zero)
        assert err_pos <= IDENT and err_zero <= IDENT


def test_large_mean_is_the_poisson_model(gh):
    """rho >= 10, s <= 0.5 (module docstring): every E A^(k) is exp(rho + s / 2) to 1e-12, on the reference and on the host."""
    rho, s = np.meshgrid(np.array([10.0, 12.0, 15.0, 20.0]), np.array([0.0, 0.1, 0.5]), indexing='ij')
    rho, s = rho.ravel(), s.ravel()
    gx, gw = _gh()
    pois = np.tile(np.exp(rho + 0.5 * s), (5, 1))
    for name, ea in (('reference', ref.ea_coefs(rho, s)), ('host', gh.ztp_expected_A(rho, s, gx, gw))):
        err = np.max(np.abs(ea - pois) / pois)
        print('large mean', name, err)
        assert err <= IDENT
    # and rho = 6, s = 0.5 is NOT inside 1e-12 in the fourth derivative: the reason the region starts higher
    far = ref.ea_coefs([6.0], [0.5])[:, 0]
    assert abs(far[4] - np.exp(6.25)) > IDENT * np.exp(6.25)


def test_closed_form_split_differs_from_the_rule_at_large_variance():
    """What the x 30 variance case of the GPU test rests on: at s = 48 the 20-node sum of e^t is off by more than 1e-2 of
    exp(rho + s / 2), so a kernel that took the e^t part on the nodes cannot pass there; at s = 1.6 the two agree to 1e-12."""
    a, b = ref.ea_coefs([0.3], [48.0]), ref.ea_coefs([0.3], [48.0], closed=False)
    assert np.all(np.abs(a - b)[1:, 0] > 1e-2 * np.abs(a)[1:, 0])
    a, b = ref.ea_coefs([0.3], [1.6]), ref.ea_coefs([0.3], [1.6], closed=False)
    assert np.all(np.abs(a - b) <= IDENT * np.abs(a))


def test_reference_derivatives_are_steins_rule():
    """`value_grad_hess` of the reference's data term differentiates through `_EA`: its gradient in (rho, s) is (E A', E A'' / 2)."""
    rho = torch.tensor([-3.0, 0.4, 2.0], dtype=torch.float64, requires_grad=True)
    s = torch.tensor([0.2, 1.0, 2.5], dtype=torch.float64, requires_grad=True)
    val = ref._EA.apply(rho, s, ref.GH_DEG, 0)
    g_r, g_s = torch.autograd.grad(val.sum(), (rho, s), create_graph=True)
    e = ref.ea_coefs(rho.detach().numpy(), s.detach().numpy())
    assert np.allclose(g_r.detach().numpy(), e[1], rtol=1e-15) and np.allclose(g_s.detach().numpy(), 0.5 * e[2], rtol=1e-15)
    g_rs, = torch.autograd.grad(g_r.sum(), s)
    assert np.allclose(g_rs.numpy(), 0.5 * e[3], rtol=1e-15)


# ---- the classes' checks that need no device ---------------------------------------------------------------------------------
def test_responses_are_checked_before_the_device_context_exists():
    import inspect
    import lrvb_amd as vb
    x, z, gid = np.ones((4, 1)), np.ones((4, 1)), np.zeros(4, dtype=np.int64)
    for bad in (0.0, 0.5, -1.0, np.nan, np.inf):
        y = np.array([1.0, 2.0, bad, 3.0])
        with pytest.raises(ValueError, match='>= 1'):
            vb.TruncatedPoissonGLMMObjective(None, x, y, z, gid, 1)
    with pytest.raises(ValueError, match='>= 1'):
        vb.TruncatedPoissonGLMMObjective(None, x, np.ones(3), z, gid, 1)
    with pytest.raises(ValueError, match='zero_link'):
        vb.HurdlePoissonGLMM(None, None, x, np.arange(4.0), z, gid, 1, zero_link='cauchit')
    for y in (np.array([0.0, 1.0, 0.5, 2.0]), np.array([0.0, -1.0, 1.0, 2.0]), np.zeros(4)):
        with pytest.raises(ValueError):
            vb.HurdlePoissonGLMM(None, None, x, y, z, gid, 1)
    sig = inspect.signature(vb.TruncatedPoissonGLMMObjective.__init__)
    assert list(sig.parameters)[1:9] == ['par', 'x', 'y', 'z', 'groups', 'n_groups', 'offset', 'beta_prior_info']
    assert sig.parameters['gh_deg'].default == 20

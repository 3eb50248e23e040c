"""The probit and cloglog links of the binomial mixed model without a GPU: the accuracy of the torch
reference tests/glmm_link_reference.py against mpmath, the package's module-level host functions (the formulas of the kernels:
inverse Mills ratio through erfcx, r = u / expm1(u)) against both, and the reduction identities.

Points: 40 pairs (rho, s), rho in [-5, 5], s in [0, 3], one at s = 0; the 20 nodes then reach t in about [-15, 18].

Bounds.  `CAP` = 1e-10 of a coefficient vector's largest magnitude is the cap the reference has to meet (10x inside the project's
Hessian bound of 1e-9); the host formulas are held to the same cap against mpmath: their worst cancellation, d = t + lambda at
t = -15 (d = 0.066 from two terms of size 15), amplifies the few ulp of erfcx by 15 / 0.066 = 230 -- about 1e-13.  The
identities compare two evaluations of the same sums in another order or at mirrored nodes: IDENT = 1e-12 of the largest magnitude
(at most 20 nodes x 13 trials of terms with a relative rounding error of a few ulp each, times the amplification above)."""
import numpy as np
import pytest
import torch

import glmm_binomial_reference as bref
import glmm_link_reference as ref

CAP, IDENT = 1e-10, 1e-12
LINKS = ref.LINKS


def _points():
    rng = np.random.default_rng(35)
    rho, s = rng.uniform(-5.0, 5.0, size=40), rng.uniform(0.0, 3.0, size=40)
    s[7] = 0.0
    rho[0], rho[1], s[0], s[1] = -5.0, 5.0, 3.0, 3.0                    # the corners that reach furthest into either tail
    return rho, s


def _gh(deg=ref.GH_DEG):
    return np.polynomial.hermite.hermgauss(deg)


@pytest.fixture(scope='module')
def gb():
    import lrvb_amd
    from lrvb_amd import glmm_binomial
    return glmm_binomial


@pytest.fixture(scope='module')
def exact():
    """E h1^(k) and E h0^(k), k = 0..4, at the 40 points on the 20-node rule with h^(k) from mpmath at 50 digits:
    exact[link][which] is 5 x 40.  Computed once."""
    import mpmath as mp
    mp.mp.dps = 50
    rho, s = _points()
    gx, gw = _gh()
    fns = {('probit', 1): lambda t: -mp.log(mp.ncdf(t)), ('probit', 0): lambda t: -mp.log(mp.ncdf(-t)),
           ('cloglog', 1): lambda t: -mp.log(-mp.expm1(-mp.exp(t)))}
    out = {link: {} for link in LINKS}
    for (link, which), fn in fns.items():
        e = np.zeros((5, rho.size))
        for n in range(rho.size):
            acc = [mp.mpf(0)] * 5
            for xk, wk in zip(gx, gw):
                t = mp.mpf(float(rho[n])) + mp.sqrt(mp.mpf(float(s[n]))) * mp.sqrt(2) * mp.mpf(float(xk))
                c = mp.taylor(fn, t, 4)                                  # mpmath.diff of the orders 0..4 on one set of evaluations: h^(k) / k!
                for k in range(5):
                    acc[k] += mp.mpf(float(wk)) / mp.sqrt(mp.pi) * c[k] * mp.factorial(k)
            e[:, n] = [float(a) for a in acc]
        out[link][which] = e
    out['cloglog'][0] = np.tile(np.array([float(mp.exp(mp.mpf(float(r)) + mp.mpf(float(v)) / 2)) for r, v in zip(rho, s)]), (5, 1))
    return out


def _worst(got, want):
    """Per coefficient vector (a row of 40 values): the largest error over that vector's largest magnitude."""
    return np.max(np.abs(got - want), axis=-1) / np.max(np.abs(want), axis=-1)


# ---- accuracy of the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('link', LINKS)
def test_reference_expectations_against_mpmath(exact, link):
    rho, s = _points()
    tr, ts = torch.tensor(rho), torch.tensor(s)
    for which in (1, 0):
        got = np.stack([ref.expected_dk(link, which, tr, ts, k).numpy() for k in range(5)])
        err = _worst(got, exact[link][which])
        print('reference', link, 'h%d' % which, err)
        assert np.all(err <= CAP)


# ---- the package's host functions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('link', LINKS)
def test_host_expectations_against_mpmath_and_reference(gb, exact, link):
    rho, s = _points()
    gx, gw = _gh()
    one, zero = np.ones_like(rho), np.zeros_like(rho)
    e1 = gb.link_expected_h(link, rho, s, one, one, gx, gw)              # y = m = 1: E h1^(k)
    e0 = gb.link_expected_h(link, rho, s, zero, one, gx, gw)             # y = 0, m = 1: E h0^(k)
    for which, got in ((1, e1), (0, e0)):
        err = _worst(got, exact[link][which])
        print('host', link, 'h%d' % which, err)
        assert np.all(err <= CAP)
    rng = np.random.default_rng(5)
    mt = rng.integers(0, 13, size=rho.size).astype(np.float64)
    y = np.floor(rng.uniform(size=rho.size) * (mt + 1.0))
    assert np.all(y <= mt) and np.any(mt == 0) and np.any(y == 0) and np.any((y == mt) & (mt > 0))
    want = ref.eh_coefs(link, rho, s, y, mt)
    got = gb.link_expected_h(link, rho, s, y, mt, gx, gw)
    assert np.all(_worst(got, want) <= CAP)
    a1, a2 = gb.link_row_derivs(link, rho, s, y, mt, gx, gw)
    assert np.array_equal(a1, got[1]) and np.array_equal(a2, 0.5 * got[2])
    exact_mix = y * exact[link][1] + (mt - y) * exact[link][0]
    assert np.all(_worst(np.stack([a1, a2]), np.stack([exact_mix[1], 0.5 * exact_mix[2]])) <= CAP)


@pytest.mark.parametrize('link', LINKS)
def test_host_per_node_terms_in_the_tails(gb, link):
    """The tail limits of the formulas the kernels use: finite values where phi / Phi would be 0 / 0 (t = -40), exact zeros where
    erfcx overflows or u = e^t is huge, no NaN anywhere on [-700, 700]."""
    t = np.array([-700.0, -40.0, -15.0, 0.0, 15.0, 40.0, 700.0])
    h1, h0 = gb.link_h(link, t)
    assert all(np.all(np.isfinite(a)) for a in h1)
    if link == 'probit':
        assert abs(h1[1][1] + 40.024968847207264) < 1e-12              # -phi(-40) / Phi(-40) to 17 digits (mpmath)
        assert all(a[-1] == 0.0 for a in h1[1:]) and h1[0][-1] == 0.0
        assert all(np.array_equal(a, (-1) ** k * b[::-1]) for k, (a, b) in enumerate(zip(h0, h1)))
    else:
        assert all(a[-1] == 0.0 and a[-2] == 0.0 for a in h1)          # u = e^40 and u = +inf: the limits, not inf / inf
        assert abs(h1[1][0] + 1.0) < 1e-15 and abs(h1[0][0] - 700.0) < 1e-12      # h1 -> -t, h1' -> -1 as t -> -inf
        assert np.array_equal(h0[0], np.exp(t)) and all(np.array_equal(a, h0[0]) for a in h0)


@pytest.mark.parametrize('link', LINKS)
def test_host_response_mean(gb, link):
    """Against the reference's node sum; the probit closed form m Phi(rho / sqrt(1 + s)) against the 128-node rule: Phi is entire
    and the rule's truncation error is far below rounding there; 128 terms of at most 1 with weights that sum to 1 round to about
    128 ulp = 3e-14, the nodes and weights of the rule at that degree are good to about 1e-13: 1e-12 absolute per trial."""
    rho, s = _points()
    gx, gw = _gh()
    mt = np.arange(rho.size) % 13.0
    got = gb.link_response_mean(link, rho, s, mt, gx, gw)
    if link == 'cloglog':
        assert np.max(np.abs(got - ref.response_mean(link, rho, s, mt))) <= IDENT * np.max(mt)
        assert np.all(got <= mt) and np.all(got >= 0.0)
    else:
        assert np.max(np.abs(got - ref.response_mean(link, rho, s, mt, deg=128))) <= 1e-12 * np.max(mt)
        assert np.array_equal(got, mt * ref.prob('probit', rho / np.sqrt(1.0 + s)))
    assert np.array_equal(gb.link_response_mean(link, rho, s, None, gx, gw) * mt, got)


# ---- reduction identities ----------------------------------------------------------------------------------------------------
def _problem(link, N=60, P=3, K=2, G=4, seed=11):
    x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, seed, link)
    eta = ref.free_to_vec(torch.tensor(free), P, K, G)
    return x, y, z, w, gid, o, mt, eta, G


def _ref_value_grad(eta, x, y, z, w, o, mt, gid, G, link):
    val, g, _ = ref.value_grad_hess(lambda p, *a: ref.data(p, *a), eta.numpy(), bref.targs(x, y, z, w, o, mt, gid, G)[:8] + (link,),
                                    want_hess=False)
    return val, g


def test_probit_is_symmetric_under_the_flip(gb):
    """(y, x, z, o) -> (m - y, -x, -z, -o) leaves the probit data term and its gradient unchanged: h0(t) = h1(-t)."""
    x, y, z, w, gid, o, mt, eta, G = _problem('probit')
    a = _ref_value_grad(eta, x, y, z, w, o, mt, gid, G, 'probit')
    b = _ref_value_grad(eta, -x, mt - y, -z, w, -o, mt, gid, G, 'probit')
    assert abs(a[0] - b[0]) <= IDENT * abs(a[0]) and np.max(np.abs(a[1] - b[1])) <= IDENT * np.max(np.abs(a[1]))
    rho, s = _points()
    gx, gw = _gh()
    mt, y = np.full(rho.size, 7.0), np.arange(rho.size) % 8.0
    e = gb.link_expected_h('probit', rho, s, y, mt, gx, gw)
    f = gb.link_expected_h('probit', -rho, s, mt - y, mt, gx, gw)
    sign = np.array([1.0, -1.0, 1.0, -1.0, 1.0])[:, None]
    assert np.all(_worst(sign * f, e) <= IDENT)


def test_cloglog_rows_without_successes_are_poisson_rows(gb):
    """y = 0: the cloglog term m e^t is the Poisson term with offset o + log m and y = 0, every derivative exp(rho + log m + s / 2)."""
    x, y, z, w, gid, o, mt, eta, G = _problem('cloglog')
    mt = np.maximum(mt, 1.0)
    rho, s = bref._rho_s(eta, torch.tensor(x), torch.tensor(z), torch.tensor(o + np.log(mt)), torch.tensor(gid.astype(np.int64)), G)
    pois = float((torch.tensor(w) * torch.exp(rho + 0.5 * s)).sum())
    val, _ = _ref_value_grad(eta, x, np.zeros_like(y), z, w, o, mt, gid, G, 'cloglog')
    assert abs(val - pois) <= IDENT * abs(pois)
    rho, s = _points()
    gx, gw = _gh()
    m = 1.0 + np.arange(rho.size) % 12.0
    e = gb.link_expected_h('cloglog', rho, s, np.zeros_like(m), m, gx, gw)
    assert np.all(_worst(e, np.tile(np.exp(rho + np.log(m) + 0.5 * s), (5, 1))) <= IDENT)


@pytest.mark.parametrize('link', LINKS)
def test_trials_against_expanded_bernoulli_rows(gb, link):
    """y successes out of m trials with weight w = a row (y = 1, m = 1, weight w y) and a row (y = 0, m = 1, weight w (m - y))."""
    x, y, z, w, gid, o, mt, eta, G = _problem(link)
    N = y.size
    a = _ref_value_grad(eta, x, y, z, w, o, mt, gid, G, link)
    x2, z2, g2, o2 = np.vstack([x, x]), np.vstack([z, z]), np.concatenate([gid, gid]), np.concatenate([o, o])
    b = _ref_value_grad(eta, x2, np.concatenate([np.ones(N), np.zeros(N)]), z2, np.concatenate([w * y, w * (mt - y)]), o2,
                        np.ones(2 * N), g2, G, link)
    assert abs(a[0] - b[0]) <= IDENT * abs(a[0]) and np.max(np.abs(a[1] - b[1])) <= IDENT * np.max(np.abs(a[1]))
    rho, s = _points()
    gx, gw = _gh()
    m, yy = np.full(rho.size, 9.0), np.arange(rho.size) % 10.0
    one = np.ones_like(rho)
    e = gb.link_expected_h(link, rho, s, yy, m, gx, gw)
    f = yy * gb.link_expected_h(link, rho, s, one, one, gx, gw) + (m - yy) * gb.link_expected_h(link, rho, s, 0.0 * one, one, gx, gw)
    assert np.all(_worst(f, e) <= IDENT)


# ---- the keyword ------------------------------------------------------------------------------------------------------------
def test_link_keyword_is_checked_before_the_device_context_exists():
    import inspect
    import lrvb_amd as vb
    x, z, gid = np.ones((4, 1)), np.ones((4, 1)), np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError, match='link'):
        vb.BinomialGLMMObjective(None, x, np.zeros(4), z, gid, 1, link='cauchit')
    sig = inspect.signature(vb.BinomialGLMMObjective.__init__)
    assert list(sig.parameters)[-1] == 'link' and sig.parameters['link'].default == 'logit'
    assert 'link' not in inspect.signature(vb.NegBinomialGLMMObjective.__init__).parameters
    assert vb.glmm_binomial.LINKS == {'logit': 0, 'probit': 1, 'cloglog': 2}
    with pytest.raises(ValueError):
        vb.glmm_binomial.link_h('logit', 0.0)

"""The ordinal mixed model on the CPU: the torch reference tests/glmm_ordinal_reference.py and the host forms
of linearresponsevariationalbayes.py_amd/glmm_ordinal.py against mpmath, and the preconditions of the GPU parity tests.  No device.

Exact values.  `_forms` restates, at 60 digits, the row term and its derivatives in t (to order 4), in (lo, hi) (to order 2) and the
two mixed orders as the model forms them: softplus(t - hi) + softplus(lo - t) - log(1 - e^-D) and sigma, sigma', .. at t - hi and at
lo - t, r = 1 / expm1(D), c = e^-D / expm1(-D)^2.  `test_exact_forms_are_the_derivatives` shows by `mpmath.diff` of the ONE expression
-log(sigma(hi - t) - sigma(lo - t)) that these are its derivatives (1e-25 of the size of the terms), so that the forms pinned below are
not merely compared with themselves.  The model's expectation is their sum over the Gauss-Hermite nodes; that the node sum
converges to the integral is shown by mpmath quadrature.

Error measure: an error of E h^(k) is taken over max(1, |exact|) for the value and over the size of the terms (sums of absolute
values, all O(1) or below for a logistic function) for the derivatives.  `CAP` = 1e-10 is the cap of the other families.

Where the reference meets the cap.  A row depends on (rho - lo, rho - hi, s, D) alone.  GRID (tests/glmm_ordinal_reference.py):
rho - lo and rho - hi in [-12, 12], s in [0, 3], D in [2^-6, 16], both end categories.  Every row of every GPU data set is asserted to
lie inside it below."""
import mpmath as mp
import numpy as np
import pytest
import torch

import glmm_ordinal_reference as ref

CAP, HOST = 1e-10, 1e-13
DPS = 60
GRID = ref.GRID
GX, GW = np.polynomial.hermite.hermgauss(ref.GH_DEG)
INF = float('inf')


@pytest.fixture(scope='module')
def go():
    import lrvb_amd
    from lrvb_amd import glmm_ordinal
    assert hasattr(glmm_ordinal, 'ordinal_expected_h') and hasattr(lrvb_amd, 'OrdinalGLMMObjective')
    return glmm_ordinal


def _at_dps(fn):
    import functools

    @functools.wraps(fn)
    def run(*a, **k):
        with mp.workdps(DPS):
            return fn(*a, **k)
    return run


def _mpf(a):
    return mp.mpf(float(a))


def _sig(x):
    return 1 / (1 + mp.exp(-x))


def _logistic(x):
    """[softplus, sigma, sigma', sigma'', sigma'''] at x; exact zeros at -inf."""
    if x == -mp.inf:
        return [mp.mpf(0)] * 5
    s = _sig(x)
    v = s * (1 - s)
    return [mp.log1p(mp.exp(-abs(x))) + max(x, 0), s, v, v * (1 - 2 * s), v * (1 - 6 * v)]


def _forms(t, lo, hi):
    """(h^(k), k = 0..4; dict of the threshold derivatives) of the row term in the model's form."""
    a, b = _logistic(t - hi), _logistic(lo - t)
    interior = lo != -mp.inf and hi != mp.inf
    D = hi - lo if interior else mp.inf
    dterm = -mp.log(-mp.expm1(-D)) if interior else mp.mpf(0)
    r = 1 / mp.expm1(D) if interior else mp.mpf(0)
    c = mp.exp(-D) / mp.expm1(-D) ** 2 if interior else mp.mpf(0)
    h = [a[0] + b[0] + dterm, a[1] - b[1], a[2] + b[2], a[3] - b[3], a[4] + b[4]]
    thr = dict(hi=-a[1] - r, lo=b[1] + r, hihi=a[2] + c, lolo=b[2] + c, lohi=-c, t_hi=-a[2], t_lo=-b[2], tt_hi=-a[3], tt_lo=b[3])
    return h, thr


def _single(t, lo, hi):
    return -mp.log(_sig(hi - t) - _sig(lo - t))


@_at_dps
def test_exact_forms_are_the_derivatives():
    """`_forms` against mpmath.diff of the single expression, in t to order 4, in (lo, hi) to order 2 and the two mixed-t orders:
    1e-25 (mpmath.diff at 60 digits holds about 30).  Interior rows at both tails, a tiny and a large D."""
    tol = mp.mpf(10) ** -25
    for t, lo, hi in ((0.3, -0.4, 0.9), (-6.0, 0.1, 0.35), (7.0, -1.0, 2.5), (1.0, 0.5, 0.5 + 2.0 ** -6), (-2.0, -3.0, 9.0), (12.0, 0.0, 1.0)):
        t, lo, hi = _mpf(t), _mpf(lo), _mpf(hi)
        h, thr = _forms(t, lo, hi)
        assert abs(_single(t, lo, hi) - h[0]) <= tol * max(1, abs(h[0]))
        for k in range(1, 5):
            assert abs(mp.diff(lambda tt: _single(tt, lo, hi), t, k) - h[k]) <= tol, (t, k)
        f = lambda tt, l, u: _single(tt, l, u)
        a, b, D = _logistic(t - hi), _logistic(lo - t), hi - lo
        r, c = 1 / mp.expm1(D), mp.exp(-D) / mp.expm1(-D) ** 2
        # every entry over the size of ITS OWN terms: r for the first orders in (lo, hi), c for the second, the sigma derivative alone
        # for the mixed-t orders (|sigma''| <= sigma')
        size = dict(lo=b[1] + r, hi=a[1] + r, lolo=b[2] + c, hihi=a[2] + c, lohi=c, t_lo=b[2], t_hi=a[2], tt_lo=b[2], tt_hi=a[2])
        for name, order in (('lo', (0, 1, 0)), ('hi', (0, 0, 1)), ('lolo', (0, 2, 0)), ('hihi', (0, 0, 2)), ('lohi', (0, 1, 1)),
                            ('t_lo', (1, 1, 0)), ('t_hi', (1, 0, 1)), ('tt_lo', (2, 1, 0)), ('tt_hi', (2, 0, 1))):
            assert abs(mp.diff(f, (t, lo, hi), order) - thr[name]) <= tol * size[name], (t, lo, hi, name)


@_at_dps
def _exact(rho, s, lo, hi, gx=GX, gw=GW):
    """(E h^(k), k = 0..4 (5 x n); the nine threshold moments (9 x n)) on the nodes, at 60 digits."""
    E, M = [], []
    for r_, s_, l_, u_ in zip(rho, s, lo, hi):
        r_, s_ = _mpf(r_), _mpf(s_)
        l_ = -mp.inf if l_ == -INF else _mpf(l_)
        u_ = mp.inf if u_ == INF else _mpf(u_)
        e, m = [mp.mpf(0)] * 5, [mp.mpf(0)] * 9
        for xk, wk in zip(gx, gw):
            t = r_ + mp.sqrt(s_) * mp.sqrt(2) * _mpf(xk)
            h, th = _forms(t, l_, u_)
            wk = _mpf(wk) / mp.sqrt(mp.pi)
            e = [p + wk * q for p, q in zip(e, h)]
            row = [th['t_hi'], th['tt_hi'] / 2, th['t_lo'], th['tt_lo'] / 2, th['hi'], th['lo'], th['hihi'], th['lolo'], th['lohi']]
            m = [p + wk * q for p, q in zip(m, row)]
        E.append([float(v) for v in e]); M.append([float(v) for v in m])
    return np.array(E).T, np.array(M).T


def _grid_points(n, seed):
    """n rows inside GRID: interior rows with D log-uniform, and both end categories; the corners among them."""
    rng = np.random.default_rng(seed)
    d_lo = rng.uniform(GRID['dist'][0], GRID['dist'][1], size=n)
    D = np.exp(rng.uniform(np.log(GRID['delta'][0]), np.log(GRID['delta'][1]), size=n))
    s = rng.uniform(GRID['s'][0], GRID['s'][1], size=n)
    d_lo[:4], D[:4], s[:4] = [12.0, -12.0 + 16.0, 12.0, 0.0], [16.0, 16.0, 2.0 ** -6, 2.0 ** -6], [3.0, 3.0, 0.0, 3.0]
    d_lo = np.maximum(d_lo, GRID['dist'][0] + D)                          # rho - hi = (rho - lo) - D stays inside
    rho = rng.normal(size=n)
    lo, hi = rho - d_lo, rho - d_lo + D
    kind = np.arange(n) % 4
    lo = np.where(kind == 2, -INF, lo)
    hi = np.where(kind == 3, INF, hi)
    return rho, s, lo, hi


def _err(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def test_reference_and_host_forms_against_mpmath_on_the_grid(go):
    """GRID, corners and both end categories included: the reference within CAP, the host forms within HOST; the threshold moments
    of the host within HOST and the reference's autograd in (lo, hi) within CAP."""
    rho, s, lo, hi = _grid_points(72, 5)
    want, wantm = _exact(rho, s, lo, hi)
    got = ref.eh_coefs(rho, s, lo, hi)
    host = go.ordinal_expected_h(rho, s, lo, hi, GX, GW)
    e_ref, e_host = _err(got, want), _err(host, want)
    print('on the grid: reference', e_ref.max(axis=1), 'host', e_host.max(axis=1))
    assert np.all(e_ref <= CAP) and np.all(e_host <= HOST)
    a1, a2 = go.ordinal_row_derivs(rho, s, lo, hi, GX, GW)
    assert np.array_equal(a1, host[1]) and np.array_equal(a2, 0.5 * host[2])
    hm = go.ordinal_threshold_moments(rho, s, lo, hi, GX, GW)
    scale = np.maximum(1.0, np.abs(wantm).max(axis=0))                    # c = 1 / D^2 on a narrow category: relative to the row's largest
    e_m = np.abs(hm - wantm) / scale
    print('threshold moments: host', e_m.max(axis=1))
    assert np.all(e_m <= HOST)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    r0 = ref._bound_derivs(t(rho), t(s), t(lo), t(hi), ref.GH_DEG, 0, [(0, 1), (1, 0), (0, 2), (2, 0), (1, 1)])
    r1 = ref._bound_derivs(t(rho), t(s), t(lo), t(hi), ref.GH_DEG, 1, [(0, 1), (1, 0)])
    r2 = ref._bound_derivs(t(rho), t(s), t(lo), t(hi), ref.GH_DEG, 2, [(0, 1), (1, 0)])
    refm = np.stack([r1[0].numpy(), 0.5 * r2[0].numpy(), r1[1].numpy(), 0.5 * r2[1].numpy(), r0[0].numpy(), r0[1].numpy(), r0[2].numpy(),
                     r0[3].numpy(), r0[4].numpy()])
    e_r = np.abs(refm - wantm) / scale
    print('threshold moments: reference autograd', e_r.max(axis=1))
    assert np.all(e_r <= CAP)
    # a sentinel's entries are exact zeros
    first, last = lo == -INF, hi == INF
    assert np.all(hm[[2, 3, 5, 7, 8]][:, first] == 0.0) and np.all(hm[[0, 1, 4, 6, 8]][:, last] == 0.0)


@_at_dps
def test_exact_moments_are_independent(go):
    """mpmath quadrature of h^(k)(t) N(t; rho, s) against the host node sums at 96 nodes: 1e-7 of max(1, |exact|) (the logistic
    function has poles at +-i pi: the rule converges, but not as for an entire function, which is why the quadrature is part of the
    model's definition and the reference runs on the class's own nodes)."""
    gx, gw = np.polynomial.hermite.hermgauss(96)
    for rho, s, lo, hi in ((0.3, 0.5, -0.4, 0.9), (-2.0, 2.0, 0.1, 0.6), (1.5, 0.3, -INF, 0.2), (0.2, 1.0, 1.1, INF)):
        r, v = _mpf(rho), _mpf(s)
        l = -mp.inf if lo == -INF else _mpf(lo)
        u = mp.inf if hi == INF else _mpf(hi)
        sd = mp.sqrt(v)
        dens = lambda t: mp.exp(-(t - r) ** 2 / (2 * v)) / mp.sqrt(2 * mp.pi * v)
        cuts = [r + j * sd for j in range(-40, 41, 4)]
        got = go.ordinal_expected_h([rho], [s], [lo], [hi], gx, gw)[:, 0]
        for k in range(5):
            want = float(mp.quad(lambda t: _forms(t, l, u)[0][k] * dens(t), cuts))
            assert abs(got[k] - want) <= 1e-7 * max(1.0, abs(want)), (rho, s, lo, hi, k, got[k], want)


def _rows(N, P, K, G):
    x, y, z, w, gid, o, alpha, free = ref.shape_data(N, P, K, G)
    return ref.rows_at(free, x, y, z, o, alpha, gid, G) + (y, w, alpha)


_inside_grid = ref.inside_grid


@pytest.mark.parametrize('N,P,K,G', ref.SHAPES)
def test_reference_meets_the_cap_at_every_row_of_the_test_problems(go, N, P, K, G):
    """Every row of every GPU data set lies inside GRID (asserted), and the reference's E h^(k) is within CAP there.  The data sets
    carry what the GPU tests rely on: J of {2, 3, 5, 16}, an empty category at N = 65, zero weights at N = 300."""
    rho, s, lo, hi, y, w, alpha = _rows(N, P, K, G)
    assert _inside_grid(rho, s, lo, hi)
    J = ref.J_OF[(N, P, K, G)]
    assert alpha.size == J - 1 and y.min() >= 0 and y.max() <= J - 1
    if N >= J:
        present = np.unique(y)
        assert (N == 65 and 2 not in present and present.size == J - 1) or present.size == J
    if N == 300:
        assert np.sum(w == 0.0) == 60
    assert np.array_equal(np.round(alpha / ref.GRID_UNIT) * ref.GRID_UNIT, alpha)
    want = _exact(rho, s, lo, hi)[0]
    got = ref.eh_coefs(rho, s, lo, hi)
    host = go.ordinal_expected_h(rho, s, lo, hi, GX, GW)
    err, err_h = _err(got, want), _err(host, want)
    print('reference against mpmath', (N, P, K, G), 'J', J, 'largest s', float(s.max()), 'errors by order', err.max(axis=1), 'host', err_h.max(axis=1))
    assert np.all(err <= CAP) and np.all(err_h <= HOST)


def test_grid_stride_data_set_lies_inside_the_grid():
    """The data set of tests/test_gpu_glmm_ordinal.py::test_grid_stride_of_the_threshold_pass (N = 131 137, seed 11) at its point; the
    profile-fit simulation is asserted inside GRID at its fitted points by the GPU test itself, which has them."""
    N, P, K, G, J = 2048 * 64 + 65, 2, 1, 3, 3
    x, y, z, w, gid, o, alpha, free = ref.problem(N, P, K, G, 11, J, empty_group=False)
    rho, s, lo, hi = ref.rows_at(free, x, y, z, o, alpha, gid, G)
    print('grid stride rows: rho - cut point in', float(np.min(rho - hi[np.isfinite(hi)].max())), float(np.max(rho - lo[np.isfinite(lo)].min())), 'largest s', float(s.max()))
    assert ref.inside_grid(rho, s, lo, hi)


@pytest.mark.parametrize('N,P,K,G', ref.SHAPES[:3] + ref.SHAPES[4:])
def test_reference_free_hessian_leaves_six_digits(N, P, K, G):
    """The precondition of the covariance and solve checks of the GPU tests (rtol 1e-6): the reference free Hessian of a data set is
    positive definite with a condition number below 1e8 (tabulated in DESIGN.md section 47).  (130, 64, 4, 2), whose dense autograd
    Hessian takes longest, is asserted by the GPU parity test alone."""
    x, y, z, w, gid, o, alpha, free = ref.shape_data(N, P, K, G)
    t = ref.targs(x, y, z, w, o, alpha, gid, G, ref.TEST_HYP)
    Hf = ref.value_grad_hess(ref.kl_free, free, t)[2]
    ev = np.linalg.eigvalsh(Hf)
    print('reference free Hessian', (N, P, K, G), 'smallest eigenvalue {:.3g} largest {:.3g} condition {:.2e}'.format(ev[0], ev[-1], ev[-1] / ev[0]))
    assert ev[0] > 0 and ev[-1] / ev[0] < 1e8


def test_reference_threshold_terms_against_central_differences():
    """The reference's autograd in alpha (gradient, tridiagonal Hessian, cross Hessian) against central differences of the reference's
    own data term and gradient at a step of 1e-5: 1e-7 of the largest entry."""
    N, P, K, G = 65, 5, 2, 3
    x, y, z, w, gid, o, alpha, free = ref.shape_data(N, P, K, G)
    t = ref.targs(x, y, z, w, o, alpha, gid, G, ref.TEST_HYP)
    g, H, cross = ref.threshold_terms(free, t)
    T = alpha.size
    assert np.all(np.triu(H, 2) == 0.0) and np.allclose(H, H.T, rtol=0, atol=1e-12 * np.abs(H).max())
    assert H[1, 2] == 0.0 and H[1, 1] != 0.0                              # category 2 is empty: alpha_2 and alpha_3 do not couple

    def f_and_grad(al):
        fr = torch.tensor(free, requires_grad=True)
        f = ref.data(ref.free_to_vec(fr, P, K, G), t[0], t[1], t[2], t[3], t[4], torch.tensor(al), t[6], G, t[9])
        gr, = torch.autograd.grad(f, fr)
        return float(f.detach()), gr.numpy()
    h = 1e-5
    for j in range(T):
        up, dn = alpha.copy(), alpha.copy()
        up[j] += h; dn[j] -= h
        (fu, gu), (fd, gd) = f_and_grad(up), f_and_grad(dn)
        assert abs((fu - fd) / (2 * h) - g[j]) <= 1e-7 * np.abs(g).max()
        assert np.max(np.abs((gu - gd) / (2 * h) - cross[:, j])) <= 1e-7 * np.abs(cross).max()
        gu_a, gd_a = ref.threshold_terms(free, t, up)[0], ref.threshold_terms(free, t, dn)[0]
        assert np.max(np.abs((gu_a - gd_a) / (2 * h) - H[:, j])) <= 1e-7 * np.abs(H).max()


def test_threshold_param_free_coordinates(go):
    """(alpha_1, gamma): the round trip, the Jacobian and the second-order term of the exponential against central differences."""
    al = np.array([-0.7, 0.1, 0.35, 2.0])
    par = go.ThresholdParam('threshold', al)
    f = par.get_free()
    assert np.allclose(f, [-0.7, np.log(0.8), np.log(0.25), np.log(1.65)], rtol=1e-15)
    par.set_free(f)
    assert np.allclose(par.get_vector(), al, rtol=0, atol=1e-15)
    A = par.free_to_vector_jac(f).toarray()
    A2 = [m.toarray() for m in par.free_to_vector_hess(f)]

    def vec(ff):
        q = go.ThresholdParam('q', al)
        q.set_free(ff)
        return np.array(q.get_vector())
    h = 1e-5
    for i in range(4):
        d = np.zeros(4); d[i] = h
        assert np.allclose((vec(f + d) - vec(f - d)) / (2 * h), A[:, i], rtol=0, atol=1e-9)
        for j in range(4):
            assert abs((vec(f + d)[j] - 2 * vec(f)[j] + vec(f - d)[j]) / h ** 2 - A2[j][i, i]) <= 1e-5
    for bad in ([0.0, 0.0], [1.0, 0.5], [0.0, np.nan], [], list(range(16))):
        with pytest.raises(ValueError):
            go.ThresholdParam('bad', np.array(bad, dtype=np.float64))


def test_category_probabilities_sum_to_one(go):
    rng = np.random.default_rng(1)
    rho, s = rng.normal(size=50) * 3.0, rng.uniform(0.0, 3.0, size=50)
    al = ref.thresholds_for(16)
    cum, prob = go.ordinal_category_probs(rho, s, al, GX, GW)
    assert cum.shape == (50, 15) and prob.shape == (50, 16)
    assert np.max(np.abs(prob.sum(1) - 1.0)) <= 1e-14 and np.all(prob > 0.0) and np.all(np.diff(cum, axis=1) > 0.0)
    # P(y <= j) of the model is sigma(alpha - t) under the integral: E h of the two-category row {y <= j} is -E log of it
    tab = np.concatenate([[-INF], al, [INF]])
    e0 = go.ordinal_expected_h(rho, 0.0, tab[3], tab[4], GX, GW)[0]
    assert np.allclose(np.exp(-e0), go.ordinal_category_probs(rho, 0.0, al, GX, GW)[1][:, 3], rtol=1e-12)

"""The committed exact values of the row-by-row tail tests, tests/golden/glmm_tail_exact.npz, without a GPU:
a seeded sample recomputed with mpmath, an independent route to the node terms, the host formulas' own figures and the mask
`resolvable` reproduced, and the share conditions under which the GPU test (tests/test_gpu_glmm_tails.py) may hold the device
pointwise.  Rows, measures and bounds: tests/glmm_tail_cases.py; the generator: tests/golden/make_glmm_tail_exact.py."""
import importlib.util
import os

import numpy as np
import pytest

import glmm_tail_cases as tc

SAMPLE = {'beta': 12, 'beta_disp': 12}                                   # rows per family, 40 where not named: the Beta rows cost 0.1 s each


@pytest.fixture(scope='module')
def gen():
    path = os.path.join(os.path.dirname(tc.FIXTURE), 'make_glmm_tail_exact.py')
    spec = importlib.util.spec_from_file_location('make_glmm_tail_exact', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module', autouse=True)
def pkg():
    import lrvb_amd
    return lrvb_amd


@pytest.mark.parametrize('family', tc.FAMILIES)
def test_fixture_holds_the_rows_of_the_helper(family):
    fx, r = tc.load(family), tc.rows(family)
    for k, a in r.items():
        assert np.array_equal(fx[k], a), (family, k)
    n = r['rho'].size
    nq = 4 if family in tc.DISPERSION else 5
    assert n % 64 != 0 and n <= 3000 and fx['deg'] == tc.DEG
    assert fx['exact'].shape == fx['mag'].shape == fx['host_rel'].shape == fx['host_abs'].shape == fx['resolvable'].shape == (nq, n)
    assert np.all(np.isfinite(fx['exact'])) and np.all(fx['mag'] >= np.abs(fx['exact']) * (1.0 - 1e-12))
    # every family reaches the far rows, the s = 0 rows and a threshold either side of t = 0
    assert r['rho'].min() <= -40.0 and r['rho'].max() >= 40.0 and {tc.S_MIN, 0.5, 3.0, 40.0} <= set(r['s']) and np.all(r['s'] > 0.0)
    th = r['rho'][r['kind'] == 2]
    assert np.any(th == 0.0) and np.any(th == np.nextafter(0.0, 1.0)) and np.any(th == np.nextafter(0.0, -1.0))
    # exact zeros: only values below the fp64 range (the far right tail of 1 - p), never a whole order
    assert np.all(np.any(fx['exact'] != 0.0, axis=-1)) and np.mean(fx['exact'] == 0.0) < 0.05
    has_mean = family in tc.HAS_MEAN
    assert np.all(np.isnan(fx['mean'])) != has_mean
    if has_mean:
        assert np.any(r['rho'] == tc.NEAR_OVERFLOW) or family in ('probit', 'beta')


@pytest.mark.parametrize('family', tc.FAMILIES)
def test_seeded_sample_recomputed_with_mpmath(gen, family):
    """At most 40 rows per family: recomputed, they round to the stored doubles bit for bit, and the mpmath values themselves lie
    within 2^-53 of them."""
    fx = tc.load(family)
    n = fx['rho'].size
    rng = np.random.default_rng([42, tc.FAMILIES.index(family)])
    idx = np.sort(rng.choice(n, size=min(SAMPLE.get(family, 40), n), replace=False))
    exact, mean, mag = gen.family_arrays(family, idx)
    assert np.array_equal(exact, fx['exact'][:, idx]) and np.array_equal(mag, fx['mag'][:, idx])
    assert np.array_equal(mean, fx['mean'][idx], equal_nan=True)
    # and before the rounding: the mpmath values themselves against the stored doubles
    import mpmath as mp
    worst = 0.0
    for n_ in idx[:3]:
        e, _, _ = gen.row_exact(family, *(fx[k][n_] for k in ('rho', 's', 'y', 'trials', 'phi')))
        for k, a in enumerate(e):
            if a != 0 and fx['exact'][k, n_] != 0.0:
                worst = max(worst, float(abs(a - mp.mpf(float(fx['exact'][k, n_]))) / abs(a)))
    assert worst <= 2.0 ** -53


def test_independent_route_to_the_node_terms(gen):
    """The generator's node terms by another route on a handful of entries, 1e-25 relative: the Beta chain rule on mpmath's polygamma
    against mpmath.diffs of the definition (as tests/test_glmm_beta_host_math.py::test_exact_moments_are_independent); the
    numerical derivatives of -log Phi, -log(1 - exp(-e^t)) and log(1 - (1 + e^eta)^-phi) against their explicit chain rules; the
    dispersion chain rules against mp.diff in (t, lambda)."""
    import mpmath as mp
    mp.mp.dps = 80
    worst = 0.0

    def cmp(got, want):
        return max(float(abs(g - w) / abs(w)) for g, w in zip(got, want))

    for t in (-40.0, -7.5, 0.7, 19.0, 40.0):
        for phi, l in ((0.3, -8.0), (15.0, 0.4), (3000.0, 3.0)):
            mp.mp.dps = 80 + int(0.45 * abs(t))
            t_, phi_, l_ = mp.mpf(t), mp.mpf(phi), mp.mpf(l)
            worst = max(worst, cmp(gen.beta_derivs(t_, phi_, l_), list(mp.diffs(gen.beta_h(phi_, l_), t_, 4))))
            got = gen.beta_disp_terms(t_, phi_, l_)
            f = gen.disp_def('beta_disp', l_)
            worst = max(worst, cmp(got, [mp.diff(f, (t_, mp.log(phi_)), o) for o in ((0, 1), (1, 1), (2, 1), (0, 2))]))
    mp.mp.dps = 80
    for t in (-40.0, -20.0, -8.0, -0.3, 8.0, 20.0, 40.0):
        t_ = mp.mpf(t)
        # probit: lambda = phi / Phi, h1' = -lambda, h1'' = lambda (t + lambda)
        lam = mp.npdf(t_) / mp.ncdf(t_)
        got = gen.probit_h1_derivs(t_)
        worst = max(worst, cmp(got[1:3], [-lam, lam * (t_ + lam)]))
        # softplus: sigma and sigma (1 - sigma)
        sg = 1 / (1 + mp.exp(-t_))
        worst = max(worst, cmp(gen.softplus_derivs(t_)[1:3], [sg, sg * (1 - sg)]))
        for phi, y in ((0.3, 0.0), (15.0, 7.0), (3000.0, 400.0)):
            phi_, y_ = mp.mpf(phi), mp.mpf(y)
            f = gen.disp_def('negbin_disp', y_)
            got = gen.negbin_disp_terms(t_, phi_, y_)
            want = [mp.diff(f, (t_ + mp.log(phi_), mp.log(phi_)), o) for o in ((0, 1), (1, 1), (2, 1), (0, 2))]
            # d_t at fixed lambda of the definition in (t, lambda) is d_eta at eta = t - lambda
            worst = max(worst, cmp(got, want))
    for t in (-40.0, -12.0, -2.0, 0.4, 2.5):
        t_ = mp.mpf(t)
        u = mp.exp(t_)
        r = u / mp.expm1(u)
        worst = max(worst, cmp(gen.cloglog_h1_derivs(t_)[1:3], [-r, -r * (1 - u - r)]))
        for phi in (0.05, 1.0, 50.0, 1e3):
            phi_ = mp.mpf(phi)
            sg, v = 1 / (1 + mp.exp(-t_)), phi_ * mp.log1p(mp.exp(t_))
            worst = max(worst, cmp(gen.ztnb_g_derivs(t_, phi_)[1:2], [phi_ * sg / mp.expm1(v)]))
    print('independent routes, relative:', worst)
    assert worst <= 1e-25


@pytest.mark.parametrize('family', tc.FAMILIES)
def test_host_figures_and_mask_are_reproduced(family):
    """The host functions re-evaluated on the whole fixture give the stored figures and the stored mask."""
    fx = tc.load(family)
    rel, ab, res = tc.host_figures(family, fx, fx['exact'], fx['mag'])
    assert np.array_equal(res, fx['resolvable'])
    assert np.array_equal(rel, fx['host_rel']) and np.array_equal(ab, fx['host_abs'])
    print(family, 'host pointwise where resolvable', np.where(res, rel, 0.0).max(-1), 'absolute', ab.max(-1), 'bounds', tc.abs_bounds(ab),
          'share', res.mean(-1))
    assert np.all(np.where(res, rel, 0.0) <= tc.CAP / 4.0)
    if family in tc.HAS_MEAN:
        _, mean = tc.host(family, fx)
        ok = np.isfinite(fx['mean'])
        assert np.all(ok | (fx['rho'] + 0.5 * fx['s'] > 700.0))
        err = tc.rel_err(mean[ok], fx['mean'][ok])
        print(family, 'host response mean, relative', err.max())
        assert np.all(err <= 1e-12)


def test_share_conditions():
    """Where the GPU test may hold the device pointwise (tests/glmm_tail_cases.py): the whole of the existing CPU grids of the Beta
    and the zero-truncated NB2 family at every order and the NB2 threshold rows; at least 90 % of all entries of logistic,
    binomial-logit, Beta and zero-truncated NB2 per family and order; probit, cloglog and zero-truncated Poisson 100 % at orders 0
    and 1 and at least 50 % at orders 2 to 4 (their formulas lose pointwise accuracy in the left tail: DESIGN.md section 42)."""
    for family in ('beta', 'ztnegbin'):
        fx = tc.load(family)
        old = fx['kind'] == 0
        assert old.sum() == (540 if family == 'beta' else 96)
        assert np.all(fx['resolvable'][:, old]), (family, np.argwhere(~fx['resolvable'][:, old]))
    fx = tc.load('ztnegbin')
    assert np.all(fx['resolvable'][:, fx['kind'] == 2])
    corner = (fx['kind'] == 2) & (fx['rho'] < -6.0)                       # either side of eta = log 1e-3 and of v = 0.01
    assert corner.sum() == 35 and np.any(fx['rho'][corner] > tc.ETA_SMALL) and np.any(fx['rho'][corner] < tc.ETA_SMALL)
    v = fx['phi'][corner] * np.log1p(np.exp(fx['rho'][corner]))
    assert np.any(v < 0.01) and np.any(v > 0.01)
    print('zero-truncated NB2, host pointwise on the corner threshold rows:', fx['host_rel'][:, corner].max(-1))
    assert np.all(fx['host_rel'][:, corner] <= tc.CAP / 4.0)         # measured 1.4e-12 (order 4, v just above 0.01 at eta = -8)
    for family in ('logistic', 'binomial', 'negbin', 'beta', 'ztnegbin'):
        share = tc.load(family)['resolvable'].mean(-1)
        assert np.all(share >= 0.9), (family, share)
    for family in tc.DISPERSION:                                         # differences of node sums: most entries, not nine in ten
        assert np.all(tc.load(family)['resolvable'].mean(-1) >= 0.5)
    for family in ('probit', 'cloglog', 'ztpoisson'):
        res = tc.load(family)['resolvable']
        assert np.all(res[:2]), (family, np.argwhere(~res[:2]))
        assert np.all(res[2:].mean(-1) >= 0.5), (family, res.mean(-1))


@pytest.mark.parametrize('family', [f for f in tc.FAMILIES if f not in tc.DISPERSION])
def test_device_mask_only_leaves_out_what_the_entry_cannot_return(family):
    """`device_mask` differs from `resolvable` only at orders 0 and 1 of a canonical entry, and only where the y rho (y) that the
    entry subtracts is more than 999 times the exact value."""
    fx = tc.load(family)
    m = tc.device_mask(family, fx)
    out = fx['resolvable'] & ~m
    assert not np.any(out[2:])
    if family not in tc.MINUS_Y:
        assert not np.any(out)
        return
    e = np.abs(fx['exact'])
    assert np.all(np.abs(fx['y'] * fx['rho'])[out[0]] > 0.999e3 * e[0][out[0]] - 1e-3 * fx['mag'][0][out[0]])
    assert np.all(np.abs(fx['y'])[out[1]] > 0.999e3 * e[1][out[1]] - 1e-3 * fx['mag'][1][out[1]])
    print(family, 'entries left to the absolute measure by the subtraction of y rho, y:', int(out[0].sum()), int(out[1].sum()), 'of', e.shape[1])

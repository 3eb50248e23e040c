"""The Gamma policies of csrc/k_glmm_walk.h (GammaLik, GammaDispLik) ROW BY ROW in their tails, on the GPU, against the exact values
of tests/golden/glmm_gamma_tail_exact.npz (mpmath at 60 digits from the fp64 rows; written by
tests/golden/make_glmm_gamma_tail_exact.py).  |A| up to 700 for A = (log y - rho) + s / 2, phi from 1e-3 to 1e8.

The data set is one row per group (G = N, K = 1, z = 1, P = 1, x = 0), N = 184 no multiple of the 64-row tile, unit weights; rho is
the row's offset (e = 0) and s the group's variance r, so that the kernels see exactly the fixture's numbers.  It runs a second time
with its rows in reversed order.  Three paths form g independently: the rows kernel (`coefs`), the influence kernel (`infl`) and the
dispersion kernel (`dmoments`); each is held against the exact values, never against another path's bits.

Bounds, derived and not tuned.  With u = 2^-53: the kernel forms d = fl(log y - rho), an error of u |d|; A = fl(d + s / 2) (s / 2 is
exact), another u |A|; exp of it turns the absolute error of its argument into a relative one of the result and adds its own
(1 ulp = 2 u for the library's exp); the product with phi adds u; the stored exact value is itself rounded, u.  So
    |g_dev - g| <= B_g g,   B_g = (|d| + |A| + 4) u        -- about (|A| + a small constant) ulp,
and the coefficients a2, c11, c12, c22 are g times a power of two, exactly.  a1 = fl(phi - g_dev) is a difference:
    |a1_dev - a1| <= B_g g + 2 u max(phi, g)  <=  (B_g + 2 u) max(phi, g)          -- absolute in max(phi, g),
and the value fl(g_dev + fl(phi rho)):  (B_g + 3 u) (g + phi |rho|).  The sums over the whole data set (`value`, d[0], d[1]) are held
to the sum of the row bounds plus N u times the sum of the magnitudes.  The test prints every error as a ratio to its bound; the
largest ratios are recorded in DESIGN.md section 43."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


@pytest.fixture(scope='module')
def fx():
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'glmm_gamma_tail_exact.npz'))
    fx = {k: f[k] for k in f.files}
    assert fx['rho'].size % 64 != 0 and fx['rho'].size > 128
    assert np.max(np.abs(fx['A'])) >= 699.0 and fx['phi'].min() == 1e-3 and fx['phi'].max() == 1e8
    return fx


def _context(vb, fx, order):
    hip = vb._hip
    N = order.size
    sel = lambda k: np.ascontiguousarray(fx[k][order])
    blocks = [dict(kind=hip.BLOCK_BOX, free_size=2, vec_size=2, dim0=2, dim1=0, lb=-np.inf, ub=np.inf)]
    ctx = vb.DeviceContext(blocks, loss='poisson', n_obs=N, n_cols=1)
    ctx.set_data(hip.SLOT_X, np.zeros((N, 1)))
    ctx.set_data(hip.SLOT_Y, sel('ly'))
    ctx.set_groups(np.arange(N), N)
    ctx.set_group_design(np.ones((N, 1)))
    ctx.set_weights(np.ones(N))
    ctx.set_offset(sel('rho'))
    ctx.set_dispersion(sel('phi'))
    return ctx, (np.zeros(1), np.ones(1), np.zeros((N, 1)), sel('s').reshape(N, 1))


def _run(vb, fx, order):
    """(value, N x 5 [a1, a2, c11, c12, c22]) of the terms entry, N x 2 [a1', a2'] of the influence entry, (d, N x 2) of the
    dispersion entry, in the order of the rows `order`."""
    ctx, pt = _context(vb, fx, order)
    N = order.size
    val, _, _, gs = ctx.glmm_gamma_terms(*pt, want_border=False)
    assert gs.shape == (N, 5)
    A = np.zeros((2, 2 + 2 * N))
    A[0, 2:2 + N] = 1.0
    A[1, 2 + N:] = 1.0
    infl = ctx.glmm_gamma_obs_influence(*pt, A)
    assert infl.shape == (N, 2)
    d, _, cl = ctx.glmm_gamma_dispersion_terms(*pt)
    assert cl.shape == (N, 2)
    ctx.close()
    return val, gs, infl, d, cl


def test_rows_against_exact_values_and_positions(vb, fx):
    N = fx['rho'].size
    fwd, rev = np.arange(N), np.arange(N)[::-1]
    val, gs, infl, d, cl = _run(vb, fx, fwd)
    val_r, gs_r, infl_r, d_r, cl_r = _run(vb, fx, rev)
    # position: the reversed run returns the same bits per row on all three paths
    assert np.array_equal(gs_r[::-1], gs) and np.array_equal(infl_r[::-1], infl) and np.array_equal(cl_r[::-1], cl)
    g, a1, phi, rho = fx['g'], fx['a1'], fx['phi'], fx['rho']
    Bg = (np.abs(fx['d']) + np.abs(fx['A']) + 4.0) * U
    Ba1 = (Bg + 2.0 * U) * np.maximum(phi, g)
    ratios = {}
    # the rows kernel: a2, c11, c12, c22 are g times 1/2, 1, -1/2, 1/4
    for col, f in ((1, 0.5), (2, 1.0), (3, -0.5), (4, 0.25)):
        ratios['terms ' + ('a1', 'a2', 'c11', 'c12', 'c22')[col]] = np.abs(gs[:, col] - f * g) / (Bg * g)
    ratios['terms a1'] = np.abs(gs[:, 0] - a1) / Ba1
    # the influence kernel and the dispersion kernel: a1' = phi - g, a2' = g / 2
    for name, got in (('influence', infl), ('dispersion', cl)):
        ratios[name + ' a1'] = np.abs(got[:, 0] - a1) / Ba1
        ratios[name + ' a2'] = np.abs(got[:, 1] - 0.5 * g) / (Bg * g)
    for k, r in ratios.items():
        i = int(np.argmax(r))
        print('{:16s} largest error / bound {:.3f} at A = {:.1f}, phi = {:g}'.format(k, float(r[i]), float(fx['A'][i]), float(phi[i])))
        assert np.all(np.isfinite(r)) and np.all(r <= 1.0), k
    assert np.all(gs[:, 3] < 0.0) and np.all(gs[:, [1, 2, 4]] > 0.0)    # the sign of c12
    # the sums over the data set: the value, and d[0] = d[1] = the value by the other kernel
    mag = g + phi * np.abs(rho)
    bound = float(np.sum((Bg + 3.0 * U) * mag) + N * U * np.sum(mag))
    import math
    want = math.fsum(fx['value'])
    for name, got in (('value', val), ('d[0]', d[0]), ('d[1]', d[1]), ('value, reversed', val_r)):
        print('{:16s} error / bound {:.3f}'.format(name, abs(got - want) / bound))
        assert abs(got - want) <= bound
    assert d[0] == d[1]


def test_single_rows_by_value(vb, fx):
    """The value of one-row data sets at the extreme rows: the largest and smallest g, the largest |A| of either sign at the
    smallest and largest phi that keep g in range."""
    A, g, phi = fx['A'], fx['g'], fx['phi']
    pick = sorted({int(np.argmax(g)), int(np.argmin(g)), int(np.argmax(A + 1e-3 * np.log(phi))), int(np.argmin(A - 1e-3 * np.log(phi))),
                   int(np.argmax(np.abs(fx['d'])))})
    for i in pick:
        val, gs, _, d, _ = _run(vb, fx, np.array([i]))
        Bg = (abs(fx['d'][i]) + abs(A[i]) + 4.0) * U
        bound = (Bg + 3.0 * U) * (g[i] + phi[i] * abs(fx['rho'][i]))
        print('row', i, 'A', float(A[i]), 'phi', float(phi[i]), 'value error / bound', abs(val - fx['value'][i]) / bound)
        assert abs(val - fx['value'][i]) <= bound and abs(d[0] - fx['value'][i]) <= bound and d[1] == d[0]

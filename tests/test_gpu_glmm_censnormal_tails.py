"""The censored Gaussian policies of csrc/k_glmm_walk.h (CensNormalLik, CensNormalDispLik) ROW BY ROW in their tails, on the GPU, against
the exact values of tests/golden/glmm_censnormal_tail_exact.npz (mpmath at 60 digits from the fp64 rows; written by
tests/golden/make_glmm_censnormal_tail_exact.py).  The argument at the centre a_0 = delta r (rho - y) runs over
+-{0, 1, 5, 5.01, 38, 700}, phi over {1e-6, 1, 1e8}, phi s over {1e-4, 1e-2} (the nodes stay in the tail), all three statuses.

The data set is one row per group (G = N, K = 1, z = 1, P = 1, x = 0), N = 165 no multiple of the 64-row tile, unit weights; rho is
the row's offset (e = 0) and s the group's variance r, so that the kernels see exactly the fixture's numbers.  It runs a second time
with its rows in reversed order: equal bits per row.  Three paths evaluate the row independently: the rows kernel (`moments`, h1<5>),
the influence kernel (`infl`, h1<2>) and the dispersion kernel (`dmoments`); each is held against the exact values, never against
another path's bits.

Bounds, derived and not tuned.  u = 2^-53.  A censored quantity is Q = pref sum_k w_k f(a_k) with pref a power of delta r.
  1. The probit h1^(j) at the argument a carries the error pinned in DESIGN.md section 42 (value 1e-10 relative; orders 1 to 4
     7.1e-15, 2.2e-14, 1.4e-13, 8.0e-11 of max(1, |H^(j)|)); below a = -40, where section 42 has no rows, the rounding model of the left
     tail is added: d = a + lambda from the continued fraction to a few ulp, w = lambda d and 1 - w to 16 ulp ABSOLUTE, so that
     H''' = lambda (1 - w) - w d carries 16 |a| ulp and H'''' = -H''' (d + lambda) - 2 w (1 - w) carries 16 a^2 ulp.  Summed with the
     weights and multiplied by |pref| = phi^(j/2): `tail`.
  2. Forming a_k: u = fl(o - y) (1 ulp of |u|), sqrt(s) and sqrt(2) x_k (1 ulp each), the fused u + sqrt(s) sx_k (1 ulp), delta r (1 ulp),
     the product (1 ulp): |a_dev - a_k| <= 4 u A_k with A_k = r (|u| + sqrt(2 s) |x_k|) >= |a_k|.  It moves f by |f'(a_k)|: `prop` holds
     |pref| sum w A_k |f'(a_k)|, with f' from the next derivative (H^(5) for the fourth).
  3. The sums and products themselves: five fused accumulations per lane and two shuffle additions (7 ulp of the magnitudes), the
     powers of delta r (up to 4 ulp), the stored exact value (1 ulp): 12 u `mag`, mag = |pref| sum w |terms of f|.
  bound = tail + 4 u prop + 12 u mag.
An observed row is closed form; its bound is the ulp count of its operations: E_0 = 0.5 (phi (u u + s)): u (1), u u (2 + 1), + s (1),
phi (1), stored (1) = 7 ulp; E_1 = phi u: 3 ulp; E_2 = phi exactly; E_3 = E_4 = 0 exactly.  The coefficients are E_j times 1, 1/2, 1,
1/2, 1/4, exactly.  The sums over the data set (`value`, d[0], d[1]) are held to the sum of the row bounds plus N u times the sum of the
magnitudes.  The test prints every error as a ratio to its bound; the largest ratios are recorded in DESIGN.md section 45."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NAMES = ('E0', 'E1', 'E2', 'E3', 'E4', 'D1', 'D2', 'L1', 'L2')
OBS_ULP = np.array([7.0, 3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 7.0, 7.0])


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


@pytest.fixture(scope='module')
def fx():
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'glmm_censnormal_tail_exact.npz'))
    fx = {k: f[k] for k in f.files}
    N = fx['o'].size
    assert N % 64 != 0 and N > 128
    assert np.max(np.abs(fx['a0'])) >= 699.0 and fx['phi'].min() == 1e-6 and fx['phi'].max() == 1e8
    assert all(np.any(fx['delta'] == d) for d in (-1.0, 0.0, 1.0))
    obs = fx['delta'] == 0.0
    fx['bound'] = np.where(obs[:, None], OBS_ULP[None, :] * U * fx['mag'], fx['tail'] + 4.0 * U * fx['prop'] + 12.0 * U * fx['mag'])
    return fx


def _context(vb, fx, order):
    hip = vb._hip
    N = order.size
    sel = lambda k: np.ascontiguousarray(fx[k][order])
    blocks = [dict(kind=hip.BLOCK_BOX, free_size=2, vec_size=2, dim0=2, dim1=0, lb=-np.inf, ub=np.inf)]
    ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=1)
    ctx.set_data(hip.SLOT_X, np.zeros((N, 1)))
    ctx.set_data(hip.SLOT_Y, sel('y'))
    ctx.set_groups(np.arange(N), N)
    ctx.set_group_design(np.ones((N, 1)))
    ctx.set_weights(np.ones(N))
    ctx.set_offset(sel('o'))
    ctx.set_dispersion(sel('phi'))
    ctx.set_censoring(sel('delta').astype(np.int32))
    gh = np.polynomial.hermite.hermgauss(20)
    return ctx, (np.zeros(1), np.ones(1), np.zeros((N, 1)), sel('s').reshape(N, 1)) + gh


def _run(vb, fx, order):
    """(value, N x 5 [a1, a2, c11, c12, c22]) of the terms entry, N x 2 [a1', a2'] of the influence entry, (d, N x 2) of the
    dispersion entry, in the order of the rows `order`."""
    ctx, pt = _context(vb, fx, order)
    N = order.size
    val, _, _, gs = ctx.glmm_censnormal_terms(*pt, want_border=False)
    assert gs.shape == (N, 5)
    A = np.zeros((2, 2 + 2 * N))
    A[0, 2:2 + N] = 1.0
    A[1, 2 + N:] = 1.0
    infl = ctx.glmm_censnormal_obs_influence(*pt, A)
    assert infl.shape == (N, 2)
    d, _, cl = ctx.glmm_censnormal_dispersion_terms(*pt)
    assert cl.shape == (N, 2)
    ctx.close()
    return val, gs, infl, d, cl


def _ratio(err, bound):
    """err / bound, with 0 / 0 = 0 (an exact zero held exactly) and anything / 0 = inf."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0.0, 0.0, err / bound)


def test_rows_against_exact_values_and_positions(vb, fx):
    N = fx['o'].size
    fwd, rev = np.arange(N), np.arange(N)[::-1]
    val, gs, infl, d, cl = _run(vb, fx, fwd)
    val_r, gs_r, infl_r, d_r, cl_r = _run(vb, fx, rev)
    # position: the reversed run returns the same bits per row on all three paths (the status comes from the row's own entry)
    assert np.array_equal(gs_r[::-1], gs) and np.array_equal(infl_r[::-1], infl) and np.array_equal(cl_r[::-1], cl)
    ex, bound = fx['exact'], fx['bound']
    ratios = {}
    # the rows kernel: a1 = E1, a2 = E2 / 2, c11 = E2, c12 = E3 / 2, c22 = E4 / 4 -- powers of two, exact
    for col, (j, f) in enumerate(((1, 1.0), (2, 0.5), (2, 1.0), (3, 0.5), (4, 0.25))):
        ratios['terms ' + ('a1', 'a2', 'c11', 'c12', 'c22')[col]] = _ratio(np.abs(gs[:, col] - f * ex[:, j]), f * bound[:, j])
    ratios['influence a1'] = _ratio(np.abs(infl[:, 0] - ex[:, 1]), bound[:, 1])
    ratios['influence a2'] = _ratio(np.abs(infl[:, 1] - 0.5 * ex[:, 2]), 0.5 * bound[:, 2])
    ratios['dispersion d1'] = _ratio(np.abs(cl[:, 0] - ex[:, 5]), bound[:, 5])
    ratios['dispersion d2'] = _ratio(np.abs(cl[:, 1] - 0.5 * ex[:, 6]), 0.5 * bound[:, 6])
    for k, r in ratios.items():
        i = int(np.argmax(r))
        print('{:16s} largest error / bound {:.3f} at a_0 = {:.2f}, phi = {:g}, delta = {:g}'.format(k, float(r[i]), float(fx['a0'][i]), float(fx['phi'][i]),
                                                                                               float(fx['delta'][i])))
        assert np.all(np.isfinite(r)) and np.all(r <= 1.0), k
    obs = fx['delta'] == 0.0
    assert np.all(gs[obs][:, 3:] == 0.0) and np.array_equal(gs[obs][:, 2], fx['phi'][obs])      # the closed form: exact zeros, c11 = phi
    assert np.all(gs[:, 0][fx['delta'] == 1.0] <= 0.0) and np.all(gs[:, 0][fx['delta'] == -1.0] >= 0.0)   # the sign of delta in the odd derivatives
    # the sums over the data set: the value (E0), d[0] (L1) and d[1] (L2)
    for name, got, j in (('value', val, 0), ('value, reversed', val_r, 0), ('d[0]', d[0], 7), ('d[1]', d[1], 8), ('d[0], reversed', d_r[0], 7)):
        b = float(np.sum(bound[:, j]) + N * U * np.sum(fx['mag'][:, j]))
        want = math.fsum(ex[:, j])
        print('{:16s} error / bound {:.3f}'.format(name, abs(got - want) / b))
        assert abs(got - want) <= b


def test_single_rows_by_value(vb, fx):
    """The value and the two lambda-sums of one-row data sets at the extreme rows: the deepest left tail at the smallest and largest
    phi, the threshold rows next to a = -5, an observed row at r u = 700, and a right tail where everything is an exact zero."""
    a0, phi, delta = fx['a0'], fx['phi'], fx['delta']
    cens = delta != 0.0
    pick = sorted({int(np.argmin(np.where(cens & (phi == 1e-6), a0, np.inf))), int(np.argmin(np.where(cens & (phi == 1e8), a0, np.inf))),
                   int(np.argmin(np.where(cens, np.abs(a0 + 5.01), np.inf))), int(np.argmin(np.where(cens, np.abs(a0 + 5.0), np.inf))),
                   int(np.argmax(np.where(cens, a0, -np.inf))), int(np.argmax(np.where(~cens, fx['mag'][:, 0], -np.inf)))})
    for i in pick:
        val, gs, _, d, _ = _run(vb, fx, np.array([i]))
        b = fx['bound'][i]
        print('row', i, 'a_0', float(a0[i]), 'phi', float(phi[i]), 'delta', float(delta[i]), 'value, d[0], d[1] error / bound',
              [float(_ratio(np.abs(np.float64(g) - fx['exact'][i, j]), b[j] + U * fx['mag'][i, j])) for g, j in ((val, 0), (d[0], 7), (d[1], 8))])
        for g, j in ((val, 0), (d[0], 7), (d[1], 8)):
            assert abs(g - fx['exact'][i, j]) <= b[j] + U * fx['mag'][i, j]

"""The ordinal policy of csrc/k_glmm_walk.h (OrdinalLik) and the threshold pass glmm_thr_rows_kernel ROW BY ROW in their tails, on the
GPU, against the exact values of tests/golden/glmm_ordinal_tail_exact.npz (mpmath at 60 digits from the fp64 rows; written by
tests/golden/make_glmm_ordinal_tail_exact.py).  rho - hi and rho - lo run over +-{0, 1e-9, 1, 38, 700}, D over
{1e-8, 1e-3, 1, 50, 800}, both end categories with their +-inf sentinel, s over {1e-4, 1e-2} (the nodes stay in the tail).

The data set is one row per group (G = N, K = 1, z = 1, P = 1, x = 0), N = 216 no multiple of the 64-row tile, unit weights; rho is the
row's offset (e = 0) and s the group's variance r, so that the kernels see exactly the fixture's numbers.  It runs a second time with
its rows in reversed order: equal bits per row.  Three paths evaluate the row independently: the rows kernel (`moments`, node<5>),
the influence kernel (`infl`, node<2>) and the threshold kernel (`thr_moments` and the closed forms in D); each is held against the
exact values, never against another path's bits.

Bounds, derived and not tuned.  u = 2^-53.  A quantity is Q = sum_k w_k f(a_k or b_k) (+ a closed form in D).
  1. LogisticLik's node expressions at an argument x, with exp, log1p and the division good to 1 ulp: e = exp(-|x|) (1),
     ie = 1 / (1 + e) (3), sg = ie or e ie (5), g2 = e ie ie (9), softplus = max(x, 0) + log1p(e) (3) -- relative; (1 - e) ie carries
     6 ulp ABSOLUTE where 1 - e cancels, so g3 = +-g2 (1 - e) ie carries 16 ulp of g2, and g4 = g2 (1 - 6 g2) 26 ulp of g2 (g2 <= 1/4).
     Summed with the weights: `node`.
  2. Forming the argument: the fold fl(alpha - o) (1 ulp of |alpha - o|), sqrt(s) and sqrt(2) x_k (1 ulp each, and the constant sqrt 2),
     their fused product with rho = 0 (1), the subtraction (1): |x_dev - x| <= 6 u A_k with A_k = |alpha - o| + sqrt(2 s) |x_k|.  It moves f
     by |f'(x)|: `prop` holds sum w A_k |f'|, with f' the next derivative (sigma'''' for the fourth).
  3. The sums themselves: five fused accumulations per lane, two shuffle additions, the signed sum of the two sides and the half of
     a2 / d2 where it is not a power-of-two scaling: 9 u `mag`, mag = sum w |terms of f|; the stored exact value and the last addition:
     1 ulp of |Q|.
  4. The closed forms in D = fl(tab[y + 1] - tab[y]) (1 ulp of D): -log(1 - e^-D), r = 1 / expm1(D) and c = e^-D / expm1(-D)^2 move by up
     to D ulp of themselves with D (their logarithmic derivatives in log D are at most D + 2) and carry 8 ulp of their own operations:
     (8 + D) u `closed`.
  bound = u (node + 6 prop + 9 mag + |Q|) + (8 + D) u closed.
The sums over the data set (the value, g, H diagonal and off-diagonal) are held to the sum of the row bounds plus N u times the sum
of the magnitudes.  The test prints every error as a ratio to its bound; the largest ratios are recorded in DESIGN.md section 47."""
import math
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
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'glmm_ordinal_tail_exact.npz'))
    fx = {k: f[k] for k in f.files}
    N, T = fx['o'].size, fx['alpha'].size
    assert N % 64 != 0 and N > 128 and T == 6
    cat = fx['cat'].astype(np.int64)
    assert set(cat) == set(range(T + 1))                                 # every category, both end categories among them
    tab = np.concatenate([[-np.inf], fx['alpha'], [np.inf]])
    D = tab[cat + 1] - tab[cat]
    assert np.allclose(sorted(set(D[np.isfinite(D)])), [1e-8, 1e-3, 1.0, 50.0, 800.0], rtol=1e-6)
    d_hi = (fx['o'] - tab[cat + 1])[cat < T]
    assert np.max(np.abs(d_hi)) >= 700.0 and np.any(np.abs(np.abs(d_hi) - 1e-9) < 1e-12) and np.any(d_hi == 0.0)
    Dc = np.where(np.isfinite(D), D, 0.0)
    fx['icat'], fx['D'] = cat, D
    fx['bound'] = U * (fx['node'] + 6.0 * fx['prop'] + 9.0 * fx['mag'] + np.abs(fx['exact'])) + (8.0 + Dc)[:, None] * U * fx['closed']
    return fx


def _run(vb, fx, order):
    """value, N x 5 [a1, a2, c11, c12, c22] of the terms entry, N x 2 [a1', a2'] of the influence entry and the five outputs of the
    threshold entry, in the order of the rows `order`."""
    hip = vb._hip
    N = order.size
    sel = lambda k: np.ascontiguousarray(fx[k][order])
    blocks = [dict(kind=hip.BLOCK_BOX, free_size=2, vec_size=2, dim0=2, dim1=0, lb=-np.inf, ub=np.inf)]
    ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=1)
    ctx.set_data(hip.SLOT_X, np.zeros((N, 1)))
    ctx.set_data(hip.SLOT_Y, sel('cat'))
    ctx.set_groups(np.arange(N), N)
    ctx.set_group_design(np.ones((N, 1)))
    ctx.set_weights(np.ones(N))
    ctx.set_offset(sel('o'))
    ctx.set_thresholds(fx['alpha'])
    pt = (np.zeros(1), np.ones(1), np.zeros((N, 1)), sel('s').reshape(N, 1)) + tuple(np.polynomial.hermite.hermgauss(20))
    val, _, _, gs = ctx.glmm_ordinal_terms(*pt, want_border=False)
    assert gs.shape == (N, 5)
    A = np.zeros((2, 2 + 2 * N))
    A[0, 2:2 + N] = 1.0
    A[1, 2 + N:] = 1.0
    infl = ctx.glmm_ordinal_obs_influence(*pt, A)
    assert infl.shape == (N, 2)
    thr = ctx.glmm_ordinal_threshold_terms(*pt)
    assert thr[4].shape == (N, fx['alpha'].size, 2)
    ctx.close()
    return val, gs, infl, thr


def _ratio(err, bound):
    """err / bound, with 0 / 0 = 0 (an exact zero held exactly) and anything / 0 = inf."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0.0, 0.0, err / bound)


def test_rows_against_exact_values_and_positions(vb, fx):
    N, T = fx['o'].size, fx['alpha'].size
    cat = fx['icat']
    fwd, rev = np.arange(N), np.arange(N)[::-1]
    val, gs, infl, thr = _run(vb, fx, fwd)
    val_r, gs_r, infl_r, thr_r = _run(vb, fx, rev)
    # position: the reversed run returns the same bits per row on all three paths (hi and lo come from the row's own entry)
    assert np.array_equal(gs_r[::-1], gs) and np.array_equal(infl_r[::-1], infl) and np.array_equal(thr_r[4][::-1], thr[4])
    ex, bound = fx['exact'], fx['bound']
    ratios = {}
    for col, (j, f) in enumerate(((1, 1.0), (2, 0.5), (2, 1.0), (3, 0.5), (4, 0.25))):
        ratios['terms ' + ('a1', 'a2', 'c11', 'c12', 'c22')[col]] = _ratio(np.abs(gs[:, col] - f * ex[:, j]), f * bound[:, j])
    ratios['influence a1'] = _ratio(np.abs(infl[:, 0] - ex[:, 1]), bound[:, 1])
    ratios['influence a2'] = _ratio(np.abs(infl[:, 1] - 0.5 * ex[:, 2]), 0.5 * bound[:, 2])
    cl = thr[4]
    has_hi, has_lo = cat < T, cat >= 1
    rows = np.arange(N)
    for name, side, col, j in (('threshold d1 hi', has_hi, 0, 5), ('threshold d2 hi', has_hi, 1, 6), ('threshold d1 lo', has_lo, 0, 7), ('threshold d2 lo', has_lo, 1, 8)):
        idx = (cat if 'hi' in name else cat - 1)[side]
        ratios[name] = _ratio(np.abs(cl[rows[side], idx, col] - ex[side, j]), bound[side, j])
    # what a row does not touch is an exact zero
    touched = np.zeros((N, T), dtype=bool)
    touched[rows[has_hi], cat[has_hi]] = True
    touched[rows[has_lo], cat[has_lo] - 1] = True
    assert np.all(cl[~touched] == 0.0)
    for k, r in ratios.items():
        i = int(np.argmax(r))
        print('{:18s} largest error / bound {:.3f} at rho = {:.9g}, category {:d}, D = {:g}, s = {:g}'.format(k, float(r[i]), float(fx['o'][i]), int(cat[i]), float(fx['D'][i]),
                                                                                                      float(fx['s'][i])))
        assert np.all(np.isfinite(r)) and np.all(r <= 1.0), k
    # the sign of the lo term's odd orders: far below lo the row pushes t up (a1 < 0), far above hi down
    tab = np.concatenate([[-np.inf], fx['alpha'], [np.inf]])
    assert np.all(gs[:, 0][fx['o'] < tab[cat] - 30.0] < -0.99) and np.all(gs[:, 0][fx['o'] > tab[cat + 1] + 30.0] > 0.99)
    # the sums over the data set: the value and the three scalar outputs of the threshold pass, entry by entry
    sums = [('value', val, ex[:, 0], bound[:, 0], fx['mag'][:, 0]), ('value, reversed', val_r, ex[:, 0], bound[:, 0], fx['mag'][:, 0])]
    for run, tag in ((thr, ''), (thr_r, ', reversed')):
        for j in range(T):
            hi_rows, lo_rows = cat == j, cat == j + 1
            part = lambda a, k1, k2: np.concatenate([a[hi_rows, k1], a[lo_rows, k2]])
            sums.append(('g[%d]%s' % (j, tag), run[0][j], part(ex, 9, 10), part(bound, 9, 10), part(fx['mag'] + fx['closed'], 9, 10)))
            sums.append(('H diag[%d]%s' % (j, tag), run[1][j], part(ex, 11, 12), part(bound, 11, 12), part(fx['mag'] + fx['closed'], 11, 12)))
            if j + 1 < T:
                sums.append(('H off[%d]%s' % (j, tag), run[2][j], ex[lo_rows, 13], bound[lo_rows, 13], fx['closed'][lo_rows, 13]))
    worst = {}
    for name, got, e, b, m in sums:
        tol = float(np.sum(b) + N * U * np.sum(m))
        want = math.fsum(e)
        r = abs(got - want) / tol if tol > 0.0 else (0.0 if got == want else np.inf)
        key = name.split('[')[0].split(',')[0]
        worst[key] = max(worst.get(key, 0.0), r)
        assert abs(got - want) <= tol, (name, got, want, tol)
    print('sums over the data set, largest error / bound', worst)


def test_single_rows_by_value(vb, fx):
    """The value of one-row data sets at the extreme rows: the deepest tails on either side of an interior category with the
    narrowest and the widest D, and both end categories at 700 from their cut point on either side."""
    cat, o, D = fx['icat'], fx['o'], fx['D']
    tab = np.concatenate([[-np.inf], fx['alpha'], [np.inf]])
    T = fx['alpha'].size
    pick = set()
    for c in (0, 1, 5, T):
        rows = np.where(cat == c)[0]
        pick.add(int(rows[np.argmin(o[rows])]))
        pick.add(int(rows[np.argmax(o[rows])]))
    for i in sorted(pick):
        val, gs, _, thr = _run(vb, fx, np.array([i]))
        b = fx['bound'][i]
        r = float(_ratio(np.abs(np.float64(val) - fx['exact'][i, 0]), b[0] + U * fx['mag'][i, 0]))
        print('row', i, 'rho', float(o[i]), 'category', int(cat[i]), 'D', float(D[i]), 'value', val, 'error / bound', r)
        assert abs(val - fx['exact'][i, 0]) <= b[0] + U * fx['mag'][i, 0]

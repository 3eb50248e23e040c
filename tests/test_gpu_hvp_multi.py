"""The fused multi-vector pass (csrc/k_hvp_multi.hip) entry by entry, not through a solver: the full form
R = X^T diag(c) X U through `ctx.hvp_multi`, the row form T = diag(s) X Zt^T through `ctx.rows_times_matrix`, both wave
counts, every column-block count, the chunk and workgroup edges of the row axis, row windows off the chunk grid and a
coefficient block at an odd offset.

Two oracles (tests/hvp_multi_reference.py): small-integer data, where the device result must be
BITWISE the int64 product whatever the summation order, and real data against a longdouble reference under the entry-wise
bound K 2^-53 1.01 A with K counted from the algorithm.  The context has a Gaussian loss with unit precision on unbounded
box layouts at theta = 0, so the curvature is exactly the weights and the packing Jacobian the identity; tuning bit 3
keeps every product matrix-free.  A failure names the entry."""
import numpy as np
import pytest

import hvp_multi_reference as hr
from oracle import models as om
from helpers import make_par, glm_data

pytestmark = pytest.mark.gpu

NO_RESIDENT, FOUR_WAVES, TWO_GEMM = 8, 4, 1


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1, 'no HIP device visible'
    return lrvb_amd


class Problem(object):
    """The declared objective  sum_n c_n (x_n . beta)^2 / 2 + sum_v a_v eta_v^2 / 2  of one case of the reference file:
    its Hessian is X^T diag(c) X on the coefficient block plus diag(a), whatever the point."""

    def __init__(self, vb, case):
        X, off = case['X'], case['off']
        N, P = X.shape
        spec = ([('box', 'pre', off, -np.inf, np.inf)] if off else []) + [('box', 'beta', P, -np.inf, np.inf)]
        self.par, _ = make_par(vb, spec)
        self.fun = vb.DeviceObjective(self.par, x=X, y=np.zeros(N), loss='gaussian', glm_param='beta' if off else None,
                                      lik_info=1.0, quad_A=case['a'], weights=case['c'])
        self.ctx = self.fun.ctx
        assert self.ctx.D == self.ctx.V == off + P
        self.theta = np.zeros(off + P)
        self.objective = vb.Objective(self.par, self.fun)

    def hvp_multi(self, U, flags=0):
        self.ctx.set_tuning(0, NO_RESIDENT | flags)
        return self.ctx.hvp_multi(self.theta, U)

    def rows(self, Zt, rowscale, n0, n1, flags=0):
        self.ctx.set_tuning(0, NO_RESIDENT | flags)
        return self.ctx.rows_times_matrix(Zt, rowscale, n0, n1)

    def close(self):
        self.ctx.close()


def assert_exact(got, want, label):
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, label
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    i, j = bad[0]
    raise AssertionError('{}: {} of {} entries differ; first ({}, {}): got {!r}, want {!r}'.format(
        label, len(bad), got.size, i, j, got[i, j], want[i, j]))


def assert_bounded(got, ref, bound, label):
    entry, ratio = hr.worst_entry(got, ref, bound)
    print('hvp_multi ratio {} {:.4f}'.format(label, ratio))
    assert ratio <= 1.0, '{}: entry {} is {:.3g} x its bound'.format(label, entry, ratio)


def check_full(vb, N, P, Q, off=0):
    label = 'full N {} P {} Q {} off {}'.format(N, P, Q, off)
    wave_flags = (0, FOUR_WAVES) if hr.eight_waves_apply(P) else (0,)
    ci = hr.make_case('int', N, P, Q, off)
    want = hr.int_full(ci)
    pr = Problem(vb, ci)
    for f in wave_flags:
        assert_exact(pr.hvp_multi(ci['U'], f), want, '{} waves {}'.format(label, hr.n_waves(P, f != 0)))
    pr.close()
    cr = hr.make_case('real', N, P, Q, off)
    ref, A = hr.ld_full(cr), hr.abs_full(cr)
    pr = Problem(vb, cr)
    for f in wave_flags:
        got = pr.hvp_multi(cr['U'], f)
        assert_bounded(got, ref, hr.bound_R(N, P, f != 0) * A, '{} waves {}'.format(label, hr.n_waves(P, f != 0)))
        if off:                                    # no observation term in front of the coefficients: the prior term alone
            assert np.array_equal(got[:, :off], cr['a'][:off] * cr['U'][:, :off]), label
    pr.close()


# ---- the full form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,Q', hr.FULL_CASES)
def test_full_form(vb, N, P, Q):
    """Every width of the P grid (NB = 1..8, both sides of each 128-column edge) at N = 1, 9, 2049; every N of the row grid
    (one chunk, a ragged last chunk, one chunk per workgroup, workgroup 0 taking two, three and four chunks) at P = 2, 130,
    1024; every vector count at P = 130, 512.  Bitwise on integers, inside the bound on real data, with eight and with
    four waves wherever eight apply."""
    check_full(vb, N, P, Q)


@pytest.mark.parametrize('N,P,Q', hr.GLM_OFF_CASES)
def test_full_form_coefficients_at_an_odd_offset(vb, N, P, Q):
    """A 3-entry box block in front of the coefficients: the rows of U and of the result start at an odd offset inside
    vectors of V = D = P + 3; the pre-block entries of the result are exactly the prior term."""
    check_full(vb, N, P, Q, off=hr.GLM_OFF)
    ci = hr.make_case('int', N, P, Q, hr.GLM_OFF)
    pr = Problem(vb, ci)
    got = pr.hvp_multi(ci['U'])
    assert np.array_equal(got[:, :hr.GLM_OFF], ci['a'][:hr.GLM_OFF] * ci['U'][:, :hr.GLM_OFF])
    pr.close()


def test_zero_weights_delete_rows(vb):
    """Zero weights on every second row: bitwise the result of the matrix without those rows (integer data, so both are
    also the oracle)."""
    N, P, Q = 2049, 130, 7
    ci = hr.make_case('int', N, P, Q)
    keep = np.arange(N) % 2 == 0
    cz = dict(ci, c=np.where(keep, ci['c'], 0.0))
    cd = dict(ci, X=np.ascontiguousarray(ci['X'][keep]), c=ci['c'][keep])
    pz, pd = Problem(vb, cz), Problem(vb, cd)
    gz, gd = pz.hvp_multi(ci['U']), pd.hvp_multi(ci['U'])
    assert_exact(gz, gd, 'zero weights against deleted rows')
    assert_exact(gz, hr.int_full(cd), 'zero weights against the oracle')
    pz.close(); pd.close()


@pytest.mark.parametrize('N,P,Q,off', [(2049, 130, 17, 0), (17, 2, 16, 0), (2049, 512, 33, 0), (2049, 130, 7, hr.GLM_OFF)])
def test_routes_agree_on_integers(vb, N, P, Q, off):
    """The two-GEMM route (tuning bit 0) and `Objective.fun_free_hvp` row by row (the one-vector pass) must be bitwise
    `ctx.hvp_multi` on integer data."""
    ci = hr.make_case('int', N, P, Q, off)
    pr = Problem(vb, ci)
    fused = pr.hvp_multi(ci['U'])
    assert_exact(fused, hr.int_full(ci), 'fused')
    assert_exact(pr.hvp_multi(ci['U'], TWO_GEMM), fused, 'two-GEMM route')
    pr.ctx.set_tuning(0, NO_RESIDENT)
    single = np.stack([pr.objective.fun_free_hvp(pr.theta, ci['U'][q]) for q in range(Q)])
    assert_exact(single, fused, 'fun_free_hvp row by row')
    pr.close()


# ---- the row form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', hr.ROWS_P)
def test_row_form(vb, P):
    """T = diag(s) X Zt^T on N = 4099 rows for Q = 1, 5, 16, 21 and windows that start and end on and off the 8-row chunk
    grid, down to one row; the scale is non-zero on every row, so the rows just past a window's end carry one.  With the
    scale and with rowscale = None; with four waves too wherever eight apply."""
    N = hr.ROWS_N
    wave_flags = (0, FOUR_WAVES) if hr.eight_waves_apply(P) else (0,)
    for kind in ('int', 'real'):
        pr = None
        for Q in hr.ROWS_Q:
            X, s, Zt = hr.rows_case(kind, P, Q)
            if pr is None:                                      # one matrix and scale per kind: only Zt changes with Q
                pr = Problem(vb, dict(X=X, c=s, a=np.ones(P), off=0))
            if kind == 'int':
                unit = hr.int_rows(X, np.ones(N), Zt)
                refs = {True: hr.to_int(s)[:, None] * unit, False: unit}
            else:
                unit, A1 = hr.ld_rows(X, np.ones(N), Zt), hr.abs_rows(X, np.ones(N), Zt)
                refs = {True: hr.to_ld(s)[:, None] * unit, False: unit}
                As = {True: np.abs(hr.to_ld(s))[:, None] * A1, False: A1}
            worst = 0.0
            for f in wave_flags:
                for (n0, n1) in hr.ROWS_WINDOWS:
                    for scaled in (True, False):
                        got = pr.rows(Zt, s if scaled else None, n0, n1, f)
                        label = 'rows P {} Q {} window ({}, {}) scaled {} waves {}'.format(P, Q, n0, n1, scaled, hr.n_waves(P, f != 0))
                        assert got.shape == (n1 - n0, Q), label
                        if kind == 'int':
                            assert_exact(got, refs[scaled][n0:n1], label)
                        else:
                            entry, ratio = hr.worst_entry(got, refs[scaled][n0:n1], hr.bound_T(P, f != 0) * As[scaled][n0:n1])
                            worst = max(worst, ratio)
                            assert ratio <= 1.0, '{}: entry {} is {:.3g} x its bound'.format(label, entry, ratio)
            if kind == 'real':
                print('hvp_multi ratio rows P {} Q {} {:.4f}'.format(P, Q, worst))
        pr.close()


@pytest.mark.parametrize('P', hr.ROWS_P)
def test_obs_loss_is_half_the_squared_row_product(vb, P):
    """`obs_loss` runs the row form with one vector and unit scale: on integer data with y = 0 it is bitwise T^2 / 2."""
    N = hr.ROWS_N
    X, s, Zt = hr.rows_case('int', P, 1)
    pr = Problem(vb, dict(X=X, c=s, a=np.ones(P), off=0))
    T = hr.int_rows(X, np.ones(N), Zt)[:, 0].astype(np.float64)
    pr.ctx.set_tuning(0, NO_RESIDENT)
    for (n0, n1) in hr.ROWS_WINDOWS:
        got = pr.ctx.obs_loss(Zt[0], n0, n1)
        assert np.array_equal(got, 0.5 * T[n0:n1] ** 2), 'window ({}, {})'.format(n0, n1)
    pr.close()


# ---- the device-side skip of a finished 16-block --------------------------------------------------------------------------
def test_dead_block_is_skipped_on_the_device(vb):
    """Q = 20 right-hand sides whose rows 16..19 are zero: the second 16-block is dead from the first iteration, its
    products are skipped on the device.  Rows 0..15 must be bitwise the Q = 16 solve, rows 16..19 exactly zero."""
    rng = np.random.default_rng(20)
    N, P = 1003, 256
    par, _ = make_par(vb, [('box', 'beta', P, -np.inf, np.inf)])
    x, y, w = glm_data(rng, N, P, om.GAUSSIAN)
    fun = vb.DeviceObjective(par, x=x, y=y, loss='gaussian', quad_A=np.ones(P), weights=w)
    fun.ctx.set_tuning(0, NO_RESIDENT)
    theta = np.zeros(P)
    B = np.zeros((20, P))
    B[:16] = rng.normal(size=(16, P))
    X16, info16, it16 = fun.ctx.cg_solve_multi(theta, B[:16])
    X20, info20, it20 = fun.ctx.cg_solve_multi(theta, B)
    assert np.all(info16 == 0) and np.all(info20 == 0) and np.all(it16 > 0)
    assert np.array_equal(X20[:16], X16) and np.array_equal(it20[:16], it16)
    assert np.all(X20[16:] == 0.0) and np.all(it20[16:] == 0)
    fun.ctx.close()

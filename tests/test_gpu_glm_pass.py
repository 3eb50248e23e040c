"""The fused observation pass (csrc/k_glm.hip) entry by entry on its three routes -- the narrow kernel, the one-pass wide
kernel and the two-pass route -- and through the two-level reducer: the value, the gradient, rows of `obs_grad` (X carries a
column of ones, so l'_n itself appears), the Hessian-vector product from the cached curvature, and a second gradient pass
that must repeat the first bit for bit.

Two oracles (tests/glm_pass_reference.py): small-integer data in four settings whose loss terms are
exact, where the device result must be BITWISE the int64 one whatever the summation order, and real data (columns of X over
six decades, weights over four, |z| <= 30) against a longdouble reference under an entry-wise bound of counted roundings.
The layout is an unbounded box evaluated in vector coordinates (J = I exactly); tuning bit 3 keeps every product
matrix-free, bit 0 takes the two-pass route above 1024 columns.  One context per case.  A failure names the entry."""
import numpy as np
import pytest

import glm_pass_reference as gr
from helpers import make_par, on_torch_stream

pytestmark = pytest.mark.gpu

NO_RESIDENT, TWO_PASS = 8, 1


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1, 'no HIP device visible'
    return lrvb_amd


class Problem(object):
    """The declared objective  sum_n w_n l(y_n, x_n . beta) + (eta - m)^T diag(a) (eta - m) / 2  of one case of the reference
    file, on an unbounded box layout."""

    def __init__(self, vb, case, two_pass=False):
        self.case = case
        X, off = case['X'], case['off']
        N, P = X.shape
        spec = ([('box', 'pre', off, -np.inf, np.inf)] if off else []) + [('box', 'beta', P, -np.inf, np.inf)]
        self.par, _ = make_par(vb, spec)
        self.fun = vb.DeviceObjective(self.par, x=X, y=case['y'], loss=case['loss'], glm_param='beta' if off else None,
                                      lik_info=1.0, quad_A=case['a'], quad_m=case['m'], weights=case['w'])
        self.ctx = self.fun.ctx
        assert self.ctx.D == self.ctx.V == off + P
        self.flags = NO_RESIDENT | (TWO_PASS if two_pass else 0)
        self.plan = gr.plan(N, P, two_pass)
        self.windows = gr.obs_windows(self.plan, off + P)

    def run(self):
        """dict(value, grad, hvp (2 x V), again (the gradient of a second pass), rows {(n0, n1): window of obs_grad})."""
        ctx, eta = self.ctx, self.case['beta']
        ctx.set_tuning(0, self.flags)                       # (a setter forgets the point: the next call runs the pass)
        out = dict(value=ctx.value(eta, False), grad=ctx.grad(eta, False))
        out['hvp'] = np.stack([ctx.hvp(eta, u, False) for u in self.case['U']])      # the curvature the gradient pass cached
        ctx.set_tuning(0, self.flags)
        out['again'] = ctx.grad(eta, False)
        out['rows'] = {(n0, n1): ctx.obs_grad(eta, n0, n1, False) for (n0, n1) in self.windows}
        return out

    def close(self):
        self.ctx.close()


def assert_exact(got, want, label):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, label
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    i = tuple(int(k) for k in bad[0])
    raise AssertionError('{}: {} of {} entries differ; first {}: got {!r}, want {!r}'.format(
        label, len(bad), got.size, i, got[i], want[i]))


def assert_same_runs(a, b, label):
    for k in ('value', 'grad', 'hvp', 'again'):
        assert_exact(a[k], b[k], '{}: {}'.format(label, k))
    for win in a['rows']:
        assert_exact(a['rows'][win], b['rows'][win], '{}: obs_grad rows {}'.format(label, win))


def check_exact(pr, out, label):
    """`out` of Problem.run against the int64 oracle of the problem's (integer) case."""
    case = pr.case
    ie = gr.int_evaluate(case)
    if ie['value'] is not None:
        assert_exact(out['value'], ie['value'], label + ': value')
    else:                                                   # logistic at beta = 0: w log 2 rounds, the value keeps the bound
        r = case['beta'] - case['m']
        ref = np.sum(case['w'].astype(gr.LD)) * np.log1p(gr.LD(1)) + gr.LD(np.sum(case['a'] * r * r)) / 2
        _, ratio = gr.worst_entry(out['value'], ref, gr.bounds(case, pr.plan)['value'])
        assert ratio <= 1.0, '{}: value is {:.3g} x its bound'.format(label, ratio)
    assert_exact(out['grad'], ie['grad'], label + ': gradient')
    assert_exact(out['again'], out['grad'], label + ': second gradient pass')
    assert_exact(out['hvp'], ie['hvp'], label + ': HVP')
    for (n0, n1), rows in out['rows'].items():
        assert_exact(rows, gr.obs_rows(case, ie['lp'], n0, n1, np.float64), '{}: obs_grad rows ({}, {})'.format(label, n0, n1))
    off = case['off']
    if off:                                                 # no observation term in front of the coefficients
        assert_exact(out['grad'][:off], case['a'][:off] * (case['beta'][:off] - case['m'][:off]), label + ': pre-block gradient')
        assert_exact(out['hvp'][:, :off], case['a'][:off] * case['U'][:, :off], label + ': pre-block HVP')


def run_exact(vb, setting, N, P, two_pass=False, off=0):
    label = '{} N {} P {}{}{}'.format(setting, N, P, ' two-pass' if two_pass else '', ' off {}'.format(off) if off else '')
    pr = Problem(vb, gr.make_case(setting, 'int', N, P, off), two_pass)
    out = pr.run()
    pr.close()
    check_exact(pr, out, label)
    return out


def run_bounded(vb, loss, N, P, two_pass=False, off=0):
    label = '{} N {} P {}{}'.format(loss, N, P, ' off {}'.format(off) if off else '')
    case = gr.make_case(loss, 'real', N, P, off)
    pr = Problem(vb, case, two_pass)
    out = pr.run()
    pr.close()
    ref, b = gr.evaluate(case, gr.LD), gr.bounds(case, pr.plan)
    worst = []
    for k in ('value', 'grad', 'hvp'):
        entry, ratio = gr.worst_entry(out[k], ref[k], b[k])
        worst.append((ratio, k, entry))
    for (n0, n1), rows in out['rows'].items():
        entry, ratio = gr.worst_entry(rows, gr.obs_rows(case, ref['lp'], n0, n1, gr.LD), gr.obs_rows_bound(b, n0, n1))
        worst.append((ratio, 'obs_grad rows ({}, {})'.format(n0, n1), entry))
    ratio, what, entry = max(worst)
    print('glm_pass ratio {} {} {:.4f} ({})'.format(pr.plan['route'], label, ratio, what))
    for k in ('value', 'grad', 'hvp'):
        print('glm_pass detail {} {} {} {:.4f}'.format(pr.plan['route'], label, k, [w for w in worst if w[1] == k][0][0]))
    assert ratio <= 1.0, '{}: {} entry {} is {:.3g} x its bound'.format(label, what, entry, ratio)
    assert_exact(out['again'], out['grad'], label + ': second gradient pass')
    if off:
        assert_exact(out['grad'][:off], case['a'][:off] * case['beta'][:off], label + ': pre-block gradient')
        assert_exact(out['hvp'][:, :off], case['a'][:off] * case['U'][:, :off], label + ': pre-block HVP')


# ---- the narrow kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', gr.NARROW_P)
def test_narrow_column_grid(vb, P):
    """Every NIT on both sides of each 128-column edge, odd widths (the scalar-load branch) and NIT = 8 off the 128 grid
    (770, 1022, 1023), at one workgroup, two, and 257 (the two-level reducer).  All four exact settings."""
    for N in gr.NARROW_P_GRID_N:
        for setting in gr.INT_SETTINGS:
            run_exact(vb, setting, N, P)


@pytest.mark.parametrize('N,P,two_pass,off', gr.real_shapes())
def test_real_data_inside_the_bound(vb, N, P, two_pass, off):
    """All three losses on real data at N = 9 and 2049 over the column grids of the three routes, N = 16391 at P = 130 (a
    second stage) and behind the 3-entry block: every entry of the value, the gradient, the rows and the HVP inside its
    bound of counted roundings."""
    for loss in gr.LOSSES:
        run_bounded(vb, loss, N, P, two_pass, off)


@pytest.mark.parametrize('P', gr.NARROW_N_GRID_P)
@pytest.mark.parametrize('N', gr.NARROW_N)
def test_narrow_row_grid(vb, N, P):
    """nblk = 1, 2, 9, 33, 255, 256 (two-level from here), 257, 545, 2048; one full round of the capped grid; a second stage
    with one live row and with two, with one workgroup and with several; the third stage (back to the first register set)
    and the fourth.  Above 16384 rows the Gaussian setting alone."""
    for setting in gr.int_settings_at(N, P):
        run_exact(vb, setting, N, P)


@pytest.mark.parametrize('N', gr.NARROW_N_AT_1024)
def test_narrow_second_and_third_stage_at_full_width(vb, N):
    run_exact(vb, 'gaussian', N, 1024)


# ---- the one-pass wide kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', gr.WIDE1_P)
@pytest.mark.parametrize('N', gr.WIDE1_N)
def test_wide1_column_grid(vb, N, P):
    """All four instantiations, both sides of their edges and odd widths, at one live row, one stage, two stages' worth and
    N = 1001; at N = 1001 the two-pass route (tuning bit 0) must be bitwise the one-pass result on integers."""
    for setting in gr.INT_SETTINGS:
        one = run_exact(vb, setting, N, P)
        if N == gr.WIDE1_TWO_PASS_N:
            assert_same_runs(run_exact(vb, setting, N, P, two_pass=True), one, '{} P {}: two-pass against one-pass'.format(setting, P))


@pytest.mark.parametrize('P,k', [(P, k) for P in gr.WIDE1_MULTI_P for k in (0, 1)])
def test_wide1_many_stages(vb, P, k):
    """More rows than four rounds of the largest grid the hardware could hold, plus 1 and plus 2: whatever the occupancy,
    every workgroup runs at least three stages (both parities of the LDS slots, both register sets), the last round has dead
    slots, and its tail is one live row or two."""
    run_exact(vb, 'gaussian', gr.wide1_multi_N(P)[k], P)


# ---- the two-pass route -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', gr.WIDE2_P)
@pytest.mark.parametrize('N', gr.WIDE2_N)
def test_two_pass_column_grid(vb, N, P):
    """Above 4096 columns: an odd width, a 2-column tail tile, a whole number of tiles and one column more; one row, one
    workgroup of rows, the 2048-row block edge of the accumulation pass and a third block (Gaussian setting alone there)."""
    for setting in gr.int_settings_at(N, P):
        run_exact(vb, setting, N, P)


@pytest.mark.parametrize('N,P', gr.WIDE2_FORCED)
def test_two_pass_forced(vb, N, P):
    """Tuning bit 0 at P = 1026: a wave of the row kernel takes a second row above 16384 rows; three row blocks at 4097."""
    for setting in gr.int_settings_at(N, P):
        run_exact(vb, setting, N, P, two_pass=True)


# ---- an adopted X that is 8-byte but not 16-byte aligned ----------------------------------------------------------------
@pytest.mark.parametrize('P', gr.ADOPTED_P)
@pytest.mark.parametrize('N', gr.ADOPTED_N)
def test_adopted_unaligned_x(vb, N, P):
    """Even P with X adopted one double past a 16-byte boundary: the pair loads are not allowed, every route falls back to
    scalar loads (wide2 never used pairs).  Bitwise the owned, aligned copy, and the oracle."""
    import torch
    for setting in gr.INT_SETTINGS:
        label = 'adopted {} N {} P {}'.format(setting, N, P)
        case = gr.make_case(setting, 'int', N, P)
        pr = Problem(vb, case)
        on_torch_stream(pr.ctx)
        owned = pr.run()
        store = torch.empty(N * P + 1, dtype=torch.float64, device='cuda:0')
        store[1:].copy_(torch.as_tensor(case['X']).reshape(-1))
        assert store[1:].data_ptr() % 16 == 8
        pr.ctx.set_data_dev(vb._hip.SLOT_X, store[1:].data_ptr(), N, P)
        adopted = pr.run()
        pr.close()
        check_exact(pr, owned, label + ' (owned)')
        assert_same_runs(adopted, owned, label)


# ---- coefficients behind a 3-entry block ------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', gr.PRE_BLOCK_P)
def test_coefficients_at_an_odd_offset(vb, P):
    """`glm_param` behind a 3-entry box block: beta, u and the outputs start at an odd offset inside vectors of V = P + 3;
    the pre-block entries of the gradient and the HVP are exactly the prior term."""
    for setting in gr.INT_SETTINGS:
        run_exact(vb, setting, gr.PRE_BLOCK_N, P, off=gr.GLM_OFF)


def test_zero_weights_delete_rows(vb):
    """Zero weights on every second row: bitwise the design without those rows (integer data, so both are also the oracle)."""
    N, P = gr.ZERO_WEIGHTS
    keep = np.arange(N) % 2 == 0
    for setting in gr.INT_SETTINGS:
        c = gr.make_case(setting, 'int', N, P)
        cz = dict(c, w=np.where(keep, c['w'], 0.0))
        cd = dict(c, X=np.ascontiguousarray(c['X'][keep]), y=c['y'][keep], w=c['w'][keep])
        pz, pd = Problem(vb, cz), Problem(vb, cd)
        oz, od = pz.run(), pd.run()
        pz.close(); pd.close()
        check_exact(pd, od, setting + ': deleted rows')
        for k in ('grad', 'hvp', 'again') + (() if setting == 'logistic0' else ('value',)):        # (w log 2 rounds by the order)
            assert_exact(oz[k], od[k], '{}: zero weights against deleted rows: {}'.format(setting, k))

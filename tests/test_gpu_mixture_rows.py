"""The mixture row kernels (csrc/k_mixture_rows.h) row by row against tests/mixture_rows_reference.py:
the grid-stride loop of both kernels past its first trip, single rows at chosen positions observed entry by entry through
probes, launches in which the two routes mix, the failure flag of both routes, the zero-weight contract and run-to-run
reproducibility.  Public path only: MixtureObjective / ctx.mixture_rows / ctx.mixture_stats / ctx.set_tuning.  Every bound is
the reference's (counted from the kernel text, or 8 unit_n calibrated on the CPU); each figure is printed before it is
asserted."""
import numpy as np
import pytest

import mixture_rows_reference as mr
from test_mixture_host_math import make_par

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def objective(vb, pr, w=None):
    fun = vb.MixtureObjective(make_par(pr['N'], pr['V'], pr['K']), pr['x'], weights=pr['w'] if w is None else w)
    fun._push_state()
    return fun


def rows(fun, pr, fz=None, **kw):
    return fun.ctx.mixture_rows(pr['K'], (pr['fz'] if fz is None else fz).ravel(), pr['lam'], **kw)


def check(tag, ev, got, schur=True):
    val2, gz, S64, R = got
    figs = {'val2': float(np.max(np.abs(val2 - ev['val2']) / ev['val2_bound'])),
            'gz': mr.max_ratio(gz, ev['gz'], ev['gz_bound']), 'S64': mr.max_ratio(S64, ev['S64'], ev['S64_bound'])}
    if schur:
        figs['R'] = mr.max_ratio(R, ev['R'], ev['R_bound'])
    print('[{}] error / bound: {}'.format(tag, ' '.join('{} {:.3f}'.format(*kv) for kv in figs.items())))
    assert np.all(np.abs(val2 - ev['val2']) <= ev['val2_bound']), (val2, ev['val2'], ev['val2_bound'])
    assert np.all(np.abs(gz - ev['gz']) <= ev['gz_bound']), mr.worst(gz, ev['gz'], ev['gz_bound'])
    assert np.all(np.abs(S64 - ev['S64']) <= ev['S64_bound']), mr.worst(S64, ev['S64'], ev['S64_bound'])
    if schur:
        assert np.all(np.abs(R - ev['R']) <= ev['R_bound']), mr.worst(R, ev['R'], ev['R_bound'])


def reference(pr, **kw):
    return mr.evaluate(pr['fz'], pr['x'], pr['w'], pr['lam'], **kw)


# ---- grid stride -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,V,K', mr.GRID_CASES)
def test_grid_stride_every_row(vb, N, V, K):
    """Two and three trips of the pair loop (buffers 0, 1, 0; the last pair half valid): gz of every row entry by entry, val2, S64
    and R by their entry-wise bounds.  (32771, 31, 32) takes the kron32 GEMM."""
    pr = mr.grid_case(N, V, K)
    assert mr.trips(N)[0] == (3 if N == 65539 else 2)
    check('grid {} {} {}'.format(N, V, K), reference(pr), rows(objective(vb, pr), pr))


@pytest.mark.parametrize('N,V,K', mr.STORE_CASES)
def test_sixteen_byte_stores_keep_their_data(vb, N, V, K):
    """The packed row of A_n leaves in 16-byte stores whose data registers must outlive the store by two wait states.  With one,
    the low dword of lanes 12 .. 15 of each 16 of a row's last store segment was overwritten now and then once two workgroups
    shared a CU (N > 2048): relative errors of 1e-7 in single entries of single rows, 2e-9 of the summed operand norm-wise.  The
    lanes are unmasked at every K here; with the one-state macro K = 17, 25, 31 failed by 1e4 .. 1e6 bounds in every run, K = 7 and
    13 (one store segment per row) did not show it."""
    pr = mr.grid_case(N, V, K)
    check('stores {} {} {}'.format(N, V, K), reference(pr), rows(objective(vb, pr), pr))


def test_dense_kernel_stride(vb):
    """Every row through the dense kernel (set_tuning(0, 2)): 32771 rows on 4 * 2048 waves, five trips of its loop."""
    N, V, K = mr.DENSE_STRIDE_CASE
    pr = mr.routed_case(N, V, K)
    assert N > 4 * mr.DENSE_MAX_GRID
    fun = objective(vb, pr)
    try:
        fun.ctx.set_tuning(0, 2)
        got = rows(fun, pr)
    finally:
        fun.ctx.set_tuning(0, 0)
    check('dense stride', reference(pr), got)


# ---- probes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,V,K,which', mr.PROBE_CASES)
def test_probe_rows_entry_by_entry(vb, N, V, K, which):
    """x = c_i e_{j_i} at the probe rows and 0 elsewhere: R[(j_i, j_i), :] = w^2 c_i^2 vec(A_n) and S64[j_i, 32 + k] = w c_i z_nk are
    single terms, compared with the mpmath row.  Positions: mr.grid_probe_positions; kinds: mr.probe_plan."""
    pr = mr.probe_case(N, V, K, which)
    truth = {q['n']: mr.mp_row_of(pr, q['n']) for q in pr['probes']}
    units = {q['n']: mr.probe_unit(pr, q['n']) for q in pr['probes']}
    ev = reference(pr, truth={n: t[2] for n, t in truth.items()}, units=units)
    val2, gz, S64, R = got = rows(objective(vb, pr), pr)
    R4 = R.reshape(V + 1, V + 1, K, K)
    fails = []
    for q in pr['probes']:
        n, j, c, w = q['n'], 1 + q['j'], q['c'], pr['w'][q['n']]
        z, g_row, A = truth[n]
        e = mr.a_error(R4[j, j] / (w * w * c * c), A)
        zb = mr.U * mr.SLACK * (ev['rel_p'][n] + 3) * (w * c * z)              # the device's p, fl(w u) and the product
        ez = float(np.max(np.abs(S64[j, 32:32 + K] - w * c * z) / zb))
        eg = float(np.max(np.abs(gz[n] - g_row) / ev['gz_bound'][n]))
        print('[probe row {} {} m {} {}] e / (8 unit) {:.3f} (unit {:.1f} U)  z {:.3f}  gz {:.3f}'.format(
            n, q['kind'], q['m'], 'dense' if ev['dense'][n] else 'fast', e / (mr.A_FACTOR * units[n]), units[n] / mr.U, ez, eg))
        if not (e <= mr.A_FACTOR * units[n] and ez <= 1.0 and eg <= 1.0):
            fails.append((n, q['kind'], e / (mr.A_FACTOR * units[n]), ez, eg))
        assert np.array_equal(S64[j, 32 + K:], np.zeros(32 - K))
    assert not fails, fails
    check('probe {} {} {} {}'.format(N, V, K, which), ev, got)


# ---- mixed routing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,V,K', mr.ROUTED_CASES + [mr.ROUTED_BIG])
def test_mixed_routing(vb, N, V, K):
    """Pairs (fast, dense), (dense, fast), (dense, dense), (fast, fast) and a dense odd last row in one launch: the dense pass fills
    the holes the masked stores left.  Default tuning, then every row forced dense, inside the same bounds."""
    pr = mr.routed_case(N, V, K)
    ev = reference(pr)
    assert ev['dense'].any() and not ev['dense'].all()
    fun = objective(vb, pr)
    check('mixed {} {} {}'.format(N, V, K), ev, rows(fun, pr))
    try:
        fun.ctx.set_tuning(0, 2)
        got = rows(fun, pr)
    finally:
        fun.ctx.set_tuning(0, 0)
    check('mixed {} {} {} forced dense'.format(N, V, K), ev, got)


# ---- failure reporting -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['dense', 'fast', 'last'])
def test_one_indefinite_row_is_reported(vb, kind):
    """Exactly one indefinite row among 32771 (the builder asserts it): a dense-route row of the second trip, a fast-route row
    with det T >= 0, the odd last row.  The Schur operand must be refused; values, gradient and statistics do not need it."""
    pr = mr.with_indefinite_row(mr.routed_case(*mr.ROUTED_BIG), kind)
    fun = objective(vb, pr)
    with pytest.raises(np.linalg.LinAlgError):
        rows(fun, pr, want_schur=True)
    with pytest.raises(np.linalg.LinAlgError):
        fun.ctx.mixture_stats(pr['K'], pr['fz'].ravel(), pr['lam'], want_schur=True)
    check('indefinite ' + kind, reference(pr, want_A=False), rows(fun, pr, want_schur=False), schur=False)
    val2, S64 = fun.ctx.mixture_stats(pr['K'], pr['fz'].ravel(), pr['lam'], want_schur=False)
    ev = reference(pr, want_A=False)
    assert np.all(np.abs(val2 - ev['val2']) <= ev['val2_bound']) and np.all(np.abs(S64 - ev['S64']) <= ev['S64_bound'])


# ---- zero weight -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ['inner', 'last'])
def test_zero_weight_row(vb, where):
    """w_n = 0: the row counts for nothing in val2, S64 and gz (its gz entries are exactly 0.0), and its local block is the zero
    matrix, so the Schur operand is refused (MixtureObjective docstring)."""
    pr = mr.routed_case(131, 17, 17)
    N = pr['N']
    n = N - 1 if where == 'last' else 40
    w = pr['w'].copy()
    w[n] = 0.0
    fun = objective(vb, pr, w=w)
    val2, gz, S64, _ = got = rows(fun, pr, want_schur=False)
    keep = np.arange(N) != n
    ev = mr.evaluate(pr['fz'][keep], pr['x'][keep], pr['w'][keep], pr['lam'], want_A=False)
    assert np.array_equal(gz[n], np.zeros(pr['K'] - 1))
    check('zero weight ' + where, ev, (val2, gz[keep], S64, None), schur=False)
    with pytest.raises(np.linalg.LinAlgError):
        rows(fun, pr, want_schur=True)
    with pytest.raises(np.linalg.LinAlgError):
        fun.ctx.mixture_stats(pr['K'], pr['fz'].ravel(), pr['lam'], want_schur=True)


# ---- reproducibility ---------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(vb):
    """`todo` is filled by atomicAdd in arbitrary order; every dense row writes its own row of the operand, so the order must not
    show: val2, gz, S64 and R of two calls on the mixed N = 32771 problem, bit for bit."""
    pr = mr.routed_case(*mr.ROUTED_BIG)
    fun = objective(vb, pr)
    a, b = rows(fun, pr), rows(fun, pr)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    c = rows(objective(vb, pr), pr)                                  # and from a fresh context
    for u, v in zip(a, c):
        assert np.array_equal(u, v)

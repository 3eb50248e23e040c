"""The dense linear algebra of csrc/k_linalg.hip against extended-precision references (tests/dense_reference.py):
blocked Cholesky at every block edge, conditioning up to 1e12, exact power-of-two scalings, the position of a failing
pivot in every residue of the four-column step and in all three kinds of diagonal block, non-finite input, the triangle
that is read, both routes of the triangular solves with a short tail block, the state of the context across failed and
smaller factorisations, the device-resident entry points, and every gemv route behind CG on a resident matrix.

Every bound is derived, none is tuned to the device; tests/test_dense_reference_host_math.py shows
LAPACK and a NumPy emulation of the device algorithm inside each of them on the same inputs.  Each test prints its worst
ratio to the bound (`DENSE|...`) before it asserts."""
import re

import numpy as np
import pytest

import dense_reference as dr

pytestmark = pytest.mark.gpu

EPS = dr.EPS
SENTINEL = -7.25e33


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _carrier(vb):
    """Any context carries the solver: chol_factor / cg_solve_matrix take matrices of any size."""
    blocks = [dict(kind=0, free_size=4, vec_size=4, dim0=4, dim1=0, lb=-np.inf, ub=np.inf)]
    return vb.DeviceContext(blocks, quad_kind=1)


@pytest.fixture(scope='module')
def ctx(vb):
    c = _carrier(vb)
    yield c
    c.close()


def reported_minor(err):
    m = re.search(r'(\d+)-th leading minor', str(err.value))
    assert m is not None, str(err.value)
    return int(m.group(1))


def _report(name, **ratios):
    print('DENSE|{}|{}'.format(name, ' '.join('{}={:.3g}'.format(k, v) for k, v in ratios.items())), flush=True)


def _solve_ratios(S, X, B, Xref, kappa):
    n = S.shape[0]
    fb, bb = dr.bounds(n, kappa)
    return dr.forward_error(X, Xref) / fb, dr.backward_error(S, X, B) / bb


# ---- 1. block edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', dr.SWEEP_N)
def test_block_edge_sweep(ctx, n):
    S, kappa, B, Xref, M, XrefM = dr.sweep_case(n)
    ctx.chol_factor(S)
    worst_f = worst_b = worst_c = 0.0
    failures = []
    rhs = [(nr, np.ascontiguousarray(B[:, :nr]), Xref[:, :nr]) for nr in dr.SWEEP_NRHS]
    rhs.append(('1-D', np.ascontiguousarray(B[:, 1]), Xref[:, 1]))
    for tag, b, xr in rhs:
        X = ctx.chol_solve(b)
        assert X.shape == b.shape
        f, bk = _solve_ratios(S, X, b, xr, kappa)
        worst_f, worst_b = max(worst_f, f), max(worst_b, bk)
        if not (f <= 1.0 and bk <= 1.0):
            failures.append(('solve', tag, f, bk))
    for Q in dr.SWEEP_Q:
        m = np.ascontiguousarray(M[:Q])
        cov = ctx.lrvb_cov(m)
        err, scale = dr.cov_error(cov, m, XrefM[:, :Q])
        c = err / (EPS * kappa * scale)
        worst_c = max(worst_c, c)
        if not c <= 1.0:
            failures.append(('cov', Q, c))
    _report('sweep n={}'.format(n), forward=worst_f, backward=worst_b, cov=worst_c)
    assert not failures, failures


# ---- 2. conditioning and exact scalings -------------------------------------------------------------------------
@pytest.mark.parametrize('kappa', dr.COND_KAPPA)
@pytest.mark.parametrize('n', dr.COND_N)
def test_conditioning_sweep(ctx, n, kappa):
    """Forward eps kappa; backward n eps up to kappa = 1e6 and n eps sqrt(kappa) above (a solve through explicit inverses of
    triangular blocks is conditionally backward stable: its residual may carry kappa(L_jj) <= sqrt(kappa_2(S))).  The ratio to
    plain n eps is printed as well.  D S D with D = diag(2^k) is exact and Cholesky is invariant to it: the unscaled
    solution of the scaled system meets the forward bound with kappa of the UNSCALED matrix."""
    S, B, Xref, d = dr.cond_case(n, kappa)
    ctx.chol_factor(S)
    X = ctx.chol_solve(B)
    f, bk = _solve_ratios(S, X, B, Xref, kappa)
    ctx.chol_factor(S * d[:, None] * d[None, :])
    Xs = d[:, None] * ctx.chol_solve(d[:, None] * B)
    fs = dr.forward_error(Xs, Xref) / (EPS * kappa)
    _report('cond n={} kappa={:.0e}'.format(n, kappa), forward=f, backward=bk,
            backward_over_plain_n_eps=bk * dr.bounds(n, kappa)[1] / (n * EPS), forward_scaled=fs,
            scaled_bitwise=float(np.array_equal(Xs, X)))
    assert f <= 1.0 and bk <= 1.0 and fs <= 1.0, (f, bk, fs)


# ---- 3. symmetry of lrvb_cov ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n,Q', dr.SYM_CASES)
def test_lrvb_cov_symmetric_bitwise(ctx, n, Q):
    """Y^T Y accumulates entry (i, j) and entry (j, i) over the same k in the same order, and a product commutes."""
    S, M = dr.sym_case(n, Q)
    ctx.chol_factor(S)
    cov = ctx.lrvb_cov(M)
    asym = np.max(np.abs(cov - cov.T) / np.maximum(np.abs(cov), 1e-300))
    _report('symmetry n={} Q={}'.format(n, Q), max_rel_asymmetry=asym)
    assert np.array_equal(cov, cov.T)


# ---- 4. position of the failing pivot ----------------------------------------------------------------------------
@pytest.mark.parametrize('k', dr.PIVOT_POSITIONS)
def test_pivot_position(ctx, k):
    """n = 130: blocks of 64 (first-block kernel), 64 (head of the trailing update) and 2 (short tail block); every residue
    mod 4 of the four-column step in each."""
    S = dr.broken_pivot(k)
    assert dr.first_bad_pivot(S) == k + 1
    with pytest.raises(np.linalg.LinAlgError) as err:
        ctx.chol_factor(S)
    assert reported_minor(err) == k + 1


@pytest.mark.parametrize('tag,S', dr.nonfinite_cases(), ids=[t for t, _ in dr.nonfinite_cases()])
def test_nonfinite_input_is_refused_at_its_pivot(ctx, tag, S):
    want = dr.first_bad_pivot(S)
    stated = dr.expected_nonfinite_index(tag)
    assert want >= 1 and (stated is None or stated == want)
    with pytest.raises(np.linalg.LinAlgError) as err:
        ctx.chol_factor(S)
    assert reported_minor(err) == want


# ---- 5. the lower triangle alone is read ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', dr.LOWER_N)
def test_lower_triangle_only(ctx, n):
    S, B = dr.lower_case(n)
    ctx.chol_factor(S)
    X = ctx.chol_solve(B)
    Sn = S.copy()
    Sn[np.triu_indices(n, 1)] = np.nan
    ctx.chol_factor(Sn)
    Xn = ctx.chol_solve(B)
    assert np.all(np.isfinite(X))
    assert np.array_equal(X, Xn)


# ---- 6. both routes of the triangular solves, short tail block ------------------------------------------------------
@pytest.mark.parametrize('n', dr.ROUTE_N)
def test_solve_routes(ctx, n):
    """257 column tiles x 2 row blocks = 514 > 512: the first forward and the first backward step take the generic GEMM +
    head-only route, the rest the fused one; at n = 129 the backward generic product contracts over ONE row.  16384 columns
    (256 tiles) stay fused throughout.  The bound holds for every column on its own."""
    S, B, Xref = dr.route_case(n)
    fb = EPS * dr.ROUTE_KAPPA
    # a larger system first: the factor and right-hand-side buffers keep its entries past the smaller system's rows, so a
    # product that contracts past the short tail block picks up non-zero stale data instead of whatever a fresh allocation holds
    ctx.chol_factor(dr.state_case(193)[0])
    ctx.chol_solve(np.ones((193, dr.ROUTE_NRHS)))
    ctx.chol_factor(S)
    X = ctx.chol_solve(B)
    cols = dr.forward_error_columns(X, Xref) / fb
    Bf = np.ascontiguousarray(B[:, :dr.ROUTE_NRHS_FUSED])
    Xf = ctx.chol_solve(Bf)
    cols_f = dr.forward_error_columns(Xf, Xref[:, :dr.ROUTE_NRHS_FUSED]) / fb
    _report('routes n={}'.format(n), generic_worst_column=np.max(cols), fused_worst_column=np.max(cols_f))
    assert np.all(np.isfinite(cols)) and np.all(np.isfinite(cols_f))
    assert np.max(cols) <= 1.0, (int(np.argmax(cols)), float(np.max(cols)))
    assert np.max(cols_f) <= 1.0, (int(np.argmax(cols_f)), float(np.max(cols_f)))


# ---- 7. state -------------------------------------------------------------------------------------------------
def test_state_across_failed_and_smaller_factorisations(vb):
    hip = vb._hip
    c = _carrier(vb)
    try:
        def solve_and_check(n):
            S, B, Xref = dr.state_case(n)
            c.chol_factor(S)
            f, bk = _solve_ratios(S, c.chol_solve(B), B, Xref, dr.SWEEP_KAPPA)
            _report('state n={}'.format(n), forward=f, backward=bk)
            assert f <= 1.0 and bk <= 1.0, (n, f, bk)
            return S, B

        S193, B193 = solve_and_check(193)
        with pytest.raises(np.linalg.LinAlgError):
            c.chol_factor(dr.broken_pivot(70))
        # the factor is stale (for the old size and for the size that failed): the library refuses and writes nothing
        for n, B in ((193, B193), (dr.PIVOT_N, np.ones((dr.PIVOT_N, 6)))):
            with pytest.raises(RuntimeError, match='no Cholesky factor'):
                c.chol_solve(B)
            with pytest.raises(RuntimeError, match='no Cholesky factor'):
                c.lrvb_cov(np.ascontiguousarray(B.T))
            X = np.full((n, 6), SENTINEL)
            assert c._lib.lrvb_chol_solve(c._h, hip.ptr(hip.as_f64(B)), n, 6, hip.ptr(X)) == hip.ERR_STATE
            assert np.all(X == SENTINEL)
            cov = np.full((6, 6), SENTINEL)
            assert c._lib.lrvb_lrvb_cov(c._h, hip.ptr(hip.as_f64(B.T)), 6, n, hip.ptr(cov)) == hip.ERR_STATE
            assert np.all(cov == SENTINEL)
        # a smaller matrix in the larger allocation
        S65, B65 = solve_and_check(65)
        with pytest.raises((RuntimeError, ValueError)):
            c.chol_solve(np.ones((64, 3)))
        with pytest.raises((RuntimeError, ValueError)):
            c.lrvb_cov(np.ones((3, 64)))
        X = np.full((64, 3), SENTINEL)
        assert c._lib.lrvb_chol_solve(c._h, hip.ptr(np.ones((64, 3))), 64, 3, hip.ptr(X)) != hip.OK
        assert np.all(X == SENTINEL)
        # the refusal left the factor in place
        _, _, Xref65 = dr.state_case(65)
        f, bk = _solve_ratios(S65, c.chol_solve(B65), B65, Xref65, dr.SWEEP_KAPPA)
        assert f <= 1.0 and bk <= 1.0, (f, bk)
        solve_and_check(130)
    finally:
        c.close()


# ---- 8. device-resident entries ---------------------------------------------------------------------------------
@pytest.mark.parametrize('D', dr.DEV_D)
def test_device_resident_entries(vb, D):
    """H is the view H[:, :D] of a D x (D + 3) buffer: leading dimension D + 3 (at D = 130 odd rows are 8-byte but not
    16-byte aligned).  Bitwise the host entries' results; the padding columns and the matrix itself are left alone."""
    import torch
    dev = torch.device('cuda:0')
    S, B, M = dr.dev_case(D)
    Q, nrhs = M.shape[0], B.shape[1]
    c = _carrier(vb)
    try:
        buf = torch.full((D, D + 3), SENTINEL, dtype=torch.float64, device=dev)
        H = buf[:, :D]
        H.copy_(torch.from_numpy(S.copy()))
        Bt = torch.from_numpy(B.copy()).to(dev)
        Mt = torch.from_numpy(M.copy()).to(dev)
        cov_t = torch.full((Q, Q), SENTINEL, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert H.data_ptr() == buf.data_ptr() and H.stride(0) == D + 3
        with pytest.raises(ValueError):
            c.chol_factor_dev(H.data_ptr(), D, D - 1)
        c.chol_factor_dev(H.data_ptr(), D, D + 3)
        c.chol_solve_dev(Bt.data_ptr(), D, nrhs)
        c.lrvb_cov_dev(Mt.data_ptr(), Q, D, cov_t.data_ptr())
        c.sync()
        X_dev, cov_dev, buf_after = Bt.cpu().numpy(), cov_t.cpu().numpy(), buf.cpu().numpy()
        c.chol_factor(S)
        X_host, cov_host = c.chol_solve(B), c.lrvb_cov(M)
        assert np.all(np.isfinite(X_host)) and np.all(np.isfinite(cov_host))
        assert np.array_equal(X_dev, X_host)
        assert np.array_equal(cov_dev, cov_host)
        assert np.all(buf_after[:, D:] == SENTINEL)
        assert np.array_equal(buf_after[:, :D], S)
    finally:
        c.close()


# ---- 9. gemv routes through CG on a resident matrix -----------------------------------------------------------------
@pytest.mark.parametrize('D', dr.CG_D)
def test_cg_resident_matrix_gemv_routes(ctx, D):
    """gemv_n_tall_kernel<2> at D = 256, <4> for even D up to 512, <8> up to 1024; the generic kernel for odd D, D < 256 and
    D > 1024.  True residual (longdouble) <= 2 tol: the stopping rule ||r|| < tol ||b|| of the header on the recurrence
    residual, and a factor 2 for its drift from the true one (of order eps kappa iterations ~ 1e-12 here)."""
    S, b = dr.cg_case(D)
    tol = dr.CG_TOL
    Minv = np.diag(1.0 / np.diag(S))
    worst = 0.0
    for tag, H, kw in (('plain', S, {}), ('dense Minv', S, dict(Minv=Minv)), ('resident', None, {}), ('resident, Minv', None, dict(Minv=Minv))):
        x, info, iters = ctx.cg_solve_matrix(H, b, tol=tol, **kw)
        res = dr.true_residual(S, x, b)
        worst = max(worst, res / (2.0 * tol))
        assert info == 0, (tag, info, iters)
        assert 0 < iters < 10 * D, (tag, iters)
        assert res <= 2.0 * tol, (tag, res, iters)
    _report('cg D={}'.format(D), residual_over_2tol=worst)

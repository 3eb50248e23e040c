"""CPU proof that the inputs and bounds of tests/test_gpu_dense_linalg.py are fair: the helpers of
tests/dense_reference.py agree with 60-digit mpmath, and on EVERY matrix the GPU file uses both LAPACK's cho_solve and a
plain NumPy emulation of the device algorithm (64-column blocks, four-column diagonal step with reciprocal square roots,
explicit 16 -> 32 -> 64 inverse blocks, solves by products with them) sit inside every bound asserted there.

Measured here (worst ratio to the bound): forward LAPACK 0.25 / emulation 0.25 (both at n = 2; 0.02 to 0.1 from n = 65 up),
backward 0.34 / 0.15 (n <= 2; below 0.01 from n = 65 up), per-column forward at 16400 right-hand sides 0.12 / 0.17, and at
kappa = 1e10 and 1e12 both meet the plain n eps backward bound with a ratio below 0.004.  lrvb_cov: LAPACK below 0.1 of the
bound from n = 15 up (the 10x slack the bound was chosen with); at n <= 5 LAPACK itself is at 0.10 to 0.22, because the
handful of roundings of ANY floating-point route already costs that much of eps kappa when nothing averages -- there only
`inside the bound` is asserted of the reference, the device bound is the same at every n."""
import numpy as np
import pytest

import dense_reference as dr

EPS = dr.EPS


def _mp_matrix(mp, A):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(A)])


@pytest.mark.parametrize('n,kappa', [(5, 1e4), (17, 1e12), (33, 1e4), (33, 1e12)])
def test_helpers_against_mpmath(n, kappa):
    import mpmath as mp
    with mp.workdps(60):
        rng = np.random.default_rng(100 + n)
        S = dr.spd_with_spectrum(rng, n, kappa)
        B = rng.normal(size=(n, 2))
        Sm, Bm = _mp_matrix(mp, S), _mp_matrix(mp, B)
        cols = [mp.lu_solve(Sm, Bm[:, j]) for j in range(2)]
        Xm = mp.matrix(n, 2)
        for j in range(2):
            for i in range(n):
                Xm[i, j] = cols[j][i]
        Xref = dr.refined_solve(S, B)
        # the refined solution against the 60-digit one: at least 100 times closer than the bound it is used to judge
        num = mp.sqrt(sum((mp.mpf(float(np.float64(Xref[i, j]))) + mp.mpf(float(Xref[i, j] - np.longdouble(np.float64(Xref[i, j])))) - Xm[i, j]) ** 2
                          for i in range(n) for j in range(2)))
        den = mp.sqrt(sum(Xm[i, j] ** 2 for i in range(n) for j in range(2)))
        ref_err = float(num / den)
        print('refined vs mpmath n={} kappa={:.0e}: {:.3g} (eps kappa = {:.3g})'.format(n, kappa, ref_err, EPS * kappa))
        assert ref_err <= 1e-2 * EPS * kappa
        # forward_error / backward_error of a LAPACK solution, recomputed at 60 digits
        X = dr.lapack_solve(S, B)
        Xd = _mp_matrix(mp, X)
        fe = float(mp.sqrt(sum((Xd[i, j] - Xm[i, j]) ** 2 for i in range(n) for j in range(2))) / den)
        assert abs(dr.forward_error(X, Xref) - fe) <= 1e-2 * fe
        R = Bm - Sm * Xd
        be = float(max(abs(R[i, j]) for i in range(n) for j in range(2))
                   / (mp.mpf(float(np.max(np.sum(np.abs(S), axis=1)))) * mp.mpf(float(np.max(np.abs(X)))) + mp.mpf(float(np.max(np.abs(B))))))
        assert abs(dr.backward_error(S, X, B) - be) <= 1e-2 * be
        # the condition number is the constructed one
        assert abs(np.linalg.cond(S) / dr.kappa_by_construction(n, kappa) - 1.0) < (1e-6 if kappa <= 1e6 else 1e-2)
        # first_bad_pivot against an unblocked Cholesky at 60 digits
        L = np.linalg.cholesky(S)
        for k in (0, n // 2, n - 1):
            Sb = S.copy()
            Sb[k, k] -= 1.5 * L[k, k] ** 2
            A = _mp_matrix(mp, Sb)
            Lm, bad = mp.zeros(n, n), 0
            for c in range(n):
                d = A[c, c] - sum(Lm[c, t] ** 2 for t in range(c))
                if not d > 0:
                    bad = c + 1
                    break
                Lm[c, c] = mp.sqrt(d)
                for r in range(c + 1, n):
                    Lm[r, c] = (A[r, c] - sum(Lm[r, t] * Lm[c, t] for t in range(c))) / Lm[c, c]
            assert bad == k + 1 == dr.first_bad_pivot(Sb)
        assert dr.first_bad_pivot(S) == 0


def _both_routes(S):
    L, Ws, info = dr.emulated_factor(S)
    assert info == 0
    return (('lapack', lambda B: dr.lapack_solve(S, B), lambda M: M @ dr.lapack_solve(S, M.T)),
            ('emulation', lambda B: dr.emulated_solve(L, Ws, B), lambda M: dr.emulated_cov(L, Ws, M)))


def _assert_solve(S, solve, B, Xref, kappa, tag, plain_backward=False):
    n = S.shape[0]
    fb, bb = dr.bounds(n, kappa)
    if plain_backward:
        bb = n * EPS
    X = solve(B)
    f, bk = dr.forward_error(X, Xref) / fb, dr.backward_error(S, X, B) / bb
    assert f <= 1.0 and bk <= 1.0, (tag, f, bk)
    return f, bk


@pytest.mark.parametrize('n', dr.SWEEP_N)
def test_block_edge_inputs_are_fair(n):
    S, kappa, B, Xref, M, XrefM = dr.sweep_case(n)
    for name, solve, cov in _both_routes(S):
        for nr in dr.SWEEP_NRHS:
            _assert_solve(S, solve, np.ascontiguousarray(B[:, :nr]), Xref[:, :nr], kappa, (name, n, nr))
        _assert_solve(S, solve, np.ascontiguousarray(B[:, 1]), Xref[:, 1], kappa, (name, n, '1-D'))
        for Q in dr.SWEEP_Q:
            m = np.ascontiguousarray(M[:Q])
            err, scale = dr.cov_error(cov(m), m, XrefM[:, :Q])
            ratio = err / (EPS * kappa * scale)
            assert ratio <= 1.0, (name, n, Q, ratio)
            if name == 'lapack' and n >= 15:
                assert ratio <= 0.1, (n, Q, ratio)          # the 10x slack of the covariance bound (module docstring for n <= 5)


@pytest.mark.parametrize('kappa', dr.COND_KAPPA)
@pytest.mark.parametrize('n', dr.COND_N)
def test_conditioning_inputs_are_fair(n, kappa):
    """Both routes meet the forward bound and the PLAIN n eps backward bound at every kappa (tighter than the n eps sqrt(kappa)
    the GPU test asserts above 1e6), on S and, after unscaling, on the exactly scaled D S D; the emulation is bitwise invariant to the scaling."""
    S, B, Xref, d = dr.cond_case(n, kappa)
    Ss, Bs = S * d[:, None] * d[None, :], d[:, None] * B
    assert np.array_equal(Ss / d[:, None] / d[None, :], S) and np.array_equal(Bs / d[:, None], B)     # the scaling is exact
    for (name, solve, _), (_, solve_s, _) in zip(_both_routes(S), _both_routes(Ss)):
        _assert_solve(S, solve, B, Xref, kappa, (name, n, kappa), plain_backward=True)
        Xs = d[:, None] * solve_s(Bs)
        assert dr.forward_error(Xs, Xref) <= EPS * kappa, (name, n, kappa)
        if name == 'emulation':
            assert np.array_equal(Xs, solve(B))


@pytest.mark.parametrize('n', dr.ROUTE_N)
def test_route_inputs_are_fair(n):
    S, B, Xref = dr.route_case(n)
    assert B.shape == (n, dr.ROUTE_NRHS) and -(-dr.ROUTE_NRHS // 64) * 2 > 512 >= (dr.ROUTE_NRHS_FUSED // 64) * 2
    for name, solve, _ in _both_routes(S):
        cols = dr.forward_error_columns(solve(B), Xref) / (EPS * dr.ROUTE_KAPPA)
        assert np.max(cols) <= 1.0, (name, n, float(np.max(cols)))


@pytest.mark.parametrize('n', dr.STATE_SIZES)
def test_state_inputs_are_fair(n):
    S, B, Xref = dr.state_case(n)
    for name, solve, _ in _both_routes(S):
        _assert_solve(S, solve, B, Xref, dr.SWEEP_KAPPA, (name, n))


def test_remaining_matrices_factor():
    """The matrices of the symmetry, lower-triangle and device-entry tests are compared bitwise with another route of the
    device there, not with a bound: here they only have to be positive definite and finite in both routes."""
    mats = [dr.sym_case(n, Q)[0] for n, Q in dr.SYM_CASES] + [dr.lower_case(n)[0] for n in dr.LOWER_N] + [dr.dev_case(D)[0] for D in dr.DEV_D]
    for S in mats:
        assert dr.first_bad_pivot(S) == 0 and dr.emulated_factor(S)[2] == 0
        assert abs(np.linalg.cond(S) / dr.SWEEP_KAPPA - 1.0) < 1e-6


def test_pivot_cases_in_reference_and_emulation():
    for k in dr.PIVOT_POSITIONS:
        S = dr.broken_pivot(k)
        assert dr.first_bad_pivot(S) == k + 1 == dr.emulated_factor(S)[2]
    for tag, S in dr.nonfinite_cases():
        want = dr.first_bad_pivot(S)
        stated = dr.expected_nonfinite_index(tag)
        assert want >= 1 and (stated is None or stated == want), tag
        assert dr.emulated_factor(S)[2] == want, tag
    # +Inf on the diagonal is a bad pivot at its own position: nothing before it is disturbed
    for tag, S in dr.nonfinite_cases():
        if tag.startswith('inf'):
            assert dr.first_bad_pivot(S) == int(tag[4:-1].split(',')[0]) + 1


@pytest.mark.parametrize('n', dr.LOWER_N)
def test_emulation_reads_the_lower_triangle_only(n):
    S, B = dr.lower_case(n)
    Sn = S.copy()
    Sn[np.triu_indices(n, 1)] = np.nan
    L, Ws, info = dr.emulated_factor(S)
    Ln, Wn, info_n = dr.emulated_factor(Sn)
    assert info == info_n == 0 and dr.first_bad_pivot(Sn) == 0
    assert np.array_equal(dr.emulated_solve(L, Ws, B), dr.emulated_solve(Ln, Wn, B))


@pytest.mark.parametrize('D', dr.CG_D)
def test_cg_inputs_are_fair(D):
    """The documented loop in plain NumPy meets the true-residual bound 2 tol, with and without the dense diagonal
    preconditioner, far inside its iteration budget."""
    S, b = dr.cg_case(D)
    for Minv in (None, np.diag(1.0 / np.diag(S))):
        x, info, iters = dr.host_pcg(S, b, Minv=Minv, tol=dr.CG_TOL)
        assert info == 0 and iters < D + 200
        assert dr.true_residual(S, x, b) <= 2.0 * dr.CG_TOL

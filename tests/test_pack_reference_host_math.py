"""The references of tests/pack_reference.py checked on the CPU, at the shapes tests/test_gpu_pack.py runs (DESIGN.md
section 30): the two oracles agree, plain float64 NumPy sits inside the entry-wise bound, single mistakes in an emulation of
the kernel's gather break the exact oracle and leave the bound by >= 100x, and the figures behind the box-complement fix."""
import mpmath as mp
import numpy as np
import pytest

import pack_reference as pr
from helpers import rel_err
from oracle import packing as opk

F64, LD = np.float64, pr.LD


def test_definitions_agree_at_small_orders():
    """The gather form of J^T A and of the second-order term against the definitions dA = dL L^T + L dL^T and a central
    difference of it, and against the project's own oracle (which states the same closed forms independently)."""
    rng = np.random.default_rng(0)
    for k in (1, 2, 3, 6):
        spec = [('psd', 'm', k, 0.3)]
        m = k * (k + 1) // 2
        f = rng.normal(size=m)
        J = pr.psd_jac_dense_definition(f, k)
        A = rng.normal(size=(m, 4))
        assert np.max(np.abs((J.T @ A.astype(LD) - pr.psd_jt_apply(f, k, A.astype(LD))).astype(F64))) < 1e-16 * np.max(np.abs(J.astype(F64))) * 10 * k
        assert rel_err(J.astype(F64), opk.psd_jac(f, k)) < 1e-15
        g = rng.normal(size=m)
        T = pr.psd_third(f, k, g).astype(F64)
        assert rel_err(T, opk.psd_third(f, k, g)) < 1e-14
        h = 1e-5                                       # d/df of J^T g: the second-order term by differences of the definition
        for col in range(m):
            e = np.zeros(m)
            e[col] = h
            num = ((pr.psd_jac_dense_definition(f + e, k).T - pr.psd_jac_dense_definition(f - e, k).T) @ g.astype(LD) / (2 * h)).astype(F64)
            assert np.max(np.abs(num - T[:, col])) < 1e-7 * max(1.0, np.max(np.abs(T)))
    # box and simplex in mpmath against differences of eta in mpmath
    with mp.workprec(200):
        for lb, ub in ((-np.inf, np.inf), (3.0, np.inf), (-np.inf, 4.0), (-2.0, 5.0)):
            for f in (-3.0, 0.25, 7.0):
                h = mp.mpf(2) ** -60
                e = pr.box_mp(f, lb, ub)
                ep, em = pr.box_mp_at(mp.mpf(f) + h, lb, ub)[0], pr.box_mp_at(mp.mpf(f) - h, lb, ub)[0]
                assert abs((ep - em) / (2 * h) - e[1]) < mp.mpf(2) ** -100 * (1 + abs(e[1]))
                assert abs((ep - 2 * e[0] + em) / h ** 2 - e[2]) < mp.mpf(2) ** -70 * (1 + abs(e[2]))


def all_exact_jt_cases():
    for k in range(1, 64):
        yield pr.a_spec(k, (0.0, 0.25, 0.5)[k % 3]), 70, k
    for Q in pr.A_EDGE_Q:
        for k in pr.A_EDGE_K:
            yield pr.a_spec(k), Q, 1000 * Q + k
    for k1, k2, nb in pr.B_CASES:
        yield pr.b_spec(k1, k2, nb), 70, 100 * k1 + k2


def test_two_oracles_agree_on_products():
    """float64 and longdouble give the same J^T A on the integer inputs, entry for entry, with the margin asserted."""
    for spec, Q, seed in all_exact_jt_cases():
        rng = np.random.default_rng(seed)
        theta, A = pr.exact_theta(spec, rng), pr.int_matrix(rng, (pr.sizes(spec)[1], Q))
        w64, wld = pr.jt_apply(spec, theta, A, F64), pr.jt_apply(spec, theta, A, LD)
        assert np.array_equal(w64.astype(LD), wld)
        pr.assert_exact_margin(np.max(pr.jt_apply(spec, theta, A, F64, True)))
        pr.assert_sixteenths(w64)


@pytest.mark.parametrize('k,simplex', pr.C_CASES)
def test_two_oracles_agree_on_hessians(k, simplex):
    spec = pr.a_spec(k) + ([('simplex', 's', 2, 2)] if simplex else [])
    D, V = pr.sizes(spec)
    rng = np.random.default_rng(k)
    theta, H = pr.exact_theta(spec, rng), pr.int_matrix(rng, (V, V))
    if simplex:
        H[V - 4:, :] = 0.0
        H[:, V - 4:] = 0.0
    w64 = pr.jthj(spec, theta, H, F64)
    pr.assert_exact_margin(np.max(pr.jthj(spec, theta, H, F64, True)))
    pr.assert_sixteenths(w64)
    if k <= 33:
        assert np.array_equal(w64.astype(LD), pr.jthj(spec, theta, H, LD))
    if k <= 17:                                       # and the dense J^T H J of the project's oracle, exact on these inputs too
        lay = opk.Layout([opk.box_block(3, -2.0, 5.0), opk.psd_block(k, 0.25), opk.box_block(2)] + ([opk.simplex_block(2, 2)] if simplex else []))
        J = lay.jac(theta)
        assert np.array_equal(J.T @ H @ J, w64)


@pytest.mark.parametrize('k', [1, 2, 17, 40])
def test_two_oracles_agree_on_second_order(k):
    spec = pr.d_spec(k)
    rng = np.random.default_rng(k)
    theta, g = pr.exact_theta(spec, rng), pr.int_matrix(rng, pr.sizes(spec)[1])
    t64 = pr.third_order(spec, theta, g, F64)[0]
    assert np.array_equal(t64.astype(LD), pr.third_order(spec, theta, g, LD)[0])
    pr.assert_sixteenths(t64)
    if k <= 17:
        lay = opk.Layout([opk.box_block(3, 0.0, np.inf), opk.box_block(2, -np.inf, 4.0), opk.box_block(2, -2.0, 5.0), opk.psd_block(k, 0.5), opk.box_block(2)])
        assert np.array_equal(lay.third_order(theta, g), t64)


@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 130])
def test_round_trip_is_exact(k):
    """vec(L L^T + diag_lb I) of an integer L with unit diagonal and its Cholesky factor back, by the left-looking recurrence
    of psd_unconstrain_kernel in float64: every pivot is exactly 1."""
    spec = [('box', 'two', 2, -2.0, 5.0), ('psd', 'm', k, (0.0, 0.25, 0.5)[k % 3])]
    theta = pr.exact_theta(spec, np.random.default_rng(k))
    eta = pr.constrain(spec, theta, F64)[0]
    assert np.array_equal(eta.astype(LD), pr.constrain(spec, theta, LD)[0])
    pr.assert_sixteenths(eta)
    A = np.zeros((k, k))
    A[np.tril_indices(k)] = eta[2:]
    L = np.zeros((k, k))
    for j in range(k):
        d = A[j, j] - spec[1][3] - np.sum(L[j, :j] ** 2)
        assert d == 1.0
        L[j, j] = 1.0
        L[j + 1:, j] = A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]
    back = L[np.tril_indices(k)]
    back[pr.ld_idx(np.arange(k), np.arange(k))] = 0.0
    assert np.array_equal(back, theta[2:])


# ---- float64 NumPy inside the bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [17, 33, 61])
def test_float64_product_inside_the_bound(k):
    spec = pr.a_spec(k)
    rng = np.random.default_rng(k)
    theta, A = pr.real_theta(spec, rng), pr.real_matrix(rng, (pr.sizes(spec)[1], 70))
    ref, bound = pr.jt_apply_bounded(spec, theta, A)
    got = emulate_layout_jt(spec, theta, A)
    q = pr.ratio(got, ref, bound)
    print('pack host ratio jt k={}: {:.3f}'.format(k, q))
    assert q <= 1.0
    # the gap this file closes: ONE wrong small entry passes the norm-wise check at 1e-13 and leaves the bound by > 100x
    wrong = got.copy()
    i, j = np.unravel_index(np.argmin(np.where(got == 0, np.inf, np.abs(got))), got.shape)
    wrong[i, j] *= 1.5
    assert rel_err(wrong, ref.astype(F64)) < 1e-13
    assert pr.ratio(wrong, ref, bound) > 100.0


def emulate_layout_jt(spec, theta, A, mistake=None, trans_in=False):
    """float64 emulation of jt_apply_kernel over a layout of box and log-Cholesky blocks."""
    blocks, D, V = pr.blocks_of(spec)
    Q = A.shape[0] if trans_in else A.shape[1]
    out = np.zeros((D, Q))
    for b in blocks:
        f = theta[b['fo']:b['fo'] + b['nf']]
        fs, vs = slice(b['fo'], b['fo'] + b['nf']), slice(b['vo'], b['vo'] + b['nv'])
        if b['kind'] == 'box':
            d1 = pr.box_eval_f64(f, b['lb'], b['ub'])[1]
            out[fs] = d1[:, None] * (A[:, vs].T if trans_in else A[vs])
        else:
            out[fs] = pr.emulate_jt_psd(f, b['k'], A[:, vs] if trans_in else A[vs], mistake, trans_in)
    return out


@pytest.mark.parametrize('k', [5, 17, 33])
def test_float64_hessian_inside_the_bound(k):
    spec = pr.a_spec(k)
    rng = np.random.default_rng(k)
    V = pr.sizes(spec)[1]
    theta, H = pr.real_theta(spec, rng), pr.real_matrix(rng, (V, V))
    ref, bound = pr.free_hessian_bounded(spec, theta, np.zeros(V), H)
    W = emulate_layout_jt(spec, theta, H, None, True)              # (H J)^T, then J^T (H J): the device's two transposed reads
    got = emulate_layout_jt(spec, theta, W, None, True)
    q = pr.ratio(got, ref, bound)
    print('pack host ratio JtHJ k={}: {:.3f}'.format(k, q))
    assert q <= 1.0


@pytest.mark.parametrize('k', [5, 17])
def test_float64_second_order_and_maps_inside_the_bound(k):
    spec = pr.d_spec(k) + [('simplex', 's', 3, 4)]
    lay = opk.Layout([opk.box_block(3, 0.0, np.inf), opk.box_block(2, -np.inf, 4.0), opk.box_block(2, -2.0, 5.0), opk.psd_block(k, 0.5),
                      opk.box_block(2), opk.simplex_block(3, 4)])
    rng = np.random.default_rng(k)
    V = pr.sizes(spec)[1]
    theta, g = pr.real_theta(spec, rng), pr.real_matrix(rng, (1, V))[0]
    ref, bound = pr.third_order(spec, theta, g)
    q = [pr.ratio(lay.third_order(theta, g), ref, bound)]
    ref, bound = pr.constrain(spec, theta)
    q.append(pr.ratio(lay.constrain(theta), ref, bound))
    ref, bound = pr.dense_jac(spec, theta)
    q.append(pr.ratio(lay.jac(theta), ref, bound))
    print('pack host ratio T, eta, J k={}: {}'.format(k, ['{:.3f}'.format(v) for v in q]))
    assert max(q) <= 1.0


@pytest.mark.parametrize('K', [2, 3, 17])
def test_float64_simplex_inside_the_bound(K):
    rng = np.random.default_rng(K)
    for frow in pr.simplex_rows(K, rng):
        g = pr.real_matrix(rng, (1, K))[0]
        P, pb, J, Jb, T, Tb = pr.simplex_row_all(frow, g)
        p64, J64 = pr.simplex_row_f64(frow)
        q = [pr.ratio(p64, P, pb + pr.TINY), pr.ratio(J64, J, Jb + pr.TINY), pr.ratio(pr.simplex_third_f64(frow, g), T, Tb + pr.TINY)]
        assert max(q) <= 1.0, (K, frow, q)
        if abs(frow).max() < 100:                     # the `common` term dropped leaves the bound
            assert pr.ratio(pr.simplex_third_f64(frow, g, True), T, Tb + pr.TINY) > 100.0


# ---- single mistakes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mistake', pr.MISTAKES)
@pytest.mark.parametrize('k', [17, 33])
def test_single_mistakes_are_caught(k, mistake):
    """Each mistake alone changes the integer result and leaves the real-data bound by >= 100x.  `no_laa` is the exception on
    the integer side: the exact inputs have L_aa = 1, so a missing closing factor is invisible there by construction and only
    the bounded oracle sees it (the test says so instead of pretending)."""
    rng = np.random.default_rng(k)
    if mistake == 'box_d2_sign':
        spec = pr.d_spec(k)
        theta, g = pr.exact_theta(spec, rng), np.ones(pr.sizes(spec)[1])
        want = np.diag(pr.third_order(spec, theta, g, F64)[0])[:7]
        got = np.concatenate([pr.box_eval_f64(theta[o:o + n], lb, ub, d2_sign=-1.0)[2] for o, n, lb, ub in ((0, 3, 0.0, np.inf), (3, 2, -np.inf, 4.0), (5, 2, -2.0, 5.0))])
        assert not np.array_equal(got, want)
        f = rng.uniform(-8, 8, 6)
        for lb, ub in ((0.0, np.inf), (-np.inf, 4.0), (-2.0, 5.0)):
            val, bnd = pr.box_arrays(f, lb, ub)
            assert pr.ratio(pr.box_eval_f64(f, lb, ub)[2], val[2], bnd[2]) <= 1.0
            assert pr.ratio(pr.box_eval_f64(f, lb, ub, d2_sign=-1.0)[2], val[2], bnd[2]) > 100.0
        return
    trans = mistake == 'transposed_read_swapped'
    spec = [('psd', 'm', k, 0.25)]
    m = pr.sizes(spec)[1]
    Q = m if trans else 70
    theta, A = pr.exact_theta(spec, rng), pr.int_matrix(rng, (m, Q))
    want = pr.jt_apply(spec, theta, A.T if trans else A, F64)
    assert np.array_equal(pr.emulate_jt_psd(theta, k, A, None, trans), want)             # the emulation itself is right
    changed = not np.array_equal(pr.emulate_jt_psd(theta, k, A, mistake, trans), want)
    assert changed == (mistake != 'no_laa')
    theta, A = pr.real_theta(spec, rng), pr.real_matrix(rng, (m, Q))
    ref, bound = pr.jt_apply_bounded(spec, theta, A.T if trans else A)
    assert pr.ratio(pr.emulate_jt_psd(theta, k, A, None, trans), ref, bound) <= 1.0
    assert pr.ratio(pr.emulate_jt_psd(theta, k, A, mistake, trans), ref, bound) >= 100.0


# ---- the figures behind the fix ----------------------------------------------------------------------------------------------------------------
def test_two_sided_complement_before_and_after():
    """eta' of a two-sided box (lb = -2, ub = 5) in float64 against mpmath.  With 1 - s formed by subtraction the relative error
    grows like e^f * 2^-53 (1e-12 at 10, 4e-8 at 20, 1e-3 at 30) and eta' is exactly 0 from f = 37; with the complement taken
    directly every f is inside the bound, and eta'(f) = eta'(-f) to within it.  The mirror point -f was always accurate."""
    fs = np.array([10.0, 20.0, 30.0, 36.0, 37.0, 40.0, 700.0, 800.0])
    for sign in (1.0, -1.0):
        val, bnd = pr.box_arrays(sign * fs, -2.0, 5.0)
        true = val[1].astype(F64)
        old = pr.box_eval_f64(sign * fs, -2.0, 5.0, 'subtract')[1]
        new = pr.box_eval_f64(sign * fs, -2.0, 5.0)[1]
        with np.errstate(divide='ignore', invalid='ignore'):
            rel_old = np.where(true > 0, np.abs(old - true) / true, 0.0)
            rel_new = np.where(true > 0, np.abs(new - true) / true, 0.0)
        print('two-sided eta\' sign {:+.0f}: relative error before {} after {}'.format(sign, rel_old, rel_new))
        assert np.all(np.abs(new.astype(LD) - val[1]).astype(F64) <= bnd[1] + pr.TINY)
        assert np.all(rel_new[:7] < 1e-15)
        if sign > 0:
            assert 1e-13 < rel_old[0] < 1e-11 and 1e-9 < rel_old[1] < 1e-6 and 1e-5 < rel_old[2] < 1e-1
            assert np.all(old[4:6] == 0.0) and np.all(rel_old[4:6] == 1.0)
            assert np.all(np.abs(old[:6].astype(LD) - val[1][:6]).astype(F64) > 100 * bnd[1][:6])
        else:
            assert np.all(rel_old[:7] < 1e-15)
    assert new[7] == 0.0 and true[7] == 0.0            # e^-800 is below float64: 0 is the right answer there


def test_simplex_complement_at_a_saturated_row():
    """Known behaviour, recorded and not changed here: the kernels form the complement (1 - p_j) by subtraction, so at a
    saturated row (one logit at 40: p_j = 1 - 4e-18 rounds to 1) the diagonal Jacobian entry p_j (1 - p_j) is 0 instead of
    4e-18 -- relative error 1 on an entry far below the row's scale p_j = 1.  The bound of section 30 is on that scale
    (p_k (delta + p_j)), so the tests hold it; whoever needs the entry itself relatively accurate must form 1 - p_j as the sum
    of the other p."""
    frow = np.array([40.0, 0.0])
    P, pb, J, Jb, _, _ = pr.simplex_row_all(frow)
    p64, J64 = pr.simplex_row_f64(frow)
    true = float(J[1, 0])
    rel = abs(J64[1, 0] - true) / true
    print('simplex J[1, 0] at logit 40: float64 {!r}, true {!r}, relative error {:.3g}'.format(J64[1, 0], true, rel))
    assert 1e-18 < true < 1e-17 and rel > 0.1
    assert pr.ratio(J64, J, Jb) <= 1.0

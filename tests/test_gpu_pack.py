"""The packing layer of `csrc/k_pack.hip` entry by entry: the free <-> vector maps, their Jacobians,
the second-order term and the structured product J^T A of `jt_apply_kernel`, on a data-free context, against the two oracles
of tests/pack_reference.py -- bitwise on integer inputs, inside a counted rounding bound on real data over decades.
`pytest -s` prints one `pack ratio` line per bounded case (error / bound, must stay <= 1)."""
import numpy as np
import pytest

import pack_reference as pr
from helpers import make_par

pytestmark = pytest.mark.gpu
INF = np.inf
F64 = np.float64
TINY = pr.TINY


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1, 'no HIP device visible'
    return lrvb_amd


def ctx_of(vb, spec):
    par, _ = make_par(vb, spec)
    return vb.DeviceContext(par.layout_blocks(), quad_kind=1)


a_spec, d_spec, b_spec = pr.a_spec, pr.d_spec, pr.b_spec


def assert_bitwise(spec, got, want, what):
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        pytest.fail('{}: {}'.format(what, pr.describe_mismatch(spec, got, want)))


def exact_jt(ctx, spec, Q, rng, what):
    D, V = pr.sizes(spec)
    theta, A = pr.exact_theta(spec, rng), pr.int_matrix(rng, (V, Q))
    want = pr.jt_apply(spec, theta, A, F64)
    pr.assert_exact_margin(np.max(pr.jt_apply(spec, theta, A, F64, True)), what)
    pr.assert_sixteenths(want, what)
    got = ctx.jac_t_matmul(theta, A)
    assert_bitwise(spec, got, want, what)
    return got


def exact_hessian(ctx, spec, rng, what, with_g, with_H, zero_from=None):
    """free_hessian_from_vector on integer g and a NON-symmetric integer H (rows and columns from `zero_from` on are zero)."""
    D, V = pr.sizes(spec)
    theta = pr.exact_theta(spec, rng)
    g = pr.int_matrix(rng, V) if with_g else np.zeros(V)
    H = pr.int_matrix(rng, (V, V)) if with_H else np.zeros((V, V))
    if zero_from is not None:
        g[zero_from:] = 0.0
        H[zero_from:, :] = 0.0
        H[:, zero_from:] = 0.0
    want = pr.jthj(spec, theta, H, F64) + pr.third_order(spec, theta, g, F64)[0]
    pr.assert_exact_margin(np.max(pr.jthj(spec, theta, H, F64, True)) + np.max(np.abs(want)), what)
    pr.assert_sixteenths(want, what)
    got = ctx.free_hessian_from_vector(theta, g, H)
    assert_bitwise(spec, got, want, what)
    return theta, g, H, got


def report(name, got, ref, bound):
    q = pr.ratio(got, ref, bound)
    print('pack ratio {}: {:.3f}'.format(name, q))
    return q


# ---- the premises of the exact oracle: this case runs first ------------------------------------------------------------------------
def test_a0_exactness_premises(vb):
    """Every exact case below rests on the device giving exp(+-0) = 1, 1 / (1 + 1) = 0.5 and log 1 = 0 exactly.  If this
    fails, the device's exp or log is not exact at these arguments and the bitwise failures of the other exact cases say
    nothing about the kernels' indexing; the bounded cases stay meaningful."""
    spec = [('box', 'free', 2, -INF, INF), ('box', 'lo', 2, 3.0, INF), ('box', 'hi', 2, -INF, 4.0), ('box', 'two', 2, -2.0, 5.0),
            ('psd', 'm', 2, 0.25)]
    ctx = ctx_of(vb, spec)
    theta = np.zeros(11)
    theta[[1, 3, 5, 7]] = -0.0
    theta[[0, 1]] = [2.0, -3.0]
    theta[9] = 3.0                                    # L = [[1, 0], [3, 1]]
    eta = ctx.constrain(theta)
    want = np.array([2.0, -3.0, 4.0, 4.0, 3.0, 3.0, 1.5, 1.5, 1.25, 3.0, 10.25])
    assert np.array_equal(eta, want), (eta, want)
    back = ctx.unconstrain(want)
    assert np.array_equal(back, theta), back          # log 1 = 0, log 3.5 - log 3.5 = 0 (array_equal takes -0 for 0)
    J = ctx.free_to_vector_jac(theta)
    assert np.array_equal(np.diag(J)[:8], [1, 1, 1, 1, 1, 1, 1.75, 1.75])
    T = ctx.free_hessian_from_vector(theta, np.ones(11), np.zeros((11, 11)))
    assert np.array_equal(np.diag(T)[:8], [0, 0, 1, 1, -1, -1, 0, 0])


# ---- a: jac_t_matmul, one block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k0,k1', [(1, 16), (17, 32), (33, 48), (49, 63)])
def test_a_every_order_at_q70(vb, k0, k1):
    for k in range(k0, k1 + 1):
        spec = a_spec(k, (0.0, 0.25, 0.5)[k % 3])
        exact_jt(ctx_of(vb, spec), spec, 70, np.random.default_rng(k), 'a k={} Q=70'.format(k))


@pytest.mark.parametrize('Q', pr.A_EDGE_Q)
def test_a_tile_edges_by_columns(vb, Q):
    for k in pr.A_EDGE_K:
        spec = a_spec(k)
        exact_jt(ctx_of(vb, spec), spec, Q, np.random.default_rng(1000 * Q + k), 'a k={} Q={}'.format(k, Q))


# ---- b: two blocks, box chunks, the single box block -----------------------------------------------------------------------------------
@pytest.mark.parametrize('k1,k2,nb', pr.B_CASES)
def test_b_two_blocks_and_box_chunks(vb, k1, k2, nb):
    spec = b_spec(k1, k2, nb)
    ctx = ctx_of(vb, spec)
    rng = np.random.default_rng(100 * k1 + k2)
    for Q in (70, 3):
        exact_jt(ctx, spec, Q, rng, 'b k=({}, {}) boxes={} Q={}'.format(k1, k2, nb, Q))
    if k1 + k2 <= 40:                                 # the other maps on the same layout (the unfused box kernels at nb = 1)
        D, V = pr.sizes(spec)
        theta = pr.exact_theta(spec, rng)
        assert_bitwise(spec, ctx.constrain(theta), pr.constrain(spec, theta, F64)[0], 'b constrain')
        assert_bitwise(spec, ctx.free_to_vector_jac(theta).T.copy(), pr.jt_apply(spec, theta, np.eye(V), F64), 'b jac^T')
        g = pr.int_matrix(rng, V)
        assert_bitwise(spec, ctx.free_hessian_from_vector(theta, g, np.zeros((V, V))), pr.third_order(spec, theta, g, F64)[0], 'b T')


# ---- c: J^T H J with a non-symmetric H; the recorded assembly; the dense route ------------------------------------------------------------
@pytest.mark.parametrize('k,simplex', pr.C_CASES)
def test_c_two_products(vb, k, simplex):
    """g = 0 isolates the two TRANS_IN = true products (k <= 63 without a simplex block) or the two dense products.  With a
    trailing simplex block theta is 0 there, but p = exp(0 - log 2) need not be exactly 1/2 on the device, so the simplex block
    gets g = 0 and zero rows and columns of H: its Jacobian only has to be finite."""
    spec = a_spec(k) + ([('simplex', 's', 2, 2)] if simplex else [])
    D, V = pr.sizes(spec)
    ctx = ctx_of(vb, spec)
    rng = np.random.default_rng(k)
    zf = V - 4 if simplex else None
    theta, g, H, got = exact_hessian(ctx, spec, rng, 'c k={} simplex={}'.format(k, simplex), False, True, zf)
    assert not np.array_equal(H, H.T)
    assert not np.array_equal(got, got.T)
    Hs = H + H.T
    direct = ctx.free_hessian_from_vector(theta, g, Hs)
    assert_bitwise(spec, direct, pr.jthj(spec, theta, Hs, F64), 'c symmetric')
    ctx.hvec_begin()
    ctx.hvec_add_block(Hs, 0, 0)
    assert_bitwise(spec, ctx.hvec_finish(theta, g), direct, 'c hvec_finish')       # one TRANS_IN = false product, then one true


# ---- d: the second-order term ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 17, 40])
def test_d_second_order_term(vb, k):
    spec = d_spec(k)
    ctx = ctx_of(vb, spec)
    rng = np.random.default_rng(k)
    theta, g, _, T = exact_hessian(ctx, spec, rng, 'd k={} T'.format(k), True, False)
    assert np.any(np.diag(T)[:5] != 0)
    D, V = pr.sizes(spec)
    H = pr.int_matrix(rng, (V, V))
    P = ctx.free_hessian_from_vector(theta, np.zeros(V), H)
    assert_bitwise(spec, ctx.free_hessian_from_vector(theta, g, H), P + T, 'd T accumulates into the product')


def test_d_single_box_block(vb):
    """One box block (the per-block box kernels, not the fused ones), one-sided so that eta'' = -1 shows its sign."""
    spec = [('psd', 'm', 3, 0.0), ('box', 'hi', 5, -INF, 4.0)]
    ctx = ctx_of(vb, spec)
    exact_hessian(ctx, spec, np.random.default_rng(5), 'd single box block', True, True)
    theta = pr.exact_theta(spec, np.random.default_rng(6))
    assert_bitwise(spec, ctx.constrain(theta), pr.constrain(spec, theta, F64)[0], 'constrain')
    assert_bitwise(spec, ctx.unconstrain(ctx.constrain(theta)), theta, 'unconstrain')
    assert_bitwise(spec, ctx.free_to_vector_jac(theta).T.copy(), pr.jt_apply(spec, theta, np.eye(11), F64), 'jac^T')


# ---- e: constrain / unconstrain round trip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 130])
def test_e_round_trip(vb, k):
    spec = [('box', 'two', 2, -2.0, 5.0), ('psd', 'm', k, (0.0, 0.25, 0.5)[k % 3])]
    ctx = ctx_of(vb, spec)
    theta = pr.exact_theta(spec, np.random.default_rng(k))
    want = pr.constrain(spec, theta, F64)[0]
    pr.assert_exact_margin(np.max(np.abs(want)))
    eta = ctx.constrain(theta)
    assert_bitwise(spec, eta, want, 'e constrain k={}'.format(k))
    assert_bitwise(spec, ctx.unconstrain(eta), theta, 'e unconstrain k={}'.format(k))


# ---- f: real data -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [17, 33, 61])
def test_f_real_jt(vb, k):
    spec = a_spec(k)
    rng = np.random.default_rng(k)
    theta, A = pr.real_theta(spec, rng), pr.real_matrix(rng, (pr.sizes(spec)[1], 70))
    ref, bound = pr.jt_apply_bounded(spec, theta, A)
    assert report('f jt k={}'.format(k), ctx_of(vb, spec).jac_t_matmul(theta, A), ref, bound) <= 1.0


@pytest.mark.parametrize('k', [5, 17, 33])
def test_f_real_two_products(vb, k):
    spec = a_spec(k)
    rng = np.random.default_rng(k)
    V = pr.sizes(spec)[1]
    theta, H = pr.real_theta(spec, rng), pr.real_matrix(rng, (V, V))
    ref, bound = pr.free_hessian_bounded(spec, theta, np.zeros(V), H)
    ctx = ctx_of(vb, spec)
    assert report('f JtHJ k={}'.format(k), ctx.free_hessian_from_vector(theta, np.zeros(V), H), ref, bound) <= 1.0
    Hs = H + H.T
    ref, bound = pr.free_hessian_bounded(spec, theta, np.zeros(V), Hs)
    ctx.hvec_begin()
    ctx.hvec_add_block(Hs, 0, 0)
    assert report('f hvec k={}'.format(k), ctx.hvec_finish(theta, np.zeros(V)), ref, bound) <= 1.0


@pytest.mark.parametrize('k', [5, 17])
def test_f_real_second_order(vb, k):
    spec = d_spec(k)
    rng = np.random.default_rng(k)
    V = pr.sizes(spec)[1]
    theta, g = pr.real_theta(spec, rng), pr.real_matrix(rng, (1, V))[0]
    ref, bound = pr.third_order(spec, theta, g)
    assert report('f T k={}'.format(k), ctx_of(vb, spec).free_hessian_from_vector(theta, g, np.zeros((V, V))), ref, bound) <= 1.0


def test_f_real_maps(vb):
    spec = d_spec(17) + [('simplex', 's', 3, 4)]
    rng = np.random.default_rng(17)
    theta = pr.real_theta(spec, rng)
    ctx = ctx_of(vb, spec)
    ref, bound = pr.constrain(spec, theta)
    assert report('f constrain', ctx.constrain(theta), ref, bound) <= 1.0
    ref, bound = pr.dense_jac(spec, theta)
    assert report('f free_to_vector_jac k=17', ctx.free_to_vector_jac(theta), ref, bound) <= 1.0


# ---- g: box edges ------------------------------------------------------------------------------------------------------------------------
G_F, G_SPEC = pr.G_F, pr.G_SPEC


def box_edge_ratios(ctx):
    """Worst error / bound of eta, eta', eta'' per block over f in G_F, and the list of broken range and limit rules."""
    n, fs = len(G_F), np.array(G_F)
    theta = np.tile(G_F, 4)
    eta = ctx.constrain(theta)
    d1 = np.diag(ctx.free_to_vector_jac(theta)).copy()
    refs = [pr.box_arrays(fs, lb, ub) for _, _, _, lb, ub in G_SPEC]
    over = np.concatenate([np.isinf(val[1].astype(F64)) for val, _ in refs])     # eta' = e^|f| beyond float64: |f| = 745, 800
    d2 = np.empty(4 * n)
    Z = np.zeros((4 * n, 4 * n))
    for i in range(4 * n):
        T = ctx.free_hessian_from_vector(theta, np.eye(4 * n)[i], Z)
        d2[i] = T[i, i]
        T[i, i] = 0.0
        assert not T[np.ix_(~over, ~over)].any()
    # with H = 0 the product part of an overflowed coordinate is Inf * 0 * Inf: its row, column and diagonal are NaN by the rules
    # of IEEE arithmetic, in every version of the kernels; eta'' is read where eta' is finite
    assert np.all(np.isnan(d2[over])) and not np.any(np.isnan(d2[~over]))
    out, broken = {}, []
    for bi, (_, name, _, lb, ub) in enumerate(G_SPEC):
        sl = slice(bi * n, (bi + 1) * n)
        if not (np.all(eta[sl] >= lb) and np.all(eta[sl] <= ub)):
            broken.append((name, 'eta outside [lb, ub]', eta[sl]))
        val, bnd = refs[bi]
        for what, got, j in (('eta', eta[sl], 0), ('d1', d1[sl], 1), ('d2', d2[sl], 2)):
            ref = val[j].astype(F64)
            inf = np.isinf(ref)                                    # +-Inf exactly where mathematics overflows float64
            if what == 'd2':
                got = np.where(over[sl], ref, got)
            if not np.array_equal(got[inf], ref[inf]) or not np.all(np.isfinite(got[~inf])):
                broken.append((name, what, 'Inf where the true value is finite, or the reverse', fs, got))
            zero = (got == 0.0) & ~inf                             # 0 only where the true value is 0 or below the normal range
            if (name, what) == ('two', 'd2'):                      # known: 1 - 2 s is exactly 0 at |f| = 1e-300 (section 30)
                zero &= np.abs(fs) >= 1.0
            if np.any(np.abs(ref[zero]) >= 2.0 ** -1022):
                broken.append((name, what, 'exactly 0 where the true value is a normal number, at f =', fs[zero & (np.abs(ref) >= 2.0 ** -1022)]))
            q = np.abs(got[~inf].astype(pr.LD) - val[j][~inf]).astype(F64) / (bnd[j][~inf] + TINY)
            out[(name, what)] = (float(np.max(q)), float(fs[~inf][np.argmax(q)]))
            if name == 'two' and what != 'eta':
                print('pack g two-sided {} error / bound at f = 10, 20, 30, 36, 37, 40: {}'.format(
                    what, ['{:.3g}'.format(v) for v in q[[6, 8, 10, 12, 14, 16]]]))
        if name == 'two':
            pos = np.arange(2, n, 2)                               # G_F[pos] = +v, G_F[pos + 1] = -v
            gap = np.abs(d1[sl][pos] - d1[sl][pos + 1]) / (bnd[1][pos] + bnd[1][pos + 1] + TINY)
            out[(name, 'd1 mirror')] = (float(np.max(gap)), float(fs[pos][np.argmax(gap)]))
    return out, broken


def test_g_box_edges(vb):
    """eta, eta' and eta'' of all four bound kinds at |f| up to 800 against mpmath.  Before the complement of the logistic was
    taken directly for f >= 0, the two-sided eta' left its bound on the MI355X by 540x at f = 10, 2.0e7 at 20, 5.7e11 at 30,
    2.4e13 at 36 and was exactly 0 from f = 37 (5.6e14); eta'' by 234x, 8.7e6, 2.5e11, 1.0e13, 2.4e14."""
    ratios, broken = box_edge_ratios(ctx_of(vb, G_SPEC))
    for key, (q, f) in sorted(ratios.items()):
        print('pack ratio g {} {}: {:.3g} at f = {}'.format(key[0], key[1], q, f))
    assert not broken, broken
    worst = max(ratios.items(), key=lambda kv: kv[1][0])
    assert worst[1][0] <= 1.0, worst


# ---- h: simplex ------------------------------------------------------------------------------------------------------------------------------
simplex_rows = pr.simplex_rows


def check_simplex(ctx, spec, theta, rng, what):
    D, V = pr.sizes(spec)
    g = pr.real_matrix(rng, (1, V))[0]
    ref, bound = pr.constrain(spec, theta)
    qs = [report(what + ' p', ctx.constrain(theta), ref, bound + TINY)]
    ref, bound = pr.dense_jac(spec, theta)
    qs.append(report(what + ' J', ctx.free_to_vector_jac(theta), ref, bound + TINY))
    ref, bound = pr.third_order(spec, theta, g)
    qs.append(report(what + ' T', ctx.free_hessian_from_vector(theta, g, np.zeros((V, V))), ref, bound + TINY))
    assert max(qs) <= 1.0, (what, qs)


@pytest.mark.parametrize('K', [2, 3, 17])
def test_h_simplex(vb, K):
    rng = np.random.default_rng(K)
    rows = simplex_rows(K, rng)
    spec5 = [('box', 'pre', 2, 0.0, INF), ('simplex', 's', 5, K)]
    check_simplex(ctx_of(vb, spec5), spec5, np.concatenate([[0.5, -1.0]] + rows), rng, 'h K={} rows=5'.format(K))
    spec1 = [('box', 'pre', 2, 0.0, INF), ('simplex', 's', 1, K)]
    ctx = ctx_of(vb, spec1)
    for i, r in enumerate(rows):
        check_simplex(ctx, spec1, np.concatenate([[0.5, -1.0], r]), rng, 'h K={} rows=1 row {}'.format(K, i))


# ---- i: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_i_refusals_leave_the_context_usable(vb):
    """Flag paths only: the Cholesky carries a NaN through its fixed loops, nothing is indexed by a value."""
    spec = a_spec(3, 0.5)
    ctx = ctx_of(vb, spec)
    rng = np.random.default_rng(3)
    first = exact_jt(ctx, spec, 70, np.random.default_rng(9), 'i before')
    good = ctx.constrain(pr.exact_theta(spec, rng))
    tri = np.tril_indices(3)
    indefinite, singular, outside = good.copy(), good.copy(), good.copy()
    indefinite[3:9] = (np.array([[1.0, 2, 0], [2, 1, 0], [0, 0, 1]]) + 0.5 * np.eye(3))[tri]
    singular[3:9] = (np.ones((3, 3)) + 0.5 * np.eye(3))[tri]              # A - diag_lb I has rank 1: the second pivot is 0
    outside[1] = 5.5                                                        # above ub = 5
    for bad, text in ((indefinite, 'not positive definite'), (singular, 'not positive definite'), (outside, 'outside the bounds')):
        with pytest.raises(ValueError, match=text):
            ctx.unconstrain(bad)
        assert np.array_equal(exact_jt(ctx, spec, 70, np.random.default_rng(9), 'i after ' + text), first)
    assert np.array_equal(ctx.unconstrain(good), pr.exact_theta(spec, np.random.default_rng(3)))


# ---- j: one context over many calls ----------------------------------------------------------------------------------------------------------
def test_j_repeat_and_fresh_context(vb):
    spec = d_spec(33)

    def one_round(ctx):
        rng = np.random.default_rng(33)
        out = [exact_jt(ctx, spec, 129, rng, 'j a Q=129')]
        out.append(exact_hessian(ctx, spec, rng, 'j c', False, True)[3])
        out.append(exact_hessian(ctx, spec, rng, 'j d', True, False)[3])
        out.append(exact_jt(ctx, spec, 1, rng, 'j a Q=1'))
        out.append(exact_hessian(ctx, spec, rng, 'j c+d', True, True)[3])
        return out
    ctx = ctx_of(vb, spec)
    r1, r2, r3 = one_round(ctx), one_round(ctx), one_round(ctx_of(vb, spec))
    for x, y, z in zip(r1, r2, r3):
        assert np.array_equal(x, y) and np.array_equal(x, z)

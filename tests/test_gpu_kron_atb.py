"""The Kronecker SYRK  K4 = sum_n c_n u_n u_n^T  (wsyrk_kron_kernel) and the two-operand product  C = A^T diag(c) B
(atb_glds_kernel<0 | 1 | 2>, the split reduction, atb_tiles_to_dense_kernel) of csrc/k_wsyrk.hip entry by entry, through the
thin entry points `ctx.kron_gram` and `ctx.weighted_atb`.

Two oracles (tests/kron_atb_reference.py): small-integer data, where the device result must be BITWISE
the exact product whatever the summation order, and real data against a longdouble reference with an entry-wise bound
K 2^-53 1.01 A_ij whose K is counted from the algorithm.  A failure names the entry: its index pairs, tile and block for K4,
its slot for the 528 x 528 sliver modes.

Known behaviour, not tested: the kernels clamp phantom rows (past N, inside the last 16-row stage) to row N - 1 and give them
weight zero, so an Inf or NaN in the LAST row of the data reaches entries through 0 * Inf; the NaN tests use row 37."""
import numpy as np
import pytest

import kron_atb_reference as kr

pytestmark = pytest.mark.gpu

BLOCKS = [dict(kind=0, free_size=3, vec_size=3, dim0=3, dim1=0, lb=-np.inf, ub=np.inf)]
P528 = kr.SLIVER_P


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1, 'no HIP device visible'
    return lrvb_amd


def kron_ctx(vb, Z):
    ctx = vb.DeviceContext(BLOCKS, loss='data_only', n_obs=Z.shape[0], n_cols=Z.shape[1], device=0)
    ctx.set_data(vb._hip.SLOT_X, Z)
    return ctx


@pytest.fixture(scope='module')
def actx(vb):
    """A context that only lends its stream and scratch to weighted_atb (it holds a small data matrix for kron_gram)."""
    Z, _ = kr.int_kron_case(np.random.default_rng(1), 40, 5)
    ctx = kron_ctx(vb, Z)
    yield ctx
    ctx.close()


def assert_kron_exact(K, want, q, label):
    if np.array_equal(K, want):
        return
    bad = np.argwhere(~(K == want))
    i, j = bad[0]
    raise AssertionError('{}: {} of {} entries differ; first ({}, {}) {}: got {!r}, want {!r}'.format(
        label, len(bad), K.size, i, j, kr.kron_entry(i, j, q), K[i, j], want[i, j]))


def assert_atb_exact(C, want, label, sliver=False):
    if np.array_equal(C, want):
        return
    bad = np.argwhere(~(C == want))
    i, j = bad[0]
    where = kr.sliver_slot(i, j) if sliver else 'tile ({}, {}), block ({}, {})'.format(i // 128, j // 128, (i % 128) // 16, (j % 128) // 16)
    slots = ''
    if sliver:
        wrong = ~(C == want)
        slots = '; wrong entries per slot: ' + ', '.join('{} {}'.format(k, int(wrong[m].sum())) for k, m in kr.slot_masks().items() if wrong[m].any())
    raise AssertionError('{}: {} of {} entries differ; first ({}, {}) [{}]: got {!r}, want {!r}{}'.format(
        label, len(bad), C.size, i, j, where, C[i, j], want[i, j], slots))


def check_kron(vb, N, q, seed=0, ctx=None):
    Z, c = kr.int_kron_case(np.random.default_rng(100003 * q + N + seed), N, q)
    own = ctx is None
    if own:
        ctx = kron_ctx(vb, Z)
    else:
        ctx.set_data(vb._hip.SLOT_X, Z)
    K = ctx.kron_gram(c)
    assert_kron_exact(K, kr.exact_kron(Z, c), q, kr.describe_kron(N, q))
    assert np.array_equal(K, K.T), 'upper triangle is not the mirror of the lower'
    if own:
        ctx.close()
    return Z, c, K


# ---- Kronecker SYRK ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', [0, 1, 2, 3])
def test_kron_exact_every_width(vb, group):
    """a. Every q in 1..64 at N = 50: every Pv mod 128 and mod 16, widths that are no multiple of the four columns a thread
    stages, the triangular decode at every v <= 2079, one (q = 32), seven (31), six (63) and two (64) real 16-blocks in the
    last tile."""
    for q in range(16 * group + 1, 16 * group + 17):
        check_kron(vb, kr.KRON_Q_SWEEP_N, q)


@pytest.mark.parametrize('stage', [0, 1, 2])
def test_kron_exact_rows_below_three_stages(vb, stage):
    """b. q = 16 (two tile rows: off-diagonal and diagonal workgroups), every N in 1..48: all ragged last stages, all but the
    first one to three splits empty."""
    for N in range(16 * stage + 1, 16 * stage + 17):
        check_kron(vb, N, kr.KRON_N_SWEEP_Q)


@pytest.mark.parametrize('N', kr.KRON_N_EXTRA)
def test_kron_exact_rows_around_split_boundaries(vb, N):
    check_kron(vb, N, kr.KRON_N_SWEEP_Q)


@pytest.mark.parametrize('N,q,splits', kr.KRON_SPLIT_CASES)
def test_kron_exact_split_counts(vb, N, q, splits):
    """c. The launcher's own split choice walked through N: 16, 24 (three groups of eight), 128, 72 and 64 splits."""
    assert kr.kron_splits(N, q) == splits
    check_kron(vb, N, q)


def int_quadform(rng, q):
    """Symmetric matrices with even integer entries and integer constants: every g_n[k] = 1/2 z^T M_k z + c_k is an integer."""
    M = 2.0 * rng.integers(-1, 2, size=(3, q, q))
    M = M + M.transpose(0, 2, 1)
    return M, rng.integers(-2, 3, size=3).astype(np.float64)


def test_kron_context_reuse(vb):
    """d. A context's row count is fixed, so the walk from 128 splits down to 8 goes through the scratch the entry points
    share: weighted_atb with 128 splits fills `tile_part` on a context whose own Kronecker product takes 8 (stale partials of
    the larger run behind the live ones), then a new X."""
    q, N = 15, 300
    assert kr.kron_splits(N, q) == 8 and kr.atb_splits(32771, 130, 130, 0) == 128
    rng = np.random.default_rng(11)
    Z, c = kr.int_kron_case(rng, N, q)
    ctx = kron_ctx(vb, Z)
    A, B, ca = kr.int_atb_case(rng, 32771, 130, 130)
    assert_atb_exact(ctx.weighted_atb(A, B, ca), kr.exact_atb(A, B, ca), '128 splits')
    assert_kron_exact(ctx.kron_gram(c), kr.exact_kron(Z, c), q, '8 splits behind 128')
    assert_atb_exact(ctx.weighted_atb(A[:300], B[:300], ca[:300]), kr.exact_atb(A[:300], B[:300], ca[:300]), '8 splits behind 128 (A^T c B)')
    Z2, _ = kr.int_kron_case(rng, N, q)
    ctx.set_data(vb._hip.SLOT_X, Z2)
    assert_kron_exact(ctx.kron_gram(c), kr.exact_kron(Z2, c), q, 'new X')
    ctx.close()


@pytest.mark.parametrize('reverse', [False, True])
def test_kron_gram_beside_quadform_gram(vb, reverse):
    """d. quadform_gram and kron_gram on one context in both orders: they share the weight column, the tiles and the dense
    scratch.  Integer matrices: G^T G is exact too."""
    q, N = 16, 1001
    rng = np.random.default_rng(21)
    Z, c = kr.int_kron_case(rng, N, q)
    M, cc = int_quadform(rng, q)
    G = 0.5 * np.einsum('na,kab,nb->nk', Z, M, Z) + cc[None, :]
    assert np.array_equal(G, np.rint(G)) and np.abs(G).max() ** 2 * N < 2.0 ** 53
    ctx = kron_ctx(vb, Z)
    steps = ['quadform', 'kron', 'kron_ones']
    for step in (steps[::-1] if reverse else steps):
        if step == 'quadform':
            assert_atb_exact(ctx.quadform_gram(M, cc, np.zeros(3)), G.T @ G, 'quadform_gram')
        elif step == 'kron':
            assert_kron_exact(ctx.kron_gram(c), kr.exact_kron(Z, c), q, 'kron_gram')
        else:
            assert_kron_exact(ctx.kron_gram(), kr.exact_kron(Z, np.ones(N)), q, 'kron_gram, unit weights')
    ctx.close()


def test_kron_zero_weights(vb):
    """e. Every other weight zero, then all of them."""
    q, N = 23, 1001
    Z, c = kr.int_kron_case(np.random.default_rng(31), N, q)
    ctx = kron_ctx(vb, Z)
    half = c.copy(); half[0::2] = 0.0
    assert_kron_exact(ctx.kron_gram(half), kr.exact_kron(Z[1::2], c[1::2]), q, 'every other weight zero')
    pv = q * (q + 1) // 2
    assert_kron_exact(ctx.kron_gram(np.zeros(N)), np.zeros((pv, pv)), q, 'all weights zero')
    assert_kron_exact(ctx.kron_gram(c), kr.exact_kron(Z, c), q, 'weights restored')
    ctx.close()


@pytest.mark.parametrize('N,q', kr.KRON_BOUND_SHAPES)
def test_kron_rounding_bound_every_entry(vb, N, q):
    """f. Real data: |K4 - ref| <= (L + S + 4) 2^-53 1.01 sum |c| |u_i| |u_j| at every entry of the lower triangle; the upper
    one is its exact mirror."""
    d = kr.real_kron_reference(N, q)
    bound = kr.bound_of(kr.kron_K(N, q), d['A'])
    ctx = kron_ctx(vb, d['Z'])
    K = ctx.kron_gram(d['c'])
    ctx.close()
    (i, j), ratio = kr.worst_entry(np.tril(K), np.tril(d['ref']), bound)
    print('kron rounding bound {}: K {}, max error / bound {:.4f} at ({}, {})'.format(kr.describe_kron(N, q), kr.kron_K(N, q), ratio, i, j))
    assert ratio <= 1.0, '{}: error / bound {:.3g} at ({}, {}) {}'.format(kr.describe_kron(N, q), ratio, i, j, kr.kron_entry(i, j, q))
    assert np.array_equal(K, K.T), 'upper triangle is not the mirror of the lower'


@pytest.mark.parametrize('N,q', [(1000, 16), (2000, 64)])
def test_kron_exact_power_of_two_scaling(vb, N, q):
    """g. Column a of z times 2^e_a and the weights times 2^7 scale K4[(a, b), (c, d)] by exactly 2^(7 + e_a + e_b + e_c + e_d):
    needs no reference; an entry that took a factor from another column breaks it."""
    d = kr.real_kron_reference(N, q)
    e = np.random.default_rng(N + q).integers(-10, 11, size=q)
    Z2, c2 = np.ldexp(d['Z'], e[None, :]), d['c'] * 128.0
    assert np.all(np.ldexp(Z2, -e[None, :]) == d['Z'])
    a, b = kr.tri_pairs(q)
    ev = e[a] + e[b]
    c1, c2x = kron_ctx(vb, d['Z']), kron_ctx(vb, Z2)
    K1, K2 = c1.kron_gram(d['c']), c2x.kron_gram(c2)
    c1.close(); c2x.close()
    want = np.ldexp(K1, 7 + ev[:, None] + ev[None, :])
    assert np.all(np.isfinite(want)) and np.all(np.abs(want[want != 0]) > 1e-200)
    assert_kron_exact(K2, want, q, 'scaling ' + kr.describe_kron(N, q))


@pytest.mark.parametrize('N,q', [(200, 16), (200, 64)])
def test_kron_nan_containment(vb, N, q):
    """h. A NaN in z[37, a] makes exactly the rows and columns whose pair contains a NaN; every other entry is bitwise what
    z[37, a] = 0 gives.  A NaN weight makes every entry NaN."""
    Z, c = kr.int_kron_case(np.random.default_rng(N + q), N, q)
    r = 37
    assert r < N - 16 and c[r] != 0
    pa, pb = kr.tri_pairs(q)
    ctx = kron_ctx(vb, Z)
    for a in (0, 3, q - 1):
        Z0 = Z.copy(); Z0[r, a] = 0.0
        Zn = Z.copy(); Zn[r, a] = np.nan
        want = kr.exact_kron(Z0, c)
        has = (pa == a) | (pb == a)
        hit = has[:, None] | has[None, :]
        ctx.set_data(vb._hip.SLOT_X, Zn)
        K = ctx.kron_gram(c)
        assert np.all(np.isnan(K[hit])), 'rows / columns with z_{} must be NaN'.format(a)
        assert_kron_exact(np.where(hit, 0.0, K), np.where(hit, 0.0, want), q, 'NaN at z[37, {}] leaked'.format(a))
    ctx.set_data(vb._hip.SLOT_X, Z)
    cn = c.copy(); cn[r] = np.nan
    assert np.all(np.isnan(ctx.kron_gram(cn))), 'a NaN weight must reach every entry'
    ctx.close()


@pytest.mark.parametrize('N,q', [(32775, 15), (2000, 64)])
def test_kron_repeatable_bitwise(vb, N, q):
    """i. The same input twice on one context and once on a fresh one."""
    d = kr.real_kron_reference(N, q)
    ctx = kron_ctx(vb, d['Z'])
    K1, K2 = ctx.kron_gram(d['c']), ctx.kron_gram(d['c'])
    ctx.close()
    ctx = kron_ctx(vb, d['Z'])
    K3 = ctx.kron_gram(d['c'])
    ctx.close()
    assert np.array_equal(K1, K2) and np.array_equal(K1, K3) and np.all(np.isfinite(K1))


# ---- two-operand product -------------------------------------------------------------------------------------------------
def check_atb(ctx, N, PA, PB, mode=0, seed=0):
    A, B, c = kr.int_atb_case(np.random.default_rng(100003 * PA + 1009 * PB + N + seed), N, PA, PB)
    C = ctx.weighted_atb(A, B, c, mode)
    assert_atb_exact(C, kr.exact_atb(A, B, c), kr.describe_atb(N, PA, PB, mode), sliver=kr.is_sliver(PA, PB, mode))
    return A, B, c, C


@pytest.mark.parametrize('PA,PB', kr.ATB_MODE0_SHAPES)
def test_atb_exact_shapes(actx, PA, PB):
    """j. Interior tiles, ragged tiles, 16-blocks skipped on either side (mt_a, mt_b) and the column clamp of the last pair."""
    check_atb(actx, 100, PA, PB)


@pytest.mark.parametrize('stage', [0, 1, 2])
def test_atb_exact_rows_below_three_stages(actx, stage):
    PA, PB = kr.ATB_MODE0_N_SWEEP
    for N in range(16 * stage + 1, 16 * stage + 17):
        check_atb(actx, N, PA, PB)


@pytest.mark.parametrize('N', [255, 257])
def test_atb_exact_rows_around_split_boundaries(actx, N):
    check_atb(actx, N, *kr.ATB_MODE0_N_SWEEP)


@pytest.mark.parametrize('N,PA,PB,splits', kr.ATB_MODE0_SPLIT_CASES)
def test_atb_exact_split_counts(actx, N, PA, PB, splits):
    assert kr.atb_splits(N, PA, PB, 0) == splits
    check_atb(actx, N, PA, PB)


def check_sliver(ctx, N):
    """Mode 1 at 528 x 528 against the exact product, slot by slot, and against mode 0 on the same operands."""
    A, B, c, C1 = check_atb(ctx, N, P528, P528, mode=1)
    C0 = ctx.weighted_atb(A, B, c, 0)
    assert_atb_exact(C0, C1, 'mode 0 against mode 1, N {}'.format(N), sliver=True)


@pytest.mark.parametrize('stage', [0, 1, 2])
def test_sliver_exact_rows_below_three_stages(actx, stage):
    """k. Every N in 1..48: each k-quarter of a ragged last stage holds 0 to 4 live rows."""
    for N in range(16 * stage + 1, 16 * stage + 17):
        check_sliver(actx, N)


@pytest.mark.parametrize('N', kr.SLIVER_N_EXTRA)
def test_sliver_exact_rows(actx, N):
    assert kr.atb_splits(N, P528, P528, 1) == {255: 8, 257: 8, 4101: 16, 32771: 128}[N]
    check_sliver(actx, N)


@pytest.mark.parametrize('N', [257, 4101])
def test_sliver_each_k_quarter_alone(actx, N):
    """k. All weight on rows 4 g .. 4 g + 3 of every 16-row stage: only the workgroups of k-quarter g contribute to the edge
    slots, so each of the four column groups of (bi, 4), the four row groups of (4, bj) and of the corner is seen alone."""
    A, B, c = kr.int_atb_case(np.random.default_rng(77 + N), N, P528, P528)
    for g in range(4):
        cg = np.where((np.arange(N) % 16) // 4 == g, c, 0.0)
        assert_atb_exact(actx.weighted_atb(A, B, cg, 1), kr.exact_atb(A, B, cg), 'k-quarter {} alone, N {}'.format(g, N), sliver=True)


def test_padded_mode_other_widths_is_the_plain_kernel(actx):
    """Mode 1 away from 528 x 528 runs the plain kernel: the same exact result."""
    check_atb(actx, 100, 258, 386, mode=1)
    check_atb(actx, 100, P528, 130, mode=1)


def test_sliver_rounding_bound_and_mode0(actx):
    """k. Real data at 528 x 528: both modes inside their bounds (edge slots of the sliver mode: 3 more additions), hence
    within the sum of the two bounds of each other."""
    N, PA, PB = kr.ATB_REAL_SHAPE
    d = kr.real_atb_reference(N, PA, PB)
    out = {}
    for mode in (0, 1):
        bound = kr.bound_of(kr.atb_K(N, PA, PB, mode), d['Abound'])
        C = actx.weighted_atb(d['A'], d['B'], d['c'], mode)
        (i, j), ratio = kr.worst_entry(C, d['ref'], bound)
        print('atb rounding bound {}: max error / bound {:.4f} at ({}, {}) [{}]'.format(kr.describe_atb(N, PA, PB, mode), ratio, i, j, kr.sliver_slot(i, j)))
        assert ratio <= 1.0, 'mode {}: error / bound {:.3g} at ({}, {}) [{}]'.format(mode, ratio, i, j, kr.sliver_slot(i, j))
        out[mode] = (C, bound)
    diff = np.abs(out[0][0].astype(kr.LD) - out[1][0].astype(kr.LD))
    assert np.all(diff <= out[0][1] + out[1][1])


@pytest.mark.parametrize('N', kr.KRON32_N)
def test_kron32_exact(actx, N):
    """l. Mode 2: the left operand tri([1, x][1, x]^T) generated on chip, against the host-built packed triangle, and bitwise
    mode 1 fed with that explicit operand."""
    x, B, c = kr.int_atb_case(np.random.default_rng(4242 + N), N, 31, P528)
    C2 = actx.weighted_atb(x, B, c, 2)
    assert_atb_exact(C2, kr.exact_atb_kron32(x, B, c), kr.describe_atb(N, 31, P528, 2), sliver=True)
    C1 = actx.weighted_atb(kr.kron_rows(kr.xtilde(x)), B, c, 1)
    assert_atb_exact(C2, C1, 'mode 2 against mode 1 on the explicit operand, N {}'.format(N), sliver=True)


def test_kron32_rounding_bound(actx):
    N = kr.KRON32_REAL_N
    d = kr.real_kron32_reference(N)
    bound = kr.bound_of(kr.atb_K(N, 31, P528, 2), d['Abound'])
    C = actx.weighted_atb(d['x'], d['B'], d['c'], 2)
    (i, j), ratio = kr.worst_entry(C, d['ref'], bound)
    print('kron32 rounding bound {}: max error / bound {:.4f} at ({}, {}) [{}]'.format(kr.describe_atb(N, 31, P528, 2), ratio, i, j, kr.sliver_slot(i, j)))
    assert ratio <= 1.0, 'error / bound {:.3g} at ({}, {}) [{}]'.format(ratio, i, j, kr.sliver_slot(i, j))


def test_atb_buffer_reuse(vb):
    """m. One context runs mode 0 at (258, 386), mode 1, mode 2 and kron_gram, all through `tile_part`; weights with zeros; a
    NaN in one column of B at row 37 stays in that column of C."""
    rng = np.random.default_rng(55)
    N = 300
    Z, cz = kr.int_kron_case(rng, 500, 23)
    ctx = kron_ctx(vb, Z)
    for rnd in range(2):
        A, B, c = kr.int_atb_case(rng, N, 258, 386)
        c[rng.random(N) < 0.3] = 0.0
        assert_atb_exact(ctx.weighted_atb(A, B, c, 0), kr.exact_atb(A, B, c), 'mode 0, round {}'.format(rnd))
        A, B, c = kr.int_atb_case(rng, N, P528, P528)
        c[rng.random(N) < 0.3] = 0.0
        assert_atb_exact(ctx.weighted_atb(A, B, c, 1), kr.exact_atb(A, B, c), 'mode 1, round {}'.format(rnd), sliver=True)
        x = rng.integers(-3, 4, size=(N, 31)).astype(np.float64)
        assert_atb_exact(ctx.weighted_atb(x, B, c, 2), kr.exact_atb_kron32(x, B, c), 'mode 2, round {}'.format(rnd), sliver=True)
        assert_kron_exact(ctx.kron_gram(cz), kr.exact_kron(Z, cz), 23, 'kron_gram, round {}'.format(rnd))
    c = np.where(c == 0.0, 1.0, c)
    for mode, L in ((0, A), (1, A), (2, x)):
        want = kr.exact_atb(kr.kron_rows(kr.xtilde(x)) if mode == 2 else A, B, c)
        for col in (5, 300, 515, 527):
            Bn = B.copy(); Bn[37, col] = np.nan
            C = ctx.weighted_atb(L, Bn, c, mode)
            hit = np.zeros(C.shape, dtype=bool); hit[:, col] = True
            B0 = B.copy(); B0[37, col] = 0.0
            want0 = kr.exact_atb(kr.kron_rows(kr.xtilde(x)) if mode == 2 else A, B0, c)
            assert np.all(np.isnan(C[hit])), 'mode {}: column {} must be NaN'.format(mode, col)
            assert_atb_exact(np.where(hit, 0.0, C), np.where(hit, 0.0, want0), 'mode {}: NaN in B[37, {}] leaked'.format(mode, col), sliver=mode > 0)
    ctx.close()


def test_argument_errors(vb, actx):
    """n. Odd widths, a mode-2 operand that is not N x 31, more than 64 columns for kron_gram: an error code and a message,
    nothing launched."""
    A, B, c = kr.int_atb_case(np.random.default_rng(0), 20, 3, 4)
    with pytest.raises(NotImplementedError, match='even widths'):
        actx.weighted_atb(A, B, c)
    with pytest.raises(NotImplementedError, match='even widths'):
        actx.weighted_atb(B, A, c, 1)
    with pytest.raises(ValueError, match='mode 2'):
        actx.weighted_atb(np.zeros((20, 30)), np.zeros((20, P528)), c, 2)
    with pytest.raises(ValueError, match='mode 2'):
        actx.weighted_atb(np.zeros((20, 31)), np.zeros((20, 130)), c, 2)
    with pytest.raises(ValueError, match='mode must be'):
        actx.weighted_atb(B, B, c, 3)
    Z, _ = kr.int_kron_case(np.random.default_rng(0), 20, 65)
    ctx = kron_ctx(vb, Z)
    with pytest.raises(NotImplementedError, match='n_cols <= 64'):
        ctx.kron_gram()
    ctx.close()
    ctx = vb.DeviceContext(BLOCKS, loss='data_only', n_obs=20, n_cols=8, device=0)
    with pytest.raises(RuntimeError, match='no data matrix'):
        ctx.kron_gram()
    ctx.close()
    check_atb(actx, 20, 4, 4)                        # the context still works

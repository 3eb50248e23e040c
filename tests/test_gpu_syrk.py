"""The tiled weighted SYRK  S = X^T diag(c) X  (csrc/k_wsyrk.hip) entry by entry: the LDS-DMA kernel, the register-staged
kernel with vector and with scalar loads, the split reduction, the shortcut sums r = X^T (c o y) and the tile unpacking.

Two oracles (tests/syrk_reference.py): small-integer data, where the device result must be BITWISE
the int64 matrix product whatever the summation order, and real data against a longdouble reference with the entry-wise
bound (L + S + 2) 2^-53 |X|^T |c| |X|.  A failure names the entry."""
import numpy as np
import pytest

import syrk_reference as sr
from oracle import models as om
from helpers import make_par, on_torch_stream

pytestmark = pytest.mark.gpu

ROUTES = ('dma', 'staged', 'unaligned')
BLOCKS = [dict(kind=0, free_size=3, vec_size=3, dim0=3, dim1=0, lb=-np.inf, ub=np.inf)]


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1, 'no HIP device visible'
    return lrvb_amd


class Gram(object):
    """A data_only context over one (N, P) shape whose X lives in two torch buffers: one 16-byte aligned, one starting at
    element 1 of its allocation (8-byte aligned only).  run(route, n_splits) -> weighted_gram() with
      'dma'        tuning (n_splits, 0), aligned rows: the LDS-DMA kernel at even P > 64, the narrow kernel at P <= 64,
                   the register-staged kernel with scalar loads at odd P
      'staged'     tuning (n_splits, 1): the register-staged kernel, vector loads at even P
      'unaligned'  tuning (n_splits, 0), rows at the odd address: scalar loads whatever P
    The buffers live as long as the object: the context borrows their addresses."""

    def __init__(self, vb, X, c):
        import torch
        self.torch, self.vb = torch, vb
        self.N, self.P = X.shape
        dev = torch.device('cuda', 0)
        self.al = torch.empty(self.N * self.P, dtype=torch.float64, device=dev)
        self.un = torch.empty(self.N * self.P + 1, dtype=torch.float64, device=dev)
        assert self.al.data_ptr() % 16 == 0 and self.un.data_ptr() % 16 == 0
        self.ctx = on_torch_stream(vb.DeviceContext(BLOCKS, loss='data_only', n_obs=self.N, n_cols=self.P, device=0), dev)
        self.set_X(X)
        self.ctx.set_weights(c)

    def set_X(self, X):
        t = self.torch.from_numpy(np.array(X, dtype=np.float64, order='C').ravel()).to(self.al.device)      # a writable copy: the shared references are read-only
        self.al.copy_(t)
        self.un[0] = np.nan                                  # what lies before the matrix must never be read
        self.un[1:].copy_(t)

    def run(self, route, n_splits=0):
        un = route == 'unaligned'
        ptr = self.un.data_ptr() + 8 if un else self.al.data_ptr()
        assert ptr % 16 == (8 if un else 0)
        self.ctx.set_data_dev(self.vb._hip.SLOT_X, ptr, self.N, self.P)
        self.ctx.set_tuning(n_splits, 1 if route == 'staged' else 0)
        S = self.ctx.weighted_gram()
        self.ctx.set_tuning(0, 0)
        return S


def assert_exact(S, want, label):
    """Bitwise equality with the integer reference; a failure names the first wrong entry and its tile."""
    want = np.asarray(want, dtype=np.float64)
    if np.array_equal(S, want):
        return
    bad = np.argwhere(~(S == want))
    i, j = bad[0]
    raise AssertionError('{}: {} of {} entries differ; first ({}, {}) [tile ({}, {}), block ({}, {})]: got {!r}, want {!r}'.format(
        label, len(bad), S.size, i, j, i // 128, j // 128, (i % 128) // 16, (j % 128) // 16, S[i, j], want[i, j]))


def check_all_routes(vb, N, P, n_splits=0, seed=0):
    rng = np.random.default_rng(100003 * P + N + seed)
    X, c, _ = sr.int_case(rng, N, P)
    want = sr.int_gram(X, c)
    g = Gram(vb, X, c)
    for route in ROUTES:
        S = g.run(route, n_splits)
        assert_exact(S, want, 'N {} P {} splits {} route {}'.format(N, P, n_splits, route))
        assert np.array_equal(S, S.T)
    g.ctx.close()


# ---- a. exact sweep over the rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', [0, 1, 2])
def test_exact_rows_below_three_stages(vb, stage):
    """Every N in 1..48 at P = 130: fewer rows than a 16-row stage, and every residue of the ragged last stage as the first,
    second and third stage of its split; all but the first one to three splits empty."""
    for N in range(16 * stage + 1, 16 * stage + 17):
        check_all_routes(vb, N, 130)


@pytest.mark.parametrize('N', [127, 128, 129, 255, 257, 30407, 45605])
def test_exact_rows(vb, N):
    """Around the split boundaries of 8 splits, and the two sizes where the automatic selection leaves 8 splits: 16 at
    N = 30407, 24 (three groups of eight: not a power of two) at N = 45605."""
    assert sr.effective_splits(N, 130) == {30407: 16, 45605: 24}.get(N, 8)
    check_all_routes(vb, N, 130)


# ---- b. exact sweep over the columns ---------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [65, 66, 67, 126, 127, 128, 129, 130, 190, 192, 194, 254, 256, 258, 382, 384, 386, 1024, 1026])
def test_exact_columns(vb, P):
    """Odd and even widths, one to nine tile rows, a last tile with 2 live columns (130, 258, 386, 1026) and with 126."""
    check_all_routes(vb, 100, P)


def test_exact_wide_triangular_decode(vb):
    """P = 2050: 17 tile rows, 153 tiles -- the triangular tile decode far past the 8 tile rows of the headline shape."""
    assert sr.num_tiles(2050) == 153
    check_all_routes(vb, 17, 2050, n_splits=8)


# ---- c. exact sweep over the split count -----------------------------------------------------------------------------
@pytest.mark.parametrize('N,P', sr.SPLIT_SHAPES)
def test_exact_split_counts(vb, N, P):
    """User split counts 1, 5, 8, 20, 64, 128 (rounded to 8, 8, 8, 24, 64, 128) on every route: the split decode, empty
    splits, the rounding and the reduction over more than 8 partials; then the count walks DOWN on the same context, so
    that stale partials of the larger run lie behind the smaller one's."""
    rng = np.random.default_rng(N * P)
    X, c, _ = sr.int_case(rng, N, P)
    want = sr.int_gram(X, c)
    g = Gram(vb, X, c)
    for route in ROUTES:
        for s in sr.SPLIT_COUNTS:
            assert_exact(g.run(route, s), want, 'N {} P {} splits {} route {}'.format(N, P, s, route))
    for route in ROUTES:
        for s in (128, 24, 8):
            assert_exact(g.run(route, s), want, 'N {} P {} splits {} (walking down) route {}'.format(N, P, s, route))
    g.ctx.close()


def test_exact_thousand_splits_one_tile(vb):
    N, P, s = sr.MANY_SPLITS_CASE
    assert sr.effective_splits(N, P, s) == 1008 and sr.num_tiles(P) == 1
    check_all_routes(vb, N, P, n_splits=s)


# ---- d. rows that are 8- but not 16-byte aligned -----------------------------------------------------------------------
@pytest.mark.parametrize('N', [100, 1001])
@pytest.mark.parametrize('P', [22, 64, 130, 256])
def test_unaligned_rows_even_width(vb, N, P):
    """Even P with X at an address that is not a multiple of 16: wsyrk_kernel<false> (P > 64), gram_small_kernel<.,
    ALIGNED16 = false> (P <= 64).  Bitwise the aligned result and the integer reference."""
    rng = np.random.default_rng(31 * P + N)
    X, c, _ = sr.int_case(rng, N, P)
    g = Gram(vb, X, c)
    S_al, S_un = g.run('dma'), g.run('unaligned')
    assert_exact(S_un, sr.int_gram(X, c), 'N {} P {} unaligned'.format(N, P))
    assert np.array_equal(S_un, S_al)
    g.ctx.close()


# ---- e. one context, many calls -----------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', [0, 1])
def test_reuse_of_one_context(vb, flags):
    """The zero padding behind the weight column is written when the buffer is allocated: later calls on the same context
    depend on it still being zero."""
    N, P = 1001, 130
    rng = np.random.default_rng(5 + flags)
    X, c, _ = sr.int_case(rng, N, P)
    ctx = vb.DeviceContext(BLOCKS, loss='data_only', n_obs=N, n_cols=P, device=0)
    ctx.set_tuning(0, flags)
    ctx.set_data(vb._hip.SLOT_X, X)
    ctx.set_weights(c)
    S0 = ctx.weighted_gram()
    assert_exact(S0, sr.int_gram(X, c), 'first call')
    c_half = c.copy(); c_half[0::2] = 0.0
    ctx.set_weights(c_half)
    assert_exact(ctx.weighted_gram(), sr.int_gram(X[1::2], c[1::2]), 'every other row zeroed')
    ctx.set_weights(np.zeros(N))
    assert_exact(ctx.weighted_gram(), np.zeros((P, P)), 'all-zero weights')
    ctx.set_weights(c)
    assert np.array_equal(ctx.weighted_gram(), S0)
    X2, _, _ = sr.int_case(rng, N, P)
    ctx.set_data(vb._hip.SLOT_X, X2)
    assert_exact(ctx.weighted_gram(), sr.int_gram(X2, c), 'new X')
    ctx.close()


@pytest.mark.parametrize('reverse', [False, True])
def test_reuse_across_entry_points(vb, reverse):
    """A Gaussian GLM objective with integer data: gram(), the Hessian and weighted_gram() on ONE context, in this order
    and in the reverse order -- the padded columns cw, cyv and zbuf each serve more than one producer before a SYRK
    depends on their padding.  Hessian minus the diagonal prior = X^T diag(w) X, bitwise."""
    N, P = 1001, 130
    rng = np.random.default_rng(77)
    X, w, y = sr.int_case(rng, N, P)
    theta = rng.integers(-2, 3, size=P).astype(np.float64)
    par, lay = make_par(vb, [('box', 'beta', P, -np.inf, np.inf)])
    fun = vb.GLMObjective(par, X, y, loss='gaussian', lik_info=1.0, prior_info=2.0, weights=w)
    want = sr.int_gram(X, w)
    l1 = X @ theta - y                                                 # l' (integers): G^T G, G[n, :] = l'_n x_n, carries no weights
    want_gram = sr.int_gram(X, l1 * l1)
    assert np.abs(want_gram).max() < 2 ** 53
    steps = ['gram', 'hessian', 'weighted_gram']
    for step in (steps[::-1] if reverse else steps):
        if step == 'gram':
            assert_exact(fun.gram(theta), want_gram, 'gram ({})'.format('reverse' if reverse else 'forward'))
        elif step == 'hessian':
            H = fun.hessian(theta, True)
            assert_exact(H - 2.0 * np.eye(P), want, 'Hessian data term ({})'.format('reverse' if reverse else 'forward'))
        else:
            assert_exact(fun.ctx.weighted_gram(), want, 'weighted_gram ({})'.format('reverse' if reverse else 'forward'))
    fun.ctx.close()


# ---- f. rounding bound, entry by entry ------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,n_splits', sr.BOUND_CASES)
def test_rounding_bound_every_entry(vb, N, P, n_splits):
    d = sr.real_reference(N, P)
    S_eff = sr.effective_splits(N, P, n_splits)
    bound = sr.elementwise_bound(N, S_eff) * d['A']
    g = Gram(vb, d['X'], d['c'])
    low = np.tril_indices(P)
    for route in ('dma', 'staged'):
        S = g.run(route, n_splits)
        (i, j), ratio = sr.worst_entry(np.tril(S), np.tril(d['S_ref']), bound)
        print('rounding bound N {} P {} splits {} route {}: max error / bound {:.4f} at ({}, {})'.format(N, P, S_eff, route, ratio, i, j))
        assert sr.max_ratio(S[low], d['S_ref'][low], bound[low]) <= 1.0, \
            'N {} P {} splits {} route {}: error / bound {:.3g} at entry ({}, {}), tile ({}, {})'.format(
                N, P, S_eff, route, ratio, i, j, i // 128, j // 128)
        assert np.array_equal(S, S.T), 'upper triangle is not the mirror of the lower'
    g.ctx.close()


# ---- g. exact scaling by powers of two ------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P', [(1000, 130), (2000, 1024)])
def test_exact_power_of_two_scaling(vb, N, P):
    """Column j of X times 2^e_j and the weights times 2^7 scale S_ij by exactly 2^(7 + e_i + e_j): every rounding commutes
    with a power of two (|x| in 1e-9 .. 1e10 here, sums below 1e27: nothing overflows or goes subnormal).  Needs no reference;
    an entry that took a term from another column breaks it."""
    d = sr.real_reference(N, P)
    e = np.random.default_rng(N + P).integers(-20, 21, size=P)
    X2, c2 = np.ldexp(d['X'], e[None, :]), d['c'] * 128.0
    assert np.all(np.ldexp(X2, -e[None, :]) == d['X']) and np.abs(X2[X2 != 0]).min() > 1e-100 and np.abs(X2).max() < 1e100
    g1, g2 = Gram(vb, d['X'], d['c']), Gram(vb, X2, c2)
    for route in ('dma', 'staged'):
        S1, S2 = g1.run(route), g2.run(route)
        want = np.ldexp(S1, 7 + e[:, None] + e[None, :])
        assert np.all(np.isfinite(want)) and np.all(np.abs(want[want != 0]) > 1e-200)
        assert_exact(S2, want, 'scaling N {} P {} route {}'.format(N, P, route))
    g1.ctx.close(); g2.ctx.close()


# ---- h. non-finite inputs stay where they belong ---------------------------------------------------------------------
@pytest.mark.parametrize('N,P', [(200, 130), (200, 258)])
def test_nan_containment(vb, N, P):
    """A NaN in X[r, j] (non-zero weight, r < N - 16) makes row and column j of S NaN and changes nothing else: every other
    entry is bitwise what X[r, j] = 0 gives.  A NaN weight makes every entry NaN."""
    rng = np.random.default_rng(N + P)
    X, c, _ = sr.int_case(rng, N, P)
    r = 37
    assert r < N - 16 and c[r] != 0
    g = Gram(vb, X, c)
    for j in (0, 63, 64, 127, 128, P - 1):
        X0 = X.copy(); X0[r, j] = 0.0
        Xn = X.copy(); Xn[r, j] = np.nan
        want = sr.int_gram(X0, c).astype(np.float64)
        hit = np.zeros((P, P), dtype=bool); hit[j, :] = True; hit[:, j] = True
        for route in ('dma', 'staged'):
            g.set_X(X0)
            assert_exact(g.run(route), want, 'X[r, {}] = 0, route {}'.format(j, route))
            g.set_X(Xn)
            S = g.run(route)
            assert np.all(np.isnan(S[hit])), 'route {}: row / column {} must be NaN'.format(route, j)
            assert_exact(np.where(hit, 0.0, S), np.where(hit, 0.0, want), 'NaN at X[r, {}] leaked, route {}'.format(j, route))
    g.set_X(X)
    cn = c.copy(); cn[r] = np.nan
    g.ctx.set_weights(cn)
    for route in ('dma', 'staged'):
        assert np.all(np.isnan(g.run(route))), 'a NaN weight must reach every entry (route {})'.format(route)
    g.ctx.close()


# ---- i. the Gaussian shortcut: r = X^T (c o y) on the diagonal tiles -------------------------------------------------
def gaussian_partial(vb, X, y, w, theta, n_splits):
    """statistics [value | gradient | tiles] of a Gaussian GLM objective (unconstrained box, lik_info = 1, no prior)
    through DeviceEngine.partial, and the profile of that call."""
    import torch
    from lrvb_amd.distributed import DeviceEngine
    P = X.shape[1]
    par, lay = make_par(vb, [('box', 'beta', P, -np.inf, np.inf)])
    fun = vb.GLMObjective(par, X, y, loss='gaussian', lik_info=1.0, weights=w)
    dev = torch.device('cuda', 0)
    th = torch.tensor(theta, device=dev)
    ctx = fun.ctx
    eng = DeviceEngine(ctx, dev)
    out = []
    for s in n_splits:
        ctx.set_tuning(s, 0)
        ctx.profile_enable(True); ctx.profile_reset()
        st = eng.partial(th).cpu().numpy().copy()
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        out.append((st, prof))
    ctx.set_tuning(0, 0)
    ctx.set_stream(None)
    return fun, lay, out


@pytest.mark.parametrize('N,P', [(1, 130), (15, 130), (16, 130), (17, 130), (31, 130), (33, 130), (1000, 130), (1001, 130),
                                 (777, 258), (777, 1024)])
def test_gaussian_shortcut_exact(vb, N, P):
    from lrvb_amd.distributed import unpack_tiles, stats_layout
    rng = np.random.default_rng(977 * P + N)
    X, w, y = sr.int_case(rng, N, P)
    theta = rng.integers(-2, 3, size=P).astype(np.float64)
    fun, lay, runs = gaussian_partial(vb, X, y, w, theta, (0, 24, 128))
    model = om.DeclaredModel(lay, loss=om.GAUSSIAN, x=X, y=y, w=w, lik_info=1.0)
    assert np.array_equal(model.layout.constrain(theta), theta)
    l0, l1, l2 = om.loss_terms(om.GAUSSIAN, y, X @ theta, 1.0)
    want_S = sr.int_gram(X, w)
    want_g = sr.int_xty(X, w, l1)                                   # x.T @ (w * l1), integers
    assert np.array_equal(want_g, X.T @ (w * l1)) and np.array_equal(want_g, want_S @ theta.astype(np.int64) - sr.int_xty(X, w, y))
    twice_value = int(np.sum(w.astype(np.int64) * (X @ theta - y).astype(np.int64) ** 2))       # value = 1/2 sum w (z - y)^2
    assert abs(twice_value) < 2 ** 52 and 0.5 * twice_value == np.sum(w * l0)
    o_val, o_g, o_t, total = stats_layout(P)
    for s, (st, prof) in zip((0, 24, 128), runs):
        label = 'N {} P {} splits {}'.format(N, P, s)
        assert st.size == total
        assert prof['pass_calls'] == 0 and prof['wsyrk_calls'] == 1, label
        assert_exact(unpack_tiles(st[o_t:], P), want_S, label + ' tiles')
        bad = np.flatnonzero(st[o_g:o_t] != want_g)
        assert bad.size == 0, '{}: gradient slot differs in {} columns, first {}: got {!r}, want {!r}'.format(
            label, bad.size, bad[0], st[o_g + bad[0]], want_g[bad[0]])
        assert st[o_val] == 0.5 * twice_value, '{}: value {!r}, want {!r}'.format(label, st[o_val], 0.5 * twice_value)
    fun.ctx.close()


def test_gaussian_shortcut_rounding_bound(vb):
    """Real data at (5003, 258): r = X^T (c o y) recovered as S_dev eta - gradient slot.  Bound: the r form of the
    entry-wise bound (A_j = sum |c_n y_n x_nj|, S + 8 for the eight-group reduction, + 1 for the final subtraction) plus
    (P + 3) 2^-53 |S_dev| |eta| for the device's S eta (P rounded products, fewer than P additions, the subtraction)."""
    from lrvb_amd.distributed import unpack_tiles, stats_layout
    N, P = 5003, 258
    d = sr.real_reference(N, P)
    eta = np.random.default_rng(3).normal(size=P)
    fun, lay, runs = gaussian_partial(vb, d['X'], d['y'], d['c'], eta, (0, 24, 128))
    o_val, o_g, o_t, total = stats_layout(P)
    LD = sr.LD
    for s, (st, prof) in zip((0, 24, 128), runs):
        S_eff = sr.effective_splits(N, P, s)
        assert prof['pass_calls'] == 0
        S_dev = unpack_tiles(st[o_t:], P)
        low = np.tril_indices(P)
        ratio_S = sr.max_ratio(S_dev[low], d['S_ref'][low], (sr.elementwise_bound(N, S_eff) * d['A'])[low])
        r_rec = S_dev.astype(LD) @ eta.astype(LD) - st[o_g:o_t].astype(LD)
        bound = sr.elementwise_bound(N, S_eff, extra=9) * d['A_r'] + (P + 3) * sr.U * 1.01 * (np.abs(S_dev).astype(LD) @ np.abs(eta).astype(LD))
        j, ratio = sr.worst_entry(r_rec, d['r_ref'], bound)
        print('shortcut N {} P {} splits {}: tiles error / bound {:.4f}, r error / bound {:.4f}'.format(N, P, S_eff, ratio_S, ratio))
        assert ratio_S <= 1.0
        assert ratio <= 1.0, 'splits {}: r error / bound {:.3g} at column {}'.format(S_eff, ratio, j[0])
    fun.ctx.close()


# ---- j. repeatability ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P', [(30407, 130), (2000, 1024)])
def test_repeatable_bitwise(vb, N, P):
    """The same call twice on one context and once on a fresh one: bitwise equal S and statistics (no atomics, fixed
    reduction orders)."""
    d = sr.real_reference(N, P)
    g = Gram(vb, d['X'], d['c'])
    S1, S2 = g.run('dma'), g.run('dma')
    T1 = g.run('staged')
    g.ctx.close()
    g = Gram(vb, d['X'], d['c'])
    assert np.array_equal(S1, S2) and np.array_equal(S1, g.run('dma')) and np.array_equal(T1, g.run('staged'))
    g.ctx.close()
    eta = np.random.default_rng(4).normal(size=P)
    fun, _, runs = gaussian_partial(vb, d['X'], d['y'], d['c'], eta, (0, 0))
    fun2, _, runs2 = gaussian_partial(vb, d['X'], d['y'], d['c'], eta, (0,))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][0], runs2[0][0])
    assert np.all(np.isfinite(runs[0][0][:1 + P]))
    fun.ctx.close(); fun2.ctx.close()

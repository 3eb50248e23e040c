"""`group_cov`, `predict` and `ranef_se` of the mixed models with K effects per group on the device (DESIGN.md section 32:
lrvb_glmm_slopes_group_cov, lrvb_glmm_slopes_predict / lrvb_glmm_poisson_predict / lrvb_glmm_binomial_predict) against the blocks of
H^-1 from the dense `fun.hessian(theta)` by `dense_reference.refined_solve`.

Shapes and seeds: those at which tests/test_gpu_glmm_slopes_device_solve.py asserts a positive definite reference Hessian at the
point of `glmm_slopes_reference.problem`; the Poisson, binomial and negative-binomial data of `glmm_poisson_reference` and
`glmm_binomial_reference` give a positive definite reference Hessian at the same seeds (checked on the CPU; smallest eigenvalues
0.28, 0.11, 0.10 at (130, 64, 4, 2) and 0.14, 0.088, 0.067 at (500, 5, 2, 60)).

Two-route rule: with err the largest entry error of a block relative to the block's largest entry (for a
row: the relative error of its variance), err_dev <= 8 err_host + kappa_2(H) D 2^-53, err_host being the `on_device=False` route
against the same reference: 8 for another summation order, the floor for a yardstick that is accidentally tiny."""
import mpmath
import numpy as np
import pytest

import dense_reference as dref
import glmm_binomial_reference as bref
import glmm_poisson_reference as pref
from test_gpu_glmm_binomial import _model as _binomial_model, _nb_model
from test_gpu_glmm_poisson import _model as _poisson_model
from test_gpu_glmm_slopes_device_solve import _model as _logistic_model, _record, _status

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = 2.0 ** -53
#        N,    P, K,  G, seed
SHAPES = [(130, 64, 4, 2, 198),                                          # full width; every group cut by a tile; a 65th row starts a third tile
          (600, 3, 1, 40, 604),                                          # K = 1
          (300, 1, 3, 7, 304),                                           # P = 1; empty last group, whose block is prior-only
          (500, 5, 2, 60, 11440),
          (3001, 7, 3, 23, 3011)]                                        # P not a multiple of 4; 47 tiles
CASES = [('logistic',) + s for s in SHAPES] + [(kind,) + SHAPES[i] for kind in ('poisson', 'binomial', 'negbinomial') for i in (0, 3)]
N_NEW = 70


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _build(vb, kind, N, P, K, G, seed):
    """(fun, free, x, z, gid, offset of the predictions or None, trials or None)."""
    if kind == 'logistic':
        fun, free, (x, _, z, _, gid) = _logistic_model(vb, N, P, K, G, seed)
        return fun, free, x, z, gid, None, None
    if kind == 'poisson':
        x, y, z, w, gid, o, free = pref.problem(N, P, K, G, seed=seed)
        return _poisson_model(vb, x, y, z, w, o, gid, G)[1], free, x, z, gid, o, None
    if kind == 'binomial':
        x, y, z, w, gid, o, mt, free = bref.problem(N, P, K, G, seed=seed)
        return _binomial_model(vb, x, y, z, w, o, mt, gid, G)[1], free, x, z, gid, o, mt
    x, y, z, w, gid, o, phi, free = bref.nb_problem(N, P, K, G, seed=seed, phi='vector')
    return _nb_model(vb, x, y, z, w, o, phi, gid, G)[1], free, x, z, gid, o, None       # the RAW offset; no trials on the response scale


def _new_rows(kind, x, z, N, P, K, G, seed):
    """70 new rows: groups drawn with repeats, some -1, and (G >= 3: the last group is empty) rows of the empty group's index."""
    rng = np.random.default_rng([seed, 32])
    xn = rng.normal(size=(N_NEW, P)) / np.sqrt(P)
    zn = np.concatenate([np.ones((N_NEW, 1)), 0.5 * rng.normal(size=(N_NEW, K - 1))], axis=1)
    gn = rng.integers(0, G, size=N_NEW)
    gn[::9] = -1
    if G >= 3:
        gn[10:15] = G - 1
    new = dict(x=xn, z=zn, groups=gn)
    if kind != 'logistic':
        new['offset'] = 0.3 * rng.normal(size=N_NEW)
    if kind == 'binomial':
        new['trials'] = rng.integers(0, 13, size=N_NEW).astype(np.float64)
    return new


def _moments(x, z, gid, P, K, G):
    """The dense moment vectors c_n (n x D, free coordinates): x on the means of beta, z on e_g -- on e_mu where gid = -1."""
    ng = 2 * P + 4 * K
    C = np.zeros((x.shape[0], ng + 2 * G * K))
    C[:, :P] = x
    for n, g in enumerate(gid):
        C[n, (2 * P if g < 0 else ng + g * K) + np.arange(K)] = z[n]
    return C


_cache = {}


def _case(vb, kind, N, P, K, G, seed):
    """The model and everything the tests of one case share, computed once: the reference H^-1 (longdouble) and both routes."""
    key = (kind, N, P, K, G, seed)
    if key in _cache:
        return _cache[key]
    fun, free, x, z, gid, off, tr = _build(vb, kind, N, P, K, G, seed)
    if G >= 3:
        assert not np.any(gid == G - 1)
    H = fun.hessian(free)
    D = H.shape[0]
    np.linalg.cholesky(H)                                                # positive definite at this seed
    new = _new_rows(kind, x, z, N, P, K, G, seed)
    n0, n1 = 3, N - 2
    Cw, Cn = _moments(x[n0:n1], z[n0:n1], gid[n0:n1], P, K, G), _moments(new['x'], new['z'], new['groups'], P, K, G)
    X = dref.refined_solve(H, np.hstack([np.eye(D), Cw.T, Cn.T]))
    Hinv = X[:, :D]
    var_w = np.einsum('nd,dn->n', Cw.astype(LD), X[:, D:D + Cw.shape[0]])
    var_n = np.einsum('nd,dn->n', Cn.astype(LD), X[:, D + Cw.shape[0]:])
    c = dict(fun=fun, free=free, x=x, z=z, gid=gid, off=off, tr=tr, new=new, H=H, D=D, kappa=float(np.linalg.cond(H)), Hinv=Hinv,
             n0=n0, n1=n1, Cw=Cw, Cn=Cn, var_w=var_w, var_n=var_n)
    c['cov_host'] = fun.group_cov(free, on_device=False)
    c['win_host'] = fun.predict(free, n0=n0, n1=n1, on_device=False)
    c['new_host'] = fun.predict(free, newdata=new, on_device=False)
    c['cov_dev'] = fun.group_cov(free, on_device=True)
    c['win_dev'] = fun.predict(free, n0=n0, n1=n1, on_device=True)
    c['new_dev'] = fun.predict(free, newdata=new, on_device=True)
    _cache[key] = c
    return c


def _block_err(got, want):
    """Largest entry error of every block relative to the block's largest entry, the maximum over the blocks."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    if got.ndim == 2:
        got, want = got[None], want[None]
    return float(max(np.max(np.abs(a - b)) / np.max(np.abs(b)) for a, b in zip(got, want)))


def _ref_blocks(Hinv, P, K, G):
    ng = 2 * P + 4 * K
    ie = ng + np.arange(G * K).reshape(G, K)
    return (Hinv[:P, :P], np.stack([Hinv[np.ix_(ie[g], ie[g])] for g in range(G)]), np.stack([Hinv[:P][:, ie[g]] for g in range(G)]))


@pytest.mark.parametrize('kind,N,P,K,G,seed', CASES)
def test_group_cov_against_the_dense_inverse(vb, kind, N, P, K, G, seed):
    c = _case(vb, kind, N, P, K, G, seed)
    want = _ref_blocks(c['Hinv'], P, K, G)
    floor = c['kappa'] * c['D'] * U53
    for name, dev, host, ref in zip(('cov_beta', 'cov_u', 'cov_beta_u'), c['cov_dev'], c['cov_host'], want):
        assert dev.shape == host.shape == ref.shape
        e_dev, e_host = _block_err(dev, ref), _block_err(host, ref)
        print('%s %s %s: err_dev %.3e, err_host %.3e, kappa D 2^-53 %.3e' % (kind, (N, P, K, G), name, e_dev, e_host, floor))
        assert e_dev <= 8.0 * e_host + floor
    se_lr, se_mf = c['fun'].ranef_se(c['free'], on_device=True)
    assert se_lr.shape == se_mf.shape == (G, K)
    assert np.array_equal(se_lr, np.sqrt(np.diagonal(c['cov_dev'][1], axis1=1, axis2=2)))
    eta_i = np.exp(c['free'][2 * P + 4 * K + G * K:]).reshape(G, K)
    assert np.allclose(se_mf, 1.0 / np.sqrt(eta_i), rtol=1e-14, atol=0)


def _rho_terms(c, rows, P, K, G):
    """Per row the longdouble sums of rho and var_mf and the sums of the absolute values of their terms."""
    fun, free = c['fun'], c['free']
    ng = 2 * P + 4 * K
    m, v = free[:P], 1.0 / np.exp(free[P:2 * P])
    e = np.vstack([free[ng:ng + G * K].reshape(G, K), free[2 * P:2 * P + K][None, :]])
    r = np.vstack([1.0 / np.exp(free[ng + G * K:]).reshape(G, K), 1.0 / np.exp(free[2 * P + K:2 * P + 2 * K])[None, :]])
    x, z, gid, off = rows
    g = np.where(gid < 0, G, gid)
    o = np.zeros(x.shape[0]) if off is None else off
    t_rho = np.concatenate([o[:, None], x * m[None, :], z * e[g]], axis=1).astype(LD)
    t_s = np.concatenate([(x * x).astype(LD) * v[None, :].astype(LD), (z * z).astype(LD) * r[g].astype(LD)], axis=1)
    return t_rho.sum(1), np.abs(t_rho).sum(1), t_s.sum(1), np.abs(t_s).sum(1)


def _gh_mean(kind, rho, s, trials, gh_x, gh_w, mp=False):
    """The response-scale mean by the rule of the kernels: float64 numpy, or mpmath at 40 digits on the same float64 inputs."""
    if not mp:
        if kind in ('poisson', 'negbinomial'):
            return np.exp(rho + 0.5 * s)
        t = rho[:, None] + np.sqrt(np.maximum(s, 0.0))[:, None] * (np.sqrt(2.0) * gh_x)[None, :]
        p = ((1.0 / (1.0 + np.exp(-t))) * (gh_w / np.sqrt(np.pi))[None, :]).sum(1)
        return p if trials is None else trials * p
    mpmath.mp.dps = 40
    out = []
    for i in range(rho.size):
        rh, sv = mpmath.mpf(float(rho[i])), mpmath.mpf(float(s[i]))
        if kind in ('poisson', 'negbinomial'):
            out.append(mpmath.exp(rh + sv / 2))
            continue
        sd = mpmath.sqrt(max(sv, 0))
        p = sum(mpmath.mpf(float(wk)) / (1 + mpmath.exp(-(rh + sd * mpmath.sqrt(2) * mpmath.mpf(float(xk))))) for xk, wk in zip(gh_x, gh_w))
        p = p / mpmath.sqrt(mpmath.pi)
        out.append(p if trials is None else p * mpmath.mpf(float(trials[i])))
    return out


@pytest.mark.parametrize('kind,N,P,K,G,seed', CASES)
def test_predict_window_and_new_rows(vb, kind, N, P, K, G, seed):
    c = _case(vb, kind, N, P, K, G, seed)
    fun, free, n0, n1, new = c['fun'], c['free'], c['n0'], c['n1'], c['new']
    floor = c['kappa'] * c['D'] * U53
    sl = slice(n0, n1)
    win_rows = (c['x'][sl], c['z'][sl], c['gid'][sl], None if c['off'] is None else c['off'][sl])
    new_rows = (new['x'], new['z'], new['groups'], new.get('offset'))
    lr16 = []
    for what, rows, dev, host, want, C, trials in (('window', win_rows, c['win_dev'], c['win_host'], c['var_w'], c['Cw'],
                                                    None if c['tr'] is None else c['tr'][sl]),
                                                   ('new rows', new_rows, c['new_dev'], c['new_host'], c['var_n'], c['Cn'], new.get('trials'))):
        n = rows[0].shape[0]
        assert all(dev[k].shape == (n,) for k in ('rho', 'var_mf', 'var_lrvb', 'mean_mf', 'mean_lrvb'))
        # rho and var_mf against longdouble sums
        rho, a_rho, s_mf, a_s = _rho_terms(c, rows, P, K, G)
        e_rho = np.max(np.abs(dev['rho'].astype(LD) - rho) / a_rho)
        e_s = np.max(np.abs(dev['var_mf'].astype(LD) - s_mf) / a_s)
        print('%s %s %s: rho %.3e, var_mf %.3e of sum |terms|, bound %.3e' % (kind, (N, P, K, G), what, e_rho, e_s, (P + K + 2) * U53))
        assert np.all(np.abs(dev['rho'].astype(LD) - rho) <= (P + K + 2) * U53 * a_rho)
        assert np.all(np.abs(dev['var_mf'].astype(LD) - s_mf) <= (P + K + 2) * U53 * a_s)
        # var_lrvb against c^T H^-1 c, the two-route rule per row
        e_dev = np.abs(dev['var_lrvb'].astype(LD) - want) / want
        e_host = np.abs(host['var_lrvb'].astype(LD) - want) / want
        print('%s %s %s: var_lrvb err_dev %.3e, err_host %.3e (max over rows), floor %.3e' % (kind, (N, P, K, G), what, float(e_dev.max()),
                                                                                         float(e_host.max()), floor))
        assert np.all(want > 0) and np.all(e_dev <= 8.0 * e_host + floor)
        # ... and against the existing public route for 16 of the rows
        pick = np.linspace(0, n - 1, 16).astype(int)
        cov = np.diag(fun.lrvb_cov(free, C[pick]))
        e_cov = np.abs(cov.astype(LD) - want[pick]) / want[pick]
        assert np.all(e_dev[pick] <= 8.0 * e_cov + floor)
        lr16.append(float(e_cov.max()))
        # the response scale: the same rule in float64 numpy on the device's own rho and variances, so that only the quadrature
        # is compared; tolerance 8 x the restatement's own error against mpmath on these inputs, floor 16 * 2^-53 relative
        sub = np.unique(np.concatenate([np.arange(min(n, 64)), pick]))
        tr = None if trials is None else trials[sub]
        for col, var in (('mean_mf', 'var_mf'), ('mean_lrvb', 'var_lrvb')):
            r_in, s_in = dev['rho'][sub], dev[var][sub]
            mine = _gh_mean(kind, r_in, s_in, tr, fun.gh_x, fun.gh_w)
            exact = _gh_mean(kind, r_in, s_in, tr, fun.gh_x, fun.gh_w, mp=True)
            live = np.array([ex != 0 for ex in exact])                   # a binomial row without trials: both are exactly zero
            assert np.array_equal(dev[col][sub][~live], np.zeros(int(np.sum(~live))))
            own = np.array([float(abs(mpmath.mpf(float(a)) - ex) / abs(ex)) for a, ex, ok in zip(mine, exact, live) if ok])
            got = np.array([float(abs(mpmath.mpf(float(a)) - ex) / abs(ex)) for a, ex, ok in zip(dev[col][sub], exact, live) if ok])
            rel = np.abs(dev[col][sub][live] - mine[live]) / np.abs(mine[live])
            print('%s %s %s %s: device vs numpy %.3e, numpy vs mpmath %.3e, device vs mpmath %.3e' % (kind, (N, P, K, G), what, col,
                                                                                               rel.max(), own.max(), got.max()))
            assert np.all(rel <= np.maximum(8.0 * own, 16.0 * U53))
            # every row of the call against the restatement, the bound taken from the rows that went through mpmath
            tol = max(8.0 * float(own.max()), 16.0 * U53)
            all_mine = _gh_mean(kind, dev['rho'], dev[var], trials, fun.gh_x, fun.gh_w)
            nz = all_mine != 0.0
            assert np.array_equal(dev[col][~nz], all_mine[~nz])
            assert np.all(np.abs(dev[col][nz] - all_mine[nz]) <= tol * np.abs(all_mine[nz]))
    print('%s %s: lrvb_cov (host route) against the reference, 16 rows each: %s' % (kind, (N, P, K, G), lr16))


@pytest.mark.parametrize('kind,N,P,K,G,seed', CASES)
def test_bitwise(vb, kind, N, P, K, G, seed):
    c = _case(vb, kind, N, P, K, G, seed)
    fun, free, n0, n1 = c['fun'], c['free'], c['n0'], c['n1']
    cols = ('rho', 'var_mf', 'var_lrvb', 'mean_mf', 'mean_lrvb')
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in cols)
    terms, schur = _record(fun)
    full = fun.predict(free, on_device=True)
    assert same(full, fun.predict(free, on_device=True))                 # two calls
    win = fun.predict(free, n0=n0, n1=n1, on_device=True)
    assert same(win, c['win_dev']) and all(np.array_equal(win[k], full[k][n0:n1]) for k in cols)       # a window is a slice
    sl = slice(7, 7 + 129 if N > 140 else N)
    copy = dict(x=c['x'][sl].copy(), z=c['z'][sl].copy(), groups=c['gid'][sl].copy())
    if c['off'] is not None:
        copy['offset'] = c['off'][sl].copy()
    if c['tr'] is not None:
        copy['trials'] = c['tr'][sl].copy()
    as_new = fun.predict(free, newdata=copy, on_device=True)
    assert all(np.array_equal(as_new[k], full[k][sl]) for k in cols)     # new rows that are the training rows
    cov = fun.group_cov(free, on_device=True)
    assert all(np.array_equal(a, b) for a, b in zip(cov, c['cov_dev']))
    assert terms == [] and schur == []                                   # the factor of the cached point was reused throughout
    fun.value(free)                                                      # drops the factor: everything is rebuilt
    assert same(fun.predict(free, on_device=True), full)
    assert len(schur) == 1 and terms[-1] is False
    assert all(np.array_equal(a, b) for a, b in zip(fun.group_cov(free, on_device=True), cov))
    assert len(schur) == 1


def test_more_tiles_than_workgroups(vb):
    """The launch caps the grid at 2048 workgroups: past 131072 rows a workgroup walks more than one tile.  138000 new rows that
    are the 600 training rows over and over must give the training call's bits, tile after tile."""
    kind, N, P, K, G, seed = CASES[1]
    c = _case(vb, kind, N, P, K, G, seed)
    fun, free = c['fun'], c['free']
    full = fun.predict(free, on_device=True)
    reps = 230
    assert reps * N > 2048 * 64 + 64
    many = fun.predict(free, newdata=dict(x=np.tile(c['x'], (reps, 1)), z=np.tile(c['z'], (reps, 1)), groups=np.tile(c['gid'], reps)),
                       on_device=True)
    for k in ('rho', 'var_mf', 'var_lrvb', 'mean_mf', 'mean_lrvb'):
        assert many[k].shape == (reps * N,) and np.array_equal(many[k], np.tile(full[k], reps))


def test_state_and_refusals(vb):
    hip = vb._hip
    N, P, K, G, seed = SHAPES[2]
    fun, free, (x, y, z, w, gid) = _logistic_model(vb, N, P, K, G, seed)
    ctx, R = fun.ctx, 2 * P + 3 * K
    ng = 2 * P + 4 * K
    m, v = free[:P], 1.0 / np.exp(free[P:2 * P])
    e = np.vstack([free[ng:ng + G * K].reshape(G, K), free[2 * P:2 * P + K][None, :]])
    r = np.ones((G + 1, K))
    pt = (m, v, e, r, fun.gh_x, fun.gh_w, np.eye(P))
    W, s = np.eye(R), np.ones(R)
    new = lambda g: (x[:4].copy(), z[:4].copy(), np.array([0, 1, g, 2]))
    predict = lambda p=pt, **kw: _status(ctx, lambda *a: ctx.glmm_slopes_predict(*a, **kw), *p)
    gcov = lambda g=G, k=K, Wm=W: _status(ctx, ctx.glmm_slopes_group_cov, Wm, s if Wm.shape[0] == R else np.ones(Wm.shape[0]), g, k)
    assert gcov() == hip.ERR_STATE and predict() == hip.ERR_STATE       # nothing resident
    fun.value(free)
    assert gcov() == hip.ERR_STATE                                       # group sums, but no factor
    fun.global_hessian(free, want_host=False)
    assert predict() == hip.ERR_STATE and predict(new=new(1)) == hip.ERR_STATE      # a factor, but no group covariance
    assert gcov(G + 1) == hip.ERR_SIZE and gcov(G - 1) == hip.ERR_SIZE   # wrong G
    R5 = 2 * P + 15
    assert gcov(k=5, Wm=np.eye(R5)) == hip.ERR_UNSUPPORTED
    assert ctx._lib.lrvb_glmm_slopes_group_cov(ctx._h, None, hip.ptr(s), P, G, K, None) == hip.ERR_INVALID
    assert ctx._lib.lrvb_glmm_slopes_group_cov(ctx._h, hip.ptr(W), None, P, G, K, None) == hip.ERR_INVALID
    assert predict() == hip.ERR_STATE
    assert gcov() == hip.OK
    assert predict() == hip.OK and predict(n0=5, n1=5) == hip.OK and predict(new=new(G)) == hip.OK        # G: the pseudo-group
    assert predict((m, v, e[:G], r[:G], fun.gh_x, fun.gh_w, np.eye(P))) == hip.OK                          # without the pseudo-group
    assert predict((m, v, e[:G], r[:G], fun.gh_x, fun.gh_w, np.eye(P)), new=new(G)) == hip.ERR_INVALID     # ... G is then outside
    assert predict(new=new(G + 1)) == hip.ERR_INVALID and predict(new=new(-2)) == hip.ERR_INVALID and predict(new=new(-1)) == hip.ERR_INVALID
    assert predict(n0=4, n1=3) == hip.ERR_INVALID and predict(n1=N + 1) == hip.ERR_INVALID
    wide = (m, v, np.vstack([e, e[:1]]), np.ones((G + 2, K)), fun.gh_x, fun.gh_w, np.eye(P))
    assert predict(wide) == hip.ERR_SIZE and predict((m, v, e[:G - 1], r[:G - 1], fun.gh_x, fun.gh_w, np.eye(P))) == hip.ERR_SIZE
    bad_r = r.copy()
    bad_r[G, 0] = 0.0
    assert predict((m, v, e, bad_r, fun.gh_x, fun.gh_w, np.eye(P))) == hip.ERR_INVALID
    # whatever drops the factor drops the group covariance
    for drop in (lambda: ctx.set_offset(np.zeros(N)), lambda: ctx.set_trials(np.ones(N)), lambda: ctx.set_group_design(z),
                 lambda: fun.value(free), lambda: fun.global_hessian(free, want_host=False)):
        fun.global_hessian(free, want_host=False)
        assert gcov() == hip.OK and predict() == hip.OK
        drop()
        assert predict() == hip.ERR_STATE and predict(new=new(1)) == hip.ERR_STATE
    ctx.set_offset(None)
    ctx.set_trials(None)
    # new weights (the class: lrvb_set_weights itself leaves the resident state alone, the key of the point changes): the factor
    # and the group covariance are rebuilt at the new state
    before = fun.predict(free, n0=0, n1=64, on_device=True)
    terms, schur = _record(fun)
    assert np.array_equal(fun.predict(free, n0=0, n1=64, on_device=True)['var_lrvb'], before['var_lrvb']) and schur == []
    fun.weights_par.set_vector(w * np.linspace(0.8, 1.2, N))
    after = fun.predict(free, n0=0, n1=64, on_device=True)
    assert len(schur) == 1 and not np.array_equal(after['var_lrvb'], before['var_lrvb'])
    assert np.allclose(after['var_lrvb'], fun.predict(free, n0=0, n1=64)['var_lrvb'], rtol=1e-9, atol=0)
    fun.weights_par.set_vector(w)
    del fun._device_terms, fun.ctx.glmm_slopes_schur
    # the class: group indices, coordinates, installed statistics -- before the device is touched
    good = dict(x=x[:4], z=z[:4], groups=np.array([0, -1, 1, 2]))
    out = fun.predict(free, newdata=good, on_device=True)
    assert out['rho'].shape == (4,) and np.all(out['var_lrvb'] > 0)
    terms, schur = _record(fun)
    for g in (G, -2, G + 5):
        with pytest.raises(ValueError):
            fun.predict(free, newdata=dict(good, groups=np.array([0, g, 1, 2])), on_device=True)
        with pytest.raises(ValueError):
            fun.predict(free, newdata=dict(good, groups=np.array([0, g, 1, 2])))
    with pytest.raises(ValueError):
        fun.predict(free, newdata=dict(good, weights=np.ones(4)), on_device=True)
    with pytest.raises(ValueError):
        fun.predict(free, n0=5, n1=N + 1, on_device=True)
    assert terms == [] and schur == []
    with pytest.raises(ValueError):
        fun.group_cov(free, is_free=False, on_device=True)
    with pytest.raises(ValueError):
        fun.predict(free, is_free=False)
    import glmm_slopes_reference as sref
    eta = np.where(sref.positive_mask(P, K, G), np.exp(free), free)
    fun.set_reduced_stats(fun.local_stats(eta), eta)
    with pytest.raises(ValueError):
        fun.group_cov(free, on_device=True)
    with pytest.raises(ValueError):
        fun.predict(free, on_device=True)
    fun.set_reduced_stats(None)
    assert np.all(np.isfinite(fun.predict(free, on_device=True)['mean_lrvb']))

"""`OrdinalGLMMObjective` on the GPU: the OrdinalLik instantiations of the shared tile walk and the threshold pass
glmm_thr_rows_kernel against the torch reference tests/glmm_ordinal_reference.py (torch's logsigmoid and nested autograd in t and in
the thresholds, none of the model's hand forms), the J = 2 identity across models, the shift and the reversal identity, the
zero-variance known answer, category probabilities, the move of one threshold against a fresh model, the grid stride of the threshold
pass, the profile fit, and the state contract with its refusals.

Error measure and bounds are those of tests/test_gpu_glmm_censnormal.py: value 1e-11, gradient 1e-10, Hessian / products / Schur
complement 1e-9 relative; the dense weight cross Hessian 1e-9; LRVB covariance and solves rtol 1e-6 on both routes; `threshold_terms`: g and H_alpha,alpha 1e-11, the cross
Hessian 1e-10, all of the largest magnitude, against autograd in alpha; identities 1e-12 of the largest magnitude.

Shapes (N, P, K, G) and J: (1, 1, 1, 1) J = 3; (37, 3, 1, 5) J = 2 with z=None and offset=None; (65, 5, 2, 3) J = 5 with category 2
empty -- a second tile of one row, a cut group and an empty group; (130, 64, 4, 2) J = 16 -- P, K and the table at their limits;
(300, 17, 4, 7) J = 5 with every fifth weight zero.  Every data set lies inside the grid on which the reference meets its 1e-10 cap
against mpmath and has a reference free Hessian of condition below 1e8 (tests/test_glmm_ordinal_host_math.py; the values are
tabulated in DESIGN.md section 47)."""
import mpmath as mp
import numpy as np
import pytest
import torch

import glmm_ordinal_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _point, _fit
from test_gpu_glmm_binomial import _prior_kw, _check_against_reference, _same
from test_gpu_glmm_ztnegbin import _largest

pytestmark = pytest.mark.gpu

SHAPES = ref.SHAPES
IDENT_SHAPES = [(130, 64, 4, 2), (300, 17, 4, 7)]
IDENT = 1e-12
assert HYP == ref.TEST_HYP


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _model(vb, x, y, z, w, o, alpha, gid, G, hyp=HYP, K=None):
    par = _par(vb, x.shape[1], K if z is None else z.shape[1], G)
    return par, vb.OrdinalGLMMObjective(par, x, y, z, gid, G, alpha, offset=o, weights=w, **_prior_kw(hyp))


_cache = {}


def _case(vb, N, P, K, G):
    key = (N, P, K, G)
    if key not in _cache:
        x, y, z, w, gid, o, alpha, free = ref.shape_data(N, P, K, G)
        bare = key == ref.BARE
        par, fun = _model(vb, x, y, None if bare else z, w, None if bare else o, alpha, gid, G, K=K)
        _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, o=o, alpha=alpha, free=free, eta=_eta(free, P, K, G), par=par, fun=fun,
                           targs=ref.targs(x, y, z, w, o, alpha, gid, G, HYP))
    return _cache[key]


def _fresh(vb, c, G, **kw):
    d = dict(c, **kw)
    return _model(vb, d['x'], d['y'], d['z'], d['w'], d['o'], d['alpha'], d['gid'], G)[1]


def _gh(fun):
    return fun.gh_x, fun.gh_w


def _thr_errs(got, want):
    return [_largest(got['g'], want[0]), _largest(got['H'], want[1]), rel_err(got['cross'], want[2])]


# ---- A: the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G):
    c = _case(vb, N, P, K, G)
    y, w, gid, fun = c['y'], c['w'], c['gid'], c['fun']
    J = ref.J_OF[(N, P, K, G)]
    assert fun.n_categories == J and fun.log_norm_const() == 0.0
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2     # an empty group, one with more than half the rows
    if N == 300:
        assert np.sum(w == 0.0) == 60
    if N == 65:
        assert not np.any(y == 2) and np.any(y == 3)                      # an empty category
    _, Hf = _check_against_reference(c['par'], fun, ref.kl_vec, ref.kl_free, c['targs'], c['free'], G, K, solves=True)
    ev = np.linalg.eigvalsh(Hf)
    print('reference free Hessian', (N, P, K, G), 'J', J, 'smallest eigenvalue', float(ev[0]), 'condition {:.1e}'.format(float(ev[-1] / ev[0])))
    assert ev[0] > 0 and ev[-1] / ev[0] < 1e8
    other = _fresh(vb, c, G)
    pt = _point(c['eta'], P, K, G) + _gh(other)
    assert _same(other.ctx.glmm_ordinal_terms(*pt), other.ctx.glmm_ordinal_terms(*pt))     # two evaluations, equal bits


@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_threshold_terms_against_the_reference_autograd(vb, N, P, K, G):
    """g and the tridiagonal H at 1e-11, the cross Hessian at 1e-10; two calls give equal bits; the entry leaves the resident sums
    alone; the free coordinates of the thresholds are the chain rule with the second-order term of the exponential."""
    c = _case(vb, N, P, K, G)
    fun = _fresh(vb, c, G)
    got = fun.threshold_terms(c['free'])
    want = ref.threshold_terms(c['free'], c['targs'])
    errs = _thr_errs(got, want)
    print('threshold terms against autograd', (N, P, K, G), 'g, H, cross', errs, 'bounds 1e-11 1e-11 1e-10')
    assert errs[0] <= 1e-11 and errs[1] <= 1e-11 and errs[2] <= 1e-10
    T = c['alpha'].size
    assert got['H'].shape == (T, T) and np.all(np.triu(got['H'], 2) == 0.0) and got['cross'].shape == (c['free'].size, T)
    if N == 65:
        assert got['H'][1, 2] == 0.0                                     # category 2 is empty: an exact zero, not a small number
    again = fun.threshold_terms(c['free'])
    assert all(np.array_equal(got[k], again[k]) for k in got)
    pt = _point(c['eta'], P, K, G) + _gh(fun)
    before = fun.ctx.glmm_ordinal_terms(*pt)
    R = np.eye(c['free'].size)[:, :2]
    sol = fun.solve(c['free'], R, on_device=True)
    fun.threshold_terms(c['free'])
    assert fun._dev_factor_key is not None and np.array_equal(fun.solve(c['free'], R, on_device=True), sol)
    assert _same(fun.ctx.glmm_ordinal_terms(*pt), before)
    assert np.array_equal(fun.hyper_grad(fun.threshold_par, c['free'], True), got['g'])
    assert np.array_equal(fun.cross_hessian(fun.threshold_par, c['free'], True), got['cross'])
    for refuse in (fun.global_cross_hessian, fun.global_sensitivity):
        with pytest.raises(NotImplementedError, match='local rows'):
            refuse(fun.threshold_par, c['free'])
    fr = fun.threshold_terms(c['free'], free_thresholds=True)
    A = np.zeros((T, T))
    A[:, 0] = 1.0
    for i in range(1, T):
        A[i:, i] = c['alpha'][i] - c['alpha'][i - 1]
    Hf = A.T @ want[1] @ A
    for i in range(1, T):
        Hf[i, i] += (c['alpha'][i] - c['alpha'][i - 1]) * want[0][i:].sum()
    e = [_largest(fr['g'], A.T @ want[0]), _largest(fr['H'], Hf), rel_err(fr['cross'], want[2] @ A)]
    print('in the free coordinates of the thresholds', e)
    assert e[0] <= 1e-11 and e[1] <= 1e-11 and e[2] <= 1e-10


@pytest.mark.parametrize('N,P,K,G', [(37, 3, 1, 5), (65, 5, 2, 3)])
def test_dense_weight_cross_hessian_against_autograd(vb, N, P, K, G):
    """`cross_hessian(weights_par)`, the host path through `_row_psi_derivs` (a1' whole: no response is subtracted), against autograd
    in the weights: 1e-9, the bound of the siblings' dense cross Hessian."""
    c = _case(vb, N, P, K, G)
    fun = c['fun']
    got = fun.cross_hessian(fun.weights_par, c['free'], True)
    want = ref.weight_cross(c['free'], c['targs'])
    print('dense weight cross Hessian', (N, P, K, G), rel_err(got, want))
    assert got.shape == (c['free'].size, N) and rel_err(got, want) <= 1e-9


# ---- B: identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_two_categories_are_the_logistic_model(vb, N, P, K, G):
    """J = 2: the binomial logit model with offset o - alpha_1 and response 1[y = 1], on value, gradient, the three H blocks, every
    group-sum column, the influence rows and the group influence, at the point and with every variance times 30."""
    c = _case(vb, N, P, K, G)
    x, z, w, gid, o = (c[k] for k in ('x', 'z', 'w', 'gid', 'o'))
    y2 = (c['y'] > (c['alpha'].size // 2)).astype(np.int64)
    a1 = np.array([0.4375])
    A = _model(vb, x, y2, z, w, o, a1, gid, G)[1]
    B = vb.BinomialGLMMObjective(_par(vb, P, K, G), x, y2.astype(np.float64), z, gid, G, offset=o - a1[0], weights=w, **_prior_kw(HYP))
    m, v, e, rr = _point(c['eta'], P, K, G)
    gh = _gh(A)
    Aop = np.random.default_rng(N).normal(size=(5, 2 * P + 2 * G * K))
    assert 0 < y2.sum() < N
    for widen in (1.0, 30.0):
        pt = (m, v * widen, e, rr * widen)
        ta, tb = A.ctx.glmm_ordinal_terms(*pt, *gh), B.ctx.glmm_binomial_terms(*pt, *gh)
        errs = [abs(tb[0] - ta[0]) / abs(ta[0])] + [_largest(ta[i], tb[i]) for i in (1, 2, 3)]
        ra, rb = A.ctx.glmm_ordinal_obs_influence(*pt, *gh, Aop), B.ctx.glmm_binomial_obs_influence(*pt, *gh, Aop)
        ga, gb = A.ctx.glmm_ordinal_group_influence(*pt, *gh, Aop), B.ctx.glmm_binomial_group_influence(*pt, *gh, Aop)
        errs += [_largest(ra, rb), _largest(ga, gb)]
        print('J = 2 against the logistic model', (N, P, K, G), 'variances x', widen, errs)
        assert max(errs) <= IDENT
        assert ta[3].shape == (G, 2 * K + K * (2 * K + 1) + 4 * K * P) and np.any(ta[2][1] != 0.0)
    assert A.fit_thresholds(lambda f, start: start, c['free'])['iterations'] == 0     # alpha_1 fixed: nothing to estimate


@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_shift_identity(vb, N, P, K, G):
    """(alpha + c, o + c) for c = 37.5 and -1e6 (alpha and o are multiples of 2^-20, so the shifted values are exact): value,
    gradient, H blocks, group sums and threshold terms."""
    c = _case(vb, N, P, K, G)
    A = _fresh(vb, c, G)
    pt = _point(c['eta'], P, K, G) + _gh(A)
    ta, ha = A.ctx.glmm_ordinal_terms(*pt), A.ctx.glmm_ordinal_threshold_terms(*pt)
    for shift in (37.5, -1e6):
        al, os_ = c['alpha'] + shift, c['o'] + shift
        assert np.array_equal(al - shift, c['alpha']) and np.array_equal(os_ - shift, c['o'])
        S = _fresh(vb, c, G, alpha=al, o=os_)
        ts, hs = S.ctx.glmm_ordinal_terms(*pt), S.ctx.glmm_ordinal_threshold_terms(*pt)
        errs = [abs(ts[0] - ta[0]) / abs(ta[0])] + [_largest(ta[i], ts[i]) for i in (1, 2, 3)]
        d = [_largest(p, q) for p, q in zip(ha, hs) if p.size]
        print('shift identity', (N, P, K, G), shift, errs, d)
        assert max(errs + d) <= IDENT


@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_reversal_identity(vb, N, P, K, G):
    """y -> J - 1 - y, alpha -> -reverse(alpha) and t -> -t: t - hi and lo - t change places.  t is negated in two ways.  With
    (x, z, o) -> -(x, z, o) at the SAME point every sum is equal (a1 and x change sign together).  With o -> -o and the point's means
    negated (x and z kept) the value and the even blocks are equal, the mean gradients and the odd block are negated, and the
    threshold gradient is reversed and negated.  (Negating the design AND the means would leave t = -o + x m + z e, no reversal.)"""
    c = _case(vb, N, P, K, G)
    A = _fresh(vb, c, G)
    T = c['alpha'].size
    m, v, e, rr = _point(c['eta'], P, K, G)
    gh = _gh(A)
    ta = A.ctx.glmm_ordinal_terms(m, v, e, rr, *gh)
    D = _fresh(vb, c, G, x=-c['x'], z=-c['z'], o=-c['o'], y=T - c['y'], alpha=-c['alpha'][::-1])
    td = D.ctx.glmm_ordinal_terms(m, v, e, rr, *gh)
    errs = [abs(td[0] - ta[0]) / abs(ta[0])] + [_largest(ta[i], td[i]) for i in (1, 2, 3)]
    print('reversal identity, design negated', (N, P, K, G), errs)
    assert max(errs) <= IDENT
    R = _fresh(vb, c, G, o=-c['o'], y=T - c['y'], alpha=-c['alpha'][::-1])
    tr = R.ctx.glmm_ordinal_terms(-m, v, -e, rr, *gh)
    sg = np.concatenate([-np.ones(P), np.ones(P)])
    errs = [abs(tr[0] - ta[0]) / abs(ta[0]), _largest(ta[1], sg * tr[1]), _largest(ta[2][0], tr[2][0]), _largest(ta[2][2], tr[2][2]),
            _largest(ta[2][1], -tr[2][1]), _largest(ta[3][:, :K], -tr[3][:, :K]), _largest(ta[3][:, K:2 * K], tr[3][:, K:2 * K])]
    ha, hr = A.ctx.glmm_ordinal_threshold_terms(m, v, e, rr, *gh), R.ctx.glmm_ordinal_threshold_terms(-m, v, -e, rr, *gh)
    errs += [_largest(ha[0], -hr[0][::-1]), _largest(ha[1], hr[1][::-1]), _largest(ha[2], hr[2][::-1]),
             _largest(ha[3][:, :P], hr[3][::-1, :P]), _largest(ha[3][:, P:], -hr[3][::-1, P:])]
    print('reversal identity', (N, P, K, G), errs)
    assert max(errs) <= IDENT


@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (300, 17, 4, 7)])
def test_zero_variance_known_answer(vb, N, P, K, G):
    """At vanishing variances t = rho: value - (prior and entropy terms of the reference) = -sum w log(sigma(hi - rho) - sigma(lo - rho))
    from mpmath at 40 digits."""
    c = _case(vb, N, P, K, G)
    eta = c['eta'].copy()
    ng, GK = 2 * P + 4 * K, G * K
    eta[P:2 * P] = 1e30
    eta[ng + GK:] = 1e30
    fun = _fresh(vb, c, G)
    t = c['targs']
    priors = float(ref._priors(torch.tensor(eta), t[0], t[2], t[3], t[6], G, t[8]))
    m, v, e, rr = _point(eta, P, K, G)
    rho = c['o'] + c['x'] @ m + np.sum(c['z'] * e[c['gid']], axis=1)
    tab = np.concatenate([[-np.inf], c['alpha'], [np.inf]])
    with mp.workdps(40):
        sig = lambda a: mp.mpf(1) if a == mp.inf else (mp.mpf(0) if a == -mp.inf else 1 / (1 + mp.exp(-a)))
        want = float(sum(-mp.mpf(float(wi)) * mp.log(sig(mp.mpf(float(tab[yi + 1])) - mp.mpf(float(r))) - sig(mp.mpf(float(tab[yi])) - mp.mpf(float(r))))
                         for wi, yi, r in zip(c['w'], c['y'], rho)))
    got = fun.value(eta, False) - priors
    print('zero variance', (N, P, K, G), got, want, abs(got - want) / abs(want))
    assert abs(got - want) <= IDENT * abs(want)


# ---- C: predictions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (130, 64, 4, 2)])
def test_category_probabilities_window_and_new_rows(vb, N, P, K, G):
    """Both routes, a window no tile boundary aligns with and new rows with group -1: the rows of prob_* sum to 1 within 1e-14 and
    equal the host form; the device route agrees with the host route; the resident state is not disturbed."""
    from lrvb_amd.glmm_ordinal import ordinal_category_probs
    c = _case(vb, N, P, K, G)
    fun, free = c['fun'], c['free']
    T = c['alpha'].size
    rng = np.random.default_rng(N)
    n_new = 9
    new = dict(x=rng.normal(size=(n_new, P)) / np.sqrt(P), z=np.concatenate([np.ones((n_new, 1)), 0.5 * rng.normal(size=(n_new, K - 1))], axis=1),
               groups=np.array([0, -1, 1, 0, -1, 1, 0, 0, -1]), offset=0.3 * rng.normal(size=n_new))
    R = np.eye(free.size)[:, :2]
    sol = fun.solve(free, R, on_device=True)
    for kw in (dict(n0=3, n1=N - 2), dict(newdata=new)):
        host, dev = fun.predict(free, **kw), fun.predict(free, on_device=True, **kw)
        n = n_new if 'newdata' in kw else N - 5
        for p in (host, dev):
            assert p['cumprob_mf'].shape == (n, T) and p['prob_lrvb'].shape == (n, T + 1)
            for var, key in (('var_mf', 'mf'), ('var_lrvb', 'lrvb')):
                assert np.max(np.abs(p['prob_' + key].sum(1) - 1.0)) <= 1e-14
                cum, prob = ordinal_category_probs(p['rho'], p[var], c['alpha'], *_gh(fun))
                assert np.max(np.abs(cum - p['cumprob_' + key])) <= 1e-13 and np.max(np.abs(prob - p['prob_' + key])) <= 1e-13
        assert np.allclose(host['rho'], dev['rho'], rtol=1e-12, atol=1e-13) and np.allclose(host['var_lrvb'], dev['var_lrvb'], rtol=1e-6)
        assert np.allclose(host['prob_lrvb'], dev['prob_lrvb'], rtol=1e-6, atol=1e-12) and np.all(dev['var_lrvb'] > 0)
    assert np.array_equal(fun.solve(free, R, on_device=True), sol)
    for key, val in (('trials', np.ones(n_new)), ('thresholds', c['alpha'])):
        with pytest.raises(ValueError, match='got {}'.format(key)):
            fun.predict(free, newdata=dict(new, **{key: val}))


# ---- D: the thresholds as a hyper-parameter ------------------------------------------------------------------------------------
def _everything(fun, free):
    t = fun.threshold_terms(free)
    return [np.array([fun.value(free)]), fun.grad(free), fun.hessian(free), t['g'], t['H'], t['cross']]


def test_moving_one_threshold_is_a_fresh_model(vb):
    """One model built at alpha whose alpha_2 is moved through `threshold_par`, against a second model built fresh at the moved
    thresholds: equal bits; back at alpha the first values return bitwise; a vector that does not increase is refused."""
    N, P, K, G = 65, 5, 2, 3
    c = _case(vb, N, P, K, G)
    free = c['free']
    A = _fresh(vb, c, G)
    base = _everything(A, free)
    A.solve(free, np.eye(free.size)[:, :1], on_device=True)
    assert A._dev_factor_key is not None
    moved = c['alpha'].copy()
    moved[1] += 0.15625
    A.threshold_par.set_vector(moved)
    got = _everything(A, free)
    assert A._dev_factor_key is None and not np.array_equal(got[0], base[0]) and np.array_equal(A.thresholds, moved)
    want = _everything(_fresh(vb, c, G, alpha=moved), free)
    assert all(np.array_equal(p, q) for p, q in zip(got, want))
    A.threshold_par.set_vector(c['alpha'])
    assert all(np.array_equal(p, q) for p, q in zip(_everything(A, free), base))
    bad = c['alpha'].copy()
    bad[2] = bad[1]
    A.threshold_par.set_vector(bad)
    for _ in range(2):                                                   # refused every time, not only at the first evaluation
        with pytest.raises(ValueError, match='strictly increasing'):
            A.value(free)
        with pytest.raises(ValueError, match='strictly increasing'):
            A.threshold_terms(free)
    A.threshold_par.set_vector(c['alpha'])
    assert all(np.array_equal(p, q) for p, q in zip(_everything(A, free), base))


def test_grid_stride_of_the_threshold_pass(vb):
    """N = 2048 * 64 + 65: workgroups take a second tile and the last tile is ragged.  The value and `threshold_terms` against the
    reference at the bounds of the module docstring."""
    N, P, K, G, J = 2048 * 64 + 65, 2, 1, 3, 3
    x, y, z, w, gid, o, alpha, free = ref.problem(N, P, K, G, 11, J, empty_group=False)
    assert ref.inside_grid(*ref.rows_at(free, x, y, z, o, alpha, gid, G))     # the reference holds its cap at every row of this data set too
    par, fun = _model(vb, x, y, z, w, o, alpha, gid, G)
    t = ref.targs(x, y, z, w, o, alpha, gid, G, HYP)
    val = float(ref.kl_free(torch.tensor(free), *t))
    got = fun.threshold_terms(free)
    errs = [abs(fun.value(free) - val) / abs(val)] + _thr_errs(got, ref.threshold_terms(free, t))
    print('grid stride', N, 'value, g, H, cross', errs)
    assert errs[0] <= 1e-11 and errs[1] <= 1e-11 and errs[2] <= 1e-11 and errs[3] <= 1e-10
    again = fun.threshold_terms(free)
    assert all(np.array_equal(got[k], again[k]) for k in got)


FIT_SHAPE, ALPHA_TRUE, BETA_TRUE = (2000, 3, 1, 40), np.array([0.0, 0.9, 2.1]), np.array([0.8, -0.7, 0.4])


def _simulate(seed=3):
    N, P, K, G = FIT_SHAPE
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P))
    gid = rng.integers(0, G, size=N).astype(np.int32)
    t = 0.6 + x @ BETA_TRUE + (0.7 * rng.normal(size=(G, K)))[gid, 0]
    y = np.searchsorted(ALPHA_TRUE, t + rng.logistic(size=N)).astype(np.int64)
    return x, y, np.ones((N, 1)), np.ones(N), gid, np.zeros(N)


def test_fit_thresholds_and_threshold_sensitivity_against_refits(vb):
    """Simulated data (J = 4), the model started from thresholds (0, 1, 2).  Refits at alpha_2 +- 0.05: the moments of beta and mu
    predicted by `threshold_sensitivity` (both routes) and by `ParametricSensitivityLinearApproximation` with `threshold_par` agree
    with the refit differences within 5 % of the largest change.  Then `fit_thresholds` (alpha_1 held at 0) ends with every spacing
    inside [half, twice] the true one."""
    N, P, K, G = FIT_SHAPE
    x, y, z, w, gid, o = _simulate()
    assert np.unique(y).size == 4
    start = np.array([0.0, 1.0, 2.0])
    par, fun = _model(vb, x, y, z, w, o, start, gid, G)
    objective = vb.Objective(par, fun)
    D = 2 * P + 4 * K + 2 * G * K
    th = _fit(vb, objective, np.zeros(D))
    assert ref.inside_grid(*ref.rows_at(th, x, y, z, o, start, gid, G))       # the fitted point lies where the reference holds its cap
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, ref.targs(x, y, z, w, o, start, gid, G, HYP))
    print('reference gradient at the fit', np.max(np.abs(g_ad)))
    assert np.max(np.abs(g_ad)) < 1e-6 and np.min(np.linalg.eigvalsh(H_ad)) > 0      # stationary by the REFERENCE gradient
    idx = np.concatenate([np.arange(P), 2 * P + np.arange(K)])
    M = np.eye(D)[idx]
    pred = [fun.threshold_sensitivity(th, M, on_device=dev)[:, 1] for dev in (False, True)]
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.threshold_par, th, start)
    pred.append((M @ lin.get_dinput_dhyper())[:, 1])
    h = 0.05
    dth = fun.threshold_sensitivity(th)[:, 1]
    fun.threshold_par.set_vector(start + np.array([0.0, h, 0.0]))
    th_p = _fit(vb, objective, th + h * dth)
    fun.threshold_par.set_vector(start - np.array([0.0, h, 0.0]))
    th_m = _fit(vb, objective, th - h * dth)
    fun.threshold_par.set_vector(start)
    diff = 0.5 * (th_p - th_m)[idx]
    for p in pred:
        print('predicted against refit', np.max(np.abs(p * h - diff)), 'largest change', np.max(np.abs(diff)))
        assert np.max(np.abs(p * h - diff)) < 0.05 * np.max(np.abs(diff)) + 1e-8
    out = fun.fit_thresholds(lambda f, s: _fit(vb, objective, s), th)
    print('fit_thresholds', out['thresholds'], 'iterations', out['iterations'], 'slope', out['slope'], 'beta', out['theta'][:P])
    sp, true = np.diff(out['thresholds']), np.diff(ALPHA_TRUE)
    assert out['thresholds'][0] == 0.0 and out['iterations'] <= 20 and np.all(np.linalg.eigvalsh(out['curvature']) > 0)
    assert np.all(sp >= 0.5 * true) and np.all(sp <= 2.0 * true)
    assert ref.inside_grid(*ref.rows_at(out['theta'], x, y, z, o, out['thresholds'], gid, G))
    slope, S = fun.threshold_profile(out['theta'])
    assert np.max(np.abs(slope)) <= 1e-6 * (np.max(np.abs(S)) + 1.0)


# ---- E: state and refusals -----------------------------------------------------------------------------------------------------
def test_state_and_refusals_by_error_code_and_text(vb):
    hip = vb._hip
    rng = np.random.default_rng(47)
    gh = np.polynomial.hermite.hermgauss(20)
    N, G, K, T = 20, 3, 2, 3

    def context(P, y=None, thresholds=(-0.5, 0.25, 1.0)):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)) / np.sqrt(P))
        ctx.set_data(hip.SLOT_Y, (np.arange(N) % (T + 1)).astype(np.float64) if y is None else y)
        if thresholds is not None:
            ctx.set_thresholds(np.array(thresholds))
        return ctx

    def call(ctx, P, K, kind, nq=20):
        Kc = min(max(K, 1), 5)
        m, v, e, rr = np.zeros(P), np.ones(P), np.zeros(G * Kc), np.ones(G * Kc)
        gx, gw = np.zeros(max(nq, 20)), np.ones(max(nq, 20))
        gx[:20], gw[:20] = gh
        head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, K, gx.ctypes.data, gw.ctypes.data, nq)
        lib = ctx._lib
        if kind == 'terms':
            val = np.empty(1)
            return lib.lrvb_glmm_ordinal_terms(*head, val.ctypes.data, None, None, None, 0)
        if kind == 'thr':
            g, hd, ho, cg, cl = np.empty(15), np.empty(15), np.empty(15), np.empty((15, 2 * P)), np.empty((G, 15, 2 * Kc))
            return lib.lrvb_glmm_ordinal_threshold_terms(*head, g.ctypes.data, hd.ctypes.data, ho.ctypes.data, cg.ctypes.data, cl.ctypes.data)
        Q = 2
        Ag, Al = np.ones((Q, 2 * P)), np.ones((G, 2 * Kc, Q))
        out = np.empty((5 * N, Q))
        if kind == 'group':
            return lib.lrvb_glmm_ordinal_group_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, out.ctypes.data)
        return lib.lrvb_glmm_ordinal_obs_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, 0, N, out.ctypes.data)

    gid = np.arange(N) % G
    for kind in ('terms', 'rows', 'group', 'thr'):
        assert call(context(65), 65, K, kind) == hip.ERR_UNSUPPORTED       # P = 65
        ctx = context(3, thresholds=None)
        ctx.set_groups(gid, G)
        ctx.set_group_design(np.ones((N, K)))
        assert call(ctx, 3, 5, kind) == hip.ERR_UNSUPPORTED                # K = 5
        assert call(ctx, 3, 0, kind) == hip.ERR_UNSUPPORTED                # K = 0
        assert call(ctx, 3, K, kind, nq=129) == hip.ERR_UNSUPPORTED        # more than 128 nodes
        assert call(ctx, 3, K, kind) == hip.ERR_STATE                      # no thresholds
        ctx.set_thresholds(np.array([-0.5, 0.25, 1.0]))
        assert call(ctx, 3, K, kind) == hip.OK
    pt = (np.zeros(3), np.ones(3), np.zeros((G, K)), np.ones((G, K))) + tuple(gh)
    none = context(3, thresholds=None)
    none.set_groups(gid, G)
    none.set_group_design(np.ones((N, K)))
    with pytest.raises(RuntimeError, match='no thresholds: call lrvb_set_thresholds first'):
        none.glmm_ordinal_terms(*pt)
    # the setter: refused with the state kept
    base = ctx.glmm_ordinal_terms(*pt)
    lib = ctx._lib
    for bad, text in (([0.0, 0.0, 1.0], 'must increase strictly'), ([0.0, 1.0, 0.5], 'must increase strictly'), ([0.0, np.nan, 1.0], 'not finite'),
                      ([0.0, np.inf], 'not finite'), ([], '1 to 15 thresholds'), (list(range(16)), '1 to 15 thresholds')):
        a = np.array(bad, dtype=np.float64)
        assert lib.lrvb_set_thresholds(ctx._h, a.ctypes.data if a.size else np.zeros(1).ctypes.data, a.size) == hip.ERR_INVALID
        with pytest.raises(ValueError, match=text):
            ctx.set_thresholds(a) if a.size else hip.check(lib.lrvb_set_thresholds(ctx._h, np.zeros(1).ctypes.data, 0))
        assert _same(ctx.glmm_ordinal_terms(*pt), base)
    # a category outside 0 .. T: refused by every entry, and nothing of the earlier state is lost
    for bad in (float(T + 1), -1.0, 1.5, np.nan):
        y = (np.arange(N) % (T + 1)).astype(np.float64)
        y[7] = bad
        wrong = context(3, y=y)
        wrong.set_groups(gid, G)
        wrong.set_group_design(np.ones((N, K)))
        for kind in ('terms', 'rows', 'group', 'thr'):
            assert call(wrong, 3, K, kind) == hip.ERR_INVALID
        with pytest.raises(ValueError, match=r'y\[7\] is .*: with 3 thresholds the categories are the integers 0 \.\. 3'):
            wrong.glmm_ordinal_terms(*pt)
    # fewer thresholds than the data has categories is found when an entry runs
    ctx.set_thresholds(np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match='with 2 thresholds the categories are the integers 0 .. 2'):
        ctx.glmm_ordinal_terms(*pt)
    ctx.set_thresholds(np.array([-0.5, 0.25, 1.0]))
    assert _same(ctx.glmm_ordinal_terms(*pt), base)
    # a point at which a sum is not finite: refused, no sums left resident, the earlier bits on the next call
    one = context(1)
    one.set_groups(gid, G)
    one.set_group_design(np.ones((N, K)))
    good = (np.array([0.3]), np.ones(1), np.zeros((G, K)), np.ones((G, K))) + tuple(gh)
    first = one.glmm_ordinal_terms(*good)
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 + 3 * K, 2 + 3 * K))
    schur = lambda: one._lib.lrvb_glmm_slopes_schur(one._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    assert schur() == hip.OK
    for m in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match='ordinal data term is not finite'):
            one.glmm_ordinal_terms(np.array([m]), *good[1:])
        assert schur() == hip.ERR_STATE                                  # no sums left resident
        if np.isnan(m):                                                  # sigma and its derivatives are bounded: only a NaN reaches these sums
            with pytest.raises(ValueError, match='threshold derivative of the ordinal data term is not finite'):
                one.glmm_ordinal_threshold_terms(np.array([m]), *good[1:])
        assert _same(one.glmm_ordinal_terms(*good), first)
    # a finite point is never refused: softplus(1e200) = 1e200, and every derivative of it is bounded
    for m in (1e200, -1e200):
        big = one.glmm_ordinal_terms(np.array([m]), *good[1:])
        assert np.isfinite(big[0]) and big[0] > 1e198 and np.all(np.isfinite(big[1])) and np.all(np.isfinite(big[2]))
    assert _same(one.glmm_ordinal_terms(*good), first)
    assert hip.load().lrvb_version() == 1
    # the constructor
    x, z = np.ones((N, 2)), np.ones((N, K))
    yy = np.arange(N) % 4
    for bad, text in ((np.where(np.arange(N) == 5, 4, yy), 'y must lie in 0 .. 3'), (np.where(np.arange(N) == 5, -1, yy), 'y must lie in 0 .. 3'),
                      (np.where(np.arange(N) == 5, 1.5, yy), 'integer categories')):
        with pytest.raises(ValueError, match=text):
            vb.OrdinalGLMMObjective(_par(vb, 2, K, G), x, bad, z, gid, G, [-0.5, 0.25, 1.0])
    for al in ([0.0, 0.0], [], list(range(16)), [0.0, np.inf]):
        with pytest.raises(ValueError, match='thresholds must'):
            vb.OrdinalGLMMObjective(_par(vb, 2, K, G), x, np.zeros(N), z, gid, G, al)

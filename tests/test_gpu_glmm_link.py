"""`BinomialGLMMObjective(link='probit' | 'cloglog')` on the GPU: the BinomialLinkLik instantiations of the
shared tile walk against the torch reference tests/glmm_link_reference.py, the aggregation, Poisson and symmetry identities,
predictions, streamed influence, the state contract of lrvb_set_link, the overflow refusal and a fit per link.

Error measure and bounds are those of tests/test_gpu_glmm_binomial.py and tests/test_gpu_glmm_binomial_influence.py: value 1e-11,
gradient 1e-10, Hessian / products / Schur complement 1e-9 relative; LRVB covariance and solves rtol 1e-6; influence rows 1e-9,
group sums against the weighted rows 1e-10, the dense cross Hessian 1e-9, quantities behind an H^-1 rtol 1e-6 with atol 1e-12.

Positive definiteness of the reference free Hessian at the off-optimum point of `problem`, checked on the CPU for exactly these
draws (seed N + P + K), smallest eigenvalue probit | cloglog: (1, 1, 1, 1) 0.180 | 0.179, (37, 3, 2, 5) 0.131 | 0.128,
(65, 5, 2, 3) 0.205 | 0.205, (130, 64, 4, 2) 0.198 | 0.242, (300, 17, 4, 7) 0.196 | 0.196 (local blocks >= 0.209).  So every
shape runs the covariance and solve checks, and asserts positive definiteness before it does.

Bounds that are this file's own.  Probit flip: the two runs evaluate the same per-node terms at mirrored arguments (the nodes of
the rule mirror to an ulp) in another lane order; 20 nodes x the worst amplification of the probit formulas (230, at t = -15:
tests/test_glmm_link_host_math.py) x 2^-53 = 5e-13, so 1e-11 of the largest entry for gradient and Hessian and 1e-12 for the
value, which has no such amplification.  Response means: per trial a sum of node terms in [0, 1] whose weights sum to 1, each good
to a few ulp: 1e-12 per trial; the probit closed form is one erfc at an argument of at most 6 in size, whose rounding is
amplified by at most x^2 = 36: 1e-13 relative."""
import numpy as np
import pytest
import torch

import glmm_link_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _point, _fit
from test_gpu_glmm_binomial import _prior_kw, _check_against_reference, _same
from test_gpu_glmm_binomial import _model as _logit_model
from test_gpu_glmm_poisson import _model as _poisson_model

pytestmark = pytest.mark.gpu

LINKS = ref.LINKS
SHAPES = [(1, 1, 1, 1), (37, 3, 2, 5), (65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7)]
INFL_SHAPES = [(37, 3, 2, 5), (65, 5, 2, 3), (130, 64, 4, 2)]


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _model(vb, x, y, z, w, o, mt, gid, G, link, hyp=HYP):
    par = _par(vb, x.shape[1], z.shape[1], G)
    return par, vb.BinomialGLMMObjective(par, x, y, z, gid, G, trials=mt, offset=o, weights=w, link=link, **_prior_kw(hyp))


_cache = {}


def _case(vb, N, P, K, G, link):
    """The model at the point of `problem`, computed once per case."""
    key = (N, P, K, G, link)
    if key not in _cache:
        x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, N + P + K, link)
        par, fun = _model(vb, x, y, z, w, o, mt, gid, G, link)
        _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, o=o, mt=mt, free=free, eta=_eta(free, P, K, G), par=par, fun=fun,
                           targs=ref.targs(x, y, z, w, o, mt, gid, G, link, HYP))
    return _cache[key]


# ---- A: the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('link', LINKS)
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G, link):
    c = _case(vb, N, P, K, G, link)
    y, mt, gid = c['y'], c['mt'], c['gid']
    if N >= 4:
        assert mt[0] == 0 and mt[1] == 1 and y[2] == 0 and mt[2] >= 2 and y[3] == mt[3] >= 2      # no trials, Bernoulli, y = 0, y = m
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2      # an empty group, one with more than half the rows
    _check_against_reference(c['par'], c['fun'], ref.kl_vec, ref.kl_free, c['targs'], c['free'], G, K, solves=True)


# ---- B: identities -----------------------------------------------------------------------------------------------------------
def _vgh(fun, eta):
    return fun.value(eta, False), fun.grad(eta, False), fun.hessian(eta, False)


@pytest.mark.parametrize('link', LINKS)
@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 64, 4, 2)])
def test_aggregated_rows_equal_the_expanded_bernoulli_rows(vb, N, P, K, G, link):
    """y successes out of m trials with weight w = a row (y = 1, weight w y) and a row (y = 0, weight w (m - y)) with one trial
    each, in the same class under the same link: x, z and the offset duplicated."""
    c = _case(vb, N, P, K, G, link)
    x, y, z, w, gid, o, mt, eta = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'mt', 'eta'))
    _, two = _model(vb, np.vstack([x, x]), np.concatenate([np.ones(N), np.zeros(N)]), np.vstack([z, z]),
                    np.concatenate([w * y, w * (mt - y)]), np.concatenate([o, o]), None, np.concatenate([gid, gid]), G, link)
    a, b = _vgh(c['fun'], eta), _vgh(two, eta)
    e = [abs(a[0] - b[0]) / abs(b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2])]
    print('aggregation', link, N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9


@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 64, 4, 2)])
def test_cloglog_without_successes_is_the_poisson_model(vb, N, P, K, G):
    """All y = 0: the cloglog term m e^t is the Poisson term with offset o + log m and y = 0 -- the closed form of E h0, to 1e-12.
    At the point of `problem` s_n <= 1.6 and the 20-node rule itself integrates e^t to an ulp, so a kernel that took E h0 on the
    nodes would pass there.  The comparison is therefore repeated with every variance times 30: s_n up to 31 and 48 at the two
    shapes, where the rule's weighted sum is off by 5e-4 and 6e-2 (computed on the CPU for these draws) and the closed form is
    not; rho + s / 2 <= 27 there, far from overflow."""
    c = _case(vb, N, P, K, G, 'cloglog')
    x, z, w, gid, o = (c[k] for k in ('x', 'z', 'w', 'gid', 'o'))
    mt = np.maximum(c['mt'], 1.0)
    zero = np.zeros(N)
    _, fun = _model(vb, x, zero, z, w, o, mt, gid, G, 'cloglog')
    _, pois = _poisson_model(vb, x, zero, z, w, o + np.log(mt), gid, G)
    ng = 2 * P + 4 * K
    for widen in (1.0, 30.0):
        eta = c['eta'].copy()
        eta[P:2 * P] /= widen                                            # the precisions of beta and of the effects
        eta[ng + G * K:] /= widen
        a, b = _vgh(fun, eta), _vgh(pois, eta)
        e = [abs(a[0] - b[0]) / abs(b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2])]
        m_, v_, e_, r_ = _point(eta, P, K, G)
        s = (x * x) @ v_ + np.sum(z * z * r_[gid], axis=1)
        print('cloglog against Poisson', N, P, K, G, 'variances x', widen, 'largest s', float(s.max()), e)
        assert max(e) < 1e-12
    assert s.max() > 30.0


@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 64, 4, 2)])
def test_probit_symmetry_under_the_flip(vb, N, P, K, G):
    """(y, x, z, o) -> (m - y, -x, -z, -o) at the same point: h0(t) = h1(-t).  Bounds: module docstring."""
    c = _case(vb, N, P, K, G, 'probit')
    x, y, z, w, gid, o, mt, eta = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'mt', 'eta'))
    _, flip = _model(vb, -x, mt - y, -z, w, -o, mt, gid, G, 'probit')
    a, b = _vgh(c['fun'], eta), _vgh(flip, eta)
    e = [abs(a[0] - b[0]) / abs(b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2])]
    print('probit flip', N, P, K, G, e)
    assert e[0] < 1e-12 and e[1] < 1e-11 and e[2] < 1e-11
    assert np.any(y != mt - y)


# ---- C: predictions ----------------------------------------------------------------------------------------------------------
def _moments(x, z, gid, P, K, G):
    ng = 2 * P + 4 * K
    C = np.zeros((x.shape[0], ng + 2 * G * K))
    C[:, :P] = x
    for n, g in enumerate(gid):
        C[n, (2 * P if g < 0 else ng + g * K) + np.arange(K)] = z[n]
    return C


@pytest.mark.parametrize('link', LINKS)
@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (130, 64, 4, 2)])
def test_predict_window_and_new_rows(vb, N, P, K, G, link):
    """Both routes; a window no tile boundary aligns with and new rows, some at the population level (group -1)."""
    from scipy.special import ndtr
    c = _case(vb, N, P, K, G, link)
    fun, free, x, z, gid, mt = c['fun'], c['free'], c['x'], c['z'], c['gid'], c['mt']
    _, _, Hf = ref.value_grad_hess(ref.kl_free, free, c['targs'])
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    Hinv = np.linalg.inv(Hf)
    rng = np.random.default_rng([N, 35])
    n_new = 70
    new = dict(x=rng.normal(size=(n_new, P)) / np.sqrt(P), z=np.concatenate([np.ones((n_new, 1)), 0.5 * rng.normal(size=(n_new, K - 1))], axis=1),
               groups=rng.integers(0, G, size=n_new), offset=0.3 * rng.normal(size=n_new),
               trials=rng.integers(0, 13, size=n_new).astype(np.float64))
    new['groups'][::9] = -1
    n0, n1 = 3, N - 2
    for what, kw, Cm, trials in (('window', dict(n0=n0, n1=n1), _moments(x[n0:n1], z[n0:n1], gid[n0:n1], P, K, G), mt[n0:n1]),
                                 ('new rows', dict(newdata=new), _moments(new['x'], new['z'], new['groups'], P, K, G), new['trials'])):
        want_var = np.einsum('nd,de,ne->n', Cm, Hinv, Cm)
        outs = [fun.predict(free, on_device=dev, **kw) for dev in (False, True)]
        for route, out in zip(('host', 'device'), outs):
            assert np.allclose(out['var_lrvb'], want_var, rtol=1e-6, atol=0)
            cap = 1e-12 * np.maximum(trials, 1.0)
            for col, var in (('mean_mf', 'var_mf'), ('mean_lrvb', 'var_lrvb')):
                want = ref.response_mean(link, out['rho'], out[var], trials, deg=128 if link == 'probit' else ref.GH_DEG)
                err = np.abs(out[col] - want)
                print('predict', link, (N, P, K, G), what, route, col, float(np.max(err / np.maximum(trials, 1.0))))
                assert out[col].shape == trials.shape and np.all(err <= cap)
                assert np.array_equal(out[col][trials == 0], np.zeros(int(np.sum(trials == 0))))
                if link == 'probit':
                    closed = trials * ndtr(out['rho'] / np.sqrt(1.0 + out[var]))
                    assert np.all(np.abs(out[col] - closed) <= 1e-13 * closed)
        assert np.allclose(outs[1]['var_lrvb'], outs[0]['var_lrvb'], rtol=1e-6, atol=0)
    # a window equals the same rows of the full result bitwise
    full = fun.predict(free, on_device=True)
    win = fun.predict(free, n0=n0, n1=n1, on_device=True)
    assert all(np.array_equal(win[k], full[k][n0:n1]) for k in full)


# ---- D: influence ------------------------------------------------------------------------------------------------------------
def _segment_sum(gid, G, v):
    out = np.zeros((G,) + v.shape[1:])
    np.add.at(out, gid, v)
    return out


_infl = {}


def _infl_case(vb, N, P, K, G, link):
    """The dense reference of tests/test_gpu_glmm_binomial_influence.py::_case for a link, computed once."""
    key = (N, P, K, G, link)
    if key in _infl:
        return _infl[key]
    c = _case(vb, N, P, K, G, link)
    t, free, eta = c['targs'], c['free'], c['eta']
    ng, GK = 2 * P + 4 * K, G * K
    p = torch.tensor(np.concatenate([eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + GK], 1.0 / eta[ng + GK:]]), requires_grad=True)
    wt = t[3].clone().requires_grad_(True)
    et = torch.cat([p[:P], 1.0 / p[P:2 * P], torch.tensor(eta[2 * P:ng]), p[2 * P:2 * P + GK], 1.0 / p[2 * P + GK:]])
    g, = torch.autograd.grad(ref.kl_vec(et, t[0], t[1], t[2], wt, *t[4:]), p, create_graph=True)
    rows_mv = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())], axis=1)
    wt2 = t[3].clone().requires_grad_(True)
    q = torch.tensor(free).requires_grad_(True)
    gf, = torch.autograd.grad(ref.kl_free(q, t[0], t[1], t[2], wt2, *t[4:]), q, create_graph=True)
    Cw = np.stack([torch.autograd.grad(gf[k], wt2, retain_graph=True)[0].numpy() for k in range(gf.numel())])
    _, _, Hf = ref.value_grad_hess(ref.kl_free, free, t)
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    _infl[key] = dict(c, rows_mv=rows_mv, Cw=Cw, Hf=Hf)
    return _infl[key]


@pytest.mark.parametrize('link', LINKS)
@pytest.mark.parametrize('N,P,K,G', INFL_SHAPES)
def test_influence_rows_windows_and_group_sums_against_autograd(vb, N, P, K, G, link):
    c = _infl_case(vb, N, P, K, G, link)
    fun, w, gid = c['fun'], c['w'], c['gid']
    pt = _point(c['eta'], P, K, G) + (fun.gh_x, fun.gh_w)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want = c['rows_mv'] @ A.T                                            # N x 21
    for Q in (5, 21):                                                    # 21 crosses the 16-column MFMA block
        got = fun.ctx.glmm_binomial_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', link, N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        win = fun.ctx.glmm_binomial_obs_influence(*pt, A[:Q], n0=3, n1=N - 2)
        assert win.shape == (N - 5, Q) and np.array_equal(win, got[3:N - 2])
    rows = fun.ctx.glmm_binomial_obs_influence(*pt, A)
    a, b = fun.ctx.glmm_binomial_group_influence(*pt, A), fun.ctx.glmm_binomial_group_influence(*pt, A)
    e = rel_err(a, _segment_sum(gid, G, w[:, None] * rows))
    print('group sums', link, N, P, K, G, e)
    assert a.shape == (G, 21) and e < 1e-10
    assert rel_err(a, _segment_sum(gid, G, w[:, None] * want)) < 1e-9   # and against autograd directly
    assert np.array_equal(a, b)                                           # bitwise reproducible
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)      # the empty group


@pytest.mark.parametrize('link', LINKS)
@pytest.mark.parametrize('N,P,K,G', INFL_SHAPES)
def test_influence_routes_stream_hyper_and_dense_cross_hessian(vb, N, P, K, G, link):
    c = _infl_case(vb, N, P, K, G, link)
    fun, par, free, w, gid = c['fun'], c['par'], c['free'], c['w'], c['gid']
    D = 2 * P + 4 * K + 2 * G * K
    want = -np.linalg.solve(c['Hf'], c['Cw']).T                           # N x D
    rows = fun.obs_influence(free, np.eye(D))
    print('arrow route', link, rel_err(rows, want))
    assert np.allclose(rows, want, rtol=1e-6, atol=1e-12)
    assert np.allclose(fun.obs_influence(free, np.eye(D), on_device=True), rows, rtol=1e-6, atol=1e-12)
    gi = fun.group_influence(free, np.eye(D))
    assert np.allclose(fun.group_influence(free, np.eye(D), on_device=True), gi, rtol=1e-6, atol=1e-12)
    assert np.allclose(gi, _segment_sum(gid, G, w[:, None] * want), rtol=1e-6, atol=1e-12)
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, free, w, stream_hyper=True)
    dense = lin.get_doutput_dhyper_rows(np.eye(D))
    assert np.allclose(dense, want, rtol=1e-6, atol=1e-12)
    n0, n1 = 7, min(N - 1, 100)
    assert np.allclose(lin.get_doutput_dhyper_rows(np.eye(D)[:3], n0=n0, n1=n1), want[n0:n1, :3], rtol=1e-6, atol=1e-12)
    # the dense weight cross Hessian (small-N protocol): a1' of these links carries no "- y"
    C = fun.cross_hessian(fun.weights_par, free, True)
    assert C.shape == (D, N) and rel_err(C, c['Cw']) < 1e-9


# ---- E: state ----------------------------------------------------------------------------------------------------------------
def test_set_link_state_contract(vb):
    hip = vb._hip
    N, P, K, G = 130, 4, 2, 5
    x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, 31, 'probit', empty_group=False)
    y1 = np.minimum(y, 1.0)                                              # responses every likelihood accepts
    eta = _eta(free, P, K, G)
    pt = _point(eta, P, K, G)
    _, plain = _logit_model(vb, x, y, z, w, o, mt, gid, G)               # the class without the keyword
    _, fun = _model(vb, x, y, z, w, o, mt, gid, G, 'logit')
    ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G * K))
    entries = lambda cx: (cx.glmm_binomial_terms(*pt, *gh), cx.glmm_binomial_obs_influence(*pt, *gh, A, n0=3, n1=N - 2),
                          cx.glmm_binomial_group_influence(*pt, *gh, A))
    base = entries(plain.ctx)
    same = lambda a, b: _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert same(entries(ctx), base)                                      # link='logit' is the class without the keyword, bit for bit
    # an invalid link is refused and changes nothing
    for bad in (-1, 3, 7):
        assert ctx._lib.lrvb_set_link(ctx._h, bad) == hip.ERR_UNSUPPORTED
        with pytest.raises(NotImplementedError):
            ctx.set_link(bad)
    assert same(entries(ctx), base)
    # a set drops the resident sums and factor
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    ctx.glmm_binomial_terms(*pt, *gh)
    assert schur() == hip.OK
    for link in (1, 2, 0, 0):
        ctx.glmm_binomial_terms(*pt, *gh)
        assert schur() == hip.OK
        ctx.set_link(link)
        assert schur() == hip.ERR_STATE
    # the logistic and Poisson entries do not read the link
    ctx.set_data(hip.SLOT_Y, y1)
    others = lambda: (ctx.glmm_slopes_terms(*pt, *gh), ctx.glmm_slopes_obs_influence(*pt, *gh, A), ctx.glmm_slopes_group_influence(*pt, *gh, A),
                      ctx.glmm_poisson_terms(*pt), ctx.glmm_poisson_obs_influence(*pt, A), ctx.glmm_poisson_group_influence(*pt, A))
    before = others()
    for link in (1, 2):
        ctx.set_link(link)
        after = others()
        assert _same(after[0], before[0]) and _same(after[3], before[3])
        assert all(np.array_equal(after[i], before[i]) for i in (1, 2, 4, 5))
    ctx.set_data(hip.SLOT_Y, y)
    # probit differs, and going back to logit gives the original bits
    ctx.set_link(1)
    probit = entries(ctx)
    assert not _same(probit[0], base[0])
    ctx.set_link(2)
    assert not _same(entries(ctx)[0], probit[0])
    ctx.set_link(0)
    assert same(entries(ctx), base)


def test_cloglog_overflow_is_refused(vb):
    """exp(rho + s / 2) is not clamped: a point where it overflows is a ValueError, as for the Poisson model."""
    N, P, K, G = 37, 3, 2, 5
    c = _case(vb, N, P, K, G, 'cloglog')
    eta = c['eta'].copy()
    assert np.isfinite(c['fun'].value(eta, False))
    n = int(np.argmax(c['mt'] - c['y']))                                 # a row with trials that failed: E h0 enters
    eta[:P] = 2000.0 * np.sign(c['x'][n])                                # rho_n = 2000 sum_j |x_nj| > 710
    assert c['mt'][n] > c['y'][n] and 2000.0 * np.sum(np.abs(c['x'][n])) > 1000.0
    with pytest.raises(ValueError):
        c['fun'].value(eta, False)
    assert np.isfinite(c['fun'].value(c['eta'], False))                  # and the context goes on working


# ---- F: fit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('link', LINKS)
def test_fit_covariance_and_tau_prior_sensitivity(vb, link):
    """The body and thresholds of tests/test_gpu_glmm_binomial.py::test_fit_covariance_and_tau_prior_sensitivity."""
    N, P, K, G = 2000, 4, 2, 30
    x, y, z, w, gid, o, mt, free0 = ref.problem(N, P, K, G, 77, link, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, o, mt, gid, G, link)
    ng = 2 * P + 4 * K
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = ref.targs(x, y, z, w, o, mt, gid, G, link, HYP)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    print('reference gradient at the fit', link, np.max(np.abs(g_ad)))
    assert np.max(np.abs(g_ad)) < 1e-6                                   # stationary by the REFERENCE gradient
    assert np.min(np.linalg.eigvalsh(H_ad)) > 0
    Hinv = np.linalg.inv(H_ad)
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    cov = gc.lrvb_cov(np.eye(ng)[:P])
    assert np.allclose(cov, Hinv[:P, :P], rtol=1e-6, atol=0)
    M = np.zeros((2, th.size))
    idx = [0, ng + (G * K) // 2]
    M[0, idx[0]], M[1, idx[1]] = 1.0, 1.0
    for on_device in (False, True):
        assert np.allclose(fun.lrvb_cov(th, M, on_device=on_device), Hinv[np.ix_(idx, idx)], rtol=1e-6, atol=1e-12)
    se_lr, se_mf = fun.ranef_se(th, on_device=True)
    ie = ng + np.arange(G * K)
    assert np.allclose(se_lr.ravel(), np.sqrt(np.diag(Hinv)[ie]), rtol=1e-6, atol=0) and se_mf.shape == (G, K)
    par.set_free(th)
    assert np.all(np.diag(cov) > 1.0 / par['beta']['info'].get())
    sens = fun.global_sensitivity(fun.tau_prior_par, th)
    h = np.array([0.05, -0.03])
    base = np.asarray(fun.tau_prior_par.get_vector(), dtype=np.float64).copy()
    fun.tau_prior_par.set_vector(base + h)
    th_p = _fit(vb, objective, th)
    fun.tau_prior_par.set_vector(base - h)
    th_m = _fit(vb, objective, th)
    fun.tau_prior_par.set_vector(base)
    diff = 0.5 * (th_p - th_m)[:ng]
    print('tau prior sensitivity', link, np.max(np.abs(sens @ h - diff)), np.max(np.abs(diff)))
    assert np.max(np.abs(sens @ h - diff)) < 0.05 * np.max(np.abs(diff)) + 1e-8

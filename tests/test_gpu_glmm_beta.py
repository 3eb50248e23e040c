"""`BetaGLMMObjective` on the GPU: the BetaLik instantiations of the shared tile walk against the torch
reference tests/glmm_beta_reference.py, the mirror identity across two models, the known answer against scipy's Beta density,
predictions, streamed influence, the state contract, the refusals, extreme points and a fit.

Error measure and bounds are those of tests/test_gpu_glmm_ztnegbin.py: value 1e-11, gradient 1e-10, Hessian / products / Schur
complement 1e-9 relative; LRVB covariance and solves rtol 1e-6; influence rows 1e-9, group sums against the weighted rows 1e-10,
the dense cross Hessian 1e-9, quantities behind an H^-1 rtol 1e-6 with atol 1e-12; identities 1e-12 of the largest magnitude.

Shapes (N, P, K, G): (1, 1, 1, 1); (37, 3, 1, 5) with z=None, offset=None and a scalar phi; (65, 5, 2, 3) with 5 nodes -- a second
tile of one row, a cut group and an empty group; (130, 64, 4, 2); (300, 17, 4, 7) with every fifth weight zero.  phi = 7.5 at the
first three, one value per row on [0.5, 1e3] (both ends present) at the last two.  Every data set with N >= 4 holds the probe rows
y[0] = 1e-12, y[1] = 1 - 1e-12 and y[2] = 0.5.  The Beta term is not convex in t, but the reference free Hessian is positive
definite at the off-optimum point of `problem` for these draws (seed N + P + K; smallest eigenvalues 0.178, 0.189, 0.199, 0.282,
0.196, computed on the CPU, printed by the parity test and recorded in DESIGN.md section 40), so every shape runs the covariance
and solve checks.  Every |rho_n| of these data sets is below 5: the reference meets its 1e-10 cap against mpmath there
(tests/test_glmm_beta_host_math.py).

Mirror identity.  h(t; l) = h(-t; -l) - phi l and h^(k)(t; l) = (-1)^k h^(k)(-t; -l).  Model B = (-x, -z, -o, 1 - y) at the SAME point
has rho' = -rho: every product of a design column with an odd derivative keeps its sign, so value + sum w phi l, gradient, H blocks
and group sums all EQUAL those of model A.  Model C = (x, z, -o, 1 - y) at the point with the means negated (-m, -e) has rho' = -rho
too, with the design unchanged: the gradient is negated on the mean coordinates and equal on the variance ones, and the cross block
of H is negated."""
import numpy as np
import pytest
import torch

import glmm_beta_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _point, _fit
from test_gpu_glmm_binomial import _prior_kw, _check_against_reference, _same, _model as _binomial_model
from test_gpu_glmm_link import _moments, _segment_sum
from test_gpu_glmm_ztnegbin import _largest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7)]
INFL_SHAPES = [(37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2)]
IDENT_SHAPES = [(130, 64, 4, 2), (300, 17, 4, 7)]
DEG = {(65, 5, 2, 3): 5}                                                 # the others: 20 nodes
IDENT = 1e-12


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _data(N, P, K, G):
    """The draws of a shape: (x, y, z, w, gid, o, phi (N), free, deg, bare) -- `bare`: the model is handed z=None, offset=None and
    the scalar phi (the reference a column of ones, zeros and N equal values)."""
    bare = (N, P, K, G) == (37, 3, 1, 5)
    x, y, z, w, gid, o, ph, free = ref.problem(N, P, K, G, N + P + K, phi='vector' if N >= 130 else 7.5, zero_weights=(N == 300))
    if bare:
        o = np.zeros(N)
        assert np.array_equal(z, np.ones((N, 1)))
    if N >= 130:
        assert ph.min() == 0.5 and ph.max() == 1e3
    return x, y, z, w, gid, o, ph, free, DEG.get((N, P, K, G), ref.GH_DEG), bare


def _model(vb, x, y, z, w, o, phi, gid, G, deg=ref.GH_DEG, hyp=HYP, K=None):
    par = _par(vb, x.shape[1], K if z is None else z.shape[1], G)
    return par, vb.BetaGLMMObjective(par, x, y, z, gid, G, phi, offset=o, weights=w, gh_deg=deg, **_prior_kw(hyp))


_cache = {}


def _case(vb, N, P, K, G):
    """The model at the point of `problem`, computed once per case."""
    key = (N, P, K, G)
    if key not in _cache:
        x, y, z, w, gid, o, ph, free, deg, bare = _data(N, P, K, G)
        par, fun = _model(vb, x, y, None if bare else z, w, None if bare else o, 7.5 if bare else ph, gid, G, deg, K=K)
        _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, o=o, ph=ph, free=free, deg=deg, eta=_eta(free, P, K, G), par=par, fun=fun,
                           targs=ref.targs(x, y, z, w, o, ph, gid, G, HYP, deg))
    return _cache[key]


def _hf(c):
    """The reference free Hessian of a case, computed once (the parity test leaves its own here)."""
    if 'Hf' not in c:
        c['Hf'] = ref.value_grad_hess(ref.kl_free, c['free'], c['targs'])[2]
    return c['Hf']


def _rho_s(c, pt):
    m, v, e, r = pt
    return c['o'] + c['x'] @ m + np.sum(c['z'] * e[c['gid']], axis=1), (c['x'] * c['x']) @ v + np.sum(c['z'] * c['z'] * r[c['gid']], axis=1)


# ---- A: the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G):
    c = _case(vb, N, P, K, G)
    y, w, gid, ph = c['y'], c['w'], c['gid'], c['ph']
    assert np.all((y > 0.0) & (y < 1.0))
    if N >= 4:
        assert (y[0], y[1], y[2]) == ref.PROBES                          # rows next to either end and in the middle
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2     # an empty group, one with more than half the rows
    if N == 300:
        assert np.sum(w == 0.0) == 60
    assert c['fun'].gh_x.size == c['deg']
    rho, _ = _rho_s(c, _point(c['eta'], P, K, G))
    assert np.max(np.abs(rho)) < 12.0                                    # where the reference meets its cap against mpmath
    _, Hf = _check_against_reference(c['par'], c['fun'], ref.kl_vec, ref.kl_free, c['targs'], c['free'], G, K, solves=True)
    c['Hf'] = Hf
    print('smallest eigenvalue of the reference free Hessian', (N, P, K, G), float(np.min(np.linalg.eigvalsh(Hf))))
    assert abs(c['fun'].log_norm_const() - ref.log_norm_const(y, ph, w)) < 1e-9
    # two evaluations at one point are bitwise equal (through a model of its own: a direct call of the terms entry on a shared
    # context would drop the factor the class believes resident)
    other = _model(vb, c['x'], c['y'], c['z'], c['w'], c['o'], c['ph'], c['gid'], G, c['deg'])[1]
    pt = _point(c['eta'], P, K, G) + (other.gh_x, other.gh_w)
    assert _same(other.ctx.glmm_beta_terms(*pt), other.ctx.glmm_beta_terms(*pt))


# ---- B: identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_mirror_identity_across_models(vb, N, P, K, G):
    """Module docstring.  First the reference alone, on the CPU and for these rows; then the `terms` entries of three models, at the
    point of `problem` and with every variance times 30."""
    c = _case(vb, N, P, K, G)
    x, y, z, w, gid, o, ph, deg = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'ph', 'deg'))
    l = np.log(y) - np.log1p(-y)
    _, B = _model(vb, -x, 1.0 - y, -z, w, -o, ph, gid, G, deg)
    _, Cm = _model(vb, x, 1.0 - y, z, w, -o, ph, gid, G, deg)
    A = _model(vb, x, y, z, w, o, ph, gid, G, deg)[1]                    # a context of its own: the terms entry is called directly
    # 1 - y is not exactly mirrored in fp64 for the probe rows (1 - (1 - 1e-12) != 1e-12): hand the mirrored models the logit itself
    for fun in (B, Cm):
        fun._y = -l
        fun.ctx.set_data(vb._hip.SLOT_Y, -l)
    m, v, e, r = _point(c['eta'], P, K, G)
    shift = float(np.sum(w * ph * l))
    for widen in (1.0, 30.0):
        pt = (m, v * widen, e, r * widen)
        rho, s = _rho_s(c, pt)
        a, b = ref.eh_coefs(rho, s, l, ph, deg), ref.eh_coefs(-rho, s, -l, ph, deg)
        b[0] -= ph * l
        b[1::2] *= -1.0
        e_ref = float(np.max(np.max(np.abs(a - b), axis=1) / np.max(np.abs(a), axis=1)))
        print('mirror identity, reference alone', (N, P, K, G), 'variances x', widen, 'largest s', float(s.max()), e_ref)
        assert e_ref <= 1e-13
        gh = (A.gh_x, A.gh_w)
        ta, tb = A.ctx.glmm_beta_terms(*pt, *gh), B.ctx.glmm_beta_terms(*pt, *gh)
        tc = Cm.ctx.glmm_beta_terms(-m, pt[1], -e, pt[3], *gh)
        big = max(abs(ta[0]), abs(shift))
        errs = [abs(ta[0] - (tb[0] - shift)) / big] + [_largest(ta[i], tb[i]) for i in (1, 2, 3)]
        sign_g = np.concatenate([-np.ones(P), np.ones(P)])
        sign_H = np.array([1.0, -1.0, 1.0])[:, None, None]
        errs += [abs(ta[0] - (tc[0] - shift)) / big, _largest(ta[1], sign_g * tc[1]), _largest(np.reshape(ta[2], (3, P, P)), sign_H * np.reshape(tc[2], (3, P, P)))]
        print('mirror identity', (N, P, K, G), 'variances x', widen, errs)
        assert max(errs) <= IDENT
    assert s.max() > 30.0


@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (300, 17, 4, 7)])
def test_single_node_known_answer(vb, N, P, K, G):
    """One node (gh_deg = 1: t = rho): value - log_norm_const - (prior and entropy terms of the reference) = -sum w log Beta(y)."""
    from scipy.stats import beta as beta_dist
    c = _case(vb, N, P, K, G)
    x, y, z, w, gid, o, ph, eta = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'ph', 'eta'))
    _, fun = _model(vb, x, y, z, w, o, ph, gid, G, 1)
    assert fun.gh_x.size == 1
    t = c['targs']
    priors = float(ref._priors(torch.tensor(eta), t[0], t[1], t[2], t[3], t[6], G, t[8]))
    rho, _ = _rho_s(c, _point(eta, P, K, G))
    mu = 1.0 / (1.0 + np.exp(-rho))
    want = -np.sum(w * beta_dist.logpdf(y, mu * ph, (1.0 - mu) * ph))
    got = fun.value(eta, False) - fun.log_norm_const() - priors
    print('single node', (N, P, K, G), got, want, abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-11 * abs(want)


# ---- C: predictions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (130, 64, 4, 2)])
def test_predict_window_and_new_rows(vb, N, P, K, G):
    """Both routes; a window no tile boundary aligns with and new rows, some at the population level (group -1).  The mean is the
    logistic E sigma whatever phi: the device route goes through the binomial predict entry with one trial, and what does not
    depend on the model's own Hessian (rho, var_mf, mean_mf) equals `BinomialGLMMObjective.predict` on the same design bitwise."""
    c = _case(vb, N, P, K, G)
    fun, free, x, z, gid, deg, w = c['fun'], c['free'], c['x'], c['z'], c['gid'], c['deg'], c['w']
    Hf = _hf(c)
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    Hinv = np.linalg.inv(Hf)
    rng = np.random.default_rng([N, 37])
    n_new = 70
    new = dict(x=rng.normal(size=(n_new, P)) / np.sqrt(P), z=np.concatenate([np.ones((n_new, 1)), 0.5 * rng.normal(size=(n_new, K - 1))], axis=1),
               groups=rng.integers(0, G, size=n_new), offset=0.3 * rng.normal(size=n_new))
    new['groups'][::9] = -1
    n0, n1 = 3, N - 2
    par_b = _par(vb, P, K, G)
    bino = vb.BinomialGLMMObjective(par_b, x, (c['y'] > 0.5).astype(np.float64), z, gid, G, offset=c['o'], weights=w, gh_deg=deg, **_prior_kw(HYP))
    for what, kw, Cm, off in (('window', dict(n0=n0, n1=n1), _moments(x[n0:n1], z[n0:n1], gid[n0:n1], P, K, G), c['o'][n0:n1]),
                              ('new rows', dict(newdata=new), _moments(new['x'], new['z'], new['groups'], P, K, G), new['offset'])):
        want_var = np.einsum('nd,de,ne->n', Cm, Hinv, Cm)
        want_rho = off + Cm @ free                                       # the means are free coordinates themselves
        outs = [fun.predict(free, on_device=dev, **kw) for dev in (False, True)]
        for route, out in zip(('host', 'device'), outs):
            assert np.allclose(out['rho'], want_rho, rtol=1e-12, atol=1e-12)
            assert np.allclose(out['var_lrvb'], want_var, rtol=1e-6, atol=0)
            for col, var in (('mean_mf', 'var_mf'), ('mean_lrvb', 'var_lrvb')):
                want = ref.response_mean(out['rho'], out[var], deg)
                err = np.abs(out[col] - want) / want
                print('predict', (N, P, K, G), what, route, col, float(np.max(err)))
                assert out[col].shape == want.shape and np.all((want > 0.0) & (want < 1.0)) and np.all(err <= 1e-12)
        assert np.allclose(outs[1]['var_lrvb'], outs[0]['var_lrvb'], rtol=1e-6, atol=0)
        ob = bino.predict(free, on_device=True, **kw)
        assert all(np.array_equal(outs[1][k], ob[k]) for k in ('rho', 'var_mf', 'mean_mf'))
    # a window equals the same rows of the full result bitwise
    full = fun.predict(free, on_device=True)
    win = fun.predict(free, n0=n0, n1=n1, on_device=True)
    assert all(np.array_equal(win[k], full[k][n0:n1]) for k in full)
    # newdata may carry a dispersion (the mean does not use it) and needs none; trials are not a key of this model
    with_phi = fun.predict(free, newdata=dict(new, dispersion=np.full(n_new, 3.0)), on_device=True)
    without = fun.predict(free, newdata=new, on_device=True)
    assert all(np.array_equal(with_phi[k], without[k]) for k in without)
    with pytest.raises(ValueError, match='trials'):
        fun.predict(free, newdata=dict(new, trials=np.ones(n_new)))


# ---- D: influence ------------------------------------------------------------------------------------------------------------
_infl = {}


def _infl_case(vb, N, P, K, G):
    """The dense reference of tests/test_gpu_glmm_link.py::_infl_case, computed once."""
    key = (N, P, K, G)
    if key in _infl:
        return _infl[key]
    c = _case(vb, N, P, K, G)
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
    Hf = _hf(c)
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    _infl[key] = dict(c, rows_mv=rows_mv, Cw=Cw, Hf=Hf)
    return _infl[key]


@pytest.mark.parametrize('N,P,K,G', INFL_SHAPES)
def test_influence_rows_windows_and_group_sums_against_autograd(vb, N, P, K, G):
    c = _infl_case(vb, N, P, K, G)
    fun, w, gid = c['fun'], c['w'], c['gid']
    pt = _point(c['eta'], P, K, G) + (fun.gh_x, fun.gh_w)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want = c['rows_mv'] @ A.T                                            # N x 21
    for Q in (5, 21):                                                    # 21 crosses the 16-column MFMA block
        got = fun.ctx.glmm_beta_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        win = fun.ctx.glmm_beta_obs_influence(*pt, A[:Q], n0=3, n1=N - 2)
        assert win.shape == (N - 5, Q) and np.array_equal(win, got[3:N - 2])
    rows = fun.ctx.glmm_beta_obs_influence(*pt, A)
    a, b = fun.ctx.glmm_beta_group_influence(*pt, A), fun.ctx.glmm_beta_group_influence(*pt, A)
    e = rel_err(a, _segment_sum(gid, G, w[:, None] * rows))
    print('group sums', N, P, K, G, e)
    assert a.shape == (G, 21) and e < 1e-10
    assert rel_err(a, _segment_sum(gid, G, w[:, None] * want)) < 1e-9   # and against autograd directly
    assert np.array_equal(a, b)                                           # bitwise reproducible
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)      # the empty group


@pytest.mark.parametrize('N,P,K,G', INFL_SHAPES)
def test_influence_routes_stream_hyper_and_dense_cross_hessian(vb, N, P, K, G):
    c = _infl_case(vb, N, P, K, G)
    fun, par, free, w, gid = c['fun'], c['par'], c['free'], c['w'], c['gid']
    D = 2 * P + 4 * K + 2 * G * K
    want = -np.linalg.solve(c['Hf'], c['Cw']).T                           # N x D
    rows = fun.obs_influence(free, np.eye(D))
    print('arrow route', rel_err(rows, want))
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
    C = fun.cross_hessian(fun.weights_par, free, True)                   # the dense weight cross Hessian (small-N protocol)
    assert C.shape == (D, N) and rel_err(C, c['Cw']) < 1e-9


# ---- E: state and refusals -----------------------------------------------------------------------------------------------------
def test_state_contract(vb):
    """The new entries read neither lrvb_set_link nor lrvb_set_trials, leave the other likelihoods' entries alone, and a missing
    dispersion is LRVB_ERR_STATE after which the context goes on working."""
    hip = vb._hip
    N, P, K, G = 130, 4, 2, 5
    x, y, z, w, gid, o, ph, free = ref.problem(N, P, K, G, 31, phi='vector', empty_group=False)
    pt = _point(_eta(free, P, K, G), P, K, G)
    _, fun = _model(vb, x, y, z, w, o, ph, gid, G)
    ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G * K))
    beta = lambda: (ctx.glmm_beta_terms(*pt, *gh), ctx.glmm_beta_obs_influence(*pt, *gh, A, n0=3, n1=N - 2),
                    ctx.glmm_beta_group_influence(*pt, *gh, A))
    same = lambda a, b: _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    base = beta()
    assert same(beta(), base)                                            # two calls at one point
    trials = np.random.default_rng(3).integers(1, 9, size=N).astype(np.float64)
    for link, tr in ((1, None), (2, trials), (0, trials), (0, None)):
        ctx.set_link(link)
        ctx.set_trials(tr)
        assert same(beta(), base)
    # the resident sums of the new entry are what the Schur entry works on; lrvb_set_dispersion drops them
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    ctx.glmm_beta_terms(*pt, *gh)
    assert schur() == hip.OK
    ctx.set_dispersion(ph)
    assert schur() == hip.ERR_STATE
    assert same(beta(), base)
    # phi and logit(y) are read from the row's own entry: permuted ones give other numbers, the original ones the same bits again
    ctx.set_dispersion(ph[::-1].copy())
    assert not _same(ctx.glmm_beta_terms(*pt, *gh), base[0])
    # no dispersion, one of the wrong length
    val = np.empty(1)
    raw = lambda: ctx._lib.lrvb_glmm_beta_terms(ctx._h, pt[0].ctypes.data, pt[1].ctypes.data, P, pt[2].ctypes.data, pt[3].ctypes.data, G, K,
                                                gh[0].ctypes.data, gh[1].ctypes.data, gh[0].size, val.ctypes.data, None, None, None, 0)
    ctx.set_dispersion(None)
    assert raw() == hip.ERR_STATE
    with pytest.raises(Exception, match='no dispersion'):
        ctx.glmm_beta_terms(*pt, *gh)
    with pytest.raises(Exception, match='no dispersion'):
        ctx.glmm_beta_obs_influence(*pt, *gh, A)
    with pytest.raises(Exception, match='no dispersion'):
        ctx.glmm_beta_group_influence(*pt, *gh, A)
    ctx.set_dispersion(np.ones(N + 1))
    assert raw() == hip.ERR_STATE
    ctx.set_dispersion(ph)
    assert same(beta(), base)                                            # and the context goes on working
    # the logistic, Poisson, binomial, zero-truncated Poisson and NB2 entries give the same bits before and after a call of the new ones
    ctx.set_trials(trials)
    others = lambda: (ctx.glmm_slopes_terms(*pt, *gh), ctx.glmm_slopes_obs_influence(*pt, *gh, A), ctx.glmm_slopes_group_influence(*pt, *gh, A),
                      ctx.glmm_poisson_terms(*pt), ctx.glmm_poisson_obs_influence(*pt, A), ctx.glmm_poisson_group_influence(*pt, A),
                      ctx.glmm_binomial_terms(*pt, *gh), ctx.glmm_binomial_obs_influence(*pt, *gh, A), ctx.glmm_binomial_group_influence(*pt, *gh, A),
                      ctx.glmm_ztpoisson_terms(*pt, *gh), ctx.glmm_ztpoisson_obs_influence(*pt, *gh, A), ctx.glmm_ztpoisson_group_influence(*pt, *gh, A),
                      ctx.glmm_ztnegbin_terms(*pt, *gh), ctx.glmm_ztnegbin_obs_influence(*pt, *gh, A), ctx.glmm_ztnegbin_group_influence(*pt, *gh, A))
    before = others()
    assert same(beta(), base)
    after = others()
    assert all(_same(after[i], before[i]) for i in (0, 3, 6, 9, 12))
    assert all(np.array_equal(after[i], before[i]) for i in (1, 2, 4, 5, 7, 8, 10, 11, 13, 14))
    assert all(not _same(before[i], base[0]) for i in (0, 6, 9, 12))     # and they are other numbers
    assert vb._hip.load().lrvb_version() == 1


def test_refusals_by_error_code(vb):
    hip = vb._hip
    rng = np.random.default_rng(47)

    def context(N, P, dispersion=True):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)) / np.sqrt(P))
        ctx.set_data(hip.SLOT_Y, rng.normal(size=N))                     # logit(y)
        if dispersion:
            ctx.set_dispersion(rng.uniform(0.5, 40.0, size=N))
        return ctx

    def call(ctx, P, G, K, kind, nq=20, n0=0, n1=None):
        Kc = min(max(K, 1), 5)
        m, v, e, rr = np.zeros(P), np.ones(P), np.zeros(max(G * Kc, 1)), np.ones(max(G * Kc, 1))
        gx, gw = np.polynomial.hermite.hermgauss(min(nq, 128))
        gx, gw = np.resize(gx, nq), np.resize(gw, nq)
        head = (ctx._h, m.ctypes.data, v.ctypes.data, P, e.ctypes.data, rr.ctypes.data, G, K, gx.ctypes.data, gw.ctypes.data, nq)
        lib = ctx._lib
        n1 = ctx.n_obs if n1 is None else n1
        if kind == 'terms':
            val = np.empty(1)
            return lib.lrvb_glmm_beta_terms(*head, val.ctypes.data, None, None, None, 0)
        Q = 2
        Ag, Al = np.ones((Q, 2 * P)), np.ones((max(G, 1), 2 * Kc, Q))
        out = np.empty((5 * max(ctx.n_obs, G), Q))
        if kind == 'group':
            return lib.lrvb_glmm_beta_group_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, out.ctypes.data)
        return lib.lrvb_glmm_beta_obs_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, n0, n1, out.ctypes.data)

    N, G, K = 20, 3, 2
    gid = np.arange(N) % G
    for kind in ('terms', 'rows', 'group'):
        wide = context(N, 65)
        assert call(wide, 65, G, K, kind) == hip.ERR_UNSUPPORTED         # P = 65
        ctx = context(N, 3)
        ctx.set_groups(gid, G)
        ctx.set_group_design(np.ones((N, K)))
        assert call(ctx, 3, G, 5, kind) == hip.ERR_UNSUPPORTED           # K = 5
        assert call(ctx, 3, G, 0, kind) == hip.ERR_UNSUPPORTED           # K = 0
        assert call(ctx, 3, G, K, kind, nq=129) == hip.ERR_UNSUPPORTED   # 129 nodes
        ctx.set_offset(np.zeros(N + 1))
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # an offset of the wrong length
        ctx.set_offset(None)
        ctx.set_dispersion(np.ones(N + 1))
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # a dispersion of the wrong length
        ctx.set_dispersion(None)
        assert call(ctx, 3, G, K, kind) == hip.ERR_STATE                 # no dispersion
        ctx.set_dispersion(np.full(N, 2.5))
        if kind == 'rows':
            assert call(ctx, 3, G, K, kind, n0=5, n1=4) == hip.ERR_INVALID and call(ctx, 3, G, K, kind, n1=N + 1) == hip.ERR_INVALID
        assert call(ctx, 3, G, K, kind) == hip.OK
        assert call(ctx, 3, G, K, kind, nq=128) == hip.OK and call(ctx, 3, G, K, kind, nq=1) == hip.OK
    # the constructor: y outside (0, 1) and a dispersion that is not positive and finite are ValueErrors that name the rows
    x, z = np.ones((N, 2)), np.ones((N, K))
    for bad in (0.0, 1.0, np.nan):
        y = np.full(N, 0.4)
        y[5] = bad
        with pytest.raises(ValueError, match='1 of 20 rows'):
            vb.BetaGLMMObjective(_par(vb, 2, K, G), x, y, z, gid, G, 2.0)
    for phi in (0.0, -3.0, np.inf):
        with pytest.raises(ValueError, match='dispersion'):
            vb.BetaGLMMObjective(_par(vb, 2, K, G), x, np.full(N, 0.4), z, gid, G, phi)


def test_non_finite_point_is_refused_and_leaves_no_sums(vb):
    """A value that is not finite after the reduction (here: a NaN mean) is LRVB_ERR_INVALID, no sums stay resident, and the context
    goes on working."""
    hip = vb._hip
    N, P, K, G = 65, 5, 2, 3
    c = _case(vb, N, P, K, G)
    fun = _model(vb, c['x'], c['y'], c['z'], c['w'], c['o'], c['ph'], c['gid'], G, c['deg'])[1]      # a context of its own
    ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
    good = _point(c['eta'], P, K, G)
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    base = ctx.glmm_beta_terms(*good, *gh)
    assert np.isfinite(base[0]) and schur() == hip.OK
    bad = (np.where(np.arange(P) == 1, np.nan, good[0]),) + good[1:]
    with pytest.raises(ValueError, match='not finite'):
        ctx.glmm_beta_terms(*bad, *gh)
    assert schur() == hip.ERR_STATE                                      # no sums left resident
    assert _same(ctx.glmm_beta_terms(*good, *gh), base) and schur() == hip.OK


def test_extreme_points_are_accepted(vb):
    """No finite point is refused.  P = 1 with x = +-1 and a mean of 2000: rho_n = +-2000 + o_n, every node far in a tail, where
    h = |t| + lgamma(1 + phi) - 2 log phi - [t > 0] phi l, h' = +-1 and h'' = 0 hold to the last bit of fp64.  E |t| = |rho| on a
    symmetric rule, so value = sum w (|rho| + ..), d value / d m = sum w sign(rho) x and d value / d v = 0: to 1e-12."""
    from scipy.special import gammaln
    N, K, G = 70, 1, 3
    rng = np.random.default_rng(9)
    x = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None]
    y, ph, w, o = rng.uniform(0.05, 0.95, size=N), np.exp(rng.uniform(np.log(0.5), np.log(1e3), size=N)), rng.uniform(0.5, 1.5, size=N), rng.normal(size=N)
    y[0], y[1] = ref.PROBES[:2]
    gid = (np.arange(N) % G).astype(np.int32)
    _, fun = _model(vb, x, y, None, w, o, ph, gid, G, K=K)
    l = np.log(y) - np.log1p(-y)
    for sign in (1.0, -1.0):
        m, v, e, r = np.array([2000.0 * sign]), np.array([0.5]), np.zeros((G, K)), np.full((G, K), 0.7)
        rho = o + x[:, 0] * m[0]
        assert np.min(np.abs(rho)) > 1990.0
        val, gg, Hb, gs = fun.ctx.glmm_beta_terms(m, v, e, r, fun.gh_x, fun.gh_w)
        want = np.sum(w * (np.abs(rho) + gammaln(1.0 + ph) - 2.0 * np.log(ph) - np.where(rho > 0.0, ph * l, 0.0)))
        want_g = np.sum(w * np.sign(rho) * x[:, 0])
        print('extreme point', sign, abs(val - want) / abs(want), abs(gg[0] - want_g) / abs(want_g), gg[1])
        assert np.isfinite(val) and abs(val - want) <= 1e-12 * abs(want)
        assert abs(gg[0] - want_g) <= 1e-12 * abs(want_g) and abs(gg[1]) <= 1e-12 * abs(want_g)
        assert np.all(np.isfinite(Hb)) and np.all(np.isfinite(gs))


# ---- F: fit ------------------------------------------------------------------------------------------------------------------
def test_fit_covariance_and_tau_prior_sensitivity(vb):
    """The body and thresholds of tests/test_gpu_glmm_ztnegbin.py::test_fit_covariance_and_tau_prior_sensitivity."""
    N, P, K, G = 2000, 4, 2, 30
    x, y, z, w, gid, o, ph, free0 = ref.problem(N, P, K, G, 77, phi=20.0, big_group=False, empty_group=False)
    w = np.ones(N)
    par, fun = _model(vb, x, y, z, w, o, 20.0, gid, G)
    ng = 2 * P + 4 * K
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(free0.size))
    targs = ref.targs(x, y, z, w, o, ph, gid, G, HYP)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    print('reference gradient at the fit', np.max(np.abs(g_ad)))
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
    print('tau prior sensitivity', np.max(np.abs(sens @ h - diff)), np.max(np.abs(diff)))
    assert np.max(np.abs(sens @ h - diff)) < 0.05 * np.max(np.abs(diff)) + 1e-8

"""`TruncatedNegBinomialGLMMObjective` and `HurdleNegBinomialGLMM` on the GPU: the TruncNegBinLik
instantiations of the shared tile walk against the torch reference tests/glmm_ztnegbin_reference.py, the phi = 1 and large-mean
identities across classes, predictions, streamed influence, the state contract, the refusals, a fit and the composite.

Error measure and bounds are those of tests/test_gpu_glmm_ztpoisson.py: value 1e-11, gradient 1e-10, Hessian / products / Schur
complement 1e-9 relative; LRVB covariance and solves rtol 1e-6; influence rows 1e-9, group sums against the weighted rows 1e-10,
the dense cross Hessian 1e-9, quantities behind an H^-1 rtol 1e-6 with atol 1e-12; identities 1e-12 of the largest magnitude.

Shapes (N, P, K, G): (1, 1, 1, 1); (37, 3, 1, 5) with z=None, offset=None and a scalar phi; (65, 5, 2, 3) with 5 nodes -- a second
tile of one row, a cut group and an empty group; (130, 64, 4, 2); (300, 17, 4, 7) with every fifth weight zero.  phi = 1.7 at the
first three, one value per row on [0.05, 1e3] (phi[0] = 0.05, phi[1] = 1e3) at the last two.  Every data set with N >= 4 holds
y[0] = y[1] = 1 and y[2] = 57.  The reference free Hessian is positive definite at the off-optimum point of `problem` for these
draws (seed N + P + K; smallest eigenvalues 0.176, 0.226, 0.186, 0.223, 0.170, computed on the CPU, printed by the parity test and
recorded in DESIGN.md section 39), so every shape runs the covariance and solve checks.

Bounds that are this file's own.  Large mean: phi = 1e3 and an offset that puts every rho_n (shifted scale) at 10 or above; the
lowest of the 20 nodes then has eta >= 10 - 7.62 sqrt(s), v = phi softplus(eta) >= 80 at s <= 2.3 and g^(k) <= v'^k e^-v < 1e-25: the
test asserts on the CPU, for its own rows, that the REFERENCE's E H^(k) equal the NB2 ones to 1e-13 of each order's largest magnitude
before the two classes are compared.  Response means: phi exp(rho + s / 2) plus a sum of node terms in [0, 1] whose weights sum to
1, each good to a few ulp: 1e-12 relative to the mean (which is >= 1)."""
import numpy as np
import pytest
import torch

import glmm_ztnegbin_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _par, _eta, _point, _fit
from test_gpu_glmm_binomial import _prior_kw, _check_against_reference, _same, _nb_model, _model as _binomial_model
from test_gpu_glmm_link import _moments, _segment_sum

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
    x, y, z, w, gid, o, ph, free = ref.problem(N, P, K, G, N + P + K, phi='vector' if N >= 130 else 1.7, zero_weights=(N == 300))
    if bare:
        o = np.zeros(N)
        assert np.array_equal(z, np.ones((N, 1)))
    if N >= 130:
        assert ph.min() == 0.05 and ph.max() == 1e3
    return x, y, z, w, gid, o, ph, free, DEG.get((N, P, K, G), ref.GH_DEG), bare


def _model(vb, x, y, z, w, o, phi, gid, G, deg=ref.GH_DEG, hyp=HYP, K=None):
    par = _par(vb, x.shape[1], K if z is None else z.shape[1], G)
    return par, vb.TruncatedNegBinomialGLMMObjective(par, x, y, z, gid, G, phi, offset=o, weights=w, gh_deg=deg, **_prior_kw(hyp))


_cache = {}


def _case(vb, N, P, K, G):
    """The model at the point of `problem`, computed once per case."""
    key = (N, P, K, G)
    if key not in _cache:
        x, y, z, w, gid, o, ph, free, deg, bare = _data(N, P, K, G)
        par, fun = _model(vb, x, y, None if bare else z, w, None if bare else o, 1.7 if bare else ph, gid, G, deg, K=K)
        _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, o=o, ph=ph, free=free, deg=deg, eta=_eta(free, P, K, G), par=par, fun=fun,
                           targs=ref.targs(x, y, z, w, o, ph, gid, G, HYP, deg))
    return _cache[key]


def _hf(c):
    """The reference free Hessian of a case, computed once (the parity test leaves its own here)."""
    if 'Hf' not in c:
        c['Hf'] = ref.value_grad_hess(ref.kl_free, c['free'], c['targs'])[2]
    return c['Hf']


def _largest(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(a)), np.max(np.abs(b))))


# ---- A: the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_reference_parity(vb, N, P, K, G):
    c = _case(vb, N, P, K, G)
    y, w, gid = c['y'], c['w'], c['gid']
    assert np.all(y >= 1.0) and y[0] == 1.0
    if N >= 4:
        assert y[1] == 1.0 and y[2] == 57.0                              # rows at the truncation point and a large count
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2     # an empty group, one with more than half the rows
    if N == 300:
        assert np.sum(w == 0.0) == 60
    assert c['fun'].gh_x.size == c['deg']
    _, Hf = _check_against_reference(c['par'], c['fun'], ref.kl_vec, ref.kl_free, c['targs'], c['free'], G, K, solves=True)
    c['Hf'] = Hf
    print('smallest eigenvalue of the reference free Hessian', (N, P, K, G), float(np.min(np.linalg.eigvalsh(Hf))))
    from scipy.special import gammaln
    ph = c['ph']
    assert abs(c['fun'].log_norm_const() - np.sum(w * (gammaln(y + ph) - gammaln(ph) - gammaln(y + 1.0)))) < 1e-9
    # two evaluations at one point are bitwise equal (through a model of its own: a direct call of the terms entry on a shared
    # context would drop the factor the class believes resident)
    other = _model(vb, c['x'], c['y'], c['z'], c['w'], c['o'], c['ph'], c['gid'], G, c['deg'])[1]
    pt = _point(c['eta'], P, K, G) + (other.gh_x, other.gh_w)
    assert _same(other.ctx.glmm_ztnegbin_terms(*pt), other.ctx.glmm_ztnegbin_terms(*pt))


# ---- B: identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_phi_one_identity_across_three_classes(vb, N, P, K, G):
    """phi = 1, one shared point, counts with zeros: the data term of the NB2 model on all rows is that of the logit Bernoulli
    model on 1[y > 0] over all rows plus that of the zero-truncated model on the rows with y > 0 -- value, gradient, H blocks and
    group sums of the three `*_terms` entries; at the point of `problem` and with every variance times 30."""
    c = _case(vb, N, P, K, G)
    x, z, w, gid, o, deg = (c[k] for k in ('x', 'z', 'w', 'gid', 'o', 'deg'))
    y = c['y'].copy()
    y[3::3] = 0.0
    pos = np.flatnonzero(y > 0.0)
    assert 0 < pos.size < N and y[2] == 57.0 and np.any(y == 1.0)
    _, nb = _nb_model(vb, x, y, z, w, o, 1.0, gid, G)
    _, zero = _binomial_model(vb, x, (y > 0.0).astype(np.float64), z, w, o, None, gid, G)
    _, count = _model(vb, x[pos], y[pos], z[pos], w[pos], o[pos], 1.0, gid[pos], G, deg)
    m, v, e, r = _point(c['eta'], P, K, G)
    for widen in (1.0, 30.0):
        pt = (m, v * widen, e, r * widen)
        gh = (zero.gh_x, zero.gh_w)
        a = nb.ctx.glmm_binomial_terms(*pt, *gh)
        b, d = zero.ctx.glmm_binomial_terms(*pt, *gh), count.ctx.glmm_ztnegbin_terms(*pt, *gh)
        s = (x * x) @ pt[1] + np.sum(z * z * pt[3][gid], axis=1)
        errs = [abs(a[0] - (b[0] + d[0])) / abs(a[0])] + [_largest(a[i], b[i] + d[i]) for i in (1, 2, 3)]
        print('phi = 1 identity', (N, P, K, G), 'variances x', widen, 'largest s', float(s.max()), errs)
        assert max(errs) <= IDENT
    assert s.max() > 30.0


@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_phi_one_is_the_binomial_model_with_y_trials(vb, N, P, K, G):
    """phi = 1: H = y sp - (y - 1) eta, the binomial term with y trials and y - 1 successes."""
    c = _case(vb, N, P, K, G)
    x, y, z, w, gid, o, eta, deg = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'o', 'eta', 'deg'))
    _, fun = _model(vb, x, y, z, w, o, 1.0, gid, G, deg)
    _, bino = _binomial_model(vb, x, y - 1.0, z, w, o, y, gid, G)
    a = (fun.value(eta, False), fun.grad(eta, False), fun.hessian(eta, False))
    b = (bino.value(eta, False), bino.grad(eta, False), bino.hessian(eta, False))
    errs = [abs(a[0] - b[0]) / abs(b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2])]
    print('phi = 1 against binomial(y, y - 1)', (N, P, K, G), errs)
    assert max(errs) <= IDENT


@pytest.mark.parametrize('N,P,K,G', IDENT_SHAPES)
def test_large_mean_is_the_negative_binomial_model(vb, N, P, K, G):
    """phi = 1e3 and an offset that puts every shifted rho_n at 10 or above: P(y = 0) is below 1e-34 on every node, the truncation
    no longer matters and the class equals `NegBinomialGLMMObjective` on the same data.  First the reference alone, on the CPU
    and for these rows."""
    c = _case(vb, N, P, K, G)
    x, y, z, w, gid, eta, deg = (c[k] for k in ('x', 'y', 'z', 'w', 'gid', 'eta', 'deg'))
    phi = 1e3
    m, v, e, r = _point(eta, P, K, G)
    lin = x @ m + np.sum(z * e[gid], axis=1)
    o = c['o'] + (10.0 + np.log(phi) - np.min(c['o'] + lin))             # the raw offset
    rho, s = o - np.log(phi) + lin, (x * x) @ v + np.sum(z * z * r[gid], axis=1)
    assert rho.min() >= 10.0 - 1e-12 and s.max() <= 2.3
    eh, nb = ref.eh_coefs(rho, s, y, phi, deg), ref.nb_coefs(rho, s, y, phi, deg)
    e_ref = float(np.max(np.max(np.abs(eh - nb), axis=1) / np.max(np.abs(nb), axis=1)))
    print('large mean, reference alone', (N, P, K, G), e_ref)
    assert e_ref <= 1e-13
    _, fun = _model(vb, x, y, z, w, o, phi, gid, G, deg)
    _, neg = _nb_model(vb, x, y, z, w, o, phi, gid, G)
    a = (fun.value(eta, False), fun.grad(eta, False), fun.hessian(eta, False))
    b = (neg.value(eta, False), neg.grad(eta, False), neg.hessian(eta, False))
    errs = [abs(a[0] - b[0]) / abs(b[0]), rel_err(a[1], b[1]), rel_err(a[2], b[2])]
    print('large mean against NB2', (N, P, K, G), errs)
    assert max(errs) <= IDENT and fun.log_norm_const() == neg.log_norm_const()


# ---- C: predictions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,G', [(65, 5, 2, 3), (130, 64, 4, 2)])
def test_predict_window_and_new_rows(vb, N, P, K, G):
    """Both routes; a window no tile boundary aligns with and new rows, some at the population level (group -1).  Then the device
    entry alone with every variance times 30: there the 20-node sum of e^t is off by percents (tests/test_glmm_ztnegbin_host_math.py)
    and only a mean whose e^t part is the closed form meets the reference."""
    c = _case(vb, N, P, K, G)
    fun, free, x, z, gid, deg, ph = c['fun'], c['free'], c['x'], c['z'], c['gid'], c['deg'], c['ph']
    Hf = _hf(c)
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    Hinv = np.linalg.inv(Hf)
    rng = np.random.default_rng([N, 37])
    n_new = 70
    new = dict(x=rng.normal(size=(n_new, P)) / np.sqrt(P), z=np.concatenate([np.ones((n_new, 1)), 0.5 * rng.normal(size=(n_new, K - 1))], axis=1),
               groups=rng.integers(0, G, size=n_new), offset=0.3 * rng.normal(size=n_new),
               dispersion=np.exp(rng.uniform(np.log(0.05), np.log(1e3), size=n_new)))
    new['groups'][::9] = -1
    n0, n1 = 3, N - 2
    for what, kw, Cm, off, phi in (('window', dict(n0=n0, n1=n1), _moments(x[n0:n1], z[n0:n1], gid[n0:n1], P, K, G), c['o'][n0:n1], ph[n0:n1]),
                                   ('new rows', dict(newdata=new), _moments(new['x'], new['z'], new['groups'], P, K, G), new['offset'],
                                    new['dispersion'])):
        want_var = np.einsum('nd,de,ne->n', Cm, Hinv, Cm)
        want_rho = off + Cm @ free                                       # the means are free coordinates themselves; the RAW offset
        outs = [fun.predict(free, on_device=dev, **kw) for dev in (False, True)]
        for route, out in zip(('host', 'device'), outs):
            assert np.allclose(out['rho'], want_rho, rtol=1e-12, atol=1e-12)
            assert np.allclose(out['var_lrvb'], want_var, rtol=1e-6, atol=0)
            for col, var in (('mean_mf', 'var_mf'), ('mean_lrvb', 'var_lrvb')):
                want = ref.response_mean(out['rho'] - np.log(phi), out[var], phi, deg)
                err = np.abs(out[col] - want) / want
                print('predict', (N, P, K, G), what, route, col, float(np.max(err)))
                assert out[col].shape == want.shape and np.all(want >= 1.0) and np.all(err <= 1e-12)
                assert np.all(out[col] > np.exp(out['rho'] + 0.5 * out[var]))      # the truncated mean exceeds the NB2 one
        assert np.allclose(outs[1]['var_lrvb'], outs[0]['var_lrvb'], rtol=1e-6, atol=0)
    # a window equals the same rows of the full result bitwise
    full = fun.predict(free, on_device=True)
    win = fun.predict(free, n0=n0, n1=n1, on_device=True)
    assert all(np.array_equal(win[k], full[k][n0:n1]) for k in full)
    # per-row phi: new rows without a dispersion are refused; an unknown key too
    with pytest.raises(ValueError, match='dispersion'):
        fun.predict(free, newdata={k: a for k, a in new.items() if k != 'dispersion'})
    with pytest.raises(ValueError, match='trials'):
        fun.predict(free, newdata=dict(new, trials=np.ones(n_new)))
    # variances times 30, on the entry itself (the group covariance of the call above is resident)
    cb = fun.group_cov(free, on_device=True)[0]
    fun.predict(free, on_device=True)
    m, v, e, r = _point(c['eta'], P, K, G)
    e2, r2 = np.vstack([e, np.zeros((1, K))]), np.vstack([r, np.ones((1, K))])
    gidn = np.where(new['groups'] < 0, G, new['groups'])
    for rows, xx, zz, gg, off, phi in ((dict(n0=n0, n1=n1), x[n0:n1], z[n0:n1], gid[n0:n1], c['o'][n0:n1], ph[n0:n1]),
                                       (dict(new=(new['x'], new['z'], gidn, new['offset'] - np.log(new['dispersion']), new['dispersion'])),
                                        new['x'], new['z'], gidn, new['offset'], new['dispersion'])):
        out = fun.ctx.glmm_ztnegbin_predict(m, 30.0 * v, e2, 30.0 * r2, fun.gh_x, fun.gh_w, cb, **rows)
        rho = off - np.log(phi) + xx @ m + np.sum(zz * e2[gg], axis=1)
        s30 = 30.0 * ((xx * xx) @ v + np.sum(zz * zz * r2[gg], axis=1))
        assert np.allclose(out[0], rho, rtol=1e-12, atol=1e-12) and np.allclose(out[1], s30, rtol=1e-12, atol=0) and s30.max() > 20.0
        for col, var in ((3, 1), (4, 2)):
            want = ref.response_mean(out[0], out[var], phi, deg)
            err = np.abs(out[col] - want) / want
            nodes = ref.response_mean(out[0], out[var], phi, deg, closed=False)
            print('predict, variances x 30', (N, P, K, G), col, float(np.max(err)), 'e^t on the nodes would give', float(np.max(np.abs(nodes - want) / want)))
            assert np.all(err <= 1e-12)
            if col == 3:
                assert np.max(np.abs(nodes - want) / want) > 1e-2


def test_overflowing_predict_mean_is_a_value_error(vb):
    """phi exp(rho + s / 2) is not clamped: new rows with an offset of 800 have no finite mean, on either route; with 600 they do."""
    N, P, K, G = 65, 5, 2, 3
    c = _case(vb, N, P, K, G)
    fun = c['fun']
    new = dict(x=c['x'][:4], z=c['z'][:4], groups=c['gid'][:4], offset=np.array([0.0, 600.0, 0.0, 600.0]), dispersion=1.7)
    for dev in (False, True):
        out = fun.predict(c['free'], newdata=new, on_device=dev)
        assert np.all(np.isfinite(out['mean_lrvb'])) and out['mean_mf'][1] > 1e200
        with pytest.raises(ValueError, match='overflows'):
            fun.predict(c['free'], newdata=dict(new, offset=np.array([0.0, 800.0, 0.0, 0.0])), on_device=dev)


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
        got = fun.ctx.glmm_ztnegbin_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        win = fun.ctx.glmm_ztnegbin_obs_influence(*pt, A[:Q], n0=3, n1=N - 2)
        assert win.shape == (N - 5, Q) and np.array_equal(win, got[3:N - 2])
    rows = fun.ctx.glmm_ztnegbin_obs_influence(*pt, A)
    a, b = fun.ctx.glmm_ztnegbin_group_influence(*pt, A), fun.ctx.glmm_ztnegbin_group_influence(*pt, A)
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
    """`set_dispersion` drops the resident sums, a missing dispersion is LRVB_ERR_STATE, and the new entries read neither
    lrvb_set_link nor lrvb_set_trials and leave the other likelihoods' entries alone."""
    hip = vb._hip
    N, P, K, G = 130, 4, 2, 5
    x, y, z, w, gid, o, ph, free = ref.problem(N, P, K, G, 31, phi='vector', empty_group=False)
    pt = _point(_eta(free, P, K, G), P, K, G)
    _, fun = _model(vb, x, y, z, w, o, ph, gid, G)
    ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
    A = np.random.default_rng(2).normal(size=(5, 2 * P + 2 * G * K))
    ztnb = lambda: (ctx.glmm_ztnegbin_terms(*pt, *gh), ctx.glmm_ztnegbin_obs_influence(*pt, *gh, A, n0=3, n1=N - 2),
                    ctx.glmm_ztnegbin_group_influence(*pt, *gh, A))
    same = lambda a, b: _same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    base = ztnb()
    assert same(ztnb(), base)                                            # two calls at one point
    trials = np.random.default_rng(3).integers(1, 9, size=N).astype(np.float64)
    for link, tr in ((1, None), (2, trials), (0, trials), (0, None)):
        ctx.set_link(link)
        ctx.set_trials(tr)
        assert same(ztnb(), base)
    # the resident sums of the new entry are what the Schur entry works on; lrvb_set_dispersion drops them
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    ctx.glmm_ztnegbin_terms(*pt, *gh)
    assert schur() == hip.OK
    ctx.set_dispersion(ph)
    assert schur() == hip.ERR_STATE
    assert same(ztnb(), base)
    # phi is read from the row's own entry: a permuted dispersion gives other numbers, the original one the same bits again
    ctx.set_dispersion(ph[::-1].copy())
    assert not _same(ctx.glmm_ztnegbin_terms(*pt, *gh), base[0])
    # no dispersion, one of the wrong length, values that are not positive and finite
    val = np.empty(1)
    raw = lambda: ctx._lib.lrvb_glmm_ztnegbin_terms(ctx._h, pt[0].ctypes.data, pt[1].ctypes.data, P, pt[2].ctypes.data, pt[3].ctypes.data, G, K,
                                                    gh[0].ctypes.data, gh[1].ctypes.data, gh[0].size, val.ctypes.data, None, None, None, 0)
    ctx.set_dispersion(None)
    assert raw() == hip.ERR_STATE
    with pytest.raises(Exception, match='no dispersion'):
        ctx.glmm_ztnegbin_terms(*pt, *gh)
    ctx.set_dispersion(np.ones(N + 1))
    assert raw() == hip.ERR_STATE
    for bad in (0.0, -1.0, np.nan, np.inf):
        d = ph.copy()
        d[7] = bad
        assert ctx._lib.lrvb_set_dispersion(ctx._h, d.ctypes.data, N) == hip.ERR_INVALID
    assert ctx._lib.lrvb_set_dispersion(ctx._h, ph.ctypes.data, 0) == hip.ERR_SIZE
    ctx.set_dispersion(ph)
    assert same(ztnb(), base)
    # the logistic, Poisson, binomial and zero-truncated Poisson entries give the same bits before and after a call of the new ones
    ctx.set_trials(trials)
    others = lambda: (ctx.glmm_slopes_terms(*pt, *gh), ctx.glmm_slopes_obs_influence(*pt, *gh, A), ctx.glmm_slopes_group_influence(*pt, *gh, A),
                      ctx.glmm_poisson_terms(*pt), ctx.glmm_poisson_obs_influence(*pt, A), ctx.glmm_poisson_group_influence(*pt, A),
                      ctx.glmm_binomial_terms(*pt, *gh), ctx.glmm_binomial_obs_influence(*pt, *gh, A), ctx.glmm_binomial_group_influence(*pt, *gh, A),
                      ctx.glmm_ztpoisson_terms(*pt, *gh), ctx.glmm_ztpoisson_obs_influence(*pt, *gh, A), ctx.glmm_ztpoisson_group_influence(*pt, *gh, A))
    before = others()
    assert same(ztnb(), base)
    after = others()
    assert all(_same(after[i], before[i]) for i in (0, 3, 6, 9))
    assert all(np.array_equal(after[i], before[i]) for i in (1, 2, 4, 5, 7, 8, 10, 11))
    assert not _same(before[6], base[0]) and not _same(before[9], base[0])     # and they are other numbers
    assert vb._hip.load().lrvb_version() == 1


def test_refusals_by_error_code(vb):
    hip = vb._hip
    rng = np.random.default_rng(47)

    def context(N, P):
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2 * P, vec_size=2 * P, dim0=2 * P, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=P)
        ctx.set_data(hip.SLOT_X, rng.normal(size=(N, P)) / np.sqrt(P))
        ctx.set_data(hip.SLOT_Y, 1.0 + rng.poisson(2.0, size=N).astype(np.float64))
        ctx.set_dispersion(rng.uniform(0.5, 4.0, size=N))
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
            return lib.lrvb_glmm_ztnegbin_terms(*head, val.ctypes.data, None, None, None, 0)
        Q = 2
        Ag, Al = np.ones((Q, 2 * P)), np.ones((max(G, 1), 2 * Kc, Q))
        out = np.empty((5 * max(ctx.n_obs, G), Q))
        if kind == 'group':
            return lib.lrvb_glmm_ztnegbin_group_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, out.ctypes.data)
        if kind == 'rows':
            return lib.lrvb_glmm_ztnegbin_obs_influence(*head, Ag.ctypes.data, Al.ctypes.data, Q, n0, n1, out.ctypes.data)
        Sbb = np.eye(P)
        return lib.lrvb_glmm_ztnegbin_predict(*head, Sbb.ctypes.data, n0, n1, None, None, None, None, None, 0, out.ctypes.data)

    N, G, K = 20, 3, 2
    gid = np.arange(N) % G
    for kind in ('terms', 'rows', 'group', 'predict'):
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
        if kind == 'rows':
            assert call(ctx, 3, G, K, kind, n0=5, n1=4) == hip.ERR_INVALID and call(ctx, 3, G, K, kind, n1=N + 1) == hip.ERR_INVALID
        if kind != 'predict':
            assert call(ctx, 3, G, K, kind) == hip.OK
            assert call(ctx, 3, G, K, kind, nq=128) == hip.OK and call(ctx, 3, G, K, kind, nq=1) == hip.OK
        else:
            assert call(ctx, 3, G, K, kind) == hip.ERR_STATE             # no group covariance resident


def test_underflow_is_refused_and_leaves_no_sums(vb):
    """No clamp: a point where phi softplus(eta) underflows to 0 on a node (rho = -2000 sum_j |x_0j| < -800) is a ValueError, no
    sums stay resident, and the context goes on working."""
    hip = vb._hip
    N, P, K, G = 65, 5, 2, 3
    c = _case(vb, N, P, K, G)
    eta = c['eta']
    fun = _model(vb, c['x'], c['y'], c['z'], c['w'], c['o'], c['ph'], c['gid'], G, c['deg'])[1]      # a context of its own
    ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
    good = _point(eta, P, K, G)
    loc = np.tile(np.eye(2 * K)[np.triu_indices(2 * K)], (G, 1))
    sc, cl, M = np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)), np.empty((2 * P + 3 * K, 2 * P + 3 * K))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, G, K, M.ctypes.data)
    base = ctx.glmm_ztnegbin_terms(*good, *gh)
    assert np.isfinite(base[0]) and schur() == hip.OK
    assert 2000.0 * np.sum(np.abs(c['x'][0])) > 800.0 + np.max(np.abs(c['o'])) + np.log(1.7) + 50.0
    bad = eta.copy()
    bad[:P] = -2000.0 * np.sign(c['x'][0])
    with pytest.raises(ValueError, match='not finite'):
        ctx.glmm_ztnegbin_terms(*_point(bad, P, K, G), *gh)
    assert schur() == hip.ERR_STATE                                      # no sums left resident
    with pytest.raises(ValueError, match='not finite'):
        fun.value(bad, False)
    assert _same(ctx.glmm_ztnegbin_terms(*good, *gh), base) and schur() == hip.OK
    assert np.isfinite(fun.value(eta, False))


# ---- F: fit ------------------------------------------------------------------------------------------------------------------
def test_fit_covariance_and_tau_prior_sensitivity(vb):
    """The body and thresholds of tests/test_gpu_glmm_ztpoisson.py::test_fit_covariance_and_tau_prior_sensitivity."""
    N, P, K, G = 2000, 4, 2, 30
    x, y, z, w, gid, o, ph, free0 = ref.problem(N, P, K, G, 77, phi=1.7, big_group=False, empty_group=False)
    w = np.ones(N)
    assert np.all(y >= 1.0) and np.any(y == 1.0)
    par, fun = _model(vb, x, y, z, w, o, 1.7, gid, G)
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


# ---- G: the composite ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero_link', ['logit', 'cloglog'])
def test_hurdle_composite(vb, zero_link):
    """`HurdleNegBinomialGLMM` with one phi per row of the whole data: its parts (phi subset to the positive rows), `value` as their
    sum, and `predict` -- the mean is the product of the parts' means under both variances and on both routes, over a window (zeros
    included) and over new rows."""
    N, P, K, G = 65, 5, 2, 3
    x, y, z, w, gid, o, _, free, _, _ = _data(N, P, K, G)
    ph = np.exp(np.random.default_rng(8).uniform(np.log(0.05), np.log(1e3), size=N))
    y = y.copy()
    y[3::3] = 0.0
    pos = np.flatnonzero(y > 0.0)
    par_z, par_c = _par(vb, P, K, G), _par(vb, P, K, G)
    hur = vb.HurdleNegBinomialGLMM(par_z, par_c, x, y, z, gid, G, ph, offset=o, zero_link=zero_link, weights=w, **_prior_kw(HYP))
    assert np.array_equal(hur.positive_rows, pos) and hur.count.n_obs == pos.size and hur.zero.n_obs == N
    assert hur.zero.link == zero_link and hur.count.G == hur.zero.G == G
    assert isinstance(hur.count, vb.TruncatedNegBinomialGLMMObjective) and np.array_equal(hur.count._phi, ph[pos])
    th_z, th_c = free, free + 0.05
    par_b = _par(vb, P, K, G)
    zero = vb.BinomialGLMMObjective(par_b, x, (y > 0.0).astype(np.float64), z, gid, G, weights=w, link=zero_link, **_prior_kw(HYP))
    _, count = _model(vb, x[pos], y[pos], z[pos], w[pos], o[pos], ph[pos], gid[pos], G)
    assert hur.value(th_z, th_c) == zero.value(th_z, True) + count.value(th_c, True)
    assert hur.log_norm_const() == count.log_norm_const()
    rng = np.random.default_rng(5)
    new = dict(x=rng.normal(size=(9, P)) / np.sqrt(P), z=np.concatenate([np.ones((9, 1)), 0.5 * rng.normal(size=(9, K - 1))], axis=1),
               groups=np.array([0, 1, -1, 0, 1, 1, -1, 0, 0]), offset=0.2 * rng.normal(size=9), dispersion=rng.uniform(0.1, 9.0, size=9))
    for kw, n, rows in ((dict(n0=2, n1=N - 3), N - 5, dict(x=x[2:N - 3], z=z[2:N - 3], groups=gid[2:N - 3], offset=o[2:N - 3],
                                                            dispersion=ph[2:N - 3])),
                        (dict(newdata=new), 9, new)):
        outs = [hur.predict(th_z, th_c, on_device=dev, **kw) for dev in (False, True)]
        pz = zero.predict(th_z, newdata=dict(x=rows['x'], z=rows['z'], groups=rows['groups']))
        pc = count.predict(th_c, newdata=rows)
        for out in outs:
            for v in ('mf', 'lrvb'):
                assert out['mean_' + v].shape == (n,)
                assert np.array_equal(out['mean_' + v], out['p_pos_' + v] * out['mean_count_' + v])
                assert np.all((out['p_pos_' + v] > 0.0) & (out['p_pos_' + v] < 1.0)) and np.all(out['mean_count_' + v] > 1.0)
            assert np.allclose(out['p_pos_lrvb'], pz['mean_lrvb'], rtol=1e-6, atol=0)
            assert np.allclose(out['mean_count_lrvb'], pc['mean_lrvb'], rtol=1e-6, atol=0)
            assert np.allclose(out['p_pos_mf'], pz['mean_mf'], rtol=1e-12, atol=0)
            assert np.allclose(out['mean_count_mf'], pc['mean_mf'], rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match='dispersion'):
        hur.predict(th_z, th_c, newdata={k: a for k, a in new.items() if k != 'dispersion'})
    # a scalar phi needs none
    hur1 = vb.HurdleNegBinomialGLMM(_par(vb, P, K, G), _par(vb, P, K, G), x, y, z, gid, G, 1.7, offset=o, zero_link=zero_link, weights=w,
                                    **_prior_kw(HYP))
    out = hur1.predict(th_z, th_c, newdata={k: a for k, a in new.items() if k != 'dispersion'})
    assert out['mean_mf'].shape == (9,) and np.all(np.isfinite(out['mean_lrvb']))

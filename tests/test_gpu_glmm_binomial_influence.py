"""Streamed weight influence of `BinomialGLMMObjective` and `NegBinomialGLMMObjective`: the row entry
`lrvb_glmm_binomial_obs_influence`, the group entry `lrvb_glmm_binomial_group_influence`, the routes behind `obs_influence` /
`group_influence`, the `stream_hyper=True` rows and the dense weight `cross_hessian`, against torch autograd of
tests/glmm_binomial_reference.py.  Tolerances are those of tests/test_gpu_glmm_poisson_influence.py for the same quantities:
influence rows 1e-9 relative, group sums against the weighted sums of the rows 1e-10, the dense cross Hessian 1e-9, quantities
behind an H^-1 rtol 1e-6 with atol 1e-12.  The three shapes are those at which the reference Hessian is positive definite at the
point of `problem` (tests/test_gpu_glmm_binomial.py), so the routes behind H^-1 are checked there, off the optimum: the identities
they implement do not need one."""
import numpy as np
import pytest
import torch

import glmm_binomial_reference as ref
from helpers import rel_err
from test_gpu_glmm_slopes import HYP, _eta, _point
from test_gpu_glmm_binomial import _model, _nb_model

pytestmark = pytest.mark.gpu

SHAPES = [(37, 3, 2, 5), (65, 5, 2, 3), (130, 64, 4, 2)]
CASES = [s + (kind,) for s in SHAPES for kind in ('binomial', 'negbinomial')]


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


_cache = {}


def _case(vb, N, P, K, G, kind):
    """The model, its reference functions and their autograd results at the point of `problem`, computed once per case."""
    key = (N, P, K, G, kind)
    if key in _cache:
        return _cache[key]
    if kind == 'binomial':
        x, y, z, w, gid, o, aux, free = ref.problem(N, P, K, G, seed=N + P + K)
        par, fun = _model(vb, x, y, z, w, o, aux, gid, G)
        kl_vec, kl_free = ref.kl_vec, ref.kl_free
    else:
        seed = 23 if (N, P, K, G) == (37, 3, 2, 5) else N + P + K
        x, y, z, w, gid, o, aux, free = ref.nb_problem(N, P, K, G, seed=seed, phi='vector')
        par, fun = _nb_model(vb, x, y, z, w, o, aux, gid, G)
        kl_vec, kl_free = ref.nb_kl_vec, ref.nb_kl_free
    t = ref.tensors(x, y, z, w, o, aux, gid, HYP)
    eta = _eta(free, P, K, G)
    ng, GK = 2 * P + 4 * K, G * K
    # d / d w of the gradient in (m, v, e, r): N x (2 P + 2 G K)
    c = torch.tensor(np.concatenate([eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + GK], 1.0 / eta[ng + GK:]]), requires_grad=True)
    wt = t[3].clone().requires_grad_(True)
    et = torch.cat([c[:P], 1.0 / c[P:2 * P], torch.tensor(eta[2 * P:ng]), c[2 * P:2 * P + GK], 1.0 / c[2 * P + GK:]])
    g, = torch.autograd.grad(kl_vec(et, t[0], t[1], t[2], wt, t[4], t[5], t[6], G, t[7]), c, create_graph=True)
    rows_mv = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())], axis=1)
    # the free-coordinate Hessian and weight cross Hessian
    wt2 = t[3].clone().requires_grad_(True)
    p = torch.tensor(free).requires_grad_(True)
    gf, = torch.autograd.grad(kl_free(p, t[0], t[1], t[2], wt2, t[4], t[5], t[6], G, t[7]), p, create_graph=True)
    Cw = np.stack([torch.autograd.grad(gf[k], wt2, retain_graph=True)[0].numpy() for k in range(gf.numel())])
    _, _, Hf = ref.value_grad_hess(kl_free, free, t[:7] + (G, t[7]))
    assert np.min(np.linalg.eigvalsh(Hf)) > 0
    _cache[key] = dict(x=x, y=y, z=z, w=w, gid=gid, free=free, eta=eta, par=par, fun=fun, rows_mv=rows_mv, Cw=Cw, Hf=Hf)
    return _cache[key]


def _segment_sum(gid, G, v):
    out = np.zeros((G,) + v.shape[1:])
    np.add.at(out, gid, v)
    return out


@pytest.mark.parametrize('N,P,K,G,kind', CASES)
def test_rows_windows_and_group_sums_against_autograd(vb, N, P, K, G, kind):
    c = _case(vb, N, P, K, G, kind)
    fun, w, gid = c['fun'], c['w'], c['gid']
    pt = _point(c['eta'], P, K, G) + (fun.gh_x, fun.gh_w)
    A = np.random.default_rng(N).normal(size=(21, 2 * P + 2 * G * K))
    want = c['rows_mv'] @ A.T                                            # N x 21
    for Q in (1, 5, 16, 21):                                             # 21 crosses the 16-column MFMA block
        got = fun.ctx.glmm_binomial_obs_influence(*pt, A[:Q])
        e = rel_err(got, want[:, :Q])
        print('rows', kind, N, P, K, G, Q, e)
        assert got.shape == (N, Q) and e < 1e-9
        for n0, n1 in ((5, 700), (N // 3, N // 3 + 1), (63, 129), (N, N), (0, 0)):      # windows no tile boundary aligns with
            n0, n1 = min(n0, N), min(n1, N)
            win = fun.ctx.glmm_binomial_obs_influence(*pt, A[:Q], n0=n0, n1=n1)
            assert win.shape == (n1 - n0, Q) and np.array_equal(win, got[n0:n1])
    rows = fun.ctx.glmm_binomial_obs_influence(*pt, A)
    a, b = fun.ctx.glmm_binomial_group_influence(*pt, A), fun.ctx.glmm_binomial_group_influence(*pt, A)
    e = rel_err(a, _segment_sum(gid, G, w[:, None] * rows))
    print('group sums', kind, N, P, K, G, e)
    assert a.shape == (G, 21) and e < 1e-10
    assert rel_err(a, _segment_sum(gid, G, w[:, None] * want)) < 1e-9   # and against autograd directly
    assert np.array_equal(a, b)                                           # bitwise reproducible
    if G >= 3:
        assert not np.any(gid == G - 1) and np.all(a[G - 1] == 0.0)      # the empty group


@pytest.mark.parametrize('N,P,K,G,kind', CASES)
def test_routes_stream_hyper_and_dense_cross_hessian(vb, N, P, K, G, kind):
    c = _case(vb, N, P, K, G, kind)
    fun, par, free, w, gid = c['fun'], c['par'], c['free'], c['w'], c['gid']
    D = 2 * P + 4 * K + 2 * G * K
    want = -np.linalg.solve(c['Hf'], c['Cw']).T                           # N x D
    rows = fun.obs_influence(free, np.eye(D))
    print('arrow route', kind, rel_err(rows, want))
    assert np.allclose(rows, want, rtol=1e-6, atol=1e-12)
    rows_dev = fun.obs_influence(free, np.eye(D), on_device=True)
    assert np.allclose(rows_dev, rows, rtol=1e-6, atol=1e-12)
    gi = fun.group_influence(free, np.eye(D))
    assert np.allclose(fun.group_influence(free, np.eye(D), on_device=True), gi, rtol=1e-6, atol=1e-12)
    assert np.allclose(gi, _segment_sum(gid, G, w[:, None] * want), rtol=1e-6, atol=1e-12)
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, free, w, stream_hyper=True)
    dense = lin.get_doutput_dhyper_rows(np.eye(D))
    print('dense factor route against the arrow route', rel_err(dense, rows))
    assert np.allclose(dense, want, rtol=1e-6, atol=1e-12)
    n0, n1 = 7, min(N - 1, 100)
    win = lin.get_doutput_dhyper_rows(np.eye(D)[:3], n0=n0, n1=n1)
    assert np.allclose(win, want[n0:n1, :3], rtol=1e-6, atol=1e-12)
    # the dense weight cross Hessian (small-N protocol) takes m psi' from the likelihood, offset included
    C = fun.cross_hessian(fun.weights_par, free, True)
    assert C.shape == (D, N) and rel_err(C, c['Cw']) < 1e-9

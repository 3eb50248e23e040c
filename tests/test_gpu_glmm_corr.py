"""`LogisticGLMMCorrObjective` / `PoissonGLMMCorrObjective` (mixed models with correlated random effects, a Wishart precision
and a block-arrow Hessian with a DENSE closed border) and the four device entries under them
(lrvb_glmm_arrow_schur / _solve_forward / _solve_back / _group_cov) on the GPU against the torch reference
tests/glmm_corr_reference.py.

Tolerances are those of the tests of the independent-effects classes for the same quantities: value 1e-11, gradient 1e-10,
Hessian, products and Schur complement 1e-9 relative (tests/test_gpu_glmm_slopes.py); the two routes of the solve by backward
error, eta_dev <= 8 eta_host + D 2^-53, and the doubled first-order forward bound (tests/test_gpu_glmm_slopes_device_solve.py);
group blocks and row variances err_dev <= 8 err_host + kappa_2(H) D 2^-53 (tests/test_gpu_glmm_predict.py); quantities behind an
H^-1 rtol 1e-6 with atol 1e-12, cross Hessians 1e-9 (tests/test_gpu_glmm_slopes_influence.py).

Shapes: those of the issue.  Seeds: the first of N + P + K, N + P + K + 1, .. at which the reference Hessian (free coordinates)
is positive definite at the point of `glmm_corr_reference.problem` (found on the CPU; smallest eigenvalues 0.12, 0.58, 0.062,
0.26).  At (500, 8, 3, 40) no seed from 511 to 535 gives one (as for the independent-effects model, tests/test_gpu_glmm_slopes.py)
while every local block is positive definite: there the Schur complement is checked as everywhere and the factorisation must
refuse it; K = 3 (NC = 10) gets its solve and group covariance at (300, 5, 3, 7), seed 308 (smallest eigenvalue 0.060)."""
import mpmath
import numpy as np
import pytest
import torch

import dense_reference as dref
import glmm_corr_reference as ref
import glmm_slopes_reference as sref
from helpers import rel_err
from test_gpu_glmm_slopes_device_solve import _backward_error, _assert_forward_bound, _fro, _status
from test_gpu_glmm_predict import _block_err, _gh_mean

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = 2.0 ** -53
#          lik,        N,   P,  K, G,  seed
SHAPES = [('logistic', 37, 3, 1, 5, 41),                                 # NC = 3
          ('logistic', 130, 3, 2, 2, 135),                               # both groups cross the 64-row tile boundary
          ('logistic', 500, 8, 3, 40, 511),                              # NC = 10, an empty group, one with more than half of the rows
          ('logistic', 257, 64, 4, 3, 325),                              # R = 143, the largest, beyond the legacy 140
          ('poisson', 300, 5, 2, 7, 307)]                                # Poisson, with an offset
POSDEF = [SHAPES[0], SHAPES[1], SHAPES[3], SHAPES[4], ('logistic', 300, 5, 3, 7, 308)]
SMALL = [SHAPES[0], SHAPES[1], SHAPES[4]]


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


def _par(vb, P, K, G):
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    par.push_param(vb.WishartParam('lam', size=K))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    return par


def _model(vb, lik, x, y, z, w, gid, o, G, hyp):
    from lrvb_amd.models import vech_to_sym
    par = _par(vb, x.shape[1], z.shape[1], G)
    kw = dict(beta_prior_info=hyp[0], mu_prior=hyp[1:3], lambda_prior=(hyp[3], vech_to_sym(hyp[4:])), weights=w)
    if lik == 'logistic':
        return par, vb.LogisticGLMMCorrObjective(par, x, y, z, gid, G, **kw)
    return par, vb.PoissonGLMMCorrObjective(par, x, y, z, gid, G, offset=o, **kw)


_cache = {}


def _case(vb, lik, N, P, K, G, seed):
    """The model and what the tests of one shape share, computed once: the reference value, gradient and Hessian in free coordinates."""
    key = (lik, N, P, K, G, seed)
    if key not in _cache:
        x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed, lik)
        hyp = ref.other_hyp(K)
        par, fun = _model(vb, lik, x, y, z, w, gid, o, G, hyp)
        targs = ref.targs(x, y, z, w, o, gid, G, hyp, lik)
        valf, gf, Hf = ref.value_grad_hess(ref.kl_free, free, targs)
        _cache[key] = dict(par=par, fun=fun, free=free, targs=targs, x=x, y=y, z=z, w=w, gid=gid, o=o, hyp=hyp, valf=valf, gf=gf, Hf=Hf,
                           sizes=ref.sizes(P, K, G))
    return _cache[key]


def _schur(H, ng):
    return H[:ng, :ng] - H[:ng, ng:] @ np.linalg.solve(H[ng:, ng:], H[ng:, :ng])


def _local_blocks(Hf, ng, G, K):
    gk = np.arange(G * K).reshape(G, K)
    li = ng + np.concatenate([gk, G * K + gk], axis=1)
    return Hf[li[:, :, None], li[:, None, :]]


@pytest.mark.parametrize('lik,N,P,K,G,seed', SHAPES)
def test_value_grad_hessian_products_and_schur(vb, lik, N, P, K, G, seed):
    c = _case(vb, lik, N, P, K, G, seed)
    par, fun, free, targs, gid = c['par'], c['fun'], c['free'], c['targs'], c['gid']
    Kv, ng, D = c['sizes']
    if (N, G) == (130, 2):
        assert all(np.unique(np.flatnonzero(gid == g) // 64).size > 1 for g in range(G))
    if G == 40:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2
    eta = ref.free_to_vec(torch.tensor(free), P, K, G).numpy()
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    e = [abs(fun.value(eta, False) - val) / abs(val), rel_err(fun.grad(eta, False), g), rel_err(fun.hessian(eta, False), H)]
    print('vector', lik, N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    assert np.allclose(par['u']['mean'].get(), eta[ng:ng + G * K].reshape(G, K))     # par holds the evaluation point
    assert np.allclose(par['lam']['df'].get(), eta[2 * P + 2 * K])
    Hd = fun.hessian(free, True)
    e = [abs(fun.value(free, True) - c['valf']) / abs(c['valf']), rel_err(fun.grad(free, True), c['gf']), rel_err(Hd, c['Hf'])]
    print('free', lik, N, P, K, G, e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-9
    objective = vb.Objective(par, fun)
    v = np.random.default_rng(3).normal(size=D)
    e_hvp = rel_err(objective.fun_free_hvp(free, v), c['Hf'] @ v)
    assert e_hvp < 1e-9
    assert rel_err(fun.sparse_hessian(free).toarray(), Hd) < 1e-14
    assert np.all(np.linalg.eigvalsh(_local_blocks(c['Hf'], ng, G, K)) > 0)          # a NOT_POSDEF would be a finding about the kernel
    HS = fun.global_hessian(free)
    e_s = rel_err(HS, _schur(c['Hf'], ng))
    print('hvp', e_hvp, 'schur', e_s)
    assert e_s < 1e-9
    gc = fun._ensure_gctx()
    fun.global_hessian(free, want_host=False)
    if np.min(np.linalg.eigvalsh(c['Hf'])) <= 0:
        assert (N, P, K, G) == (500, 8, 3, 40)
        with pytest.raises(np.linalg.LinAlgError):
            gc.chol_factor_last()
        return
    gc.chol_factor_last()
    assert np.allclose(gc.lrvb_cov(np.eye(ng)[:P]), np.linalg.inv(c['Hf'])[:P, :P], rtol=1e-6, atol=0)


def _arrow_inputs(fun, free):
    """What `global_hessian` sends to lrvb_glmm_arrow_schur at `free`, the group sums of the point left resident: (blocks, scale,
    d, A0, A1), and (s, rows, Hx, loc) of the host arrow in free coordinates."""
    from lrvb_amd import glmm_corr as gcm
    from lrvb_amd.block_arrow import _to_groups
    K, G, ng = fun.K, fun.G, fun.n_global
    eta = fun._eta(free, True)
    _, Hgg, rows, Hx, loc = fun._arrow_to_free(fun._closed(eta), eta)
    _, _, e_mu, _, n, V, e, ig = fun._split(eta)
    A0, A1 = gcm.glmm_corr_border_tables(K, n, V, fun._closed_jac(eta))
    jl = _to_groups(fun._jac(eta)[0][ng:], G, K)[:, :, 0]
    scale = np.concatenate([jl[:, :K], -jl[:, K:] / ig ** 2], axis=1)
    iu = np.triu_indices(2 * K)
    return (np.ascontiguousarray(loc[:, iu[0], iu[1]]), scale, e - e_mu[None, :], A0, A1), (fun._coupled_scaling(eta), rows, Hx, loc)


@pytest.mark.parametrize('lik,N,P,K,G,seed', SHAPES)
def test_arrow_schur_entry_by_entry(vb, lik, N, P, K, G, seed):
    """M of lrvb_glmm_arrow_schur against sum_g C_g^T A_g^-1 C_g formed in numpy, group by group, from the host border."""
    c = _case(vb, lik, N, P, K, G, seed)
    fun, free = c['fun'], c['free']
    args, (s, rows, Hx, loc) = _arrow_inputs(fun, free)
    M = fun.ctx.glmm_arrow_schur(*args)
    NC = K + 1 + K * (K + 1) // 2
    R = 2 * P + NC
    assert M.shape == (R, R) and args[3].shape == (2 * K, NC) and args[4].shape == (2 * K, K, NC)
    Hx4 = Hx.reshape(R, 2, G, K)
    want = np.zeros((R, R))
    for g in range(G):
        Cg = np.concatenate([Hx4[:, 0, g], Hx4[:, 1, g]], axis=1)                    # R x 2 K
        want += Cg @ np.linalg.solve(loc[g], Cg.T)
    e = rel_err(M * s[:, None] * s[None, :], want)
    print('arrow schur', lik, N, P, K, G, 'R', R, e)
    assert e < 1e-9
    assert np.array_equal(fun.ctx.glmm_arrow_schur(*args), M)                        # two calls: equal bits


@pytest.mark.parametrize('N,P,K,G,seed', [(130, 5, 2, 3, 0), (257, 64, 4, 3, 1), (90, 3, 1, 4, 2)])
def test_tables_of_the_legacy_layout_reproduce_slopes_schur(vb, N, P, K, G, seed):
    """Tables that encode the coupled layout of `LogisticGLMMSlopesObjective` ([e_mu_k, a_k, b_k] per component, NC = 3 K): M of
    lrvb_glmm_arrow_schur against M of lrvb_glmm_slopes_schur at the same point.  The closed entries are rounded differently
    (A0 + A1 d against the host's product), so not bitwise: 1e-12 relative.  NC = 3 K is the legacy layout itself, so each
    family's solve entries accept the other's factor there."""
    x, y, z, w, gid, free = sref.problem(N, P, K, G, seed)
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, weights=w)
    sent = []
    schur = fun.ctx.glmm_slopes_schur
    fun.ctx.glmm_slopes_schur = lambda *a: sent.append(a) or schur(*a)
    fun.global_hessian(free, want_host=False)
    del fun.ctx.glmm_slopes_schur
    (blocks, scale, closed), = sent
    M_legacy = schur(blocks, scale, closed)
    eta = np.where(sref.positive_mask(P, K, G), np.exp(free), free)
    ng = 2 * P + 4 * K
    e_mu, a, b = eta[2 * P:2 * P + K], eta[2 * P + 2 * K:ng:2], eta[2 * P + 2 * K + 1:ng:2]
    d = eta[ng:ng + G * K].reshape(G, K) - e_mu[None, :]
    ta, tb = 1.0 / b, -a / b ** 2
    A0, A1 = np.zeros((2 * K, 3 * K)), np.zeros((2 * K, K, 3 * K))
    for k in range(K):
        A0[k, 3 * k] = -a[k] / b[k]
        A1[k, k, 3 * k + 1], A1[k, k, 3 * k + 2] = ta[k], tb[k]
        A0[K + k, 3 * k + 1], A0[K + k, 3 * k + 2] = 0.5 * ta[k], 0.5 * tb[k]
    full = np.zeros((G, 2 * K, 3 * K))                                   # the closed rows of the legacy entry, each in the columns of its component
    for i in range(2 * K):
        full[:, i, 3 * (i % K):3 * (i % K) + 3] = closed[:, i]
    assert np.allclose(A0[None] + np.einsum('ilc,gl->gic', A1, d), full, rtol=1e-14, atol=0)
    M_arrow = fun.ctx.glmm_arrow_schur(blocks, scale, d, A0, A1)
    e = rel_err(M_arrow, M_legacy)
    print('legacy layout through the tables', N, P, K, G, e)
    assert M_arrow.shape == M_legacy.shape and e < 1e-12
    Rl = np.random.default_rng(1).normal(size=(G, 2 * K, 3))
    red_a = fun.ctx.glmm_arrow_solve_forward(Rl, 3 * K)                               # the arrow factor is resident
    red_l = fun.ctx.glmm_slopes_solve_forward(Rl)                                     # ... and the legacy entry reads the same layout
    assert np.array_equal(red_a, red_l)


def _both_routes(fun, free, R):
    H = fun.hessian(free)
    Xh = fun.solve(free, R, on_device=False)
    Xd = fun.solve(free, R, on_device=True)
    assert Xd.shape == Xh.shape == np.shape(R)
    return H, Xd, Xh, _backward_error(H, Xd, R), _backward_error(H, Xh, R), float(np.linalg.cond(H))


@pytest.mark.parametrize('lik,N,P,K,G,seed', POSDEF)
def test_solve_and_lrvb_cov_both_routes(vb, lik, N, P, K, G, seed):
    """The two routes by the backward-error rule on the dense H = fun.hessian(theta); and both against the dense inverse of the
    REFERENCE Hessian: that matrix differs from the solved one by up to the Hessian tolerance 1e-9 (relative), so the first-order
    bound, doubled, is ||X - X_ref|| <= 2 kappa (eta + 1e-9) ||X_ref||."""
    c = _case(vb, lik, N, P, K, G, seed)
    fun, free, Hf = c['fun'], c['free'], c['Hf']
    Kv, ng, D = c['sizes']
    rng = np.random.default_rng(seed)
    Q = 21 if P == 64 else 5
    R = rng.normal(size=D) if K == 1 else rng.normal(size=(D, Q))
    H, Xd, Xh, e_dev, e_host, kappa = _both_routes(fun, free, R)
    print('%s: eta_dev %.3e, eta_host %.3e, kappa_2(H) %.4e' % ((lik, N, P, K, G), e_dev, e_host, kappa))
    assert e_dev <= 8.0 * e_host + D * U53
    _assert_forward_bound(Xd, Xh, 2.0 * kappa * (e_dev + e_host), 'X')
    Xref = np.linalg.solve(Hf, R)
    kref = float(np.linalg.cond(Hf))
    _assert_forward_bound(Xh, Xref, 2.0 * kref * (e_host + 1e-9), 'X host against the reference inverse')
    _assert_forward_bound(Xd, Xref, 2.0 * kref * (e_dev + 1e-9), 'X device against the reference inverse')
    M = rng.normal(size=(4, D))
    want = M @ np.linalg.solve(Hf, M.T)
    Rm = np.ascontiguousarray(M.T)
    em_d, em_h = _backward_error(H, fun.solve(free, Rm, on_device=True), Rm), _backward_error(H, fun.solve(free, Rm), Rm)
    for on_device, em in ((False, em_h), (True, em_d)):
        cov = fun.lrvb_cov(free, M, on_device=on_device)
        # |M (X - X_ref)| <= ||M|| ||X - X_ref||: the same bound, on the scale ||M|| ||X_ref||
        assert float(_fro(cov - want)) <= 2.0 * kref * (em + 1e-9) * float(_fro(M)) * float(_fro(np.linalg.solve(Hf, M.T)))
    assert np.array_equal(fun.solve(free, R, on_device=True), Xd)                     # the factor is reused: equal bits


def _moments(x, z, gid, P, K, G, ng):
    C = np.zeros((x.shape[0], ng + 2 * G * K))
    C[:, :P] = x
    for n, g in enumerate(gid):
        C[n, (2 * P if g < 0 else ng + g * K) + np.arange(K)] = z[n]
    return C


@pytest.mark.parametrize('lik,N,P,K,G,seed', POSDEF)
def test_group_cov_ranef_se_and_predict(vb, lik, N, P, K, G, seed):
    c = _case(vb, lik, N, P, K, G, seed)
    fun, free, x, z, gid, o = c['fun'], c['free'], c['x'], c['z'], c['gid'], c['o']
    Kv, ng, D = c['sizes']
    H = fun.hessian(free)
    np.linalg.cholesky(H)
    kappa = float(np.linalg.cond(H))
    floor = kappa * D * U53
    rng = np.random.default_rng([seed, 32])
    n_new = 40
    new = dict(x=rng.normal(size=(n_new, P)) / np.sqrt(P), z=np.concatenate([np.ones((n_new, 1)), 0.5 * rng.normal(size=(n_new, K - 1))], axis=1),
               groups=rng.integers(0, G, size=n_new))
    new['groups'][::7] = -1                                                           # population-level rows
    if lik == 'poisson':
        new['offset'] = 0.3 * rng.normal(size=n_new)
    n0, n1 = 3, N - 2
    Cw, Cn = _moments(x[n0:n1], z[n0:n1], gid[n0:n1], P, K, G, ng), _moments(new['x'], new['z'], new['groups'], P, K, G, ng)
    X = dref.refined_solve(H, np.hstack([np.eye(D), Cw.T, Cn.T]))
    Hinv = X[:, :D]
    var_w = np.einsum('nd,dn->n', Cw.astype(LD), X[:, D:D + Cw.shape[0]])
    var_n = np.einsum('nd,dn->n', Cn.astype(LD), X[:, D + Cw.shape[0]:])
    ie = ng + np.arange(G * K).reshape(G, K)
    want = (Hinv[:P, :P], np.stack([Hinv[np.ix_(ie[g], ie[g])] for g in range(G)]), np.stack([Hinv[:P][:, ie[g]] for g in range(G)]))
    cov_host, cov_dev = fun.group_cov(free, on_device=False), fun.group_cov(free, on_device=True)
    for name, dev, host, rf in zip(('cov_beta', 'cov_u', 'cov_beta_u'), cov_dev, cov_host, want):
        assert dev.shape == host.shape == rf.shape
        e_dev, e_host = _block_err(dev, rf), _block_err(host, rf)
        print('%s %s: err_dev %.3e, err_host %.3e, floor %.3e' % ((lik, N, P, K, G), name, e_dev, e_host, floor))
        assert e_dev <= 8.0 * e_host + floor
    assert all(np.array_equal(a, b) for a, b in zip(fun.group_cov(free, on_device=True), cov_dev))       # two calls
    se_lr, se_mf = fun.ranef_se(free, on_device=True)
    assert np.array_equal(se_lr, np.sqrt(np.diagonal(cov_dev[1], axis1=1, axis2=2)))
    assert np.allclose(se_mf, 1.0 / np.sqrt(np.exp(free[ng + G * K:]).reshape(G, K)), rtol=1e-14, atol=0)
    se_h = fun.ranef_se(free)[0]
    assert np.allclose(se_h, np.sqrt(np.diagonal(cov_host[1], axis1=1, axis2=2)), rtol=1e-12, atol=0)
    # rows: the window and new rows with population-level ones
    m, v = free[:P], np.exp(-free[P:2 * P])
    e2 = np.vstack([free[ng:ng + G * K].reshape(G, K), free[2 * P:2 * P + K][None, :]])
    r2 = np.vstack([np.exp(-free[ng + G * K:]).reshape(G, K), np.exp(-free[2 * P + K:2 * P + 2 * K])[None, :]])
    for what, rows, wantv, kw in (('window', (x[n0:n1], z[n0:n1], gid[n0:n1], None if lik == 'logistic' else o[n0:n1]), var_w, dict(n0=n0, n1=n1)),
                                  ('new rows', (new['x'], new['z'], new['groups'], new.get('offset')), var_n, dict(newdata=new))):
        host, dev = fun.predict(free, on_device=False, **kw), fun.predict(free, on_device=True, **kw)
        xs, zs, gs, off = rows
        gi = np.where(gs < 0, G, gs)
        off = np.zeros(xs.shape[0]) if off is None else off
        t_rho = np.concatenate([off[:, None], xs * m[None, :], zs * e2[gi]], axis=1).astype(LD)
        t_s = np.concatenate([(xs * xs).astype(LD) * v[None, :].astype(LD), (zs * zs).astype(LD) * r2[gi].astype(LD)], axis=1)
        assert np.all(np.abs(dev['rho'].astype(LD) - t_rho.sum(1)) <= (P + K + 2) * U53 * np.abs(t_rho).sum(1))
        assert np.all(np.abs(dev['var_mf'].astype(LD) - t_s.sum(1)) <= (P + K + 2) * U53 * np.abs(t_s).sum(1))
        e_dev = np.abs(dev['var_lrvb'].astype(LD) - wantv) / wantv
        e_host = np.abs(host['var_lrvb'].astype(LD) - wantv) / wantv
        print('%s %s: var_lrvb err_dev %.3e, err_host %.3e, floor %.3e' % ((lik, N, P, K, G), what, float(e_dev.max()), float(e_host.max()), floor))
        assert np.all(wantv > 0) and np.all(e_dev <= 8.0 * e_host + floor)
        # the response scale on the device's own rho and variances: 8 x the float64 restatement's own error against mpmath, floor 16 * 2^-53
        sub = np.linspace(0, xs.shape[0] - 1, 12).astype(int)
        kind = 'logistic' if lik == 'logistic' else 'poisson'
        for col, var in (('mean_mf', 'var_mf'), ('mean_lrvb', 'var_lrvb')):
            mine = _gh_mean(kind, dev['rho'][sub], dev[var][sub], None, fun.gh_x, fun.gh_w)
            exact = _gh_mean(kind, dev['rho'][sub], dev[var][sub], None, fun.gh_x, fun.gh_w, mp=True)
            own = np.array([float(abs(mpmath.mpf(float(a)) - ex) / abs(ex)) for a, ex in zip(mine, exact)])
            assert np.all(np.abs(dev[col][sub] - mine) / np.abs(mine) <= np.maximum(8.0 * own, 16.0 * U53))
    full = fun.predict(free, on_device=True)
    win = fun.predict(free, n0=n0, n1=n1, on_device=True)
    assert all(np.array_equal(win[k], full[k][n0:n1]) for k in full)                 # a window is a slice, bit for bit


@pytest.mark.parametrize('lik,N,P,K,G,seed', SMALL)
def test_influence_against_the_dense_cross_hessian_route(vb, lik, N, P, K, G, seed):
    c = _case(vb, lik, N, P, K, G, seed)
    par, fun, free, targs, Hf, w, gid = c['par'], c['fun'], c['free'], c['targs'], c['Hf'], c['w'], c['gid']
    Kv, ng, D = c['sizes']
    wt = targs[3].clone().requires_grad_(True)
    p = torch.tensor(free).requires_grad_(True)
    g, = torch.autograd.grad(ref.kl_free(p, targs[0], targs[1], targs[2], wt, *targs[4:]), p, create_graph=True)
    Cw = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(D)])
    Cf = fun.cross_hessian(fun.weights_par, free, True)
    assert Cf.shape == (D, N) and rel_err(Cf, Cw) < 1e-9
    want = -np.linalg.solve(Hf, Cw).T                                                 # N x D
    for on_device in (False, True):
        rows = fun.obs_influence(free, np.eye(D), on_device=on_device)
        print('obs_influence', lik, N, P, K, G, on_device, rel_err(rows, want))
        assert np.allclose(rows, want, rtol=1e-6, atol=1e-12)
        gi = fun.group_influence(free, np.eye(D), on_device=on_device)
        gw = np.zeros((G, D))
        np.add.at(gw, gid, w[:, None] * want)
        assert gi.shape == (G, D) and np.allclose(gi, gw, rtol=1e-6, atol=1e-12)
    assert np.array_equal(fun.obs_influence(free, np.eye(ng)[:2], n0=7, n1=30), fun.obs_influence(free, np.eye(D)[:2], n0=7, n1=30))
    lin = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, free, w, stream_hyper=True)
    dense = lin.get_doutput_dhyper_rows(np.eye(D)[:4])
    assert np.allclose(dense, want[:, :4], rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize('lik,N,P,K,G,seed', [SHAPES[1], POSDEF[4], SHAPES[4]])
def test_lambda_prior_cross_hessian_and_sensitivity(vb, lik, N, P, K, G, seed):
    """lambda_prior = [nu0 | vech W0]: the KL is linear in it; cross Hessian and d theta_global / d hyper against autograd."""
    c = _case(vb, lik, N, P, K, G, seed)
    fun, free, targs, Hf = c['fun'], c['free'], c['targs'], c['Hf']
    Kv, ng, D = c['sizes']
    hy = targs[7].clone().requires_grad_(True)
    p = torch.tensor(free).requires_grad_(True)
    val = ref.kl_free(p, *targs[:7], hy, lik)
    g, = torch.autograd.grad(val, p, create_graph=True)
    C_all = np.stack([torch.autograd.grad(g[k], hy, retain_graph=True)[0].numpy() for k in range(D)])
    g_h, = torch.autograd.grad(val, hy)
    assert np.array_equal(np.asarray(fun.lambda_prior_par.get_vector()), c['hyp'][3:])
    assert rel_err(fun.hyper_grad(fun.lambda_prior_par, free, True), g_h.numpy()[3:]) < 1e-10
    for par_h, cols in ((fun.lambda_prior_par, slice(3, None)), (fun.mu_prior_par, slice(1, 3)), (fun.beta_prior_info_par, slice(0, 1))):
        C = fun.cross_hessian(par_h, free, True)
        assert C.shape == C_all[:, cols].shape and rel_err(C, C_all[:, cols]) < 1e-9
        assert np.all(C[ng:] == 0.0)
        sens = fun.global_sensitivity(par_h, free)
        want = -np.linalg.solve(Hf, C_all[:, cols])[:ng]
        assert np.allclose(sens, want, rtol=1e-6, atol=1e-12)


def _fit(vb, objective, theta0):
    th, _ = vb.OptimizationUtils.minimize_objective_trust_ncg(objective, theta0, False, maxiter=300, gtol=1e-7, disp=False)
    th = np.asarray(th, dtype=np.float64)
    for _ in range(8):                                   # Newton polish where the ratio test stalls at the rounding of f
        g = objective.fun_free_grad(th)
        if np.max(np.abs(g)) < 1e-8:
            break
        th = th - objective.fun.solve(th, g)
    return th


def test_fit_recovers_a_negative_correlation(vb):
    N, P, K, G = 2000, 3, 2, 40
    rng = np.random.default_rng(2000)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), rng.normal(size=(N, 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    sd = np.array([1.0, 0.8])
    cov = np.array([[1.0, -0.6], [-0.6, 1.0]]) * sd[:, None] * sd[None, :]
    u = rng.multivariate_normal(np.array([0.3, -0.2]), cov, size=G)
    beta = np.array([0.8, -0.5, 0.3])
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid]).sum(1))))).astype(np.float64)
    w, o, hyp = np.ones(N), np.zeros(N), ref.default_hyp(K)
    par, fun = _model(vb, 'logistic', x, y, z, w, gid, o, G, hyp)
    Kv, ng, D = ref.sizes(P, K, G)
    objective = vb.Objective(par, fun)
    th = _fit(vb, objective, np.zeros(D))
    targs = ref.targs(x, y, z, w, o, gid, G, hyp)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    print('reference gradient at the optimum', np.max(np.abs(g_ad)))
    assert np.max(np.abs(g_ad)) < 1e-6                                   # stationary by the REFERENCE gradient
    assert np.min(np.linalg.eigvalsh(H_ad)) > 0
    Hinv = np.linalg.inv(H_ad)
    M = np.eye(D)[:P]
    for on_device in (False, True):
        assert np.allclose(fun.lrvb_cov(th, M, on_device=on_device), Hinv[:P, :P], rtol=1e-6, atol=0)
    cov_hat, corr_hat = fun.ranef_cov(th)
    print('estimated covariance of the effects', cov_hat.ravel(), 'correlation', corr_hat[0, 1])
    assert corr_hat[0, 1] < 0 and np.allclose(np.diag(corr_hat), 1.0)
    par.set_free(th)
    assert np.allclose(cov_hat, np.linalg.inv(par['lam']['v'].get()) / (par['lam']['df'].get() - K - 1.0))


def test_bitwise_and_state_through_the_raw_entries(vb):
    """Two calls of every new entry give equal bits; the refusals, by status code."""
    hip = vb._hip
    lik, N, P, K, G, seed = POSDEF[4]
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed, lik)        # a model of its own: the test ends with the groups set anew
    c = dict(x=x, y=y, z=z, gid=gid)
    _, fun = _model(vb, lik, x, y, z, w, gid, o, G, ref.other_hyp(K))
    ctx = fun.ctx
    NC = K + 1 + K * (K + 1) // 2
    R = 2 * P + NC
    args, (s, rows, Hx, loc) = _arrow_inputs(fun, free)
    blocks, scale, d, A0, A1 = args
    rng = np.random.default_rng(5)
    Rl, xc, W = rng.normal(size=(G, 2 * K, 3)), rng.normal(size=(R, 3)), np.eye(R) + 0.01 * np.ones((R, R))
    M = np.empty((R, R))

    def schur(k=K, nc=NC, g=G, b=blocks, ptrs=None):
        a0, a1 = np.zeros((2 * max(k, 1), max(nc, 1))), np.zeros((2 * max(k, 1), max(k, 1), max(nc, 1)))
        if (k, nc) == (K, NC):
            a0, a1 = A0, A1
        out = np.empty((2 * P + max(nc, 0), 2 * P + max(nc, 0)))
        p = [hip.ptr(b), hip.ptr(scale), hip.ptr(d), hip.ptr(a0), hip.ptr(a1), hip.ptr(out)] if ptrs is None else ptrs
        return ctx._lib.lrvb_glmm_arrow_schur(ctx._h, p[0], p[1], p[2], p[3], p[4], g, k, nc, p[5])
    fwd = lambda a=Rl, nc=NC: _status(ctx, ctx.glmm_arrow_solve_forward, a, nc)
    back = lambda a=xc, g=G, k=K, nc=NC: _status(ctx, ctx.glmm_arrow_solve_back, a, g, k, nc)
    gcov = lambda g=G, k=K, nc=NC: _status(ctx, ctx.glmm_arrow_group_cov, np.eye(2 * P + nc), np.ones(2 * P + nc), g, k, nc)
    # bitwise
    assert schur() == hip.OK
    a = (ctx.glmm_arrow_solve_forward(Rl, NC), ctx.glmm_arrow_solve_back(xc, G, K, NC), ctx.glmm_arrow_group_cov(W, s, G, K, NC))
    assert schur() == hip.OK
    b = (ctx.glmm_arrow_solve_forward(Rl, NC), ctx.glmm_arrow_solve_back(xc, G, K, NC), ctx.glmm_arrow_group_cov(W, s, G, K, NC))
    assert all(np.array_equal(p, q) and np.all(np.isfinite(p)) for p, q in zip(a, b))
    # unsupported sizes, null pointers, a wrong G
    assert schur(k=0) == hip.ERR_UNSUPPORTED and schur(k=5) == hip.ERR_UNSUPPORTED
    assert schur(nc=K - 1) == hip.ERR_UNSUPPORTED and schur(nc=17) == hip.ERR_UNSUPPORTED
    assert fwd(nc=17) == hip.ERR_UNSUPPORTED and back(nc=K - 1, a=np.ones((2 * P + K - 1, 3))) == hip.ERR_UNSUPPORTED
    assert gcov(nc=17) == hip.ERR_UNSUPPORTED and fwd(np.ones((G, 10, 3))) == hip.ERR_UNSUPPORTED
    good = [hip.ptr(blocks), hip.ptr(scale), hip.ptr(d), hip.ptr(A0), hip.ptr(A1), hip.ptr(M)]
    for i in range(6):
        assert schur(ptrs=[None if j == i else q for j, q in enumerate(good)]) == hip.ERR_INVALID
    assert ctx._lib.lrvb_glmm_arrow_solve_forward(ctx._h, None, G, K, NC, 3, hip.ptr(M)) == hip.ERR_INVALID
    assert ctx._lib.lrvb_glmm_arrow_group_cov(ctx._h, None, hip.ptr(s), P, G, K, NC, None) == hip.ERR_INVALID
    assert schur(g=G + 1) == hip.ERR_SIZE and fwd(np.ones((G - 1, 2 * K, 3))) == hip.ERR_SIZE and gcov(g=G + 1) == hip.ERR_SIZE
    # state: a factor of another coupled layout is refused by either family
    assert schur() == hip.OK and fwd() == hip.OK and back() == hip.OK and gcov() == hip.OK
    assert fwd(nc=NC + 1) == hip.ERR_STATE and gcov(nc=NC - 1) == hip.ERR_STATE       # an arrow entry asked for another NC
    legacy_fwd = lambda: _status(ctx, ctx.glmm_slopes_solve_forward, Rl)
    legacy_gcov = lambda: _status(ctx, ctx.glmm_slopes_group_cov, np.eye(2 * P + 3 * K), np.ones(2 * P + 3 * K), G, K)
    assert legacy_fwd() == hip.ERR_STATE and legacy_gcov() == hip.ERR_STATE           # legacy entries on an arrow factor, NC = 10 != 9
    closed = np.zeros((G, 2 * K, 3))
    assert _status(ctx, ctx.glmm_slopes_schur, blocks, scale, closed) == hip.OK       # the legacy factor, 3 K columns
    assert legacy_fwd() == hip.OK
    assert fwd() == hip.ERR_STATE and back() == hip.ERR_STATE and gcov() == hip.ERR_STATE     # arrow entries on a legacy factor
    # an uploaded block that is not positive definite: a handled status, and no factor is left
    bad = blocks.copy()
    bad[1, 2 * K] = -1.0                                                 # entry (1, 1) of group 1's block
    assert schur(b=bad) == hip.ERR_NOT_POSDEF
    assert fwd() == hip.ERR_STATE and legacy_fwd() == hip.ERR_STATE
    assert schur() == hip.OK and fwd() == hip.OK
    # whatever drops the legacy factor drops this one; without sums nothing is eliminated
    fun.value(free)
    assert fwd() == hip.ERR_STATE and gcov() == hip.ERR_STATE
    # the class: free coordinates and this process's own rows only
    with pytest.raises(ValueError):
        fun.solve(ref.free_to_vec(torch.tensor(free), P, K, G).numpy(), np.ones(free.size), is_free=False, on_device=True)
    with pytest.raises(ValueError):
        fun.group_cov(free, is_free=False, on_device=True)
    assert np.all(np.isfinite(fun.solve(free, np.ones(free.size), on_device=True)))
    with pytest.raises(ValueError):
        _par_bad = vb.ModelParamsDict('params')
        _par_bad.push_param(vb.UVNParamVector('beta', length=P))
        _par_bad.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            _par_bad.push_param(vb.GammaParam('tau%d' % k))
        _par_bad.push_param(vb.UVNParamArray('u', shape=(G, K)))
        vb.LogisticGLMMCorrObjective(_par_bad, c['x'], c['y'], c['z'], c['gid'], G)
    _arrow_inputs(fun, free)                                             # the group sums of the point, resident again
    assert schur() == hip.OK
    ctx.set_groups(c['gid'], G)
    assert schur() == hip.ERR_STATE and fwd() == hip.ERR_STATE           # no group sums resident

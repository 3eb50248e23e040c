"""The host state the model classes share (`DeviceModel`, models.py) on the GPU, one objective per family:
a memoised evaluation is computed once per point, dropped when a reduce hook is installed or removed and when the weights
change, installed statistics reproduce the plain path and are refused under a hook, and `fun()` is the value at `par`.

Every comparison is bit for bit: both sides are the same device entries on the same inputs.  Shapes: N = 33 rows (a ragged tail
for every tile), P = 3 columns, 4 groups of unequal size (one of them empty), K = 2 effects, 3 classes, 2 mixture components, a
3-dimensional response.

`op` is the family's memoised evaluation and `entry` the device entry behind the memo, spied on to count evaluations; the hook is
an identity "reduction" that records the length of every buffer it is handed (`counted` picks the lengths of `entry`).  The
full-covariance logit-normal class memoises its dense Hessian for `cg_solve` (its `hvp` is matrix-free and keeps nothing);
softmax memoises the point of its matrix-free `hvp` (one gradient-only terms call); the mixture has no dense Hessian and no
memo: its evaluation is `global_hessian`, of which only the results are compared."""
import numpy as np
import pytest
import scipy.optimize

import glmm_slopes_reference as slopes_ref
import lmvn_reference
from test_lmm_host_math import make_par as lmm_par, random_eta as lmm_eta
from test_logitnormal_host_math import problem as logitnormal_problem
from test_mixture_host_math import make_par as mixture_par, problem as mixture_problem
from test_softmax_host_math import _problem as softmax_problem

pytestmark = pytest.mark.gpu

N, P, G, K = 33, 3, 4, 2
V_DIR = np.linspace(-1.0, 1.0, 64)


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


class Case(object):
    """build(weights) -> (par, fun); x: the free point; op(fun) -> array; entry(fun) -> (object, method name) of the device entry
    behind the memo (None: no memo); counted(n): the hook buffer of that entry; at_point: statistics belong to a point."""

    def __init__(self, build, w, x, op=None, entry=None, counted=lambda n: True, at_point=False, stats=None):
        self.build, self.w, self.x, self.entry, self.counted, self.at_point, self.stats = build, w, x, entry, counted, at_point, stats
        self.op = op or (lambda fun: fun.hvp(x, V_DIR[:x.size], True))


def _logitnormal(vb):
    x, y, w, eta = logitnormal_problem(N, P, 1)

    def build(w):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        return par, vb.LogitNormalRegressionObjective(par, x, y, prior_info=0.7, weights=w)
    par, _ = build(w)
    par.set_vector(eta)
    return Case(build, w, par.get_free(), entry=lambda f: (f.ctx, 'logitnormal_terms'), at_point=True, stats=lambda f, e: f.local_stats(e))


_LMVN_OPTIMUM = {}


def _logitnormal_mvn(vb):
    x, y, w, free, _ = lmvn_reference.problem(N, P, 2, with_extremes=False)

    def build(w):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.MVNParam('beta', dim=P))
        return par, vb.LogitNormalMVNRegressionObjective(par, x, y, prior_info=0.7, weights=w)
    if 'x' not in _LMVN_OPTIMUM:           # `cg_solve` wants a positive definite Hessian: the optimum, found once
        _, fun = build(w)
        _LMVN_OPTIMUM['x'] = scipy.optimize.minimize(fun.value, free, jac=fun.grad, method='L-BFGS-B', options=dict(maxiter=200)).x
    xo = _LMVN_OPTIMUM['x']
    return Case(build, w, xo, op=lambda f: f.cg_solve(xo, V_DIR[:xo.size])[0], entry=lambda f: (f, 'mvn_terms'),
                at_point=True, stats=lambda f, e: f.local_stats(e))


def _softmax(vb):
    x, y, w, beta = softmax_problem(np.random.default_rng(3), N, P, 3)
    D = beta.size

    def build(w):
        par = vb.ModelParamsDict('par')
        par.push_param(vb.ArrayParam('beta', shape=(2, P), lb=-2.0, ub=2.0))        # a box: the memo holds the chain terms
        return par, vb.SoftmaxRegressionObjective(par, x, y, 3, prior_info=0.5, weights=w)
    par, _ = build(w)
    par.set_vector(np.clip(beta.ravel(), -1.5, 1.5))
    return Case(build, w, par.get_free(), entry=lambda f: (f.ctx, 'softmax_terms'), counted=lambda n: n == D + 1)


def _normal_regression(vb):
    rng = np.random.default_rng(4)
    x = rng.random((N, P))
    y = x @ np.exp(rng.random((P, 3))) + rng.normal(size=(N, 3))
    w = rng.uniform(0.5, 1.5, N)

    def build(w):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.ArrayParam(name='beta', shape=(P, 3), lb=0.))
        par.push_param(vb.PosDefMatrixParam('lambda', size=3))
        return par, vb.NormalRegressionObjective(par, x, y, weights=w)
    par, _ = build(w)
    return Case(build, w, rng.normal(size=par.free_size()) * 0.3, entry=lambda f: (f.ctx, 'weighted_gram'), stats=lambda f, e: f.local_stats())


def _lmm(vb):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(N, P))
    gid = np.repeat(np.arange(G), [15, 9, 6, 3]).astype(np.int32)
    y = x @ rng.normal(size=P) + (rng.normal(size=G) * 0.7)[gid] + rng.normal(size=N) * 0.5
    w = rng.uniform(0.5, 1.5, N)

    def build(w):
        par = lmm_par(P, G)
        return par, vb.LMMObjective(par, x, y, gid, G, weights=w)
    par, _ = build(w)
    par.set_vector(lmm_eta(rng, P, G))
    return Case(build, w, par.get_free(), entry=lambda f: (f.ctx, 'grouped_stats'), stats=lambda f, e: f.local_stats())


def _mixture(vb):
    x, w, theta = mixture_problem(N, 3, 2, 6)

    def build(w):
        par = mixture_par(N, 3, 2)
        return par, vb.MixtureObjective(par, x, pi_prior=1.2, phi_prior=0.9, weights=w)
    return Case(build, w, theta, op=lambda f: f.global_hessian(theta), stats=lambda f, e: f.local_stats(theta))


def _mixed_model(vb):
    x, y, z, w, gid, free = slopes_ref.problem(N, P, K, G, 7)
    assert len(set(np.bincount(gid, minlength=G))) > 2                # groups of unequal size

    def build(w):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        return par, vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, beta_prior_info=1.3, mu_prior=(0.2, 0.7), tau_prior=(1.5, 0.8),
                                                   weights=w)
    return Case(build, w, free, entry=lambda f: (f.ctx, 'glmm_slopes_terms'), at_point=True, stats=lambda f, e: f.local_stats(e))


FAMILIES = {'logitnormal': _logitnormal, 'logitnormal_mvn': _logitnormal_mvn, 'softmax': _softmax, 'quadform': _normal_regression,
            'lmm': _lmm, 'mixture': _mixture, 'mixed_model': _mixed_model}
family = pytest.mark.parametrize('name', sorted(FAMILIES))


def _spy(case, fun):
    """Counts the calls of the device entry behind the memo."""
    calls = []
    if case.entry is not None:
        obj, attr = case.entry(fun)
        inner = getattr(obj, attr)
        setattr(obj, attr, lambda *a, **k: (calls.append(attr), inner(*a, **k))[1])
    return calls


@family
def test_memo_is_computed_once_and_dropped_with_the_hook(vb, name):
    case = FAMILIES[name](vb)
    _, fun = case.build(case.w)
    calls = _spy(case, fun)
    first = case.op(fun)                                               # no hook: this process's own sums
    n0 = len(calls)
    sizes = []
    fun.ctx.set_reduce_hook(lambda ptr, n, stream: sizes.append(n))    # an identity reduction that records its buffers
    hooked = case.op(fun)
    seen = [n for n in sizes if case.counted(n)]
    assert len(seen) >= 1, 'the evaluation formed before the hook was installed was reused under it'
    assert np.array_equal(hooked, first)
    again = case.op(fun)                                               # (a): the same point, the hook still installed
    assert np.array_equal(again, hooked)
    if case.entry is not None:
        assert [n for n in sizes if case.counted(n)] == seen and len(calls) == 2 * n0 and n0 >= 1
    fun.ctx.set_reduce_hook(None)
    unhooked = case.op(fun)
    assert np.array_equal(unhooked, first)
    if case.entry is not None:
        assert len(calls) == 3 * n0, 'the evaluation formed under the hook was reused after its removal'


@family
def test_weight_change_drops_the_memo(vb, name):
    case = FAMILIES[name](vb)
    _, fun = case.build(case.w)
    before = case.op(fun)
    w2 = case.w * np.linspace(0.5, 1.5, N)
    fun.weights_par.set_vector(w2)
    after = case.op(fun)
    assert not np.array_equal(after, before)
    assert np.array_equal(after, case.op(case.build(w2)[1]))


@pytest.mark.parametrize('name', sorted(set(FAMILIES) - {'softmax'}))          # softmax has no statistics to install
def test_installed_statistics(vb, name):
    case = FAMILIES[name](vb)
    par, fun = case.build(case.w)
    par.set_free(case.x)
    eta = np.array(par.get_vector(), dtype=np.float64)
    if case.at_point:
        plain = fun.hessian(eta, False)
        fun.set_reduced_stats(case.stats(fun, eta), eta)
        assert np.array_equal(fun.hessian(eta, False), plain)
        with pytest.raises(ValueError, match='the installed statistics were formed at another point'):
            fun.hessian(eta * 1.01, False)
        fun.set_reduced_stats(None)
        calls = _spy(case, fun)
        assert np.array_equal(fun.hessian(eta, False), plain) and len(calls) >= 1        # the plain path again
        fun.hessian(eta * 1.01, False)
    flat = case.stats(fun, eta)
    fun.ctx.set_reduce_hook(lambda ptr, n, stream: None)
    with pytest.raises(RuntimeError):
        fun.set_reduced_stats(flat, eta) if case.at_point else fun.set_reduced_stats(flat)
    fun.set_reduced_stats(None)
    fun.ctx.set_reduce_hook(None)


@family
def test_call_is_the_value_at_the_parameter(vb, name):
    case = FAMILIES[name](vb)
    par, fun = case.build(case.w)
    par.set_free(case.x)
    assert fun() == fun.value(par.get_free(), True)

"""Random-intercept logistic regression (logistic GLMM) with linear-response covariances.

    y_n ~ Bernoulli(sigma(x_n . beta + u_g(n))),  u_g ~ N(mu, 1 / tau)

Simulates data, fits the mean-field posterior with scipy's trust-ncg on the arrow products, prints the LRVB standard errors of
beta, mu and log tau (through the Schur complement of the arrow Hessian) next to the mean-field ones, ranks the groups by their
influence on one coefficient (streamed on the device), drops the top group, refits and prints the predicted change next to the
actual one, predicts a refit under a changed prior on tau by linear response and compares with the refit, and prints wall times.

    python examples/logistic_glmm.py [--small]
"""
import os
import sys
import time

import numpy as np
import scipy.optimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lrvb_amd as vb                                                     # noqa: E402
from lrvb_amd import glmm                                                 # noqa: E402


def newton_step(fun, th):
    """One Newton step on the arrow system: the Schur complement for the global part, the 2 x 2 blocks for the local one."""
    ng, G = fun.n_global, fun.G
    g = fun.grad(th, True)
    HS = fun.global_hessian(th)
    _, Hgg, rows, Hx, loc = fun._arrow(th, True)
    se, si = glmm.arrow_local_solve(loc, g[ng:ng + G], g[ng + G:])
    rhs = g[:ng].copy()
    rhs[rows] -= Hx @ np.concatenate([se, si])
    dg = np.linalg.solve(HS, rhs)
    t = Hx.T @ dg[rows]
    le, li = glmm.arrow_local_solve(loc, g[ng:ng + G] - t[:G], g[ng + G:] - t[G:])
    return th - np.concatenate([dg, le, li])


def fit(objective, fun, th0):
    opt = scipy.optimize.minimize(objective.fun_free, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp, x0=th0,
                                  method='trust-ncg', options={'gtol': 1e-6, 'maxiter': 200})
    th = opt.x
    for _ in range(10):                                # polish where the ratio test stalls at the rounding of f
        if np.max(np.abs(fun.grad(th, True))) < 1e-7:
            break
        th = newton_step(fun, th)
    return th


def main():
    small = '--small' in sys.argv
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, tau = rng.normal(size=P) * 0.8, 0.3, 2.0
    u = mu + rng.normal(size=G) / np.sqrt(tau)
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + u[gid])))).astype(np.float64)

    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParam('mu'))
    par.push_param(vb.GammaParam('tau'))
    par.push_param(vb.UVNParamVector('u', length=G))
    fun = vb.LogisticGLMMObjective(par, x, y, gid, G)
    objective = vb.Objective(par, fun)
    ng = fun.n_global

    t0 = time.perf_counter()
    th = fit(objective, fun, np.zeros(par.free_size()))
    print('fit: %.2f s, max |free gradient| %.2e' % (time.perf_counter() - t0, np.max(np.abs(fun.grad(th, True)))))

    # wall times: arrow build (everything asked for), Schur step, one product
    eta = fun._eta(th, True)
    best = lambda f: min(_timed(f) for _ in range(3))
    t_build = best(lambda: fun._device_terms(eta, True, True))
    t_schur = best(lambda: fun.global_hessian(th, want_host=False)) - best(lambda: fun._device_terms(eta, True, True, want_border=False))
    fun.hvp(th, np.ones(th.size), True)
    v = rng.normal(size=th.size)
    t_hvp = best(lambda: fun.hvp(th, v, True))
    print('arrow build %.4f s   Schur step %.4f s   one product %.5f s' % (t_build, t_schur, t_hvp))

    # LRVB standard errors of beta, mu and log tau next to the mean-field ones
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    par.set_free(th)
    a, b = float(np.ravel(par['tau']['shape'].get())[0]), float(np.ravel(par['tau']['rate'].get())[0])
    from scipy import special
    M = np.zeros((P + 2, ng))
    M[np.arange(P), np.arange(P)] = 1.0                                   # E beta_j = m_j
    M[P, 2 * P] = 1.0                                                     # E mu = e_mu
    M[P + 1, 2 * P + 2], M[P + 1, 2 * P + 3] = special.polygamma(1, a) * a, -1.0      # E log tau = digamma(a) - log b, free = logs
    cov = gc.lrvb_cov(M)
    se_lr = np.sqrt(np.diag(cov))
    se_mf = np.concatenate([1.0 / np.sqrt(par['beta']['info'].get()), [1.0 / np.sqrt(float(np.ravel(par['mu']['info'].get())[0]))],
                            [np.sqrt(special.polygamma(1, a))]])
    names = ['beta[%d]' % j for j in range(P)] + ['mu', 'log tau']
    print('%-10s %12s %12s' % ('', 'mean-field se', 'LRVB se'))
    for k in list(range(min(P, 4))) + [P, P + 1]:
        print('%-10s %12.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))

    # leave one cluster out: groups ranked by their streamed influence on beta[0], the top one dropped and refitted
    Mb = np.zeros((1, ng))
    Mb[0, 0] = 1.0
    t0 = time.perf_counter()
    gi = fun.group_influence(th, Mb)[:, 0]                               # d beta[0] / d (multiplier on the group's weights)
    t_gi = time.perf_counter() - t0
    top = np.argsort(-np.abs(gi))[:5]
    print('group influence on beta[0] (%.3f s): top groups %s, influence %s' % (t_gi, top.tolist(), np.array2string(gi[top], precision=5)))
    g = int(top[0])
    w = np.ones(N)
    w[gid == g] = 0.0
    fun.weights_par.set_vector(w)
    th_drop = fit(objective, fun, th)
    fun.weights_par.set_vector(np.ones(N))
    print('drop group %d (%d rows): beta[0] predicted change %.4e, actual change %.4e'
          % (g, int(np.sum(gid == g)), -gi[g], th_drop[0] - th[0]))

    # a changed prior on tau: linear-response prediction against the refit
    hp = fun.tau_prior_par
    new = np.array([3.0, 2.0])
    sens = fun.global_sensitivity(hp, th)
    pred = th[:ng] + sens @ (new - hp.get_vector())
    hp.set_vector(new)
    th2 = fit(objective, fun, th)
    move = th2[:ng] - th[:ng]
    print('tau_prior (1, 1) -> (3, 2): largest move of a global parameter %.3e, prediction error %.3e'
          % (np.max(np.abs(move)), np.max(np.abs(pred - th2[:ng]))))


def _timed(f):
    t = time.perf_counter()
    f()
    return time.perf_counter() - t


if __name__ == '__main__':
    main()

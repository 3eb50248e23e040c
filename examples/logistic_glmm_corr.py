"""Logistic mixed model with a CORRELATED random intercept and slope per group -- lme4's `(1 + x | g)` -- next to the model that
takes the two effects as independent.

    y_n ~ Bernoulli(sigma(x_n . beta + u_g0 + x_n0 u_g1)),  u_g ~ N(mu, Sigma),  corr(u_g0, u_g1) = -0.6

Simulates the data, fits `LogisticGLMMSlopesObjective` (independent effects, a Gamma precision each) and
`LogisticGLMMCorrObjective` (a Wishart precision matrix) with scipy's trust-ncg on the block-arrow products (Newton polish on the
arrow solve), and prints the estimated correlation of the effects and, under both models, the LRVB standard errors of beta and of
a few groups' effects.

    python examples/logistic_glmm_corr.py [--small]
"""
import os
import sys
import time

import numpy as np
import scipy.optimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lrvb_amd as vb                                                     # noqa: E402


def fit(objective, fun, th0):
    opt = scipy.optimize.minimize(objective.fun_free, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp, x0=th0,
                                  method='trust-ncg', options={'gtol': 1e-6, 'maxiter': 300})
    th = opt.x
    for _ in range(10):                                # polish where the ratio test stalls at the rounding of f
        g = fun.grad(th, True)
        if np.max(np.abs(g)) < 1e-7:
            break
        th = th - fun.solve(th, g, on_device=True)
    return th


def main():
    small = '--small' in sys.argv
    N, P, G = (20000, 4, 200) if small else (1000000, 16, 10000)
    K = 2
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    z = np.stack([np.ones(N), x[:, 0] * np.sqrt(P)], axis=1)              # intercept and the slope of the first covariate
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, sd, rho = rng.normal(size=P) * 0.8, np.array([0.3, -0.2]), np.array([0.9, 0.6]), -0.6
    Sigma = np.array([[1.0, rho], [rho, 1.0]]) * sd[:, None] * sd[None, :]
    u = rng.multivariate_normal(mu, Sigma, size=G)
    y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid]).sum(1))))).astype(np.float64)

    def parameter(precision):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for p in precision:
            par.push_param(p)
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        return par
    out = {}
    for name in ('independent', 'correlated'):
        if name == 'independent':
            par = parameter([vb.GammaParam('tau%d' % k) for k in range(K)])
            fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G)
        else:
            par = parameter([vb.WishartParam('lam', size=K)])
            fun = vb.LogisticGLMMCorrObjective(par, x, y, z, gid, G)
        objective = vb.Objective(par, fun)
        t0 = time.perf_counter()
        th = fit(objective, fun, np.zeros(par.free_size()))
        print('%s effects: fit %.2f s, max |free gradient| %.2e' % (name, time.perf_counter() - t0, np.max(np.abs(fun.grad(th, True)))))
        cov_beta = fun.group_cov(th, on_device=True)[0]
        se_u, se_u_mf = fun.ranef_se(th, on_device=True)
        out[name] = (np.sqrt(np.diag(cov_beta)), se_u, se_u_mf)
        if name == 'correlated':
            cov_hat, corr_hat = fun.ranef_cov(th)
            print('effects: simulated sd %s, correlation %.2f; estimated sd %s, correlation %.3f'
                  % (sd, rho, np.array2string(np.sqrt(np.diag(cov_hat)), precision=3), corr_hat[0, 1]))
    print('LRVB standard errors    %12s %12s' % ('independent', 'correlated'))
    for j in range(min(P, 4)):
        print('%-22s %12.5f %12.5f' % ('beta[%d]' % j, out['independent'][0][j], out['correlated'][0][j]))
    for g in range(3):
        for k in range(K):
            print('%-22s %12.5f %12.5f' % ('u[%d, %d]' % (g, k), out['independent'][1][g, k], out['correlated'][1][g, k]))


if __name__ == '__main__':
    main()

"""Poisson mixed model -- counts with a log link, an exposure offset, a random intercept and a random slope per group -- with
linear-response covariances.

    y_n ~ Poisson(exposure_n exp(x_n . beta + u_g0 + t_n u_g1 / 2)),  u_gk ~ N(mu_k, 1 / tau_k)

Simulates counts with exposure, fits the mean-field posterior with scipy's trust-ncg on the block-arrow products (Newton polish on the arrow
solve), prints the LRVB standard errors of beta and mu (through the Schur complement of the block-arrow Hessian) next to the
mean-field ones, ranks the groups by their influence on beta[0] (streamed on the device), drops the top group, refits and prints
the predicted change next to the actual one.

    python examples/poisson_glmm.py [--small] [--device-solve] [--predict]

--device-solve takes the Newton polish and the operand of the group influence through the device-resident block-arrow solve
(`on_device=True`): the border of the Hessian never reaches the host.  --predict prints, after the standard errors, the standard
errors of a few groups' effects and the fitted rates of a few rows and of one unseen design row at the population level, each
with its LRVB and its mean-field standard error (`ranef_se`, `predict`: the rows are streamed on the device).
"""
import os
import sys
import time

import numpy as np
import scipy.optimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lrvb_amd as vb                                                     # noqa: E402


def fit(objective, fun, th0, on_device=False):
    opt = scipy.optimize.minimize(objective.fun_free, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp, x0=th0,
                                  method='trust-ncg', options={'gtol': 1e-6, 'maxiter': 200})
    th = opt.x
    for _ in range(10):                                # polish where the ratio test stalls at the rounding of f
        g = fun.grad(th, True)
        if np.max(np.abs(g)) < 1e-7:
            break
        th = th - fun.solve(th, g, on_device=on_device)
    return th


def main():
    small = '--small' in sys.argv
    device_solve = '--device-solve' in sys.argv
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    K = 2
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    t = rng.standard_normal(N)                                            # a covariate of its own for the random slope: its mean
    z = np.stack([np.ones(N), 0.5 * t], axis=1)                           # slope is mu[1] alone (x has no intercept: that is mu[0])
    offset = np.log(rng.uniform(0.5, 2.0, size=N))                        # log exposure
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, tau = rng.normal(size=P) * 0.5, np.array([0.3, -0.2]), np.array([4.0, 8.0])
    u = mu[None, :] + rng.normal(size=(G, K)) / np.sqrt(tau)[None, :]
    y = rng.poisson(np.exp(offset + x @ beta + (z * u[gid]).sum(1))).astype(np.float64)

    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    fun = vb.PoissonGLMMObjective(par, x, y, z, gid, G, offset=offset)
    objective = vb.Objective(par, fun)
    ng = fun.n_global

    t0 = time.perf_counter()
    th = fit(objective, fun, np.zeros(par.free_size()), device_solve)
    print('fit: %.2f s, max |free gradient| %.2e, counts up to %d' % (time.perf_counter() - t0, np.max(np.abs(fun.grad(th, True))), int(y.max())))
    par.set_free(th)
    print('beta[:4] fitted %s, simulated %s' % (np.array2string(par['beta']['mean'].get()[:4], precision=3), np.array2string(beta[:4], precision=3)))
    print('mu fitted %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))

    # LRVB standard errors of beta and mu next to the mean-field ones
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    par.set_free(th)
    M = np.zeros((P + K, ng))
    M[np.arange(P), np.arange(P)] = 1.0                                   # E beta_j = m_j
    M[P + np.arange(K), 2 * P + np.arange(K)] = 1.0                       # E mu_k = e_mu_k
    se_lr = np.sqrt(np.diag(gc.lrvb_cov(M)))
    se_mf = np.concatenate([1.0 / np.sqrt(par['beta']['info'].get()), 1.0 / np.sqrt(par['mu']['info'].get())])
    names = ['beta[%d]' % j for j in range(P)] + ['mu[%d]' % k for k in range(K)]
    print('%-10s %12s %12s' % ('', 'mean-field se', 'LRVB se'))
    for k in list(range(min(P, 4))) + [P + k for k in range(K)]:
        print('%-10s %12.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))

    if '--predict' in sys.argv:
        se_u, se_u_mf = fun.ranef_se(th, on_device=True)
        print('%-10s %12s %12s' % ('', 'mean-field se', 'LRVB se'))
        for g in range(3):
            for k in range(K):
                print('%-10s %12.5f %12.5f' % ('u[%d, %d]' % (g, k), se_u_mf[g, k], se_u[g, k]))
        t0 = time.perf_counter()
        fitted = fun.predict(th, on_device=True)                          # all N rows; the group blocks are already resident
        t_fit = time.perf_counter() - t0
        x_new = rng.standard_normal((1, P)) / np.sqrt(P)
        unseen = fun.predict(th, newdata=dict(x=x_new, z=np.array([[1.0, 0.5]]), groups=[-1], offset=np.zeros(1)), on_device=True)
        print('fitted rate of %d rows in %.3f s; the linear predictor and its standard errors:' % (N, t_fit))
        print('%-12s %10s %10s %12s %10s %10s' % ('row', 'rho', 'rate', 'mean-field se', 'LRVB se', 'group'))
        for label, out, i, g in [('%d' % i, fitted, i, int(gid[i])) for i in range(4)] + [('unseen', unseen, 0, -1)]:
            print('%-12s %10.4f %10.4f %12.5f %10.5f %10s' % (label, out['rho'][i], out['mean_lrvb'][i], np.sqrt(out['var_mf'][i]),
                                                           np.sqrt(out['var_lrvb'][i]), 'population' if g < 0 else str(g)))

    # leave one cluster out: groups ranked by their streamed influence on beta[0], the top one dropped and refitted
    Mb = np.zeros((1, ng))
    Mb[0, 0] = 1.0
    t0 = time.perf_counter()
    gi = fun.group_influence(th, Mb, on_device=device_solve)[:, 0]       # d beta[0] / d (multiplier on the group's weights)
    t_gi = time.perf_counter() - t0
    top = np.argsort(-np.abs(gi))[:5]
    print('group influence on beta[0] (%.3f s): top groups %s, influence %s' % (t_gi, top.tolist(), np.array2string(gi[top], precision=5)))
    g = int(top[0])
    w = np.ones(N)
    w[gid == g] = 0.0
    fun.weights_par.set_vector(w)
    th_drop = fit(objective, fun, th, device_solve)
    fun.weights_par.set_vector(np.ones(N))
    print('drop group %d (%d rows): beta[0] predicted change %.4e, actual change %.4e'
          % (g, int(np.sum(gid == g)), -gi[g], th_drop[0] - th[0]))


if __name__ == '__main__':
    main()

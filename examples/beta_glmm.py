"""Beta mixed model -- continuous proportions strictly inside (0, 1) with a random intercept and a random slope per group -- with
linear-response covariances (glmmTMB's `beta_family(link = "logit")` with a known precision):

    y_n ~ Beta(mu_n phi, (1 - mu_n) phi),   logit mu_n = x_n . beta + z_n . u_g(n),   u_gk ~ N(mu_k, 1 / tau_k)

`BetaGLMMObjective` is fitted at the precision the data were drawn with and once more at a wrong one.  Printed: fitted against
simulated beta and mu, the LRVB standard errors of beta and mu against the mean-field ones, fitted means E sigma(t) against the
group averages of y, and value - log_norm_const() (-ELBO up to constants that do not depend on phi: the lower the better) at the
two precisions.

    python examples/beta_glmm.py [--small] [--device-solve]

--device-solve takes the Newton polish and the predictions through the device-resident block-arrow solve (`on_device=True`).
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


def params(P, K, G):
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    return par


def standard_errors(par, fun, th, P, K):
    """(mean-field, LRVB) standard errors of beta and mu at the fit th."""
    ng = fun.n_global
    gc = fun._ensure_gctx()
    fun.global_hessian(th, want_host=False)
    gc.chol_factor_last()
    par.set_free(th)
    M = np.zeros((P + K, ng))
    M[np.arange(P), np.arange(P)] = 1.0                                   # E beta_j = m_j
    M[P + np.arange(K), 2 * P + np.arange(K)] = 1.0                       # E mu_k = e_mu_k
    se_lr = np.sqrt(np.diag(gc.lrvb_cov(M)))
    se_mf = np.concatenate([1.0 / np.sqrt(par['beta']['info'].get()), 1.0 / np.sqrt(par['mu']['info'].get())])
    return se_mf, se_lr


def main():
    small = '--small' in sys.argv
    device_solve = '--device-solve' in sys.argv
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    K, phi, phi_wrong = 2, 12.0, 3.0
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    t = rng.standard_normal(N)                                            # a covariate of its own for the random slope
    z = np.stack([np.ones(N), 0.5 * t], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    tau = np.array([4.0, 8.0])
    beta, mu = rng.normal(size=P) * 0.5, np.array([-0.6, 0.4])
    u = mu[None, :] + rng.normal(size=(G, K)) / np.sqrt(tau)[None, :]
    m = 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid]).sum(1))))
    y = rng.beta(m * phi, (1.0 - m) * phi)
    inside = (y > 0.0) & (y < 1.0)                                        # exact zeros or ones are refused by the model, not clipped
    print('proportions: %d rows, %d strictly inside (0, 1), mean %.3f, variance %.4f' % (N, inside.sum(), y.mean(), y.var()))
    x, z, gid, y, m = x[inside], z[inside], gid[inside], y[inside], m[inside]
    N = y.size
    names = ['beta[%d]' % j for j in range(P)] + ['mu[%d]' % k for k in range(K)]
    shown = list(range(min(P, 4))) + [P + k for k in range(K)]

    values, th0 = {}, None
    for ph in (phi, phi_wrong):
        par = params(P, K, G)
        fun = vb.BetaGLMMObjective(par, x, y, z, gid, G, ph)
        objective = vb.Objective(par, fun)
        t0 = time.perf_counter()
        th = fit(objective, fun, np.zeros(par.free_size()) if th0 is None else th0, device_solve)
        th0 = th
        print('\nphi = %g: %.2f s, max |free gradient| %.2e' % (ph, time.perf_counter() - t0, np.max(np.abs(fun.grad(th, True)))))
        par.set_free(th)
        print('beta[:4] fitted %s, simulated %s' % (np.array2string(par['beta']['mean'].get()[:4], precision=3), np.array2string(beta[:4], precision=3)))
        print('mu fitted %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))
        se_mf, se_lr = standard_errors(par, fun, th, P, K)
        print('%-10s %14s %12s' % ('', 'mean-field se', 'LRVB se'))
        for k in shown:
            print('%-10s %14.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))
        values[ph] = fun.value(th, True) - fun.log_norm_const()
        if ph == phi:
            n = min(N, 20000)
            fitted = fun.predict(th, n0=0, n1=n, on_device=device_solve)
            print('rows 0..5: y %s' % np.array2string(y[:6], precision=3))
            print('  fitted mean (LRVB variance) %s, (mean-field) %s' % (np.array2string(fitted['mean_lrvb'][:6], precision=3),
                                                                        np.array2string(fitted['mean_mf'][:6], precision=3)))
            g = gid[:n]
            cnt = np.maximum(np.bincount(g, minlength=G), 1)
            avg_y, avg_f = np.bincount(g, weights=y[:n], minlength=G) / cnt, np.bincount(g, weights=fitted['mean_lrvb'], minlength=G) / cnt
            print('first %d rows: mean y %.4f, mean fitted %.4f; groups 0..4: average y %s, average fitted mean %s; largest gap over the groups %.4f'
                  % (n, y[:n].mean(), fitted['mean_lrvb'].mean(), np.array2string(avg_y[:5], precision=3), np.array2string(avg_f[:5], precision=3),
                     np.max(np.abs(avg_y - avg_f))))
    print('\nvalue - log_norm_const (-ELBO up to constants free of phi; lower is better): phi = %g: %.1f, phi = %g: %.1f'
          % (phi, values[phi], phi_wrong, values[phi_wrong]))


if __name__ == '__main__':
    main()

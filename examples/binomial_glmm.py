"""Binomial and negative-binomial mixed models -- aggregated successes out of trials, and over-dispersed counts, each with a
random intercept and a random slope per group -- with linear-response covariances.

    1.  y_n ~ Binomial(m_n, sigma(x_n . beta + u_g0 + t_n u_g1 / 2)),  u_gk ~ N(mu_k, 1 / tau_k)
        Simulates aggregated data (the `cbind(successes, failures)` form: N rows stand for sum m_n Bernoulli trials), fits the
        mean-field posterior and prints the LRVB standard errors of beta and mu next to the mean-field ones.
    2.  y_n ~ NB2(mean exposure_n exp(x_n . beta + z_n . u_g), dispersion phi)
        Simulates over-dispersed counts and fits `PoissonGLMMObjective` and `NegBinomialGLMMObjective` (phi known) side by
        side: the Poisson fit is over-confident, and both sets of LRVB standard errors are printed.

    python examples/binomial_glmm.py [--small] [--device-solve] [--link probit|cloglog]

--device-solve takes the Newton polish through the device-resident block-arrow solve (`on_device=True`).
--link fits model 1 alone under that link, p = Phi(.) or p = 1 - exp(-exp(.)), on data simulated under it,
and prints the LRVB standard errors against the mean-field ones, the random-effect standard errors and a few fitted means.
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


def link_model(link, rng, x, z, gid, G, lin, beta, mu, names, shown, device_solve):
    """Model 1 under the probit or the cloglog link, on data simulated under that link."""
    from scipy.special import ndtr
    if link not in ('probit', 'cloglog'):
        raise SystemExit("--link takes 'probit' or 'cloglog'")
    N, P = x.shape
    K = z.shape[1]
    trials = rng.integers(1, 21, size=N).astype(np.float64)
    p = ndtr(lin) if link == 'probit' else -np.expm1(-np.exp(lin))
    y = rng.binomial(trials.astype(np.int64), p).astype(np.float64)
    par = params(P, K, G)
    fun = vb.BinomialGLMMObjective(par, x, y, z, gid, G, trials=trials, link=link)
    objective = vb.Objective(par, fun)
    t0 = time.perf_counter()
    th = fit(objective, fun, np.zeros(par.free_size()), device_solve)
    print('binomial fit, %s link: %d rows for %d trials, %.2f s, max |free gradient| %.2e'
          % (link, N, int(trials.sum()), time.perf_counter() - t0, np.max(np.abs(fun.grad(th, True)))))
    par.set_free(th)
    print('beta[:4] fitted %s, simulated %s' % (np.array2string(par['beta']['mean'].get()[:4], precision=3), np.array2string(beta[:4], precision=3)))
    print('mu fitted %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))
    se_mf, se_lr = standard_errors(par, fun, th, P, K)
    print('%-10s %14s %12s' % ('', 'mean-field se', 'LRVB se'))
    for k in shown:
        print('%-10s %14.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))
    u_lr, u_mf = fun.ranef_se(th, on_device=device_solve)
    print('se(u_g0): mean-field median %.4f, LRVB median %.4f' % (np.median(u_mf[:, 0]), np.median(u_lr[:, 0])))
    fitted = fun.predict(th, n0=0, n1=5, on_device=device_solve)
    print('rows 0..4: successes %s of %s, fitted mean (LRVB variance) %s' % (y[:5].astype(int), trials[:5].astype(int),
                                                                           np.array2string(fitted['mean_lrvb'], precision=2)))


def main():
    small = '--small' in sys.argv
    device_solve = '--device-solve' in sys.argv
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    K = 2
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    t = rng.standard_normal(N)                                            # a covariate of its own for the random slope
    z = np.stack([np.ones(N), 0.5 * t], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, tau = rng.normal(size=P) * 0.5, np.array([0.3, -0.2]), np.array([4.0, 8.0])
    u = mu[None, :] + rng.normal(size=(G, K)) / np.sqrt(tau)[None, :]
    lin = x @ beta + (z * u[gid]).sum(1)
    names = ['beta[%d]' % j for j in range(P)] + ['mu[%d]' % k for k in range(K)]
    shown = list(range(min(P, 4))) + [P + k for k in range(K)]
    if '--link' in sys.argv:
        link_model(sys.argv[sys.argv.index('--link') + 1], rng, x, z, gid, G, lin, beta, mu, names, shown, device_solve)
        return

    # ---- 1. aggregated binomial data ----------------------------------------------------------------------------------------
    trials = rng.integers(1, 21, size=N).astype(np.float64)
    y = rng.binomial(trials.astype(np.int64), 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)
    par = params(P, K, G)
    fun = vb.BinomialGLMMObjective(par, x, y, z, gid, G, trials=trials)
    objective = vb.Objective(par, fun)
    t0 = time.perf_counter()
    th = fit(objective, fun, np.zeros(par.free_size()), device_solve)
    print('binomial fit: %d rows for %d trials, %.2f s, max |free gradient| %.2e'
          % (N, int(trials.sum()), time.perf_counter() - t0, np.max(np.abs(fun.grad(th, True)))))
    par.set_free(th)
    print('beta[:4] fitted %s, simulated %s' % (np.array2string(par['beta']['mean'].get()[:4], precision=3), np.array2string(beta[:4], precision=3)))
    print('mu fitted %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))
    se_mf, se_lr = standard_errors(par, fun, th, P, K)
    print('%-10s %14s %12s' % ('', 'mean-field se', 'LRVB se'))
    for k in shown:
        print('%-10s %14.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))
    del fun, objective

    # ---- 2. over-dispersed counts: Poisson against negative binomial ------------------------------------------------------------
    phi = 2.0
    offset = np.log(rng.uniform(0.5, 2.0, size=N))                        # log exposure
    mean = np.exp(offset + lin)
    yc = rng.poisson(mean * rng.gamma(phi, 1.0 / phi, size=N)).astype(np.float64)      # NB2: a gamma-mixed Poisson
    print('\ncounts: mean %.2f, variance %.2f (Poisson would have variance = mean)' % (yc.mean(), yc.var()))
    se = {}
    for label, make in (('Poisson', lambda p: vb.PoissonGLMMObjective(p, x, yc, z, gid, G, offset=offset)),
                        ('NB(phi=%g)' % phi, lambda p: vb.NegBinomialGLMMObjective(p, x, yc, z, gid, G, phi, offset=offset))):
        par = params(P, K, G)
        fun = make(par)
        objective = vb.Objective(par, fun)
        t0 = time.perf_counter()
        th = fit(objective, fun, np.zeros(par.free_size()), device_solve)
        print('%s fit: %.2f s, max |free gradient| %.2e' % (label, time.perf_counter() - t0, np.max(np.abs(fun.grad(th, True)))))
        se[label] = standard_errors(par, fun, th, P, K)[1]
        par.set_free(th)
        print('  beta[:4] fitted %s, simulated %s' % (np.array2string(par['beta']['mean'].get()[:4], precision=3),
                                                      np.array2string(beta[:4], precision=3)))
        del fun, objective
    labels = list(se)
    print('%-10s %14s %14s' % ('LRVB se', labels[0], labels[1]))
    for k in shown:
        print('%-10s %14.5f %14.5f' % (names[k], se[labels[0]][k], se[labels[1]][k]))


if __name__ == '__main__':
    main()

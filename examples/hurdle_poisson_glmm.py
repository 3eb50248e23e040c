"""Hurdle Poisson mixed model -- counts with more zeros than a Poisson model allows, with a random intercept and a random slope
per group in both parts -- next to a plain Poisson mixed model of the same counts, with linear-response covariances.

    P(y_n = 0) = 1 - p_n,   P(y_n = k) = p_n Poisson(k; lambda_n) / (1 - exp(-lambda_n)),  k >= 1
    logit p_n = x_n . beta^z + z_n . u^z_g(n),   log lambda_n = o_n + x_n . beta^c + z_n . u^c_g(n),   u_gk ~ N(mu_k, 1 / tau_k)

The likelihood factorises: `HurdlePoissonGLMM` holds a `BinomialGLMMObjective` on 1[y > 0] over all rows and a
`TruncatedPoissonGLMMObjective` on the rows with y > 0, fitted one after the other.  Printed: the two
models' value - log_norm_const() (-ELBO up to the same constants: the lower the better), the LRVB standard errors of beta and mu
against the mean-field ones for both parts, and fitted means E y = p E [y | y > 0] next to the Poisson model's.

    python examples/hurdle_poisson_glmm.py [--small] [--device-solve] [--dispersion PHI]

--device-solve takes the Newton polish and the predictions through the device-resident block-arrow solve (`on_device=True`).
--dispersion PHI draws the positive counts from the zero-truncated NB2 law with mean lambda_n and dispersion PHI (variance
lambda + lambda^2 / PHI before truncation) and fits a third model, `HurdleNegBinomialGLMM` with that known PHI (DESIGN.md section
39): its zero part is the hurdle Poisson model's, so only the count part, `TruncatedNegBinomialGLMMObjective`, is fitted again, and
its value - log_norm_const() is printed next to the other two.
"""
import os
import sys
import time

import numpy as np
import scipy.optimize
from scipy.special import gammaln

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
    dispersion = float(sys.argv[sys.argv.index('--dispersion') + 1]) if '--dispersion' in sys.argv else None
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    K = 2
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    t = rng.standard_normal(N)                                            # a covariate of its own for the random slope
    z = np.stack([np.ones(N), 0.5 * t], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    offset = np.log(rng.uniform(0.5, 2.0, size=N))                        # log exposure of the count part
    tau = np.array([4.0, 8.0])
    beta_z, mu_z = rng.normal(size=P) * 0.5, np.array([-0.4, 0.3])        # the hurdle: fewer than half of the rows are positive
    beta_c, mu_c = rng.normal(size=P) * 0.5, np.array([0.8, -0.2])
    u_z = mu_z[None, :] + rng.normal(size=(G, K)) / np.sqrt(tau)[None, :]
    u_c = mu_c[None, :] + rng.normal(size=(G, K)) / np.sqrt(tau)[None, :]
    p_pos = 1.0 / (1.0 + np.exp(-(x @ beta_z + (z * u_z[gid]).sum(1))))
    lam = np.exp(offset + x @ beta_c + (z * u_c[gid]).sum(1))
    # zero-truncated Poisson (or NB2) draws by inversion on (P(0), 1)
    from scipy.stats import nbinom, poisson
    if dispersion is None:
        p0 = np.exp(-lam)
        positive = poisson.ppf(p0 + rng.uniform(size=N) * (1.0 - p0), lam)
    else:
        pr = dispersion / (dispersion + lam)
        p0 = pr ** dispersion
        positive = nbinom.ppf(np.minimum(p0 + rng.uniform(size=N) * (1.0 - p0), 1.0 - 1e-12), dispersion, pr)
    y = np.where(rng.uniform(size=N) < p_pos, np.maximum(positive, 1.0), 0.0)
    print('counts: %d rows, %.1f %% zeros (a Poisson law of the same mean would have %.1f %%), mean %.2f, variance %.2f'
          % (N, 100.0 * np.mean(y == 0), 100.0 * np.exp(-y.mean()), y.mean(), y.var()))
    names = ['beta[%d]' % j for j in range(P)] + ['mu[%d]' % k for k in range(K)]
    shown = list(range(min(P, 4))) + [P + k for k in range(K)]

    # ---- the hurdle model: two independent fits ------------------------------------------------------------------------------
    par_z, par_c = params(P, K, G), params(P, K, G)
    hur = vb.HurdlePoissonGLMM(par_z, par_c, x, y, z, gid, G, offset=offset, zero_link='logit')
    th = {}
    for label, par, fun, beta, mu in (('zero part (Bernoulli, logit)', par_z, hur.zero, beta_z, mu_z),
                                      ('count part (zero-truncated Poisson, %d rows)' % hur.positive_rows.size, par_c, hur.count, beta_c, mu_c)):
        objective = vb.Objective(par, fun)
        t0 = time.perf_counter()
        th[label] = fit(objective, fun, np.zeros(par.free_size()), device_solve)
        print('\n%s: %.2f s, max |free gradient| %.2e' % (label, time.perf_counter() - t0, np.max(np.abs(fun.grad(th[label], True)))))
        par.set_free(th[label])
        print('beta[:4] fitted %s, simulated %s' % (np.array2string(par['beta']['mean'].get()[:4], precision=3), np.array2string(beta[:4], precision=3)))
        print('mu fitted %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))
        se_mf, se_lr = standard_errors(par, fun, th[label], P, K)
        print('%-10s %14s %12s' % ('', 'mean-field se', 'LRVB se'))
        for k in shown:
            print('%-10s %14.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))
    th_z, th_c = th.values()
    v_hurdle = hur.value(th_z, th_c) - hur.log_norm_const()

    # ---- a plain Poisson mixed model of the same counts ----------------------------------------------------------------------------
    par_p = params(P, K, G)
    pois = vb.PoissonGLMMObjective(par_p, x, y, z, gid, G, offset=offset)
    t0 = time.perf_counter()
    th_p = fit(vb.Objective(par_p, pois), pois, np.zeros(par_p.free_size()), device_solve)
    print('\nPoisson fit: %.2f s, max |free gradient| %.2e' % (time.perf_counter() - t0, np.max(np.abs(pois.grad(th_p, True)))))
    v_pois = pois.value(th_p, True) + float(np.sum(gammaln(y + 1.0)))     # its constant: -sum log y!
    print('\nvalue - log_norm_const (-ELBO up to common constants; lower is better): hurdle %.1f, Poisson %.1f' % (v_hurdle, v_pois))

    # ---- the hurdle NB2 model: the same zero part, the count part with the known dispersion --------------------------------------
    if dispersion is not None:
        par_n = params(P, K, G)
        hnb = vb.HurdleNegBinomialGLMM(params(P, K, G), par_n, x, y, z, gid, G, dispersion, offset=offset, zero_link='logit')
        t0 = time.perf_counter()
        th_n = fit(vb.Objective(par_n, hnb.count), hnb.count, th_c, device_solve)
        print('\ncount part (zero-truncated NB2, phi = %g): %.2f s, max |free gradient| %.2e'
              % (dispersion, time.perf_counter() - t0, np.max(np.abs(hnb.count.grad(th_n, True)))))
        par_n.set_free(th_n)
        print('beta[:4] fitted %s, simulated %s' % (np.array2string(par_n['beta']['mean'].get()[:4], precision=3), np.array2string(beta_c[:4], precision=3)))
        v_nb = hnb.value(th_z, th_n) - hnb.log_norm_const()
        print('value - log_norm_const: hurdle NB2 %.1f against hurdle Poisson %.1f (Poisson %.1f)' % (v_nb, v_hurdle, v_pois))
        fn = hnb.predict(th_z, th_n, n0=0, n1=6, on_device=device_solve)
        print('rows 0..5: hurdle NB2 E [y | y > 0] %s, E y %s' % (np.array2string(fn['mean_count_lrvb'], precision=3),
                                                                 np.array2string(fn['mean_lrvb'], precision=3)))

    fitted = hur.predict(th_z, th_c, n0=0, n1=6, on_device=device_solve)
    fp = pois.predict(th_p, n0=0, n1=6, on_device=device_solve)
    print('rows 0..5: y %s' % y[:6].astype(int))
    print('  hurdle  P(y > 0) %s' % np.array2string(fitted['p_pos_lrvb'], precision=3))
    print('  hurdle  E [y | y > 0] %s' % np.array2string(fitted['mean_count_lrvb'], precision=3))
    print('  hurdle  E y (LRVB variance) %s, (mean-field) %s' % (np.array2string(fitted['mean_lrvb'], precision=3),
                                                                 np.array2string(fitted['mean_mf'], precision=3)))
    print('  Poisson E y (LRVB variance) %s' % np.array2string(fp['mean_lrvb'], precision=3))
    full = hur.predict(th_z, th_c, n0=0, n1=min(N, 20000), on_device=device_solve)
    n = full['mean_lrvb'].size
    print('first %d rows: mean y %.3f, mean fitted E y hurdle %.3f, Poisson %.3f; share of zeros %.3f, mean fitted P(y = 0) hurdle %.3f'
          % (n, y[:n].mean(), full['mean_lrvb'].mean(), pois.predict(th_p, n0=0, n1=n, on_device=device_solve)['mean_lrvb'].mean(),
             np.mean(y[:n] == 0), 1.0 - full['p_pos_lrvb'].mean()))


if __name__ == '__main__':
    main()

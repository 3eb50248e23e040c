"""Censored Gaussian (Tobit) mixed model -- a Gaussian response of which about 30 % of the rows are only known to exceed a censoring
point, with a random intercept and a random slope per group -- with linear-response covariances and an estimated precision
(`censReg`, `lmec`, `brms(y | cens(c) ~ ..)`):

    y*_n ~ N(x_n . beta + z_n . u_g(n), 1 / phi),   u_gk ~ N(mu_k, 1 / tau_k),   y_n = min(y*_n, c_n),   status +1 where y*_n > c_n

`CensoredNormalGLMMObjective` is built with phi0 = phi / 4 and the precision 1 / sigma^2 is estimated by `fit_dispersion` (profile Newton
on lambda = log(phi / phi0)).  Printed: the lambda path, beta fitted by the censored model next to the fit that wrongly treats the
censored rows as observed and next to the simulated values, phi-hat of both, the LRVB standard errors of beta and mu against the
mean-field ones, and the fitted latent means of censored rows against the censoring points.

    python examples/censored_glmm.py [--small] [--device-solve] [--survival]

--device-solve takes the Newton polish, the sensitivities and the predictions through the device-resident block-arrow solve
(`on_device=True`).  --survival reads the same data as log-times: T = exp(y*) are event times, the study ends at C = exp(c), the
model is the log-normal accelerated-failure-time model with shared frailties (`survreg(dist = "lognormal") + frailty`), fitted on
log min(T, C), and the acceleration factors exp(beta) and the median survival times exp(fitted) are printed.
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


def estimate(label, x, y, z, gid, G, P, K, phi0, status, device_solve):
    """The model with the given status fitted with an estimated precision: (par, fun, out of fit_dispersion)."""
    par = params(P, K, G)
    fun = vb.CensoredNormalGLMMObjective(par, x, y, z, gid, G, phi0, censoring=status)
    objective = vb.Objective(par, fun)

    def inner(f, start):
        t0 = time.perf_counter()
        th = fit(objective, f, start, device_solve)
        slope, curv = f.dispersion_profile(th, on_device=device_solve)
        print('  %s: lambda %+.6f   phi %9.4f   profile slope %+.4e   curvature %.4e   (%.2f s)'
              % (label, f.log_dispersion, phi0 * np.exp(f.log_dispersion), slope, curv, time.perf_counter() - t0), flush=True)
        return th

    return par, fun, fun.fit_dispersion(inner, np.zeros(par.free_size()))


def main():
    small = '--small' in sys.argv
    device_solve = '--device-solve' in sys.argv
    survival = '--survival' in sys.argv
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    K, phi = 2, 4.0
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), 0.5 * rng.standard_normal((N, 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, tau = 0.8 * rng.standard_normal(P), np.array([0.8, -0.2]), np.array([4.0, 9.0])
    u = mu[None, :] + rng.standard_normal((G, K)) / np.sqrt(tau)[None, :]
    t = x @ beta + (z * u[gid]).sum(1)
    ystar = t + rng.standard_normal(N) / np.sqrt(phi)
    cut = np.quantile(ystar, 0.7) + 0.6 * rng.standard_normal(N)          # the censoring points: about 30 % of the latent values lie above theirs
    status = (ystar > cut).astype(np.int32)
    y = np.where(status == 1, cut, ystar)
    what = 'log-times' if survival else 'responses'
    print('%s: %d rows, %.1f %% right-censored; mean of the recorded values %.3f, of the latent ones %.3f'
          % (what, N, 100.0 * status.mean(), y.mean(), ystar.mean()))
    if survival:
        print('  event or end of study at exp(y): median recorded time %.3f, median event time %.3f' % (np.median(np.exp(y)), np.median(np.exp(ystar))))
    print('censored Gaussian mixed model, N = %d, P = %d, G = %d, K = %d: simulated phi = %g (sigma = %.3f), phi0 = %g' % (N, P, G, K, phi, phi ** -0.5, phi / 4.0))
    par, fun, out = estimate('censored', x, y, z, gid, G, P, K, phi / 4.0, status, device_solve)
    par_n, fun_n, out_n = estimate('ignoring the censoring', x, y, z, gid, G, P, K, phi / 4.0, None, device_solve)
    th, th_n = out['theta'], out_n['theta']
    print('phi-hat = %.4f (censored fit), %.4f (censored rows taken as observed), simulated %.4f; lambda-hat %.6f after %d steps'
          % (phi / 4.0 * out['phi_scale'], phi / 4.0 * out_n['phi_scale'], phi, out['lam'], out['iterations']))
    print('standard error of lambda-hat from the profile curvature: %.4f' % (1.0 / np.sqrt(out['curvature'])))
    par.set_free(th)
    par_n.set_free(th_n)
    b, b_n = par['beta']['mean'].get(), par_n['beta']['mean'].get()
    print('%-10s %12s %12s %24s' % ('', 'simulated', 'censored fit', 'ignoring the censoring'))
    for j in range(min(P, 6)):
        print('%-10s %12.4f %12.4f %24.4f' % ('beta[%d]' % j, beta[j], b[j], b_n[j]))
    print('root mean square error of beta: censored fit %.4f, ignoring the censoring %.4f (attenuated towards zero)'
          % (np.sqrt(np.mean((b - beta) ** 2)), np.sqrt(np.mean((b_n - beta) ** 2))))
    print('mu fitted %s, ignoring the censoring %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3),
                                                                      np.array2string(par_n['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))
    if survival:
        print('acceleration factors exp(beta[:4]): fitted %s, simulated %s' % (np.array2string(np.exp(b[:4]), precision=3), np.array2string(np.exp(beta[:4]), precision=3)))
    se_mf, se_lr = standard_errors(par, fun, th, P, K)
    names = ['beta[%d]' % j for j in range(P)] + ['mu[%d]' % k for k in range(K)]
    print('%-10s %14s %12s' % ('', 'mean-field se', 'LRVB se'))
    for k in list(range(min(P, 4))) + [P + k for k in range(K)]:
        print('%-10s %14.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))
    n = min(N, 20000)
    fitted = fun.predict(th, n0=0, n1=n, on_device=device_solve)
    c = status[:n] == 1
    print('first %d rows: fitted latent mean against the latent value, rms %.4f (sigma %.4f); censored rows: fitted mean above the censoring point on %.1f %%'
          % (n, np.sqrt(np.mean((fitted['mean_lrvb'] - ystar[:n]) ** 2)), phi ** -0.5, 100.0 * np.mean(fitted['mean_lrvb'][c] > y[:n][c])))
    print('rows 0..5: status %s, recorded %s' % (status[:6], np.array2string(y[:6], precision=3)))
    print('  fitted latent mean %s, its LRVB sd %s, mean-field sd %s' % (np.array2string(fitted['mean_lrvb'][:6], precision=3),
                                                                       np.array2string(np.sqrt(fitted['var_lrvb'][:6]), precision=3),
                                                                       np.array2string(np.sqrt(fitted['var_mf'][:6]), precision=3)))
    if survival:
        print('  median survival time exp(fitted) %s' % np.array2string(np.exp(fitted['mean_lrvb'][:6]), precision=3))


if __name__ == '__main__':
    main()

"""Gamma mixed model with a log link -- right-skewed positive amounts (costs, durations, concentrations) with a random intercept and
a random slope per group -- with linear-response covariances and an estimated shape (DESIGN.md section 43;
`glmer(family = Gamma(link = "log"))`):

    y_n ~ Gamma(shape phi, mean mu_n),   log mu_n = x_n . beta + z_n . u_g(n),   u_gk ~ N(mu_k, 1 / tau_k)

`GammaGLMMObjective` is built with phi0 = phi / 4 and the shape is estimated by `fit_dispersion` (profile Newton on lambda =
log(phi / phi0)).  Printed: the lambda path, fitted against simulated beta and mu, the LRVB standard errors of beta and mu against the
mean-field ones, the refitted change of beta and mu from phi0 to phi-hat against the change predicted by the linear response (in one
step from phi0, and integrated along the path), and fitted means exp(rho + var / 2) against the group averages of y.

    python examples/gamma_glmm.py [--small] [--device-solve] [--two-part]

--device-solve takes the Newton polish, the sensitivities and the predictions through the device-resident block-arrow solve
(`on_device=True`).  --two-part sets a share of the responses to zero and fits `HurdleGammaGLMM` (zeros plus positive amounts):
P(y > 0), E[y | y > 0] and their product against the group averages.
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


def group_averages(gid, G, *cols):
    cnt = np.maximum(np.bincount(gid, minlength=G), 1)
    return [np.bincount(gid, weights=c, minlength=G) / cnt for c in cols]


def two_part(x, y, z, gid, G, P, K, phi, device_solve):
    par_zero, par_pos = params(P, K, G), params(P, K, G)
    H = vb.HurdleGammaGLMM(par_zero, par_pos, x, y, z, gid, G, phi)
    print('two-part model: %d rows, %d zeros, %d positive amounts' % (y.size, int(np.sum(y == 0.0)), H.positive_rows.size))
    t0 = time.perf_counter()
    th_zero = fit(vb.Objective(par_zero, H.zero), H.zero, np.zeros(par_zero.free_size()), device_solve)
    th_pos = fit(vb.Objective(par_pos, H.count), H.count, np.zeros(par_pos.free_size()), device_solve)
    print('both parts fitted in %.2f s; value - log_norm_const %.1f' % (time.perf_counter() - t0, H.value(th_zero, th_pos) - H.log_norm_const()))
    n = min(y.size, 20000)
    out = H.predict(th_zero, th_pos, n0=0, n1=n, on_device=device_solve)
    g = gid[:n]
    avg_pos, avg_y, avg_p, avg_m = group_averages(g, G, (y[:n] > 0.0).astype(np.float64), y[:n], out['p_pos_lrvb'], out['mean_lrvb'])
    print('first %d rows: share of positive rows %.4f, mean P(y > 0) %.4f; mean y %.4f, mean E y %.4f'
          % (n, np.mean(y[:n] > 0.0), out['p_pos_lrvb'].mean(), y[:n].mean(), out['mean_lrvb'].mean()))
    print('groups 0..4: share positive %s, P(y > 0) %s' % (np.array2string(avg_pos[:5], precision=3), np.array2string(avg_p[:5], precision=3)))
    print('groups 0..4: average y %s, E y = P(y > 0) E[y | y > 0] %s' % (np.array2string(avg_y[:5], precision=3), np.array2string(avg_m[:5], precision=3)))
    print('rows 0..5: E[y | y > 0] under the LRVB variance %s, under the mean-field one %s'
          % (np.array2string(out['mean_count_lrvb'][:6], precision=3), np.array2string(out['mean_count_mf'][:6], precision=3)))


def main():
    small = '--small' in sys.argv
    device_solve = '--device-solve' in sys.argv
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    K, phi = 2, 6.0
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), 0.5 * rng.standard_normal((N, 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, tau = 0.6 * rng.standard_normal(P), np.array([0.8, -0.2]), np.array([4.0, 9.0])
    u = mu[None, :] + rng.standard_normal((G, K)) / np.sqrt(tau)[None, :]
    t = x @ beta + (z * u[gid]).sum(1)
    y = rng.gamma(phi, np.exp(t) / phi)
    if '--two-part' in sys.argv:
        p_pos = 1.0 / (1.0 + np.exp(-(0.7 + 0.5 * x[:, 0] + 0.6 * (u[gid, 0] - mu[0]))))
        y = np.where(rng.uniform(size=N) < p_pos, y, 0.0)
        two_part(x, y, z, gid, G, P, K, phi, device_solve)
        return
    print('amounts: %d rows, mean %.3f, median %.3f, largest %.1f (right-skewed: shape %g)' % (N, y.mean(), np.median(y), y.max(), phi))
    par = params(P, K, G)
    fun = vb.GammaGLMMObjective(par, x, y, z, gid, G, phi / 4.0)
    objective = vb.Objective(par, fun)
    D = par.free_size()
    idx = np.concatenate([np.arange(P), 2 * P + np.arange(K)])
    M = np.eye(D)[idx]
    names = ['beta[%d]' % j for j in range(P)] + ['mu[%d]' % k for k in range(K)]
    shown = list(range(min(P, 4))) + [P + k for k in range(K)]
    path = []                                                             # (lambda, theta, d moments / d lambda) at every inner fit

    def inner(f, start):
        t0 = time.perf_counter()
        th = fit(objective, f, start, device_solve)
        slope, curv = f.dispersion_profile(th, on_device=device_solve)
        path.append((f.log_dispersion, th.copy(), f.dispersion_sensitivity(th, M, on_device=device_solve)))
        print('  lambda %+.6f   phi %9.4f   profile slope %+.4e   curvature %.4e   (%.2f s)'
              % (f.log_dispersion, phi / 4.0 * np.exp(f.log_dispersion), slope, curv, time.perf_counter() - t0), flush=True)
        return th

    print('Gamma mixed model, N = %d, P = %d, G = %d, K = %d: simulated phi = %g, phi0 = %g' % (N, P, G, K, phi, phi / 4.0))
    out = fun.fit_dispersion(inner, np.zeros(D))
    th, lam = out['theta'], out['lam']
    print('phi-hat = %.4f (simulated %.4f), lambda-hat = %.6f after %d steps; slope %.2e, curvature %.4e'
          % (phi / 4.0 * out['phi_scale'], phi, lam, out['iterations'], out['slope'], out['curvature']))
    print('standard error of lambda-hat from the profile curvature: %.4f' % (1.0 / np.sqrt(out['curvature'])))
    par.set_free(th)
    print('beta[:4] fitted %s, simulated %s' % (np.array2string(par['beta']['mean'].get()[:4], precision=3), np.array2string(beta[:4], precision=3)))
    print('mu fitted %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))
    se_mf, se_lr = standard_errors(par, fun, th, P, K)
    print('%-10s %14s %12s' % ('', 'mean-field se', 'LRVB se'))
    for k in shown:
        print('%-10s %14.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))
    # the whole path from phi0 to phi-hat: the refitted change of beta and mu against two predictions of it -- one linear step from
    # phi0 (a step of lambda-hat, far outside the linear range), and the linear response integrated along the path of the inner fits
    # (trapezoid rule over its lambdas in increasing order)
    path.sort(key=lambda p: p[0])
    path = [p for p in path if p[0] <= lam + 1e-12]
    one_step, actual = lam * path[0][2], (th - path[0][1])[idx]
    along = sum((b[0] - a[0]) * 0.5 * (a[2] + b[2]) for a, b in zip(path[:-1], path[1:]))
    print('from phi0 to phi-hat (lambda = %.3f): change of the moments, refitted against predicted' % lam)
    for k in shown:
        print('  %-8s refit %+.5e   one linear step from phi0 %+.5e   linear response along the path %+.5e' % (names[k], actual[k], one_step[k], along[k]))
    print('largest difference: one step %.2e, along the path %.2e, against the largest change %.2e'
          % (np.max(np.abs(one_step - actual)), np.max(np.abs(along - actual)), np.max(np.abs(actual))))
    n = min(N, 20000)
    fitted = fun.predict(th, n0=0, n1=n, on_device=device_solve)
    print('rows 0..5: y %s' % np.array2string(y[:6], precision=3))
    print('  fitted mean (LRVB variance) %s, (mean-field) %s' % (np.array2string(fitted['mean_lrvb'][:6], precision=3),
                                                                np.array2string(fitted['mean_mf'][:6], precision=3)))
    avg_y, avg_f = group_averages(gid[:n], G, y[:n], fitted['mean_lrvb'])
    print('first %d rows: mean y %.4f, mean fitted %.4f; groups 0..4: average y %s, average fitted mean %s'
          % (n, y[:n].mean(), fitted['mean_lrvb'].mean(), np.array2string(avg_y[:5], precision=3), np.array2string(avg_f[:5], precision=3)))


if __name__ == '__main__':
    main()

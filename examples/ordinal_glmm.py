"""Ordinal mixed model -- a rating on J = 5 ordered categories with a random intercept and a random slope per group -- with estimated
thresholds and linear-response covariances (`ordinal::clmm`, `brms(family = cumulative)`):

    P(y_n <= j | t_n) = sigma(alpha_{j+1} - t_n),   t_n = x_n . beta + z_n . u_g(n),   u_gk ~ N(mu_k, 1 / tau_k)

`OrdinalGLMMObjective` is started from equally spaced thresholds and the spacings are estimated by `fit_thresholds` (profile Newton on
gamma_j = log(alpha_{j+1} - alpha_j), alpha_1 held fixed: a common shift is not identified against mu_0).  Printed: the path of the
thresholds, beta fitted next to the simulated values, the LRVB standard errors of beta and mu against the mean-field ones, the change
of beta predicted by `threshold_sensitivity` for a moved threshold against a refit, and the fitted category shares against the
observed ones.

    python examples/ordinal_glmm.py [--small] [--device-solve]

--device-solve takes the Newton polish, the sensitivities and the predictions through the device-resident block-arrow solve
(`on_device=True`).
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
    K, J = 2, 5
    alpha = np.array([0.0, 0.7, 1.9, 2.6])
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), 0.5 * rng.standard_normal((N, 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, tau = 0.8 * rng.standard_normal(P), np.array([1.2, -0.2]), np.array([4.0, 9.0])
    u = mu[None, :] + rng.standard_normal((G, K)) / np.sqrt(tau)[None, :]
    t = x @ beta + (z * u[gid]).sum(1)
    y = np.searchsorted(alpha, t + rng.logistic(size=N))
    shares = np.bincount(y, minlength=J) / N
    print('ordinal mixed model, N = %d, P = %d, G = %d, K = %d, J = %d: observed shares %s' % (N, P, G, K, J, np.array2string(shares, precision=4)))
    start = alpha[0] + np.arange(J - 1, dtype=np.float64)
    par = params(P, K, G)
    fun = vb.OrdinalGLMMObjective(par, x, y, z, gid, G, start)
    objective = vb.Objective(par, fun)

    def inner(f, th0):
        t0 = time.perf_counter()
        th = fit(objective, f, th0, device_solve)
        slope, S = f.threshold_profile(th, on_device=device_solve)
        print('  thresholds %s   largest profile slope %.3e   smallest curvature %.3e   (%.2f s)'
              % (np.array2string(f.thresholds, precision=5), np.max(np.abs(slope)), np.min(np.linalg.eigvalsh(S)), time.perf_counter() - t0), flush=True)
        return th

    print('path of the thresholds from equal spacings %s (simulated %s):' % (start, alpha))
    out = fun.fit_thresholds(inner, np.zeros(par.free_size()))
    th = out['theta']
    se_gamma = np.sqrt(np.diag(np.linalg.inv(out['curvature'])))
    print('thresholds fitted %s after %d steps; standard errors of the log-spacings from the profile curvature %s'
          % (np.array2string(out['thresholds'], precision=4), out['iterations'], np.array2string(se_gamma, precision=4)))
    par.set_free(th)
    b = par['beta']['mean'].get().copy()
    print('%-10s %12s %12s' % ('', 'simulated', 'fitted'))
    for j in range(min(P, 6)):
        print('%-10s %12.4f %12.4f' % ('beta[%d]' % j, beta[j], b[j]))
    print('mu fitted %s, simulated %s' % (np.array2string(par['mu']['mean'].get(), precision=3), np.array2string(mu, precision=3)))
    se_mf, se_lr = standard_errors(par, fun, th, P, K)
    names = ['beta[%d]' % j for j in range(P)] + ['mu[%d]' % k for k in range(K)]
    print('%-10s %14s %12s' % ('', 'mean-field se', 'LRVB se'))
    for k in list(range(min(P, 4))) + [P + k for k in range(K)]:
        print('%-10s %14.5f %12.5f' % (names[k], se_mf[k], se_lr[k]))
    # the change of beta predicted for a moved threshold against a refit
    fitted_alpha = out['thresholds']
    h = 0.05
    dth = fun.threshold_sensitivity(th, on_device=device_solve)[:, 1]
    moved = fitted_alpha.copy()
    moved[1] += h
    fun.threshold_par.set_vector(moved)
    th_moved = fit(objective, fun, th + h * dth, device_solve)
    fun.threshold_par.set_vector(fitted_alpha)
    print('alpha_2 moved by %+.2f: change of beta[:4] predicted %s, refitted %s'
          % (h, np.array2string(h * dth[:4], precision=5), np.array2string((th_moved - th)[:4], precision=5)))
    n = min(N, 20000)
    fitted = fun.predict(th, n0=0, n1=n, on_device=device_solve)
    print('first %d rows: fitted category shares %s (LRVB), %s (mean-field), observed %s'
          % (n, np.array2string(fitted['prob_lrvb'].mean(0), precision=4), np.array2string(fitted['prob_mf'].mean(0), precision=4),
             np.array2string(np.bincount(y[:n], minlength=J) / n, precision=4)))
    print('rows 0..3: category %s, P(y <= j) %s' % (y[:4], np.array2string(fitted['cumprob_lrvb'][:4], precision=3).replace('\n', '')))


if __name__ == '__main__':
    main()

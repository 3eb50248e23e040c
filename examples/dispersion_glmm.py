"""Estimated dispersion: the precision of a Beta mixed model, or the dispersion of an NB2 one, as the declared
hyper-parameter lambda = `log_dispersion_par` of phi = e^lambda phi0.

Data are simulated at a known phi and the model is built at phi0 = phi / 4.  `fit_dispersion` then runs a profile Newton iteration
on lambda (slope and curvature of min_theta F(theta, lambda), F = value - log_norm_const(), from one extra pass over the rows and
one block-arrow solve per step).  Printed: the path of lambda, phi-hat against the simulated phi, and -- the library's main
product -- the change of beta and mu that `dispersion_sensitivity` PREDICTS for a step of 0.2 in lambda next to what a refit gives.

    python examples/dispersion_glmm.py [--small] [--family beta|negbin] [--device-solve]

--device-solve takes the Newton polish and the sensitivity through the device-resident block-arrow solve (`on_device=True`).
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


def main():
    small = '--small' in sys.argv
    device_solve = '--device-solve' in sys.argv
    family = sys.argv[sys.argv.index('--family') + 1] if '--family' in sys.argv else 'beta'
    if family not in ('beta', 'negbin'):
        raise SystemExit('--family beta|negbin')
    N, P, G = (20000, 8, 200) if small else (1000000, 64, 10000)
    K = 2
    phi = 12.0 if family == 'beta' else 3.0
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, P)) / np.sqrt(P)
    z = np.concatenate([np.ones((N, 1)), 0.5 * rng.standard_normal((N, 1))], axis=1)
    gid = rng.integers(0, G, size=N).astype(np.int32)
    beta, mu, tau = 0.6 * rng.standard_normal(P), np.array([0.3, -0.2]), np.array([4.0, 9.0])
    u = mu[None, :] + rng.standard_normal((G, K)) / np.sqrt(tau)[None, :]
    t = x @ beta + (z * u[gid]).sum(1)
    par = params(P, K, G)
    if family == 'beta':
        m = 1.0 / (1.0 + np.exp(-t))
        y = np.clip(rng.beta(m * phi, (1.0 - m) * phi), 1e-12, 1.0 - 1e-12)
        fun = vb.BetaGLMMObjective(par, x, y, z, gid, G, phi / 4.0)
    else:
        m = np.exp(1.0 + t)
        y = rng.poisson(rng.gamma(phi, m / phi)).astype(np.float64)
        fun = vb.NegBinomialGLMMObjective(par, x, y, z, gid, G, phi / 4.0, offset=np.ones(N))
    objective = vb.Objective(par, fun)
    D = par.free_size()

    path = []

    def inner(f, start):
        t0 = time.perf_counter()
        th = fit(objective, f, start, device_solve)
        slope, curv = f.dispersion_profile(th, on_device=device_solve)
        path.append((f.log_dispersion, slope, curv, time.perf_counter() - t0))
        print('  lambda %+.6f   phi %9.4f   profile slope %+.4e   curvature %.4e   (%.2f s)'
              % (f.log_dispersion, phi / 4.0 * np.exp(f.log_dispersion), slope, curv, path[-1][3]), flush=True)
        return th

    print('%s mixed model, N = %d, P = %d, G = %d, K = %d: simulated phi = %g, phi0 = %g' % (family, N, P, G, K, phi, phi / 4.0))
    out = fun.fit_dispersion(inner, np.zeros(D))
    th, lam = out['theta'], out['lam']
    print('phi-hat = %.4f (simulated %.4f), lambda-hat = %.6f after %d steps; slope %.2e, curvature %.4e'
          % (phi / 4.0 * out['phi_scale'], phi, lam, out['iterations'], out['slope'], out['curvature']))
    print('standard error of lambda-hat from the profile curvature: %.4f' % (1.0 / np.sqrt(out['curvature'])))

    # the linear response of the fit to lambda against a refit
    idx = np.concatenate([np.arange(P), 2 * P + np.arange(K)])
    M = np.eye(D)[idx]
    step = 0.2
    pred = step * fun.dispersion_sensitivity(th, M, on_device=device_solve)
    fun.log_dispersion_par.set_vector(np.array([lam + step]))
    th2 = fit(objective, fun, th + step * fun.dispersion_sensitivity(th, on_device=device_solve), device_solve)
    fun.log_dispersion_par.set_vector(np.array([lam]))
    actual = (th2 - th)[idx]
    print('a step of %.1f in lambda: predicted against refitted change' % step)
    for j, (p, a) in enumerate(zip(pred, actual)):
        if j < 4 or j >= P:
            print('  %-8s predicted %+.5e   refit %+.5e' % ('beta[%d]' % j if j < P else 'mu[%d]' % (j - P), p, a))
    print('largest difference %.2e against the largest change %.2e' % (np.max(np.abs(pred - actual)), np.max(np.abs(actual))))


if __name__ == '__main__':
    main()

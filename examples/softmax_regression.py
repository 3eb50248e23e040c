"""Multinomial (softmax) logistic regression with K classes: a trust-region Newton-CG fit on matrix-free Hessian-vector products,
the LRVB standard errors of a few coefficients, the weight sensitivity of one coefficient for every row (streamed, nothing of
size D x N is formed), a refit without the 0.5 % of rows that push that coefficient hardest one way against its linear
prediction, and the wall time of value + gradient, one Hessian-vector product and one Hessian build.  Runs on one GPU:

    python -c "import __graft_entry__ as g; g.build()"
    python examples/softmax_regression.py            # N = 1e6, P = 256, K = 10 (D = 2304)
    python examples/softmax_regression.py --small    # N = 20000, P = 32, K = 4
"""
import os
import sys
import time

import numpy as np
import scipy.optimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lrvb_amd as vb                                               # noqa: E402

small = '--small' in sys.argv
N, P, K = (20_000, 32, 4) if small else (1_000_000, 256, 10)
D = (K - 1) * P
rng = np.random.default_rng(3)
x = rng.normal(size=(N, P)) / np.sqrt(P)
btrue = rng.normal(size=(K - 1, P)) * 1.5
z = np.hstack([np.zeros((N, 1)), x @ btrue.T])
u = rng.gumbel(size=z.shape)
y = np.argmax(z + u, axis=1).astype(np.int32)                       # softmax sampling by the Gumbel-max trick
del z, u

par = vb.ModelParamsDict('par')
par.push_param(vb.ArrayParam('beta', shape=(K - 1, P)))
fun = vb.SoftmaxRegressionObjective(par, x, y, K, prior_info=1.0)
objective = vb.Objective(par, fun)


def fit(x0):
    """trust-ncg on matrix-free products; then value-free Newton steps (H^-1 g by CG on the same products): near the optimum
    the value, a sum over N rows, resolves decreases only to ~1e-16 of itself and trust-ncg's ratio test stalls."""
    res = scipy.optimize.minimize(objective.fun_free, x0=x0, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp,
                                  method='trust-ncg', options={'gtol': 1e-8, 'maxiter': 100})
    x, newton = res.x, 0
    for _ in range(3):
        g = objective.fun_free_grad(x)
        if np.max(np.abs(g)) <= 1e-8:
            break
        x, newton = x - fun.cg_solve(x, g, tol=1e-10)[0], newton + 1
    res.x, res.newton = x, newton
    return res


t0 = time.perf_counter()
res = fit(np.zeros(D))
opt = res.x
print('N = {}, P = {}, K = {} (D = {}): trust-ncg {} iterations, {} products, {} Newton-CG steps, |grad| = {:.1e}, {:.2f} s'.format(
    N, P, K, D, res.nit, res.nhev, res.newton, np.max(np.abs(objective.fun_free_grad(opt))), time.perf_counter() - t0))

# LRVB (Laplace) standard errors of the first coefficient of each class
w0 = fun.weights_par.get_vector().copy()
sens = vb.ParametricSensitivityLinearApproximation(fun, par, fun.weights_par, opt, w0, stream_hyper=True)
idx = [a * P for a in range(K - 1)]
M = np.eye(D)[idx]
se = np.sqrt(np.diag(sens.get_lrvb_cov(M)))
for a, (i, s) in enumerate(zip(idx, se)):
    print('beta[{}, 0] = {:+.4f} +- {:.4f}   (true {:+.4f})'.format(a, opt[i], s, btrue[a, 0]))

# weight sensitivity of beta[0, 0] for every row, streamed from the resident factor
t0 = time.perf_counter()
infl = sens.get_doutput_dhyper_rows(M[:1])[:, 0]
print('d beta[0, 0] / d w_n for all {} rows: {:.3f} s'.format(N, time.perf_counter() - t0))

# drop the 0.5 % of rows whose removal raises beta[0, 0] most (removal = w_n: 1 -> 0, change -infl_n), then refit
n_drop = max(1, N // 200)
drop = np.argsort(infl)[:n_drop]
predicted = opt[0] - infl[drop].sum()
w1 = w0.copy()
w1[drop] = 0.0
fun.weights_par.set_vector(w1)
refit = fit(opt).x
fun.weights_par.set_vector(w0)
print('drop {} rows: beta[0, 0] {:+.4f} -> predicted {:+.4f}, refit {:+.4f} (LRVB se {:.4f})'.format(
    n_drop, opt[0], predicted, refit[0], se[0]))

# timings at the optimum (one warm call first)
v = rng.normal(size=D)


def timed(f, reps):
    f()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    return (time.perf_counter() - t) / reps * 1e3


b = opt
print('value + gradient: {:.2f} ms'.format(timed(lambda: fun.ctx.softmax_terms(b, K, want_hess=False), 10)))
print('Hessian-vector product: {:.2f} ms'.format(timed(lambda: fun.ctx.softmax_hvp(b, K, v), 10)))
print('Hessian build ({} SYRK blocks): {:.2f} ms'.format(K * (K - 1) // 2, timed(lambda: fun.ctx.softmax_terms(b, K), 3)))

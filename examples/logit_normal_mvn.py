"""Logistic regression with a full-covariance Gaussian posterior q(beta) = N(m, Lambda^-1) next to the mean-field fit of the
same data: the mean-field sd, its linear-response (LRVB) correction, the full-covariance VB sd and its LRVB sd, then the wall
time of one Hessian build, one gradient and one Hessian-vector product at the large size.  Runs on one GPU:

    python -c "import __graft_entry__ as g; g.build()"
    python examples/logit_normal_mvn.py [P] [N] [P_big] [N_big]
"""
import os
import sys
import time

import numpy as np
import scipy.optimize

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lrvb_amd as vb                                               # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 6
N = int(float(sys.argv[2])) if len(sys.argv) > 2 else 5000
P_big = int(sys.argv[3]) if len(sys.argv) > 3 else 64
N_big = int(float(sys.argv[4])) if len(sys.argv) > 4 else 1_000_000
rng = np.random.default_rng(7)
x = rng.normal(size=(N, P)) / np.sqrt(P)
x[:, 1] = 0.8 * x[:, 0] + 0.2 * x[:, 1]                             # correlated covariates: the mean field underestimates
y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-x @ (rng.normal(size=P) * 2.0)))).astype(np.float64)


def fit(par, fun, D):
    objective = vb.Objective(par, fun)
    opt = scipy.optimize.minimize(objective.fun_free, jac=objective.fun_free_grad, hessp=objective.fun_free_hvp,
                                  x0=np.zeros(D), method='trust-ncg', options={'gtol': 1e-8})
    H = objective.fun_free_hessian(opt.x)
    fun.ctx.chol_factor(H)
    return opt.x, np.sqrt(np.diag(fun.ctx.lrvb_cov(np.eye(D)[:P])))


par_mf = vb.ModelParamsDict('mf')
par_mf.push_param(vb.UVNParamVector('beta', length=P))
th_mf, lrvb_mf = fit(par_mf, vb.LogitNormalRegressionObjective(par_mf, x, y, prior_info=0.5), 2 * P)
par_mf.set_free(th_mf)

par = vb.ModelParamsDict('full')
par.push_param(vb.MVNParam('beta', dim=P))
D = P + P * (P + 1) // 2
th, lrvb_full = fit(par, vb.LogitNormalMVNRegressionObjective(par, x, y, prior_info=0.5), D)
par.set_free(th)

np.set_printoptions(precision=4, suppress=True)
print('mean-field sd          :', 1.0 / np.sqrt(par_mf['beta']['info'].get()))
print('mean-field LRVB sd     :', lrvb_mf)
print('full-covariance VB sd  :', np.sqrt(np.diag(par['beta'].cov())))
print('full-covariance LRVB sd:', lrvb_full)

# timing at the large size (device work synchronised by the host copies of each call)
xb = rng.normal(size=(N_big, P_big)) / np.sqrt(P_big)
yb = (rng.uniform(size=N_big) < 1.0 / (1.0 + np.exp(-xb @ rng.normal(size=P_big)))).astype(np.float64)
parb = vb.ModelParamsDict('big')
parb.push_param(vb.MVNParam('beta', dim=P_big))
fb = vb.LogitNormalMVNRegressionObjective(parb, xb, yb)
Db = P_big + P_big * (P_big + 1) // 2
Lam = np.eye(P_big) + 0.25 * (xb.T @ xb)
eta = np.concatenate([np.zeros(P_big), Lam[np.tril_indices(P_big)]])
m, S, _ = fb._point(eta)
v = rng.normal(size=Db)
fb.mvn_terms(m, S)                                                   # warm-up: buffers
fb.hessian(eta, False); fb.grad(eta, False); fb.hvp(eta, v, False)
for name, f in (('data-term Hessian (m, vech Sigma)', lambda: fb.mvn_terms(m, S)),
                ('Hessian (m, vech Lambda)', lambda: fb.hessian(eta, False)),
                ('value + gradient', lambda: fb.grad(eta, False)),
                ('Hessian-vector product', lambda: fb.hvp(eta, v, False))):
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    print('N = %d, P = %d, D = %d: %-34s %8.1f ms (best of 3)' % (N_big, P_big, Db, name, 1e3 * min(ts)))

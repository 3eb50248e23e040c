"""Times the logistic mixed model with random slopes (DESIGN.md sections 18 and 19) next to the random-intercept class at N rows,
P coefficients, G groups, Q outputs: per model the value-only terms call (the rows pass), the influence row entry over all N and
the group entry, four times each -- first `LogisticGLMMObjective`, then `LogisticGLMMSlopesObjective` at K = 1 with z = 1 (the same
model), then at K = 4.  Wall times include the host copies (the N x Q result is 128 MB at the default shape); run under
`rocprofv3 --kernel-trace --stats` for the kernel durations: the dispatches of one kernel name appear in this order, four per
model."""
import sys, os, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import lrvb_amd as vb
N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000000
P = int(sys.argv[2]) if len(sys.argv) > 2 else 64
G = int(float(sys.argv[3])) if len(sys.argv) > 3 else 10000
Q = int(sys.argv[4]) if len(sys.argv) > 4 else 16
KS = 4
rng = np.random.default_rng(1)
x = rng.standard_normal((N, P)) / np.sqrt(P)
zs = np.concatenate([np.ones((N, 1)), rng.standard_normal((N, KS - 1))], axis=1)
gid = rng.integers(0, G, size=N).astype(np.int32)
u, beta = rng.normal(size=(G, KS)) * 0.7, rng.normal(size=P) * 0.8
y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + (zs * u[gid]).sum(1))))).astype(np.float64)
w = rng.uniform(0.5, 1.5, size=N)
v = np.full(P, np.exp(-6.0))


def run(label, terms, rows, groups):
    for rep in range(4):
        t0 = time.perf_counter(); val = terms(); t1 = time.perf_counter()
        r = rows(); t2 = time.perf_counter()
        g = groups(); t3 = time.perf_counter()
        print('%s N = %d, P = %d, G = %d, Q = %d: value-only terms %.2f ms, rows (N x Q to the host) %.2f ms, group influence %.2f ms'
              % (label, N, P, G, Q, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), flush=True)
    print('%s value %.6e, |rows| %.3e, |groups| %.3e' % (label, val, np.abs(r).max(), np.abs(g).max()), flush=True)
    return r, g


par = vb.ModelParamsDict('params')
par.push_param(vb.UVNParamVector('beta', length=P))
par.push_param(vb.UVNParam('mu'))
par.push_param(vb.GammaParam('tau'))
par.push_param(vb.UVNParamVector('u', length=G))
fun = vb.LogisticGLMMObjective(par, x, y, gid, G, gh_deg=20, weights=w)
fun._push_state()
pt = (beta, v, u[:, 0], np.full(G, np.exp(-3.0)), fun.gh_x, fun.gh_w)
A1 = rng.normal(size=(Q, 2 * P + 2 * G))
ctx = fun.ctx
r0, g0 = run('intercept class:', lambda: ctx.glmm_terms(*pt, want_grad=False, want_hess=False)[0],
             lambda: ctx.glmm_obs_influence(*pt, A1), lambda: ctx.glmm_group_influence(*pt, A1))
del fun, ctx
for K in (1, KS):
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    fun = vb.LogisticGLMMSlopesObjective(par, x, y, zs[:, :K], gid, G, gh_deg=20, weights=w)         # the constructor puts the weights on the device
    pt = (beta, v, u[:, :K], np.full((G, K), np.exp(-3.0)), fun.gh_x, fun.gh_w)
    A = A1 if K == 1 else rng.normal(size=(Q, 2 * P + 2 * G * K))
    ctx = fun.ctx
    r, g = run('slopes class, K = %d:' % K, lambda: ctx.glmm_slopes_terms(*pt, want_grad=False, want_hess=False)[0],
               lambda: ctx.glmm_slopes_obs_influence(*pt, A), lambda: ctx.glmm_slopes_group_influence(*pt, A))
    if K == 1:
        print('K = 1 against the intercept class: rows %.2e, groups %.2e (max abs difference)'
              % (np.abs(r - r0).max(), np.abs(g - g0).max()), flush=True)
    del fun, ctx

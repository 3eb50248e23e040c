"""Times the streamed weight influence of the logistic mixed model at N rows, P coefficients, G groups,
Q outputs: the value-only `lrvb_glmm_terms` call (the yardstick pass), the row entry over all N and the group entry.  Wall times
include the host copies (the N x Q result is 128 MB at the default shape); run under `rocprofv3 --kernel-trace --stats` for the
kernel durations."""
import sys, os, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import lrvb_amd as vb
N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1000000
P = int(sys.argv[2]) if len(sys.argv) > 2 else 64
G = int(float(sys.argv[3])) if len(sys.argv) > 3 else 10000
Q = int(sys.argv[4]) if len(sys.argv) > 4 else 16
rng = np.random.default_rng(1)
x = rng.standard_normal((N, P)) / np.sqrt(P)
gid = rng.integers(0, G, size=N).astype(np.int32)
u, beta = rng.normal(size=G) * 0.7, rng.normal(size=P) * 0.8
y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + u[gid])))).astype(np.float64)
par = vb.ModelParamsDict('params')
par.push_param(vb.UVNParamVector('beta', length=P))
par.push_param(vb.UVNParam('mu'))
par.push_param(vb.GammaParam('tau'))
par.push_param(vb.UVNParamVector('u', length=G))
fun = vb.LogisticGLMMObjective(par, x, y, gid, G, gh_deg=20, weights=rng.uniform(0.5, 1.5, size=N))
fun._push_state()
pt = (beta, np.full(P, np.exp(-6.0)), u, np.full(G, np.exp(-3.0)), fun.gh_x, fun.gh_w)
A = rng.normal(size=(Q, 2 * P + 2 * G))
ctx = fun.ctx
for rep in range(4):
    t0 = time.perf_counter(); val = ctx.glmm_terms(*pt, want_grad=False, want_hess=False)[0]; t1 = time.perf_counter()
    rows = ctx.glmm_obs_influence(*pt, A); t2 = time.perf_counter()
    grp = ctx.glmm_group_influence(*pt, A); t3 = time.perf_counter()
    print('N = %d, P = %d, G = %d, Q = %d: value-only terms %.2f ms, rows (N x Q to the host) %.2f ms, group influence %.2f ms'
          % (N, P, G, Q, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), flush=True)
print('value %.6e, |rows| %.3e, |groups| %.3e' % (val, np.abs(rows).max(), np.abs(grp).max()))

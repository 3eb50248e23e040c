"""Times the Poisson mixed model next to the logistic slopes class, in one process, at N rows, P
coefficients, G groups, Q outputs: for K = 1 and K = 4, first `LogisticGLMMSlopesObjective` (the yardstick), then
`PoissonGLMMObjective` on the same x, z and groups -- the value-only terms call (the rows pass), the influence row entry over all N,
the group entry, four times each, and H^-1 R with Q columns on the device-resident factors, fresh (the factors are built) and cached.
Wall times include the host copies (the N x Q result is 128 MB at the default shape); run under `rocprofv3 --kernel-trace --stats`
for the kernel durations.

    python tools/time_glmm_poisson.py [N [P [G [Q]]]]
"""
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
zs = np.concatenate([np.ones((N, 1)), 0.5 * rng.standard_normal((N, KS - 1))], axis=1)
gid = rng.integers(0, G, size=N).astype(np.int32)
u, beta = rng.normal(size=(G, KS)) * 0.5, rng.normal(size=P) * 0.5
off = np.log(rng.uniform(0.5, 2.0, size=N))
w = rng.uniform(0.5, 1.5, size=N)
v = np.full(P, np.exp(-6.0))


def run(label, fun, terms, rows, groups, free):
    for rep in range(4):
        t0 = time.perf_counter(); val = terms(); t1 = time.perf_counter()
        r = rows(); t2 = time.perf_counter()
        g = groups(); t3 = time.perf_counter()
        print('%s N = %d, P = %d, G = %d, Q = %d: value-only terms %.2f ms, rows (N x Q to the host) %.2f ms, group influence %.2f ms'
              % (label, N, P, G, Q, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), flush=True)
    print('%s value %.6e, |rows| %.3e, |groups| %.3e' % (label, val, np.abs(r).max(), np.abs(g).max()), flush=True)
    rhs = np.random.default_rng(2).normal(size=(free.size, Q))
    try:
        t0 = time.perf_counter(); s0 = fun.solve(free, rhs, on_device=True); t1 = time.perf_counter()
        s1 = fun.solve(free, rhs, on_device=True); t2 = time.perf_counter()
        print('%s solve on the device, %d columns: fresh %.1f ms, cached %.1f ms (equal: %s)'
              % (label, Q, (t1 - t0) * 1e3, (t2 - t1) * 1e3, np.array_equal(s0, s1)), flush=True)
    except np.linalg.LinAlgError as err:
        print('%s solve on the device: the Hessian is not positive definite at this point (%s)' % (label, err), flush=True)


for K in (1, KS):
    z = zs[:, :K]
    lin = x @ beta + (z * u[gid, :K]).sum(1)
    free = np.concatenate([beta, np.full(P, 6.0), np.zeros(K), np.full(K, 3.0), np.tile([np.log(G / 2.0), np.log(G / 4.0)], K),
                           u[:, :K].ravel(), np.full(G * K, 3.0)])
    pt = (beta, v, u[:, :K], np.full((G, K), np.exp(-3.0)))
    A = rng.normal(size=(Q, 2 * P + 2 * G * K))
    for family in ('logistic', 'poisson'):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        if family == 'logistic':
            y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-lin))).astype(np.float64)
            fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, gh_deg=20, weights=w)
            ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
            run('logistic, K = %d:' % K, fun, lambda: ctx.glmm_slopes_terms(*pt, *gh, want_grad=False, want_hess=False)[0],
                lambda: ctx.glmm_slopes_obs_influence(*pt, *gh, A), lambda: ctx.glmm_slopes_group_influence(*pt, *gh, A), free)
        else:
            y = rng.poisson(np.exp(off + lin)).astype(np.float64)
            fun = vb.PoissonGLMMObjective(par, x, y, z, gid, G, offset=off, weights=w)
            ctx = fun.ctx
            run('poisson,  K = %d:' % K, fun, lambda: ctx.glmm_poisson_terms(*pt, want_grad=False, want_hess=False)[0],
                lambda: ctx.glmm_poisson_obs_influence(*pt, A), lambda: ctx.glmm_poisson_group_influence(*pt, A), free)
        del fun, ctx

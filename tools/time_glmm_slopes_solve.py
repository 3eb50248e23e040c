"""Times `LogisticGLMMSlopesObjective.solve(theta, R)` at N rows, P coefficients, K effects, G groups for
Q = 1 and Q = 16 right-hand sides with non-zero local rows: wall time at a FRESH point (terms, elimination, factor, solve) and at
a CACHED point (the solve alone), three repetitions each, the first of them after one untimed warm-up solve.

    python tools/time_glmm_slopes_solve.py [N P K G] [--host]

Default: the device-resident route `on_device=True`; `--host`: the host route `block_arrow_solve` (the only one before section 21,
so the script also runs on a checkout that lacks the keyword).  Run under `rocprofv3 --kernel-trace --stats` with `--once` for the
kernel durations of one fresh device solve at Q = 16."""
import os
import sys
import time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import lrvb_amd as vb
flags = [a for a in sys.argv[1:] if a.startswith('--')]
nums = [a for a in sys.argv[1:] if not a.startswith('--')]
N, P, K, G = (int(float(a)) for a in (nums + ['1e6', '64', '4', '1e4'][len(nums):]))
host, once = '--host' in flags, '--once' in flags
rng = np.random.default_rng(1)
x = rng.standard_normal((N, P)) / np.sqrt(P)
z = np.concatenate([np.ones((N, 1)), rng.standard_normal((N, K - 1))], axis=1)
gid = rng.integers(0, G, size=N).astype(np.int32)
u, beta = rng.normal(size=(G, K)) * 0.7, rng.normal(size=P) * 0.8
y = (rng.uniform(size=N) < 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid]).sum(1))))).astype(np.float64)
free = np.concatenate([beta, np.full(P, 6.0), np.zeros(K), np.full(K, 3.0), np.tile([np.log(G / 2.0), np.log(G / 4.0)], K),
                       u.ravel(), np.full(G * K, 3.0)])
par = vb.ModelParamsDict('params')
par.push_param(vb.UVNParamVector('beta', length=P))
par.push_param(vb.UVNParamVector('mu', length=K))
for k in range(K):
    par.push_param(vb.GammaParam('tau%d' % k))
par.push_param(vb.UVNParamArray('u', shape=(G, K)))
fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G)
solve = (lambda th, rhs: fun.solve(th, rhs)) if host else (lambda th, rhs: fun.solve(th, rhs, on_device=True))
label = 'host route' if host else 'device route'
D = free.size
step = 0
for Q in ((16,) if once else (1, 16)):
    rhs = rng.normal(size=D) if Q == 1 else rng.normal(size=(D, Q))
    if not once:
        solve(free, rhs)                                                  # warm-up: allocations, first launches
    for rep in range(1 if once else 3):
        step += 1
        th = free.copy()
        th[0] += 1e-6 * step                                              # a point nobody has seen
        t0 = time.perf_counter(); X = solve(th, rhs); t1 = time.perf_counter()
        X2 = solve(th, rhs); t2 = time.perf_counter()
        print('%s N = %d, P = %d, K = %d, G = %d, Q = %d: fresh point %.1f ms, cached point %.1f ms'
              % (label, N, P, K, G, Q, (t1 - t0) * 1e3, (t2 - t1) * 1e3), flush=True)
    if not once:                                                          # the residual of column 0 by the host arrow product
        x0, r0 = (X[:, 0], rhs[:, 0]) if Q > 1 else (X, rhs)
        print('%s Q = %d: |H x - r| / |r| = %.2e' % (label, Q, np.linalg.norm(fun.hvp(th, x0) - r0) / np.linalg.norm(r0)), flush=True)

"""Times the host block-arrow algebra of the logistic mixed models on random symmetric positive definite
pieces: best-of-5 wall times of the Schur term, the solve with Q right-hand sides and the product, for `glmm_slopes.block_arrow_*`
at any K and, at K = 1, for the intercept's `glmm.arrow_*` on the same pieces.  No GPU is used.

    python tools/time_block_arrow_host.py P G K Q          (default 64 10000 1 16; pin OMP_NUM_THREADS for comparable figures)
"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lrvb_amd import glmm, glmm_slopes as gs

P = int(sys.argv[1]) if len(sys.argv) > 1 else 64
G = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10000
K = int(sys.argv[3]) if len(sys.argv) > 3 else 1
Q = int(sys.argv[4]) if len(sys.argv) > 4 else 16


def pieces(P, G, K, seed=0):
    """Hgg, the 2 P + 3 K coupled rows, Hx (R x 2 G K) and loc (G x 2 K x 2 K) with correlations of magnitude at most 0.8."""
    rng = np.random.default_rng(seed)
    n, ng = 2 * K, 2 * P + 4 * K
    rows = gs.coupled_rows(P, K)
    Hx = rng.normal(size=(rows.size, 2 * G * K)) * 0.3
    d = np.sqrt(rng.uniform(1.0, 2.0, size=(G, n)))
    s = rng.choice([-1.0, 1.0], size=(G, n))
    rho = rng.uniform(-0.8 / (n - 1), 0.8, size=G)                        # I + rho (s s^T - I) is positive definite
    C = rho[:, None, None] * s[:, :, None] * s[:, None, :]
    C[:, np.arange(n), np.arange(n)] = 1.0
    loc = C * d[:, :, None] * d[:, None, :]
    Z = rng.normal(size=(ng, ng))
    Hgg = Z @ Z.T / ng + np.eye(ng)
    Hgg[np.ix_(rows, rows)] += gs.block_arrow_schur_term(rows, Hx, loc)   # the Schur complement is Z Z^T / ng + I
    return Hgg, rows, Hx, loc


def best(f, reps=5):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t)


Hgg, rows, Hx, loc = pieces(P, G, K)
rng = np.random.default_rng(1)
Rhs, v = rng.normal(size=(Hgg.shape[0] + 2 * G * K, Q)), rng.normal(size=Hgg.shape[0] + 2 * G * K)
routes = [('block_arrow', gs.block_arrow_schur_term, gs.block_arrow_solve, gs.block_arrow_matvec, loc)]
if K == 1:
    routes.append(('arrow', glmm.arrow_schur_term, glmm.arrow_solve, glmm.arrow_matvec,
                   np.stack([loc[:, 0, 0], loc[:, 0, 1], loc[:, 1, 1]], axis=1)))
out = {}
for name, schur, solve, matvec, L in routes:
    out[name] = solve(Hgg, rows, Hx, L, Rhs)
    print('P = %d, G = %d, K = %d, Q = %d: %s_schur_term %.4f s, %s_solve %.4f s, %s_matvec %.5f s'
          % (P, G, K, Q, name, best(lambda: schur(rows, Hx, L)), name, best(lambda: solve(Hgg, rows, Hx, L, Rhs)),
             name, best(lambda: matvec(Hgg, rows, Hx, L, v))), flush=True)
res = np.max(np.abs(np.column_stack([gs.block_arrow_matvec(Hgg, rows, Hx, loc, x) for x in out['block_arrow'].T]) - Rhs))
print('residual of the solve %.2e' % res + ('' if K != 1 else ', the two routes differ by %.2e relative'
                                           % (np.max(np.abs(out['arrow'] - out['block_arrow'])) / np.max(np.abs(out['arrow'])))))

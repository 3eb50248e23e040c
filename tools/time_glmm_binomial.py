"""Times the three binomial kernels next to the logistic instantiations of the same tile walk, in ONE
process: for K = 1 and K = 4, first `LogisticGLMMSlopesObjective` (the yardstick: the parent's code, unchanged), then
`BinomialGLMMObjective` with trials and an offset on the same x, z, groups and point -- the value-only terms call (the rows pass),
the influence row entry over all N and the group entry, REPS times each.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_binomial.py [N [P [G [Q]]]]

for the kernel durations, then

    python tools/time_glmm_binomial.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel and K (calls, median, min, max in ns) and, per binomial kernel, the verdict of section 27's
criterion: is its median within the logistic median plus that yardstick's own max - min over its dispatches in the same run?
Every kernel is dispatched REPS times at K = 1 and then REPS times at K = 4, which is how the trace is split.
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
KERNELS = (('rows', 'glmm_slopes_rows_kernel', 'LogisticLik', 'BinomialLik'),
           ('influence rows', 'glmm_slopes_infl_rows_kernel', None, 'glmm_binomial_infl_rows_kernel'),
           ('group sums', 'glmm_slopes_infl_gsum_kernel', 'LogisticLik', 'BinomialLik'))


def summarize(trace, out):
    with open(trace, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = {}
    for r in rows:
        dur.setdefault(r['Kernel_Name'], []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))

    def pick(base, policy, other=None):
        """The dispatches of the instantiation: a templated kernel by its policy, an own entry by its name."""
        hits = [k for k in dur if (other in k if other else (base in k and (policy is None or policy in k)))]
        assert len(hits) == 1, (base, policy, other, hits)
        d = dur[hits[0]]
        assert len(d) == 2 * REPS, (hits[0], len(d))
        return d[:REPS], d[REPS:]

    lines = [('kernel', 'likelihood', 'K', 'calls', 'median_ns', 'min_ns', 'max_ns', 'spread_ns', 'binomial_minus_logistic_ns', 'verdict')]
    for label, base, lpol, bpol in KERNELS:
        lo = pick(base, lpol)
        bi = pick(base, bpol) if lpol else pick(base, None, other=bpol)
        for i, K in enumerate((1, 4)):
            lm, bm = float(np.median(lo[i])), float(np.median(bi[i]))
            spread = max(lo[i]) - min(lo[i])
            lines.append((label, 'logistic', K, len(lo[i]), lm, min(lo[i]), max(lo[i]), spread, '', ''))
            lines.append((label, 'binomial', K, len(bi[i]), bm, min(bi[i]), max(bi[i]), max(bi[i]) - min(bi[i]), bm - lm,
                          'within the spread' if bm - lm <= spread else 'slower: %.2f %%' % (100.0 * (bm - lm) / lm)))
    with open(out, 'w', newline='') as f:
        csv.writer(f).writerows(lines)
    for l in lines:
        print(','.join(str(v) for v in l))


if len(sys.argv) > 1 and sys.argv[1] == '--summarize':
    summarize(sys.argv[2], sys.argv[3])
    sys.exit(0)

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
off = 0.3 * rng.standard_normal(N)
trials = rng.integers(1, 13, size=N).astype(np.float64)
w = rng.uniform(0.5, 1.5, size=N)
v = np.full(P, np.exp(-6.0))


def run(label, terms, rows, groups):
    for rep in range(REPS):
        t0 = time.perf_counter(); val = terms(); t1 = time.perf_counter()
        r = rows(); t2 = time.perf_counter()
        g = groups(); t3 = time.perf_counter()
        print('%s N = %d, P = %d, G = %d, Q = %d: value-only terms %.2f ms, rows (N x Q to the host) %.2f ms, group influence %.2f ms'
              % (label, N, P, G, Q, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3), flush=True)
    print('%s value %.6e, |rows| %.3e, |groups| %.3e' % (label, val, np.abs(r).max(), np.abs(g).max()), flush=True)


for K in (1, KS):
    z = zs[:, :K]
    pr = 1.0 / (1.0 + np.exp(-(off + x @ beta + (z * u[gid, :K]).sum(1))))
    pt = (beta, v, u[:, :K], np.full((G, K), np.exp(-3.0)))
    A = rng.normal(size=(Q, 2 * P + 2 * G * K))
    for family in ('logistic', 'binomial'):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        if family == 'logistic':
            y = (rng.uniform(size=N) < pr).astype(np.float64)
            fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, gh_deg=20, weights=w)
            ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
            run('logistic, K = %d:' % K, lambda: ctx.glmm_slopes_terms(*pt, *gh, want_grad=False, want_hess=False)[0],
                lambda: ctx.glmm_slopes_obs_influence(*pt, *gh, A), lambda: ctx.glmm_slopes_group_influence(*pt, *gh, A))
        else:
            y = rng.binomial(trials.astype(np.int64), pr).astype(np.float64)
            fun = vb.BinomialGLMMObjective(par, x, y, z, gid, G, trials=trials, offset=off, gh_deg=20, weights=w)
            ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
            run('binomial, K = %d:' % K, lambda: ctx.glmm_binomial_terms(*pt, *gh, want_grad=False, want_hess=False)[0],
                lambda: ctx.glmm_binomial_obs_influence(*pt, *gh, A), lambda: ctx.glmm_binomial_group_influence(*pt, *gh, A))
        del fun, ctx

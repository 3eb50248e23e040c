"""Times the walks of the Gamma mixed model next to the Poisson instantiations of the same tile walk -- the
yardstick: the other likelihood whose expectation is closed form -- in ONE process, at K = 1 and then at K = 4:
`PoissonGLMMObjective` and `GammaGLMMObjective` on the same x, z, groups, offset and point: the value-only terms call (the rows pass),
the influence row entry over all N and the group entry, and for the Gamma model its dispersion rows pass, REPS times each.  The
Gamma model has no predict kernel of its own (its fitted mean is the Poisson one), so none is timed.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_gamma.py [N [P [G [Q]]]]

for the kernel durations (no counters in that run), then

    python tools/time_glmm_gamma.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel, K and family: calls, median, min, max in ns, the spread (max - min over the timed dispatches of
the same run) and the ratio of the median to the Poisson median.  Reported as measured; none of it is a pass threshold.  Every
kernel is dispatched equally often at either K (K is an argument, not a template parameter), so the first REPS dispatches of the
first half of a kernel's trace are the K = 1 ones and the first REPS of the second half the K = 4 ones.
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
KS = (1, 4)
FAMILIES = ('poisson', 'gamma')
# kernel label -> per family, the substrings that pick its dispatches out of the trace (spaces removed from the names)
KERNELS = (('rows', {'poisson': ('glmm_slopes_rows_kernel', '<PoissonLik'), 'gamma': ('glmm_slopes_rows_kernel', '<GammaLik')}),
           ('influence rows', {'poisson': ('glmm_poisson_infl_rows_kernel',), 'gamma': ('glmm_gamma_infl_rows_kernel',)}),
           ('group sums', {'poisson': ('glmm_slopes_infl_gsum_kernel', '<PoissonLik'), 'gamma': ('glmm_slopes_infl_gsum_kernel', '<GammaLik')}),
           ('dispersion rows', {'gamma': ('glmm_disp_rows_kernel', 'GammaDispLik')}))


def summarize(trace, out):
    with open(trace, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = {}
    for r in rows:
        dur.setdefault(r['Kernel_Name'].replace(' ', ''), []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))

    def pick(keys, which):
        hits = [k for k in dur if all(s in k for s in keys)]
        assert len(hits) == 1, (keys, hits, sorted(k for k in dur if 'glmm' in k))
        d = dur[hits[0]]
        assert len(d) % len(KS) == 0 and len(d) >= len(KS) * REPS, (hits[0], len(d))
        start = which * (len(d) // len(KS))
        return d[start:start + REPS]

    lines = [('kernel', 'K', 'family', 'calls', 'median_ns', 'min_ns', 'max_ns', 'spread_ns', 'ratio_to_poisson')]
    for label, names in KERNELS:
        for which, K in enumerate(KS):
            parts = {fam: pick(names[fam], which) for fam in FAMILIES if fam in names}
            base = {fam: float(np.median(parts[fam])) for fam in parts}
            for fam in parts:
                d = parts[fam]
                lines.append((label, K, fam, len(d), base[fam], min(d), max(d), max(d) - min(d),
                              '%.3f' % (base[fam] / base['poisson']) if 'poisson' in base else ''))
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
rng = np.random.default_rng(1)
x = rng.standard_normal((N, P)) / np.sqrt(P)
gid = rng.integers(0, G, size=N).astype(np.int32)
beta = rng.normal(size=P) * 0.5
off = 0.3 * rng.standard_normal(N)
w = rng.uniform(0.5, 1.5, size=N)
v = np.full(P, np.exp(-6.0))
phi = np.exp(rng.uniform(np.log(0.5), np.log(50.0), size=N))


def timed(label, fn):
    out = None
    for rep in range(REPS):
        t0 = time.perf_counter(); out = fn(); t1 = time.perf_counter()
        print('%s: %.2f ms' % (label, (t1 - t0) * 1e3), flush=True)
    return out


for K in KS:
    z = np.concatenate([np.ones((N, 1)), 0.5 * rng.standard_normal((N, K - 1))], axis=1)
    u = rng.normal(size=(G, K)) * 0.5
    t = off + x @ beta + (z * u[gid]).sum(1)
    counts = rng.poisson(np.exp(t)).astype(np.float64)
    amounts = np.maximum(rng.gamma(phi, np.exp(t) / phi), 1e-300)
    pt = (beta, v, u, np.full((G, K), np.exp(-3.0)))
    A = rng.normal(size=(Q, 2 * P + 2 * G * K))
    for fam in FAMILIES:
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        if fam == 'poisson':
            fun = vb.PoissonGLMMObjective(par, x, counts, z, gid, G, offset=off, weights=w)
        else:
            fun = vb.GammaGLMMObjective(par, x, amounts, z, gid, G, phi, offset=off, weights=w)
        ctx, name = fun.ctx, 'glmm_' + fam
        tag = '%s, K = %d, N = %d, P = %d, G = %d' % (fam, K, N, P, G)
        val = timed('%s: value-only terms' % tag, lambda: getattr(ctx, name + '_terms')(*pt, want_grad=False, want_hess=False)[0])
        r = timed('%s: influence rows, Q = %d (N x Q to the host)' % (tag, Q), lambda: getattr(ctx, name + '_obs_influence')(*pt, A))
        g = timed('%s: group influence' % tag, lambda: getattr(ctx, name + '_group_influence')(*pt, A))
        print('%s: value %.6e, |rows| %.3e, |groups| %.3e' % (tag, val, np.abs(r).max(), np.abs(g).max()), flush=True)
        if fam == 'gamma':
            d = timed('%s: dispersion terms' % tag, lambda: ctx.glmm_gamma_dispersion_terms(*pt)[0])
            print('%s: d %.6e (the value again)' % (tag, d[0]), flush=True)
        del fun, ctx

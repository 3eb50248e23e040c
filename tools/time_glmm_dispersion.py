"""Times the log-dispersion pass of the Beta and the NB2 mixed model next to the rows kernel of the SAME
family -- the yardstick -- in ONE process, at K = 1 and then at K = 4: `BetaGLMMObjective` and `NegBinomialGLMMObjective` on the same
x, z, groups, offset and point: the value-only terms call (glmm_slopes_rows_kernel<BetaLik | BinomialLik>) and the dispersion entry
(glmm_disp_rows_kernel<BetaDispLik | NegBinDispLik>), REPS times each.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_dispersion.py [N [P [G]]]

for the kernel durations (no counters in that run), then

    python tools/time_glmm_dispersion.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel, K and family: calls, median, min, max in ns, the spread and the ratio of the median to the
family's rows kernel.  Reported as measured; none of it is a pass threshold.  Every kernel is dispatched equally often at either K
(K is an argument, not a template parameter), so the first REPS dispatches of the first half of a kernel's trace are the K = 1 ones
and the first REPS of the second half the K = 4 ones.
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
KS = (1, 4)
FAMILIES = ('beta', 'negbin')
# kernel label -> per family, the substrings that pick its dispatches out of the trace (spaces removed from the names)
KERNELS = (('rows', {'beta': ('glmm_slopes_rows_kernel', '<BetaLik'), 'negbin': ('glmm_slopes_rows_kernel', '<BinomialLik>')}),
           ('dispersion rows', {'beta': ('glmm_disp_rows_kernel', 'BetaDispLik'), 'negbin': ('glmm_disp_rows_kernel', 'NegBinDispLik')}))


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

    lines = [('kernel', 'K', 'family', 'calls', 'median_ns', 'min_ns', 'max_ns', 'spread_ns', 'ratio_to_family_rows')]
    for which, K in enumerate(KS):
        for fam in FAMILIES:
            base = float(np.median(pick(KERNELS[0][1][fam], which)))
            for label, names in KERNELS:
                d = pick(names[fam], which)
                lines.append((label, K, fam, len(d), float(np.median(d)), min(d), max(d), max(d) - min(d), '%.3f' % (float(np.median(d)) / base)))
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
    mu = 1.0 / (1.0 + np.exp(-t))
    counts = rng.negative_binomial(phi, phi / (phi + np.exp(t))).astype(np.float64)
    prop = np.clip(rng.beta(mu * phi, (1.0 - mu) * phi), 1e-12, 1.0 - 1e-12)
    pt = (beta, v, u, np.full((G, K), np.exp(-3.0)))
    for fam in FAMILIES:
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        if fam == 'beta':
            fun = vb.BetaGLMMObjective(par, x, prop, z, gid, G, phi, offset=off, gh_deg=20, weights=w)
            terms, disp = fun.ctx.glmm_beta_terms, fun.ctx.glmm_beta_dispersion_terms
        else:
            fun = vb.NegBinomialGLMMObjective(par, x, counts, z, gid, G, phi, offset=off, gh_deg=20, weights=w)
            terms, disp = fun.ctx.glmm_binomial_terms, fun.ctx.glmm_negbin_dispersion_terms
        head = pt + (fun.gh_x, fun.gh_w)
        tag = '%s, K = %d, N = %d, P = %d, G = %d' % (fam, K, N, P, G)
        val = timed('%s: value-only terms' % tag, lambda: terms(*head, want_grad=False, want_hess=False)[0])
        d, cg, cl = timed('%s: dispersion terms' % tag, lambda: disp(*head))
        print('%s: value %.6e, d %s, |cross global| %.3e, |cross local| %.3e' % (tag, val, d, np.abs(cg).max(), np.abs(cl).max()), flush=True)
        del fun

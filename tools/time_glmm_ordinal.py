"""Times the walks of the ordinal mixed model next to three yardsticks in ONE process, at K = 1 and then at
K = 4, on the same x, z, groups, offset and point:

    logit    `BinomialGLMMObjective(link='logit')`: ONE logistic node function per node;
    probit   `BinomialGLMMObjective(link='probit')`: two node functions per node (success and failure), as the ordinal policy has
             (t - hi and lo - t);
    beta     `BetaGLMMObjective`: its dispersion rows pass is the yardstick of the threshold pass (same head, one scalar per row);
    ordinal  `OrdinalGLMMObjective` at J = 5 and J = 16 categories.

Per model: the value-only terms call (the rows pass), the influence row entry over all N, the group entry and, where the model has
one, the dispersion or threshold pass, REPS times each.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_ordinal.py [N [P [G [Q]]]]

for the kernel durations (no counters in that run), then

    python tools/time_glmm_ordinal.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel, K and variant: calls, median, min, max in ns, the spread (max - min over the timed dispatches of the
same run) and the ratios of the median to the logit and to the probit median (the threshold pass: to the Beta dispersion pass).
Reported as measured; none of it is a pass threshold.  A kernel is dispatched equally often for every (K, variant) it serves, in the
order of the loops below, so its trace splits into equal consecutive parts.
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
KS = (1, 4)
JS = (5, 16)
VARIANTS = (('logit', None), ('probit', None), ('beta', None)) + tuple(('ordinal', J) for J in JS)
# kernel label -> per family, the substrings that pick its dispatches out of the trace (spaces removed from the names)
KERNELS = (('rows', {'logit': ('glmm_slopes_rows_kernel', '<BinomialLik'), 'probit': ('glmm_slopes_rows_kernel', 'BinomialLinkLik<1'),
                     'ordinal': ('glmm_slopes_rows_kernel', '<OrdinalLik')}),
           ('influence rows', {'logit': ('glmm_binomial_infl_rows_kernel',), 'probit': ('glmm_link_infl_rows_kernel<1',),
                               'ordinal': ('glmm_ordinal_infl_rows_kernel',)}),
           ('group sums', {'logit': ('glmm_slopes_infl_gsum_kernel', '<BinomialLik'), 'probit': ('glmm_slopes_infl_gsum_kernel', 'BinomialLinkLik<1'),
                           'ordinal': ('glmm_slopes_infl_gsum_kernel', '<OrdinalLik')}),
           ('hyper rows', {'beta': ('glmm_disp_rows_kernel', 'BetaDispLik'), 'ordinal': ('glmm_thr_rows_kernel',)}))


def summarize(trace, out):
    with open(trace, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = {}
    for r in rows:
        dur.setdefault(r['Kernel_Name'].replace(' ', ''), []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))

    def pick(keys, part, parts):
        hits = [k for k in dur if all(s in k for s in keys)]
        assert len(hits) == 1, (keys, hits, sorted(k for k in dur if 'glmm' in k))
        d = dur[hits[0]]
        assert len(d) % parts == 0 and len(d) >= parts * REPS, (hits[0], len(d), parts)
        start = part * (len(d) // parts)
        return d[start:start + REPS]

    lines = [('kernel', 'K', 'variant', 'calls', 'median_ns', 'min_ns', 'max_ns', 'spread_ns', 'ratio_to_logit', 'ratio_to_probit', 'ratio_to_beta')]
    for label, names in KERNELS:
        for ik, K in enumerate(KS):
            got = {}
            for fam, J in VARIANTS:
                if fam not in names:
                    continue
                nv = len(JS) if fam == 'ordinal' else 1
                iv = JS.index(J) if fam == 'ordinal' else 0
                got[(fam, J)] = pick(names[fam], ik * nv + iv, len(KS) * nv)
            med = {k: float(np.median(d)) for k, d in got.items()}
            ratio = lambda k, base: '%.3f' % (med[k] / med[(base, None)]) if (base, None) in med else ''
            for (fam, J), d in got.items():
                lines.append((label, K, fam if J is None else '%s J %d' % (fam, J), len(d), med[(fam, J)], min(d), max(d), max(d) - min(d),
                              ratio((fam, J), 'logit'), ratio((fam, J), 'probit'), ratio((fam, J), 'beta')))
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
    lat = t + rng.logistic(size=N)
    pr = 1.0 / (1.0 + np.exp(-t))
    pt = (beta, v, u, np.full((G, K), np.exp(-3.0)))
    A = rng.normal(size=(Q, 2 * P + 2 * G * K))
    for fam, J in VARIANTS:
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        hyper = None
        if fam in ('logit', 'probit'):
            fun = vb.BinomialGLMMObjective(par, x, (lat > 0.0).astype(np.float64), z, gid, G, offset=off, weights=w, link=fam)
            name = 'glmm_binomial'
        elif fam == 'beta':
            yb = np.clip(rng.beta(pr * phi, (1.0 - pr) * phi), 1e-12, 1.0 - 1e-12)
            fun = vb.BetaGLMMObjective(par, x, yb, z, gid, G, phi, offset=off, weights=w)
            name, hyper = 'glmm_beta', 'glmm_beta_dispersion_terms'
        else:
            alpha = np.quantile(lat, np.arange(1, J) / J)
            fun = vb.OrdinalGLMMObjective(par, x, np.searchsorted(alpha, lat), z, gid, G, alpha, offset=off, weights=w)
            name, hyper = 'glmm_ordinal', 'glmm_ordinal_threshold_terms'
        nodes = (fun.gh_x, fun.gh_w)
        ctx = fun.ctx
        tag = '%s%s, K = %d, N = %d, P = %d, G = %d' % (fam, '' if J is None else ' J %d' % J, K, N, P, G)
        val = timed('%s: value-only terms' % tag, lambda: getattr(ctx, name + '_terms')(*pt, *nodes, want_grad=False, want_hess=False)[0])
        r = timed('%s: influence rows, Q = %d (N x Q to the host)' % (tag, Q), lambda: getattr(ctx, name + '_obs_influence')(*pt, *nodes, A))
        g = timed('%s: group influence' % tag, lambda: getattr(ctx, name + '_group_influence')(*pt, *nodes, A))
        print('%s: value %.6e, |rows| %.3e, |groups| %.3e' % (tag, val, np.abs(r).max(), np.abs(g).max()), flush=True)
        if hyper:
            d = timed('%s: %s' % (tag, hyper), lambda: getattr(ctx, hyper)(*pt, *nodes)[0])
            print('%s: first hyper derivatives %s' % (tag, np.asarray(d)[:2]), flush=True)
        del fun, ctx

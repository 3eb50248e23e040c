"""Times the walks of the censored Gaussian mixed model next to two yardsticks in ONE process, at K = 1 and then
at K = 4, on the same x, z, groups, offset and point:

    probit      `BinomialGLMMObjective(link='probit')`: the policy whose h1 the censored rows call -- it evaluates h1 twice per node
                (success and failure), a censored row once;
    gamma       `GammaGLMMObjective`: the other policy with a precision and a closed-form row, the yardstick of the observed rows;
    censnormal  `CensoredNormalGLMMObjective` at the censoring shares 0, 0.3 and 1 (left and right alternating).

Per model: the value-only terms call (the rows pass), the influence row entry over all N, the group entry and, where the model has
one, the dispersion rows pass, REPS times each.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_censnormal.py [N [P [G [Q]]]]

for the kernel durations (no counters in that run), then

    python tools/time_glmm_censnormal.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel, K and variant: calls, median, min, max in ns, the spread (max - min over the timed dispatches of the
same run) and the ratios of the median to the probit and to the Gamma median.  Reported as measured; none of it is a pass threshold.
A kernel is dispatched equally often for every (K, variant) it serves, in the order of the loops below, so its trace splits into equal
consecutive parts.
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
KS = (1, 4)
SHARES = (0.0, 0.3, 1.0)
VARIANTS = (('probit', None), ('gamma', None)) + tuple(('censnormal', s) for s in SHARES)
# kernel label -> per family, the substrings that pick its dispatches out of the trace (spaces removed from the names)
KERNELS = (('rows', {'probit': ('glmm_slopes_rows_kernel', 'BinomialLinkLik<1'), 'gamma': ('glmm_slopes_rows_kernel', '<GammaLik'),
                     'censnormal': ('glmm_slopes_rows_kernel', '<CensNormalLik')}),
           ('influence rows', {'probit': ('glmm_link_infl_rows_kernel<1',), 'gamma': ('glmm_gamma_infl_rows_kernel',),
                               'censnormal': ('glmm_censnormal_infl_rows_kernel',)}),
           ('group sums', {'probit': ('glmm_slopes_infl_gsum_kernel', 'BinomialLinkLik<1'), 'gamma': ('glmm_slopes_infl_gsum_kernel', '<GammaLik'),
                           'censnormal': ('glmm_slopes_infl_gsum_kernel', '<CensNormalLik')}),
           ('dispersion rows', {'gamma': ('glmm_disp_rows_kernel', 'GammaDispLik'), 'censnormal': ('glmm_disp_rows_kernel', 'CensNormalDispLik')}))


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

    lines = [('kernel', 'K', 'variant', 'calls', 'median_ns', 'min_ns', 'max_ns', 'spread_ns', 'ratio_to_probit', 'ratio_to_gamma')]
    for label, names in KERNELS:
        for ik, K in enumerate(KS):
            got = {}
            for fam, share in VARIANTS:
                if fam not in names:
                    continue
                nv = len(SHARES) if fam == 'censnormal' else 1
                iv = SHARES.index(share) if fam == 'censnormal' else 0
                got[(fam, share)] = pick(names[fam], ik * nv + iv, len(KS) * nv)
            med = {k: float(np.median(d)) for k, d in got.items()}
            for (fam, share), d in got.items():
                lines.append((label, K, fam if share is None else '%s share %g' % (fam, share), len(d), med[(fam, share)], min(d), max(d), max(d) - min(d),
                              '%.3f' % (med[(fam, share)] / med[('probit', None)]) if ('probit', None) in med else '',
                              '%.3f' % (med[(fam, share)] / med[('gamma', None)]) if ('gamma', None) in med else ''))
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
    ystar = t + rng.standard_normal(N) / np.sqrt(phi)
    amounts = np.maximum(rng.gamma(phi, np.exp(t) / phi), 1e-300)
    side = np.where(np.arange(N) % 2 == 0, 1, -1)
    draw = rng.uniform(size=N)
    gap = rng.uniform(0.0, 1.5, size=N) / np.sqrt(phi)
    pt = (beta, v, u, np.full((G, K), np.exp(-3.0)))
    A = rng.normal(size=(Q, 2 * P + 2 * G * K))
    for fam, share in VARIANTS:
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        nodes, disp = (), None
        if fam == 'probit':
            fun = vb.BinomialGLMMObjective(par, x, (ystar > t).astype(np.float64), z, gid, G, offset=off, weights=w, link='probit')
            name, nodes = 'glmm_binomial', (fun.gh_x, fun.gh_w)
        elif fam == 'gamma':
            fun = vb.GammaGLMMObjective(par, x, amounts, z, gid, G, phi, offset=off, weights=w)
            name, disp = 'glmm_gamma', 'glmm_gamma_dispersion_terms'
        else:
            st = np.where(draw < share, side, 0).astype(np.int32)
            fun = vb.CensoredNormalGLMMObjective(par, x, ystar - st * gap, z, gid, G, phi, censoring=st, offset=off, weights=w)
            name, nodes, disp = 'glmm_censnormal', (fun.gh_x, fun.gh_w), 'glmm_censnormal_dispersion_terms'
        ctx = fun.ctx
        tag = '%s%s, K = %d, N = %d, P = %d, G = %d' % (fam, '' if share is None else ' share %g' % share, K, N, P, G)
        val = timed('%s: value-only terms' % tag, lambda: getattr(ctx, name + '_terms')(*pt, *nodes, want_grad=False, want_hess=False)[0])
        r = timed('%s: influence rows, Q = %d (N x Q to the host)' % (tag, Q), lambda: getattr(ctx, name + '_obs_influence')(*pt, *nodes, A))
        g = timed('%s: group influence' % tag, lambda: getattr(ctx, name + '_group_influence')(*pt, *nodes, A))
        print('%s: value %.6e, |rows| %.3e, |groups| %.3e' % (tag, val, np.abs(r).max(), np.abs(g).max()), flush=True)
        if disp:
            d = timed('%s: dispersion terms' % tag, lambda: getattr(ctx, disp)(*pt, *nodes)[0])
            print('%s: d %.6e %.6e' % (tag, d[0], d[1]), flush=True)
        del fun, ctx

"""Times the kernels of the probit and the cloglog link next to the logit `BinomialLik` instantiations of the
same tile walk -- the yardstick -- in ONE process: for K = 1 and K = 4, `BinomialGLMMObjective` with trials and an offset under
link = 'logit', 'probit', 'cloglog' on the same x, z, groups and point: the value-only terms call (the rows pass), the influence
row entry over all N, the group entry and `predict` over all N on the device, REPS times each.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_link.py [N [P [G [Q]]]]

for the kernel durations (no counters in that run), then

    python tools/time_glmm_link.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel, link and K: calls, median, min, max in ns, the ratio of the median to the logit median and the
yardstick's own spread (max - min over its dispatches in the same run).  Reported as measured; none of it is a pass threshold.
Every kernel is dispatched REPS times at K = 1 and then REPS times at K = 4 ahead of anything else that launches it (the first
`predict` forms the terms and the factor once more), which is how the trace is split.
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
LINKS = ('logit', 'probit', 'cloglog')
# kernel label -> per link, the substrings that pick its dispatches out of the trace
KERNELS = (('rows', {'logit': ('glmm_slopes_rows_kernel', 'BinomialLik'), 'probit': ('glmm_slopes_rows_kernel', 'BinomialLinkLik<1'),
                     'cloglog': ('glmm_slopes_rows_kernel', 'BinomialLinkLik<2')}),
           ('influence rows', {'logit': ('glmm_binomial_infl_rows_kernel',), 'probit': ('glmm_link_infl_rows_kernel<1',),
                               'cloglog': ('glmm_link_infl_rows_kernel<2',)}),
           ('group sums', {'logit': ('glmm_slopes_infl_gsum_kernel', 'BinomialLik'), 'probit': ('glmm_slopes_infl_gsum_kernel', 'BinomialLinkLik<1'),
                           'cloglog': ('glmm_slopes_infl_gsum_kernel', 'BinomialLinkLik<2')}),
           ('predict', {'logit': ('glmm_binomial_predict_rows_kernel',), 'probit': ('glmm_link_predict_rows_kernel<1',),
                        'cloglog': ('glmm_link_predict_rows_kernel<2',)}))


def summarize(trace, out):
    with open(trace, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = {}
    for r in rows:
        dur.setdefault(r['Kernel_Name'].replace(' ', ''), []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))

    def pick(keys):
        hits = [k for k in dur if all(s in k for s in keys)]
        assert len(hits) == 1, (keys, hits, sorted(k for k in dur if 'glmm' in k))
        d = dur[hits[0]]
        half = len(d) // 2                                               # K = 1 first, then K = 4; the timed dispatches lead each half
        assert half >= REPS and len(d) == 2 * half, (hits[0], len(d))
        return d[:REPS], d[half:half + REPS]

    lines = [('kernel', 'link', 'K', 'calls', 'median_ns', 'min_ns', 'max_ns', 'spread_ns', 'ratio_to_logit')]
    for label, names in KERNELS:
        parts = {link: pick(names[link]) for link in LINKS}
        for i, K in enumerate((1, 4)):
            base = float(np.median(parts['logit'][i]))
            for link in LINKS:
                d = parts[link][i]
                lines.append((label, link, K, len(d), float(np.median(d)), min(d), max(d), max(d) - min(d), '%.3f' % (float(np.median(d)) / base)))
    with open(out, 'w', newline='') as f:
        csv.writer(f).writerows(lines)
    for l in lines:
        print(','.join(str(v) for v in l))


if len(sys.argv) > 1 and sys.argv[1] == '--summarize':
    summarize(sys.argv[2], sys.argv[3])
    sys.exit(0)

import lrvb_amd as vb
from scipy.special import ndtr
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
PROB = {'logit': lambda t: 1.0 / (1.0 + np.exp(-t)), 'probit': ndtr, 'cloglog': lambda t: -np.expm1(-np.exp(t))}


def timed(label, fn):
    out = None
    for rep in range(REPS):
        t0 = time.perf_counter(); out = fn(); t1 = time.perf_counter()
        print('%s: %.2f ms' % (label, (t1 - t0) * 1e3), flush=True)
    return out


for K in (1, KS):
    z = zs[:, :K]
    eta = off + x @ beta + (z * u[gid, :K]).sum(1)
    pt = (beta, v, u[:, :K], np.full((G, K), np.exp(-3.0)))
    # the point of tools/time_glmm_predict.py in free coordinates, at which the block arrow is positive definite
    th = np.concatenate([beta, np.full(P, 6.0), np.zeros(K), np.full(K, 3.0), np.tile([np.log(G / 2.0), np.log(G / 4.0)], K),
                         u[:, :K].ravel(), np.full(G * K, 3.0)])
    A = rng.normal(size=(Q, 2 * P + 2 * G * K))
    for link in LINKS:
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        y = rng.binomial(trials.astype(np.int64), PROB[link](eta)).astype(np.float64)
        fun = vb.BinomialGLMMObjective(par, x, y, z, gid, G, trials=trials, offset=off, gh_deg=20, weights=w, link=link)
        ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
        tag = '%s, K = %d, N = %d, P = %d, G = %d' % (link, K, N, P, G)
        val = timed('%s: value-only terms' % tag, lambda: ctx.glmm_binomial_terms(*pt, *gh, want_grad=False, want_hess=False)[0])
        r = timed('%s: influence rows, Q = %d (N x Q to the host)' % (tag, Q), lambda: ctx.glmm_binomial_obs_influence(*pt, *gh, A))
        g = timed('%s: group influence' % tag, lambda: ctx.glmm_binomial_group_influence(*pt, *gh, A))
        fit = timed('%s: predict, all rows (5 x N to the host)' % tag, lambda: fun.predict(th, on_device=True))
        print('%s: value %.6e, |rows| %.3e, |groups| %.3e, mean fitted probability %.4f' % (
            tag, val, np.abs(r).max(), np.abs(g).max(), np.mean(fit['mean_lrvb'] / trials)), flush=True)
        del fun, ctx

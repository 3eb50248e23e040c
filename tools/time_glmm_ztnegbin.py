"""Times the three walks of the zero-truncated NB2 mixed model next to the binomial (logit and cloglog) and
the zero-truncated Poisson instantiations of the same tile walk -- the yardsticks -- in ONE process, at K = 2:
`BinomialGLMMObjective` under both links, `TruncatedPoissonGLMMObjective` and `TruncatedNegBinomialGLMMObjective` on the same x, z,
groups, offset and point: the value-only terms call (the rows pass), the influence row entry over all N, the group entry and
`predict` over all N on the device, REPS times each.  Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_ztnegbin.py [N [P [G [Q]]]]

for the kernel durations (no counters in that run), then

    python tools/time_glmm_ztnegbin.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel and family: calls, median, min, max in ns, the spread (max - min over the timed dispatches of the
same run) and the ratio of the median to the logit, the cloglog and the zero-truncated Poisson median.  Reported as measured; none
of it is a pass threshold.  The first REPS dispatches of every kernel are the timed ones (the first `predict` forms the terms and
the factor once more, behind them).
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
FAMILIES = ('logit', 'cloglog', 'ztpoisson', 'ztnegbin')
# kernel label -> per family, the substrings that pick its dispatches out of the trace (spaces removed from the names)
KERNELS = (('rows', {'logit': ('glmm_slopes_rows_kernel', '<BinomialLik>'), 'cloglog': ('glmm_slopes_rows_kernel', 'BinomialLinkLik<2'),
                     'ztpoisson': ('glmm_slopes_rows_kernel', 'TruncPoissonLik'), 'ztnegbin': ('glmm_slopes_rows_kernel', 'TruncNegBinLik')}),
           ('influence rows', {'logit': ('glmm_binomial_infl_rows_kernel',), 'cloglog': ('glmm_link_infl_rows_kernel<2',),
                               'ztpoisson': ('glmm_ztpoisson_infl_rows_kernel',), 'ztnegbin': ('glmm_ztnegbin_infl_rows_kernel',)}),
           ('group sums', {'logit': ('glmm_slopes_infl_gsum_kernel', '<BinomialLik>'), 'cloglog': ('glmm_slopes_infl_gsum_kernel', 'BinomialLinkLik<2'),
                           'ztpoisson': ('glmm_slopes_infl_gsum_kernel', 'TruncPoissonLik'),
                           'ztnegbin': ('glmm_slopes_infl_gsum_kernel', 'TruncNegBinLik')}),
           ('predict', {'logit': ('glmm_binomial_predict_rows_kernel',), 'cloglog': ('glmm_link_predict_rows_kernel<2',),
                        'ztpoisson': ('glmm_ztpoisson_predict_rows_kernel',), 'ztnegbin': ('glmm_ztnegbin_predict_rows_kernel',)}))


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
        assert len(dur[hits[0]]) >= REPS, (hits[0], len(dur[hits[0]]))
        return dur[hits[0]][:REPS]

    lines = [('kernel', 'family', 'calls', 'median_ns', 'min_ns', 'max_ns', 'spread_ns', 'ratio_to_logit', 'ratio_to_cloglog', 'ratio_to_ztpoisson')]
    for label, names in KERNELS:
        parts = {fam: pick(names[fam]) for fam in FAMILIES}
        base = {fam: float(np.median(parts[fam])) for fam in FAMILIES}
        for fam in FAMILIES:
            d = parts[fam]
            lines.append((label, fam, len(d), base[fam], min(d), max(d), max(d) - min(d)) +
                         tuple('%.3f' % (base[fam] / base[b]) for b in ('logit', 'cloglog', 'ztpoisson')))
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
K = 2
rng = np.random.default_rng(1)
x = rng.standard_normal((N, P)) / np.sqrt(P)
z = np.concatenate([np.ones((N, 1)), 0.5 * rng.standard_normal((N, K - 1))], axis=1)
gid = rng.integers(0, G, size=N).astype(np.int32)
u, beta = rng.normal(size=(G, K)) * 0.5, rng.normal(size=P) * 0.5
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


lam = np.exp(off + x @ beta + (z * u[gid]).sum(1))
counts = rng.negative_binomial(phi, phi / (phi + lam)).astype(np.float64)
pt = (beta, v, u, np.full((G, K), np.exp(-3.0)))
# the point of tools/time_glmm_predict.py in free coordinates, at which the block arrow is positive definite
th = np.concatenate([beta, np.full(P, 6.0), np.zeros(K), np.full(K, 3.0), np.tile([np.log(G / 2.0), np.log(G / 4.0)], K),
                     u.ravel(), np.full(G * K, 3.0)])
A = rng.normal(size=(Q, 2 * P + 2 * G * K))
for fam in FAMILIES:
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    pos = np.maximum(counts, 1.0)                                        # all N rows, so that the four walk the same rows
    if fam in ('logit', 'cloglog'):
        fun = vb.BinomialGLMMObjective(par, x, (counts > 0).astype(np.float64), z, gid, G, offset=off, gh_deg=20, weights=w, link=fam)
        name = 'glmm_binomial'
    elif fam == 'ztpoisson':
        fun = vb.TruncatedPoissonGLMMObjective(par, x, pos, z, gid, G, offset=off, gh_deg=20, weights=w)
        name = 'glmm_ztpoisson'
    else:
        fun = vb.TruncatedNegBinomialGLMMObjective(par, x, pos, z, gid, G, phi, offset=off, gh_deg=20, weights=w)
        name = 'glmm_ztnegbin'
    ctx, head = fun.ctx, pt + (fun.gh_x, fun.gh_w)
    tag = '%s, K = %d, N = %d, P = %d, G = %d' % (fam, K, N, P, G)
    val = timed('%s: value-only terms' % tag, lambda: getattr(ctx, name + '_terms')(*head, want_grad=False, want_hess=False)[0])
    r = timed('%s: influence rows, Q = %d (N x Q to the host)' % (tag, Q), lambda: getattr(ctx, name + '_obs_influence')(*head, A))
    g = timed('%s: group influence' % tag, lambda: getattr(ctx, name + '_group_influence')(*head, A))
    fit = timed('%s: predict, all rows (5 x N to the host)' % tag, lambda: fun.predict(th, on_device=True))
    print('%s: value %.6e, |rows| %.3e, |groups| %.3e, mean fitted value %.4f' % (
        tag, val, np.abs(r).max(), np.abs(g).max(), np.mean(fit['mean_lrvb'])), flush=True)
    del fun, ctx

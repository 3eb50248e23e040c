"""Times the prediction kernels next to their yardsticks, in ONE process: for K = 1 and K = 4 on one
`LogisticGLMMSlopesObjective`, REPS times each,

    the influence row entry at Q outputs over all N    glmm_slopes_infl_rows_kernel      (the yardstick: same tile, same gathers)
    the elimination                                    glmm_slopes_schur_rows_kernel     (the yardstick of the group covariance)
    the group covariance                               glmm_slopes_group_cov_kernel
    predict over all N                                 glmm_slopes_predict_rows_kernel
    predict over all N on a second model whose rows are SORTED by group -- the same kernel, the same loads, but the K P + K K
                                                       gathered doubles of a row are those of its neighbours in the tile: the
                                                       difference is the cost of gathering them from G different places

Run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_glmm_predict.py [N [P [G [Q]]]]

for the kernel durations, then

    python tools/time_glmm_predict.py --summarize DIR/.../*_kernel_trace.csv OUT.csv

which writes one line per kernel and K: calls, median, min, max in ns.  Reported as measured; none of it is a pass threshold.
"""
import sys, os, time, csv
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

REPS = 5
KERNELS = ('glmm_slopes_infl_rows_kernel', 'glmm_slopes_schur_rows_kernel', 'glmm_slopes_group_cov_kernel', 'glmm_slopes_predict_rows_kernel')


def summarize(trace, out):
    with open(trace, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = {}
    for r in rows:
        for k in KERNELS:
            if k in r['Kernel_Name']:
                dur.setdefault(k, []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    lines = [('kernel', 'K', 'variant', 'calls', 'median_ns', 'min_ns', 'max_ns')]
    for k in KERNELS:
        d = dur[k]
        per_k = len(d) // 2                                              # K = 1 first, then K = 4
        for i, K in enumerate((1, 4)):
            part = d[i * per_k:(i + 1) * per_k]
            if k == 'glmm_slopes_predict_rows_kernel':                   # REPS with the rows as they come, then REPS sorted by group
                chunks = (('rows spread over the groups', part[:REPS]), ('rows sorted by group', part[REPS:]))
            elif len(part) == REPS + 1:                                   # the elimination and the group covariance run once more, for the second model
                chunks = (('', part[:REPS]), ('second model (rows sorted by group), not part of the statistics above', part[REPS:]))
            else:
                chunks = (('', part),)
            for name, c in chunks:
                lines.append((k, K, name, len(c), float(np.median(c)), min(c), max(c)))
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
w = rng.uniform(0.5, 1.5, size=N)


def timed(label, fn):
    out = None
    for rep in range(REPS):
        t0 = time.perf_counter(); out = fn(); t1 = time.perf_counter()
        print('%s: %.2f ms' % (label, (t1 - t0) * 1e3), flush=True)
    return out


for K in (1, KS):
    z = zs[:, :K]
    pr = 1.0 / (1.0 + np.exp(-(x @ beta + (z * u[gid, :K]).sum(1))))
    y = (rng.uniform(size=N) < pr).astype(np.float64)
    # the point of tools/time_glmm_slopes_solve.py, at which the block arrow is positive definite
    th = np.concatenate([beta, np.full(P, 6.0), np.zeros(K), np.full(K, 3.0), np.tile([np.log(G / 2.0), np.log(G / 4.0)], K),
                         u[:, :K].ravel(), np.full(G * K, 3.0)])
    tag = 'K = %d, N = %d, P = %d, G = %d' % (K, N, P, G)
    for order, groups in (('rows spread over the groups', gid), ('rows sorted by group', np.sort(gid))):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        fun = vb.LogisticGLMMSlopesObjective(par, x, y, z, groups, G, gh_deg=20, weights=w)
        ctx, gh = fun.ctx, (fun.gh_x, fun.gh_w)
        if groups is gid:
            pt = (beta, np.full(P, np.exp(-6.0)), u[:, :K], np.full((G, K), np.exp(-3.0)))
            A = rng.normal(size=(Q, 2 * P + 2 * G * K))
            timed('%s: influence rows, Q = %d (N x Q to the host)' % (tag, Q), lambda: ctx.glmm_slopes_obs_influence(*pt, *gh, A))

            def factor():
                fun.value(th)                                            # drops the factor: the elimination runs again
                return fun._device_factors(th, True)
            timed('%s: terms + elimination + Schur factor' % tag, factor)
            cov = timed('%s: group covariance (chol_solve of R columns, upload, kernel, (G + 1) rows to the host)' % tag,
                        lambda: fun.group_cov(th, on_device=True))
        # sorted by group the K P + K K gathered doubles of a row are those of its neighbours: the difference is the cost of the gather
        fit = timed('%s: predict, all rows, %s (5 x N to the host)' % (tag, order), lambda: fun.predict(th, on_device=True))
        del fun, ctx
    se = np.sqrt(cov[1].diagonal(axis1=1, axis2=2))
    print('%s: se(u) LRVB %.4f .. %.4f, sd of the linear predictor LRVB / mean-field: median %.3f' % (
        tag, se.min(), se.max(), np.median(np.sqrt(fit['var_lrvb'] / fit['var_mf']))), flush=True)

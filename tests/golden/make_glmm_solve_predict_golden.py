"""Cases and recorder of tests/golden/glmm_solve_predict_parent.npz: the outputs and the refusals of the device-resident block-arrow
layer of the K-effect mixed models (lrvb_glmm_slopes_schur, lrvb_glmm_slopes_solve_forward / _back, lrvb_glmm_slopes_group_cov and
the three predict entries) on the logistic, Poisson, binomial and negative-binomial families, and the binomial walk
(terms, row and group influence) with trials != 1, as the commit BEFORE the window walk, the local triangular solves and the
host bodies were shared computed them on an MI355X.  tests/test_gpu_glmm_solve_predict_golden.py asks the
present build for the same bits and the same messages.

The shapes are the six of make_glmm_golden.CASES; the storage rules, `digest`, `matches` and RAW_MAX are that file's: every case is
rebuilt from its seed, only a digest of the inputs is stored, arrays of up to RAW_MAX doubles raw, larger ones as shape + SHA-256.
The point of a case is the point of `glmm_slopes_reference.problem` at the case's seed, as in
tests/test_gpu_glmm_slopes_device_solve.py and tests/test_gpu_glmm_predict.py; the recorder goes through the objective classes, so
a point at which a factorisation is refused ends the recording with that error.  A refusal is stored as its status code and the
text of lrvb_last_error().

Recording (once, from a build of the parent commit, in a process of its own; the library under test never writes the file):

    python tests/golden/make_glmm_solve_predict_golden.py --root <tree with the parent's liblrvb_hip.so> --commit <its hash> [--out FILE]
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_glmm_golden as mg                                           # noqa: E402
from make_glmm_golden import RAW_MAX, digest, matches                   # noqa: E402,F401

FIXTURE = os.path.join(HERE, 'glmm_solve_predict_parent.npz')
CASES = mg.CASES
FAMILIES = ('logistic', 'poisson', 'binomial', 'negbinomial')
SOLVE_QS = (1, 70, 129)                                                  # workgroups of 64 / 128 / 256 threads in launch_glmm_slopes_solve
INFL_QS = mg.QS
N_NEW = 70                                                               # new rows: a second tile of six rows
COLS = ('rho', 'var_mf', 'var_lrvb', 'mean_mf', 'mean_lrvb')
REFUSAL_CASE = 'cut_group'
N_REFUSALS = 60
# The rule of tests/test_gpu_glmm_slopes_device_solve.py: the first of N + P + K, N + P + K + 1, .. at which the reference Hessian
# of every family is positive definite at the point of the problem (found on the CPU with the modules of tests/).
SEEDS = dict(degenerate=3, cut_group=72, unit_design=41, many_groups=220, wrap=321, middle_tile=198)
# many_groups (40 groups of about five rows, three effects each) has no such seed among the first forty: where the spread of the
# e_g about e_mu exceeds their variances, the block of (e_g, log b_k) is indefinite unless the data outweigh it, and five Bernoulli
# rows do not.  Its point keeps a quarter of every deviation e_g - e_mu; the smallest eigenvalue of the four reference Hessians is
# then 0.050 (logistic), 0.17, 0.15, 0.14.
SHRINK = dict(many_groups=0.25)


def _refs():
    if mg.TESTS not in sys.path:
        sys.path.insert(0, mg.TESTS)
    import glmm_binomial_reference as bref
    import glmm_poisson_reference as pref
    import glmm_slopes_reference as sref
    return sref, pref, bref


def build_case(case, seed=None):
    """dict of the inputs of one case.  x, z, w, gid and the free point are those of `glmm_slopes_reference.problem` at the
    seed of SEEDS (z with its non-intercept columns halved, as the Poisson and binomial problems have it), with the case's
    modifications of make_glmm_golden.build_case; y, offset, trials and dispersion per family; the new rows; the right-hand
    sides of the solve."""
    sref, pref, bref = _refs()
    N, P, K, G = case['shape']
    seed = SEEDS[case['name']] if seed is None else seed
    kw = dict(big_group=case.get('big_group', True))
    _, y_log, _, _, _, _ = sref.problem(N, P, K, G, seed, **kw)
    _, y_poi, _, _, _, o_poi, _ = pref.problem(N, P, K, G, seed, **kw)
    x, y_bin, z, w, gid, o_bin, trials, free = bref.problem(N, P, K, G, seed, **kw)
    _, y_nb, _, _, _, _, phi, _ = bref.nb_problem(N, P, K, G, seed, phi='vector', **kw)
    if case['name'] in SHRINK:
        ng, e_mu = 2 * P + 4 * K, free[2 * P:2 * P + K]
        free = free.copy()
        free[ng:ng + G * K] = (e_mu + SHRINK[case['name']] * (free[ng:ng + G * K].reshape(G, K) - e_mu)).ravel()
    rng = np.random.default_rng([N, P, K, G])
    if 'sizes' in case:                                                  # groups of the given sizes, rows in a shuffled order
        gid = np.repeat(np.arange(G), case['sizes']).astype(np.int32)[rng.permutation(N)]
    if case.get('zero_weights'):
        w = w.copy()
        w[gid == 2] = 0.0
        w[[0, 17, 64, N - 1]] = 0.0
    rn = np.random.default_rng([N, P, K, G, 33])
    gn = rn.integers(0, G, size=N_NEW)
    gn[::9] = -1                                                         # the pseudo-group of a population-level row
    new = dict(x=rn.normal(size=(N_NEW, P)) / np.sqrt(P),
               z=np.concatenate([np.ones((N_NEW, 1)), 0.5 * rn.normal(size=(N_NEW, K - 1))], axis=1), groups=gn.astype(np.int32),
               offset=0.3 * rn.normal(size=N_NEW), trials=rn.integers(0, 13, size=N_NEW).astype(np.float64))
    D = 2 * P + 4 * K + 2 * G * K
    rhs = {Q: np.random.default_rng([N, P, K, G, Q, 34]).normal(size=(D, Q)) for Q in SOLVE_QS}
    return dict(x=x, z=z, w=w, gid=gid, free=free, y_logistic=y_log, y_poisson=y_poi, y_binomial=y_bin, y_negbinomial=y_nb,
                o_poisson=o_poi, o_binomial=o_bin, trials=trials, phi=phi, new=new, rhs=rhs, deg=case.get('deg', 20))


def inputs_digest(b):
    h = hashlib.sha256()
    for k in ('x', 'z', 'w', 'free', 'y_logistic', 'y_poisson', 'y_binomial', 'y_negbinomial', 'o_poisson', 'o_binomial', 'trials', 'phi'):
        h.update(np.ascontiguousarray(b[k], dtype='<f8').tobytes())
    h.update(np.ascontiguousarray(b['gid'], dtype='<i4').tobytes())
    for k in ('x', 'z', 'offset', 'trials'):
        h.update(np.ascontiguousarray(b['new'][k], dtype='<f8').tobytes())
    h.update(np.ascontiguousarray(b['new']['groups'], dtype='<i4').tobytes())
    for Q in SOLVE_QS:
        h.update(np.ascontiguousarray(b['rhs'][Q], dtype='<f8').tobytes())
    return h.hexdigest()


def eta_of(b, P, K, G):
    """The vector coordinates of the free point."""
    sref = _refs()[0]
    return np.where(sref.positive_mask(P, K, G), np.exp(b['free']), b['free'])


def new_rows(family, b):
    """The `newdata` of `predict` for one family: the logistic model takes no offset, only the binomial one takes trials."""
    new = dict(x=b['new']['x'], z=b['new']['z'], groups=b['new']['groups'])
    if family != 'logistic':
        new['offset'] = b['new']['offset']
    if family == 'binomial':
        new['trials'] = b['new']['trials']
    return new


def objective(vb, case, b, family):
    N, P, K, G = case['shape']
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    kw = dict(beta_prior_info=mg.HYP[0], mu_prior=mg.HYP[1:3], tau_prior=mg.HYP[3:5], weights=b['w'])
    x, z, gid, y = b['x'], b['z'], b['gid'], b['y_' + family]
    if family == 'logistic':
        return vb.LogisticGLMMSlopesObjective(par, x, y, z, gid, G, gh_deg=b['deg'], **kw)
    if family == 'poisson':
        return vb.PoissonGLMMObjective(par, x, y, z, gid, G, offset=b['o_poisson'], **kw)
    if family == 'binomial':
        return vb.BinomialGLMMObjective(par, x, y, z, gid, G, trials=b['trials'], offset=b['o_binomial'], gh_deg=b['deg'], **kw)
    return vb.NegBinomialGLMMObjective(par, x, y, z, gid, G, b['phi'], offset=b['o_binomial'], gh_deg=b['deg'], **kw)


def _capture(ctx, name, sink):
    """Keep what the context method `name` is given and returns, call by call."""
    inner = getattr(ctx, name)

    def outer(*a, **k):
        out = inner(*a, **k)
        sink.append((a, out))
        return out
    setattr(ctx, name, outer)


def run_case(vb, case, b):
    """{'<family>/<output>': array} on the build `vb` was imported from."""
    N, P, K, G = case['shape']
    n0, n1 = mg.window(N)
    out = {}
    for family in FAMILIES:
        fun = objective(vb, case, b, family)
        ctx, free = fun.ctx, b['free']
        schur, fwd, back, gcov = [], [], [], []
        for name, sink in (('glmm_slopes_schur', schur), ('glmm_slopes_solve_forward', fwd), ('glmm_slopes_solve_back', back),
                           ('glmm_slopes_group_cov', gcov)):
            _capture(ctx, name, sink)
        for Q in SOLVE_QS:
            fun.solve(free, b['rhs'][Q], on_device=True)
            out['%s/solve_forward_q%d' % (family, Q)], out['%s/solve_back_q%d' % (family, Q)] = fwd[-1][1], back[-1][1]
        assert len(schur) == 1 and len(fwd) == len(back) == len(SOLVE_QS)        # one factor for the three solves
        out[family + '/schur'] = schur[0][1]
        fun.group_cov(free, on_device=True)
        out[family + '/group_cov'] = gcov[-1][1]
        res = fun.predict(free, n0=n0, n1=n1, on_device=True)
        out[family + '/predict_window'] = np.stack([res[k] for k in COLS])
        res = fun.predict(free, newdata=new_rows(family, b), on_device=True)
        out[family + '/predict_new'] = np.stack([res[k] for k in COLS])
        assert len(schur) == 1
        if family == 'binomial':                                         # the walk with trials != 1 and an offset
            pt = mg.point(eta_of(b, P, K, G), P, K, G) + (fun.gh_x, fun.gh_w)
            val, gg, Hb, gs = ctx.glmm_binomial_terms(*pt)
            out.update({'binomial/value': np.array([val]), 'binomial/grad': gg, 'binomial/H_blocks': Hb, 'binomial/group_sums': gs})
            for Q in INFL_QS:
                A = mg.operand(case, Q)
                out['binomial/obs_influence_q%d' % Q] = ctx.glmm_binomial_obs_influence(*pt, A, n0, n1)
                out['binomial/group_influence_q%d' % Q] = ctx.glmm_binomial_group_influence(*pt, A)
        del fun
    return out


def run_refusals(vb, case, b):
    """{'<entry>/<what is wrong>': (status, text of lrvb_last_error())} by direct calls of the C entries, on the logistic family."""
    hip = vb._hip
    N, P, K, G = case['shape']
    fun = objective(vb, case, b, 'logistic')
    ctx, free = fun.ctx, b['free']
    lib, h, p = ctx._lib, ctx._h, hip.ptr
    R, Q = 2 * P + 3 * K, 3
    out = {}

    def record(key, status):
        out[key] = (int(status), hip.last_error())
        assert int(status) != hip.OK, key

    eta = eta_of(b, P, K, G)
    m, v = hip.as_f64(eta[:P]).copy(), hip.as_f64(1.0 / eta[P:2 * P])
    ng, GK = 2 * P + 4 * K, G * K
    e2 = hip.as_f64(np.vstack([eta[ng:ng + GK].reshape(G, K), eta[2 * P:2 * P + K][None, :]]))
    r2 = hip.as_f64(np.vstack([1.0 / eta[ng + GK:].reshape(G, K), 1.0 / eta[2 * P + K:2 * P + 2 * K][None, :]]))
    gx, gw = hip.as_f64(fun.gh_x), hip.as_f64(fun.gh_w)
    Sbb, W, s = hip.as_f64(np.eye(P)), hip.as_f64(np.eye(R)), hip.as_f64(np.ones(R))
    M, red, Xl = np.empty((R, R)), np.empty((R, Q)), np.empty((G, 2 * K, Q))
    Rl, xc = hip.as_f64(np.ones((G, 2 * K, Q))), hip.as_f64(np.ones((R, Q)))
    gbuf, pout = np.empty((G + 1, K * K + K * P)), np.empty((5, N))
    xn, zn = hip.as_f64(b['new']['x'][:4]).copy(), hip.as_f64(b['new']['z'][:4]).copy()

    def fwd(Rl_=Rl, G_=G, K_=K, Q_=Q, red_=red):
        return lib.lrvb_glmm_slopes_solve_forward(h, p(Rl_), G_, K_, Q_, p(red_))

    def back(xc_=xc, G_=G, K_=K, Q_=Q, X_=Xl):
        return lib.lrvb_glmm_slopes_solve_back(h, p(xc_), G_, K_, Q_, p(X_))

    def gcov(W_=W, s_=s, P_=P, G_=G, K_=K):
        return lib.lrvb_glmm_slopes_group_cov(h, p(W_), p(s_), P_, G_, K_, p(gbuf))

    def predict(mean=m, e_=e2, r_=r2, Gp=G + 1, K_=K, cov=Sbb, n0=0, n1=N, new=None, out_=pout, z_new=True):
        rows = [None, None, None, 0]
        if new is not None:
            gid = np.ascontiguousarray(new, dtype=np.int32)
            rows = [p(xn), p(zn) if z_new else None, gid.ctypes.data, gid.size]
        return lib.lrvb_glmm_slopes_predict(h, p(mean), p(v), P, p(e_), p(r_), Gp, K_, p(gx), p(gw), gx.size, p(cov), n0, n1, *rows, p(out_))

    # nothing resident
    args = []
    _capture(ctx, 'glmm_slopes_schur', args)
    fun.global_hessian(free, want_host=False)                            # the blocks, chain factors and closed rows of this point
    loc, sc, cl = (hip.as_f64(a).copy() for a in args[0][0])
    del ctx.glmm_slopes_schur
    ctx.set_group_design(b['z'])                                         # drops the sums and the factor
    schur = lambda loc_=loc, sc_=sc, cl_=cl, G_=G, K_=K, M_=M: lib.lrvb_glmm_slopes_schur(h, p(loc_), p(sc_), p(cl_), G_, K_, p(M_))
    record('schur/no_sums', schur())
    record('solve_forward/no_sums', fwd())
    record('solve_back/no_sums', back())
    record('group_cov/no_sums', gcov())
    record('predict/no_sums', predict())
    fun.value(free)                                                      # group sums, no factor
    record('schur/null_blocks', schur(loc_=None))
    record('schur/null_out', schur(M_=None))
    record('schur/k_0', schur(K_=0))
    record('schur/k_5', schur(K_=5))
    record('schur/k_other', schur(K_=K + 1))
    record('schur/wrong_g', schur(G_=G + 1))
    record('solve_forward/no_factor', fwd())
    record('solve_back/no_factor', back())
    record('group_cov/no_factor', gcov())
    record('predict/no_factor', predict())
    bad_loc = loc.copy()
    bad_loc[1, 0] = -1.0                                                 # the first pivot of group 1
    record('schur/not_positive_definite', schur(loc_=bad_loc))
    record('solve_forward/after_bad_block', fwd())
    assert schur() == hip.OK
    for name, entry in (('solve_forward', fwd), ('solve_back', back)):
        record(name + '/k_0', entry(K_=0))
        record(name + '/k_5', entry(K_=5))
        record(name + '/k_other', entry(K_=K + 1))
        record(name + '/q_0', entry(Q_=0))
        record(name + '/wrong_g', entry(G_=G - 1))
    record('solve_forward/null_in', fwd(Rl_=None))
    record('solve_forward/null_out', fwd(red_=None))
    record('solve_back/null_in', back(xc_=None))
    record('solve_back/null_out', back(X_=None))
    record('solve_back/no_forward', back())
    assert fwd() == hip.OK
    record('solve_back/other_columns', back(xc_=hip.as_f64(np.ones((R, 2))), Q_=2, X_=np.empty((G, 2 * K, 2))))
    assert back() == hip.OK
    record('group_cov/null_w', gcov(W_=None))
    record('group_cov/null_s', gcov(s_=None))
    record('group_cov/k_0', gcov(K_=0))
    record('group_cov/k_5', gcov(K_=5))
    record('group_cov/wrong_g', gcov(G_=G + 1))
    record('group_cov/wrong_p', gcov(P_=P + 1))
    record('predict/no_group_cov', predict())
    record('predict/no_group_cov_new_rows', predict(new=[0, 1, 1, 0]))
    assert gcov() == hip.OK
    assert predict() == hip.OK and predict(new=[0, G, 1, 2]) == hip.OK
    record('predict/null_mean', predict(mean=None))
    record('predict/null_cov_beta', predict(cov=None))
    record('predict/null_out', predict(out_=None))
    record('predict/k_0', predict(K_=0))
    record('predict/k_5', predict(K_=5))
    record('predict/groups_above', predict(e_=hip.as_f64(np.vstack([e2, e2[:1]])), r_=hip.as_f64(np.vstack([r2, r2[:1]])), Gp=G + 2))
    record('predict/groups_below', predict(e_=e2[:G - 1].copy(), r_=r2[:G - 1].copy(), Gp=G - 1))
    record('predict/new_group_above', predict(new=[0, G + 1, 1, 2]))
    record('predict/new_group_negative', predict(new=[0, 1, -1, 2]))
    record('predict/new_group_pseudo_without_its_row', predict(e_=e2[:G].copy(), r_=r2[:G].copy(), Gp=G, new=[0, G, 1, 2]))
    record('predict/new_rows_without_z', predict(new=[0, 1, 1, 0], z_new=False))
    record('predict/window_high', predict(n1=N + 1))
    record('predict/window_reversed', predict(n0=4, n1=3))
    bad_r = r2.copy()
    bad_r[G, 0] = 0.0
    record('predict/pseudo_r_not_positive', predict(r_=bad_r))
    fun.value(free)                                                      # a later terms call drops the factor and what hangs on it
    record('solve_forward/after_terms', fwd())
    record('group_cov/after_terms', gcov())
    record('predict/after_terms', predict())
    del fun
    # the intercept's elimination leaves no factor for the K-effect solve
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParam('mu'))
    par.push_param(vb.GammaParam('tau'))
    par.push_param(vb.UVNParamVector('u', length=G))
    fun = vb.LogisticGLMMObjective(par, b['x'], b['y_logistic'], b['gid'], G, gh_deg=b['deg'], weights=b['w'])
    ctx = fun.ctx
    lib, h = ctx._lib, ctx._h
    ctx.glmm_terms(m, v, e2[:G, 0].copy(), r2[:G, 0].copy(), fun.gh_x, fun.gh_w)
    rng = np.random.default_rng(7)
    d = rng.uniform(1.0, 2.0, size=(G, 2))
    loc1 = hip.as_f64(np.stack([d[:, 0], rng.uniform(-0.5, 0.5, size=G), d[:, 1]], axis=1))
    sc1, cl1, M1 = hip.as_f64(rng.uniform(0.5, 1.5, size=(G, 2))), hip.as_f64(rng.normal(size=(G, 6))), np.empty((2 * P + 3, 2 * P + 3))
    assert lib.lrvb_glmm_schur(h, p(loc1), p(sc1), p(cl1), G, p(M1)) == hip.OK
    record('solve_forward_k1_after_intercept_schur',
           lib.lrvb_glmm_slopes_solve_forward(h, p(hip.as_f64(np.ones((G, 2, Q)))), G, 1, Q, p(np.empty((2 * P + 3, Q)))))
    record('group_cov_k1_after_intercept_schur',
           lib.lrvb_glmm_slopes_group_cov(h, p(hip.as_f64(np.eye(2 * P + 3))), p(hip.as_f64(np.ones(2 * P + 3))), P, G, 1, None))
    del fun
    return out


def refusal_matches(fixture, key, got):
    return (int(fixture['refusal/' + key + ':status']), str(fixture['refusal/' + key + ':text'])) == got


def main(argv):
    import argparse
    import subprocess
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--root', required=True, help='the tree whose build is recorded (it holds lrvb_amd.py and the built library)')
    ap.add_argument('--commit', required=True, help='the commit hash of that tree')
    ap.add_argument('--out', default=FIXTURE)
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.root))
    import lrvb_amd as vb
    assert os.path.dirname(os.path.abspath(vb.__file__)).startswith(os.path.abspath(a.root)), vb.__file__
    assert vb._hip.device_count() >= 1, 'no HIP device visible'
    store = {'parent_commit': np.array(a.commit),
             'hipcc_version': np.array(subprocess.run(['hipcc', '--version'], capture_output=True, text=True, check=True).stdout.strip())}
    for case in CASES:
        b = build_case(case)
        store[case['name'] + ':inputs'] = np.array(inputs_digest(b))
        for key, arr in run_case(vb, case, b).items():
            key = case['name'] + '/' + key
            arr = np.asarray(arr, dtype=np.float64)
            assert np.all(np.isfinite(arr)), key
            if arr.size <= RAW_MAX:
                store[key] = arr
            else:
                store[key + ':shape'], store[key + ':sha256'] = np.array(arr.shape), np.array(digest(arr))
    case = next(c for c in CASES if c['name'] == REFUSAL_CASE)
    for key, (status, text) in run_refusals(vb, case, build_case(case)).items():
        store['refusal/' + key + ':status'], store['refusal/' + key + ':text'] = np.array(status), np.array(text)
        print('%-50s %d  %s' % (key, status, text))
    np.savez(a.out, **store)
    print('wrote %s: %d entries, %d bytes' % (a.out, len(store), os.path.getsize(a.out)))


if __name__ == '__main__':
    main(sys.argv[1:])

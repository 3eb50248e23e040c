"""Cases and recorder of tests/golden/glmm_intercept_parent.npz: the outputs and the refusals of the four random-intercept entries
(lrvb_glmm_{terms,schur,obs_influence,group_influence}) as the commit BEFORE they moved onto the shared likelihood policy, the shared
host bodies and the shared resident buffer computed them on an MI355X.
tests/test_gpu_glmm_intercept_golden.py asks the present build for the same bits and the same messages.

The storage rules, `digest` and `matches` are those of make_glmm_golden.py: every case is rebuilt from its seed, only a digest of
the inputs is stored, arrays of up to RAW_MAX doubles raw, larger ones as shape + SHA-256.  A refusal is stored as its status code
and the text of lrvb_last_error().

Recording (once, from a build of the parent commit, in a process of its own; the library under test never writes the file):

    python tests/golden/make_glmm_intercept_golden.py --root <tree with the parent's liblrvb_hip.so> --commit <its hash> [--out FILE]
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_glmm_golden as mg                                           # noqa: E402

FIXTURE = os.path.join(HERE, 'glmm_intercept_parent.npz')
QS = mg.QS

# (N, P, G) and what the case is the smallest witness of
CASES = [
    dict(name='degenerate', shape=(1, 1, 1)),                            # the degenerate walk
    dict(name='cut_group', shape=(65, 5, 3), deg=5),                     # second tile of one row; group 1 cut at row 64: both partial
                                                                         # slots and the fixup; group 2 empty; nq = 5
    dict(name='small', shape=(37, 3, 5)),
    dict(name='many_groups', shape=(200, 17, 40), big_group=False),      # most groups whole inside a tile; 4 P = 68 < 256
    dict(name='odd_p', shape=(300, 63, 7), zero_weights=True),           # 4 P = 252: threads 252..255 own no column; the MFMA loop pads
    dict(name='middle_tile', shape=(130, 64, 2), sizes=(30, 100)),       # every thread owns a column; group 1 covers the tile 64..127
]
REFUSAL_CASE = 'small'


def _gref():
    if mg.TESTS not in sys.path:
        sys.path.insert(0, mg.TESTS)
    import glmm_reference as gref
    return gref


def build_case(case):
    """dict of the inputs of one case: x, y, w, gid, eta (vector coordinates of the point), deg."""
    gref = _gref()
    N, P, G = case['shape']
    x, y, w, gid, free = gref.problem(N, P, G, seed=N + P + G, big_group=case.get('big_group', True))
    rng = np.random.default_rng([N, P, G])
    if 'sizes' in case:                                                  # groups of the given sizes, rows in a shuffled order
        gid = np.repeat(np.arange(G), case['sizes']).astype(np.int32)[rng.permutation(N)]
    if case.get('zero_weights'):
        w = w.copy()
        w[gid == 2] = 0.0
        w[[0, 17, 64, N - 1]] = 0.0
    eta = np.where(gref.positive_mask(P, G), np.exp(free), free)
    return dict(x=x, y=y, w=w, gid=gid, eta=eta, deg=case.get('deg', 20))


def inputs_digest(b):
    h = hashlib.sha256()
    for k in ('x', 'y', 'w', 'eta'):
        h.update(np.ascontiguousarray(b[k], dtype='<f8').tobytes())
    h.update(np.ascontiguousarray(b['gid'], dtype='<i4').tobytes())
    return h.hexdigest()


def point(eta, P, G):
    ng = 2 * P + 4
    return eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:]


def operand(case, Q):
    N, P, G = case['shape']
    return np.random.default_rng([N, P, G, Q]).normal(size=(Q, 2 * P + 2 * G))


def schur_inputs(case):
    """Positive-definite 2 x 2 blocks [a11, a12, a22] (a11, a22 in (1, 2), |a12| < 1/2), chain factors and closed-form rows."""
    N, P, G = case['shape']
    rng = np.random.default_rng([N, P, G, 7])
    d = rng.uniform(1.0, 2.0, size=(G, 2))
    loc = np.stack([d[:, 0], rng.uniform(-0.5, 0.5, size=G), d[:, 1]], axis=1)
    return loc, rng.uniform(0.5, 1.5, size=(G, 2)), rng.normal(size=(G, 6))


def objective(vb, case, b):
    N, P, G = case['shape']
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParam('mu'))
    par.push_param(vb.GammaParam('tau'))
    par.push_param(vb.UVNParamVector('u', length=G))
    return vb.LogisticGLMMObjective(par, b['x'], b['y'], b['gid'], G, gh_deg=b['deg'], beta_prior_info=mg.HYP[0],
                                    mu_prior=mg.HYP[1:3], tau_prior=mg.HYP[3:5], weights=b['w'])


def run_case(vb, case, b):
    """{'<output>': array} of the four entries on the build `vb` was imported from."""
    N, P, G = case['shape']
    fun = objective(vb, case, b)
    ctx = fun.ctx
    pt = point(b['eta'], P, G) + (fun.gh_x, fun.gh_w)
    n0, n1 = mg.window(N)
    sch = schur_inputs(case)
    out = {}
    val, gg, gl, Hb, B, L = ctx.glmm_terms(*pt)
    out.update(value=np.array([val]), grad=gg, grad_local=gl, H_blocks=Hb, border=B, local=L)
    out['schur'] = ctx.glmm_schur(*sch)
    val, gg, gl, Hb, B, L = ctx.glmm_terms(*pt, want_border=False)
    assert B is None
    out.update({'no_border/value': np.array([val]), 'no_border/grad': gg, 'no_border/grad_local': gl, 'no_border/H_blocks': Hb,
                'no_border/local': L})
    out['no_border/schur'] = ctx.glmm_schur(*sch)                       # the border stayed on the device
    res = ctx.glmm_terms(*pt, want_grad=False, want_hess=False)
    assert all(a is None for a in res[1:])
    out['value_only'] = np.array([res[0]])
    for Q in QS:
        A = operand(case, Q)
        out['obs_influence_q%d' % Q] = ctx.glmm_obs_influence(*pt, A, n0, n1)
        out['group_influence_q%d' % Q] = ctx.glmm_group_influence(*pt, A)
    del fun
    return out


def run_refusals(vb, case, b):
    """{'<entry>/<what is wrong>': (status, text of lrvb_last_error())} by direct calls of the C entries."""
    hip = vb._hip
    N, P, G = case['shape']
    fun = objective(vb, case, b)
    ctx = fun.ctx
    lib, h, p = ctx._lib, ctx._h, hip.ptr
    m, v, e, r = (hip.as_f64(a).copy() for a in point(b['eta'], P, G))
    gx, gw = hip.as_f64(fun.gh_x), hip.as_f64(fun.gh_w)
    Q = 5
    Ag, Al = hip.as_f64(np.ones((Q, 2 * P))), hip.as_f64(np.ones((G, 2 * Q)))
    val, o_rows, o_grp = np.empty(1), np.empty((N, Q)), np.empty((G, Q))
    bad_v, bad_r = v.copy(), r.copy()
    bad_v[1], bad_r[2] = 0.0, -1.0
    out = {}

    def record(key, status):
        out[key] = (int(status), hip.last_error())
        assert int(status) != hip.OK, key

    def terms(mean=m, var=v, P_in=P, e_=e, r_=r, G_in=G, nq=gx.size):
        return lib.lrvb_glmm_terms(h, p(mean), p(var), P_in, p(e_), p(r_), G_in, p(gx), p(gw), nq, p(val), None, None, None, None, None)

    def rows(mean=m, var=v, P_in=P, e_=e, r_=r, G_in=G, nq=gx.size, Q_=Q, n0=0, n1=N):
        return lib.lrvb_glmm_obs_influence(h, p(mean), p(var), P_in, p(e_), p(r_), G_in, p(gx), p(gw), nq, p(Ag), p(Al), Q_, n0, n1, p(o_rows))

    def groups(mean=m, var=v, P_in=P, e_=e, r_=r, G_in=G, nq=gx.size, Q_=Q):
        return lib.lrvb_glmm_group_influence(h, p(mean), p(var), P_in, p(e_), p(r_), G_in, p(gx), p(gw), nq, p(Ag), p(Al), Q_, p(o_grp))

    loc, sc, cl = (hip.as_f64(a) for a in schur_inputs(case))
    M = np.empty((2 * P + 3, 2 * P + 3))
    record('schur/no_sums', lib.lrvb_glmm_schur(h, p(loc), p(sc), p(cl), G, p(M)))          # before any terms call on this context
    for name, entry in (('terms', terms), ('obs_influence', rows), ('group_influence', groups)):
        record(name + '/null', entry(mean=None))
        record(name + '/nodes_0', entry(nq=0))
        record(name + '/nodes_129', entry(nq=129))
        record(name + '/len_mean', entry(P_in=P + 1))
        record(name + '/len_e', entry(G_in=G + 1))
        record(name + '/var_not_positive', entry(var=bad_v))
        record(name + '/r_not_positive', entry(r_=bad_r))
    record('obs_influence/q_0', rows(Q_=0))
    record('group_influence/q_0', groups(Q_=0))
    record('obs_influence/window_low', rows(n0=-1))
    record('obs_influence/window_high', rows(n1=N + 1))
    assert terms() == hip.OK
    bad_loc = loc.copy()
    bad_loc[1] = [1.0, 2.0, 1.0]                                        # a11 a22 - a12^2 < 0
    record('schur/not_positive_definite', lib.lrvb_glmm_schur(h, p(bad_loc), p(sc), p(cl), G, p(M)))
    assert terms() == hip.OK
    cl3 = hip.as_f64(cl.reshape(G, 2, 3))
    record('slopes_schur_after_intercept_terms', lib.lrvb_glmm_slopes_schur(h, p(loc), p(sc), p(cl3), G, 1, p(M)))
    del fun
    # the other way round: the K-effect terms entry at K = 1, then the intercept's elimination
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=1))
    par.push_param(vb.GammaParam('tau0'))
    par.push_param(vb.UVNParamArray('u', shape=(G, 1)))
    fun = vb.LogisticGLMMSlopesObjective(par, b['x'], b['y'], np.ones((N, 1)), b['gid'], G, gh_deg=b['deg'], weights=b['w'])
    ctx = fun.ctx
    ctx.glmm_slopes_terms(m, v, e.reshape(G, 1), r.reshape(G, 1), fun.gh_x, fun.gh_w)
    record('schur_after_slopes_terms', ctx._lib.lrvb_glmm_schur(ctx._h, p(loc), p(sc), p(cl), G, p(M)))
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
            if arr.size <= mg.RAW_MAX:
                store[key] = arr
            else:
                store[key + ':shape'], store[key + ':sha256'] = np.array(arr.shape), np.array(mg.digest(arr))
    case = next(c for c in CASES if c['name'] == REFUSAL_CASE)
    for key, (status, text) in run_refusals(vb, case, build_case(case)).items():
        store['refusal/' + key + ':status'], store['refusal/' + key + ':text'] = np.array(status), np.array(text)
        print('%-45s %d  %s' % (key, status, text))
    np.savez(a.out, **store)
    print('wrote %s: %d entries, %d bytes' % (a.out, len(store), os.path.getsize(a.out)))


if __name__ == '__main__':
    main(sys.argv[1:])

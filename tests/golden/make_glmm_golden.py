"""Cases and recorder of tests/golden/glmm_walk_parent.npz: the outputs of the six K-effect mixed-model entries
(lrvb_glmm_{slopes,poisson}_{terms,obs_influence,group_influence}) as the commit BEFORE the merge of the two tile walks
 computed them on an MI355X.  tests/test_gpu_glmm_walk_golden.py asks the present build for the same bits.

Every case is rebuilt from its seed (`build_case`), so no inputs are stored -- only a digest of them, which the CPU companion
test compares.  Arrays of up to RAW_MAX doubles are stored raw, larger ones as shape + SHA-256 of their little-endian bytes.

Recording (once, from a build of the parent commit, in a process of its own; the library under test never writes the file):

    python tests/golden/make_glmm_golden.py --root <tree with the parent's liblrvb_hip.so> --commit <its hash> [--out FILE]

A second table, POLICY_CASES x POLICY_FAMILIES, records tests/golden/glmm_policies_parent.npz with `--table policies`: the
likelihood policies other than the logistic and the Poisson one (binomial with trials and an offset, probit, cloglog,
zero-truncated Poisson and NB2, Beta, Gamma, censored Gaussian) through their terms, row and group influence, predict and
dispersion entries, as the commit BEFORE the node loop and the lane reduction of k_glmm_walk.h were shared
computed them.  Same storage rules; tests/test_gpu_glmm_policies_golden.py asks the present build for the same bits.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, 'glmm_walk_parent.npz')
RAW_MAX = 2048
HYP = (1.3, 0.2, 0.7, 1.5, 0.8)
QS = (5, 21)                                                             # one block of 16 outputs; two (the nqb > 1 path)

# (N, P, K, G) and what the case is the smallest witness of (ISSUE of the merge)
CASES = [
    dict(name='degenerate', shape=(1, 1, 1, 1)),                         # the degenerate walk
    dict(name='cut_group', shape=(65, 5, 2, 3), deg=5),                  # second tile of one row, a group cut by the boundary; nq = 5
    dict(name='unit_design', shape=(37, 3, 1, 5), z_none=True, offset_none=True),   # K = 1; Poisson: z=None and offset=None
    dict(name='many_groups', shape=(200, 17, 3, 40), big_group=False),   # 4 K P = 204 < 256; 27 scalar columns
    dict(name='wrap', shape=(300, 17, 4, 7), zero_weights=True),         # 4 K P = 272: the second owned column partly populated
    dict(name='middle_tile', shape=(130, 64, 4, 2), sizes=(30, 100)),    # all four owned columns; group 1 covers the tile 64..127
]


def _import_refs():
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import glmm_poisson_reference as pref
    import glmm_slopes_reference as sref
    return pref, sref


def build_case(case):
    """dict of the inputs of one case: x, y_poisson, y_logistic, z (N x K, ones where the model is given z=None), w, gid, o
    (zeros where the model is given offset=None), eta (vector coordinates of the point), deg."""
    pref, sref = _import_refs()
    N, P, K, G = case['shape']
    x, y, z, w, gid, o, free = pref.problem(N, P, K, G, seed=N + P + K, big_group=case.get('big_group', True))
    rng = np.random.default_rng([N, P, K, G])
    if 'sizes' in case:                                                  # groups of the given sizes, rows in a shuffled order
        gid = np.repeat(np.arange(G), case['sizes']).astype(np.int32)[rng.permutation(N)]
    if case.get('zero_weights'):
        w = w.copy()
        w[gid == 2] = 0.0
        w[[0, 17, 64, N - 1]] = 0.0
    if case.get('offset_none'):
        o = np.zeros(N)
    eta = np.where(sref.positive_mask(P, K, G), np.exp(free), free)
    return dict(x=x, y_poisson=y, y_logistic=np.minimum(y, 1.0), z=z, w=w, gid=gid, o=o, eta=eta, deg=case.get('deg', 20))


def inputs_digest(b):
    h = hashlib.sha256()
    for k in ('x', 'y_poisson', 'y_logistic', 'z', 'w', 'o', 'eta'):
        h.update(np.ascontiguousarray(b[k], dtype='<f8').tobytes())
    h.update(np.ascontiguousarray(b['gid'], dtype='<i4').tobytes())
    return h.hexdigest()


def point(eta, P, K, G):
    ng = 2 * P + 4 * K
    return (eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G * K].reshape(G, K), 1.0 / eta[ng + G * K:].reshape(G, K))


def operand(case, Q):
    N, P, K, G = case['shape']
    return np.random.default_rng([N, P, K, G, Q]).normal(size=(Q, 2 * P + 2 * G * K))


def window(N):
    return (3, N - 2) if N > 5 else (0, N)


def run_case(vb, case, b):
    """{'<family>/<output>': array} of the six entries on the build `vb` was imported from."""
    N, P, K, G = case['shape']
    pt = point(b['eta'], P, K, G)
    z = None if case.get('z_none') else b['z']
    n0, n1 = window(N)
    out = {}
    for family in ('logistic', 'poisson'):
        par = vb.ModelParamsDict('params')
        par.push_param(vb.UVNParamVector('beta', length=P))
        par.push_param(vb.UVNParamVector('mu', length=K))
        for k in range(K):
            par.push_param(vb.GammaParam('tau%d' % k))
        par.push_param(vb.UVNParamArray('u', shape=(G, K)))
        kw = dict(beta_prior_info=HYP[0], mu_prior=HYP[1:3], tau_prior=HYP[3:5], weights=b['w'])
        if family == 'logistic':
            fun = vb.LogisticGLMMSlopesObjective(par, b['x'], b['y_logistic'], b['z'], b['gid'], G, gh_deg=b['deg'], **kw)   # takes no z=None
            gh = (fun.gh_x, fun.gh_w)
            terms, rows, groups = fun.ctx.glmm_slopes_terms, fun.ctx.glmm_slopes_obs_influence, fun.ctx.glmm_slopes_group_influence
        else:
            fun = vb.PoissonGLMMObjective(par, b['x'], b['y_poisson'], z, b['gid'], G,
                                          offset=None if case.get('offset_none') else b['o'], **kw)
            gh = ()
            terms, rows, groups = fun.ctx.glmm_poisson_terms, fun.ctx.glmm_poisson_obs_influence, fun.ctx.glmm_poisson_group_influence
        val, gg, Hb, gs = terms(*pt, *gh)
        out[family + '/value'], out[family + '/grad'], out[family + '/H_blocks'], out[family + '/group_sums'] = np.array([val]), gg, Hb, gs
        out[family + '/scalar_columns'] = terms(*pt, *gh, want_border=False)[3]           # the strided copy-out
        out[family + '/value_only'] = np.array([terms(*pt, *gh, want_grad=False, want_hess=False)[0]])
        for Q in QS:
            A = operand(case, Q)
            out['%s/obs_influence_q%d' % (family, Q)] = rows(*pt, *gh, A, n0, n1)
            out['%s/group_influence_q%d' % (family, Q)] = groups(*pt, *gh, A)
        del fun
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype='<f8').tobytes()).hexdigest()


def matches(fixture, key, a):
    """Bitwise: the raw array where the fixture holds one, shape and digest otherwise."""
    a = np.asarray(a, dtype=np.float64)
    if key in fixture:
        want = fixture[key]
        return want.shape == a.shape and want.tobytes() == np.ascontiguousarray(a, dtype='<f8').tobytes()
    return tuple(fixture[key + ':shape']) == a.shape and str(fixture[key + ':sha256']) == digest(a)


# ---- the second table: the likelihood policies ------------------------------------------------------------
POLICY_FIXTURE = os.path.join(HERE, 'glmm_policies_parent.npz')
N_NEW = 70                                                               # new rows of predict: a second tile of six rows
PREDICT_COLS = 5

# (N, P, K, G), the number of nodes, and what the case is the smallest witness of in the walk of a row over its four lanes
POLICY_CASES = [
    dict(name='one_node', shape=(1, 1, 1, 1), deg=1),                    # three of the four lanes own no node; 63 dead rows; the row is censored
    dict(name='cut_group', shape=(65, 5, 2, 3), deg=5, zero_weights=True, spread=5.0),   # lane 0 owns two nodes; a second tile of one
                                                                         # row; a group cut by the boundary; an empty group; zero weights
    dict(name='table_limit', shape=(37, 3, 1, 5), deg=128, spread=1.0),  # the node table full: 32 nodes per lane
    dict(name='all_columns', shape=(130, 64, 4, 2), deg=20, sizes=(30, 100), spread=2.0),   # P = 64: all four owned columns
]

# The objective class of a family, what its constructor takes from the case behind (par, x, y, z, gid, G), and which entries are
# recorded.  `negbin` is the binomial policy with trials y + phi: only its dispersion entry is a walk of its own.
POLICY_FAMILIES = [
    dict(name='binomial', cls='BinomialGLMMObjective', kw=('trials',), predict=True),
    dict(name='probit', cls='BinomialGLMMObjective', kw=('trials',), link='probit', predict=True),
    dict(name='cloglog', cls='BinomialGLMMObjective', kw=('trials',), link='cloglog', predict=True),
    dict(name='ztpoisson', cls='TruncatedPoissonGLMMObjective', predict=True),
    dict(name='ztnegbin', cls='TruncatedNegBinomialGLMMObjective', kw=('dispersion',), predict=True),
    dict(name='beta', cls='BetaGLMMObjective', kw=('dispersion',), dispersion=True),
    dict(name='gamma', cls='GammaGLMMObjective', kw=('dispersion',), dispersion=True, nodes=False),
    dict(name='censnormal', cls='CensoredNormalGLMMObjective', kw=('dispersion', 'censoring'), predict=True, dispersion=True),
    dict(name='negbin', cls='NegBinomialGLMMObjective', kw=('dispersion',), terms=False, dispersion=True),
]
TERMS_OUTPUTS = (['value', 'grad', 'H_blocks', 'group_sums', 'scalar_columns', 'value_only']
                 + ['%s_q%d' % (e, q) for e in ('obs_influence', 'group_influence') for q in QS])
PREDICT_OUTPUTS = ['predict_window', 'predict_new']
DISPERSION_OUTPUTS = ['dispersion_d', 'dispersion_cross_global', 'dispersion_cross_local']


def policy_outputs(fam):
    return ((TERMS_OUTPUTS if fam.get('terms', True) else []) + (PREDICT_OUTPUTS if fam.get('predict') else [])
            + (DISPERSION_OUTPUTS if fam.get('dispersion') else []))


def _policy_refs():
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import glmm_beta_reference as beta
    import glmm_binomial_reference as bref
    import glmm_censnormal_reference as cens
    import glmm_gamma_reference as gamma
    import glmm_link_reference as lref
    import glmm_slopes_reference as sref
    import glmm_ztnegbin_reference as ztnb
    import glmm_ztpoisson_reference as ztp
    return dict(beta=beta, bref=bref, cens=cens, gamma=gamma, lref=lref, sref=sref, ztnb=ztnb, ztp=ztp)


def build_policy_case(case):
    """dict of the inputs of one case.  x, z, w, gid and the point are those of `glmm_binomial_reference.problem` at the seed
    N + P + K; ONE offset for every family, that problem's plus a permutation of linspace(-spread, spread, N), so that the nodes
    reach the tails in which the node functions branch (`policy_coverage`); per family the responses and the per-row data of its
    own reference's `problem` at that seed (dispersions one value per row); the new rows of predict."""
    r = _policy_refs()
    N, P, K, G = case['shape']
    seed = N + P + K
    x, yb, z, w, gid, o, mb, free = r['bref'].problem(N, P, K, G, seed)
    rng = np.random.default_rng([N, P, K, G, 46])
    if 'sizes' in case:                                                  # groups of the given sizes, rows in a shuffled order
        gid = np.repeat(np.arange(G), case['sizes']).astype(np.int32)[rng.permutation(N)]
    if case.get('zero_weights'):
        w = w.copy()
        w[[0, 17, N - 1]] = 0.0
    if case.get('spread'):
        o = o + np.linspace(-case['spread'], case['spread'], N)[rng.permutation(N)]
    fam = {'binomial': dict(y=yb, trials=mb)}
    for link in ('probit', 'cloglog'):
        p = r['lref'].problem(N, P, K, G, seed, link)
        fam[link] = dict(y=p[1], trials=p[6])
    fam['ztpoisson'] = dict(y=r['ztp'].problem(N, P, K, G, seed)[1])
    p = r['ztnb'].problem(N, P, K, G, seed, phi='vector')
    fam['ztnegbin'] = dict(y=p[1], dispersion=p[6])
    p = r['beta'].problem(N, P, K, G, seed, phi='vector')
    fam['beta'] = dict(y=p[1], dispersion=p[6])
    p = r['gamma'].problem(N, P, K, G, seed, phi='vector')
    fam['gamma'] = dict(y=p[1], dispersion=p[6])
    p = r['cens'].problem(N, P, K, G, seed, phi='vector', mode='mixed')
    st = p[7].copy()
    if N < 3:
        st[0] = 1                                                        # the single row is censored
    fam['censnormal'] = dict(y=p[1], dispersion=p[6], censoring=st)
    p = r['bref'].nb_problem(N, P, K, G, seed, phi='vector')
    fam['negbin'] = dict(y=p[1], dispersion=p[6])
    rn = np.random.default_rng([N, P, K, G, 47])
    gn = rn.integers(0, G, size=N_NEW)
    gn[::9] = -1                                                         # the pseudo-group of a population-level row
    new = dict(x=rn.normal(size=(N_NEW, P)) / np.sqrt(P),
               z=np.concatenate([np.ones((N_NEW, 1)), 0.5 * rn.normal(size=(N_NEW, K - 1))], axis=1), groups=gn.astype(np.int32),
               offset=0.3 * rn.normal(size=N_NEW), trials=rn.integers(0, 13, size=N_NEW).astype(np.float64),
               dispersion=np.exp(rn.uniform(np.log(0.05), np.log(50.0), size=N_NEW)))
    eta = np.where(r['sref'].positive_mask(P, K, G), np.exp(free), free)
    return dict(x=x, z=z, w=w, gid=gid, o=o, eta=eta, deg=case['deg'], fam=fam, new=new)


def policy_inputs_digest(b):
    h = hashlib.sha256()
    for k in ('x', 'z', 'w', 'o', 'eta'):
        h.update(np.ascontiguousarray(b[k], dtype='<f8').tobytes())
    h.update(np.ascontiguousarray(b['gid'], dtype='<i4').tobytes())
    for f in POLICY_FAMILIES:
        for k in ('y',) + f.get('kw', ()):
            h.update(np.ascontiguousarray(b['fam'][f['name']][k], dtype='<f8').tobytes())
    for k in ('x', 'z', 'offset', 'trials', 'dispersion'):
        h.update(np.ascontiguousarray(b['new'][k], dtype='<f8').tobytes())
    h.update(np.ascontiguousarray(b['new']['groups'], dtype='<i4').tobytes())
    return h.hexdigest()


def policy_rows(case, b):
    """(rho, s) of every row at the point of the case, rho including the offset."""
    N, P, K, G = case['shape']
    m, v, e, r = point(b['eta'], P, K, G)
    return b['o'] + b['x'] @ m + (b['z'] * e[b['gid']]).sum(1), (b['x'] * b['x']) @ v + (b['z'] * b['z'] * r[b['gid']]).sum(1)


def policy_coverage(case, b):
    """Which branches of the node functions the nodes of this case take, by the host forms of the policies: the probit continued
    fraction below t = -5 (by a success or, at -t, by a failure), the cloglog and zero-truncated Poisson select past u = 700 and
    the log1p form of the cloglog value past u = log 2, the NB2 corner eta < log 1e-3 with v < 0.01 (and a node outside it), the
    continued fraction on a censored row, and whether the first tile of group-sorted rows holds neighbours of all three statuses."""
    from lrvb_amd import glmm_binomial as gb
    from lrvb_amd import glmm_hurdle as gh
    rho, s = policy_rows(case, b)
    t = gb._nodes(rho, s, *np.polynomial.hermite.hermgauss(b['deg']))[0]
    with np.errstate(over='ignore'):
        u = np.exp(t)
    phi = b['fam']['ztnegbin']['dispersion'][:, None]
    eta = t - np.log(phi)
    corner = (eta < gh.ZTNB_ETA_SMALL) & (phi * gh._logistic_node(eta)[0] < gh.ZTNB_V_SMALL)
    c = b['fam']['censnormal']
    st = np.asarray(c['censoring'], dtype=np.float64)
    a = (st * np.sqrt(c['dispersion']))[:, None] * (t - c['y'][:, None])
    tile = st[np.argsort(b['gid'], kind='stable')][:GLMM_TILE]
    return dict(probit_cf=bool(np.any(t < gb.PROBIT_CF_BELOW) and np.any(-t < gb.PROBIT_CF_BELOW)), probit_plain=bool(np.any(np.abs(t) < 5.0)),
                select_700=bool(np.any(u > 700.0)), cloglog_log1p=bool(np.any((u > gb.LOG2) & (u <= 700.0))), cloglog_log=bool(np.any(u <= gb.LOG2)),
                ztnb_corner=bool(np.any(corner)), ztnb_factored=bool(np.any(~corner)),
                censored_cf=bool(np.any(a[st != 0.0] < gb.PROBIT_CF_BELOW)),
                statuses_mixed=bool(set(tile) == {-1.0, 0.0, 1.0} and np.any(tile[1:] != tile[:-1])))


GLMM_TILE = 64
COVERAGE = ('probit_cf', 'probit_plain', 'select_700', 'cloglog_log1p', 'cloglog_log', 'ztnb_corner', 'ztnb_factored', 'censored_cf',
            'statuses_mixed')


def coverage_of_all_cases():
    """Every branch is taken by a node of at least one case."""
    got = [policy_coverage(c, build_policy_case(c)) for c in POLICY_CASES]
    return {k: any(g[k] for g in got) for k in COVERAGE}


def policy_objective(vb, case, b, fam):
    N, P, K, G = case['shape']
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParamVector('mu', length=K))
    for k in range(K):
        par.push_param(vb.GammaParam('tau%d' % k))
    par.push_param(vb.UVNParamArray('u', shape=(G, K)))
    d = b['fam'][fam['name']]
    kw = dict(beta_prior_info=HYP[0], mu_prior=HYP[1:3], tau_prior=HYP[3:5], weights=b['w'], offset=b['o'])
    kw.update({k: d[k] for k in fam.get('kw', ())})
    if fam.get('nodes', True):
        kw['gh_deg'] = b['deg']
    if 'link' in fam:
        kw['link'] = fam['link']
    return getattr(vb, fam['cls'])(par, b['x'], d['y'], b['z'], b['gid'], G, **kw)


def policy_new_rows(fam, b):
    new = {k: b['new'][k] for k in ('x', 'z', 'groups', 'offset')}
    if 'trials' in fam.get('kw', ()):
        new['trials'] = b['new']['trials']
    if fam['name'] == 'ztnegbin':
        new['dispersion'] = b['new']['dispersion']
    return new


def run_policy_case(vb, case, b):
    """{'<family>/<output>': array} on the build `vb` was imported from, through the device hooks of the objective classes.  The
    predict entries read a group covariance that the case does not need to be positive definite for: after the full terms call
    the local factor is built from blocks 1000 I (lrvb_glmm_slopes_schur) and the covariance from W = cov_beta = I / 20."""
    N, P, K, G = case['shape']
    n0, n1 = window(N)
    eta = b['eta']
    out = {}
    for fam in POLICY_FAMILIES:
        name = fam['name']
        fun = policy_objective(vb, case, b, fam)
        pt = fun._point(eta)
        if fam.get('terms', True):
            val, gg, Hb, gs = fun._terms(*pt)
            out[name + '/value'], out[name + '/grad'], out[name + '/H_blocks'], out[name + '/group_sums'] = np.array([val]), gg, Hb, gs
            out[name + '/scalar_columns'] = fun._terms(*pt, want_border=False)[3]
            out[name + '/value_only'] = np.array([fun._terms(*pt, want_grad=False, want_hess=False)[0]])
            for Q in QS:
                A = operand(case, Q)
                out['%s/obs_influence_q%d' % (name, Q)] = fun._obs_influence(*pt, A, n0=n0, n1=n1)
                out['%s/group_influence_q%d' % (name, Q)] = fun._group_influence(*pt, A)
        if fam.get('dispersion'):
            d, cg, cl = fun._dispersion_entry(pt)
            out[name + '/dispersion_d'], out[name + '/dispersion_cross_global'], out[name + '/dispersion_cross_local'] = d, cg, cl
        if fam.get('predict'):
            fun._terms(*pt)                                              # the group sums with their border, resident
            R = 2 * P + 3 * K
            iu = np.triu_indices(2 * K)
            fun.ctx.glmm_slopes_schur(np.tile((1e3 * np.eye(2 * K))[iu], (G, 1)), np.ones((G, 2 * K)), np.zeros((G, 2 * K, 3)))
            fun.ctx.glmm_slopes_group_cov(0.05 * np.eye(R), np.ones(R), G, K)
            m, v, e, r = pt[:4]
            e2 = np.vstack([e, eta[2 * P:2 * P + K][None, :]])
            r2 = np.vstack([r, 1.0 / eta[2 * P + K:2 * P + 2 * K][None, :]])
            p2, cov = (m, v, e2, r2) + tuple(pt[4:]), 0.05 * np.eye(P)
            out[name + '/predict_window'] = fun._predict_entry(p2, cov, (n0, n1), None)
            out[name + '/predict_new'] = fun._predict_entry(p2, cov, None, fun._predict_rows_of(policy_new_rows(fam, b), 0, None))
        del fun
    return out


TABLES = {'walk': lambda: (FIXTURE, CASES, build_case, inputs_digest, run_case),
          'policies': lambda: (POLICY_FIXTURE, POLICY_CASES, build_policy_case, policy_inputs_digest, run_policy_case)}


def main(argv):
    import argparse
    import subprocess
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--root', required=True, help='the tree whose build is recorded (it holds lrvb_amd.py and the built library)')
    ap.add_argument('--commit', required=True, help='the commit hash of that tree')
    ap.add_argument('--table', choices=sorted(TABLES), default='walk')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    fixture, cases, build_case, inputs_digest, run_case = TABLES[a.table]()
    a.out = a.out or fixture
    sys.path.insert(0, os.path.abspath(a.root))
    import lrvb_amd as vb
    assert os.path.dirname(os.path.abspath(vb.__file__)).startswith(os.path.abspath(a.root)), vb.__file__
    assert vb._hip.device_count() >= 1, 'no HIP device visible'
    if a.table == 'policies':
        cov = coverage_of_all_cases()
        assert all(cov.values()), cov
    store = {'parent_commit': np.array(a.commit),
             'hipcc_version': np.array(subprocess.run(['hipcc', '--version'], capture_output=True, text=True, check=True).stdout.strip())}
    for case in cases:
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
    np.savez(a.out, **store)
    print('wrote %s: %d entries, %d bytes' % (a.out, len(store), os.path.getsize(a.out)))


if __name__ == '__main__':
    main(sys.argv[1:])

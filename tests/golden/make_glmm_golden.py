"""Cases and recorder of tests/golden/glmm_walk_parent.npz: the outputs of the six K-effect mixed-model entries
(lrvb_glmm_{slopes,poisson}_{terms,obs_influence,group_influence}) as the commit BEFORE the merge of the two tile walks
 computed them on an MI355X.  tests/test_gpu_glmm_walk_golden.py asks the present build for the same bits.

Every case is rebuilt from its seed (`build_case`), so no inputs are stored -- only a digest of them, which the CPU companion
test compares.  Arrays of up to RAW_MAX doubles are stored raw, larger ones as shape + SHA-256 of their little-endian bytes.

Recording (once, from a build of the parent commit, in a process of its own; the library under test never writes the file):

    python tests/golden/make_glmm_golden.py --root <tree with the parent's liblrvb_hip.so> --commit <its hash> [--out FILE]
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
    np.savez(a.out, **store)
    print('wrote %s: %d entries, %d bytes' % (a.out, len(store), os.path.getsize(a.out)))


if __name__ == '__main__':
    main(sys.argv[1:])

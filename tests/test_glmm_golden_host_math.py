"""tests/golden/glmm_walk_parent.npz and tests/golden/glmm_intercept_parent.npz without a GPU: the fixture loads and names the commit it was recorded from, its cases
rebuild from their seeds to the inputs it was recorded with and are the witnesses they are meant to be, and the recorded values
and gradients of both models agree with the torch references (tests/glmm_slopes_reference.py, tests/glmm_poisson_reference.py)
to the tolerances of `_check_against_reference` in the GPU tests: value 1e-11, gradient 1e-10 relative.  So a fixture recorded from
a broken build does not pass for the truth that tests/test_gpu_glmm_walk_golden.py compares against bit for bit.  The intercept
fixture is checked the same way against tests/glmm_reference.py, at the same tolerances; what it holds raw
of the Hessian pieces at the 1e-9 of tests/test_gpu_glmm.py.  tests/golden/glmm_solve_predict_parent.npz: the
inputs digests, how many cases hold each output raw, and the raw solves and predict columns against a dense solve and a dense
inverse of the torch reference Hessians of the four families."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_glmm_golden as mg                                           # noqa: E402
import make_glmm_intercept_golden as ig                                  # noqa: E402
import glmm_reference as gref                                            # noqa: E402
import glmm_poisson_reference as pref                                    # noqa: E402
import glmm_slopes_reference as sref                                     # noqa: E402
from helpers import rel_err                                              # noqa: E402

IDS = [c['name'] for c in mg.CASES]


@pytest.fixture(scope='module')
def fixture():
    with np.load(mg.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_fixture_names_its_parent_and_is_complete(fixture):
    assert os.path.getsize(mg.FIXTURE) < 256 * 1024
    assert re.fullmatch(r'[0-9a-f]{40}', str(fixture['parent_commit']))
    assert 'HIP version' in str(fixture['hipcc_version'])
    outputs = ['value', 'grad', 'H_blocks', 'group_sums', 'scalar_columns', 'value_only']
    outputs += ['%s_q%d' % (e, q) for e in ('obs_influence', 'group_influence') for q in mg.QS]
    for case in mg.CASES:
        N, P, K, G = case['shape']
        for family in ('logistic', 'poisson'):
            for name in outputs:
                key = '%s/%s/%s' % (case['name'], family, name)
                raw = key in fixture
                assert raw != (key + ':sha256' in fixture and key + ':shape' in fixture), key
                if raw:
                    assert fixture[key].size <= mg.RAW_MAX and np.all(np.isfinite(fixture[key]))
                else:
                    assert np.prod(fixture[key + ':shape']) > mg.RAW_MAX
            head = '%s/%s/' % (case['name'], family)
            assert fixture[head + 'value'].tobytes() == fixture[head + 'value_only'].tobytes()
            assert fixture[head + 'grad'].shape == (2 * P,)
            assert fixture[head + 'scalar_columns'].shape == (G, 2 * K + K * (2 * K + 1))


@pytest.mark.parametrize('case', mg.CASES, ids=IDS)
def test_cases_rebuild_from_their_seeds(fixture, case):
    a, b = mg.build_case(case), mg.build_case(case)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert mg.inputs_digest(a) == str(fixture[case['name'] + ':inputs'])


def test_cases_are_the_witnesses_they_are_meant_to_be():
    built = {c['name']: (c, mg.build_case(c)) for c in mg.CASES}
    sizes = lambda name: np.bincount(built[name][1]['gid'], minlength=built[name][0]['shape'][3])
    assert [c['shape'] for c in mg.CASES] == [(1, 1, 1, 1), (65, 5, 2, 3), (37, 3, 1, 5), (200, 17, 3, 40), (300, 17, 4, 7), (130, 64, 4, 2)]
    s = sizes('cut_group')                                               # group 1 is cut by the boundary at row 64; group 2 is empty
    assert s[0] < 64 < s[0] + s[1] and s[2] == 0 and built['cut_group'][1]['deg'] == 5
    assert built['unit_design'][0]['z_none'] and np.all(built['unit_design'][1]['z'] == 1.0)
    assert np.all(built['unit_design'][1]['o'] == 0.0) and built['unit_design'][0]['offset_none']
    s = sizes('many_groups')
    end = np.cumsum(s)                                                   # sorted rows: group g is [end - s, end)
    assert np.sum((s > 0) & ((end - s) // 64 == (end - 1) // 64)) > 30 and s[-1] == 0        # most groups whole inside a tile
    assert np.sum(built['wrap'][1]['w'] == 0.0) > 4 and np.all(built['wrap'][1]['w'][built['wrap'][1]['gid'] == 2] == 0.0)
    s = sizes('middle_tile')                                             # group 1 holds every row of the tile 64 .. 127
    assert s[0] <= 64 and s[0] + s[1] >= 128
    for name, (c, b) in built.items():
        if not c.get('offset_none'):
            assert np.any(b['o'] != 0.0)
        assert b['deg'] == (5 if name == 'cut_group' else 20)
    assert mg.QS == (5, 21) and mg.window(65) == (3, 63) and mg.window(1) == (0, 1)


@pytest.mark.parametrize('case', mg.CASES, ids=IDS)
def test_recorded_values_and_gradients_agree_with_the_references(fixture, case):
    N, P, K, G = case['shape']
    b = mg.build_case(case)
    want = {'logistic': sref.data_pieces(b['x'], b['y_logistic'], b['z'], b['w'], b['gid'], G, b['eta'], gh_deg=b['deg']),
            'poisson': pref.data_pieces(b['x'], b['y_poisson'], b['z'], b['w'], b['o'], b['gid'], G, b['eta'])}
    for family, ref in want.items():
        head = '%s/%s/' % (case['name'], family)
        val = float(fixture[head + 'value'][0])
        e = [abs(val - ref['value']) / abs(ref['value']), rel_err(fixture[head + 'grad'], ref['g_glob']),
             rel_err(fixture[head + 'scalar_columns'][:, :2 * K], ref['g_loc'])]
        print(case['name'], family, e)
        assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-10


# ---- tests/golden/glmm_intercept_parent.npz: the random-intercept entries ---------------------------------
I_IDS = [c['name'] for c in ig.CASES]
I_OUTPUTS = (['value', 'grad', 'grad_local', 'H_blocks', 'border', 'local', 'schur', 'no_border/value', 'no_border/grad',
              'no_border/grad_local', 'no_border/H_blocks', 'no_border/local', 'no_border/schur', 'value_only']
             + ['%s_q%d' % (e, q) for e in ('obs_influence', 'group_influence') for q in ig.QS])


@pytest.fixture(scope='module')
def ifixture():
    with np.load(ig.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_intercept_fixture_names_its_parent_and_is_complete(ifixture):
    assert os.path.getsize(ig.FIXTURE) < 256 * 1024
    assert re.fullmatch(r'[0-9a-f]{40}', str(ifixture['parent_commit']))
    assert 'HIP version' in str(ifixture['hipcc_version'])
    for case in ig.CASES:
        N, P, G = case['shape']
        head = case['name'] + '/'
        for name in I_OUTPUTS:
            key = head + name
            raw = key in ifixture
            assert raw != (key + ':sha256' in ifixture and key + ':shape' in ifixture), key
            if raw:
                assert ifixture[key].size <= mg.RAW_MAX and np.all(np.isfinite(ifixture[key]))
            else:
                assert np.prod(ifixture[key + ':shape']) > mg.RAW_MAX
        # the three terms calls agree on what they share: the border is a matter of the copy-out only
        for name in ('value', 'grad', 'grad_local', 'H_blocks', 'local', 'schur'):
            one, other = head + name, head + 'no_border/' + name
            if one in ifixture:
                assert ifixture[one].tobytes() == ifixture[other].tobytes(), one
            else:
                assert str(ifixture[one + ':sha256']) == str(ifixture[other + ':sha256']), one
        assert ifixture[head + 'value'].tobytes() == ifixture[head + 'value_only'].tobytes()
        assert ifixture[head + 'grad'].shape == (2 * P,) and ifixture[head + 'grad_local'].shape == (G, 2)
        assert ifixture[head + 'local'].shape == (G, 3)
    refusals = [k for k in ifixture if k.startswith('refusal/') and k.endswith(':status')]
    assert len(refusals) == 29 and all(int(ifixture[k]) < 0 and str(ifixture[k[:-len('status')] + 'text']) for k in refusals)
    text = lambda k: str(ifixture['refusal/' + k + ':text'])
    assert text('slopes_schur_after_intercept_terms') == 'no group sums of 1 effects resident: call lrvb_glmm_slopes_terms first'
    assert text('schur_after_slopes_terms') == text('schur/no_sums') == 'no group sums resident: call lrvb_glmm_terms first'
    assert text('terms/len_e') == 'Wrong size for e / r.  Expected 5, got 6'


@pytest.mark.parametrize('case', ig.CASES, ids=I_IDS)
def test_intercept_cases_rebuild_from_their_seeds(ifixture, case):
    a, b = ig.build_case(case), ig.build_case(case)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert ig.inputs_digest(a) == str(ifixture[case['name'] + ':inputs'])


def test_intercept_cases_are_the_witnesses_they_are_meant_to_be():
    built = {c['name']: (c, ig.build_case(c)) for c in ig.CASES}
    sizes = lambda name: np.bincount(built[name][1]['gid'], minlength=built[name][0]['shape'][2])
    assert [c['shape'] for c in ig.CASES] == [(1, 1, 1), (65, 5, 3), (37, 3, 5), (200, 17, 40), (300, 63, 7), (130, 64, 2)]
    s = sizes('cut_group')                                               # group 1 is cut by the boundary at row 64 (partial slot 1 of tile 0,
    assert 0 < s[0] < 64 < s[0] + s[1] and s[2] == 0                     # slot 0 of tile 1); group 2 is empty
    s = sizes('many_groups')
    end = np.cumsum(s)                                                   # sorted rows: group g is [end - s, end)
    assert np.sum((s > 0) & ((end - s) // 64 == (end - 1) // 64)) > 30 and s[-1] == 0        # most groups whole inside a tile
    w, gid = built['odd_p'][1]['w'], built['odd_p'][1]['gid']
    assert np.all(w[gid == 2] == 0.0) and np.sum(gid == 2) > 0 and np.sum(w == 0.0) > np.sum(gid == 2)   # a whole group and single rows
    assert 4 * 63 == 252 < 256 and 63 % 4 == 3                           # threads 252..255 own no column; the last k-step is padded
    s = sizes('middle_tile')                                             # group 1 holds every row of the tile 64 .. 127: three pieces
    assert tuple(s) == (30, 100) and 4 * 64 == 256
    for name, (c, b) in built.items():
        assert b['deg'] == (5 if name == 'cut_group' else 20)
    assert ig.QS == (5, 21) and ig.REFUSAL_CASE in built


@pytest.mark.parametrize('case', ig.CASES, ids=I_IDS)
def test_intercept_recorded_outputs_agree_with_the_reference(ifixture, case):
    N, P, G = case['shape']
    b = ig.build_case(case)
    ref = gref.data_pieces(b['x'], b['y'], b['w'], b['gid'], G, b['eta'], gh_deg=b['deg'])
    head = case['name'] + '/'
    val = float(ifixture[head + 'value'][0])
    e = [abs(val - ref['value']) / abs(ref['value']), rel_err(ifixture[head + 'grad'], ref['g_glob']),
         rel_err(ifixture[head + 'grad_local'], ref['g_loc'])]
    print(case['name'], e)
    assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-10
    for name, want in (('H_blocks', ref['Hb']), ('border', ref['border']), ('local', ref['loc'])):
        if head + name in ifixture:                                      # stored raw
            e2 = rel_err(ifixture[head + name], want)
            print(case['name'], name, e2)
            assert e2 < 1e-9
        else:
            assert tuple(ifixture[head + name + ':shape']) == want.shape


# ---- tests/golden/glmm_solve_predict_parent.npz: the device-resident solve, the group covariance and predict --
import make_glmm_solve_predict_golden as sp                              # noqa: E402
import glmm_binomial_reference as bref                                   # noqa: E402

S_IDS = [c['name'] for c in sp.CASES]
S_OUTPUTS = (['schur', 'group_cov', 'predict_window', 'predict_new']
             + ['%s_q%d' % (e, q) for e in ('solve_forward', 'solve_back') for q in sp.SOLVE_QS])
S_BINOMIAL = ['value', 'grad', 'H_blocks', 'group_sums'] + ['%s_q%d' % (e, q) for e in ('obs_influence', 'group_influence') for q in sp.INFL_QS]
U53 = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope='module')
def sfixture():
    with np.load(sp.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def _raw_count(fx, name):
    return sum(('%s/%s/%s' % (c['name'], fam, name)) in fx for c in sp.CASES for fam in sp.FAMILIES) // len(sp.FAMILIES)


def test_solve_predict_fixture_names_its_parent_and_is_complete(sfixture):
    assert os.path.getsize(sp.FIXTURE) < 1024 * 1024
    assert re.fullmatch(r'[0-9a-f]{40}', str(sfixture['parent_commit']))
    assert 'HIP version' in str(sfixture['hipcc_version'])
    assert sp.CASES is mg.CASES and sp.RAW_MAX == mg.RAW_MAX == 2048 and sp.SOLVE_QS == (1, 70, 129)
    for case in sp.CASES:
        N, P, K, G = case['shape']
        R = 2 * P + 3 * K
        n0, n1 = mg.window(N)
        for fam in sp.FAMILIES:
            head = '%s/%s/' % (case['name'], fam)
            for name in S_OUTPUTS + (S_BINOMIAL if fam == 'binomial' else []):
                key = head + name
                raw = key in sfixture
                assert raw != (key + ':sha256' in sfixture and key + ':shape' in sfixture), key
                if raw:
                    assert sfixture[key].size <= mg.RAW_MAX and np.all(np.isfinite(sfixture[key]))
                else:
                    assert np.prod(sfixture[key + ':shape']) > mg.RAW_MAX
            assert sfixture[head + 'predict_window'].shape == (5, n1 - n0) and sfixture[head + 'predict_new'].shape == (5, sp.N_NEW)
            assert sfixture[head + 'solve_forward_q1'].shape == (R, 1) and sfixture[head + 'solve_back_q1'].shape == (G, 2 * K, 1)
    # So that the checks below are not hollow, every kind is held raw in at least three of the six cases, for every Q it has -- but
    # for ONE: the forward pass at Q = 129 is (2 P + 3 K) x 129 doubles, 645 and 1161 in the two smallest cases and 2064 = RAW_MAX + 16
    # in the third (P = 5, K = 2), so it is raw in two.  The counts, by the shapes:
    assert [_raw_count(sfixture, 'solve_back_q%d' % q) for q in sp.SOLVE_QS] == [6, 4, 3]          # G 2 K Q
    assert [_raw_count(sfixture, 'solve_forward_q%d' % q) for q in sp.SOLVE_QS] == [6, 3, 2]       # (2 P + 3 K) Q
    assert _raw_count(sfixture, 'group_cov') == 5                                                   # (G + 1) (K K + K P)
    assert _raw_count(sfixture, 'predict_window') == _raw_count(sfixture, 'predict_new') == 6       # 5 n, n <= 300
    refusals = [k for k in sfixture if k.startswith('refusal/') and k.endswith(':status')]
    assert len(refusals) == sp.N_REFUSALS and all(int(sfixture[k]) < 0 and str(sfixture[k[:-len('status')] + 'text']) for k in refusals)
    text = lambda k: str(sfixture['refusal/' + k + ':text'])
    assert text('solve_forward_k1_after_intercept_schur') == 'no factor of 1 effects resident: call lrvb_glmm_slopes_schur first'
    assert text('solve_back/no_forward') == 'no forward pass resident: call lrvb_glmm_slopes_solve_forward first'
    assert text('schur/not_positive_definite') == 'a local block of the logistic mixed model with slopes is not positive definite'
    assert text('predict/no_group_cov') == 'no group covariance of 2 effects resident: call lrvb_glmm_slopes_group_cov first'


@pytest.mark.parametrize('case', sp.CASES, ids=S_IDS)
def test_solve_predict_cases_rebuild_from_their_seeds(sfixture, case):
    a, b = sp.build_case(case), sp.build_case(case)
    assert sp.inputs_digest(a) == sp.inputs_digest(b) == str(sfixture[case['name'] + ':inputs'])
    N, P, K, G = case['shape']
    assert np.any(a['new']['groups'] == -1) and np.all(a['new']['groups'] < G) and np.any(a['trials'] != 1.0) and np.any(a['o_binomial'] != 0.0)


_href = {}


def _reference_hessian(case, b, fam):
    """The dense Hessian of the torch reference in free coordinates at the point of the case, computed once."""
    key = (case['name'], fam)
    if key not in _href:
        N, P, K, G = case['shape']
        x, z, w, gid = b['x'], b['z'], b['w'], b['gid']
        if fam == 'logistic':
            t = sref.tensors(x, b['y_logistic'], z, w, gid, mg.HYP)
            f, args = sref.kl_free, t[:5] + (G, t[5], b['deg'])
        elif fam == 'poisson':
            f, args = pref.kl_free, pref.targs(x, b['y_poisson'], z, w, b['o_poisson'], gid, G, mg.HYP)
        elif fam == 'binomial':
            f, args = bref.kl_free, bref.targs(x, b['y_binomial'], z, w, b['o_binomial'], b['trials'], gid, G, mg.HYP)
        else:
            f, args = bref.nb_kl_free, bref.targs(x, b['y_negbinomial'], z, w, b['o_binomial'], b['phi'], gid, G, mg.HYP)
        deg, bref.GH_DEG = bref.GH_DEG, b['deg']                          # the binomial reference reads its node count from the module
        try:
            H = gref.value_grad_hess(f, b['free'], args)[2]
        finally:
            bref.GH_DEG = deg
        np.linalg.cholesky(H)                                            # the point of the case: positive definite in every family
        _href[key] = (H, float(np.linalg.cond(H)))
    return _href[key]


def _fro(a):
    return np.sqrt(np.sum(np.square(np.asarray(a, dtype=LD))))


def _backward_error(H, X, R):
    """tests/test_gpu_glmm_slopes_device_solve.py::_backward_error: ||R - H X||_F / (||H||_F ||X||_F + ||R||_F) in longdouble."""
    Hl, Xl, Rl = (np.asarray(a, dtype=LD).reshape(a.shape[0], -1) for a in (H, X, R))
    return float(_fro(Rl - Hl @ Xl) / (_fro(Hl) * _fro(Xl) + _fro(Rl)))


@pytest.mark.parametrize('case', sp.CASES, ids=S_IDS)
def test_recorded_solves_agree_with_block_arrow_solve(sfixture, case):
    """The raw solve outputs against the host route, `block_arrow_solve` on the blocks of the reference Hessian, by the rules of
    tests/test_gpu_glmm_slopes_device_solve.py: eta_dev <= 8 eta_host + D 2^-53 and ||X_dev - X_host||_F <= 2 kappa_2(H)
    (eta_dev + eta_host) ||X_host||_F.  The fixture holds the local rows of X only, so its own backward error cannot be formed; the
    forward bound is taken with the largest eta_dev the first rule admits, 2 kappa (9 eta_host + D 2^-53), eta_host measured in
    longdouble.  The forward pass (H_xl H_ll^-1 R_l) / s is held to the same rule on the local system (kappa_2(H_ll), the measured
    backward error of the host's H_ll^-1 R_l, D_l = 2 G K), plus D_l 2^-53 for the product, relative to ||H_xl / s||_F ||H_ll^-1 R_l||_F."""
    from lrvb_amd.block_arrow import _from_groups, _local_index, block_arrow_solve
    from lrvb_amd.glmm_slopes import coupled_rows
    N, P, K, G = case['shape']
    b = sp.build_case(case)
    ng, rows = 2 * P + 4 * K, coupled_rows(P, K)
    eta = sp.eta_of(b, P, K, G)
    # Hx[r, l] = s_r C_g[l, r]: the device holds the border in the coordinates (mean, var, e_mu, a, b)
    s = np.concatenate([np.ones(P), -1.0 / eta[P:2 * P], np.stack([np.ones(K), eta[ng - 2 * K:ng:2], eta[ng - 2 * K + 1:ng:2]], axis=1).ravel()])
    li = ng + _local_index(G, K)
    seen = 0
    for fam in sp.FAMILIES:
        H, kappa = _reference_hessian(case, b, fam)
        D, Dl = H.shape[0], H.shape[0] - ng
        Hgg, Hx, Hll = H[:ng, :ng], H[rows][:, ng:], H[ng:, ng:]
        loc = H[li[:, :, None], li[:, None, :]]
        kl = float(np.linalg.cond(Hll))
        for Q in sp.SOLVE_QS:
            head = '%s/%s/' % (case['name'], fam)
            Rhs = b['rhs'][Q]
            if head + 'solve_back_q%d' % Q in sfixture:
                Xh = block_arrow_solve(Hgg, rows, Hx, loc, Rhs)
                e_host = _backward_error(H, Xh, Rhs)
                got = _from_groups(sfixture[head + 'solve_back_q%d' % Q], G, K)
                err, bound = float(_fro(got - Xh[ng:]) / _fro(Xh)), 2.0 * kappa * (9.0 * e_host + D * U53)
                print(case['name'], fam, Q, 'back: err %.3e, eta_host %.3e, kappa %.3e, bound %.3e' % (err, e_host, kappa, bound))
                assert err <= bound
                seen += 1
            if head + 'solve_forward_q%d' % Q in sfixture:
                tl = block_arrow_solve(Hgg, rows, Hx, loc, np.vstack([np.zeros((ng, Q)), Rhs[ng:]]), schur_solve=lambda r: np.zeros_like(r))[ng:]
                e_l = _backward_error(Hll, tl, Rhs[ng:])
                Hs = Hx / s[:, None]
                err = float(_fro(sfixture[head + 'solve_forward_q%d' % Q] - Hs @ tl) / (_fro(Hs) * _fro(tl)))
                bound = 2.0 * kl * (9.0 * e_l + Dl * U53) + Dl * U53
                print(case['name'], fam, Q, 'forward: err %.3e, eta_host %.3e, kappa_l %.3e, bound %.3e' % (err, e_l, kl, bound))
                assert err <= bound
                seen += 1
    assert seen >= 4 * 2                                                 # Q = 1 is raw in every case


def _gh_mean(kind, rho, s, trials, gh_x, gh_w, mp=False):
    """tests/test_gpu_glmm_predict.py::_gh_mean: the response-scale mean by the rule of the kernels."""
    import mpmath
    if not mp:
        if kind in ('poisson', 'negbinomial'):
            return np.exp(rho + 0.5 * s)
        t = rho[:, None] + np.sqrt(np.maximum(s, 0.0))[:, None] * (np.sqrt(2.0) * gh_x)[None, :]
        p = ((1.0 / (1.0 + np.exp(-t))) * (gh_w / np.sqrt(np.pi))[None, :]).sum(1)
        return p if trials is None else trials * p
    mpmath.mp.dps = 40
    out = []
    for i in range(rho.size):
        rh, sv = mpmath.mpf(float(rho[i])), mpmath.mpf(float(s[i]))
        if kind in ('poisson', 'negbinomial'):
            out.append(mpmath.exp(rh + sv / 2))
            continue
        sd = mpmath.sqrt(max(sv, 0))
        p = sum(mpmath.mpf(float(wk)) / (1 + mpmath.exp(-(rh + sd * mpmath.sqrt(2) * mpmath.mpf(float(xk))))) for xk, wk in zip(gh_x, gh_w))
        p = p / mpmath.sqrt(mpmath.pi)
        out.append(p if trials is None else p * mpmath.mpf(float(trials[i])))
    return out


@pytest.mark.parametrize('case', sp.CASES, ids=S_IDS)
def test_recorded_predictions_agree_with_the_dense_inverse(sfixture, case):
    """The raw predict columns against `block_arrow.predict_rows` with the blocks of a dense inverse, by the rules of
    tests/test_gpu_glmm_predict.py: rho and var_mf within (P + K + 2) 2^-53 of the sum of the absolute values of their terms,
    var_lrvb by the two-route rule err <= 8 err_host + kappa_2(H) D 2^-53 (err_host: the float64 inverse; both against the inverse
    refined by one Newton step in longdouble), the two means against the float64 restatement of the quadrature on the recorded
    rho and variances within 8 x that restatement's own error against mpmath (floor 16 x 2^-53), on the first eight rows."""
    import mpmath
    from lrvb_amd.block_arrow import predict_rows
    N, P, K, G = case['shape']
    b = sp.build_case(case)
    ng, GK = 2 * P + 4 * K, G * K
    eta = sp.eta_of(b, P, K, G)
    m, v = eta[:P], 1.0 / eta[P:2 * P]
    e2 = np.vstack([eta[ng:ng + GK].reshape(G, K), eta[2 * P:2 * P + K][None, :]])
    r2 = np.vstack([1.0 / eta[ng + GK:].reshape(G, K), 1.0 / eta[2 * P + K:2 * P + 2 * K][None, :]])
    gh_x, gh_w = np.polynomial.hermite.hermgauss(b['deg'])
    n0, n1 = mg.window(N)
    ie = np.vstack([ng + np.arange(GK).reshape(G, K), 2 * P + np.arange(K)[None, :]])       # the e rows of every group, then e_mu
    for fam in sp.FAMILIES:
        H, kappa = _reference_hessian(case, b, fam)
        Hinv = np.linalg.inv(H)
        Hl, X0 = H.astype(LD), Hinv.astype(LD)
        Hinv_ld = X0 + X0 @ (np.eye(H.shape[0], dtype=LD) - Hl @ X0)    # one Newton step: error kappa^2 u^2, far below either route's
        blocks = lambda A: (A[:P, :P], np.stack([A[np.ix_(ie[g], ie[g])] for g in range(G + 1)]), np.stack([A[:P][:, ie[g]] for g in range(G + 1)]))
        (cb, cu, cbu), ref_blocks = blocks(Hinv), blocks(Hinv_ld)
        floor = kappa * H.shape[0] * U53
        off = {'logistic': None, 'poisson': b['o_poisson'], 'binomial': b['o_binomial'], 'negbinomial': b['o_binomial']}[fam]   # the negative binomial predicts at its RAW offset
        tr = b['trials'] if fam == 'binomial' else None                  # ... and through the Poisson mean: no trials
        new = sp.new_rows(fam, b)
        sl = slice(n0, n1)
        gnew = np.where(new['groups'] < 0, G, new['groups'])
        for what, rows, trials in (('predict_window', (b['x'][sl], b['z'][sl], b['gid'][sl], None if off is None else off[sl]),
                                    None if tr is None else tr[sl]),
                                   ('predict_new', (new['x'], new['z'], gnew, new.get('offset')), new.get('trials'))):
            got = sfixture['%s/%s/%s' % (case['name'], fam, what)]
            x, z, gid, o = rows
            rho, s_mf, v_lr = predict_rows(x, z, gid, o, m, v, e2, r2, cb, cu, cbu)
            t_rho = np.concatenate([(np.zeros(x.shape[0]) if o is None else o)[:, None], x * m[None, :], z * e2[gid]], axis=1).astype(LD)
            t_s = np.concatenate([(x * x).astype(LD) * v[None, :].astype(LD), (z * z).astype(LD) * r2[gid].astype(LD)], axis=1)
            assert np.all(np.abs(got[0].astype(LD) - t_rho.sum(1)) <= (P + K + 2) * U53 * np.abs(t_rho).sum(1))
            assert np.all(np.abs(got[1].astype(LD) - t_s.sum(1)) <= (P + K + 2) * U53 * np.abs(t_s).sum(1))
            want = predict_rows(x, z, gid, o, m, v, e2, r2, *ref_blocks)[2]
            e_fix, e_host = np.abs(got[2].astype(LD) - want) / want, np.abs(v_lr.astype(LD) - want) / want
            print(case['name'], fam, what, 'var_lrvb: err %.3e, err_host %.3e, floor %.3e' % (float(e_fix.max()), float(e_host.max()), floor))
            assert np.all(want > 0) and np.all(e_fix <= 8.0 * e_host + floor)
            sub = np.arange(min(8, x.shape[0]))
            trs = None if trials is None else trials[sub]
            for col, var in ((3, 1), (4, 2)):
                mine = _gh_mean(fam, got[0][sub], got[var][sub], trs, gh_x, gh_w)
                exact = _gh_mean(fam, got[0][sub], got[var][sub], trs, gh_x, gh_w, mp=True)
                for a, d, ex in zip(mine, got[col][sub], exact):
                    if ex == 0:
                        assert a == 0.0 and d == 0.0                     # a binomial row without trials
                        continue
                    own = float(abs(mpmath.mpf(float(a)) - ex) / abs(ex))
                    assert abs(d - a) <= max(8.0 * own, 16.0 * U53) * abs(a)


# ---- tests/golden/glmm_policies_parent.npz: the likelihood policies behind the shared node loop ------------
import torch                                                             # noqa: E402

P_IDS = [c['name'] for c in mg.POLICY_CASES]
TERMS_FAMILIES = [f for f in mg.POLICY_FAMILIES if f.get('terms', True)]


@pytest.fixture(scope='module')
def pfixture():
    with np.load(mg.POLICY_FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_policy_fixture_names_its_parent_and_is_complete(pfixture):
    assert os.path.getsize(mg.POLICY_FIXTURE) < 1024 * 1024
    assert re.fullmatch(r'[0-9a-f]{40}', str(pfixture['parent_commit']))
    assert 'HIP version' in str(pfixture['hipcc_version'])
    assert [f['name'] for f in TERMS_FAMILIES] == ['binomial', 'probit', 'cloglog', 'ztpoisson', 'ztnegbin', 'beta', 'gamma', 'censnormal']
    assert [f['name'] for f in mg.POLICY_FAMILIES if f.get('predict')] == ['binomial', 'probit', 'cloglog', 'ztpoisson', 'ztnegbin', 'censnormal']
    assert [f['name'] for f in mg.POLICY_FAMILIES if f.get('dispersion')] == ['beta', 'gamma', 'censnormal', 'negbin']
    for case in mg.POLICY_CASES:
        N, P, K, G = case['shape']
        n0, n1 = mg.window(N)
        for fam in mg.POLICY_FAMILIES:
            head = '%s/%s/' % (case['name'], fam['name'])
            for name in mg.policy_outputs(fam):
                key = head + name
                raw = key in pfixture
                assert raw != (key + ':sha256' in pfixture and key + ':shape' in pfixture), key
                if raw:
                    assert pfixture[key].size <= mg.RAW_MAX and np.all(np.isfinite(pfixture[key]))
                else:
                    assert np.prod(pfixture[key + ':shape']) > mg.RAW_MAX
            if fam.get('terms', True):
                assert pfixture[head + 'value'].tobytes() == pfixture[head + 'value_only'].tobytes()
                assert pfixture[head + 'grad'].shape == (2 * P,)
                assert pfixture[head + 'scalar_columns'].shape == (G, 2 * K + K * (2 * K + 1))
            if fam.get('predict'):
                assert pfixture[head + 'predict_window'].shape == (5, n1 - n0) and pfixture[head + 'predict_new'].shape == (5, mg.N_NEW)
            if fam.get('dispersion'):
                assert pfixture[head + 'dispersion_d'].shape == (2,) and pfixture[head + 'dispersion_cross_global'].shape == (2 * P,)
                assert pfixture[head + 'dispersion_cross_local'].shape == (G, 2 * K)
    assert len(pfixture) == 2 + len(mg.POLICY_CASES) + sum(
        (1 if '%s/%s/%s' % (c['name'], f['name'], o) in pfixture else 2)
        for c in mg.POLICY_CASES for f in mg.POLICY_FAMILIES for o in mg.policy_outputs(f))


@pytest.mark.parametrize('case', mg.POLICY_CASES, ids=P_IDS)
def test_policy_cases_rebuild_from_their_seeds(pfixture, case):
    a, b = mg.build_policy_case(case), mg.build_policy_case(case)
    assert mg.policy_inputs_digest(a) == mg.policy_inputs_digest(b) == str(pfixture[case['name'] + ':inputs'])


def test_policy_cases_are_the_witnesses_they_are_meant_to_be():
    built = {c['name']: (c, mg.build_policy_case(c)) for c in mg.POLICY_CASES}
    assert [(c['shape'], c['deg']) for c in mg.POLICY_CASES] == [((1, 1, 1, 1), 1), ((65, 5, 2, 3), 5), ((37, 3, 1, 5), 128), ((130, 64, 4, 2), 20)]
    owned = lambda deg: [len(range(q4, deg, 4)) for q4 in range(4)]     # the nodes of the four lanes of a row
    assert owned(1) == [1, 0, 0, 0] and owned(5) == [2, 1, 1, 1] and owned(128) == [32] * 4 and mg.GLMM_TILE - 1 == 63
    assert built['one_node'][1]['fam']['censnormal']['censoring'][0] != 0                  # the single row is censored
    c, b = built['cut_group']
    s = np.bincount(b['gid'], minlength=3)                               # group 1 is cut by the boundary at row 64; group 2 is empty
    assert 0 < s[0] < 64 < s[0] + s[1] == 65 and s[2] == 0 and np.sum(b['w'] == 0.0) >= 3
    c, b = built['all_columns']
    assert tuple(np.bincount(b['gid'], minlength=2)) == (30, 100) and c['shape'][1] == 64
    for name, (c, b) in built.items():
        f = b['fam']
        assert np.any(f['binomial']['trials'] != 1.0) or c['shape'][0] == 1
        assert np.all(f['ztpoisson']['y'] >= 1.0) and np.all(f['ztnegbin']['y'] >= 1.0) and np.all(f['gamma']['y'] > 0.0)
        assert np.all((f['beta']['y'] > 0.0) & (f['beta']['y'] < 1.0)) and np.any(b['o'] != 0.0)
        cov = mg.policy_coverage(c, b)
        if c['shape'][0] >= 64:                                          # statuses -1, 0, +1 as neighbours inside one tile
            assert cov['statuses_mixed']
    assert built['cut_group'][0]['deg'] == 5 and all(mg.policy_coverage(*built['cut_group']).values())   # every branch on nodes of weight >= 0.011
    assert all(mg.coverage_of_all_cases().values())
    assert np.any(built['cut_group'][1]['new']['groups'] == -1)


import contextlib                                                        # noqa: E402


@contextlib.contextmanager
def _reference_nodes(r, deg):
    """The binomial reference reads its node count from the module and the link reference binds it as a default, in the forward
    pass and again in the backward one: both are set to the case's for as long as the reference is evaluated AND differentiated."""
    keep = r['bref'].GH_DEG, r['lref'].expected_dk
    r['bref'].GH_DEG = deg
    r['lref'].expected_dk = lambda link, which, mu, s, k: keep[1](link, which, mu, s, k, deg)
    try:
        yield
    finally:
        r['bref'].GH_DEG, r['lref'].expected_dk = keep


def _policy_reference(r, case, b, name):
    """eta -> the data term of the family by its torch reference, at the case's number of nodes (inside `_reference_nodes`)."""
    N, P, K, G = case['shape']
    x, z, w, o, gid, deg, d = b['x'], b['z'], b['w'], b['o'], b['gid'], b['deg'], b['fam'][name]
    if name == 'binomial':
        ta = r['bref'].targs(x, d['y'], z, w, o, d['trials'], gid, G)
        return lambda eta: r['bref'].kl_vec(eta, *ta) - r['bref']._priors(eta, ta[0], ta[1], ta[2], ta[3], ta[6], G, ta[8])
    if name in ('probit', 'cloglog'):
        ta = r['lref'].targs(x, d['y'], z, w, o, d['trials'], gid, G, name)
        return lambda eta: r['lref'].data(eta, *ta[:8], name)
    if name == 'ztpoisson':
        ta = r['ztp'].targs(x, d['y'], z, w, o, gid, G)
        return lambda eta: r['ztp'].data(eta, *ta[:7], deg)
    if name == 'censnormal':
        ta = r['cens'].targs(x, d['y'], z, w, o, d['dispersion'], gid, G, d['censoring'])
        return lambda eta: r['cens'].data(eta, *ta[:8], ta[9], deg)
    mod = r[{'ztnegbin': 'ztnb', 'beta': 'beta', 'gamma': 'gamma'}[name]]
    ta = mod.targs(x, d['y'], z, w, o, d['dispersion'], gid, G)
    return lambda eta: mod.data(eta, *ta[:8], mod.GH_DEG if name == 'gamma' else deg)


@pytest.mark.parametrize('case', mg.POLICY_CASES, ids=P_IDS)
def test_recorded_policy_values_and_gradients_agree_with_the_references(pfixture, case):
    """Value 1e-11 and gradients 1e-10 relative, the tolerances of `_check_against_reference` (tests/test_gpu_glmm_binomial.py) that
    the `test_reference_parity` of every one of these families runs.  The gradient of the reference is taken in eta by autograd and
    moved to the coordinates of the entry: v = 1 / i_beta and r = 1 / i, so d/dv = -i^2 d/di."""
    N, P, K, G = case['shape']
    b = mg.build_policy_case(case)
    eta, ng, GK = b['eta'], 2 * P + 4 * K, G * K
    r = mg._policy_refs()
    for fam in TERMS_FAMILIES:
        t = torch.tensor(eta, requires_grad=True)
        with _reference_nodes(r, b['deg']):
            val = _policy_reference(r, case, b, fam['name'])(t)
            g = torch.autograd.grad(val, t)[0].numpy()
        val = float(val.detach())
        g_glob = np.concatenate([g[:P], -eta[P:2 * P] ** 2 * g[P:2 * P]])
        g_loc = np.concatenate([g[ng:ng + GK].reshape(G, K), (-eta[ng + GK:] ** 2 * g[ng + GK:]).reshape(G, K)], axis=1)
        head = '%s/%s/' % (case['name'], fam['name'])
        e = [abs(float(pfixture[head + 'value'][0]) - val) / abs(val), rel_err(pfixture[head + 'grad'], g_glob),
             rel_err(pfixture[head + 'scalar_columns'][:, :2 * K], g_loc)]
        print(case['name'], fam['name'], e)
        assert e[0] < 1e-11 and e[1] < 1e-10 and e[2] < 1e-10

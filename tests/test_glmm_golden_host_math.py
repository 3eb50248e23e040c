"""tests/golden/glmm_walk_parent.npz and tests/golden/glmm_intercept_parent.npz without a GPU: the fixture loads and names the commit it was recorded from, its cases
rebuild from their seeds to the inputs it was recorded with and are the witnesses they are meant to be, and the recorded values
and gradients of both models agree with the torch references (tests/glmm_slopes_reference.py, tests/glmm_poisson_reference.py)
to the tolerances of `_check_against_reference` in the GPU tests: value 1e-11, gradient 1e-10 relative.  So a fixture recorded from
a broken build does not pass for the truth that tests/test_gpu_glmm_walk_golden.py compares against bit for bit.  The intercept
fixture is checked the same way against tests/glmm_reference.py, at the same tolerances; what it holds raw
of the Hessian pieces at the 1e-9 of tests/test_gpu_glmm.py."""
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

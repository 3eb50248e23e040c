"""The four random-intercept entries (`glmm_terms`, `glmm_schur`, `glmm_obs_influence`, `glmm_group_influence`) reproduce BIT FOR BIT
what the commit before they moved onto the shared likelihood policy, the shared host bodies and the shared resident buffer computed
on an MI355X: every output equals the raw array of tests/golden/glmm_intercept_parent.npz, or its shape and
SHA-256 where the array is large, and every refusal its status code and its message.  No tolerance -- the move keeps every
floating-point expression, every summation order and every check.  Cases, seeds and the recorder:
tests/golden/make_glmm_intercept_golden.py; the fixture itself is checked on the CPU by tests/test_glmm_golden_host_math.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_glmm_intercept_golden as ig                                  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


@pytest.fixture(scope='module')
def fixture():
    with np.load(ig.FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('case', ig.CASES, ids=[c['name'] for c in ig.CASES])
def test_outputs_are_bitwise_those_of_the_parent(vb, fixture, case):
    b = ig.build_case(case)
    assert ig.inputs_digest(b) == str(fixture[case['name'] + ':inputs'])             # the inputs the fixture was recorded with
    got = ig.run_case(vb, case, b)
    assert len(got) == 6 + 1 + 5 + 1 + 1 + 2 * len(ig.QS)
    differ = [key for key, arr in got.items() if not ig.mg.matches(fixture, case['name'] + '/' + key, arr)]
    for key in differ:                                                               # a figure for whoever has to find the expression
        full = case['name'] + '/' + key
        if full in fixture and fixture[full].shape == np.shape(got[key]):
            print(full, 'max |difference|', np.max(np.abs(fixture[full] - got[key])))
    assert not differ


def test_refusals_are_those_of_the_parent(vb, fixture):
    case = next(c for c in ig.CASES if c['name'] == ig.REFUSAL_CASE)
    got = ig.run_refusals(vb, case, ig.build_case(case))
    recorded = sorted(k[len('refusal/'):-len(':status')] for k in fixture if k.startswith('refusal/') and k.endswith(':status'))
    assert sorted(got) == recorded and len(recorded) == 29
    differ = {k: v for k, v in got.items() if not ig.refusal_matches(fixture, k, v)}
    print(differ)
    assert not differ

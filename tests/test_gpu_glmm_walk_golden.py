"""The six K-effect mixed-model entries (`glmm_slopes_*` and `glmm_poisson_*`: terms, obs_influence, group_influence) reproduce BIT
FOR BIT what the commit before the merge of the two tile walks computed on an MI355X: every output equals
the raw array of tests/golden/glmm_walk_parent.npz, or its shape and SHA-256 where the array is large.  No tolerance -- the merge
keeps every floating-point expression and every summation order.  Cases, seeds and the recorder: tests/golden/make_glmm_golden.py;
the fixture itself is checked on the CPU by tests/test_glmm_golden_host_math.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_glmm_golden as mg                                           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


@pytest.fixture(scope='module')
def fixture():
    with np.load(mg.FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('case', mg.CASES, ids=[c['name'] for c in mg.CASES])
def test_outputs_are_bitwise_those_of_the_parent(vb, fixture, case):
    b = mg.build_case(case)
    assert mg.inputs_digest(b) == str(fixture[case['name'] + ':inputs'])             # the inputs the fixture was recorded with
    got = mg.run_case(vb, case, b)
    assert len(got) == 2 * (6 + 2 * len(mg.QS))
    differ = [key for key, arr in got.items() if not mg.matches(fixture, case['name'] + '/' + key, arr)]
    for key in differ:                                                               # a figure for whoever has to find the expression
        full = case['name'] + '/' + key
        if full in fixture and fixture[full].shape == np.shape(got[key]):
            print(full, 'max |difference|', np.max(np.abs(fixture[full] - got[key])))
    assert not differ

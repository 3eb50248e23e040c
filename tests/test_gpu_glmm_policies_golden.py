"""The likelihood policies of k_glmm_walk.h other than the logistic and the Poisson one -- binomial with trials and an offset, probit,
cloglog, zero-truncated Poisson and NB2, Beta, Gamma, censored Gaussian -- reproduce BIT FOR BIT, through their terms, row and
group influence, predict and dispersion entries, what the commit before their node loop and lane reduction were shared computed on
an MI355X: every output equals the raw array of tests/golden/glmm_policies_parent.npz, or its shape and
SHA-256 where the array is large.  No tolerance -- sharing the loop keeps every floating-point expression and every summation order.
One case per row of POLICY_CASES (tests/golden/make_glmm_golden.py), the smallest shapes at which the walk of a row over its four
lanes can go wrong; the fixture itself is checked on the CPU by tests/test_glmm_golden_host_math.py."""
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
    with np.load(mg.POLICY_FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('case', mg.POLICY_CASES, ids=[c['name'] for c in mg.POLICY_CASES])
def test_policy_outputs_are_bitwise_those_of_the_parent(vb, fixture, case):
    b = mg.build_policy_case(case)
    assert mg.policy_inputs_digest(b) == str(fixture[case['name'] + ':inputs'])      # the inputs the fixture was recorded with
    got = mg.run_policy_case(vb, case, b)
    assert sorted(got) == sorted('%s/%s' % (f['name'], o) for f in mg.POLICY_FAMILIES for o in mg.policy_outputs(f))
    differ = [key for key, arr in got.items() if not mg.matches(fixture, case['name'] + '/' + key, arr)]
    for key in differ:                                                               # a figure for whoever has to find the expression
        full = case['name'] + '/' + key
        if full in fixture and fixture[full].shape == np.shape(got[key]):
            print(full, 'max |difference|', np.max(np.abs(fixture[full] - got[key])))
    assert not differ

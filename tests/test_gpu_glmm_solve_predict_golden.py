"""The device-resident block-arrow layer of the K-effect mixed models (`glmm_slopes_schur`, `glmm_slopes_solve_forward` / `_back`,
`glmm_slopes_group_cov`, the three predict entries) on the logistic, Poisson, binomial and negative-binomial families, and the
binomial walk with trials != 1, reproduce BIT FOR BIT what the commit before the window walk, the local triangular solves and the
host bodies were shared computed on an MI355X: every output equals the raw array of
tests/golden/glmm_solve_predict_parent.npz, or its shape and SHA-256 where the array is large, and every refusal its status code and
its message.  No tolerance -- the move keeps every floating-point expression, every summation order and every check.  Cases, seeds
and the recorder: tests/golden/make_glmm_solve_predict_golden.py; the fixture itself is checked on the CPU by
tests/test_glmm_golden_host_math.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_glmm_solve_predict_golden as sp                              # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


@pytest.fixture(scope='module')
def fixture():
    with np.load(sp.FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('case', sp.CASES, ids=[c['name'] for c in sp.CASES])
def test_outputs_are_bitwise_those_of_the_parent(vb, fixture, case):
    b = sp.build_case(case)
    assert sp.inputs_digest(b) == str(fixture[case['name'] + ':inputs'])             # the inputs the fixture was recorded with
    got = sp.run_case(vb, case, b)
    assert len(got) == len(sp.FAMILIES) * (2 * len(sp.SOLVE_QS) + 4) + 4 + 2 * len(sp.INFL_QS)
    differ = [key for key, arr in got.items() if not sp.matches(fixture, case['name'] + '/' + key, arr)]
    for key in differ:                                                               # a figure for whoever has to find the expression
        full = case['name'] + '/' + key
        if full in fixture and fixture[full].shape == np.shape(got[key]):
            print(full, 'max |difference|', np.max(np.abs(fixture[full] - got[key])))
    assert not differ


def test_refusals_are_those_of_the_parent(vb, fixture):
    case = next(c for c in sp.CASES if c['name'] == sp.REFUSAL_CASE)
    got = sp.run_refusals(vb, case, sp.build_case(case))
    recorded = sorted(k[len('refusal/'):-len(':status')] for k in fixture if k.startswith('refusal/') and k.endswith(':status'))
    assert sorted(got) == recorded and len(recorded) == sp.N_REFUSALS
    differ = {k: v for k, v in got.items() if not sp.refusal_matches(fixture, k, v)}
    print(differ)
    assert not differ

"""`LogisticGLMMObjective` as the K = 1 instance of the shared mixed-model class: what the random-slopes class did and the intercept
class did not before the two were joined -- the initial weights on the device from the constructor on, `stats_size`, the
`on_device` keyword -- and the statistics buffer through the shared code.  Reference: tests/glmm_reference.py."""
import numpy as np
import pytest

import glmm_reference as ref
from helpers import rel_err

pytestmark = pytest.mark.gpu


def test_constructor_pushes_weights_and_shared_statistics():
    import lrvb_amd as vb
    N, P, G = 37, 3, 5
    x, y, w, gid, free = ref.problem(N, P, G, seed=N + P)
    assert not np.all(w == 1.0) and not np.any(gid == G - 1)             # weights that matter, an empty group
    par = vb.ModelParamsDict('params')
    par.push_param(vb.UVNParamVector('beta', length=P))
    par.push_param(vb.UVNParam('mu'))
    par.push_param(vb.GammaParam('tau'))
    par.push_param(vb.UVNParamVector('u', length=G))
    fun = vb.LogisticGLMMObjective(par, x, y, gid, G, weights=w)         # no fun._push_state() here
    ng = 2 * P + 4
    eta = np.where(ref.positive_mask(P, G), np.exp(free), free)
    want = ref.data_pieces(x, y, w, gid, G, eta)['value']
    assert abs(ref.data_pieces(x, y, np.ones(N), gid, G, eta)['value'] - want) > 1e-3 * abs(want)
    val = fun.ctx.glmm_terms(eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + G], 1.0 / eta[ng + G:], fun.gh_x, fun.gh_w)[0]
    print('data term: device %.15e, reference %.15e' % (val, want))
    assert abs(val - want) < 1e-11 * abs(want)
    # on_device=True is refused before anything is launched: the intercept has no factor entry on the device
    with pytest.raises(ValueError):
        fun.solve(free, np.ones(free.size), on_device=True)
    # the statistics buffer of the shared code
    stats = fun.local_stats(eta)
    assert fun.stats_size() == stats.size == 1 + 2 * P + 3 * P * P + G * (5 + 4 * P)
    H = fun.hessian(eta, False)
    fun.set_reduced_stats(stats, eta)
    err = rel_err(fun.hessian(eta, False), H)
    print('Hessian from the installed statistics against the direct one: %.3e' % err)
    assert err < 1e-13

"""The host layer of the mixed models is likelihood-independent: `glmm_slopes_closed_forms` fed the data pieces of the POISSON
reference (tests/glmm_poisson_reference.py) reproduces the autograd gradient and Hessian of the full Poisson KL, and the closed
coefficient formulas of DESIGN.md section 26 are the autograd derivatives of psi = exp(rho + s / 2).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glmm_poisson_reference as ref                                     # noqa: E402

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def test_closed_coefficients_are_the_derivatives_of_psi():
    """a1 = h - w y, a2 = h / 2, c11 = h, c12 = h / 2, c22 = h / 4 with h = w psi, to 1e-13 relative."""
    rng = np.random.default_rng(0)
    n = 400
    rho, s = rng.normal(size=n) * 2.0, rng.uniform(0.0, 3.0, size=n)
    w, y = rng.uniform(0.5, 1.5, size=n), rng.poisson(3.0, size=n).astype(np.float64)
    psi, p_r, p_s, p_rr, p_rs, p_ss = ref.psi_coefs(rho, s)
    h = w * np.exp(rho + 0.5 * s)
    assert _rel(w * psi, h) < 1e-13
    for got, want in ((h - w * y, w * (p_r - y)), (0.5 * h, w * p_s), (h, w * p_rr), (0.5 * h, w * p_rs), (0.25 * h, w * p_ss)):
        assert _rel(got, want) < 1e-13


@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 6, 4, 2)])
def test_closed_forms_on_poisson_pieces_reproduce_the_reference(N, P, K, G):
    """The tolerances of tests/test_glmm_slopes_host_math.py: value 1e-12, gradient 1e-10, Hessian 1e-9 (vector and free)."""
    from lrvb_amd import glmm_slopes as gs
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed=N + P + K)
    mask = ref.positive_mask(P, K, G)
    eta = np.where(mask, np.exp(free), free)
    ng = 2 * P + 4 * K
    cf = gs.glmm_slopes_closed_forms(P, K, G, eta, ref.data_pieces(x, y, z, w, o, gid, G, eta), *HYP)
    targs = ref.targs(x, y, z, w, o, gid, G, HYP)
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    assert abs(cf['value'] - val) <= 1e-12 * abs(val)
    assert _rel(cf['grad'], g) < 1e-10
    assert _rel(gs.block_arrow_dense(cf['Hgg'], cf['rows'], cf['Hx'], cf['loc']), H) < 1e-9
    j1, j2 = np.where(mask, eta, 1.0), np.where(mask, eta, 0.0)
    gf, Hgg, rows, Hx, loc = gs.block_arrow_to_free(cf, j1, j2, ng, G, K)
    _, g_f, H_f = ref.value_grad_hess(ref.kl_free, free, targs)
    assert _rel(gf, g_f) < 1e-10
    assert _rel(gs.block_arrow_dense(Hgg, rows, Hx, loc), H_f) < 1e-9

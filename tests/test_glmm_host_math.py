"""The N-independent closed forms of the logistic mixed model (`glmm_closed_forms` and the arrow helpers of
linearresponsevariationalbayes.py_amd/glmm.py) against the torch reference tests/glmm_reference.py, without a GPU: the data
pieces are formed in numpy from the reference's own per-row derivatives."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glmm_reference as ref                                             # noqa: E402

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0
SHAPES = [(40 + 9 * G, P, G) for P in (1, 3, 8) for G in (1, 5, 40)]


def _setup(N, P, G, seed=0):
    from lrvb_amd import glmm
    x, y, w, gid, free = ref.problem(N, P, G, seed)
    mask = ref.positive_mask(P, G)
    eta = np.where(mask, np.exp(free), free)
    data = ref.data_pieces(x, y, w, gid, G, eta)
    cf = glmm.glmm_closed_forms(P, G, eta, data, *HYP)
    args = ref.tensors(x, y, w, gid, HYP)
    targs = (args[0], args[1], args[2], args[3], G, args[4])
    return glmm, x, gid, free, eta, mask, cf, targs


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize('N,P,G', SHAPES)
def test_closed_forms_reproduce_reference(N, P, G):
    glmm, x, gid, free, eta, mask, cf, targs = _setup(N, P, G)
    ng = 2 * P + 4
    if G >= 3:
        assert not np.any(gid == G - 1)                                  # the empty group
    # vector coordinates
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    assert abs(cf['value'] - val) <= 1e-11 * abs(val)
    assert _rel(cf['grad'], g) < 1e-10
    Hd = glmm.arrow_dense(cf['Hgg'], cf['rows'], cf['Hx'], cf['loc'])
    assert _rel(Hd, H) < 1e-9
    # the sparsity claim, on the REFERENCE Hessian: no local entries outside the (e_g, i_g) pairs, no border in row i_mu
    Hll = H[ng:, ng:].copy()
    ie, ii = np.arange(G), np.arange(G, 2 * G)
    Hll[ie, ie] = Hll[ii, ii] = Hll[ie, ii] = Hll[ii, ie] = 0.0
    assert np.all(Hll == 0.0)
    assert np.all(H[2 * P + 1, ng:] == 0.0)
    # free coordinates
    j1 = np.where(mask, eta, 1.0)
    j2 = np.where(mask, eta, 0.0)
    gf, Hgg, rows, Hx, loc = glmm.arrow_to_free(cf, j1, j2, ng, G)
    valf, g_f, H_f = ref.value_grad_hess(ref.kl_free, free, targs)
    assert abs(valf - val) <= 1e-12 * abs(val)
    assert _rel(gf, g_f) < 1e-10
    Hfd = glmm.arrow_dense(Hgg, rows, Hx, loc)
    assert _rel(Hfd, H_f) < 1e-9
    # arrow product
    rng = np.random.default_rng(1)
    v = rng.normal(size=free.size)
    assert _rel(glmm.arrow_matvec(Hgg, rows, Hx, loc, v), H_f @ v) < 1e-9
    # Schur complement from the pieces against the reference Hessian's
    HS = Hgg.copy()
    HS[np.ix_(rows, rows)] -= glmm.arrow_schur_term(rows, Hx, loc)
    HS_ref = H_f[:ng, :ng] - H_f[:ng, ng:] @ np.linalg.solve(H_f[ng:, ng:], H_f[ng:, :ng])
    assert _rel(HS, HS_ref) < 1e-9
    # local solve
    be, bi = rng.normal(size=G), rng.normal(size=G)
    se, si = glmm.arrow_local_solve(loc, be, bi)
    sol = np.linalg.solve(H_f[ng:, ng:], np.concatenate([be, bi]))
    assert _rel(np.concatenate([se, si]), sol) < 1e-9


def test_indefinite_local_block_is_refused():
    from lrvb_amd import glmm
    loc = np.array([[1.0, 2.0, 1.0]])
    with pytest.raises(np.linalg.LinAlgError):
        glmm.arrow_schur_term(np.arange(3), np.ones((3, 2)), loc)

"""The N-independent closed forms of the logistic mixed model with random slopes (`glmm_slopes_closed_forms` and the block-arrow
helpers of linearresponsevariationalbayes.py_amd/glmm_slopes.py) against the torch reference tests/glmm_slopes_reference.py,
without a GPU: the data pieces are formed in numpy from the reference's own per-row derivatives."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glmm_reference as ref1                                            # noqa: E402
import glmm_slopes_reference as ref                                      # noqa: E402

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0
SHAPES = [(60 + 9 * G, P, K, G) for K in (1, 2, 4) for (P, G) in ((1, 1), (3, 5), (8, 12))]


def _setup(N, P, K, G, seed=0):
    from lrvb_amd import glmm_slopes as gs
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed)
    mask = ref.positive_mask(P, K, G)
    eta = np.where(mask, np.exp(free), free)
    data = ref.data_pieces(x, y, z, w, gid, G, eta)
    cf = gs.glmm_slopes_closed_forms(P, K, G, eta, data, *HYP)
    t = ref.tensors(x, y, z, w, gid, HYP)
    targs = (t[0], t[1], t[2], t[3], t[4], G, t[5])
    return gs, gid, free, eta, mask, cf, targs


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize('N,P,K,G', SHAPES)
def test_closed_forms_and_block_arrow_reproduce_reference(N, P, K, G):
    gs, gid, free, eta, mask, cf, targs = _setup(N, P, K, G)
    ng = 2 * P + 4 * K
    if G >= 3:
        assert not np.any(gid == G - 1) and np.sum(gid == 0) > N / 2     # the empty group, the big group
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    assert abs(cf['value'] - val) <= 1e-12 * abs(val)
    assert _rel(cf['grad'], g) < 1e-10
    Hd = gs.block_arrow_dense(cf['Hgg'], cf['rows'], cf['Hx'], cf['loc'])
    assert _rel(Hd, H) < 1e-9
    # the sparsity claim on the REFERENCE Hessian: no border in the rows i_mu_k, no entries between different groups
    assert np.all(H[2 * P + K:2 * P + 2 * K, ng:] == 0.0)
    Hll = H[ng:, ng:].copy()
    li = gs._local_index(G, K)
    Hll[li[:, :, None], li[:, None, :]] = 0.0
    assert np.all(Hll == 0.0)
    # free coordinates
    j1, j2 = np.where(mask, eta, 1.0), np.where(mask, eta, 0.0)
    gf, Hgg, rows, Hx, loc = gs.block_arrow_to_free(cf, j1, j2, ng, G, K)
    valf, g_f, H_f = ref.value_grad_hess(ref.kl_free, free, targs)
    assert _rel(gf, g_f) < 1e-10
    Hfd = gs.block_arrow_dense(Hgg, rows, Hx, loc)
    assert _rel(Hfd, H_f) < 1e-9
    # product, Schur term and solve against the dense matrix
    rng = np.random.default_rng(1)
    v = rng.normal(size=free.size)
    assert _rel(gs.block_arrow_matvec(Hgg, rows, Hx, loc, v), Hfd @ v) < 1e-10
    # (the point is not an optimum, so the matrix need not be positive definite there: the linear algebra is checked on the
    # block arrow shifted by a multiple of the identity that makes it so)
    lam = max(0.0, -np.min(np.linalg.eigvalsh(Hfd))) + 1.0
    Hfd = Hfd + lam * np.eye(free.size)
    Hgg = Hgg + lam * np.eye(ng)
    loc = loc + lam * np.eye(2 * K)[None]
    assert _rel(gs.block_arrow_dense(Hgg, rows, Hx, loc), Hfd) < 1e-15
    M = gs.block_arrow_schur_term(rows, Hx, loc)
    M_ref = Hfd[np.ix_(rows, ng + np.arange(2 * G * K))] @ np.linalg.solve(Hfd[ng:, ng:], Hfd[np.ix_(ng + np.arange(2 * G * K), rows)])
    assert _rel(M, M_ref) < 1e-10
    R = rng.normal(size=(free.size, 3))
    X = gs.block_arrow_solve(Hgg, rows, Hx, loc, R)
    assert _rel(X, np.linalg.solve(Hfd, R)) < 1e-10
    assert _rel(gs.block_arrow_solve(Hgg, rows, Hx, loc, R[:, 0]), X[:, 0]) < 1e-14
    S = Hgg.copy()
    S[np.ix_(rows, rows)] -= M
    Xs = gs.block_arrow_solve(Hgg, rows, Hx, loc, R, schur_solve=lambda B: np.linalg.solve(S, B))
    assert _rel(Xs, X) < 1e-10


def test_group_sum_packing_round_trip():
    gs, gid, free, eta, mask, cf, targs = _setup(80, 3, 2, 4)
    x, y, z, w, gid, _ = ref.problem(80, 3, 2, 4, 0)
    d = ref.data_pieces(x, y, z, w, gid, 4, eta)
    flat = gs.pack_group_sums(d['g_loc'], d['loc'], d['border'])
    assert flat.shape == (4, gs.group_sums_ncol(3, 2)[1])
    gl, loc, border = gs.unpack_group_sums(flat, 3, 2)
    assert np.array_equal(gl, d['g_loc']) and np.array_equal(loc, d['loc']) and np.array_equal(border, d['border'])
    assert gs.unpack_group_sums(flat[:, :gs.group_sums_ncol(3, 2)[0]], 3, 2)[2] is None


def test_non_positive_definite_local_block_raises():
    gs, gid, free, eta, mask, cf, targs = _setup(100, 3, 2, 5)
    loc = cf['loc'].copy()
    loc[2, 1, 1] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        gs.block_arrow_schur_term(cf['rows'], cf['Hx'], loc)
    with pytest.raises(np.linalg.LinAlgError):
        gs.block_arrow_solve(cf['Hgg'], cf['rows'], cf['Hx'], loc, np.ones(free.size))


@pytest.mark.parametrize('N,P,G', [(70, 1, 1), (120, 4, 7)])
def test_one_effect_with_unit_design_is_the_intercept_model(N, P, G):
    """K = 1, z = 1: the closed forms equal `glmm_closed_forms` on the same pieces to 1e-13."""
    from lrvb_amd import glmm, glmm_slopes as gs
    x, y, w, gid, free = ref1.problem(N, P, G, 3)
    eta = np.where(ref1.positive_mask(P, G), np.exp(free), free)
    assert np.array_equal(ref1.positive_mask(P, G), ref.positive_mask(P, 1, G))
    d1 = ref1.data_pieces(x, y, w, gid, G, eta)
    dk = ref.data_pieces(x, y, np.ones((N, 1)), w, gid, G, eta)
    a = glmm.glmm_closed_forms(P, G, eta, d1, *HYP)
    b = gs.glmm_slopes_closed_forms(P, 1, G, eta, dk, *HYP)
    assert abs(a['value'] - b['value']) <= 1e-13 * abs(a['value'])
    assert _rel(b['grad'], a['grad']) < 1e-13 and _rel(b['Hgg'], a['Hgg']) < 1e-13 and _rel(b['Hx'], a['Hx']) < 1e-13
    assert np.array_equal(a['rows'], b['rows'])
    loc = np.stack([b['loc'][:, 0, 0], b['loc'][:, 0, 1], b['loc'][:, 1, 1]], axis=1)
    assert _rel(loc, a['loc']) < 1e-13

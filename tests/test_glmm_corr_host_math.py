"""The N-independent closed forms of the mixed models with correlated random effects (`glmm_corr_closed_forms`,
`glmm_corr_border_tables` of linearresponsevariationalbayes.py_amd/glmm_corr.py) and the optional arguments they need of
block_arrow.py, against the torch reference tests/glmm_corr_reference.py, without a GPU: the data pieces are formed in numpy from
the reference's own per-row derivatives.  Tolerances are those of tests/test_glmm_slopes_host_math.py for the same quantities:
value 1e-12, gradient 1e-10, Hessian 1e-9, products and solves 1e-10 relative."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glmm_corr_reference as ref                                        # noqa: E402
import glmm_slopes_reference as sref                                     # noqa: E402

#          lik,        N,  P, K, G
SHAPES = [('logistic', 69, 1, 1, 1), ('logistic', 105, 3, 1, 5), ('logistic', 105, 3, 2, 5), ('logistic', 168, 8, 3, 12),
          ('logistic', 105, 3, 4, 5), ('poisson', 123, 5, 2, 7)]


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _w0(hyp, K):
    from lrvb_amd.models import vech_to_sym
    return vech_to_sym(hyp[4:])


def _free_jac(P, K, G, eta, free):
    """(j1, j2, dense) of `block_arrow_to_free`: element-wise exp above the lower bounds (0; K - 1 for n), the log-Cholesky block."""
    from lrvb_amd.packing import pos_def_matrix_free_to_vector_jac, pos_def_matrix_free_to_vector_hess
    Kv, ng, D = ref.sizes(P, K, G)
    o = 2 * P + 2 * K
    mask = np.zeros(D, dtype=bool)
    mask[P:2 * P] = mask[2 * P + K:o] = mask[ng + G * K:] = True
    j1, j2 = np.where(mask, eta, 1.0), np.where(mask, eta, 0.0)
    j1[o] = j2[o] = eta[o] - (K - 1.0)
    fv = free[o + 1:ng]
    return j1, j2, (o + 1, pos_def_matrix_free_to_vector_jac(fv), pos_def_matrix_free_to_vector_hess(fv))


def _setup(lik, N, P, K, G, seed=0):
    from lrvb_amd import glmm_corr as gc
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, seed, lik)
    hyp = ref.other_hyp(K)
    eta = ref.free_to_vec(torch.tensor(free), P, K, G).numpy()
    data = ref.data_pieces(x, y, z, w, o, gid, G, eta, lik)
    cf = gc.glmm_corr_closed_forms(P, K, G, eta, data, hyp[0], hyp[1], hyp[2], hyp[3], _w0(hyp, K))
    return gc, gid, free, eta, data, cf, ref.targs(x, y, z, w, o, gid, G, hyp, lik)


@pytest.mark.parametrize('lik,N,P,K,G', SHAPES)
def test_closed_forms_and_block_arrow_reproduce_reference(lik, N, P, K, G):
    from lrvb_amd import block_arrow as ba
    gc, gid, free, eta, data, cf, targs = _setup(lik, N, P, K, G)
    Kv, ng, D = ref.sizes(P, K, G)
    assert ng == 2 * P + 2 * K + 1 + Kv and np.array_equal(cf['rows'], ref.coupled_rows(P, K)) and len(cf['rows']) == 2 * P + gc.n_closed(K)
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    assert abs(cf['value'] - val) <= 1e-12 * abs(val)
    assert _rel(cf['grad'], g) < 1e-10
    Hd = ba.block_arrow_dense(cf['Hgg'], cf['rows'], cf['Hx'], cf['loc'])
    assert _rel(Hd, H) < 1e-9
    # the sparsity claim on the REFERENCE Hessian: no border in the rows i_mu_k, no entries between different groups -- and a
    # DENSE closed border: every e_gk meets every e_mu_l (V of `problem` has no zero entry)
    assert np.all(H[2 * P + K:2 * P + 2 * K, ng:] == 0.0)
    Hll = H[ng:, ng:].copy()
    li = ba._local_index(G, K)
    Hll[li[:, :, None], li[:, None, :]] = 0.0
    assert np.all(Hll == 0.0)
    assert np.all(H[2 * P:2 * P + K, ng:ng + G * K] != 0.0)
    # free coordinates: the global Jacobian has one dense block
    j1, j2, dense = _free_jac(P, K, G, eta, free)
    gf, Hgg, rows, Hx, loc = ba.block_arrow_to_free(cf, j1, j2, ng, G, K, dense=dense)
    valf, g_f, H_f = ref.value_grad_hess(ref.kl_free, free, targs)
    assert abs(valf - val) <= 1e-13 * abs(val)
    assert _rel(gf, g_f) < 1e-10
    Hfd = ba.block_arrow_dense(Hgg, rows, Hx, loc)
    assert _rel(Hfd, H_f) < 1e-9
    rng = np.random.default_rng(1)
    v = rng.normal(size=free.size)
    assert _rel(ba.block_arrow_matvec(Hgg, rows, Hx, loc, v), Hfd @ v) < 1e-10
    # the linear algebra on the block arrow shifted by a multiple of the identity that makes it positive definite
    lam = max(0.0, -np.min(np.linalg.eigvalsh(Hfd))) + 1.0
    Hfd = Hfd + lam * np.eye(free.size)
    Hgg = Hgg + lam * np.eye(ng)
    loc = loc + lam * np.eye(2 * K)[None]
    R = rng.normal(size=(free.size, 3))
    X = ba.block_arrow_solve(Hgg, rows, Hx, loc, R)
    assert _rel(X, np.linalg.solve(Hfd, R)) < 1e-10
    # group blocks against the dense inverse; the means of mu are the first K closed columns
    Hinv = np.linalg.inv(Hfd)
    cb, cu, cbu = ba.block_arrow_group_cov(Hgg, rows, Hx, loc, P, K, population=True, mu=2 * P + np.arange(K))
    ie = ng + np.arange(G * K).reshape(G, K)
    imu = 2 * P + np.arange(K)
    assert cu.shape == (G + 1, K, K) and cbu.shape == (G + 1, P, K)
    assert _rel(cb, Hinv[:P, :P]) < 1e-10
    for gi in range(G):
        assert _rel(cu[gi], Hinv[np.ix_(ie[gi], ie[gi])]) < 1e-10 and _rel(cbu[gi], Hinv[:P][:, ie[gi]]) < 1e-10
    assert _rel(cu[G], Hinv[np.ix_(imu, imu)]) < 1e-10 and _rel(cbu[G], Hinv[:P][:, imu]) < 1e-10
    if K > 2:                                                            # without n_closed: 3 K closed columns (NC = 3 K up to K = 2)
        with pytest.raises(ValueError):
            ba.block_arrow_group_cov_by_phases(ng, rows, P, K, np.ones(len(rows)), None, None)


@pytest.mark.parametrize('P,G', [(1, 1), (4, 7)])
def test_one_effect_is_the_independent_model(P, G):
    """K = 1: Wishart_1(n, V) is Gamma(n / 2, 1 / (2 V)), so the model is `glmm_slopes_closed_forms` under a = n / 2,
    b = 1 / (2 V), a0 = nu0 / 2, b0 = W0 / 2 up to a constant: value DIFFERENCES between two points and gradients mapped by
    the chain rule (d/dn = 1/2 d/da, d/dV = -1 / (2 V^2) d/db) agree to 1e-11 relative."""
    from lrvb_amd import glmm_corr as gc, glmm_slopes as gs
    N, K = 60 + 9 * G, 1
    hyp = ref.other_hyp(1)
    Kv, ng, D = ref.sizes(P, 1, G)
    out = []
    for seed in (3, 4):
        x, y, z, w, gid, o, free = ref.problem(N, P, K, G, 3, 'logistic')
        if seed == 4:                                                    # another point, the same data
            free = free + 0.1 * np.random.default_rng(4).normal(size=free.size)
        eta = ref.free_to_vec(torch.tensor(free), P, K, G).numpy()
        data = ref.data_pieces(x, y, z, w, o, gid, G, eta)
        a = gc.glmm_corr_closed_forms(P, 1, G, eta, data, hyp[0], hyp[1], hyp[2], hyp[3], _w0(hyp, 1), want_hess=False)
        n, V = eta[2 * P + 2], eta[2 * P + 3]
        eta_s = np.concatenate([eta[:2 * P + 2], [0.5 * n, 0.5 / V], eta[ng:]])
        b = gs.glmm_slopes_closed_forms(P, 1, G, eta_s, data, hyp[0], hyp[1], hyp[2], 0.5 * hyp[3], 0.5 * hyp[4], want_hess=False)
        gb = b['grad'].copy()
        gb[2 * P + 2], gb[2 * P + 3] = 0.5 * gb[2 * P + 2], -0.5 / V ** 2 * gb[2 * P + 3]
        assert _rel(a['grad'], gb) < 1e-11
        out.append((a['value'], b['value']))
    da, db = out[1][0] - out[0][0], out[1][1] - out[0][1]
    assert abs(da) > 1e-3 and abs(da - db) <= 1e-11 * max(abs(out[0][0]), abs(out[1][0]))


@pytest.mark.parametrize('lik,N,P,K,G', SHAPES)
def test_border_tables_and_phases_reproduce_the_dense_solve(lik, N, P, K, G):
    """A0 + A1 . d_g, times the chain factors, is the closed part of the host border in free coordinates; and the three phases
    of the device-resident solve, restated in numpy exactly as the device holds them (C_g from the packed group sums and the two
    tables, L_g, U_g, the scaling s with ones on the closed columns), reproduce the dense solve and the group blocks."""
    from lrvb_amd import block_arrow as ba, glmm_slopes as gs
    gc, gid, free, eta, data, cf, targs = _setup(lik, N, P, K, G, seed=2)
    Kv, ng, D = ref.sizes(P, K, G)
    NC, K2 = gc.n_closed(K), 2 * K
    j1, j2, dense = _free_jac(P, K, G, eta, free)
    _, Hgg, rows, Hx, loc = ba.block_arrow_to_free(cf, j1, j2, ng, G, K, dense=dense)
    lam = max(0.0, -np.min(np.linalg.eigvalsh(ba.block_arrow_dense(Hgg, rows, Hx, loc)))) + 1.0
    Hgg, loc = Hgg + lam * np.eye(ng), loc + lam * np.eye(K2)[None]
    H = ba.block_arrow_dense(Hgg, rows, Hx, loc)
    m, ib, e_mu, i_mu, n, V, e, ig = gc._split_eta_corr(eta, P, K, G)
    r, d = 1.0 / ig, e - e_mu[None, :]
    Jc = np.eye(NC)
    Jc[K, K] = n - (K - 1.0)
    Jc[K + 1:, K + 1:] = dense[1]
    A0v, A1v = gc.glmm_corr_border_tables(K, n, V)
    A0, A1 = gc.glmm_corr_border_tables(K, n, V, Jc)
    assert A0.shape == (K2, NC) and A1.shape == (K2, K, NC)
    assert np.allclose(A0, A0v @ Jc, rtol=1e-15, atol=0) and np.allclose(A1, A1v @ Jc, rtol=1e-15, atol=0)
    jl = ba._to_groups(j1[ng:], G, K)[:, :, 0]
    scale = np.concatenate([jl[:, :K], -r * r * jl[:, K:]], axis=1)
    closed = (A0[None] + np.einsum('ilc,gl->gic', A1, d)) * scale[:, :, None]          # G x 2 K x NC
    want = Hx[2 * P:].reshape(NC, 2, G, K).transpose(2, 1, 3, 0).reshape(G, K2, NC)
    assert _rel(closed, want) < 1e-13
    # the device's C_g from the packed group sums (the column layout of include/lrvb_hip.h) and the tables
    nsc, ncol = gs.group_sums_ncol(P, K)
    bord = gs.pack_group_sums(data['g_loc'], data['loc'], data['border'])[:, nsc:]
    R = 2 * P + NC
    C = np.zeros((G, K2, R))
    for i in range(K2):
        k = i % K
        b_m, b_v = (0, 2) if i < K else (1, 3)
        C[:, i, :P] = bord[:, (b_m * K + k) * P:(b_m * K + k + 1) * P]
        C[:, i, P:2 * P] = bord[:, (b_v * K + k) * P:(b_v * K + k + 1) * P]
    C[:, :, 2 * P:] = A0[None] + np.einsum('ilc,gl->gic', A1, d)
    C *= scale[:, :, None]
    L = np.linalg.cholesky(loc)
    U = np.linalg.solve(L, C)
    s = np.concatenate([j1[:P], -j1[P:2 * P] / ib ** 2, np.ones(NC)])
    M = np.einsum('gir,gis->rs', U, U) * s[:, None] * s[None, :]
    Mref = ba.block_arrow_schur_term(rows, Hx, loc)
    assert _rel(M, Mref) < 1e-10
    S = Hgg.copy()
    S[np.ix_(rows, rows)] -= M
    state = {}

    def forward(Rl):
        assert Rl.shape[:2] == (G, K2) and Rl.flags['C_CONTIGUOUS']
        state['T'] = np.linalg.solve(L, Rl)
        return np.einsum('gir,giq->rq', U, state['T'])

    def back(xc):
        assert xc.shape[0] == R
        return np.linalg.solve(L.transpose(0, 2, 1), state['T'] - np.einsum('gir,rq->giq', U, xc))
    schur_solve = lambda rhs: np.linalg.solve(S, rhs)
    rng = np.random.default_rng(7)
    for Q in (1, 5):
        Rhs = rng.normal(size=(free.size, Q))
        X = ba.block_arrow_solve_by_phases(Rhs, ng, rows, s, forward, schur_solve, back)
        Xd = np.linalg.solve(H, Rhs)
        assert X.shape == Xd.shape and np.linalg.norm(X - Xd) <= 1e-10 * np.linalg.norm(Xd)
    v = rng.normal(size=free.size)
    xv = ba.block_arrow_solve_by_phases(v, ng, rows, s, forward, schur_solve, back)
    assert xv.shape == v.shape and np.linalg.norm(xv - np.linalg.solve(H, v)) <= 1e-10 * np.linalg.norm(xv)
    # the group blocks by phases, the holder's half restated from the same L_g, U_g
    chol = ba._local_chol(loc)
    cov_beta, buf = ba.block_arrow_group_cov_by_phases(ng, rows, P, K, s, schur_solve,
                                                       ba._host_group_blocks(chol, np.ascontiguousarray(U.transpose(2, 1, 0)), P, K,
                                                                             mu=2 * P + np.arange(K)), n_closed=NC)
    cu, cbu = ba.unpack_group_cov(buf, P, K)
    Hinv = np.linalg.inv(H)
    ie = ng + np.arange(G * K).reshape(G, K)
    assert _rel(cov_beta, Hinv[:P, :P]) < 1e-10
    for gi in range(G):
        assert _rel(cu[gi], Hinv[np.ix_(ie[gi], ie[gi])]) < 1e-10 and _rel(cbu[gi], Hinv[:P][:, ie[gi]]) < 1e-10


def test_reference_point_and_slopes_reference_share_the_data_term():
    """The reference's data term is that of tests/glmm_slopes_reference.py: with the closed terms removed (zero weights) the two
    KLs differ by what does not depend on the data."""
    N, P, K, G = 90, 3, 2, 4
    x, y, z, w, gid, o, free = ref.problem(N, P, K, G, 5)
    hyp = ref.other_hyp(K)
    eta = ref.free_to_vec(torch.tensor(free), P, K, G)
    Kv, ng, D = ref.sizes(P, K, G)
    eta_s = torch.cat([eta[:2 * P + 2 * K], torch.ones(2 * K, dtype=torch.float64), eta[ng:]])
    t = sref.tensors(x, y, z, w, gid)
    t0 = sref.tensors(x, y, z, 0.0 * w, gid)
    data_s = sref.kl_vec(eta_s, t[0], t[1], t[2], t[3], t[4], G, t[5]) - sref.kl_vec(eta_s, t0[0], t0[1], t0[2], t0[3], t0[4], G, t0[5])
    a = ref.kl_vec(eta, *ref.targs(x, y, z, w, o, gid, G, hyp))
    a0 = ref.kl_vec(eta, *ref.targs(x, y, z, 0.0 * w, o, gid, G, hyp))
    assert abs(float(a - a0) - float(data_s)) <= 1e-12 * abs(float(data_s))

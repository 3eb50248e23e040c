"""`block_arrow_solve_by_phases` (linearresponsevariationalbayes.py_amd/glmm_slopes.py) without a GPU.  The three phases of the
device-resident block-arrow solve are restated in numpy exactly as the device holds them -- C_g from the
group sums by the column layout of include/lrvb_hip.h, `scale` and `closed_rows` as `global_hessian` builds them, L_g, U_g -- and
the result is compared with a dense solve in free coordinates.  This pins the scaling s of the coupled rows and both layouts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glmm_slopes_reference as ref                                      # noqa: E402

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0
SHAPES = [(3, 2, 5), (5, 3, 7), (8, 1, 4)]                               # P, K, G


def _device_restatement(gs, P, K, G, eta, j1, data, loc_f):
    """(s, forward, back, M) as the device forms them: everything below reads the packed G x ncol group sums."""
    ng, K2 = 2 * P + 4 * K, 2 * K
    nsc, ncol = gs.group_sums_ncol(P, K)
    gsum = gs.pack_group_sums(data['g_loc'], data['loc'], data['border'])
    assert gsum.shape == (G, ncol)
    # global_hessian: the chain factors of the local coordinates and the closed-form border entries
    _, ib, e_mu, _, a, b, e, ig = gs._split_eta(eta, P, K, G)
    r = 1.0 / ig
    d = e - e_mu[None, :]
    ta, tb = 1.0 / b, -a / b ** 2
    closed = np.zeros((G, K2, 3))
    closed[:, :K, 0], closed[:, :K, 1], closed[:, :K, 2] = -(a / b)[None, :], d * ta[None, :], d * tb[None, :]
    closed[:, K:, 1], closed[:, K:, 2] = 0.5 * ta[None, :], 0.5 * tb[None, :]
    jl = gs._to_groups(j1[ng:], G, K)[:, :, 0]
    scale = np.concatenate([jl[:, :K], -r * r * jl[:, K:]], axis=1)
    # the kernel's C_g (2 K x R): row e_gk = f [b = 0 | b = 2 | closed in the columns of k], row r_gk = f [b = 1 | b = 3 | closed]
    R = 2 * P + 3 * K
    C = np.zeros((G, K2, R))
    bord = gsum[:, nsc:]
    for i in range(K2):
        k = i % K
        b_m, b_v = (0, 2) if i < K else (1, 3)
        C[:, i, :P] = bord[:, (b_m * K + k) * P:(b_m * K + k + 1) * P]
        C[:, i, P:2 * P] = bord[:, (b_v * K + k) * P:(b_v * K + k + 1) * P]
        C[:, i, 2 * P + 3 * k:2 * P + 3 * k + 3] = closed[:, i]
    C *= scale[:, :, None]
    L = np.linalg.cholesky(loc_f)
    U = np.linalg.solve(L, C)
    dv = np.concatenate([np.ones(P), -1.0 / ib ** 2, np.ones(3 * K)])
    s = j1[gs.coupled_rows(P, K)] * dv
    state = {}

    def forward(Rl):
        assert Rl.shape[:2] == (G, K2) and Rl.flags['C_CONTIGUOUS']
        state['T'] = np.linalg.solve(L, Rl)
        return np.einsum('gir,giq->rq', U, state['T'])

    def back(xc):
        assert xc.shape[0] == R
        return np.linalg.solve(L.transpose(0, 2, 1), state['T'] - np.einsum('gir,rq->giq', U, xc))
    return s, forward, back, np.einsum('gir,gis->rs', U, U)


@pytest.mark.parametrize('P,K,G', SHAPES)
def test_phases_reproduce_the_dense_solve(P, K, G):
    from lrvb_amd import glmm_slopes as gs
    N = 60 + 9 * G
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=0)
    mask = ref.positive_mask(P, K, G)
    eta = np.where(mask, np.exp(free), free)
    data = ref.data_pieces(x, y, z, w, gid, G, eta)
    cf = gs.glmm_slopes_closed_forms(P, K, G, eta, data, *HYP)
    ng = 2 * P + 4 * K
    j1, j2 = np.where(mask, eta, 1.0), np.where(mask, eta, 0.0)
    _, Hgg, rows, Hx, loc = gs.block_arrow_to_free(cf, j1, j2, ng, G, K)
    assert np.array_equal(rows, gs.coupled_rows(P, K))
    H = gs.block_arrow_dense(Hgg, rows, Hx, loc)
    s, forward, back, M = _device_restatement(gs, P, K, G, eta, j1, data, loc)
    # the border of the free-coordinate Hessian is s_r C_g[l, r]: the Schur term in free coordinates is (s s^T) o M
    S = Hgg.copy()
    S[np.ix_(rows, rows)] -= M * s[:, None] * s[None, :]
    Sref = Hgg.copy()
    Sref[np.ix_(rows, rows)] -= gs.block_arrow_schur_term(rows, Hx, loc)
    assert np.max(np.abs(S - Sref)) <= 1e-10 * np.max(np.abs(Sref))
    schur_solve = lambda rhs: np.linalg.solve(S, rhs)
    rng = np.random.default_rng(7)
    for Q in (1, 5):
        R = rng.normal(size=(free.size, Q))
        X = gs.block_arrow_solve_by_phases(R, ng, rows, s, forward, schur_solve, back)
        Xd = np.linalg.solve(H, R)
        assert X.shape == Xd.shape
        assert np.linalg.norm(X - Xd) <= 1e-10 * np.linalg.norm(Xd)
    v = rng.normal(size=free.size)
    xv = gs.block_arrow_solve_by_phases(v, ng, rows, s, forward, schur_solve, back)
    assert xv.shape == v.shape and np.linalg.norm(xv - np.linalg.solve(H, v)) <= 1e-10 * np.linalg.norm(xv)
    with pytest.raises(ValueError):
        gs.block_arrow_solve_by_phases(v[:-1], ng, rows, s, forward, schur_solve, back)

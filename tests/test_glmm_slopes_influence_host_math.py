"""Host side of the streamed weight influence of `LogisticGLMMSlopesObjective`, without a GPU: the row
formula of `lrvb_glmm_slopes_obs_influence` restated in numpy on the two operand layouts of `split_influence_operand`, against
torch autograd of tests/glmm_slopes_reference.py with respect to the weights (1e-9 relative, the project's tolerance for influence
rows), and the operand route -block_arrow_solve(C_w) against the dense solve at a point where the reference Hessian is positive
definite (rtol 1e-6, atol 1e-12: a quantity behind an H^-1)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glmm_slopes_reference as ref                                      # noqa: E402

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def rows_numpy(x, y, z, gid, G, eta, A_global, A_local, gh_deg=20):
    """out[n][q] = a1' (x_n . A_m[q] + sum_k z_nk A_e[q, g(n), k]) + a2' ((x_n o x_n) . A_v[q] + sum_k z_nk^2 A_r[q, g(n), k]) from
    A_global (Q x 2 P) and A_local (G x 2 K x Q); a1' = psi_rho - y and a2' = psi_s per unit weight by the reference's psi."""
    P, K = x.shape[1], z.shape[1]
    c = ref.row_coefs(x, y, z, np.ones(x.shape[0]), gid, G, eta, gh_deg)
    al = A_local[gid]                                                    # N x 2 K x Q
    lin = x @ A_global[:, :P].T + np.einsum('nk,nkq->nq', z, al[:, :K])
    quad = (x * x) @ A_global[:, P:].T + np.einsum('nk,nkq->nq', z * z, al[:, K:])
    return c['a1'][:, None] * lin + c['a2'][:, None] * quad


def rows_autograd(x, y, z, w, gid, G, eta, A):
    """N x Q: column q is the derivative with respect to the weights of A[q] . (gradient of the reference in (m, v, e, r))."""
    P, K = x.shape[1], z.shape[1]
    ng, GK = 2 * P + 4 * K, G * K
    t = ref.tensors(x, y, z, w, gid, HYP)
    c = torch.tensor(np.concatenate([eta[:P], 1.0 / eta[P:2 * P], eta[ng:ng + GK], 1.0 / eta[ng + GK:]]), requires_grad=True)
    wt = t[3].clone().requires_grad_(True)
    et = torch.cat([c[:P], 1.0 / c[P:2 * P], torch.tensor(eta[2 * P:ng]), c[2 * P:2 * P + GK], 1.0 / c[2 * P + GK:]])
    g, = torch.autograd.grad(ref.kl_vec(et, t[0], t[1], t[2], wt, t[4], G, t[5]), c, create_graph=True)
    return np.stack([torch.autograd.grad(g @ torch.tensor(A[q]), wt, retain_graph=True)[0].numpy() for q in range(A.shape[0])], axis=1)


@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 5, 4, 2)])
def test_row_formula_and_operand_layouts_against_autograd(N, P, K, G):
    from lrvb_amd import glmm_slopes as gs
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=N + P + K)
    eta = np.where(ref.positive_mask(P, K, G), np.exp(free), free)
    Q = 7
    A = np.random.default_rng(N).normal(size=(Q, 2 * P + 2 * G * K))
    Ag, Al = gs.split_influence_operand(A, P, K, G)
    assert Ag.shape == (Q, 2 * P) and Al.shape == (G, 2 * K, Q) and Ag.flags.c_contiguous and Al.flags.c_contiguous
    for g in range(G):
        for k in range(K):
            assert np.array_equal(Al[g, k], A[:, 2 * P + g * K + k]) and np.array_equal(Al[g, K + k], A[:, 2 * P + G * K + g * K + k])
    got = rows_numpy(x, y, z, gid, G, eta, Ag, Al)
    want = rows_autograd(x, y, z, w, gid, G, eta, A)
    assert got.shape == (N, Q) and _rel(got, want) < 1e-9
    with pytest.raises(ValueError):
        gs.split_influence_operand(A[:, :-1], P, K, G)


def _optimum(free, targs, iters=60):
    """Damped Newton on the reference in free coordinates, to a point where its Hessian is positive definite."""
    th = free.copy()
    for _ in range(iters):
        val, g, H = ref.value_grad_hess(ref.kl_free, th, targs)
        if np.max(np.abs(g)) < 1e-9:
            break
        lam = max(0.0, 1e-3 - np.min(np.linalg.eigvalsh(H)))
        step = np.linalg.solve(H + lam * np.eye(th.size), g)
        t = 1.0
        while t > 1e-8 and not ref.value_grad_hess(ref.kl_free, th - t * step, targs, want_hess=False)[0] < val:
            t *= 0.5
        th = th - t * step
    return th


def test_block_arrow_solve_of_the_weight_cross_hessian_matches_the_dense_solve():
    from lrvb_amd import glmm_slopes as gs
    N, P, K, G = 400, 3, 2, 6
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=77, big_group=False, empty_group=False)
    w = np.ones(N)
    t = ref.tensors(x, y, z, w, gid, HYP)
    targs = (t[0], t[1], t[2], t[3], t[4], G, t[5])
    th = _optimum(np.zeros(free.size), targs)
    _, g_ad, H_ad = ref.value_grad_hess(ref.kl_free, th, targs)
    assert np.max(np.abs(g_ad)) < 1e-6 and np.min(np.linalg.eigvalsh(H_ad)) > 0        # on the REFERENCE
    wt = t[3].clone().requires_grad_(True)
    p = torch.tensor(th).requires_grad_(True)
    g, = torch.autograd.grad(ref.kl_free(p, t[0], t[1], t[2], wt, t[4], G, t[5]), p, create_graph=True)
    Cw = np.stack([torch.autograd.grad(g[k], wt, retain_graph=True)[0].numpy() for k in range(g.numel())])
    mask = ref.positive_mask(P, K, G)
    eta = np.where(mask, np.exp(th), th)
    cf = gs.glmm_slopes_closed_forms(P, K, G, eta, ref.data_pieces(x, y, z, w, gid, G, eta), *HYP)
    j1, j2 = np.where(mask, eta, 1.0), np.where(mask, eta, 0.0)
    _, Hgg, rows, Hx, loc = gs.block_arrow_to_free(cf, j1, j2, 2 * P + 4 * K, G, K)
    got = -gs.block_arrow_solve(Hgg, rows, Hx, loc, Cw)
    want = -np.linalg.solve(H_ad, Cw)
    assert got.shape == (free.size, N)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-12)

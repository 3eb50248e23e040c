"""The host algebra of `group_cov` / `predict` without a GPU: `block_arrow_group_cov`, `predict_rows` and the
phase driver `block_arrow_group_cov_by_phases` (linearresponsevariationalbayes.py_amd/block_arrow.py).

  1. Random symmetric positive definite block arrows, K = 1..4, P = 1 included, one group without data (its border holds only
     the closed-form columns): the three blocks against the same blocks of a dense inverse (`dense_reference.refined_solve`), and
     the row formula against c^T H^-1 c for the dense moment vector c = (x at m, z at e_g) -- a population row has z on the
     e_mu columns.
  2. The phase driver with numpy callables that hold the factor as the device does -- L_g, U_g = L_g^-1 C_g in the device's
     coordinates, the scaling s of the coupled rows, the (G + 1) x (K K + K P) buffer -- on the pieces of the real model.  This
     pins s, W and both layouts.

Bound: the entries of a block of H^-1, relative to the block's largest entry, within kappa_2(H) D 2^-53 -- the first-order forward
bound of a Cholesky solve (eps kappa) with D for the length of the sums."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_reference as dref                                           # noqa: E402
import glmm_slopes_reference as ref                                      # noqa: E402

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)
SHAPES = [(3, 1, 5), (1, 2, 4), (5, 3, 6), (4, 4, 3)]                    # P, K, G


def _random_arrow(gs, P, K, G, rng):
    """(Hgg, rows, Hx, loc) of a positive definite block arrow; the last group has no data columns in its border."""
    ng, R = 2 * P + 4 * K, 2 * P + 3 * K
    rows = gs.coupled_rows(P, K)
    A = rng.normal(size=(ng, ng))
    Hgg = A @ A.T
    B = rng.normal(size=(G, 2 * K, 2 * K))
    loc = B @ B.transpose(0, 2, 1) + 0.5 * np.eye(2 * K)
    Hx = rng.normal(size=(R, 2 * G * K))
    li = gs._local_index(G, K)
    Hx[:2 * P, li[G - 1]] = 0.0
    H = gs.block_arrow_dense(Hgg, rows, Hx, loc)
    shift = max(0.0, -np.min(np.linalg.eigvalsh(H))) + 1.0
    Hgg = Hgg + shift * np.eye(ng)
    loc = loc + shift * np.eye(2 * K)
    return Hgg, rows, Hx, loc


def _rel(got, want):
    want = np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)) / np.max(np.abs(want)))


def _dense_blocks(Hinv, P, K, G):
    ng = 2 * P + 4 * K
    ie = ng + np.arange(G * K).reshape(G, K)
    mu = 2 * P + np.arange(K)
    cu = np.stack([Hinv[np.ix_(ie[g], ie[g])] for g in range(G)] + [Hinv[np.ix_(mu, mu)]])
    cbu = np.stack([Hinv[:P][:, ie[g]] for g in range(G)] + [Hinv[:P][:, mu]])
    return Hinv[:P, :P], cu, cbu


def _check_blocks(got, Hinv, P, K, G, bound, what):
    want = _dense_blocks(Hinv, P, K, G)
    for name, a, b in zip(('cov_beta', 'cov_u', 'cov_beta_u'), got, want):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        blocks = [(a, b)] if a.ndim == 2 else list(zip(a, b))
        err = max(_rel(x, y) for x, y in blocks)
        print('%s %s: max block error %.3e, bound %.3e' % (what, name, err, bound))
        assert err <= bound


def _moment_rows(x, z, gid, P, K, G):
    """The dense moment vectors c_n (n x D): x on the columns of m, z on e_g -- on e_mu for the pseudo-group G."""
    ng = 2 * P + 4 * K
    C = np.zeros((x.shape[0], ng + 2 * G * K))
    C[:, :P] = x
    for n, g in enumerate(gid):
        cols = 2 * P + np.arange(K) if g == G else ng + g * K + np.arange(K)
        C[n, cols] = z[n]
    return C


@pytest.mark.parametrize('P,K,G', SHAPES)
def test_blocks_and_rows_against_a_dense_inverse(P, K, G):
    from lrvb_amd import glmm_slopes as gs
    rng = np.random.default_rng(100 * P + 10 * K + G)
    Hgg, rows, Hx, loc = _random_arrow(gs, P, K, G, rng)
    H = gs.block_arrow_dense(Hgg, rows, Hx, loc)
    D = H.shape[0]
    Hinv = dref.refined_solve(H, np.eye(D))
    bound = float(np.linalg.cond(H)) * D * 2.0 ** -53
    got = gs.block_arrow_group_cov(Hgg, rows, Hx, loc, P, K, population=True)
    _check_blocks(got, Hinv, P, K, G, bound, 'random arrow (P, K, G) = %s:' % ((P, K, G),))
    short = gs.block_arrow_group_cov(Hgg, rows, Hx, loc, P, K)
    assert short[1].shape == (G, K, K) and short[2].shape == (G, P, K)
    assert np.array_equal(short[1], got[1][:G]) and np.array_equal(short[2], got[2][:G]) and np.array_equal(short[0], got[0])
    # the empty group: its blocks are not those of any other group, and they are compared above like every other
    n = 40
    x, z = rng.normal(size=(n, P)), rng.normal(size=(n, K))
    gid = rng.integers(0, G, size=n)
    gid[:6] = G                                                          # population rows
    gid[6:10] = G - 1                                                    # rows in the group without data
    ng = 2 * P + 4 * K
    m, v = rng.normal(size=P), rng.uniform(0.5, 2.0, size=P)
    e, r = rng.normal(size=(G + 1, K)), rng.uniform(0.5, 2.0, size=(G + 1, K))
    off = rng.normal(size=n)
    rho, s_mf, v_lr = gs.predict_rows(x, z, gid, off, m, v, e, r, *got)
    assert np.allclose(rho, off + x @ m + np.sum(z * e[gid], axis=1), rtol=1e-13, atol=1e-13)
    assert np.allclose(s_mf, (x * x) @ v + np.sum(z * z * r[gid], axis=1), rtol=1e-13, atol=0)
    C = _moment_rows(x, z, gid, P, K, G).astype(np.longdouble)
    want = np.einsum('nd,de,ne->n', C, Hinv, C)
    scale = np.einsum('nd,de,ne->n', np.abs(C), np.abs(Hinv), np.abs(C))
    err = float(np.max(np.abs(v_lr - want) / scale))
    print('rows: max error relative to sum |terms| %.3e, bound %.3e' % (err, bound))
    assert err <= bound
    assert np.all(v_lr > 0.0)
    assert np.array_equal(gs.predict_rows(x, z, gid, None, m, v, e, r, *got)[0] + off, rho)


def _device_holder(gs, P, K, G, eta, j1, data, loc_f):
    """(s, L, U) as the device holds them (tests/test_glmm_slopes_device_solve_host_math.py): C_g from the packed group sums by the
    column layout of include/lrvb_hip.h, scaled by the chain factors; U_g = L_g^-1 C_g."""
    ng, K2 = 2 * P + 4 * K, 2 * K
    nsc, ncol = gs.group_sums_ncol(P, K)
    gsum = gs.pack_group_sums(data['g_loc'], data['loc'], data['border'])
    _, ib, e_mu, _, a, b, e, ig = gs._split_eta(eta, P, K, G)
    r = 1.0 / ig
    d = e - e_mu[None, :]
    ta, tb = 1.0 / b, -a / b ** 2
    closed = np.zeros((G, K2, 3))
    closed[:, :K, 0], closed[:, :K, 1], closed[:, :K, 2] = -(a / b)[None, :], d * ta[None, :], d * tb[None, :]
    closed[:, K:, 1], closed[:, K:, 2] = 0.5 * ta[None, :], 0.5 * tb[None, :]
    jl = gs._to_groups(j1[ng:], G, K)[:, :, 0]
    scale = np.concatenate([jl[:, :K], -r * r * jl[:, K:]], axis=1)
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
    return j1[gs.coupled_rows(P, K)] * dv, L, U


def _device_group_blocks(L, U, P, K):
    """lrvb_glmm_slopes_group_cov in numpy, group by group, in the layout of its buffer."""
    G = L.shape[0]

    def group_blocks(W, s):
        assert W.shape == (2 * P + 3 * K,) * 2 and W.flags['C_CONTIGUOUS']
        buf = np.empty((G + 1, K * K + K * P))
        for g in range(G):
            Y = np.linalg.solve(L[g].T, U[g] * s[None, :])[:K]               # the rows of e_g.
            E = Y @ W
            Ai = np.linalg.inv(L[g] @ L[g].T)[:K, :K]
            buf[g, :K * K] = (Ai + E @ Y.T).ravel()
            buf[g, K * K:] = (-E[:, :P]).ravel()                           # k-major, the P values contiguous
        mu = 2 * P + 3 * np.arange(K)
        buf[G, :K * K], buf[G, K * K:] = W[np.ix_(mu, mu)].ravel(), W[mu, :P].ravel()
        return buf
    return group_blocks


@pytest.mark.parametrize('P,K,G', [(3, 2, 5), (5, 3, 7), (1, 4, 4), (8, 1, 4)])
def test_phase_driver_with_the_device_layouts(P, K, G):
    from lrvb_amd import glmm_slopes as gs
    N = 60 + 9 * G
    x, y, z, w, gid, free = ref.problem(N, P, K, G, seed=0)
    assert not np.any(gid == G - 1)                                       # the empty group: its block is prior-only
    mask = ref.positive_mask(P, K, G)
    eta = np.where(mask, np.exp(free), free)
    data = ref.data_pieces(x, y, z, w, gid, G, eta)
    cf = gs.glmm_slopes_closed_forms(P, K, G, eta, data, *HYP)
    ng = 2 * P + 4 * K
    j1, j2 = np.where(mask, eta, 1.0), np.where(mask, eta, 0.0)
    _, Hgg, rows, Hx, loc = gs.block_arrow_to_free(cf, j1, j2, ng, G, K)
    H = gs.block_arrow_dense(Hgg, rows, Hx, loc)
    D = H.shape[0]
    Hinv = dref.refined_solve(H, np.eye(D))
    bound = float(np.linalg.cond(H)) * D * 2.0 ** -53
    s, L, U = _device_holder(gs, P, K, G, eta, j1, data, loc)
    assert np.any(s != 1.0)
    S = Hgg.copy()
    S[np.ix_(rows, rows)] -= np.einsum('gir,gis->rs', U, U) * s[:, None] * s[None, :]
    cov_beta, buf = gs.block_arrow_group_cov_by_phases(ng, rows, P, K, s, lambda rhs: np.linalg.solve(S, rhs),
                                                       _device_group_blocks(L, U, P, K))
    assert buf.shape == (G + 1, K * K + K * P)
    got = (cov_beta,) + gs.unpack_group_cov(buf, P, K)
    _check_blocks(got, Hinv, P, K, G, bound, 'phases (P, K, G) = %s:' % ((P, K, G),))
    host = gs.block_arrow_group_cov(Hgg, rows, Hx, loc, P, K, population=True)
    _check_blocks(host, Hinv, P, K, G, bound, 'host   (P, K, G) = %s:' % ((P, K, G),))
    with pytest.raises(ValueError):
        gs.block_arrow_group_cov_by_phases(ng, rows, P, K, s[:-1], None, None)

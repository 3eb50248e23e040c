"""The intercept's `glmm.arrow_*` functions are adapters over the K-generic `block_arrow` module at K = 1: here they are held
against the 2 x 2 closed forms written out below (inverse by determinant, the explicit [ee ei; ei ii] scatter) to 1e-12 relative --
the local blocks have correlation at most 0.8 and diagonals in [1, 2], a condition number below about 20, so both routes carry
a few units of rounding.  Also the refusals (a non-positive pivot in any row of the recurrence, an indefinite Schur complement) and
the sparse export against the dense one.  Host numpy only: no GPU."""
import numpy as np
import pytest

from lrvb_amd import glmm, block_arrow as ba
from helpers import rel_err

TOL = 1e-12


def _inverse(loc):
    det = loc[:, 0] * loc[:, 2] - loc[:, 1] ** 2
    return loc[:, 2] / det, -loc[:, 1] / det, loc[:, 0] / det


def _schur_term(Hx, loc):
    G = loc.shape[0]
    i11, i12, i22 = _inverse(loc)
    Ce, Ci = Hx[:, :G], Hx[:, G:]
    return (Ce * i11) @ Ce.T + (Ci * i22) @ Ci.T + (Ce * i12) @ Ci.T + (Ci * i12) @ Ce.T


def _pieces(P, G, seed):
    """The generator of test_glmm_influence_host_math._pieces, the Schur term by the closed form above."""
    rng = np.random.default_rng(seed)
    ng = 2 * P + 4
    rows = np.concatenate([np.arange(2 * P), [2 * P, 2 * P + 2, 2 * P + 3]])
    Hx = rng.normal(size=(rows.size, 2 * G)) * 0.3
    a = rng.uniform(1.0, 2.0, size=G)
    c = rng.uniform(1.0, 2.0, size=G)
    b = rng.uniform(-0.8, 0.8, size=G) * np.sqrt(a * c)
    loc = np.stack([a, b, c], axis=1)
    Z = rng.normal(size=(ng, ng))
    Hgg = Z @ Z.T / ng + np.eye(ng)
    Hgg[np.ix_(rows, rows)] += _schur_term(Hx, loc)
    return Hgg, rows, Hx, loc


def _dense(Hgg, rows, Hx, loc):
    ng, G = Hgg.shape[0], loc.shape[0]
    H = np.zeros((ng + 2 * G, ng + 2 * G))
    H[:ng, :ng] = Hgg
    H[rows, ng:] = Hx
    H[ng:, rows] = Hx.T
    ie, ii = np.arange(ng, ng + G), np.arange(ng + G, ng + 2 * G)
    H[ie, ie], H[ie, ii], H[ii, ie], H[ii, ii] = loc[:, 0], loc[:, 1], loc[:, 1], loc[:, 2]
    return H


def _solve(Hgg, rows, Hx, loc, R):
    """Block elimination with the 2 x 2 inverses by determinant."""
    ng, G = Hgg.shape[0], loc.shape[0]
    i11, i12, i22 = (t[:, None] for t in _inverse(loc))
    Rg, Re, Ri = R[:ng], R[ng:ng + G], R[ng + G:]
    te, ti = i11 * Re + i12 * Ri, i12 * Re + i22 * Ri
    rhs = Rg.copy()
    rhs[rows] -= Hx[:, :G] @ te + Hx[:, G:] @ ti
    S = Hgg.copy()
    S[np.ix_(rows, rows)] -= _schur_term(Hx, loc)
    xg = np.linalg.solve(S, rhs)
    ce, ci = Hx[:, :G].T @ xg[rows], Hx[:, G:].T @ xg[rows]
    return np.vstack([xg, te - (i11 * ce + i12 * ci), ti - (i12 * ce + i22 * ci)])


@pytest.mark.parametrize('P,G', [(1, 1), (3, 7), (8, 40)])
def test_intercept_adapters_match_the_2x2_closed_forms(P, G):
    Hgg, rows, Hx, loc = _pieces(P, G, seed=10 * P + G)
    ng = Hgg.shape[0]
    rng = np.random.default_rng(P)
    # local solve and Schur term: inverse by determinant
    be, bi = rng.normal(size=G), rng.normal(size=G)
    i11, i12, i22 = _inverse(loc)
    se, si = glmm.arrow_local_solve(loc, be, bi)
    assert rel_err(np.concatenate([se, si]), np.concatenate([i11 * be + i12 * bi, i12 * be + i22 * bi])) < TOL
    assert rel_err(glmm.arrow_schur_term(rows, Hx, loc), _schur_term(Hx, loc)) < TOL
    # dense matrix and product: the explicit scatter (both local layouts give the same matrix)
    H = _dense(Hgg, rows, Hx, loc)
    assert np.array_equal(glmm.arrow_dense(Hgg, rows, Hx, loc), H)
    blocks = np.stack([np.stack([loc[:, 0], loc[:, 1]], axis=1), np.stack([loc[:, 1], loc[:, 2]], axis=1)], axis=1)
    assert np.array_equal(glmm.arrow_dense(Hgg, rows, Hx, blocks), H)
    v = rng.normal(size=ng + 2 * G)
    assert rel_err(glmm.arrow_matvec(Hgg, rows, Hx, loc, v), H @ v) < TOL
    # solve: a matrix of right-hand sides and a vector
    R = rng.normal(size=(ng + 2 * G, 3))
    want = _solve(Hgg, rows, Hx, loc, R)
    got = glmm.arrow_solve(Hgg, rows, Hx, loc, R)
    assert got.shape == want.shape and rel_err(got, want) < TOL
    one = glmm.arrow_solve(Hgg, rows, Hx, loc, R[:, 0])
    assert one.shape == (ng + 2 * G,) and rel_err(one, want[:, 0]) < TOL


def test_refusals():
    Hgg, rows, Hx, loc = _pieces(3, 7, seed=4)
    R = np.ones((Hgg.shape[0] + 14, 2))
    negative = loc.copy()
    negative[5, 0] = -1.0                                                # loc[g, 0] < 0
    indefinite = loc.copy()
    indefinite[2, 1] = 1.5 * np.sqrt(loc[2, 0] * loc[2, 2])              # a negative determinant
    for bad in (negative, indefinite):
        with pytest.raises(np.linalg.LinAlgError):
            glmm.arrow_schur_term(rows, Hx, bad)
        with pytest.raises(np.linalg.LinAlgError):
            glmm.arrow_solve(Hgg, rows, Hx, bad, R)
    Hbad = Hgg.copy()
    Hbad[0, 0] -= 50.0                                                   # the local blocks are fine, the Schur complement is not
    with pytest.raises(np.linalg.LinAlgError):
        glmm.arrow_solve(Hbad, rows, Hx, loc, R)


@pytest.mark.parametrize('K', [2, 4])
@pytest.mark.parametrize('row', ['first', 'last'])
def test_one_non_positive_pivot_is_refused(K, row):
    """All pivots of all blocks are positive except one, in the first or the last row of the recurrence, of one group."""
    n, G = 2 * K, 5
    rng = np.random.default_rng(K)
    L = np.tril(rng.normal(size=(G, n, n)) * 0.3, -1) + np.eye(n)[None]
    D = np.ones((G, n))
    loc = np.einsum('gik,gk,gjk->gij', L, D, L)
    assert ba._local_chol(loc)[0].shape == (n, n, G)
    D[3, 0 if row == 'first' else n - 1] = -0.5                          # L D L^T: the pivots of the Cholesky recurrence are D
    loc = np.einsum('gik,gk,gjk->gij', L, D, L)
    Hx = rng.normal(size=(4, 2 * G * K))
    with pytest.raises(np.linalg.LinAlgError):
        ba.block_arrow_schur_term(np.arange(4), Hx, loc)
    with pytest.raises(np.linalg.LinAlgError):
        ba.block_arrow_solve(np.eye(6), np.arange(4), Hx, loc, np.ones(6 + 2 * G * K))
    with pytest.raises(np.linalg.LinAlgError):
        ba.block_arrow_local_solve(loc, np.ones((G, n)))


@pytest.mark.parametrize('K', [1, 2, 4])
def test_sparse_export_equals_the_dense_one(K):
    P, G = 3, 6
    rng = np.random.default_rng(20 + K)
    ng, R = 2 * P + 4 * K, 2 * P + 3 * K
    rows = np.sort(rng.choice(ng, size=R, replace=False))
    Hx = rng.normal(size=(R, 2 * G * K))
    Hx[:, 1] = 0.0                                                       # structural zeros of the border are not stored
    Z = rng.normal(size=(G, 2 * K, 2 * K))
    loc = Z @ Z.transpose(0, 2, 1)
    Hgg = rng.normal(size=(ng, ng))
    Hgg = Hgg + Hgg.T
    S = ba.block_arrow_sparse(Hgg, rows, Hx, loc)
    assert S.format == 'csr' and S.nnz == ng * ng + 2 * R * (2 * G * K - 1) + G * 4 * K * K
    assert np.array_equal(S.toarray(), ba.block_arrow_dense(Hgg, rows, Hx, loc))

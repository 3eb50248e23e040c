"""`glmm.arrow_solve`: H^-1 R for the arrow Hessian of `LogisticGLMMObjective` from its pieces (global block, coupled rows,
border, G local 2 x 2 blocks), against `np.linalg.solve` on `arrow_dense` of the same pieces.  Host numpy only: no GPU."""
import numpy as np
import pytest

from lrvb_amd import glmm
from helpers import rel_err


def _pieces(P, G, seed, zero_border_group=None):
    """A random symmetric positive definite arrow: Hgg (n_global^2), the 2 P + 3 coupled rows, Hx and loc (G x 3)."""
    rng = np.random.default_rng(seed)
    ng = 2 * P + 4
    rows = np.concatenate([np.arange(2 * P), [2 * P, 2 * P + 2, 2 * P + 3]])
    Hx = rng.normal(size=(rows.size, 2 * G)) * 0.3
    if zero_border_group is not None:
        Hx[:, zero_border_group] = 0.0
        Hx[:, G + zero_border_group] = 0.0
    a = rng.uniform(1.0, 2.0, size=G)
    c = rng.uniform(1.0, 2.0, size=G)
    b = rng.uniform(-0.8, 0.8, size=G) * np.sqrt(a * c)                   # not diagonal: psi_rho_s couples e_g and i_g
    loc = np.stack([a, b, c], axis=1)
    Z = rng.normal(size=(ng, ng))
    Hgg = Z @ Z.T / ng + np.eye(ng)
    Hgg[np.ix_(rows, rows)] += glmm.arrow_schur_term(rows, Hx, loc)       # the Schur complement is Z Z^T / ng + I
    return Hgg, rows, Hx, loc


@pytest.mark.parametrize('P,G,zero', [(3, 7, 2), (1, 1, None), (1, 5, 0), (6, 1, None), (8, 40, 11)])
@pytest.mark.parametrize('Q', [1, 3, 20])
def test_arrow_solve_matches_the_dense_solve(P, G, zero, Q):
    Hgg, rows, Hx, loc = _pieces(P, G, seed=100 * P + G, zero_border_group=zero)
    H = glmm.arrow_dense(Hgg, rows, Hx, loc)
    assert np.min(np.linalg.eigvalsh(H)) > 0
    R = np.random.default_rng(Q).normal(size=(H.shape[0], Q))
    want = np.linalg.solve(H, R)
    got = glmm.arrow_solve(Hgg, rows, Hx, loc, R)
    assert got.shape == want.shape
    assert rel_err(got, want) < 1e-10
    # residual through the arrow product, column by column
    for q in range(Q):
        assert rel_err(glmm.arrow_matvec(Hgg, rows, Hx, loc, got[:, q]), R[:, q]) < 1e-10
    if Q == 1:                                                           # a plain vector comes back as one
        v = glmm.arrow_solve(Hgg, rows, Hx, loc, R[:, 0])
        assert v.shape == (H.shape[0],) and rel_err(v, want[:, 0]) < 1e-10


def test_a_schur_solver_from_outside_replaces_the_host_factor():
    Hgg, rows, Hx, loc = _pieces(4, 9, seed=5)
    H = glmm.arrow_dense(Hgg, rows, Hx, loc)
    S = Hgg.copy()
    S[np.ix_(rows, rows)] -= glmm.arrow_schur_term(rows, Hx, loc)
    calls = []

    def schur_solve(B):
        calls.append(B.shape)
        return np.linalg.solve(S, B)
    R = np.random.default_rng(1).normal(size=(H.shape[0], 3))
    got = glmm.arrow_solve(Hgg, rows, Hx, loc, R, schur_solve=schur_solve)
    assert calls == [(Hgg.shape[0], 3)]
    assert rel_err(got, np.linalg.solve(H, R)) < 1e-10


def test_indefinite_pieces_raise():
    Hgg, rows, Hx, loc = _pieces(3, 6, seed=9)
    R = np.ones((Hgg.shape[0] + 12, 2))
    bad = loc.copy()
    bad[4, 1] = 1.5 * np.sqrt(bad[4, 0] * bad[4, 2])                     # det < 0
    with pytest.raises(np.linalg.LinAlgError):
        glmm.arrow_solve(Hgg, rows, Hx, bad, R)
    bad = loc.copy()
    bad[0, 0] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        glmm.arrow_solve(Hgg, rows, Hx, bad, R)
    Hbad = Hgg.copy()
    Hbad[0, 0] -= 50.0                                                   # the local blocks are fine, the Schur complement is not
    with pytest.raises(np.linalg.LinAlgError):
        glmm.arrow_solve(Hbad, rows, Hx, loc, R)

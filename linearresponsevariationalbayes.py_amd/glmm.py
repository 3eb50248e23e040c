"""Logistic mixed model with a random intercept:

    y_n ~ Bernoulli(sigma(x_n . beta + u_{g(n)})),   u_g ~ N(mu, 1 / tau),   n = 1..N,  g = 0..G-1

with q(beta) = UVNParamVector(P), q(mu) = UVNParam, q(tau) = GammaParam, q(u) = UVNParamVector(G), the group effects pushed
last.  Vector coordinates eta = [m (P) | i_beta (P) | e_mu, i_mu | a, b | e (G) | i (G)], n_global = 2 P + 4.

    KL(eta) =  sum_n w_n [ psi(rho_n, s_n) - y_n rho_n ]        rho_n = x_n . m + e_g(n),  s_n = (x_n o x_n) . (1 / i_beta) + 1 / i_g(n)
             + 1/2 E tau ( sum_g [(e_g - e_mu)^2 + 1 / i_g] + G / i_mu ) - 1/2 G E log tau
             + 1/2 tau_beta sum_j (m_j^2 + 1 / i_beta_j)
             + 1/2 kappa0 ((e_mu - mu0)^2 + 1 / i_mu)
             - (a0 - 1) E log tau + b0 E tau
             + 1/2 sum_j log i_beta_j + 1/2 log i_mu + 1/2 sum_g log i_g - gamma_entropy(a, b)

(the Gaussian entropies up to their additive constants, as `LogitNormalRegressionObjective` keeps them).  The O(N) work --
the quadrature per row, the per-group segmented sums of the arrow's border and local blocks, the three weighted products of
the global block -- is `lrvb_glmm_terms` (csrc/k_glmm.hip); everything N-independent is `glmm_closed_forms` below, plain
numpy on the data pieces, so it is testable without a GPU.  The Hessian is an arrow: a dense global block, G local 2 x 2
blocks (NOT diagonal: psi_rho_s couples e_g and i_g) and a border of 2 P + 3 coupled global rows (i_mu does not couple).

This is the model of glmm_slopes.py at K = 1 with the unit group design, and the host code says so: the functions below are
adapters over `glmm_slopes_closed_forms` and block_arrow.py that keep the G x 3 layout [ee, ei, ii] of the local blocks, and the
class is `_LogisticMixedModel` on the intercept's own device entries.
"""
import numpy as np

from .block_arrow import (block_arrow_to_free, block_arrow_matvec, block_arrow_dense, block_arrow_schur_term,
                          block_arrow_local_solve, block_arrow_solve)
from .glmm_slopes import _LogisticMixedModel, glmm_slopes_closed_forms


def _blocks(loc):
    """The local blocks as G x 2 x 2 from either layout: G x 3 ([ee, ei, ii]) or G x 2 x 2."""
    loc = np.asarray(loc, dtype=np.float64)
    return loc if loc.ndim == 3 else loc[:, [[0, 1], [1, 2]]]


def _triples(loc):
    """Inverse of `_blocks`: G x 3."""
    return np.stack([loc[:, 0, 0], loc[:, 0, 1], loc[:, 1, 1]], axis=1)


def glmm_closed_forms(P, G, eta, data, tau_beta, mu0, kappa0, a0, b0, want_hess=True):
    """The N-independent part of the model, in VECTOR coordinates, from the data-dependent pieces: `glmm_slopes_closed_forms` at K = 1.

    eta: [m | i_beta | e_mu, i_mu | a, b | e | i].  data: dict of the data term in the coordinates (m, v = 1 / i_beta, e,
    r = 1 / i): 'value', 'g_glob' (2 P: d/dm, d/dv), 'g_loc' (G x 2: sum_g a1, sum_g a2), and for the Hessian 'Hb' (3 x P x P:
    mm, mv, vv), 'border' (G x 4 P: sum c11 x | sum c12 x | sum c12 x o x | sum c22 x o x) and 'loc' (G x 3: sum c11, c12, c22).

    Returns dict: 'value', 'grad' (V), and with want_hess 'Hgg' (n_global x n_global), 'rows' (the 2 P + 3 coupled global
    coordinates), 'Hx' ((2 P + 3) x 2 G, columns [e_0..e_G-1 | i_0..i_G-1]) and 'loc' (G x 3: ee, ei, ii of each local block).
    """
    d = dict(data)
    if d.get('loc') is not None:
        d['loc'] = _blocks(d['loc'])
    if d.get('border') is not None:
        d['border'] = np.asarray(d['border']).reshape(G, 4, P)
    out = glmm_slopes_closed_forms(P, 1, G, eta, d, tau_beta, mu0, kappa0, a0, b0, want_hess=want_hess)
    if 'loc' in out:
        out['loc'] = _triples(out['loc'])
    return out


def arrow_to_free(cf, j1, j2, n_global, G):
    """The pieces of `glmm_closed_forms` in FREE coordinates for an element-wise packing (j1 = d eta / d theta, j2 = its second
    derivative, both V-vectors): (grad, Hgg, rows, Hx, loc)."""
    g, Hgg, rows, Hx, loc = block_arrow_to_free(dict(cf, loc=_blocks(cf['loc'])), j1, j2, n_global, G, 1)
    return g, Hgg, rows, Hx, _triples(loc)


def arrow_matvec(Hgg, rows, Hx, loc, v):
    """H v for the arrow (global block, border rows, G local 2 x 2 blocks): O(n_global^2 + P G)."""
    return block_arrow_matvec(Hgg, rows, Hx, _blocks(loc), v)


def arrow_dense(Hgg, rows, Hx, loc):
    return block_arrow_dense(Hgg, rows, Hx, _blocks(loc))


def arrow_schur_term(rows, Hx, loc):
    """M = sum_g C_g A_g^-1 C_g^T on the coupled rows (host route; the device route is lrvb_glmm_schur)."""
    return block_arrow_schur_term(rows, Hx, _blocks(loc))


def arrow_local_solve(loc, be, bi):
    """A_g^-1 [be_g; bi_g] for every group."""
    s = block_arrow_local_solve(_blocks(loc), np.stack([be, bi], axis=1))
    return s[:, 0], s[:, 1]


def arrow_solve(Hgg, rows, Hx, loc, R, schur_solve=None):
    """H^-1 R for the arrow (R: D x Q or a D-vector, D = n_global + 2 G) without the dense matrix, by `block_arrow_solve`.  A local
    block or a Schur complement that is not positive definite raises `np.linalg.LinAlgError`."""
    return block_arrow_solve(Hgg, rows, Hx, _blocks(loc), R, schur_solve=schur_solve)


class LogisticGLMMObjective(_LogisticMixedModel):
    """The mixed model with one effect per group and the unit group design, on its own kernels over the rows (csrc/k_glmm.hip)."""

    def __init__(self, par, x, y, groups, n_groups, beta_prior_info=1.0, mu_prior=(0.0, 1.0), tau_prior=(1.0, 1.0), gh_deg=20,
                 names=('beta', 'mu', 'tau', 'u'), weights=None, device=0):
        super().__init__(par, x, y, None, groups, n_groups, beta_prior_info, mu_prior, tau_prior, gh_deg, names, weights, device)

    def _layout(self, par, names):
        """[beta (mean, info) | mu (mean, info) | tau (shape, rate) | u (mean, info)]: mu is a UVNParam, tau one GammaParam."""
        P, G = self.P, self.G
        ng = 2 * P + 4
        want = [(names[0], 'mean', 0, P), (names[0], 'info', P, 2 * P), (names[1], 'mean', 2 * P, 2 * P + 1),
                (names[1], 'info', 2 * P + 1, 2 * P + 2), (names[2], 'shape', 2 * P + 2, 2 * P + 3),
                (names[2], 'rate', 2 * P + 3, ng), (names[3], 'mean', ng, ng + G), (names[3], 'info', ng + G, ng + 2 * G)]
        msg = ('the parameter must be [UVNParamVector {} ({}) | UVNParam {} | GammaParam {} | UVNParamVector {} ({})] '
               'in this order, the group effects pushed last'.format(names[0], P, names[1], names[2], names[3], G))
        return want, msg, 'the parameter holds more than the four blocks of the model'

    # ---- the device entries, in the K = 1 layouts of the shared code ----------------------------------------------------------
    def _terms(self, *point, **want):
        """Everything, for `local_stats`: the group sums stacked as [g_loc 2 | loc 3 | border 4 P], the layout at K = 1."""
        val, gg, gl, Hb, B, L = self.ctx.glmm_terms(*point, **want)
        return val, gg, Hb, np.hstack([gl, L, B])

    def _device_terms(self, eta, want_grad, want_hess, want_border=True):
        """The evaluation path hands on the arrays the entry filled, unstacked: no G x (5 + 4 P) copy per evaluation."""
        val, gg, gl, Hb, B, L = self.ctx.glmm_terms(*self._point(eta), want_grad=want_grad or want_hess, want_hess=want_hess,
                                                    want_border=want_border)
        return dict(value=val, g_glob=gg, g_loc=gl, Hb=Hb, loc=None if L is None else _blocks(L),
                    border=None if B is None else B.reshape(self.G, 4, self.P))

    def _schur(self, local_blocks, border_scale, closed_rows):
        return self.ctx.glmm_schur(local_blocks, border_scale, closed_rows.reshape(self.G, 6))

    def _obs_influence(self, *point_and_operand, **window):
        return self.ctx.glmm_obs_influence(*point_and_operand, **window)

    def _group_influence(self, *point_and_operand):
        return self.ctx.glmm_group_influence(*point_and_operand)

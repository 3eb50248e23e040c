"""Independent fp64 torch reference of `OrdinalGLMMObjective`, shared by the CPU and GPU tests, laid out like
tests/glmm_censnormal_reference.py.

The prior and entropy terms are `glmm_slopes_reference.kl_vec` with zero weights.  The data term is

    sum_n w_n E h_n(t),   t ~ N(rho_n, s_n),   rho_n = o_n + x_n . m + z_n . e_g(n),
    h(t; lo, hi) = -logsigmoid(hi - t) - logsigmoid(t - lo) - log(-expm1(-(hi - lo))),   lo = alpha_y, hi = alpha_{y+1},

on the CLASS'S OWN nodes (gh_deg of them: the quadrature is part of the model's definition, as for the logistic model), with
`torch.nn.functional.logsigmoid`; an end category has no third term and its missing cut point is +-inf.  That this h equals the
single expression -log(sigma(hi - t) - sigma(lo - t)) is checked against mpmath at 40 digits in
tests/test_glmm_ordinal_host_math.py; the single expression itself loses every digit in the right tail and is no reference.

Derivatives in t AND in the thresholds alpha are nested autograd passes of that expression -- none of the hand forms of the model
(sigma', sigma'', 1 / expm1(D), e^-D / expm1(-D)^2) appears anywhere -- and derivatives in (rho, s) are defined by Stein's identity on
the same nodes (`_EH`).  alpha is an argument of `data`, so `threshold_terms` has a reference by autograd in alpha.

Against mpmath the reference meets the 1e-10 cap on the GRID stated below; every GPU data set lies inside it (asserted in
tests/test_glmm_ordinal_host_math.py).

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import numpy as np
import torch
import torch.nn.functional as F

import glmm_binomial_reference as bref
import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)
from glmm_ztpoisson_reference import _rule

GH_DEG = 20
# The grid on which `expected_h` (orders 0 to 4) meets 1e-10 of max(1, |exact|) against mpmath quadrature: (rho - lo, rho - hi) the
# row's position against its two cut points (an end category has one of them), s its variance, D = hi - lo.
GRID = dict(dist=(-12.0, 12.0), s=(0.0, 3.0), delta=(2.0 ** -6, 16.0))


def table(alpha):
    inf = torch.full((1,), float('inf'), dtype=torch.float64)
    return torch.cat([-inf, alpha, inf])


def h_row(t, lo, hi):
    """h(t; lo, hi) elementwise; lo = -inf or hi = +inf on an end category."""
    interior = torch.isfinite(lo) & torch.isfinite(hi)
    D = torch.where(interior, hi - lo, torch.ones_like(t + lo))
    return -F.logsigmoid(hi - t) - F.logsigmoid(t - lo) - torch.where(interior, torch.log(-torch.expm1(-D)), torch.zeros_like(D))


def _partial(t, lo, hi, k):
    """d_t^k h elementwise by k nested autograd passes, differentiable in lo and hi where they require it."""
    with torch.enable_grad():
        tt = t.detach().requires_grad_(True)
        h = h_row(tt, lo, hi)
        for _ in range(k):
            h, = torch.autograd.grad(h.sum(), tt, create_graph=True)
    return h


def expected_h(mu, s, lo, hi, k, deg=GH_DEG):
    """E d_t^k h at t ~ N(mu, s); lo, hi one value per row (differentiable: a graph through alpha is kept)."""
    t, wts = _rule(mu, s, deg)
    return (_partial(t, lo[:, None], hi[:, None], k) * wts[None, :]).sum(1)


class _EH(torch.autograd.Function):
    """E d_t^k h, differentiated in (mu, s) by Stein's identity on the same nodes and in (lo, hi) by autograd of the row expression."""
    @staticmethod
    def forward(ctx, mu, s, lo, hi, deg, k):
        ctx.save_for_backward(mu, s, lo, hi)
        ctx.deg, ctx.k = deg, k
        return expected_h(mu, s, lo, hi, k, deg).detach()

    @staticmethod
    def backward(ctx, go):
        mu, s, lo, hi = ctx.saved_tensors
        k, deg = ctx.k, ctx.deg
        need = ctx.needs_input_grad
        g_lo = g_hi = None
        if need[2] or need[3]:
            g_lo, g_hi = _EB.apply(mu, s, lo, hi, deg, k)
        return (go * _EH.apply(mu, s, lo, hi, deg, k + 1) if need[0] else None,
                go * 0.5 * _EH.apply(mu, s, lo, hi, deg, k + 2) if need[1] else None,
                go * g_lo if need[2] else None, go * g_hi if need[3] else None, None, None)


def _bound_derivs(mu, s, lo, hi, deg, k, orders):
    """E d_t^k d_lo^a d_hi^b h for (a, b) in orders, by nested autograd in detached copies of lo and hi (a sentinel's derivative is 0)."""
    with torch.enable_grad():
        l = lo.detach().requires_grad_(True)
        u = hi.detach().requires_grad_(True)
        out = []
        for a, b in orders:
            e = expected_h(mu.detach(), s.detach(), l, u, k, deg)
            for var in [l] * a + [u] * b:
                if not e.requires_grad:
                    e = torch.zeros_like(mu)
                    continue
                g, = torch.autograd.grad(e.sum(), var, create_graph=True, allow_unused=True)
                e = torch.zeros_like(mu) if g is None else g
            out.append(torch.nan_to_num(e.detach(), nan=0.0))
    return out


class _EB(torch.autograd.Function):
    """(d_lo, d_hi) of E d_t^k h, themselves differentiable once more in (mu, s) by Stein's identity and in (lo, hi) by autograd."""
    @staticmethod
    def forward(ctx, mu, s, lo, hi, deg, k):
        ctx.save_for_backward(mu, s, lo, hi)
        ctx.deg, ctx.k = deg, k
        return tuple(_bound_derivs(mu, s, lo, hi, deg, k, [(1, 0), (0, 1)]))

    @staticmethod
    def backward(ctx, g_lo, g_hi):
        mu, s, lo, hi = ctx.saved_tensors
        k, deg = ctx.k, ctx.deg
        l1, u1 = _bound_derivs(mu, s, lo, hi, deg, k + 1, [(1, 0), (0, 1)])
        l2, u2 = _bound_derivs(mu, s, lo, hi, deg, k + 2, [(1, 0), (0, 1)])
        ll, lu, uu = _bound_derivs(mu, s, lo, hi, deg, k, [(2, 0), (1, 1), (0, 2)])
        return (g_lo * l1 + g_hi * u1, 0.5 * (g_lo * l2 + g_hi * u2), g_lo * ll + g_hi * lu, g_lo * lu + g_hi * uu, None, None)


def data(eta, x, y, z, w, o, alpha, gid, G, deg=GH_DEG):
    """The data term; y the categories (a long tensor), alpha the T thresholds (differentiable)."""
    rho, s = bref._rho_s(eta, x, z, o, gid, G)
    tab = table(alpha)
    return (w * _EH.apply(rho, s, tab[y], tab[y + 1], deg, 0)).sum()


def _priors(eta, x, z, w, gid, G, hyp):
    return sref.kl_vec(eta, x, torch.zeros_like(w), z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_vec(eta, x, y, z, w, o, alpha, gid, G, hyp, deg=GH_DEG):
    return data(eta, x, y, z, w, o, alpha, gid, G, deg) + _priors(eta, x, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, alpha, gid, G, hyp, deg=GH_DEG):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, alpha, gid, G, hyp, deg)


def targs(x, y, z, w, o, alpha, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """The arguments of `kl_vec` / `kl_free` behind the point."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    return (t(x), torch.tensor(np.asarray(y, dtype=np.int64)), t(z), t(w), t(o), t(alpha), torch.tensor(np.asarray(gid, dtype=np.int64)), G,
            t(hyp), deg)


def weight_cross(free, t):
    """d2 data / d free d w^T (D x N, numpy): column n is the gradient of row n's term per unit weight, by autograd in the weights."""
    x, y, z, w, o, al, gid, G, hyp, deg = t
    fr = torch.tensor(np.asarray(free, dtype=np.float64), requires_grad=True)
    ww = w.clone().requires_grad_(True)
    f = data(free_to_vec(fr, x.shape[1], z.shape[1], G), x, y, z, ww, o, al, gid, G, deg)
    g, = torch.autograd.grad(f, fr, create_graph=True)
    return torch.stack([torch.autograd.grad(g[i], ww, retain_graph=True)[0] for i in range(g.numel())]).numpy()


def threshold_terms(free, t, alpha=None):
    """(g (T), H (T x T), cross (D x T) in free coordinates of theta) of the data term in the thresholds alpha, by autograd."""
    x, y, z, w, o, al, gid, G, hyp, deg = t
    al = (al if alpha is None else torch.tensor(np.asarray(alpha, dtype=np.float64))).clone().requires_grad_(True)
    fr = torch.tensor(np.asarray(free, dtype=np.float64), requires_grad=True)
    f = data(free_to_vec(fr, x.shape[1], z.shape[1], G), x, y, z, w, o, al, gid, G, deg)
    g, = torch.autograd.grad(f, al, create_graph=True)
    H, cross = [], []
    for j in range(al.numel()):
        hj, cj = torch.autograd.grad(g[j], (al, fr), retain_graph=True, allow_unused=True)
        H.append(torch.zeros_like(al) if hj is None else hj)
        cross.append(torch.zeros_like(fr) if cj is None else cj)
    return g.detach().numpy(), torch.stack(H).numpy(), torch.stack(cross, dim=1).numpy()


SHAPES = [(1, 1, 1, 1), (37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7)]
BARE = (37, 3, 1, 5)
TEST_HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                     # the priors the GPU tests run with (tests/test_gpu_glmm_slopes.py, HYP)
J_OF = {(1, 1, 1, 1): 3, (37, 3, 1, 5): 2, (65, 5, 2, 3): 5, (130, 64, 4, 2): 16, (300, 17, 4, 7): 5}
GRID_UNIT = 2.0 ** -20                                                   # alpha and o are multiples of it: a common shift up to 2^32 keeps them exact


def thresholds_for(J):
    """J - 1 increasing cut points on the grid 2^-20, spread over about [-1.6, 2.0] with unequal spacings."""
    T = J - 1
    a = -1.6 + 3.6 * (np.arange(T) + 0.5 * np.sin(np.arange(T))) / max(T, 1) if T > 1 else np.array([0.3])
    a = np.round(np.sort(a) / GRID_UNIT) * GRID_UNIT
    assert np.all(np.diff(a) > 2.0 ** -6)
    return a


def problem(N, P, K, G, seed, J, zero_weights=False, empty_category=None, **kw):
    """x, z, w, gid, o and the point of `glmm_binomial_reference.problem`; the thresholds of `thresholds_for(J)`; y drawn from the
    cumulative logit law at o + x beta + z . u.  empty_category: a category whose rows are moved to the next one.  o is rounded to
    multiples of 2^-20.  Returns (x, y (ints), z, w, gid, o, alpha, free)."""
    x, _, z, w, gid, o, _, free = bref.problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 47])
    alpha = thresholds_for(J)
    o = np.round(o / GRID_UNIT) * GRID_UNIT
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    t = o + x @ beta + (z * u[gid]).sum(1)
    lat = t + rng.logistic(size=N)
    y = np.searchsorted(alpha, lat).astype(np.int64)                      # y = #{j: alpha_j < latent}
    if N >= J:
        y[:J] = np.arange(J)                                             # every category present, both end categories among them
    if empty_category is not None:
        y[y == empty_category] = empty_category + 1
    if zero_weights:
        w = w.copy()
        w[::5] = 0.0
    return x, y, z, w, gid, o, alpha, free


def shape_data(N, P, K, G):
    """The data set of a test shape, seed N + P + K: J of J_OF, every fifth weight zero at N = 300, category 2 empty at N = 65, and for
    BARE the unit design with a zero offset."""
    x, y, z, w, gid, o, alpha, free = problem(N, P, K, G, N + P + K, J_OF[(N, P, K, G)], zero_weights=(N == 300),
                                              empty_category=2 if N == 65 else None)
    if (N, P, K, G) == BARE:
        o = np.zeros(N)
        assert np.array_equal(z, np.ones((N, 1)))
    return x, y, z, w, gid, o, alpha, free


def rows_at(free, x, y, z, o, alpha, gid, G):
    """(rho, s, lo, hi) of every row at the free-coordinate point `free` (numpy): what a row's term depends on."""
    P, K = x.shape[1], z.shape[1]
    eta = np.where(positive_mask(P, K, G), np.exp(free), free)
    ng = 2 * P + 4 * K
    e, ig = eta[ng:ng + G * K].reshape(G, K), eta[ng + G * K:].reshape(G, K)
    rho = o + x @ eta[:P] + (z * e[gid]).sum(1)
    s = (x * x) @ (1.0 / eta[P:2 * P]) + (z * z * (1.0 / ig)[gid]).sum(1)
    tab = np.concatenate([[-np.inf], np.asarray(alpha, dtype=np.float64), [np.inf]])
    return rho, s, tab[y], tab[y + 1]


def inside_grid(rho, s, lo, hi):
    """Whether every row lies inside GRID: rho - lo and rho - hi (where the cut point is finite), s and D = hi - lo."""
    d = np.concatenate([(rho - lo)[np.isfinite(lo)], (rho - hi)[np.isfinite(hi)]])
    D = (hi - lo)[np.isfinite(lo) & np.isfinite(hi)]
    return bool(d.min() >= GRID['dist'][0] and d.max() <= GRID['dist'][1] and s.min() >= GRID['s'][0] and s.max() <= GRID['s'][1]
                and (D.size == 0 or (D.min() >= GRID['delta'][0] and D.max() <= GRID['delta'][1])))


def _t(a):
    return torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)))


def eh_coefs(rho, s, lo, hi, deg=GH_DEG):
    """E h^(k), k = 0..4 (5 x n, numpy) by the reference's rule."""
    rho, s, lo, hi = (_t(a) for a in np.broadcast_arrays(rho, s, lo, hi))
    return np.stack([expected_h(rho, s, lo, hi, k, deg).detach().numpy() for k in range(5)])

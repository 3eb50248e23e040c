"""Independent fp64 torch reference of `CensoredNormalGLMMObjective`, shared by the CPU and GPU tests, laid
out like tests/glmm_gamma_reference.py.

The prior and entropy terms are `glmm_slopes_reference.kl_vec` with zero weights.  The data term is

    sum_n w_n E h_n(t),   t ~ N(rho_n, s_n),   rho_n = o_n + x_n . m + z_n . e_g(n),   phi_n = e^lambda phi0_n,
    status 0:    h(t) = phi (y - t)^2 / 2            on the 96-node Gauss-Hermite rule, which is exact for a quadratic -- NOT the closed
                                                     form phi ((y - rho)^2 + s) / 2 that the model and its kernels use;
    status +-1:  h(t) = -log Phi(delta sqrt(phi) (t - y))   by `torch.special.log_ndtr` on the CLASS'S OWN nodes (gh_deg of them): the
                                                     quadrature is part of the model's definition there, as for the probit link.

Derivatives in t are k nested autograd passes of those two expressions -- no inverse Mills ratio, no erfcx, no continued fraction
anywhere -- and derivatives in (rho, s) are defined by Stein's identity on the same nodes (`_EH`).  The row term is also
differentiable in lambda (j nested passes), which gives the reference of `dispersion_terms`.

Against mpmath (tests/test_glmm_censnormal_host_math.py) the reference meets the 1e-10 cap on the grid stated there; every GPU data
set lies inside it.

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import numpy as np
import torch

import glmm_binomial_reference as bref
import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)
from glmm_ztpoisson_reference import _rule

GH_OBS = 96                                                              # observed rows: exact for the quadratic
GH_DEG = 20                                                              # censored rows: the model's own rule (its default gh_deg)
LOG_2PI_HALF = 0.9189385332046727


def h_observed(phi, y, t, lam):
    return 0.5 * (phi * torch.exp(lam)) * (y - t) ** 2


def h_censored(phi, y, delta, t, lam):
    return -torch.special.log_ndtr(delta * torch.sqrt(phi * torch.exp(lam)) * (t - y))


def _partial(fn, t, lam, k, j):
    """d_t^k d_lambda^j fn(t, lambda) elementwise, by k + j nested autograd passes; a derivative that no longer depends on its
    variable is an exact zero."""
    with torch.enable_grad():
        tt = t.detach().requires_grad_(True)
        ll = (torch.zeros_like(t) + lam.detach()).requires_grad_(True)
        h = fn(tt, ll)
        for var in [tt] * k + [ll] * j:
            if not h.requires_grad:
                h = torch.zeros_like(t)
                continue
            g, = torch.autograd.grad(h.sum(), var, create_graph=True, allow_unused=True)
            h = torch.zeros_like(t) if g is None else g
    return h.detach()


def expected_h(mu, s, phi, y, st, lam, k, j=0, deg=GH_DEG):
    """E d_t^k d_lambda^j h at t ~ N(mu, s); phi, y and the status st (a float tensor of -1, 0, +1) one value per row, lam a scalar."""
    obs = st == 0.0
    t, wts = _rule(mu, s, GH_OBS)
    eo = (_partial(lambda tt, ll: h_observed(phi[:, None], y[:, None], tt, ll), t, lam, k, j) * wts[None, :]).sum(1)
    t, wts = _rule(mu, s, deg)
    delta = torch.where(obs, torch.ones_like(st), st)                   # an observed row's node sum is not read; keep it finite
    ec = (_partial(lambda tt, ll: h_censored(phi[:, None], y[:, None], delta[:, None], tt, ll), t, lam, k, j) * wts[None, :]).sum(1)
    return torch.where(obs, eo, ec)


class _EH(torch.autograd.Function):
    """E d_t^k d_lambda^j h, differentiated in (mu, s) by Stein's identity on the same nodes and in lambda by one more pass, to any order."""
    @staticmethod
    def forward(ctx, mu, s, lam, phi, y, st, deg, k, j):
        ctx.save_for_backward(mu, s, lam, phi, y, st)
        ctx.deg, ctx.k, ctx.j = deg, k, j
        return expected_h(mu, s, phi, y, st, lam, k, j, deg)

    @staticmethod
    def backward(ctx, go):
        mu, s, lam, phi, y, st = ctx.saved_tensors
        k, j, deg = ctx.k, ctx.j, ctx.deg
        need = ctx.needs_input_grad
        return (go * _EH.apply(mu, s, lam, phi, y, st, deg, k + 1, j) if need[0] else None,
                go * 0.5 * _EH.apply(mu, s, lam, phi, y, st, deg, k + 2, j) if need[1] else None,
                (go * _EH.apply(mu, s, lam, phi, y, st, deg, k, j + 1)).sum() if need[2] else None, None, None, None, None, None, None)


def data(eta, x, y, z, w, o, phi, gid, G, st, deg=GH_DEG, lam=None):
    rho, s = bref._rho_s(eta, x, z, o, gid, G)
    lam = torch.zeros((), dtype=torch.float64) if lam is None else lam
    return (w * _EH.apply(rho, s, lam, phi, y, st, deg, 0, 0)).sum()


def _priors(eta, x, y, z, w, gid, G, hyp):
    return sref.kl_vec(eta, x, y, z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_vec(eta, x, y, z, w, o, phi, gid, G, hyp, st, deg=GH_DEG):
    return data(eta, x, y, z, w, o, phi, gid, G, st, deg) + _priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, phi, gid, G, hyp, st, deg=GH_DEG):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, phi, gid, G, hyp, st, deg)


def targs(x, y, z, w, o, phi, gid, G, st, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """The arguments of `kl_vec` / `kl_free` behind the point; st: the status per row, or None for all observed."""
    st = np.zeros(len(y)) if st is None else np.asarray(st, dtype=np.float64)
    return bref.targs(x, y, z, w, o, phi, gid, G, hyp) + (torch.tensor(st), deg)


def log_norm_const(phi, w, st, lam=0.0):
    """sum over the observed rows of w [log(phi) / 2 - log(2 pi) / 2] (numpy), what the value drops."""
    o = np.asarray(st) == 0
    return float(np.sum(w[o] * (0.5 * (np.log(phi[o]) + lam) - LOG_2PI_HALF)))


def dispersion_terms(free, t):
    """(F_lambda, F_lambda,lambda, J_lambda in free coordinates) of F = data - log_norm_const at lambda = 0 by autograd in lambda;
    t = `targs(..)`."""
    x, y, z, w, o, phi, gid, G, hyp, st, deg = t
    fr = torch.tensor(np.asarray(free, dtype=np.float64), requires_grad=True)
    lam = torch.zeros((), dtype=torch.float64, requires_grad=True)
    eta = free_to_vec(fr, x.shape[1], z.shape[1], G)
    f = data(eta, x, y, z, w, o, phi, gid, G, st, deg, lam) - 0.5 * lam * w[st == 0.0].sum()
    d1, = torch.autograd.grad(f, lam, create_graph=True)
    d2, = torch.autograd.grad(d1, lam, retain_graph=True)
    cross, = torch.autograd.grad(d1, fr)
    return float(d1.detach()), float(d2.detach()), cross.numpy()


SHAPES = [(1, 1, 1, 1), (37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7)]
BARE = (37, 3, 1, 5)
TEST_HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                     # the priors the GPU tests run with (tests/test_gpu_glmm_slopes.py, HYP)
MODES = ('mixed', 'observed', 'censored')
PHI_LO, PHI_HI = 0.25, 16.0
Y_GRID = 2.0 ** -20                                                      # y and o are multiples of it: a common shift up to 2^32 keeps them exact


def problem(N, P, K, G, seed, phi=2.0, mode='mixed', zero_weights=False, **kw):
    """x, z, w, gid, o and the point of `glmm_binomial_reference.problem`; phi a scalar, or 'vector' for one value per row,
    log-uniform on [0.25, 16] with both ends present (N >= 2); the latent y* drawn from N(o + x beta + z . u, 1 / phi).  The status:
    'observed' all 0; 'censored' every row +1 or -1 (alternating); 'mixed' about 30 % censored, left and right, at a censoring point
    drawn within 1.5 sd of the latent value on the side the status says.  y and o are rounded to multiples of 2^-20, so that
    (y + c, o + c) is exact for the shifts of the tests.  Returns (x, y, z, w, gid, o, phi (N), st (N ints), free)."""
    x, _, z, w, gid, o, _, free = bref.problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 45])
    if isinstance(phi, str):
        ph = np.exp(rng.uniform(np.log(PHI_LO), np.log(PHI_HI), size=N))
        if N >= 2:
            ph[0], ph[-1] = PHI_LO, PHI_HI
    else:
        ph = np.full(N, float(phi))
    o = np.round(o / Y_GRID) * Y_GRID
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    sd = 1.0 / np.sqrt(ph)
    ystar = o + x @ beta + (z * u[gid]).sum(1) + sd * rng.normal(size=N)
    if mode == 'observed':
        st = np.zeros(N, dtype=np.int32)
    elif mode == 'censored':
        st = np.where(np.arange(N) % 2 == 0, 1, -1).astype(np.int32)
    else:
        draw = rng.uniform(size=N)
        st = np.where(draw < 0.15, -1, np.where(draw < 0.30, 1, 0)).astype(np.int32)
        if N >= 3:
            st[0], st[1], st[2] = 1, -1, 0
    gap = sd * rng.uniform(0.0, 1.5, size=N)
    y = ystar - st * gap                                                 # right-censored: the bound lies below the latent value
    y = np.round(y / Y_GRID) * Y_GRID
    if zero_weights:
        w = w.copy()
        w[::5] = 0.0
    return x, y, z, w, gid, o, ph, st, free


def shape_data(N, P, K, G, mode='mixed'):
    """The data set of a test shape, seed N + P + K: phi = 2 below N = 130 and one value per row from there, every fifth weight zero
    at N = 300, and for BARE the unit design with a zero offset."""
    x, y, z, w, gid, o, ph, st, free = problem(N, P, K, G, N + P + K, phi='vector' if N >= 130 else 2.0, mode=mode, zero_weights=(N == 300))
    if (N, P, K, G) == BARE:
        o = np.zeros(N)
        assert np.array_equal(z, np.ones((N, 1)))
    return x, y, z, w, gid, o, ph, st, free


def _t(a):
    return torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)))


def eh_coefs(rho, s, y, phi, st, deg=GH_DEG, lam=0.0):
    """E h^(k), k = 0..4 (5 x n, numpy) by the reference's rule."""
    rho, s, y, phi, st = (_t(a) for a in np.broadcast_arrays(rho, s, y, phi, np.asarray(st, dtype=np.float64)))
    lam = torch.tensor(float(lam), dtype=torch.float64)
    return np.stack([expected_h(rho, s, phi, y, st, lam, k, 0, deg).numpy() for k in range(5)])


def eh_dispersion(rho, s, y, phi, st, deg=GH_DEG):
    """(E h_l, E d_t h_l, E d_t^2 h_l, E h_ll) (4 x n, numpy) by the reference's rule: autograd in lambda."""
    rho, s, y, phi, st = (_t(a) for a in np.broadcast_arrays(rho, s, y, phi, np.asarray(st, dtype=np.float64)))
    lam = torch.zeros((), dtype=torch.float64)
    return np.stack([expected_h(rho, s, phi, y, st, lam, k, j, deg).numpy() for k, j in ((0, 1), (1, 1), (2, 1), (0, 2))])

"""Independent fp64 torch reference of `GammaGLMMObjective`, shared by the CPU and GPU tests, laid out like
tests/glmm_beta_reference.py.

The prior and entropy terms are `glmm_slopes_reference.kl_vec` with zero weights.  The data term is

    sum_n w_n E h(t),   t ~ N(rho_n, s_n),   rho_n = o_n + x_n . m + z_n . e_g(n),   h(t) = phi (y e^{-t} + t) = phi (exp(log y - t) + t)

on the `deg`-node Gauss-Hermite rule, deg = 96 -- NOT the closed form exp(log y - rho + s / 2) that the model and its kernels use, so
that the reference is independent of the code under test.  Its derivatives are defined by Stein's identity on the same nodes
(`_EH`), h^(k) being taken by k nested autograd passes of torch.exp.

The rule integrates e^{-t} against the Gaussian: with a = sqrt(2 s) the node sum of exp(-a x) against sqrt(pi) e^{a^2 / 4}.  Against
mpmath the 96-node rule holds 2e-14 of every E h^(k) for s <= 100 (measured in tests/test_glmm_gamma_host_math.py; 3e-8 at
s = 200, where it has left the 1e-10 cap) WHATEVER rho and y: the factor exp(log y - rho) stands outside the sum.  The data sets of
`shape_data` have s below 2.5, and the tests that widen the variances check the identities of the kernels, not this reference.

Coordinates, `positive_mask`, `free_to_vec` and `value_grad_hess` are those of glmm_slopes_reference."""
import numpy as np
import torch

import glmm_binomial_reference as bref
import glmm_slopes_reference as sref
from glmm_slopes_reference import positive_mask, free_to_vec, value_grad_hess          # noqa: F401  (re-exported for the tests)
from glmm_ztpoisson_reference import dk, _rule

GH_DEG = 96


def h_of(phi, ly):
    """h(.; phi, log y) as a function of t."""
    def h(t):
        return phi * (torch.exp(ly - t) + t)
    return h


def expected_h(mu, s, phi, ly, k, deg=GH_DEG):
    """E h^(k) at t ~ N(mu, s) on the nodes; phi and ly = log y one value per row."""
    t, wts = _rule(mu, s, deg)
    return (dk(h_of(phi[:, None], ly[:, None]), t, k) * wts[None, :]).sum(1)


class _EH(torch.autograd.Function):
    """E h^(k), differentiated in (mu, s) by Stein's identity on the same nodes, to any order."""
    @staticmethod
    def forward(ctx, mu, s, phi, ly, deg, k):
        ctx.save_for_backward(mu, s, phi, ly)
        ctx.deg, ctx.k = deg, k
        return expected_h(mu, s, phi, ly, k, deg)

    @staticmethod
    def backward(ctx, go):
        mu, s, phi, ly = ctx.saved_tensors
        return (go * _EH.apply(mu, s, phi, ly, ctx.deg, ctx.k + 1), go * 0.5 * _EH.apply(mu, s, phi, ly, ctx.deg, ctx.k + 2),
                None, None, None, None)


def data(eta, x, y, z, w, o, phi, gid, G, deg=GH_DEG):
    """y: the responses themselves, strictly positive."""
    rho, s = bref._rho_s(eta, x, z, o, gid, G)
    return (w * _EH.apply(rho, s, phi, torch.log(y), deg, 0)).sum()


def _priors(eta, x, y, z, w, gid, G, hyp):
    return sref.kl_vec(eta, x, y, z, torch.zeros_like(w), gid, G, hyp, 1)


def kl_vec(eta, x, y, z, w, o, phi, gid, G, hyp, deg=GH_DEG):
    return data(eta, x, y, z, w, o, phi, gid, G, deg) + _priors(eta, x, y, z, w, gid, G, hyp)


def kl_free(free, x, y, z, w, o, phi, gid, G, hyp, deg=GH_DEG):
    return kl_vec(free_to_vec(free, x.shape[1], z.shape[1], G), x, y, z, w, o, phi, gid, G, hyp, deg)


def targs(x, y, z, w, o, phi, gid, G, hyp=(1.0, 0.0, 1.0, 1.0, 1.0), deg=GH_DEG):
    """The arguments of `kl_vec` / `kl_free` behind the point; o is the offset on the log scale."""
    return bref.targs(x, y, z, w, o, phi, gid, G, hyp) + (deg,)


def log_norm_const(y, phi, w):
    """sum w [phi log phi - lgamma(phi) + (phi - 1) log y] (numpy), what the value drops."""
    from scipy.special import gammaln
    return float(np.sum(w * (phi * np.log(phi) - gammaln(phi) + (phi - 1.0) * np.log(y))))


PROBES = (1e-12, 1e12, 1.0)
PHI_LO, PHI_HI = 0.05, 1e4


def problem(N, P, K, G, seed, phi=7.5, zero_weights=False, **kw):
    """x, z, w, gid, o and the point of `glmm_binomial_reference.problem`; phi a scalar, or 'vector' for one value per row,
    log-uniform on [0.05, 1e4] with phi[3] = 0.05 and phi[4] = 1e4 (N >= 5: the two ends sit behind the probe rows, whose own phi
    stays a draw); y drawn from Gamma(shape phi, mean exp(o + x beta + z . u)), every draw finite and positive (a draw that
    underflows at a tiny shape is raised to 1e-300).  Then three probe rows (N >= 4): y[0] = 1e-12, y[1] = 1e12, y[2] = 1.
    zero_weights: every fifth weight is 0.  Returns (x, y, z, w, gid, o, phi (N), free)."""
    x, _, z, w, gid, o, _, free = bref.problem(N, P, K, G, seed, **kw)
    rng = np.random.default_rng([seed, 11])
    if isinstance(phi, str):
        ph = np.exp(rng.uniform(np.log(PHI_LO), np.log(PHI_HI), size=N))
        if N >= 5:
            ph[3], ph[4] = PHI_LO, PHI_HI
    else:
        ph = np.full(N, float(phi))
    ng = 2 * P + 4 * K
    beta, u = free[:P], free[ng:ng + G * K].reshape(G, K)
    mu = np.exp(o + x @ beta + (z * u[gid]).sum(1))
    y = np.maximum(rng.gamma(ph, mu / ph), 1e-300)
    assert np.all(np.isfinite(y) & (y > 0.0))
    if N >= 4:
        y[0], y[1], y[2] = PROBES
    if zero_weights:
        w = w.copy()
        w[::5] = 0.0
    return x, y, z, w, gid, o, ph, free


SHAPES = [(1, 1, 1, 1), (37, 3, 1, 5), (65, 5, 2, 3), (130, 64, 4, 2), (300, 17, 4, 7)]
BARE = (37, 3, 1, 5)
TEST_HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                     # the priors the GPU tests run with (tests/test_gpu_glmm_slopes.py, HYP)


def shape_data(N, P, K, G, centred):
    """The data set of a test shape, seed N + P + K: phi = 7.5 below N = 130 and one value per row from there, every fifth weight
    zero at N = 300, and for BARE the unit design with a zero offset.  centred: log y of the two extreme probe rows is added to
    their offsets (o[0] += log 1e-12, o[1] += log 1e12), which by the scale identity makes them ordinary rows; the RAW variant
    leaves them at full size.  Returns (x, y, z, w, gid, o, phi (N), free)."""
    x, y, z, w, gid, o, ph, free = problem(N, P, K, G, N + P + K, phi='vector' if N >= 130 else 7.5, zero_weights=(N == 300))
    if (N, P, K, G) == BARE:
        o = np.zeros(N)
        assert np.array_equal(z, np.ones((N, 1)))
    if N >= 130:
        assert ph.min() == PHI_LO and ph.max() == PHI_HI
    if centred and N >= 4:
        o = o.copy()
        o[0] += np.log(PROBES[0])
        o[1] += np.log(PROBES[1])
    return x, y, z, w, gid, o, ph, free


def _t(a):
    return torch.tensor(np.atleast_1d(np.asarray(a, dtype=np.float64)))


def eh_coefs(rho, s, ly, phi, deg=GH_DEG):
    """E h^(k), k = 0..4 (5 x n, numpy) by the reference's rule; ly = log(y)."""
    rho, s, ly, phi = (_t(a) for a in np.broadcast_arrays(rho, s, ly, phi))
    return np.stack([expected_h(rho, s, phi, ly, k, deg).numpy() for k in range(5)])


def response_mean(rho, s, deg=GH_DEG):
    """E e^t, t ~ N(rho, s), on the nodes (numpy)."""
    rho, s = (_t(a) for a in np.broadcast_arrays(rho, s))
    t, wts = _rule(rho, s, deg)
    return (torch.exp(t) * wts[None, :]).sum(1).numpy()

"""The references of the binomial and negative-binomial mixed models against each other and against torch.distributions, the
likelihood-independent host layer fed the binomial pieces, and the constructor refusals of `BinomialGLMMObjective` and
`NegBinomialGLMMObjective` (which fire before a device context exists).  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glmm_binomial_reference as ref                                    # noqa: E402
import glmm_slopes_reference as sref                                     # noqa: E402

HYP = (1.3, 0.2, 0.7, 1.5, 0.8)                                          # tau_beta, mu0, kappa0, a0, b0


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _eta(free, P, K, G):
    return np.where(ref.positive_mask(P, K, G), np.exp(free), free)


@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 6, 4, 2)])
def test_one_trial_and_no_offset_is_the_logistic_reference(N, P, K, G):
    x, y, z, w, gid, free = sref.problem(N, P, K, G, seed=N + P + K)
    eta = _eta(free, P, K, G)
    a = ref.value_grad_hess(ref.kl_vec, eta, ref.targs(x, y, z, w, np.zeros(N), np.ones(N), gid, G, HYP))
    t = sref.tensors(x, y, z, w, gid, HYP)
    b = sref.value_grad_hess(sref.kl_vec, eta, t[:5] + (G, t[5]))
    assert abs(a[0] - b[0]) <= 1e-14 * abs(b[0]) and _rel(a[1], b[1]) < 1e-13 and _rel(a[2], b[2]) < 1e-13


@pytest.mark.parametrize('phi', [1.7, 'vector'])
@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 6, 4, 2)])
def test_negative_binomial_is_the_binomial_term_at_shifted_trials_and_offset(N, P, K, G, phi):
    """The identity under test, per row and under the same quadrature rule:
        (y + phi) E logaddexp(log phi, t) - y rho  =  (y + phi) E softplus(t - log phi) - y (rho - log phi)  +  phi log phi,
    since logaddexp(log phi, t) = log phi + softplus(t - log phi) and (y + phi) log phi - y log phi = phi log phi.  So the NB
    reference is the binomial reference at trials y + phi and offset o - log phi plus the constant sum_n w_n phi_n log phi_n;
    gradient and Hessian agree without a constant."""
    x, y, z, w, gid, o, ph, free = ref.nb_problem(N, P, K, G, seed=N + P + K, phi=phi)
    eta = _eta(free, P, K, G)
    a = ref.value_grad_hess(ref.nb_kl_vec, eta, ref.targs(x, y, z, w, o, ph, gid, G, HYP))
    b = ref.value_grad_hess(ref.kl_vec, eta, ref.targs(x, y, z, w, o - np.log(ph), y + ph, gid, G, HYP))
    const = float(np.sum(w * ph * np.log(ph)))
    assert abs(a[0] - (b[0] + const)) <= 1e-13 * abs(a[0])
    assert _rel(a[1], b[1]) < 1e-12 and _rel(a[2], b[2]) < 1e-11


def test_negative_binomial_reference_is_the_expected_negative_log_probability():
    """E_q[-log NB(y | mean e^t, dispersion phi)] under the Gauss-Hermite rule, plus log_norm_const = sum w [lgamma(y + phi) -
    lgamma(phi) - lgamma(y + 1)], is the NB data term minus sum w phi log phi (the part of -log p that (y + phi) logaddexp(log
    phi, t) - y t leaves out: -log p = (y + phi) log(phi + e^t) - y t - phi log phi - [lgamma terms])."""
    N, P, K, G = 60, 3, 2, 4
    x, y, z, w, gid, o, ph, free = ref.nb_problem(N, P, K, G, seed=8, phi='vector')
    eta = _eta(free, P, K, G)
    t = ref.tensors(x, y, z, w, o, ph, gid)
    te = torch.tensor(eta)
    rho, s = ref._rho_s(te, t[0], t[2], t[4], t[6], G)
    gx, gw = np.polynomial.hermite.hermgauss(ref.GH_DEG)
    nodes, wts = torch.tensor(np.sqrt(2.0) * gx), torch.tensor(gw / np.sqrt(np.pi))
    tt = rho[:, None] + torch.sqrt(s)[:, None] * nodes[None, :]
    # total_count = phi, logits = t - log phi: mean phi e^logits = e^t
    nb = torch.distributions.NegativeBinomial(total_count=t[5][:, None], logits=tt - torch.log(t[5])[:, None])
    e_nlp = float((t[3] * (-(nb.log_prob(t[1][:, None])) * wts[None, :]).sum(1)).sum())
    lnc = float((t[3] * (torch.lgamma(t[1] + t[5]) - torch.lgamma(t[5]) - torch.lgamma(t[1] + 1.0))).sum())
    data = float(ref.nb_data(te, t[0], t[1], t[2], t[3], t[4], t[5], t[6], G))
    const = float(np.sum(w * ph * np.log(ph)))
    assert abs((e_nlp + lnc) - (data - const)) <= 1e-12 * abs(data)


@pytest.mark.parametrize('N,P,K,G', [(37, 3, 2, 5), (130, 6, 4, 2)])
def test_closed_forms_on_binomial_pieces_reproduce_the_reference(N, P, K, G):
    """The tolerances of tests/test_glmm_slopes_host_math.py: value 1e-12, gradient 1e-10, Hessian 1e-9 (vector and free)."""
    from lrvb_amd import glmm_slopes as gs
    x, y, z, w, gid, o, mt, free = ref.problem(N, P, K, G, seed=N + P + K)
    mask = ref.positive_mask(P, K, G)
    eta = _eta(free, P, K, G)
    ng = 2 * P + 4 * K
    cf = gs.glmm_slopes_closed_forms(P, K, G, eta, ref.data_pieces(x, y, z, w, o, mt, gid, G, eta), *HYP)
    targs = ref.targs(x, y, z, w, o, mt, gid, G, HYP)
    val, g, H = ref.value_grad_hess(ref.kl_vec, eta, targs)
    assert abs(cf['value'] - val) <= 1e-12 * abs(val)
    assert _rel(cf['grad'], g) < 1e-10
    assert _rel(gs.block_arrow_dense(cf['Hgg'], cf['rows'], cf['Hx'], cf['loc']), H) < 1e-9
    j1, j2 = np.where(mask, eta, 1.0), np.where(mask, eta, 0.0)
    gf, Hgg, rows, Hx, loc = gs.block_arrow_to_free(cf, j1, j2, ng, G, K)
    _, g_f, H_f = ref.value_grad_hess(ref.kl_free, free, targs)
    assert _rel(gf, g_f) < 1e-10
    assert _rel(gs.block_arrow_dense(Hgg, rows, Hx, loc), H_f) < 1e-9


def test_problem_has_the_rows_the_kernel_must_get_right():
    x, y, z, w, gid, o, mt, free = ref.problem(65, 5, 2, 3, seed=72)
    assert mt[0] == 0.0 and mt[1] == 1.0 and mt.max() > 1.0 and np.all(mt == np.round(mt))
    assert np.all((0.0 <= y) & (y <= mt)) and np.any((0.0 < y) & (y < mt)) and np.any(o != 0.0)


def test_constructor_refusals_need_no_device():
    import lrvb_amd as vb
    N, P, K, G = 12, 2, 1, 3
    rng = np.random.default_rng(0)
    x, z, gid = rng.normal(size=(N, P)), np.ones((N, K)), np.arange(N) % G
    mt = np.full(N, 4.0)
    y = np.full(N, 2.0)
    o = np.zeros(N)

    def binom(y=y, trials=mt, offset=o):
        return vb.BinomialGLMMObjective(None, x, y, z, gid, G, trials=trials, offset=offset)

    def bad(v, i, val):
        v = v.copy()
        v[i] = val
        return v

    for kw in (dict(y=bad(y, 3, 5.0)),                                   # y > trials
               dict(y=bad(y, 3, -1.0)),
               dict(y=bad(y, 3, np.nan)),
               dict(y=np.full(N, 2.0), trials=None),                     # y > 1 with one trial per row
               dict(trials=bad(mt, 0, -1.0), y=np.zeros(N)),             # negative trials
               dict(trials=bad(mt, 0, np.inf)),
               dict(trials=mt[:-1]), dict(offset=o[:-1]), dict(y=y[:-1]),    # wrong lengths
               dict(offset=bad(o, 5, np.nan)), dict(offset=bad(o, 5, np.inf))):
        with pytest.raises(ValueError):
            binom(**kw)

    def negbin(dispersion, y=y, offset=None):
        return vb.NegBinomialGLMMObjective(None, x, y, z, gid, G, dispersion, offset=offset)

    for args in ((0.0,), (-1.0,), (np.nan,), (np.full(N - 1, 2.0),), (bad(np.full(N, 2.0), 4, 0.0),)):
        with pytest.raises(ValueError):
            negbin(*args)
    with pytest.raises(ValueError):
        negbin(1.5, y=bad(y, 2, -1.0))
    with pytest.raises(ValueError):
        negbin(1.5, offset=bad(o, 1, np.nan))

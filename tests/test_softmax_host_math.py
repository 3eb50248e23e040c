"""Multinomial (softmax) regression on the host: the numpy reference against torch fp64 autograd (extreme logits included),
the block layout of the Hessian, the free conversion on a box-bounded ArrayParam, and the input checks of
SoftmaxRegressionObjective (all raised before anything reaches the device)."""
import numpy as np
import pytest
import torch

import lrvb_amd as vb
import softmax_reference as sr


def _torch_value(x, y, w, eta, K):
    X = torch.as_tensor(x)
    B = eta.reshape(K - 1, x.shape[1])
    z = torch.cat([torch.zeros(x.shape[0], 1, dtype=torch.float64), X @ B.T], dim=1)
    lse = torch.logsumexp(z, dim=1)
    return (torch.as_tensor(w) * (lse - z[torch.arange(len(y)), torch.as_tensor(y, dtype=torch.long)])).sum()


def _problem(rng, N, P, K, scale=1.0):
    x = rng.normal(size=(N, P))
    y = rng.integers(0, K, size=N)
    w = rng.uniform(0.0, 2.0, size=N)
    w[::5] = 0.0
    beta = rng.normal(size=(K - 1, P)) * scale
    return x, y, w, beta


@pytest.mark.parametrize('K,P,N', [(2, 3, 17), (3, 5, 40), (5, 4, 31), (17, 2, 60)])
def test_reference_matches_autograd(K, P, N):
    rng = np.random.default_rng(K * 100 + P)
    x, y, w, beta = _problem(rng, N, P, K)
    eta = torch.tensor(beta.ravel(), requires_grad=True)
    f = _torch_value(x, y, w, eta, K)
    g, = torch.autograd.grad(f, eta, create_graph=True)
    H = torch.stack([torch.autograd.grad(g[i], eta, retain_graph=True)[0] for i in range(eta.numel())]).numpy()
    assert abs(sr.value(x, y, w, beta) - f.item()) <= 1e-12 * abs(f.item())
    np.testing.assert_allclose(sr.grad(x, y, w, beta), g.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sr.hessian(x, w, beta), H, rtol=1e-11, atol=1e-12)
    v = rng.normal(size=beta.size)
    np.testing.assert_allclose(sr.hvp(x, w, beta, v), H @ v, rtol=1e-11, atol=1e-11)
    # d2 f / d eta d w_n: the gradient of the per-row loss
    C = sr.cross_hessian(x, y, beta)
    for n in (0, N // 2, N - 1):
        e = np.zeros(N); e[n] = 1.0
        np.testing.assert_allclose(C[:, n], sr.grad(x, y, e, beta), rtol=1e-12, atol=1e-14)


def test_reference_extreme_logits_are_finite_and_exact():
    rng = np.random.default_rng(3)
    K, P, N = 4, 3, 12
    x = rng.normal(size=(N, P)) * 1e3
    y = rng.integers(0, K, size=N)
    w = np.ones(N)
    beta = rng.normal(size=(K - 1, P))
    z = sr.logits(x, beta)
    assert np.abs(z).max() >= 1e3
    val = sr.value(x, y, w, beta)
    eta = torch.tensor(beta.ravel(), requires_grad=True)
    f = _torch_value(x, y, w, eta, K)
    g, = torch.autograd.grad(f, eta)
    assert np.isfinite(val) and abs(val - f.item()) <= 1e-12 * abs(f.item())
    np.testing.assert_allclose(sr.grad(x, y, w, beta), g.numpy(), rtol=1e-12, atol=1e-9)
    assert np.all(np.isfinite(sr.hessian(x, w, beta)))


def test_hessian_block_layout_and_k2_is_logistic():
    rng = np.random.default_rng(5)
    K, P, N = 4, 3, 25
    x, y, w, beta = _problem(rng, N, P, K)
    H = sr.hessian(x, w, beta)
    p = sr.probs(x, beta)
    np.testing.assert_allclose(H[P:2 * P, 2 * P:3 * P], -(x.T * (w * p[:, 1] * p[:, 2])) @ x, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(H, H.T, rtol=0, atol=1e-13)
    # K = 2: log(1 + e^z) - [y = 1] z, the logistic GLM loss
    y2 = rng.integers(0, 2, size=N)
    b2 = rng.normal(size=(1, P))
    z = x @ b2[0]
    assert abs(sr.value(x, y2, w, b2) - np.sum(w * (np.logaddexp(0.0, z) - y2 * z))) < 1e-12 * N


def test_free_conversion_on_box_bounded_array():
    """Free-coordinate Hessian = J^T H J + diag(g o d2 eta / d theta2) for a box-bounded ArrayParam, against autograd of the
    free-coordinate objective (the map a bounded box uses: packing.constrain)."""
    rng = np.random.default_rng(11)
    K, P, N = 3, 2, 30
    x, y, w, _ = _problem(rng, N, P, K)
    lb, ub = -2.0, 3.0
    par = vb.ArrayParam('beta', shape=(K - 1, P), lb=lb, ub=ub)
    theta = rng.normal(size=(K - 1) * P) * 0.5
    par.set_free(theta)
    beta = par.get().copy()
    J = par.free_to_vector_jac(theta)
    J = J.toarray() if hasattr(J, 'toarray') else np.asarray(J)
    g = sr.grad(x, y, w, beta)
    t = torch.tensor(theta, requires_grad=True)
    eta = lb + (ub - lb) / (1.0 + torch.exp(-t))            # logistic box map
    np.testing.assert_allclose(eta.detach().numpy(), beta.ravel(), rtol=1e-14, atol=1e-14)
    f = _torch_value(x, y, w, eta, K)
    gt, = torch.autograd.grad(f, t, create_graph=True)
    Ht = torch.stack([torch.autograd.grad(gt[i], t, retain_graph=True)[0] for i in range(t.numel())]).numpy()
    d2 = (torch.autograd.functional.hessian(lambda s: (lb + (ub - lb) / (1.0 + torch.exp(-s))).sum(), t.detach())).diagonal().numpy()
    np.testing.assert_allclose(J.T @ g, gt.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(J.T @ sr.hessian(x, w, beta) @ J + np.diag(g * d2), Ht, rtol=1e-11, atol=1e-12)


def _par(K, P, name='beta'):
    par = vb.ModelParamsDict('par')
    par.push_param(vb.ArrayParam(name, shape=(K - 1, P)))
    return par


@pytest.mark.parametrize('K', [1, 18, 2.5])
def test_refuses_bad_class_count(K):
    with pytest.raises(ValueError, match='n_classes'):
        vb.SoftmaxRegressionObjective(_par(3, 2), np.ones((4, 2)), np.zeros(4, dtype=int), K)


def test_refuses_wide_design():
    with pytest.raises(ValueError, match='1024'):
        vb.SoftmaxRegressionObjective(_par(3, 1025), np.ones((2, 1025)), np.zeros(2, dtype=int), 3)


@pytest.mark.parametrize('y', [np.array([0, 1, 3, 1]), np.array([0, -1, 1, 1]), np.array([0.0, 0.5, 1.0, 1.0]),
                               np.array([0, 1, 2]), np.array(['a', 'b', 'a', 'b'])])
def test_refuses_bad_labels(y):
    with pytest.raises(ValueError):
        vb.SoftmaxRegressionObjective(_par(3, 2), np.ones((4, 2)), y, 3)


@pytest.mark.parametrize('shape', [(3, 2), (2, 3), (6,)])
def test_refuses_parameter_of_wrong_shape(shape):
    par = vb.ModelParamsDict('par')
    par.push_param(vb.ArrayParam('beta', shape=shape))
    with pytest.raises(ValueError, match='ArrayParam'):
        vb.SoftmaxRegressionObjective(par, np.ones((4, 2)), np.zeros(4, dtype=int), 3)


def test_refuses_parameter_with_extra_entries():
    par = _par(3, 2)
    par.push_param(vb.VectorParam('other', 2))
    with pytest.raises(ValueError, match='nothing else'):
        vb.SoftmaxRegressionObjective(par, np.ones((4, 2)), np.zeros(4, dtype=int), 3)

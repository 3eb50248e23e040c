"""The softmax pass (csrc/k_softmax.hip, `softmax_pass_kernel`) entry by entry through the public path
(`DeviceContext.softmax_set_labels / softmax_terms / softmax_hvp / softmax_obs_influence / set_tuning`): all three modes
(gradient, product, rows-only) on every instance the dispatch launches, at one, two, three and four trips of the chunk loop,
on both staging routes, with four and eight waves.

Two oracles (tests/softmax_pass_reference.py): an integer design on which every output is exactly
representable and the device result must be BITWISE the int64 computation, and real data against a longdouble reference under
entry-wise bounds counted from the kernel text.  p of EVERY row is read through unit probes of the influence rows; single
rows (chunk and trip boundaries, both T registers, every extreme kind of logits) also through indicator columns of X.  The
same assertions are passed by the float64 restatement of the kernel on the CPU
(tests/test_softmax_pass_reference_host_math.py).  A failure names the entry."""
import numpy as np
import pytest
import torch

import softmax_pass_reference as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1, 'no HIP device visible'
    return lrvb_amd


class DeviceBackend(object):
    """One context on one case of the reference file; the interface of `sp.F64Backend`."""

    def __init__(self, vb, c, aligned=True, K_blocks=None):
        X = c['X']
        self.c, self.K = c, c['K']
        N, P = X.shape
        D = ((K_blocks or self.K) - 1) * P
        self.ctx = vb.DeviceContext([dict(kind=vb._hip.BLOCK_BOX, free_size=D, vec_size=D, dim0=D, dim1=0, lb=-np.inf, ub=np.inf)],
                                    loss='data_only', n_obs=N, n_cols=P)
        if aligned:
            self.ctx.set_data(vb._hip.SLOT_X, X)
        else:                                                   # an even-P design on a base offset by 8 bytes: the 4-byte staging
            self.store = torch.empty(N * P + 1, dtype=torch.float64, device='cuda:0')
            Xd = self.store[1:].view(N, P)
            Xd.copy_(torch.as_tensor(X))
            assert Xd.data_ptr() % 16 == 8
            torch.cuda.synchronize()
            self.ctx.set_data_dev(vb._hip.SLOT_X, Xd.data_ptr(), N, P)
        self.ctx.set_weights(c['w'])
        self.ctx.softmax_set_labels(c['y'], self.K)

    def terms(self, flags=0):
        self.ctx.set_tuning(0, flags)
        val, g, _ = self.ctx.softmax_terms(self.c['beta'].ravel(), self.K, want_hess=False)
        return val, g

    def hvp(self, flags=0):
        self.ctx.set_tuning(0, flags)
        return self.ctx.softmax_hvp(self.c['beta'].ravel(), self.K, self.c['V'].ravel())

    def influence(self, A, n0, n1, flags=0):
        self.ctx.set_tuning(0, flags)
        return self.ctx.softmax_obs_influence(self.c['beta'].ravel(), self.K, A, n0, n1)

    def hessian(self):
        self.ctx.set_tuning(0, 0)
        return self.ctx.softmax_terms(self.c['beta'].ravel(), self.K)[2]

    def close(self):
        self.ctx.close()


def maker(vb):
    return lambda c, aligned: DeviceBackend(vb, c, aligned)


def _id(case):
    return '-'.join(str(int(v)) for v in case)


# ---- the exact oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,aligned', sp.EXACT_CASES, ids=[_id(c) for c in sp.EXACT_CASES])
def test_exact_design_bitwise(vb, N, P, K, aligned):
    """Gradient, product, influence rows and p of every row bit for bit; the value bitwise on the saturated-only variant and
    bounded on the mixed one.  Every width of the column grid at N = 9 and 2121, every N of the row grid at P = 2, 130, 129,
    1024, 1023, the offset base; both wave counts wherever the four-wave bit changes the instance."""
    sp.check_exact_case(maker(vb), N, P, K, aligned)


@pytest.mark.parametrize('N,P,K', sp.HESS_CASES, ids=[_id(c) for c in sp.HESS_CASES])
def test_exact_hessian_blocks(vb, N, P, K):
    """The weight columns w p_a (delta_ab - p_b) and the block bookkeeping: placement at (a P, b P), the mirror, the batch
    boundary (K = 16: 64 + 56 blocks at P = 66 on the batched route; P = 9 and P = 3 take a launch per block)."""
    sp.check_hessian(maker(vb), N, P, K)


# ---- real data under the counted bounds ----------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K,aligned', sp.REAL_CASES, ids=[_id(c) for c in sp.REAL_CASES])
def test_real_data_inside_the_bounds(vb, N, P, K, aligned):
    """Value, every entry of the gradient, of the product and of the influence rows, and p of every row, inside the bounds;
    the probe rows and the extreme rows (arg-max in the reference class, lane 0, lane Km - 1, an exact tie, all logits below
    -750, gaps of 30 and 700, the last row extreme when N mod 8 != 0, a zero weight) stand alone in indicator columns."""
    ratios = sp.check_real_case(maker(vb), N, P, K, aligned)
    print('softmax pass ratio N {} P {} K {} aligned {} {}'.format(N, P, K, aligned, {k: round(v, 4) for k, v in sorted(ratios.items())}))


@pytest.mark.parametrize('P,K,Q', sp.INFL_CASES, ids=[_id(c) for c in sp.INFL_CASES])
def test_influence_windows(vb, P, K, Q):
    """N = 4099 (three trips over the whole range): windows that start and end on and off the 8-row chunk grid, down to one
    row; Q below, at and above floor(16 / Km) outputs per launch (Km = 5: 15 of 16 lanes; Km = 16: one output per launch)."""
    ratios = sp.check_influence_windows(maker(vb), P, K, Q)
    print('softmax pass ratio influence windows P {} K {} Q {} {:.4f}'.format(P, K, Q, ratios['influence']))


# ---- state ------------------------------------------------------------------------------------------------------------------
def _outputs(be, A):
    val, g = be.terms()
    return val, g, be.hvp(), be.influence(A, 0, be.c['X'].shape[0])


def test_relabelled_context_matches_a_fresh_one(vb):
    """K = 17 first, then K = 3 on the same context: the p buffer is zeroed only when it grows, so the rows behind N (K - 1)
    hold K = 17 probabilities.  Every output must be bit-identical to a fresh context's, and inside the bounds."""
    N, P = sp.STATE_CASE
    big, small = sp.real_case(N, P, 17), sp.real_case(N, P, 3)
    small['X'] = big['X']                                       # one design: only labels, beta, V and A change
    be = DeviceBackend(vb, big)
    _outputs(be, big['A'])
    be.c, be.K = small, 3
    be.ctx.set_weights(small['w'])
    be.ctx.softmax_set_labels(small['y'], 3)
    got = _outputs(be, small['A'])
    be.close()
    fresh = DeviceBackend(vb, small)
    want = _outputs(fresh, small['A'])
    fresh.close()
    assert got[0] == want[0]
    for a, b, name in zip(got[1:], want[1:], ('gradient', 'product', 'influence')):
        sp.assert_exact(a, b, 'relabelled context, ' + name)
    ref = sp.ld_eval(small)
    bnd = sp.bounds(small, ref)
    sp.assert_bounded(got[1], ref['g'], bnd['g'], 'gradient relabelled')
    sp.assert_bounded(got[2], ref['hv'], bnd['hv'], 'product relabelled')


def test_two_calls_new_weights_and_another_point(vb):
    """Two calls are bit-identical; new weights are picked up (bitwise the exact oracle with them); a product at another beta
    forms p again (bitwise a fresh context's, and another result)."""
    N, P = sp.STATE_CASE
    c = sp.exact_case(N, P, 8)
    be = DeviceBackend(vb, c)
    first, second = _outputs(be, c['A']), _outputs(be, c['A'])
    assert first[0] == second[0]
    for a, b in zip(first[1:], second[1:]):
        assert np.array_equal(a, b)
    c2 = dict(c, w=np.roll(c['w'], 3) + 1.0)
    be.c = c2
    be.ctx.set_weights(c2['w'])
    e2 = sp.exact_outputs(c2)
    sp.assert_exact(be.hvp(), e2['hv'], 'product after new weights (p kept, weights re-read)')
    sp.assert_exact(be.terms()[1], e2['g'], 'gradient after new weights')
    be.close()
    # another point, real data: p must be formed again (bitwise a fresh context's product there, inside the bound, another result)
    c = sp.real_case(N, P, 5)
    be = DeviceBackend(vb, c)
    hv1 = be.hvp()
    c4 = dict(c, beta=0.5 * c['beta'])
    be.c = c4
    hv4 = be.hvp()
    be.close()
    fresh = DeviceBackend(vb, c4)
    want = fresh.hvp()
    fresh.close()
    sp.assert_exact(hv4, want, 'product at another beta')
    ref = sp.ld_eval(c4)
    sp.assert_bounded(hv4, ref['hv'], sp.bounds(c4, ref)['hv'], 'product at another beta')
    assert not np.array_equal(hv4, hv1)

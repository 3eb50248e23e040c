"""The host state every model class shares (`DeviceModel`, models.py): weights upload, the one-entry memos and their key,
installed statistics -- driven through a stub context, no device."""
import numpy as np
import pytest

from lrvb_amd.models import DeviceModel
from lrvb_amd.packing import HyperVectorParam, VectorParam

N_OBS, DIM = 5, 3


class StubContext(object):
    def __init__(self):
        self.hook_epoch = 0
        self.has_reduce_hook = False
        self.uploads = []
        self.solves = []

    def set_weights(self, w):
        self.uploads.append(np.array(w))

    def cg_solve_matrix(self, H, b, x0=None, Minv=None, tol=1e-8, maxiter=0):
        self.solves.append(H)
        return np.linalg.solve(H, b), 0, 1


class Toy(DeviceModel):
    def __init__(self, weights=None):
        self.ctx = StubContext()
        self._declare_weights(N_OBS, weights)
        self._declare_hyper('ridge', HyperVectorParam('ridge', 1, val=np.ones(1)))
        self.n_hessian = 0

    def hessian(self, x, is_free=True):
        self.n_hessian += 1
        x = np.asarray(x, dtype=np.float64)
        return np.outer(x, x) + (float(self.ridge_par.get_vector()[0]) + float(np.sum(self.weights_par.get_vector()))) * np.eye(x.size)


class ToyAtPoint(Toy):
    _stats_at_point = True


def test_weights_are_declared_and_sized():
    f = Toy()
    assert f.hyper_kind(f.weights_par) == 'weights' and f.tilt_par is None
    assert np.array_equal(f.weights_par.get_vector(), np.ones(N_OBS))
    with pytest.raises(ValueError):
        Toy(weights=np.ones(N_OBS + 1))
    with pytest.raises(NotImplementedError):
        f.hyper_kind(VectorParam('other', 2))


def test_push_state_uploads_only_what_changed():
    f = Toy(weights=np.arange(1.0, N_OBS + 1))
    up = f.ctx.uploads
    f._push_state()
    assert len(up) == 1 and np.array_equal(up[0], np.arange(1.0, N_OBS + 1))
    f._push_state()
    assert len(up) == 1                                       # unchanged: nothing is sent
    f.weights_par.set_vector(np.full(N_OBS, 2.0))
    f._push_state()
    f._push_state()
    assert len(up) == 2 and np.array_equal(up[1], np.full(N_OBS, 2.0))
    f.weights_par = HyperVectorParam('weights', N_OBS, val=np.full(N_OBS, 3.0))      # another parameter object, same size
    f._push_state()
    f._push_state()
    assert len(up) == 3 and np.array_equal(up[2], np.full(N_OBS, 3.0))
    plain = VectorParam('weights', N_OBS, val=np.full(N_OBS, 4.0))                     # no `version`: compared by contents
    assert getattr(plain, 'version', None) is None
    f.weights_par = plain
    f._push_state()
    f._push_state()
    assert len(up) == 4 and np.array_equal(up[3], np.full(N_OBS, 4.0))
    plain.set_vector(np.full(N_OBS, 5.0))
    f._push_state()
    f._push_state()
    assert len(up) == 5 and np.array_equal(up[4], np.full(N_OBS, 5.0))


X0 = np.array([0.5, -1.0, 2.0])

CHANGES = {
    'another point': lambda f: dict(x=X0 + 1.0),
    'the other is_free': lambda f: dict(is_free=False),
    'weights': lambda f: f.weights_par.set_vector(np.full(N_OBS, 2.0)),
    'a non-weight hyper-parameter': lambda f: f.ridge_par.set_vector(np.array([3.0])),
    'hook epoch': lambda f: setattr(f.ctx, 'hook_epoch', f.ctx.hook_epoch + 1),
    'statistics installed': lambda f: f._install_reduced_stats(np.ones(4), 4),
}


@pytest.mark.parametrize('what', sorted(CHANGES))
def test_hessian_memo_hits_and_misses(what):
    f = Toy()
    H = f._hessian_cached(X0, True)
    assert f._hessian_cached(X0.copy(), True) is H and f.n_hessian == 1
    at = dict(x=X0, is_free=True)
    at.update(CHANGES[what](f) or {})
    H2 = f._hessian_cached(at['x'], at['is_free'])
    assert f.n_hessian == 2, what
    assert np.array_equal(H2, Toy.hessian(f, at['x'], at['is_free']))      # the memo holds the value of the new state
    assert f._hessian_cached(at['x'], at['is_free']) is H2 and f.n_hessian == 3


def test_clearing_statistics_is_a_miss_and_never_restores_an_earlier_key():
    f = Toy()
    f._push_state()
    before = f._data_key()
    f._install_reduced_stats(np.ones(4), 4)
    f._hessian_cached(X0, True)
    installed = f._data_key()
    f._install_reduced_stats(None)
    f._hessian_cached(X0, True)
    assert f.n_hessian == 2
    assert len({before, installed, f._data_key()}) == 3
    assert f._installed_stats() is None


def test_default_hvp_and_cg_solve_use_the_cached_hessian():
    f = Toy()
    v = np.array([1.0, 2.0, 3.0])
    H = Toy.hessian(f, X0)
    assert np.array_equal(f.hvp(X0, v, True), H @ v) and np.array_equal(f.hvp(X0, v), H @ v)
    sol, info, _ = f.cg_solve(X0, v)
    assert f.n_hessian == 2 and info == 0 and f.ctx.solves[0] is f._hessian_cached(X0, True)
    assert np.allclose(H @ sol, v, rtol=0, atol=1e-12)
    assert len(f.ctx.uploads) == 1                             # one upload of the weights for all of these


def test_memo_slots_are_independent():
    f = Toy()
    made = []
    assert f._memo('a', 1, lambda: made.append('a') or 'A') == 'A'
    assert f._memo('b', 1, lambda: made.append('b') or 'B') == 'B'
    assert f._memo('a', 1, lambda: made.append('a') or 'A2') == 'A' and made == ['a', 'b']
    assert f._memo('a', 2, lambda: made.append('a') or 'A2') == 'A2'
    f._forget('b', 'never made')
    assert f._memo('b', 1, lambda: 'B2') == 'B2' and f._memo('a', 2, lambda: 'A3') == 'A2'


def test_call_is_the_value_at_the_parameter():
    f = Toy()
    f.par = VectorParam('theta', DIM, val=X0)
    f.value = lambda x, is_free: (float(np.sum(x)), is_free)
    assert f() == (float(np.sum(f.par.get_free())), True)


def test_install_reduced_stats_refusals():
    f, g = Toy(), ToyAtPoint()
    with pytest.raises(ValueError, match='expected 4 statistics$'):
        f._install_reduced_stats(np.ones(5), 4)
    with pytest.raises(ValueError, match='expected 4 statistics and the point they were formed at'):
        g._install_reduced_stats(np.ones(5), 4, eta=X0)
    with pytest.raises(ValueError, match='expected 4 statistics and the point they were formed at'):
        g._install_reduced_stats(np.ones(4), 4)                # the point is required
    assert f._installed_stats() is None and g._installed_stats(X0) is None and f._stats_token == g._stats_token == 0
    for h in (f, g):
        h.ctx.has_reduce_hook = True
        with pytest.raises(RuntimeError):
            h._install_reduced_stats(np.ones(4), 4, eta=X0)
        h._install_reduced_stats(None)                         # clearing is allowed under a hook
        h.ctx.has_reduce_hook = False


def test_install_reduced_stats_keeps_private_copies():
    g = ToyAtPoint()
    flat, eta = np.arange(4.0), X0.copy()
    g._install_reduced_stats(flat, 4, eta=eta)
    flat[:] = -1.0
    eta[:] = -1.0
    assert np.array_equal(g._installed_stats(X0), np.arange(4.0))
    with pytest.raises(ValueError, match='the installed statistics were formed at another point'):
        g._installed_stats(X0 + 1.0)
    f = Toy()                                                  # a family whose statistics belong to no point
    f._install_reduced_stats([[0.0, 1.0], [2.0, 3.0]], 4)
    assert np.array_equal(f._installed_stats(), np.arange(4.0)) and np.array_equal(f._installed_stats(X0), np.arange(4.0))

"""The likelihood policies of csrc/k_glmm_walk.h ROW BY ROW in their tails, on the GPU, against the exact values of
tests/golden/glmm_tail_exact.npz (mpmath).  Data sets, rows, measures and bounds: tests/glmm_tail_cases.py.

Every family runs as one data set of one row per group (G = N, K = 1, z = 1, P = 1, x = 0), N no multiple of the 64-row tile, and
a second time with its rows in reversed order.  Every entry refuses r = 0, so the "s = 0" rows run at the smallest positive double
(tests/glmm_tail_cases.py, `rows`), and the exact values are computed at that s.  Checked per family:
  terms      the five coefficients of every row from the `*_terms` entry (the five-order instantiation `moments` / `node<5>`),
  influence  a1' and a2' of every row from the `*_obs_influence` entry with A[0] = ones on e, A[1] = ones on r (the two-order
             instantiation `infl` / `node<2>`), against the exact values and never against the bits of the terms path,
  position   the reversed run returns the same bits per row on both paths,
  value      one weighted call per decade of |exact[0]| and 16 single-row data sets,
  refusals   cloglog, zero-truncated Poisson and NB2 with one row moved to t = -760.
Bounds: pointwise CAP = 1e-10 where the fixture says the entry is resolvable, and everywhere the absolute measure at 8 x the host
formula's own worst figure (floor 64 x 2^-53); Poisson relative (|rho + s / 2| + 4) 2^-52, the argument rounding plus one exp.
No bound here comes from the device's output.  The test prints the device's worst figures (recorded in DESIGN.md section 42)."""
import math

import numpy as np
import pytest

import glmm_tail_cases as tc

pytestmark = pytest.mark.gpu

# family -> (fixture, terms entry, influence entry, takes nodes)
ENTRIES = {'intercept': ('logistic', 'glmm_terms', 'glmm_obs_influence', True),
           'logistic': ('logistic', 'glmm_slopes_terms', 'glmm_slopes_obs_influence', True),
           'binomial': ('binomial', 'glmm_binomial_terms', 'glmm_binomial_obs_influence', True),
           'negbin': ('negbin', 'glmm_binomial_terms', 'glmm_binomial_obs_influence', True),
           'probit': ('probit', 'glmm_binomial_terms', 'glmm_binomial_obs_influence', True),
           'cloglog': ('cloglog', 'glmm_binomial_terms', 'glmm_binomial_obs_influence', True),
           'poisson': ('poisson', 'glmm_poisson_terms', 'glmm_poisson_obs_influence', False),
           'ztpoisson': ('ztpoisson', 'glmm_ztpoisson_terms', 'glmm_ztpoisson_obs_influence', True),
           'ztnegbin': ('ztnegbin', 'glmm_ztnegbin_terms', 'glmm_ztnegbin_obs_influence', True),
           'beta': ('beta', 'glmm_beta_terms', 'glmm_beta_obs_influence', True),
           'beta_disp': ('beta_disp', 'glmm_beta_dispersion_terms', None, True),
           'negbin_disp': ('negbin_disp', 'glmm_negbin_dispersion_terms', None, True)}
FAMILIES = tuple(f for f in ENTRIES if f not in tc.DISPERSION)
# family -> (predict entry, the per-row extras of its new rows behind the offset)
PREDICT = {'probit': ('glmm_binomial_predict', ('trials',)), 'cloglog': ('glmm_binomial_predict', ('trials',)),
           'ztpoisson': ('glmm_ztpoisson_predict', ()), 'ztnegbin': ('glmm_ztnegbin_predict', ('phi',)),
           'beta': ('glmm_binomial_predict', (None,))}
REFUSING = ('cloglog', 'ztpoisson', 'ztnegbin')


@pytest.fixture(scope='module')
def vb():
    import lrvb_amd
    assert lrvb_amd._hip.device_count() >= 1
    return lrvb_amd


_fixtures = {}


def _fx(family):
    name = ENTRIES[family][0]
    if name not in _fixtures:
        _fixtures[name] = tc.load(name)
    return _fixtures[name]


class Rows:
    """A device context holding the rows `order` of a family's fixture, one row per group, and the calls on it."""

    def __init__(self, vb, family, order, offset=None):
        hip = vb._hip
        fx = _fx(family)
        self.family, self.fx, self.order = family, fx, np.asarray(order)
        self.N = N = self.order.size
        name, self.terms_entry, self.infl_entry, self.nodes = ENTRIES[family]
        sel = lambda k: np.ascontiguousarray(fx[k][self.order])
        blocks = [dict(kind=hip.BLOCK_BOX, free_size=2, vec_size=2, dim0=2, dim1=0, lb=-np.inf, ub=np.inf)]
        ctx = self.ctx = vb.DeviceContext(blocks, loss='logistic', n_obs=N, n_cols=1)
        ctx.set_data(hip.SLOT_X, np.zeros((N, 1)))
        ctx.set_data(hip.SLOT_Y, sel('y'))
        ctx.set_groups(np.arange(N), N)
        if family != 'intercept':
            ctx.set_group_design(np.ones((N, 1)))
        ctx.set_weights(np.ones(N))
        self.rho = sel('rho') if offset is None else offset
        own_offset = family not in ('intercept', 'logistic')              # the logistic entries take no offset: rho = e[n]
        if own_offset:
            ctx.set_offset(self.rho)
        if name in ('binomial', 'negbin', 'probit', 'cloglog', 'negbin_disp'):
            ctx.set_trials(sel('trials'))
            ctx.set_link({'probit': 1, 'cloglog': 2}.get(name, 0))
        if name in ('ztnegbin', 'beta', 'beta_disp', 'negbin_disp'):
            ctx.set_dispersion(sel('phi'))
        e = np.zeros(N) if own_offset else self.rho
        r = sel('s')
        gx, gw = tc.gh()
        self.gh = (gx, gw) if self.nodes else ()
        if family == 'intercept':
            self.point = (np.zeros(1), np.ones(1), e, r)
        else:
            self.point = (np.zeros(1), np.ones(1), e.reshape(N, 1), r.reshape(N, 1))

    def terms(self):
        """(value, N x 5 sums [a1, a2, c11, c12, c22]) in the order of the FIXTURE's rows `order`."""
        fn = getattr(self.ctx, self.terms_entry)
        if self.family == 'intercept':
            val, _, gl, _, _, L = fn(*self.point, *self.gh)
            return val, np.hstack([gl, L])
        val, _, _, gs = fn(*self.point, *self.gh, want_border=False)
        assert gs.shape == (self.N, 5)
        return val, gs

    def influence(self):
        """N x 2: a1' (the entry's own, y subtracted where the policy is canonical) and a2' of every row."""
        N = self.N
        A = np.zeros((2, 2 + 2 * N))
        A[0, 2:2 + N] = 1.0
        A[1, 2 + N:] = 1.0
        out = getattr(self.ctx, self.infl_entry)(*self.point, *self.gh, A)
        assert out.shape == (N, 2)
        return out

    def dispersion(self):
        """(d (2): sum w h_l and sum w h_ll; N x 2: E d_t h_l and E d_t^2 h_l / 2 of every row) of a dispersion entry."""
        d, _, cl = getattr(self.ctx, self.terms_entry)(*self.point, *self.gh)
        assert cl.shape == (self.N, 2)
        return d, cl

    def predict_new_rows(self):
        """The predict entry on NEW rows that repeat the context's own (x = 0, z = 1, group n, the row's offset and extras): 5 x N."""
        N, ctx, fx = self.N, self.ctx, self.fx
        self.terms()                                                     # the group sums, their factor and the group covariance
        ctx.glmm_slopes_schur(np.tile(np.eye(2)[np.triu_indices(2)], (N, 1)), np.ones((N, 2)), np.zeros((N, 2, 3)))
        ctx.glmm_slopes_group_cov(np.eye(5), np.ones(5), N, 1, want_host=False)
        entry, extras = PREDICT[self.family]
        extra = tuple(None if k is None else np.ascontiguousarray(fx[k][self.order]) for k in extras)
        new = (np.zeros((N, 1)), np.ones((N, 1)), np.arange(N), self.rho) + extra
        return getattr(ctx, entry)(*self.point, *self.gh, np.zeros((1, 1)), new=new)

    def close(self):
        self.ctx.close()


def _errors(family, fx, got, orders, idx=None):
    """(pointwise worst on the device mask, absolute worst) per order of `orders`; got is len(orders) x n."""
    sl = slice(None) if idx is None else idx
    exact = fx['exact'][orders][:, sl]
    mask = tc.device_mask(fx['name'], fx)[orders][:, sl]
    sc = tc.scale(fx['name'], {k: fx[k][sl] for k in ('rho', 's', 'y', 'trials', 'phi')}, fx['exact'][:, sl])[orders]
    rel = np.where(mask, tc.rel_err(got, exact), 0.0)
    return rel.max(-1), (np.abs(got - exact) / sc).max(-1)


def _bounds(fx, orders):
    return tc.abs_bounds(fx['host_abs'])[orders]


def _poisson_check(fx, got, orders, what):
    exact = fx['exact'][orders]
    bound = (np.abs(fx['rho'] + 0.5 * fx['s']) + 4.0) * 2.0 ** -52
    rel = np.abs(got - exact) / exact
    print('poisson', what, 'worst relative error over its bound (|rho + s / 2| + 4) 2^-52:', float(np.max(rel / bound)))
    assert np.all(rel <= bound)


@pytest.mark.parametrize('family', FAMILIES)
def test_rows_terms_influence_and_position(vb, family):
    fx = dict(_fx(family), name=ENTRIES[family][0])
    N = fx['rho'].size
    assert N % 64 != 0 and fx['deg'] == tc.DEG and np.any(fx['kind'][-(N % 64):] >= 0)     # the last tile is part of it
    fwd, rev = Rows(vb, family, np.arange(N)), Rows(vb, family, np.arange(N)[::-1])
    _, sums = fwd.terms()
    infl = fwd.influence()
    _, sums_r = rev.terms()
    infl_r = rev.influence()
    fwd.close(); rev.close()
    assert np.all(np.isfinite(sums)) and np.all(np.isfinite(infl))
    # position: a row's sums come from its own four lanes in an order that does not depend on its slot
    assert np.array_equal(sums_r[::-1], sums) and np.array_equal(infl_r[::-1], infl)
    got, c11 = tc.undo(fx['name'], fx, sums)
    assert np.array_equal(c11, got[1])                                   # a2 = c11 / 2 exactly
    y = fx['y'] if fx['name'] in tc.MINUS_Y else 0.0
    got_i = np.stack([infl[:, 0] + y, 2.0 * infl[:, 1]])
    if family == 'poisson':
        _poisson_check(fx, got, [1, 2, 3, 4], 'terms')
        _poisson_check(fx, got_i, [1, 2], 'influence')
        return
    for what, g, orders in (('terms', got, [1, 2, 3, 4]), ('influence', got_i, [1, 2])):
        rel, ab = _errors(family, fx, g, orders)
        bound = _bounds(fx, orders)
        host_rel = np.where(fx['resolvable'], fx['host_rel'], 0.0).max(-1)[orders]
        print(family, what, 'orders', orders, 'pointwise device', rel, 'host', host_rel, '| absolute device', ab, 'host',
              fx['host_abs'].max(-1)[orders], 'bound', bound)
        assert np.all(rel <= tc.CAP), (family, what, rel)
        assert np.all(ab <= bound), (family, what, ab, bound)


@pytest.mark.parametrize('family', tc.DISPERSION)
def test_dispersion_rows_and_position(vb, family):
    """`cross_local` of the dispersion entries: each row's E d_t h_l and E d_t^2 h_l / 2 (orders 1 and 2 of the fixture's four)."""
    fx = dict(_fx(family), name=family)
    N = fx['rho'].size
    assert N % 64 != 0
    fwd, rev = Rows(vb, family, np.arange(N)), Rows(vb, family, np.arange(N)[::-1])
    _, cl = fwd.dispersion()
    _, cl_r = rev.dispersion()
    fwd.close(); rev.close()
    assert np.all(np.isfinite(cl)) and np.array_equal(cl_r[::-1], cl)
    got = np.stack([cl[:, 0], 2.0 * cl[:, 1]])
    rel, ab = _errors(family, fx, got, [1, 2])
    bound = _bounds(fx, [1, 2])
    print(family, 'cross_local, E d_t h_l and E d_t^2 h_l: pointwise device', rel, 'host',
          np.where(fx['resolvable'], fx['host_rel'], 0.0).max(-1)[[1, 2]], '| absolute device', ab, 'host', fx['host_abs'].max(-1)[[1, 2]],
          'bound', bound)
    assert np.all(rel <= tc.CAP) and np.all(ab <= bound)


@pytest.mark.parametrize('family', tc.DISPERSION)
def test_dispersion_sums_by_decade_and_probes(vb, family):
    """d = (sum w h_l, sum w h_ll) as the value is checked: one call per decade of |exact| with weight 1 on the decade, the entries
    that are not resolvable in one more class under the absolute measure, and 16 single-row data sets."""
    fx = dict(_fx(family), name=family)
    N = fx['rho'].size
    sc = tc.scale(family, fx, fx['exact'])
    bounds = tc.abs_bounds(fx['host_abs'])
    rows = Rows(vb, family, np.arange(N))
    for j, k in ((0, 0), (1, 3)):                                        # d[0] is order 0 of the fixture (h_l), d[1] order 3 (h_ll)
        e = fx['exact'][k]
        dec = np.where(fx['resolvable'][k], np.floor(np.log10(np.abs(np.where(e == 0.0, 1.0, e)))), np.inf)
        worst, worst_abs = 0.0, 0.0
        for d in np.unique(dec):
            w = (dec == d).astype(np.float64)
            rows.ctx.set_weights(w)
            got = rows.dispersion()[0][j]
            want, size = math.fsum(w * e), math.fsum(w * np.abs(e))
            if np.isfinite(d):
                worst = max(worst, abs(got - want) / size)
                assert abs(got - want) <= tc.CAP * size, (family, j, d, got, want)
            else:
                worst_abs = max(worst_abs, abs(got - want) / math.fsum(w * sc[k]))
                assert abs(got - want) <= bounds[k] * math.fsum(w * sc[k]), (family, j, got, want)
        print(family, 'd[%d] by decade:' % j, np.unique(dec).size, 'classes, worst over sum |exact|', worst, '| unresolvable class, absolute',
              worst_abs, 'bound', bounds[k])
    rows.close()
    worst_host = np.argsort(-np.maximum(fx['host_abs'][0], fx['host_abs'][3]), kind='stable')[:10]
    th = np.flatnonzero(fx['kind'] == 2)
    picks = list(dict.fromkeys(list(worst_host) + list(th[np.linspace(0, th.size - 1, 6).astype(int)])))[:16]
    worst_rel, worst_abs = 0.0, 0.0
    for n in picks:
        rows = Rows(vb, family, np.array([n]))
        d = rows.dispersion()[0]
        rows.close()
        for j, k in ((0, 0), (1, 3)):
            err = abs(d[j] - fx['exact'][k, n])
            if fx['resolvable'][k, n]:
                worst_rel = max(worst_rel, err / abs(fx['exact'][k, n]))
                assert err <= tc.CAP * abs(fx['exact'][k, n]), (family, n, j)
            worst_abs = max(worst_abs, err / sc[k, n])
            assert err <= bounds[k] * sc[k, n], (family, n, j)
    print(family, 'single-row probes of d', len(picks), 'pointwise', worst_rel, 'absolute', worst_abs)


@pytest.mark.parametrize('family', tuple(PREDICT))
def test_response_means_on_new_rows(vb, family):
    """The predict entry on new rows that repeat the family's rows: its own rho and mean-field variance are the fixture's rho and s
    (asserted), and its mean-field mean is within 1e-12 of the exact mean -- the bound of the existing predict tests
    (tests/test_gpu_glmm_ztnegbin.py).  Rows up to the offset 600, just below the overflow of exp, are part of it."""
    fx = _fx(family)
    N = fx['rho'].size
    rows = Rows(vb, family, np.arange(N))
    out = rows.predict_new_rows()
    rows.close()
    assert out.shape == (5, N)
    assert np.all(np.abs(out[0] - fx['rho']) <= 1e-12 * np.abs(fx['rho'])) and np.all(np.abs(out[1] - fx['s']) <= 1e-12 * fx['s'])
    keep = np.isfinite(fx['mean'])
    assert keep.all() or family in ('ztpoisson', 'ztnegbin', 'cloglog')
    if family in ('ztpoisson', 'ztnegbin', 'cloglog'):
        assert np.any(fx['rho'][keep] == tc.NEAR_OVERFLOW)
    want = fx['mean'] * (fx['trials'] if family in ('probit', 'cloglog') else 1.0)
    err = tc.rel_err(out[3][keep], want[keep])
    print(family, 'mean-field response mean on', int(keep.sum()), 'new rows, worst relative error', float(err.max()))
    assert np.all(err <= 1e-12)


def _undo_value(fx, val, w):
    """The entry's value plus the sum w y rho it subtracted."""
    if fx['name'] not in tc.MINUS_Y:
        return val
    return val + math.fsum(w * fx['y'] * fx['rho'])


@pytest.mark.parametrize('family', FAMILIES)
def test_value_by_decade(vb, family):
    """One call per decade of |exact[0]| with weight 1 on the decade's rows and 0 elsewhere: the class sum within CAP of
    sum |exact[0]|.  The rows whose value the entry cannot resolve (device mask) form one more class under the absolute measure."""
    fx = dict(_fx(family), name=ENTRIES[family][0])
    N = fx['rho'].size
    e0 = fx['exact'][0]
    mask = tc.device_mask(fx['name'], fx)[0]
    dec = np.where(mask, np.floor(np.log10(np.abs(np.where(e0 == 0.0, 1.0, e0)))), np.inf)
    rows = Rows(vb, family, np.arange(N))
    bound0 = _bounds(fx, [0])[0]
    sc0 = tc.scale(fx['name'], fx, fx['exact'])[0]
    worst, worst_abs = 0.0, 0.0
    for d in np.unique(dec):
        w = (dec == d).astype(np.float64)
        rows.ctx.set_weights(w)
        val = _undo_value(fx, rows.terms()[0], w)
        want, size = math.fsum(w * e0), math.fsum(w * np.abs(e0))
        if np.isfinite(d):
            if family == 'poisson':
                tol = float(np.max((np.abs(fx['rho'] + 0.5 * fx['s']) + 4.0)[w > 0]) * 2.0 ** -52) * size
            else:
                tol = tc.CAP * size
            worst = max(worst, abs(val - want) / size)
            assert abs(val - want) <= tol, (family, d, val, want)
        else:
            worst_abs = max(worst_abs, abs(val - want) / math.fsum(w * sc0))
            assert abs(val - want) <= bound0 * math.fsum(w * sc0), (family, val, want)
    rows.close()
    print(family, 'value by decade:', np.unique(dec).size, 'classes, worst class error over sum |exact|', worst,
          '| unresolvable class, absolute', worst_abs, 'bound', bound0)


@pytest.mark.parametrize('family', FAMILIES)
def test_value_single_row_probes(vb, family):
    """16 data sets of ONE row: where the host formula's value is worst, and threshold rows spread over the branches."""
    fx = dict(_fx(family), name=ENTRIES[family][0])
    worst_host = np.argsort(-fx['host_abs'][0], kind='stable')[:10]
    th = np.flatnonzero(fx['kind'] == 2)
    picks = list(dict.fromkeys(list(worst_host) + list(th[np.linspace(0, th.size - 1, 6).astype(int)])))[:16]
    mask = tc.device_mask(fx['name'], fx)[0]
    bound0 = _bounds(fx, [0])[0]
    sc0 = tc.scale(fx['name'], fx, fx['exact'])[0]
    worst_rel, worst_abs = 0.0, 0.0
    for n in picks:
        rows = Rows(vb, family, np.array([n]))
        w = np.zeros(fx['rho'].size)
        w[n] = 1.0
        val = _undo_value(fx, rows.terms()[0], w)
        rows.close()
        want = fx['exact'][0, n]
        err = abs(val - want)
        if family == 'poisson':
            assert err <= (abs(fx['rho'][n] + 0.5 * fx['s'][n]) + 4.0) * 2.0 ** -52 * want
            continue
        if mask[n]:
            worst_rel = max(worst_rel, err / abs(want))
            assert err <= tc.CAP * abs(want), (family, n, val, want)
        worst_abs = max(worst_abs, err / sc0[n])
        assert err <= bound0 * sc0[n], (family, n, val, want)
    print(family, 'single-row value probes', len(picks), 'pointwise', worst_rel, 'absolute', worst_abs, 'bound', bound0)


@pytest.mark.parametrize('family', REFUSING)
def test_refusal_next_to_extreme_rows(vb, family):
    """The refusals stay: with one row at t = -760 (e^t = 0 on its node: r = 0 / 0, R = 1 / 0) the entry raises and leaves no sums
    resident; without it the next call returns the bits it returned before."""
    hip = vb._hip
    fx = _fx(family)
    N = fx['rho'].size
    rows = Rows(vb, family, np.arange(N))
    ctx = rows.ctx
    loc, sc, cl, M = np.tile(np.eye(2)[np.triu_indices(2)], (N, 1)), np.ones((N, 2)), np.zeros((N, 2, 3)), np.empty((5, 5))
    schur = lambda: ctx._lib.lrvb_glmm_slopes_schur(ctx._h, loc.ctypes.data, sc.ctypes.data, cl.ctypes.data, N, 1, M.ctypes.data)
    val, sums = rows.terms()
    assert schur() != hip.ERR_STATE                                      # sums are resident
    n = int(np.flatnonzero((fx['y'] > 0.0) & (fx['s'] == tc.S_MIN))[0])         # a row with a success: its h1 is evaluated on the node
    bad = fx['rho'].copy()
    bad[n] = -760.0
    ctx.set_offset(bad)
    with pytest.raises(ValueError, match='not finite'):
        rows.terms()
    assert schur() == hip.ERR_STATE                                      # no sums left resident
    ctx.set_offset(fx['rho'])
    val2, sums2 = rows.terms()
    assert val2 == val and np.array_equal(sums2, sums)
    rows.close()

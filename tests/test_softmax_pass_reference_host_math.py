"""CPU checks of tests/softmax_pass_reference.py: the dispatch table covers every instance of
`softmax_pass_kernel` at two or more trips; the longdouble reference agrees with the mpmath rows of
tests/golden/softmax_pass_probes.npz, with tests/softmax_reference.py and with torch autograd; the exactness claims of the
integer design hold in `fractions` arithmetic; the float64 restatement of the kernel's order passes every assertion the device
has to pass; each restated fault fails at least one case of the GPU file."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import softmax_pass_reference as sp
import softmax_reference as sr

LD = sp.LD


def make(c, aligned):
    return sp.F64Backend(c, aligned)


def mutant(mut):
    return lambda c, aligned: sp.F64Backend(c, aligned, mut=mut)


# ---- the dispatch table -----------------------------------------------------------------------------------------------------
def _reached(min_trips):
    got = set()
    for (N, P, K, aligned) in sp.REAL_CASES + sp.EXACT_CASES:
        if sp.full_trips(N) < min_trips:                           # a trip of one row does not count
            continue
        for f in sp.wave_flags(P, aligned):
            for mode in sp.MODES:                                  # every case runs all three modes over all N rows
                got.add((mode,) + sp.dispatch(P, aligned, mode, f != 0))
    return got


def test_dispatch_table_has_the_launched_instances():
    inst = sp.all_instances()
    assert len(inst) == 59                                         # 19 gradient (no 8-wave NB = 8), 20 product, 20 rows-only
    assert sp.dispatch(1024, True, sp.GRAD) == (8, 4, False)       # the exception
    assert sp.dispatch(1024, True, sp.HVP) == (8, 8, False) and sp.dispatch(1024, True, sp.ROWS) == (8, 8, False)
    assert sp.dispatch(1024, True, sp.HVP, True) == (8, 4, False)
    assert sp.dispatch(130, False, sp.HVP) == (2, 4, True) and sp.dispatch(129, True, sp.ROWS) == (2, 4, True)
    assert sp.dispatch(128, True, sp.HVP) == (1, 4, False) and sp.dispatch(256, True, sp.GRAD) == (2, 8, False)
    for P in range(1, 1025):
        for aligned in (True, False):
            for mode in sp.MODES:
                for four in (False, True):
                    assert (mode,) + sp.dispatch(P, aligned, mode, four) in inst


def test_every_instance_is_reached_at_two_trips_and_every_pair_at_three():
    missing = sp.all_instances() - _reached(2)
    assert not missing, 'instances no GPU case reaches at two or more trips: {}'.format(sorted(missing))
    three = _reached(3)
    for mode in sp.MODES:
        pairs = {(nw, odd) for (m, nb, nw, odd) in three if m == mode}
        assert pairs == {(4, True), (4, False), (8, False)}, (mode, pairs)
    for (P, K, Q) in sp.INFL_CASES:                                # the influence windows: three trips in the rows-only mode
        assert sp.trips(sp.INFL_N) == 3 and sp.full_trips(sp.INFL_N) == 2
        G = 16 // (K - 1)
        assert Q > G or K == 2 or Q % G != 0
    assert any(K - 1 == 5 for _, K, _ in sp.INFL_CASES) and any(K - 1 == 16 for _, K, _ in sp.INFL_CASES)
    assert any(Q > 16 // (K - 1) and Q % (16 // (K - 1)) != 0 for _, K, Q in sp.INFL_CASES)
    assert sp.trips(2049) == 2 and sp.trips(4097) == 3 and sp.trips(6145) == 4 and sp.trips(2048) == 1
    assert sp.full_trips(2049) == 1 and sp.full_trips(sp.N_TWO_TRIPS) == 2 and sp.full_trips(4097) == 2 and sp.full_trips(6145) == 3


def test_case_lists_cover_the_grids():
    for cases, klist in ((sp.REAL_CASES, sp.K_REAL), (sp.EXACT_CASES, sp.K_EXACT)):
        assert {K for _, _, K, _ in cases} == set(klist)
        for P in sp.P_EVEN + sp.P_ODD:
            assert {N for N, p, _, _ in cases if p == P} >= {9, sp.N_TWO_TRIPS}
        for P in sp.P_ROWGRID:
            assert {N for N, p, _, al in cases if p == P and al} >= set(sp.N_GRID)
        assert {N for N, p, _, al in cases if not al} == {9, sp.N_TWO_TRIPS, 4097}
        assert {K - 1 for N, _, K, _ in cases if sp.trips(N) >= 3} >= {1, max(klist) - 1}


# ---- the inputs are what they claim ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K', [(6145, 130, 17), (17, 40, 5), (9, 3, 2), (2049, 20, 8)])
def test_real_case_design(N, P, K):
    c = sp.real_case(N, P, K)
    X, w, y, beta = c['X'], c['w'], c['y'], c['beta']
    Km = K - 1
    assert np.all(X[:, 0] == 1.0) and np.all(beta[:, 0] == 0.0)
    assert np.any(w == 0.0) and w[0] > 0.0
    z = sr.logits(X, beta)[:, 1:]
    kinds = set()
    for (r, kind, j) in c['plan']:
        assert np.flatnonzero(X[:, j]).tolist() == [r] and X[r, j] == 1.0          # an indicator column
        kinds.add(kind)
        if kind == 'probe':
            continue
        assert np.array_equal(z[r], sp.extreme_logits(kind, Km)), kind            # the logits hold exactly
        assert w[r] > 0.0
    zz = {k: sp.extreme_logits(k, Km) for k in sp.EXTREME_KINDS}
    assert np.all(zz['ref max'] < 0)
    assert np.argmax(zz['lane0 max']) == 0 and zz['lane0 max'][0] > 0
    assert np.argmax(zz['last max']) == Km - 1 and zz['last max'][Km - 1] > 0
    assert (zz['tie'][0] == zz['tie'][Km - 1] == zz['tie'].max()) if Km > 1 else zz['tie'][0] == 0.0
    assert np.all(zz['all low'] <= -750) and np.all(np.exp(zz['all low']) == 0.0)
    assert zz['gap 30'].max() == 30 and zz['gap 700'].max() == 700 and np.exp(-700.0) > 2.0 ** -1022
    if P >= 40:
        assert kinds >= set(sp.EXTREME_KINDS) | {'probe'}
        rows = {r for r, _, _ in c['plan']}
        assert rows >= {r for r in sp.PROBE_ROWS if r < N} | {N - 1}
        assert {int(y[r]) for r, k, _ in c['plan']} >= {0, 1, K - 1}
        assert w[7] == 0.0
        if N % 8:
            assert ('gap 700 last' in kinds) and N - 1 in rows
    assert np.abs(z[[n for n in range(N) if n not in {r for r, k, _ in c['plan'] if k != 'probe'}]]).max() < 40


def test_exact_design_is_aperiodic_against_the_chunk_and_the_grid():
    c = sp.exact_case(6145, 130, 16)
    for v in (c['kind'], c['w'], c['y']):
        for lag in (4, 8, 2048, 4096):
            assert np.mean(v[lag:] != v[:-lag]) > 0.4, lag
    assert set(c['kind'].tolist()) == {-1, 0, 1}
    assert not np.any(sp.exact_case(300, 9, 4, saturated_only=True)['kind'] == 0)


@pytest.mark.parametrize('N,P,K', [(37, 5, 4), (21, 2, 16), (19, 1, 2), (26, 7, 8)])
def test_exactness_claims_in_fractions(N, P, K):
    """Definitions in `fractions`, with the saturation facts (exp(0) = 1, exp(x) = 0 for x <= -745.2 in float64) checked
    on the actual logits: p, r, gradient, u, product, influence rows, Hessian blocks and the saturated value are what
    `exact_outputs` / `exact_hessian` return, and all are exactly representable."""
    c = sp.exact_case(N, P, K)
    e = sp.exact_outputs(c)
    Km = K - 1
    X = [[Fraction(int(v)) for v in row] for row in c['X']]
    z = sr.logits(c['X'], c['beta'])
    assert np.array_equal(z[:, 1:], np.outer(c['kind'], 1000.0 * (np.arange(Km) + 1)))
    p = []
    for n in range(N):
        m = max(z[n].max(), 0.0)
        ex = np.exp(z[n] - m)
        assert set(ex.tolist()) <= {0.0, 1.0}                      # every exp argument is 0 or <= -1000
        s = int(ex.sum())
        p.append([Fraction(int(ex[a + 1]), s) for a in range(Km)])
    E = sp.onehot(c['y'], Km)
    w = [Fraction(int(v)) for v in c['w']]
    r = [[w[n] * (p[n][a] - int(E[n, a])) for a in range(Km)] for n in range(N)]
    g = [[sum(r[n][a] * X[n][j] for n in range(N)) for j in range(P)] for a in range(Km)]
    V = [[Fraction(int(v)) for v in row] for row in c['V']]
    t = [[sum(X[n][j] * V[a][j] for j in range(P)) for a in range(Km)] for n in range(N)]
    u = [[w[n] * p[n][a] * (t[n][a] - sum(p[n][b] * t[n][b] for b in range(Km))) for a in range(Km)] for n in range(N)]
    hv = [[sum(u[n][a] * X[n][j] for n in range(N)) for j in range(P)] for a in range(Km)]

    def same(fr, arr):
        flat = [v for row in fr for v in row]
        got = np.asarray(arr).ravel()
        assert len(flat) == got.size
        for v, x in zip(flat, got):
            assert Fraction(float(x)) == v                         # bit for bit: the float64 IS the rational
    same(p, e['p']); same(r, e['r']); same(g, e['g']); same(u, e['u']); same(hv, e['hv'])
    Q = c['A'].shape[0]
    A = c['A'].astype(np.int64).reshape(Q, Km, P)
    infl = [[sum((p[n][a] - int(E[n, a])) * int(np.dot(A[q, a], c['X'][n].astype(np.int64))) for a in range(Km)) for q in range(Q)]
            for n in range(N)]
    same(infl, e['infl'])
    H = sp.exact_hessian(c)
    for (a, b) in ((0, 0), (0, Km - 1), (Km - 1, Km - 1), (Km // 2, 0)):
        col = [w[n] * p[n][a] * ((1 if a == b else 0) - p[n][b]) for n in range(N)]
        blk = [[sum(col[n] * X[n][i] * X[n][j] for n in range(N)) for j in range(P)] for i in range(P)]
        same(blk, H[a * P:(a + 1) * P, b * P:(b + 1) * P])
    assert np.array_equal(H, H.T)
    cs = sp.exact_case(N, P, K, saturated_only=True)
    val = sum(Fraction(int(cs['w'][n])) * int(max(sr.logits(cs['X'], cs['beta'])[n].max(), 0) - sr.logits(cs['X'], cs['beta'])[n, cs['y'][n]])
              for n in range(N))
    assert Fraction(sp.exact_outputs(cs)['value_sat']) == val


def test_exact_magnitudes_stay_far_below_2_53_at_the_largest_cases():
    for (N, P, K) in [(6145, 1024, 8), (6145, 130, 16), (4099, 1024, 2), (2049, 1024, 16)]:
        sp.exact_outputs(sp.exact_case(N, P, K))                   # asserts |K^2 x| < 2^52 inside
    sp.exact_hessian(sp.exact_case(300, 66, 16))


# ---- the longdouble reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,P,K', sp.GOLDEN_CASES)
def test_longdouble_reference_against_mpmath_rows(N, P, K):
    """Every row of the golden cases (all extreme kinds among them): the longdouble reference is within 1/16 of the bound of
    the mpmath value, and within 64 units of ITS roundoff 2^-64 of it relative to the bound's magnitudes."""
    c = sp.real_case(N, P, K)
    ref = sp.ld_eval(c)
    bnd = sp.bounds(c, ref)
    with np.load(sp.GOLDEN) as z:
        name = '{}_{}_{}'.format(N, P, K)
        mp = {k: z[name + '/' + k + '_hi'].astype(LD) + z[name + '/' + k + '_lo'].astype(LD) for k in ('p', 'vterm', 'r', 'u')}
    for key, B in (('p', bnd['p']), ('vterm', bnd['vterm']), ('r', bnd['r']), ('u', bnd['u'])):
        ratio = sp.max_ratio(np.zeros(B.shape), ref[key] - mp[key], B)
        print('softmax pass longdouble against mpmath {} {} {:.2e}'.format(name, key, ratio))
        assert ratio <= 1.0 / 16.0, (key, ratio)
    sel = np.asarray(mp['p'], dtype=np.float64) > 2.0 ** -1000
    rel = np.abs(ref['p'] - mp['p'])[sel] / mp['p'][sel]
    assert float(rel.max()) <= 800 * 2.0 ** -64                    # 700-unit logit gaps: the argument's rounding alone is 700 2^-64


@pytest.mark.parametrize('N,P,K', [(300, 7, 3), (203, 34, 17), (50, 2, 2)])
def test_longdouble_reference_against_numpy_and_autograd(N, P, K):
    c = sp.real_case(N, P, K)
    ref = sp.ld_eval(c)
    x, y, w, beta, V = c['X'], c['y'], c['w'], c['beta'], c['V']
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.max(np.abs(b)))
    assert abs(float(ref['value']) - sr.value(x, y, w, beta)) <= 1e-12 * abs(sr.value(x, y, w, beta))
    assert rel(ref['g'], sr.grad(x, y, w, beta)) <= 1e-12
    assert rel(ref['hv'], sr.hvp(x, w, beta, V.ravel())) <= 1e-11
    assert rel(ref['p'], sr.probs(x, beta)) <= 1e-12
    A = c['A']
    iref, _, _ = sp.ld_influence(c, ref, A, 0, N)
    assert rel(iref, (A @ sr.cross_hessian(x, y, beta)).T) <= 1e-11
    X, W, Y = torch.as_tensor(x), torch.as_tensor(w), torch.as_tensor(y, dtype=torch.long)
    th = torch.tensor(beta.ravel(), requires_grad=True)
    zt = torch.cat([torch.zeros(N, 1, dtype=torch.float64), X @ th.reshape(K - 1, P).T], dim=1)
    val = (W * (torch.logsumexp(zt, dim=1) - zt[torch.arange(N), Y])).sum()
    g, = torch.autograd.grad(val, th, create_graph=True)
    hv, = torch.autograd.grad(g @ torch.as_tensor(V.ravel()), th)
    assert abs(float(ref['value']) - val.item()) <= 1e-12 * abs(val.item())
    assert rel(ref['g'], g.detach().numpy()) <= 1e-11 and rel(ref['hv'], hv.numpy()) <= 1e-11


# ---- the float64 restatement through the device's assertions -------------------------------------------------------------
CHEAP_REAL = [c for c in sp.REAL_CASES if sp.is_cheap(c[0], c[1], c[2])]
CHEAP_EXACT = [c for c in sp.EXACT_CASES if sp.is_cheap(c[0], c[1], c[2])]
LARGE = [(2121, 1024, 3, True), (4097, 130, 16, True), (4097, 129, 17, True), (6145, 2, 17, True)]


def test_restatement_inside_every_bound_on_real_data():
    worst = {}
    cases = CHEAP_REAL + [c for c in LARGE if c in sp.REAL_CASES]
    assert len(cases) >= 60
    for (N, P, K, aligned) in cases:
        for k, v in sp.check_real_case(make, N, P, K, aligned).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('softmax pass restatement worst ratios', {k: round(v, 4) for k, v in sorted(worst.items())})
    assert set(worst) == {'value', 'gradient', 'product', 'influence', 'p'} and max(worst.values()) <= 1.0


def test_restatement_bitwise_on_exact_data():
    cases = CHEAP_EXACT + [c for c in [(4097, 130, 16, True), (4097, 129, 16, True), (6145, 2, 16, True)] if c in sp.EXACT_CASES]
    assert len(cases) >= 60
    for (N, P, K, aligned) in cases:
        sp.check_exact_case(make, N, P, K, aligned)


@pytest.mark.parametrize('P,K,Q', [(130, 6, 7), (2, 17, 2), (129, 4, 11)])
def test_restatement_on_the_influence_windows(P, K, Q):
    r = sp.check_influence_windows(make, P, K, Q)
    print('softmax pass restatement influence windows', P, K, Q, round(r['influence'], 4))


@pytest.mark.parametrize('N,P,K', [(300, 9, 16), (77, 3, 4)])
def test_restatement_hessian_bitwise(N, P, K):
    sp.check_hessian(make, N, P, K)


# ---- the mutation catalogue -------------------------------------------------------------------------------------------------
def _pick(cases, shapes):
    return [next(c for c in cases if (c[0], c[1]) == s and c[3]) for s in shapes]


ONE_TRIP = _pick(sp.EXACT_CASES, [(9, 130), (2047, 130), (17, 129), (2048, 2)])
MULTI_TRIP = _pick(sp.EXACT_CASES, [(2121, 130), (4097, 129), (2121, 258)])


def _fails(check, mk, *args):
    try:
        check(mk, *args)
    except AssertionError:
        return True
    return False


def _real_cases_for_kill():
    have = [c for c in sp.REAL_CASES if c[0] in (17, 2121, 4097) and c[1] in (129, 130)]
    assert len(have) >= 4
    return have


@pytest.mark.parametrize('mut', sp.PASS_MUTATIONS)
def test_every_restated_fault_fails_a_gpu_case(mut):
    """Each fault, applied to the restatement, breaks bitwise equality on the exact design AND leaves a bound on real data in
    cases of the GPU file.  The stale-half and slot faults are invisible to every one-trip case of the exact oracle (what the
    suite could see before) when modelled from the second trip on, and fail every multi-trip case."""
    mk = mutant(mut)
    exact_multi = [c for c in MULTI_TRIP if _fails(sp.check_exact_case, mk, *c)]
    exact_one = [c for c in ONE_TRIP if _fails(sp.check_exact_case, mk, *c)]
    real = [c for c in _real_cases_for_kill() if _fails(sp.check_real_case, mk, *c)]
    print('softmax pass mutation {!r}: exact one-trip {}/{}, exact multi-trip {}/{}, real {}/{}'.format(
        mut, len(exact_one), len(ONE_TRIP), len(exact_multi), len(MULTI_TRIP), len(real), len(_real_cases_for_kill())))
    assert len(exact_multi) == len(MULTI_TRIP)
    if mut.startswith('stale'):
        assert not exact_one
    elif mut == 'phantom row weighted':                             # needs a ragged last chunk
        assert exact_one == [c for c in ONE_TRIP if c[0] % 8]
    elif mut == 'm not clamped':                                    # a -1 row has m = -1000 Km .. : exp(-m) overflows
        assert exact_one
    else:
        assert exact_one
    assert real, 'no real-data case notices'


@pytest.mark.parametrize('mut', sp.ROWS_MUTATIONS)
def test_every_restated_fault_of_the_rows_mode_fails(mut):
    mk = mutant(mut)
    assert _fails(sp.check_influence_windows, mk, 130, 6, 7)
    assert _fails(sp.check_exact_case, mk, *MULTI_TRIP[0])


def test_unmutated_restatement_passes_the_kill_cases():
    for c in ONE_TRIP + MULTI_TRIP:
        sp.check_exact_case(make, *c)
    for c in _real_cases_for_kill():
        sp.check_real_case(make, *c)

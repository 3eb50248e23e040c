"""tests/mixture_rows_reference.py on the CPU: the reference agrees with the project's oracle and with
exact AD of the torch restatement, every problem builder stays inside its design for every case the GPU file uses, the
bounds hold for a plain float64 evaluation and fail for the mistakes the GPU tests are there to catch, and the calibration of
the conditioning-limited bound."""
import numpy as np
import pytest
import torch

import torch_ref as tr
from oracle import mixture as om
import mixture_rows_reference as mr


@pytest.mark.parametrize('N,V,K', [(12, 3, 2), (25, 4, 3), (30, 5, 4), (20, 7, 8)])
def test_reference_matches_oracle_and_mpmath(N, V, K):
    pr = mr.routed_problem(N, V, K, 'cycle', seed=11)
    ev = mr.evaluate(pr['fz'], pr['x'], pr['w'], pr['lam'], keep_A=range(N))
    o_val2, o_g, o_H, o_S64, o_R = om.mixture_rows(pr['fz'].ravel(), pr['x'], pr['w'], pr['lam'])
    assert np.all(np.abs(o_val2 - ev['val2']) <= 16 * ev['val2_bound'])          # the oracle sums N terms in sequence
    assert mr.max_ratio(o_g, ev['gz'], ev['gz_bound']) <= 1.0
    assert mr.max_ratio(o_S64, ev['S64'], ev['S64_bound']) <= 1.0
    assert np.max(np.abs(o_R - ev['R'])) <= 1e-11 * np.max(np.abs(o_R))          # the oracle solves the unscaled block
    for n in range(N):
        z, gz, A = mr.mp_row_of(pr, n)
        assert np.max(np.abs(z - ev['z'][n]) / z) <= 2 * mr.U
        assert np.all(np.abs(gz - ev['gz'][n]) <= ev['gz_bound'][n])
        assert ev['ld_A'] and mr.a_error(ev['A_rows'][n], A) <= 1.5 * mr.U              # longdouble Woodbury, rounded to float64, against mpmath
        # the oracle's free Hessian block is the H of mp_row: J H^-1 J^T from it
        p = ev['z'][n]
        J = np.diag(p)[:, 1:] - np.outer(p, p[1:])
        assert mr.a_error(J @ np.linalg.solve(o_H[n], J.T), A) <= 1e3 * mr.U * np.linalg.cond(o_H[n])


@pytest.mark.parametrize('N,V,K', [(9, 3, 3), (7, 4, 4)])
def test_reference_matches_exact_ad(N, V, K):
    """Value, local gradient and the block-diagonal local Hessian of the torch restatement of the whole -ELBO: the rows enter it
    through val2 and nothing else depends on the logits, so AD in the logits at fixed globals is the row kernel's mathematics."""
    from scipy import special
    pr = mr.routed_problem(N, V, K, 'cycle', seed=5)
    rng = np.random.default_rng(0)
    fg = rng.normal(size=K + V * K) * 0.3 + 0.5
    alpha, beta = np.exp(fg[:K]), np.exp(fg[K:]).reshape(V, K)
    lam = np.vstack([special.digamma(alpha) - special.digamma(alpha.sum()),
                     special.digamma(beta) - special.digamma(beta.sum(0, keepdims=True))])
    x = pr['x']
    fz = (np.hstack([np.ones((N, 1)), x]) @ lam)
    fz = fz[:, 1:] - fz[:, :1] + 0.1 * rng.normal(size=(N, K - 1))
    ev = mr.evaluate(fz, x, pr['w'], lam, keep_A=range(N))
    ft = tr.mixture_objective(x, K, 1.5, 0.8)
    tw = torch.tensor(pr['w'])
    tg = torch.tensor(fg)
    fl = lambda z: ft(torch.cat([tg, z]), tw)
    tz = torch.tensor(fz.ravel())
    g_ad = torch.func.grad(fl)(tz).numpy().reshape(N, K - 1)
    np.testing.assert_allclose(ev['gz'], g_ad, rtol=1e-11, atol=1e-12)
    H_ad = torch.func.hessian(fl)(tz).numpy()
    for n in range(N):
        sl = slice(n * (K - 1), (n + 1) * (K - 1))
        p = ev['z'][n]
        J = np.diag(p)[:, 1:] - np.outer(p, p[1:])
        A_ad = J @ np.linalg.solve(H_ad[sl, sl], J.T)
        assert mr.a_error(ev['A_rows'][n], A_ad) <= 1e-10
    # the value: the two sums are the only terms of the -ELBO that move with the logits
    z0 = torch.tensor((fz + 0.05).ravel())
    ev0 = mr.evaluate(fz + 0.05, x, pr['w'], lam, want_A=False)
    assert abs((fl(tz) - fl(z0)).item() - (ev['val2'].sum() - ev0['val2'].sum())) <= 1e-11 * abs(ev['val2']).sum()


def test_restatements_agree_and_mistakes_are_seen():
    """Both float64 restatements against the mpmath truth inside a few hundred U kappa, and the bound 8 unit_n rejects the
    results of the mistakes of the mutation check: categories un-swapped on one side only, Woodbury on a dense row's neighbour,
    a stale weight."""
    pr = mr.routed_case(61, 5, 4)
    P = mr._prelude(pr['fz'], pr['x'], pr['w'], pr['lam'], np.float64)
    Aw = mr.woodbury_A(P['p'], P['g'], pr['w'], P['m'])
    Ac = mr.scaled_cholesky_A(P['p'], P['g'], pr['w'], P['m'])
    seen = 0
    for n in range(pr['N']):
        A = mr.mp_row_of(pr, n)[2]
        route, kappa, e_w, e_c = mr.calibrate_row(pr, n)
        unit = mr.probe_unit(pr, n)
        assert e_w <= 300 * mr.U * kappa and e_c <= 300 * mr.U * kappa
        assert mr.a_error(Ac[n], A) <= mr.A_FACTOR * unit and (route == 'dense' or mr.a_error(Aw[n], A) <= mr.A_FACTOR * unit)
        m = int(P['m'][n])
        if m != 0:
            perm = np.arange(pr['K']); perm[[0, m]] = perm[[m, 0]]
            assert mr.a_error(A[:, perm], A) > 1e6 * mr.A_FACTOR * unit           # columns un-swapped, rows not
            seen += 1
        nb = n ^ 1
        if nb < pr['N']:
            assert mr.a_error(mr.mp_row_of(pr, nb)[2], A) > 1e6 * mr.A_FACTOR * unit   # the pair partner's row in this row's place
        w_stale = pr['w'].copy(); w_stale[n] = pr['w'][(n + 7) % pr['N']]
        Ps = mr._prelude(pr['fz'][n:n + 1], pr['x'][n:n + 1], w_stale[n:n + 1], pr['lam'], np.float64)
        assert mr.a_error(mr.scaled_cholesky_A(Ps['p'], Ps['g'], w_stale[n:n + 1])[0], A) > 1e3 * mr.A_FACTOR * unit
    assert seen > 10


@pytest.mark.parametrize('case', [c for c, _ in mr.all_cases()], ids=lambda c: '-'.join(str(v) for v in c))
def test_builders_stay_inside_their_design(case):
    """The builders assert their own design when they run (check_design, the probe assertions); here additionally what the
    GPU file relies on: both routes present where routing is mixed, the pair kinds, the trips, the probes' properties."""
    pr = dict(mr.all_cases())[case]()
    N, K = pr['N'], pr['K']
    rt = mr.check_design(pr)
    dense = rt['dmin_w'] <= mr.FAST_THRESHOLD
    assert np.array_equal(dense, pr['dense'])
    assert not np.any((rt['dmin_w'] > mr.DENSE_BAND[1]) & (rt['dmin_w'] < mr.FAST_MIN))
    if case[0] == 'grid':
        assert not dense.any() and mr.trips(N)[0] == (3 if N == 65539 else 2)
    elif case[0] == 'store':
        tri = K * (K + 1) // 2
        pairs = (tri + (tri & 1)) // 2
        assert not dense.any() and N > 2048 and (pairs - 1) % 64 >= 12              # the last store segment reaches lane 12
    else:
        pairs = set((bool(dense[i]), bool(dense[i + 1])) for i in range(0, N - 1, 2))
        want = {(False, True)} if N == 2 else {(False, True), (True, False), (True, True), (False, False)}
        assert want <= pairs
        assert N % 2 == 0 or case[0] == 'probe' or dense[-1]                     # a dense odd last row
    if case[0] == 'probe':
        kinds = [q['kind'] for q in pr['probes']]
        assert {'fast', 'dense', 'tie', 'zero', 'sat12', 'sat200'} <= set(kinds)
        ms = set(q['m'] for q in pr['probes'])
        if case[4] == 'all':
            assert {0, 1, 15, 16, K - 1} <= ms
            assert set(mr.grid_probe_positions()) == set(q['n'] for q in pr['probes'])
        else:
            assert {0, 1, K - 1} <= ms
        assert len(set(q['j'] for q in pr['probes'])) == len(pr['probes'])
    if case == ('routed',) + mr.ROUTED_BIG:
        for kind in ('dense', 'fast', 'last'):
            bad = mr.with_indefinite_row(pr, kind)                                  # asserts: exactly this row is indefinite
            n = bad['bad_row']
            assert np.array_equal(np.flatnonzero(np.any(bad['fz'] != pr['fz'], axis=1)), [n])
            assert (kind != 'dense' or n >= 32768) and (kind != 'last' or n == N - 1) and (kind != 'fast' or not pr['dense'][n])


@pytest.mark.parametrize('case', [c for c, _ in mr.all_cases()], ids=lambda c: '-'.join(str(v) for v in c))
def test_calibration(case, capsys):
    """e_n of the float64 restatement of each row's route in units of U kappa_n, for EVERY row of the case (8192 rows -- largest
    kappa, even strides, all probes -- of the two K = 32 cases above LD_BUDGET): below the constant recorded in mr.CAL for its
    route and K, and below the few hundred U kappa past which a restatement would be wrong.  The truth is the longdouble
    Woodbury form of `evaluate`, checked here against mpmath on the probes and on the rows of largest kappa and largest e."""
    pr = dict(mr.all_cases())[case]()
    K, N = pr['K'], pr['N']
    rows = np.arange(N) if N * K * K <= mr.LD_BUDGET else np.array(mr.calibration_rows(pr, 8192))
    ev = mr.evaluate(pr['fz'][rows], pr['x'][rows], pr['w'][rows], pr['lam'], keep_A=range(rows.size))
    assert ev['ld_A']
    ratio = ev['e'] / (mr.U * ev['kappa'])
    for q in pr.get('probes', ()):
        if q['kind'] == 'sat200':
            i = int(np.flatnonzero(rows == q['n'])[0])
            assert ratio[i] <= mr.CAL_SAT200
            ratio[i] = 0.0
    worst = {}
    for route, sel in (('fast', ~ev['dense']), ('dense', ev['dense'])):
        if sel.any():
            worst[route] = float(ratio[sel].max())
            assert worst[route] <= mr.CAL[(route, K)] <= 300, (route, worst[route])
    check = set(int(np.flatnonzero(rows == q['n'])[0]) for q in pr.get('probes', ()))
    check.update(np.argsort(ev['kappa'])[-2:].tolist() + np.argsort(ratio)[-2:].tolist() + [0, rows.size - 1])
    for i in check:
        A = mr.mp_row_of(pr, int(rows[i]))[2]
        assert mr.a_error(ev['A_rows'][i], A) <= max(1.5 * mr.U, 0.25 * ev['unit'][i])       # float64 rounding, or a quarter unit
    with capsys.disabled():
        print('\n[calibration {}] {} rows, max e / (U kappa): {}'.format(case, rows.size, ' '.join('{} {:.1f}'.format(*kv) for kv in worst.items())))

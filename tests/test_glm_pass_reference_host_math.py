"""The oracles of tests/test_gpu_glm_pass.py are fair and sharp, shown on the CPU before any GPU is involved
(tests/glm_pass_reference.py): at every shape of the GPU file the int64 reference is the longdouble
one and every partial sum stays an exact float64, beta of the real cases keeps |z| <= 30, an honest float64 evaluation sits
inside the derived bound, and each mistake the pass can make -- a dropped last row, the row past N counted, a row given its
stage partner's y and w, the previous stage's z, one wave's columns missing from z, two exchanged output columns, a block
missing from the reducer, a workgroup's value partial missing -- breaks the exact comparison and leaves the bound by at
least 100 x.  The norm-wise `helpers.rel_err` at 1e-10, the only check the pass had, does not see a wrong small column."""
import numpy as np
import pytest

import glm_pass_reference as gr
from helpers import rel_err

SHARP = 100.0
LD_ENTRIES = 1 << 22                       # above this many entries of X the integer case is replayed in float64, not longdouble


def test_launch_geometry():
    """The helpers reproduce the launcher at the sizes the shape lists were chosen for."""
    narrow = {N: gr.plan(N, 130) for N in gr.NARROW_N}
    assert [narrow[N]['nblk_hi'] for N in (1, 8, 9, 65, 257, 2039, 2040, 2041, 2049, 4353, 16383, 16384, 16385)] == \
        [1, 1, 2, 9, 33, 255, 255, 256, 257, 545, 2048, 2048, 2048]
    assert [narrow[N]['two_level'] for N in (2040, 2041)] == [False, True]
    assert [narrow[N]['stages_hi'] for N in (16384, 16385, 32767, 32769, 49153)] == [1, 2, 2, 3, 4]
    assert [gr.plan(1, P)['nit'] for P in (1, 128, 129, 256, 257, 512, 513, 1024)] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert [gr.route(P) for P in (1024, 1025, 4096, 4097)] == ['narrow', 'wide1', 'wide1', 'wide2']
    assert gr.route(1026, two_pass=True) == 'wide2' and gr.route(1024, two_pass=True) == 'narrow'
    assert [gr.wide1_shape(P) for P in (1026, 1536, 1538, 2048, 2050, 3072, 3074, 4096)] == \
        [(2, 6), (2, 6), (2, 8), (2, 8), (4, 6), (4, 6), (4, 8), (4, 8)]
    assert {gr.wide1_shape(P) for P in gr.WIDE1_MULTI_P} == {(2, 6), (2, 8), (4, 6), (4, 8)}
    assert [gr.wide1_slot_ceiling(P) for P in (1026, 2050)] == [4096, 2048]
    assert [gr.wide1_multi_N(P) for P in (1026, 4096)] == [[16385, 16386], [8193, 8194]]
    for P in gr.WIDE1_MULTI_P:                                     # at least three stages at EVERY possible grid
        for N in gr.wide1_multi_N(P):
            pl = gr.plan(N, P)
            assert pl['stages_lo'] >= 3 and pl['grid_hi'] * 2 * pl['stages_lo'] > N + 1
    w2 = gr.plan(16389, 1026, two_pass=True)
    assert (w2['grid_hi'], w2['stages_hi'], w2['nblk_hi']) == (4096, 2, 9)
    assert [gr.plan(N, 4097)['nblk_hi'] for N in gr.WIDE2_N] == [1, 1, 1, 1, 2, 3]
    # the rounding counts at one case of each route
    pl = gr.plan(49153, 130)
    assert gr.k_z(pl) == 2 + 2 + 6 and gr.reducer_roundings(2048) == 16 + (16 // 4 + 3 + 2 + 7)
    assert gr.k_acc(pl) == 1 + 1 + 2 * 4 + 3 + gr.reducer_roundings(2048) + 2
    assert gr.k_val(pl) == 1 + 4 + 2 + 3 + (4 + 9) + 2
    pl = gr.plan(2049, 4096)
    assert gr.k_z(pl) == 2 + 8 + 6 + 3 and pl['grid_lo'] == 256 and pl['grid_hi'] == 1025 and pl['stages_hi'] == 5
    assert gr.k_acc(pl) == 1 + 1 + 10 + 0 + gr.reducer_roundings(1025) + 2
    pl = gr.plan(2049, 4225)
    assert gr.k_z(pl) == 2 + 34 + 6 and gr.k_acc(pl) == 1 + 1 + 512 + 3 + gr.reducer_roundings(2) + 2


def _check_mutations_int(case, pl, ie):
    ref, mu = gr.mutations(case, pl, ie)
    for name, (v, g) in mu.items():
        assert v != ref['value'] or not np.array_equal(g, ref['grad']), 'integer case blind to: ' + name
    return set(mu)


@pytest.mark.parametrize('N,P,two_pass,off', gr.int_shapes())
def test_integer_oracle(N, P, two_pass, off):
    pl = gr.plan(N, P, two_pass)
    for setting in gr.int_settings_at(N, P):
        assert gr.partial_sum_ceiling(setting, N, P) < 2.0 ** 53
        case = gr.make_case(setting, 'int', N, P, off)
        ie = gr.int_evaluate(case)
        other = gr.evaluate(case, gr.LD if N * P <= LD_ENTRIES else np.float64)
        for k in ('grad', 'hvp', 'lp', 'cw'):
            assert 4.0 * np.max(np.abs(ie[k])) < 2.0 ** 53
            # (longdouble keeps exp(-800): the two coincide once that is a float64, as every device quantity is)
            assert np.array_equal(other[k].astype(np.float64), ie[k]), (setting, k)
        if ie['value'] is not None:
            assert float(other['value']) == ie['value'], setting
        else:                                                      # logistic at beta = 0: w log 2 rounds; the value keeps the bound
            b = gr.bounds(case, pl)
            assert gr.max_ratio(gr.evaluate(case, np.float64)['value'], gr.evaluate(case, gr.LD)['value'], b['value']) <= 1.0
        assert np.all(case['w'] != 0) and np.all(case['X'][:, 0] == 1)
        if setting == 'gaussian':
            _check_mutations_int(case, pl, ie)


@pytest.mark.parametrize('N,P,two_pass,off', gr.real_shapes())
def test_real_oracle(N, P, two_pass, off):
    pl = gr.plan(N, P, two_pass)
    for loss in gr.LOSSES:
        case = gr.make_case(loss, 'real', N, P, off)
        ref, f64, b = gr.evaluate(case, gr.LD), gr.evaluate(case, np.float64), gr.bounds(case, pl)
        assert float(np.max(np.abs(ref['z']))) <= gr.Z_MAX
        assert np.all(case['w'] != 0) and np.all(case['X'][:, 0] == 1)
        for k in ('value', 'grad', 'hvp'):
            assert gr.max_ratio(f64[k], ref[k], b[k]) <= 1.0, (loss, k)
        for (n0, n1) in gr.obs_windows(pl, off + P):
            got = gr.obs_rows(case, f64['lp'], n0, n1, np.float64)
            assert gr.max_ratio(got, gr.obs_rows(case, ref['lp'], n0, n1, gr.LD), gr.obs_rows_bound(b, n0, n1)) <= 1.0
        base, mu = gr.mutations(case, pl, ref)
        for name, (v, g) in mu.items():
            r = max(gr.max_ratio(v, base['value'], b['value']), gr.max_ratio(g, base['grad'], b['grad']))
            assert r >= SHARP, '{}: too forgiving of "{}": ratio {:.3g}'.format(loss, name, r)


@pytest.mark.parametrize('N,P,two_pass', [(2049, 130, False), (16391, 130, False), (1001, 2050, False), (2049, 4098, False),
                                          (4097, 1026, True)])
def test_every_mutation_applies_on_every_route(N, P, two_pass):
    """At one multi-block shape of each route all eight mistakes are formed, on integers and on real data."""
    pl = gr.plan(N, P, two_pass)
    ci = gr.make_case('gaussian', 'int', N, P)
    assert _check_mutations_int(ci, pl, gr.int_evaluate(ci)) == set(gr.MUTATIONS)
    cr = gr.make_case(gr.POISSON, 'real', N, P)
    assert set(gr.mutations(cr, pl, gr.evaluate(cr, gr.LD))[1]) == set(gr.MUTATIONS)


@pytest.mark.parametrize('loss', gr.LOSSES)
def test_norm_wise_comparison_is_blind_to_a_small_column(loss):
    """The gap: one row's term missing from the gradient entry of the smallest column of X passes rel_err at 1e-10 (the
    tightest tolerance of the earlier tests) and leaves the entry-wise bound by more than 100 x."""
    N, P = 2049, 130
    case = gr.make_case(loss, 'real', N, P)
    ref, b = gr.evaluate(case, gr.LD), gr.bounds(case, gr.plan(N, P))
    g, j = gr.small_column_mutation(case, ref, limit=1e-11 * float(np.max(np.abs(ref['grad']))))
    assert g[j] != ref['grad'][j]
    assert rel_err(g.astype(np.float64), ref['grad'].astype(np.float64)) < 1e-10
    assert gr.max_ratio(g, ref['grad'], b['grad']) >= SHARP


def test_zero_weight_rows_are_deleted_rows():
    """What the GPU file asks of the device holds for the references."""
    N, P = gr.ZERO_WEIGHTS
    keep = np.arange(N) % 2 == 0
    for setting in gr.INT_SETTINGS:
        c = gr.make_case(setting, 'int', N, P)
        cz = dict(c, w=np.where(keep, c['w'], 0.0))
        cd = dict(c, X=c['X'][keep], y=c['y'][keep], w=c['w'][keep])
        ez, ed = gr.int_evaluate(cz), gr.int_evaluate(cd)
        assert ez['value'] == ed['value'] and np.array_equal(ez['grad'], ed['grad']) and np.array_equal(ez['hvp'], ed['hvp'])


def test_loss_roundings_cover_a_perturbed_evaluation():
    """The per-loss error terms are upper bounds: moving z by Ez units and e^z, log1p by E ulp, then rounding every operation
    (a float64 evaluation of a longdouble-perturbed input) stays inside L + D Ez."""
    rng = np.random.default_rng(5)
    z = rng.uniform(-30, 30, size=4000)
    for loss in gr.LOSSES:
        y = rng.integers(0, 2, size=z.size).astype(np.float64) if loss != gr.GAUSSIAN else rng.normal(size=z.size)
        Ez = 51.0 * np.abs(z)                                     # (forming zh rounds once more)
        zh = z * (1.0 + 50.0 * gr.U_ROUND * rng.choice([-1.0, 1.0], size=z.size))
        ref = gr.loss_terms(loss, y.astype(gr.LD), z.astype(gr.LD))
        got = gr.loss_terms(loss, y, zh)
        L0, L1, L2, D1, D2 = gr.loss_roundings(loss, y, z)
        lim = (L0 + np.abs(np.asarray(ref[1], dtype=np.float64)) * Ez, L1 + D1 * Ez, L2 + D2 * Ez)
        for k in range(2):                                         # (l'' of the reference formula differs from the device's: see loss_terms)
            err = np.abs(got[k].astype(gr.LD) - ref[k])
            assert np.all(err <= gr.U_ROUND * gr.SECOND_ORDER * lim[k] + 0), (loss, k)

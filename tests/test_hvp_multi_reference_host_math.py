"""The oracles of tests/test_gpu_hvp_multi.py are fair and sharp, shown on the CPU before any GPU is involved
(tests/hvp_multi_reference.py): at every shape of the GPU file the integer reference is the longdouble
one, an honest float64 evaluation sits inside the derived bound, and each mistake a fused kernel can make -- a dropped tail
row, a neighbour's weight, two exchanged columns, a neighbour vector's result, the row past N counted -- breaks the exact
comparison and leaves the bound by at least 100 x."""
import numpy as np
import pytest

import hvp_multi_reference as hr

ALL_FULL = [(N, P, Q, 0) for (N, P, Q) in hr.FULL_CASES] + [(N, P, Q, hr.GLM_OFF) for (N, P, Q) in hr.GLM_OFF_CASES]
SHARP = 100.0


def test_launch_geometry():
    """The helpers reproduce the launcher: every NB from 1 to 8, eight waves at even NB, the chunk and grid counts at the
    sizes where workgroup 0 takes its second and third chunk."""
    assert sorted({hr.n_blocks(P) for P in hr.P_GRID}) == list(range(1, 9))
    assert [hr.padded_cols(P) for P in (2, 128, 130, 1022, 1024)] == [128, 128, 256, 1024, 1024]
    assert [hr.n_waves(P) for P in (2, 130, 258, 512, 640, 1024)] == [4, 8, 4, 8, 4, 8]
    assert hr.n_waves(1024, four_waves=True) == 4
    assert [hr.n_chunks(N) for N in (1, 7, 8, 9, 17)] == [1, 1, 1, 2, 3]
    assert [(hr.grid(N), hr.chunks_per_workgroup(N)) for N in (9, 2047, 2048, 2049, 4096, 4097, 6145)] == \
        [(2, 1), (256, 1), (256, 1), (256, 2), (256, 2), (256, 3), (256, 4)]
    assert hr.roundings_R(6145, 1024) == 1024 + 8 + 1 + 32 + 256 + 2 and hr.roundings_T(2) == 2 + 4 + 2
    assert len(hr.FULL_CASES) == len(set(hr.FULL_CASES))
    for P in hr.P_GRID:
        assert {(1, P, 16), (9, P, 16), (2049, P, 16)} <= set(hr.FULL_CASES)
    for N in hr.N_GRID:
        assert {(N, 2, 16), (N, 130, 16), (N, 1024, 16)} <= set(hr.FULL_CASES)
    for Q in hr.Q_GRID:
        assert {(2049, 130, Q), (2049, 512, Q)} <= set(hr.FULL_CASES)


@pytest.mark.parametrize('N,P,Q,off', ALL_FULL)
def test_full_form_oracles(N, P, Q, off):
    # exact: int64 == longdouble, entry by entry; every mutation changes at least one entry
    ci = hr.make_case('int', N, P, Q, off)
    want = hr.int_full(ci)
    assert np.max(np.abs(want)) < 2 ** 40
    assert np.array_equal(hr.ld_full(ci), want.astype(hr.LD))
    assert np.array_equal(hr.f64_full(ci), want.astype(np.float64))
    for name, m in hr.full_mutations(ci, want, hr.to_int).items():
        assert not np.array_equal(m, want), 'integer case blind to: ' + name
    # bounded: plain float64 inside, every mutation far outside
    cr = hr.make_case('real', N, P, Q, off)
    ref, A = hr.ld_full(cr), hr.abs_full(cr)
    for four in (False, True):
        bound = hr.bound_R(N, P, four) * A
        assert hr.max_ratio(hr.f64_full(cr), ref, bound) <= 1.0
    bound = hr.bound_R(N, P) * A                                # the larger of the two wave forms' bounds
    for name, m in hr.full_mutations(cr, ref, hr.to_ld).items():
        r = hr.max_ratio(m, ref, bound)
        assert r >= SHARP, 'real case too forgiving of "{}": ratio {:.3g}'.format(name, r)


@pytest.mark.parametrize('P', hr.ROWS_P)
@pytest.mark.parametrize('Q', hr.ROWS_Q)
def test_row_form_oracles(P, Q):
    X, s, Zt = hr.rows_case('int', P, Q)
    want = hr.int_rows(X, s, Zt)
    assert np.array_equal(hr.ld_rows(X, s, Zt), want.astype(hr.LD))
    assert np.array_equal(hr.f64_rows(X, s, Zt), want.astype(np.float64))
    assert np.all(s != 0)
    for name, m in hr.rows_mutations(X, s, Zt, want, hr.to_int).items():
        assert not np.array_equal(m, want), 'integer case blind to: ' + name
    X, s, Zt = hr.rows_case('real', P, Q)
    ref, A = hr.ld_rows(X, s, Zt), hr.abs_rows(X, s, Zt)
    assert np.all(s != 0)
    bound = hr.bound_T(P) * A
    assert hr.max_ratio(hr.f64_rows(X, s, Zt), ref, hr.bound_T(P, True) * A) <= 1.0
    for name, m in hr.rows_mutations(X, s, Zt, ref, hr.to_ld).items():
        r = hr.max_ratio(m, ref, bound)
        assert r >= SHARP, 'real case too forgiving of "{}": ratio {:.3g}'.format(name, r)


def test_zero_weight_rows_are_deleted_rows():
    """What the GPU file asks of the device holds for the references: zero weights on every second row give the result of
    deleting those rows."""
    c = hr.make_case('int', 2049, 130, 7)
    keep = np.arange(2049) % 2 == 0
    cz = dict(c, c=np.where(keep, c['c'], 0.0))
    cd = dict(c, X=c['X'][keep], c=c['c'][keep])
    assert np.array_equal(hr.int_full(cz), hr.int_full(cd))

"""Writes tests/golden/glmm_gamma_tail_exact.npz: the rows and the exact values of the row-by-row tail test of the Gamma policy
(tests/test_gpu_glmm_gamma_tails.py).  mpmath only; run from anywhere:
    python tests/golden/make_glmm_gamma_tail_exact.py

A row is (rho, s, log y, phi) in fp64; with A = (log y - rho) + s / 2 the exact values are, at 60 digits and FROM THOSE fp64 NUMBERS,
    g = phi exp(A),   a1 = phi - g,   value = g + phi rho
(the other four coefficients are g times 1/2, 1, -1/2, 1/4).  Targets of A: 0, +-1, +-30, +-100, +-500, +-700, each split three ways
into (log y, rho, s) -- rho in {-300, 0.37, 250}, s in {5e-324 (the entries refuse 0), 0.7, 40}, log y what is left, held inside
+-700 so that y itself is a finite double -- times phi in {1e-3, 0.05, 1, 7.5, 1e4, 1e8}.  Rows whose g leaves [1e-300, 1e306] are
dropped: past them the value overflows (the refusal is tested elsewhere) or g nears the subnormals and has no relative accuracy to pin.
The file holds rho, s, ly, phi, A and d = log y - rho (fp64 roundings of the exact numbers, for the bound), g, a1, value."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
TARGETS = (0.0, 1.0, -1.0, 30.0, -30.0, 100.0, -100.0, 500.0, -500.0, 700.0, -700.0)
SPLITS = ((-300.0, 5e-324), (0.37, 0.7), (250.0, 40.0))
PHIS = (1e-3, 0.05, 1.0, 7.5, 1e4, 1e8)


def rows():
    out = []
    for A in TARGETS:
        for rho, s in SPLITS:
            ly = float(np.clip(A + rho - 0.5 * s, -700.0, 700.0))
            for phi in PHIS:
                out.append((rho, s, ly, phi))
    return np.array(out)


def main():
    keep, cols = [], []
    for rho, s, ly, phi in rows():
        r, v, l, p = (mp.mpf(float(a)) for a in (rho, s, ly, phi))
        d = l - r
        A = d + v / 2
        g = p * mp.exp(A)
        if not (mp.mpf('1e-300') <= g <= mp.mpf('1e306')):
            continue
        keep.append((rho, s, ly, phi))
        cols.append([float(A), float(d), float(g), float(p - g), float(g + p * r)])
    keep, cols = np.array(keep), np.array(cols)
    assert keep.shape[0] % 64 != 0 and keep.shape[0] > 128               # more than two tiles, the last one partial
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'glmm_gamma_tail_exact.npz')
    np.savez(path, rho=keep[:, 0], s=keep[:, 1], ly=keep[:, 2], phi=keep[:, 3], A=cols[:, 0], d=cols[:, 1], g=cols[:, 2], a1=cols[:, 3],
             value=cols[:, 4])
    print(path, keep.shape[0], 'rows; |A| up to', float(np.max(np.abs(cols[:, 0]))), 'g from', float(cols[:, 2].min()), 'to', float(cols[:, 2].max()))


if __name__ == '__main__':
    main()

"""Writes tests/golden/glmm_ordinal_tail_exact.npz: the rows and the exact values of the row-by-row tail test of the ordinal policy
(tests/test_gpu_glmm_ordinal_tails.py).  mpmath only; run from anywhere:
    python tests/golden/make_glmm_ordinal_tail_exact.py

A row is (o, s, category) in fp64 next to ONE table of six thresholds; the test runs it as its own group with x = 0, so that rho_x = 0,
rho = o and the variance is s.  With the 20 Gauss-Hermite nodes x_k, weights w_k (numpy's fp64 values), lo = alpha_y, hi = alpha_{y+1}
(-inf / +inf on the two end categories) and D = hi - lo, everything below is formed at 60 digits FROM THOSE fp64 NUMBERS:
    a_k = sqrt(2 s) x_k - (hi - o),   b_k = (lo - o) - sqrt(2 s) x_k,   sp, sg, g2, g3, g4: softplus, sigma and its three derivatives,
    E_0 = sum w [sp(a) + sp(b)] - log(1 - e^-D),  E_1 = sum w [sg(a) - sg(b)],  E_2 = sum w [g2(a) + g2(b)],  E_3 = sum w [g3(a) - g3(b)],
    E_4 = sum w [g4(a) + g4(b)],
    T_0..3 = -sum w g2(a),  -sum w g3(a) / 2,  -sum w g2(b),  +sum w g3(b) / 2           (d1_hi, d2_hi, d1_lo, d2_lo of the threshold pass)
    T_4..8 = -sum w sg(a) - r,  sum w sg(b) + r,  sum w g2(a) + c,  sum w g2(b) + c,  -c,   r = 1 / expm1(D),  c = e^-D / expm1(-D)^2.
The table: alpha = cumsum(0, 1e-8, 1e-3, 1, 50, 800) in fp64, so that the five interior categories have D in {1e-8, 1e-3, 1, 50, 800}.
Targets: rho - hi (rows anchored at hi) and rho - lo (rows anchored at lo) over +-{0, 1e-9, 1, 38, 700}, every interior category
and both end categories, s in {1e-4, 1e-2} (the nodes then stay within +-0.08 and +-0.8 of the centre: in the tail).

Next to the exact values the file holds what the derived bound of the test is assembled from, per quantity Q = sum w f:
    node = sum w C_j M_j        the rounding of LogisticLik's node expressions, in units of u = 2^-53: counts C = (3, 5, 9, 16, 26) for
                                (sp, sg, g2, g3, g4) on the magnitudes M = (sp, sg, g2, g2, g2) (g3 = g2 (1 - e) / (1 + e) and
                                g4 = g2 (1 - 6 g2) carry ABSOLUTE errors of that size where their last factor cancels), at a and at b
    prop = sum w A_k |f'|       A_k = |anchor - o| + sqrt(2 s) |x_k| >= |argument|: what an error of 6 u A_k in forming the argument moves
                                (the fold, sqrt(s), sqrt(2) x_k, the product, the fused addition, the subtraction), f' the next derivative
    mag  = sum w |terms of f|   what the roundings of the sums and products act on
    closed = the closed-form part in D: |log term|, r, c                      (its own ulp counts are applied by the test)."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
DELTAS = (1e-8, 1e-3, 1.0, 50.0, 800.0)
ALPHA = np.cumsum(np.array((0.0,) + DELTAS))
TARGETS = (0.0, 1e-9, -1e-9, 1.0, -1.0, 38.0, -38.0, 700.0, -700.0)
VARS = (1e-4, 1e-2)
C_NODE = (3, 5, 9, 16, 26)
GX, GW = np.polynomial.hermite.hermgauss(20)
INF = float('inf')


def rows():
    out = []
    T = ALPHA.size
    for s in VARS:
        for cat in range(T + 1):
            anchors = ([ALPHA[cat]] if cat < T else []) + ([ALPHA[cat - 1]] if cat >= 1 else [])      # hi, lo where they are finite
            for anchor in anchors:
                for d in TARGETS:
                    out.append((anchor + d, s, float(cat)))
    return np.array(out)


def logistic(x):
    """[sp, sg, g2, g3, g4, g5] at x (sigma'''' last); exact zeros at -inf."""
    if x == -mp.inf:
        return [mp.mpf(0)] * 6
    sg = 1 / (1 + mp.exp(-x))
    v = sg * (1 - sg) if x < 30 else mp.exp(-x) / (1 + mp.exp(-x)) ** 2
    d = 1 - 2 * sg
    return [mp.log1p(mp.exp(-abs(x))) + max(x, 0), sg, v, v * d, v * (1 - 6 * v), v * d * (1 - 12 * v)]


def one(o, s, cat):
    cat = int(cat)
    o, s = mp.mpf(float(o)), mp.mpf(float(s))
    tab = [-mp.inf] + [mp.mpf(float(a)) for a in ALPHA] + [mp.inf]
    lo, hi = tab[cat], tab[cat + 1]
    interior = lo != -mp.inf and hi != mp.inf
    n = 14
    ex, node, prop, mag = ([mp.mpf(0)] * n for _ in range(4))
    ex, node, prop, mag = list(ex), list(node), list(prop), list(mag)
    for xk, wk in zip(GX, GW):
        tk = mp.sqrt(2 * s) * mp.mpf(float(xk))
        wq = mp.mpf(float(wk)) / mp.sqrt(mp.pi)
        a = tk - (hi - o) if hi != mp.inf else -mp.inf
        b = (lo - o) - tk if lo != -mp.inf else -mp.inf
        Aa = abs(hi - o) + abs(tk) if hi != mp.inf else mp.mpf(0)
        Ab = abs(lo - o) + abs(tk) if lo != -mp.inf else mp.mpf(0)
        fa, fb = logistic(a), logistic(b)
        Ma, Mb = [fa[0], fa[1], fa[2], fa[2], fa[2]], [fb[0], fb[1], fb[2], fb[2], fb[2]]
        for j in range(5):
            sign = -1 if j & 1 else 1
            ex[j] += wq * (fa[j] + sign * fb[j])
            node[j] += wq * C_NODE[j] * (Ma[j] + Mb[j])
            prop[j] += wq * (Aa * abs(fa[j + 1]) + Ab * abs(fb[j + 1]))
            mag[j] += wq * (abs(fa[j]) + abs(fb[j]))
        # the threshold pass: (index, coefficient, which side, derivative order)
        for i, (coef, f, M, A, j) in enumerate(((-1, fa, Ma, Aa, 2), (-mp.mpf(1) / 2, fa, Ma, Aa, 3), (-1, fb, Mb, Ab, 2), (mp.mpf(1) / 2, fb, Mb, Ab, 3),
                                               (-1, fa, Ma, Aa, 1), (1, fb, Mb, Ab, 1), (1, fa, Ma, Aa, 2), (1, fb, Mb, Ab, 2))):
            ex[5 + i] += wq * coef * f[j]
            node[5 + i] += wq * abs(coef) * C_NODE[j] * M[j]
            prop[5 + i] += wq * abs(coef) * A * abs(f[j + 1])
            mag[5 + i] += wq * abs(coef) * abs(f[j])
    closed = [mp.mpf(0)] * n
    if interior:
        D = hi - lo
        lt, r, c = -mp.log(-mp.expm1(-D)), 1 / mp.expm1(D), mp.exp(-D) / mp.expm1(-D) ** 2
        ex[0] += lt
        ex[9] -= r
        ex[10] += r
        ex[11] += c
        ex[12] += c
        ex[13] = -c
        closed[0], closed[9], closed[10], closed[11], closed[12], closed[13] = abs(lt), r, r, c, c, c
    return ex, node, prop, mag, closed


def main():
    R = rows()
    cols = [[], [], [], [], []]
    for row in R:
        for c, v in zip(cols, one(*row)):
            c.append([float(x) for x in v])
    ex, node, prop, mag, closed = (np.array(c) for c in cols)
    N = R.shape[0]
    assert N % 64 != 0 and N > 128                                       # more than two tiles, the last one partial
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'glmm_ordinal_tail_exact.npz')
    np.savez(path, o=R[:, 0], s=R[:, 1], cat=R[:, 2], alpha=ALPHA, exact=ex, node=node, prop=prop, mag=mag, closed=closed)
    print(path, N, 'rows;', 'categories', np.bincount(R[:, 2].astype(int)), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

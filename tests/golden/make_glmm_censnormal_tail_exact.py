"""Writes tests/golden/glmm_censnormal_tail_exact.npz: the rows and the exact values of the row-by-row tail test of the censored
Gaussian policies (tests/test_gpu_glmm_censnormal_tails.py).  mpmath only; run from anywhere:
    python tests/golden/make_glmm_censnormal_tail_exact.py

A row is (o, y, s, phi, delta) in fp64; the test runs it as its own group with x = 0, so that rho = o and the variance is s.  With
r = sqrt(phi), u = o - y and the 20 Gauss-Hermite nodes x_k, weights w_k (numpy's fp64 values), everything below is formed at 60 digits
FROM THOSE fp64 NUMBERS:
    censored   a_k = delta r (u + sqrt(2 s) x_k),   E_j = (delta r)^j sum_k w_k / sqrt(pi) H^(j)(a_k),  j = 0..4,  H = -log Phi,
               D1 = (delta r / 2) sum w (a H'' + H'),  D2 = (phi / 2) sum w (a H''' + 2 H''),  L1 = sum w a H' / 2,  L2 = sum w a (a H'' + H') / 4
    observed   E = [phi (u^2 + s) / 2, phi u, phi, 0, 0],  D1 = phi u,  D2 = phi,  L1 = L2 = E_0.
Targets: the argument at the centre a_0 = delta r u in +-{0, 1, 5, 5.01, 38, 700} (5 and 5.01 lie either side of the continued-fraction
threshold of the probit h1, 38 either side of where erfcx overflows, 700 deep in both tails) x phi in {1e-6, 1, 1e8} x phi s in
{1e-4, 1e-2} (the nodes then stay within +-0.08 and +-0.8 of a_0: in the tail) x delta in {+1, -1}; observed rows at r u in
{0, +-1, +-38, +-700} x the three phi.

Next to the exact values the file holds what the derived bound of the test is assembled from, per quantity Q = pref sum w f(a_k):
    tail = |pref| sum w B(a_k)         B: the pinned error of h1^(j) at a (value 1e-10 relative; orders 1 to 4
                                       7.1e-15, 2.2e-14, 1.4e-13, 8.0e-11 of max(1, |H^(j)|)), plus, below a = -40 where section 42 has no
                                       rows, the rounding model of the left tail: 16 ulp, 16 |a| ulp, 16 a^2 ulp at orders 2, 3, 4
    prop = |pref| sum w A_k |d f / d a|    A_k = r (|u| + sqrt(2 s) |x_k|) >= |a_k|: what an error of 4 ulp A_k in forming a_k moves
    mag  = |pref| sum w |terms of f|       what the roundings of the sums and products act on."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
A0 = (0.0, 1.0, 5.0, 5.01, 38.0, 700.0)
PHIS = (1e-6, 1.0, 1e8)
PHI_S = (1e-4, 1e-2)
OBS = (0.0, 1.0, -1.0, 38.0, -38.0, 700.0, -700.0)
Y = 0.37
E42 = (1e-10, 7.1e-15, 2.2e-14, 1.4e-13, 8.0e-11)
U = mp.mpf(2) ** -53
GX, GW = np.polynomial.hermite.hermgauss(20)


def rows():
    out = []
    for ps in PHI_S:
        for phi in PHIS:
            r = np.sqrt(phi)
            for a0 in A0:
                for sign in ((1.0,) if a0 == 0.0 else (1.0, -1.0)):
                    for delta in (1.0, -1.0):
                        out.append((Y + sign * a0 / (delta * r), Y, ps / phi, phi, delta))
                if a0 == 0.0:                                            # keep the count of rows per (phi, phi s) even: a second centre next to 0
                    for delta in (1.0, -1.0):
                        out.append((Y + 1e-9 / (delta * r), Y, ps / phi, phi, delta))
    for phi in PHIS:
        for ru in OBS:
            out.append((Y + ru / np.sqrt(phi), Y, 1e-2 / phi, phi, 0.0))
    return np.array(out)


def H_all(a):
    """[H, H', .., H^(5)] at a: the inverse-Mills recurrences at 60 digits (the cancellations of the left tail cost 12 digits at
    a = -700), the fifth derivative by differentiating the recurrence once more."""
    l = mp.npdf(a) / mp.ncdf(a)
    d = a + l
    w = l * d
    l1 = -w                                                             # lambda' = -lambda (a + lambda)
    d1 = 1 + l1
    w1 = l1 * d + l * d1
    l2 = -w1
    d2 = l2
    w2 = l2 * d + 2 * l1 * d1 + l * d2
    l3 = -w2
    d3 = l3
    w3 = l3 * d + 3 * l2 * d1 + 3 * l1 * d2 + l * d3
    H0 = -mp.log(mp.ncdf(a)) if a < 0 else -mp.log1p(-mp.ncdf(-a))
    return [H0, -l, w, w1, w2, w3]


def B_all(a, H):
    tail = [0, 0, 16 * U, 16 * abs(a) * U, 16 * a * a * U] if a < -40 else [0] * 5
    return [E42[0] * abs(H[0])] + [E42[j] * max(1, abs(H[j])) + tail[j] for j in range(1, 5)]


def one(o, y, s, phi, delta):
    o, y, s, phi = (mp.mpf(float(v)) for v in (o, y, s, phi))
    u = o - y
    if delta == 0.0:
        e0 = phi * (u * u + s) / 2
        ex = [e0, phi * u, phi, 0, 0, phi * u, phi, e0, e0]
        return ex, [0] * 9, [0] * 9, [abs(v) for v in ex]
    r = mp.sqrt(phi)
    dr = int(delta) * r
    names = 9
    ex, tail, prop, mag = ([mp.mpf(0)] * names for _ in range(4))
    ex, tail, prop, mag = list(ex), list(tail), list(prop), list(mag)
    pref = [1, dr, phi, dr * phi, phi * phi, dr / 2, phi / 2, mp.mpf(1) / 2, mp.mpf(1) / 4]
    for xk, wk in zip(GX, GW):
        tu = u + mp.sqrt(2 * s) * mp.mpf(float(xk))
        wq = mp.mpf(float(wk)) / mp.sqrt(mp.pi)
        a = dr * tu
        Ak = r * (abs(u) + mp.sqrt(2 * s) * abs(mp.mpf(float(xk))))
        H = H_all(a)
        B = B_all(a, H)
        aa = abs(a)
        f = [H[0], H[1], H[2], H[3], H[4], a * H[2] + H[1], a * H[3] + 2 * H[2], a * H[1], a * (a * H[2] + H[1])]
        tl = [B[0], B[1], B[2], B[3], B[4], aa * B[2] + B[1], aa * B[3] + 2 * B[2], aa * B[1], a * a * B[2] + aa * B[1]]
        pr = [abs(H[1]), abs(H[2]), abs(H[3]), abs(H[4]), abs(H[5]), 2 * abs(H[2]) + aa * abs(H[3]), 3 * abs(H[3]) + aa * abs(H[4]),
              abs(H[1]) + aa * abs(H[2]), 3 * aa * abs(H[2]) + a * a * abs(H[3]) + abs(H[1])]
        mg = [abs(H[0]), abs(H[1]), abs(H[2]), abs(H[3]), abs(H[4]), aa * abs(H[2]) + abs(H[1]), aa * abs(H[3]) + 2 * abs(H[2]), aa * abs(H[1]),
              a * a * abs(H[2]) + aa * abs(H[1])]
        for i in range(names):
            ex[i] += wq * pref[i] * f[i]
            tail[i] += wq * abs(pref[i]) * tl[i]
            prop[i] += wq * abs(pref[i]) * Ak * pr[i]
            mag[i] += wq * abs(pref[i]) * mg[i]
    return ex, tail, prop, mag


def main():
    R = rows()
    cols = [[], [], [], []]
    for row in R:
        for c, v in zip(cols, one(*row)):
            c.append([float(x) for x in v])
    ex, tail, prop, mag = (np.array(c) for c in cols)
    N = R.shape[0]
    assert N % 64 != 0 and N > 128                                       # more than two tiles, the last one partial
    a0 = R[:, 4] * np.sqrt(R[:, 3]) * (R[:, 0] - R[:, 1])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'glmm_censnormal_tail_exact.npz')
    np.savez(path, o=R[:, 0], y=R[:, 1], s=R[:, 2], phi=R[:, 3], delta=R[:, 4], a0=a0, exact=ex, tail=tail, prop=prop, mag=mag)
    print(path, N, 'rows;', int(np.sum(R[:, 4] == 1)), 'right-censored,', int(np.sum(R[:, 4] == -1)), 'left-censored,', int(np.sum(R[:, 4] == 0)),
          'observed; |a_0| up to', float(np.max(np.abs(a0))))


if __name__ == '__main__':
    main()

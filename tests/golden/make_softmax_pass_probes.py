"""Writes tests/golden/softmax_pass_probes.npz: every row of the small real cases `GOLDEN_CASES` of
tests/softmax_pass_reference.py (ordinary rows, the probe rows and every extreme kind) in mpmath at 60 digits, from the inputs
as exact float64, straight from the definitions with no shift:

    z_a = x . beta_a,  S = 1 + sum_a e^{z_a},  p_a = e^{z_a} / S,  term = w (log S - z_y),  r_a = w (p_a - [y = a + 1]),
    t_a = x . V_a,     u_a = w p_a (t_a - sum_b p_b t_b)

Per case "N_P_K" the file holds N_P_K/{p, vterm, r, u}_hi and _lo: the value rounded to float64 and the remainder rounded to
float64 (about 106 bits together), which is what shows the longdouble reference good to well under the bounds of DESIGN.md
section 44.  mpmath only; run from anywhere:  python tests/golden/make_softmax_pass_probes.py"""
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import softmax_pass_reference as sp                                      # noqa: E402

mp.mp.dps = 60


def mpf(x):
    return mp.mpf(float(x))


def row_exact(x, w, y, beta, V):
    Km = beta.shape[0]
    z = [mp.fsum(mpf(a) * mpf(b) for a, b in zip(x, beta[a_])) for a_ in range(Km)]
    t = [mp.fsum(mpf(a) * mpf(b) for a, b in zip(x, V[a_])) for a_ in range(Km)]
    S = 1 + mp.fsum(mp.exp(v) for v in z)
    p = [mp.exp(v) / S for v in z]
    zy = z[y - 1] if y > 0 else mp.mpf(0)
    term = mpf(w) * (mp.log(S) - zy)
    r = [mpf(w) * (p[a] - (1 if y == a + 1 else 0)) for a in range(Km)]
    pt = mp.fsum(p[a] * t[a] for a in range(Km))
    u = [mpf(w) * p[a] * (t[a] - pt) for a in range(Km)]
    return p, term, r, u


def split(vals):
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(float(h))) for v, h in zip(vals, hi)])
    return hi, lo


def save(path, arrays):
    """An .npz with fixed time stamps and a fixed member order: two runs give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[k]), allow_pickle=False)


def main():
    out = {}
    for (N, P, K) in sp.GOLDEN_CASES:
        c = sp.real_case(N, P, K)
        Km = K - 1
        rows = [row_exact(c['X'][n], c['w'][n], int(c['y'][n]), c['beta'], c['V']) for n in range(N)]
        name = '{}_{}_{}'.format(N, P, K)
        for key, vals, shape in (('p', [v for r in rows for v in r[0]], (N, Km)), ('vterm', [r[1] for r in rows], (N,)),
                                 ('r', [v for r in rows for v in r[2]], (N, Km)), ('u', [v for r in rows for v in r[3]], (N, Km))):
            hi, lo = split(vals)
            out[name + '/' + key + '_hi'], out[name + '/' + key + '_lo'] = hi.reshape(shape), lo.reshape(shape)
    save(sp.GOLDEN, out)


if __name__ == '__main__':
    main()

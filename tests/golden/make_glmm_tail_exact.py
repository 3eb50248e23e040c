"""Writes tests/golden/glmm_tail_exact.npz: the exact values of the row-by-row tail tests (tests/glmm_tail_cases.py, DESIGN.md
section 42).  mpmath only; run from anywhere:  python tests/golden/make_glmm_tail_exact.py [--jobs J] [family ..]
(the result does not depend on J: the rows are independent)

Every node term is the derivative of the UNSHIFTED, UNFACTORED definition: numerical differentiation `mpmath.diffs` (what
`mpmath.taylor` calls -- taylor itself chops a term below the working epsilon to an exact 0, which is how -log Phi(20) "evaluates
to 0") or, for the Beta family, the plain chain rule on mpmath's own polygamma.  Digits: 60, plus 0.45 per unit of the farthest
|t| for the Beta family, whose plain chain rule cancels log10(1 / mu) digits.  The probit upper tail goes through
-log1p(-ncdf(-t)), the cloglog and truncated families through log1p(-exp(-u)).  Node terms below 1e-9000 (cloglog and truncated
Poisson at t > 10, u > 22026) are taken as 0: they are 0 in fp64 at any weight.  No exact value that is non-zero in mpmath and
above 1e-300 may come out as 0.0.

Per family F the file holds F/kind, F/rho, F/s, F/y, F/trials, F/phi (the rows), F/deg, F/exact (5 x n; 4 x n for the two dispersion families), F/mean (the exact
response mean per trial, NaN where the policy has none of its own or it overflows), F/mag (5 x n), and the HOST function's own figures F/host_rel, F/host_abs
(5 x n each) with the mask F/resolvable (5 x n)."""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import glmm_tail_cases as tc                                             # noqa: E402

DPS = 60


def mpf(x):
    return mp.mpf(float(x))


def _d(fn, t):
    return list(mp.diffs(fn, t, 4))


def softplus_derivs(t):
    return _d(lambda x: mp.log1p(mp.exp(x)), t)


def probit_h1_derivs(t):
    """-log Phi and its derivatives at t."""
    if t < 0:
        return _d(lambda x: -mp.log(mp.ncdf(x)), t)
    return _d(lambda x: -mp.log1p(-mp.ncdf(-x)), t)


def cloglog_h1_derivs(t):
    """-log(1 - exp(-e^t)) and its derivatives at t."""
    if t > 10:
        return [mp.mpf(0)] * 5
    if t < 0:
        return _d(lambda x: -mp.log(-mp.expm1(-mp.exp(x))), t)
    return _d(lambda x: -mp.log1p(-mp.exp(-mp.exp(x))), t)


def ztnb_g_derivs(t, phi):
    """log(1 - (1 + e^eta)^-phi) and its derivatives at eta = t."""
    if phi * mp.log1p(mp.exp(t)) < 1:
        return _d(lambda x: mp.log(-mp.expm1(-phi * mp.log1p(mp.exp(x)))), t)
    return _d(lambda x: mp.log1p(-mp.exp(-phi * mp.log1p(mp.exp(x)))), t)


def beta_derivs(t, phi, l):
    """The plain chain rule on the unshifted h with mpmath's polygamma (tests/test_glmm_beta_host_math.py::_mp_derivs)."""
    mu, nu = 1 / (1 + mp.exp(-t)), 1 / (1 + mp.exp(t))
    v = mu * nu
    d = nu - mu
    m1, m2, m3, m4 = v, v * d, v * (1 - 6 * v), v * d * (1 - 12 * v)
    a, b = phi * mu, phi * nu
    F = [None] + [phi ** j * (mp.polygamma(j - 1, a) + (-1) ** j * mp.polygamma(j - 1, b)) for j in (1, 2, 3, 4)]
    F[1] -= phi * l
    return [mp.loggamma(a) + mp.loggamma(b) - phi * l * mu,
            F[1] * m1,
            F[2] * m1 ** 2 + F[1] * m2,
            F[3] * m1 ** 3 + 3 * F[2] * m1 * m2 + F[1] * m3,
            F[4] * m1 ** 4 + 6 * F[3] * m1 ** 2 * m2 + F[2] * (3 * m2 ** 2 + 4 * m1 * m3) + F[1] * m4]


def beta_disp_terms(t, phi, l):
    """[h_l, d_t h_l, d_t^2 h_l, h_ll] of the unshifted Beta h by the plain chain rule (tests/test_glmm_dispersion_host_math.py)."""
    mu, nu = 1 / (1 + mp.exp(-t)), 1 / (1 + mp.exp(t))
    v, d = mu * nu, nu - mu
    a, b = phi * mu, phi * nu
    pa, pb = [mp.polygamma(j, a) for j in range(3)], [mp.polygamma(j, b) for j in range(3)]
    first = a * pa[0] + b * pb[0] - l * a
    K1 = phi * (pa[0] + a * pa[1] - pb[0] - b * pb[1] - l)
    K2 = phi ** 2 * (2 * pa[1] + a * pa[2] + 2 * pb[1] + b * pb[2])
    return [first, K1 * v, K2 * v ** 2 + K1 * v * d, first + a ** 2 * pa[1] + b ** 2 * pb[1]]


def negbin_disp_terms(eta, phi, y):
    """The same four of the NB2 term at eta = t - log phi (tests/test_glmm_dispersion_host_math.py::_mp_negbin)."""
    sg = 1 / (1 + mp.exp(-eta))
    sp = mp.log1p(mp.exp(eta)) if eta < 0 else eta + mp.log1p(mp.exp(-eta))
    g2 = sg * (1 - sg)
    g3 = g2 * (1 - 2 * sg)
    m = y + phi
    return [phi * sp - m * sg + y, phi * sg - m * g2, phi * g2 - m * g3, phi * sp - 2 * phi * sg + m * g2]


def disp_scales(family, t, phi, c):
    """The size of the terms that the device formula ADDS at a node, per quantity (tests/test_glmm_dispersion_host_math.py, "Measure"):
    these four are differences of such terms formed behind the node sums, and a sum of fp64 terms cannot be better than eps times the
    largest.  The `mag` of the two dispersion families."""
    if family == 'beta_disp':
        mu, nu = 1 / (1 + mp.exp(-t)), 1 / (1 + mp.exp(t))
        v = mu * nu
        a, b = phi * mu, phi * nu
        p0a, p0b = abs(mp.polygamma(0, 1 + a)), abs(mp.polygamma(0, 1 + b))
        p1a, p1b = mp.polygamma(1, 1 + a), mp.polygamma(1, 1 + b)
        p2a, p2b = abs(mp.polygamma(2, 1 + a)), abs(mp.polygamma(2, 1 + b))
        first = a * p0a + b * p0b + abs(c) * a
        k1 = phi * v * (p0a + a * p1a + p0b + b * p1b + abs(c))
        return [first + 2, k1, phi * phi * v * v * (2 * p1a + a * p2a + 2 * p1b + b * p2b) + abs(nu - mu) * k1,
                first + a * a * p1a + b * b * p1b]
    sg = 1 / (1 + mp.exp(-t))
    sp = mp.log1p(mp.exp(t)) if t < 0 else t + mp.log1p(mp.exp(-t))
    g2 = sg * (1 - sg)
    g3 = abs(g2 * (1 - 2 * sg))
    m = c + phi
    return [phi * sp + m * sg + c, phi * sg + m * g2, phi * g2 + m * g3, phi * sp + 2 * phi * sg + m * g2]


def disp_def(family, c):
    """The definition as a function of (t, lambda) at phi0 = 1, for the independent route of the CPU test (mp.diff in both)."""
    if family == 'beta_disp':
        return lambda t, lam: (mp.loggamma(mp.exp(lam) / (1 + mp.exp(-t))) + mp.loggamma(mp.exp(lam) / (1 + mp.exp(t)))
                               - mp.exp(lam) * c / (1 + mp.exp(-t)))
    return lambda t, lam: (c + mp.exp(lam)) * mp.log1p(mp.exp(t - lam)) - c * (t - lam)


def beta_h(phi, l):
    """The unshifted definition itself, for the independent route of the CPU test."""
    return lambda t: mp.loggamma(phi / (1 + mp.exp(-t))) + mp.loggamma(phi / (1 + mp.exp(t))) - phi * l / (1 + mp.exp(-t))


def nodes(rho, s):
    """[(t_k, w_k)] of the 20-node rule in mpmath; s = 0: every node sits at rho and the weights sum to 1."""
    if s == 0.0:
        return [(mpf(rho), mp.mpf(1))]
    gx, gw = tc.gh()
    sd = mp.sqrt(mpf(s)) * mp.sqrt(2)
    return [(mpf(rho) + sd * mpf(x), mpf(w) / mp.sqrt(mp.pi)) for x, w in zip(gx, gw)]


def row_exact(family, rho, s, y, trials, phi):
    """(exact (5 mpf), mean node part (mpf or None), mag (5 mpf)) of one row."""
    mp.mp.dps = DPS
    if family in ('beta', 'beta_disp'):
        far = abs(rho) + 5.4 * np.sqrt(2.0 * s)
        mp.mp.dps = DPS + int(0.45 * far)
    y_, m_, phi_ = mpf(y), mpf(trials), mpf(phi)
    closed = mp.exp(mpf(rho) + mpf(s) / 2)                               # E e^t
    if family == 'poisson':
        return [closed] * 5, None, [closed] * 5
    nq = 4 if family in tc.DISPERSION else 5
    acc, mag, mean = [mp.mpf(0)] * nq, [mp.mpf(0)] * nq, None
    for t, w in nodes(rho, s):
        if family in ('logistic', 'binomial', 'negbin'):
            term = [m_ * a for a in softplus_derivs(t)]
        elif family == 'probit':
            h1, h0 = probit_h1_derivs(t), probit_h1_derivs(-t)
            term = [y_ * a + (m_ - y_) * (-1) ** k * b for k, (a, b) in enumerate(zip(h1, h0))]
        elif family == 'cloglog':
            term = [y_ * a for a in cloglog_h1_derivs(t)]
            mean = (mean or 0) + w * -mp.expm1(-mp.exp(t))
        elif family == 'ztpoisson':
            term = [-a for a in cloglog_h1_derivs(t)]
            mean = (mean or closed) + w * term[1]
        elif family == 'beta_disp':
            term = beta_disp_terms(t, phi_, y_)
        elif family == 'negbin_disp':
            term = negbin_disp_terms(t, phi_, y_)
        elif family == 'ztnegbin':
            term = [(y_ + phi_) * a + b for a, b in zip(softplus_derivs(t), ztnb_g_derivs(t, phi_))]
            mean = (mean or phi_ * closed) + w * phi_ * mp.exp(t) / mp.expm1(phi_ * mp.log1p(mp.exp(t)))
        elif family == 'beta':
            term = beta_derivs(t, phi_, y_)
            mean = (mean or 0) + w / (1 + mp.exp(-t))
        else:
            raise ValueError(family)
        acc = [a + w * b for a, b in zip(acc, term)]
        size = disp_scales(family, t, phi_, y_) if family in tc.DISPERSION else [abs(b) for b in term]
        mag = [a + w * b for a, b in zip(mag, size)]
    if family == 'probit':
        mean = mp.ncdf(mpf(rho) / mp.sqrt(1 + mpf(s)))
    if family == 'cloglog':
        acc = [a + (m_ - y_) * closed for a in acc]
        mag = [a + (m_ - y_) * closed for a in mag]
    if family == 'ztpoisson':
        acc = [a + closed for a in acc]
        mag = [a + closed for a in mag]
    return acc, mean, mag


def _float(a):
    f = float(a)
    assert f != 0.0 or abs(a) < mp.mpf('1e-300'), 'an exact value that is not zero came out as 0.0: {}'.format(a)
    return f


def family_arrays(family, idx=None):
    """exact (5 x n), mean (n), mag (5 x n) of the rows idx (all) of a family."""
    r = tc.rows(family)
    idx = np.arange(r['rho'].size) if idx is None else np.asarray(idx)
    nq = 4 if family in tc.DISPERSION else 5
    exact, mean, mag = np.zeros((nq, idx.size)), np.full(idx.size, np.nan), np.zeros((nq, idx.size))
    for j, n in enumerate(idx):
        e, m, g = row_exact(family, r['rho'][n], r['s'][n], r['y'][n], r['trials'][n], r['phi'][n])
        exact[:, j], mag[:, j] = [_float(a) for a in e], [float(a) for a in g]
        if m is not None and m < mp.mpf('1e308'):
            mean[j] = float(m)
    return exact, mean, mag


def _chunk(job):
    return family_arrays(*job)


def _save(path, arrays):
    """An .npz with fixed time stamps and a fixed member order: two runs give the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[k]), allow_pickle=False)


def main(families, jobs=1):
    import multiprocessing
    out = {}
    if os.path.exists(tc.FIXTURE):
        with np.load(tc.FIXTURE) as z:
            out = {k: z[k] for k in z.files}
    for family in families:
        r = tc.rows(family)
        chunks = np.array_split(np.arange(r['rho'].size), max(1, min(4 * jobs, r['rho'].size)))
        with multiprocessing.Pool(jobs) as pool:
            parts = pool.map(_chunk, [(family, c) for c in chunks])
        exact, mean, mag = (np.concatenate([p[i] for p in parts], axis=-1) for i in range(3))
        rel, ab, res = tc.host_figures(family, r, exact, mag)
        out = {k: a for k, a in out.items() if not k.startswith(family + '/')}
        for k, a in r.items():
            out[family + '/' + k] = a
        for k, a in (('deg', np.array(tc.DEG)), ('exact', exact), ('mean', mean), ('mag', mag), ('host_rel', rel), ('host_abs', ab),
                     ('resolvable', res)):
            out[family + '/' + k] = a
        print(family, 'rows', r['rho'].size, 'host pointwise where resolvable', np.where(res, rel, 0.0).max(-1), 'host absolute',
              ab.max(-1), 'share resolvable', res.mean(-1), flush=True)
    _save(tc.FIXTURE, out)


if __name__ == '__main__':
    args = sys.argv[1:]
    jobs = int(args.pop(args.index('--jobs') + 1)) if '--jobs' in args else 1
    args = [a for a in args if a != '--jobs']
    main(args or tc.FAMILIES, jobs)

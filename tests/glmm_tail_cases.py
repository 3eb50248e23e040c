"""Rows, host figures and readers of the row-by-row tail tests of the mixed-model likelihoods: shared by the
generator tests/golden/make_glmm_tail_exact.py, the CPU test tests/test_glmm_tail_exact_host_math.py and the GPU test
tests/test_gpu_glmm_tails.py.  Not a conftest: it is imported by name.

One row per group.  A data set has G = N groups of one row, K = 1, z = 1, P = 1, x = 0 and mean = 0, so that row n has
rho_n = offset_n + e[n] and s_n = r[n] EXACTLY, and the K = 1 group sums of a `*_terms` entry are the row's own five coefficients
[a1, a2, c11, c12, c22] = w [E H' (- y), E H'' / 2, E H'', E H''' / 2, E H'''' / 4] (include/lrvb_hip.h, lrvb_glmm_slopes_terms: "at
K = 1 with z = 1 these are the columns of lrvb_glmm_terms in its order").

Rows of a family (`rows`): kind 0 the family's existing CPU grid, kind 1 its extension to rho in RHO_EXT x s in S_EXT, kind 2 the
threshold rows (s = S_MIN, which stands for 0: every node sits at rho) either side of every branch and select of the device policy.  `rho` is what the
policy integrates over (for the NB2 families the SHIFTED eta = t - log phi).

"exact[k]" is E H^(k) per unit weight on the 20-node rule, WITHOUT the "- y rho" / "- y" that the canonical entries subtract:
    logistic, binomial, negbin   m E softplus^(k),  m = trials (negbin: y + phi)
    probit, cloglog              y E h1^(k) + (m - y) E h0^(k)
    poisson                      exp(rho + s / 2), every order
    ztpoisson                    E A^(k),  A = log(exp(e^t) - 1)
    ztnegbin                     (y + phi) E softplus^(k) + E g^(k),  g = log(1 - (1 + e^eta)^-phi)
    beta                         E h^(k),  h = lgamma(phi sigma) + lgamma(phi (1 - sigma)) - phi l sigma   (the fixture's y is l = logit y)
    beta_disp, negbin_disp       FOUR rows: E h_l, E d_t h_l, E d_t^2 h_l, E h_ll, the derivatives in lambda = log phi of the Beta h and of
                                 the NB2 term (y + phi) softplus(eta) - y eta, eta = t - log phi
                                 Their `mag` is the size of the terms the device formula adds (section 41's scale), not sum w |term|:
                                 the four are differences formed BEHIND the node sums.
`mean` is the exact response mean per trial of the policies that have one of their own (HAS_MEAN), NaN where it overflows.

Measures (`CAP` = 1e-10).  Pointwise |got - exact| / |exact| <= CAP on the entries of the fixture's mask `resolvable`
(|exact| >= 1e-3 mag, mag = sum_k w_k |H^(k)(t_k)|, and the host formula within CAP / 4 there).  Absolute |got - exact| / scale on
every entry, scale = max(1, |exact|, family size) (`scale`), bound 8 x the host formula's own worst figure with a floor of
64 x 2^-53 (`abs_bounds`).  A canonical entry returns fl(E H' - y) and fl(E H - y rho): what lies below 2^-53 of y (y rho) is not in
its output, so the device is held pointwise at orders 0 and 1 only where |exact| >= 1e-3 (mag + |y rho|) resp. (mag + |y|)
(`device_mask`); every other entry stays under the absolute measure, whose scale is at least y."""
import os

import numpy as np

CAP = 1e-10
DEG = 20
FLOOR = 64.0 * 2.0 ** -53
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'glmm_tail_exact.npz')
FAMILIES = ('logistic', 'binomial', 'negbin', 'probit', 'cloglog', 'poisson', 'ztpoisson', 'ztnegbin', 'beta', 'beta_disp', 'negbin_disp')
DISPERSION = ('beta_disp', 'negbin_disp')                                # four quantities per row: E h_l, E d_t h_l, E d_t^2 h_l, E h_ll
HAS_MEAN = ('probit', 'cloglog', 'ztpoisson', 'ztnegbin', 'beta')        # the policies with a response mean of their own
NEAR_OVERFLOW = 600.0                                                    # the offset just below the overflow of exp (the predict rows)
MINUS_Y = ('logistic', 'binomial', 'negbin', 'poisson', 'ztpoisson', 'ztnegbin')     # the entry subtracts y rho and y
RHO_EXT = np.array([-40.0, -30.0, -12.0, -5.0, -2.0, 0.4, 2.5, 5.0, 12.0, 30.0, 40.0])
S_EXT = np.array([0.0, 0.5, 3.0, 40.0])
S_MIN = 5e-324                                                           # stands for s = 0 (see `rows`)
LOG700 = float(np.log(700.0))
ETA_SMALL = -6.907755278982137                                           # log 1e-3, TruncNegBinLik::ETA_SMALL


def gh():
    return np.polynomial.hermite.hermgauss(DEG)


def around(tau):
    """nextafter(tau, -inf), tau, nextafter(tau, +inf), tau (1 -+ 1e-6); around 0 the last two are -+1e-6."""
    rel = (-1e-6, 1e-6) if tau == 0.0 else (tau * (1.0 - 1e-6), tau * (1.0 + 1e-6))
    return np.array([np.nextafter(tau, -np.inf), tau, np.nextafter(tau, np.inf), rel[0], rel[1]])


def _grid(*axes):
    return [a.ravel() for a in np.meshgrid(*axes, indexing='ij')]


def _softplus(t):
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def _softplus_inv(v):
    return float(np.log(np.expm1(v)))


def _pack(kind, rho, s, y=0.0, trials=1.0, phi=1.0):
    n = max(np.size(a) for a in (rho, s, y, trials, phi))
    f = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)).copy()
    return dict(kind=np.full(n, kind, dtype=np.int64), rho=f(rho), s=f(s), y=f(y), trials=f(trials), phi=f(phi))


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _link_points():
    rng = np.random.default_rng(35)                                      # tests/test_glmm_link_host_math.py::_points
    rho, s = rng.uniform(-5.0, 5.0, size=40), rng.uniform(0.0, 3.0, size=40)
    s[7] = 0.0
    rho[0], rho[1], s[0], s[1] = -5.0, 5.0, 3.0, 3.0
    return rho, s


def _trials_y(n):
    """trials in {1, 13, 1e6} x y in {0, 1, trials}, cycled over n rows."""
    i = np.arange(n)
    trials = np.array([1.0, 13.0, 1e6])[i % 3]
    y = np.where((i // 3) % 3 == 0, 0.0, np.where((i // 3) % 3 == 1, 1.0, trials))
    return trials, y


def rows(family):
    """The rows of a family: dict(kind, rho, s, y, trials, phi), N not a multiple of 64."""
    rho_e, s_e = _grid(RHO_EXT, S_EXT)
    if family == 'logistic':
        parts = [_pack(1, np.tile(rho_e, 2), np.tile(s_e, 2), y=np.repeat([0.0, 1.0], rho_e.size)),
                 _pack(2, np.tile(around(0.0), 2), 0.0, y=np.repeat([0.0, 1.0], 5))]
    elif family == 'binomial':
        rho, s, trials, yk = _grid(RHO_EXT, S_EXT, np.array([1.0, 13.0, 1e6]), np.arange(3.0))
        y = np.where(yk == 0, 0.0, np.where(yk == 1, 1.0, trials))
        t5, y5 = _trials_y(5)
        parts = [_pack(1, rho, s, y=y, trials=trials), _pack(2, around(0.0), 0.0, y=y5, trials=t5)]
    elif family == 'negbin':
        rho, s, phi = _grid(RHO_EXT, S_EXT, np.array([0.05, 1.0, 1e3]))
        y = np.arange(rho.size) % 7.0
        parts = [_pack(1, rho, s, y=y, trials=y + phi, phi=phi),
                 _pack(2, around(0.0), 0.0, y=np.arange(5.0), trials=np.arange(5.0) + 1.0, phi=1.0)]
    elif family in ('probit', 'cloglog'):
        rho0, s0 = _link_points()
        t0, y0 = _trials_y(40)
        t1, y1 = _trials_y(rho_e.size)
        parts = [_pack(0, rho0, s0, y=y0, trials=t0), _pack(1, rho_e, s_e, y=y1, trials=t1),
                 _pack(1, NEAR_OVERFLOW, np.array([0.0, 3.0]), y=np.array([1.0, 0.0]), trials=np.array([1.0, 13.0]))]
        th = [around(0.0)]
        if family == 'probit':
            th.append(np.array([-40.0, -37.6, -20.0, -8.0, 8.0, 20.0, 37.4, 40.0]))   # erfcx(-t / sqrt 2) overflows between 37.4 and 37.6
        else:
            th.append(around(LOG700))                                    # u = e^t = 700
        th = np.concatenate(th)
        th = np.tile(th, 2)
        # cloglog: successes AND failures on every threshold row -- past u = 700 the policy sets r (below 1e-301) to 0 by design, and
        # with y = trials that flushed value would be the whole of E H'
        parts.append(_pack(2, th, 0.0, y=np.repeat([1.0, 5.0], th.size // 2),
                           trials=np.repeat([1.0, 13.0] if family == 'probit' else [2.0, 13.0], th.size // 2)))
    elif family == 'poisson':
        parts = [_pack(1, rho_e, s_e), _pack(2, around(0.0), 0.0)]       # y = 0: the relative bound on exp is then the entry's own
    elif family == 'ztpoisson':
        rho0, s0 = _grid(np.array([-12.0, -10.0, -8.0, -5.0, -2.0, 0.0, 2.5, 5.0]), np.array([0.0, 0.5, 1.5, 3.0]))
        th = np.concatenate([around(0.0), around(LOG700)])
        parts = [_pack(0, rho0, s0), _pack(1, rho_e, s_e), _pack(1, NEAR_OVERFLOW, np.array([0.0, 3.0])), _pack(2, th, 0.0)]
        n = 0
        for p in parts:
            p['y'] = 1.0 + (n + np.arange(p['rho'].size)) % 7.0
            n += p['rho'].size
    elif family == 'ztnegbin':
        phi0, rho0, s0 = _grid(np.array([0.05, 1.0, 50.0, 1e3]), np.array([-30.0, -12.0, -5.0, 0.4, 2.5, 5.0]), S_EXT)
        phi1, rho1, s1 = _grid(np.array([0.05, 1.0, 50.0, 1e3]), np.array([-40.0, -2.0, 12.0, 30.0, 40.0]), S_EXT)
        th_eta, th_phi = [], []
        for phi in (2.0, 50.0):                                          # t = 0 (not phi = 1: there g = log sigma and H''' (0) is exactly 0)
            th_eta.append(around(0.0)); th_phi.append(np.full(5, phi))
        for phi in (1.0, 10.0, 10.01, 50.0):                             # eta = log 1e-3, v = phi softplus either side of 0.01
            th_eta.append(around(ETA_SMALL)); th_phi.append(np.full(5, phi))
        for eta in (-8.0, -12.0, -20.0):                                 # v = 0.01 below log 1e-3
            th_eta.append(np.full(5, eta)); th_phi.append(around(0.01 / float(_softplus(eta))))
        for phi in (1e3, 1e5):                                           # v = 700
            th_eta.append(around(_softplus_inv(700.0 / phi))); th_phi.append(np.full(5, phi))
        parts = [_pack(0, rho0, s0, phi=phi0), _pack(1, rho1, s1, phi=phi1),
                 _pack(1, NEAR_OVERFLOW, np.array([0.0, 3.0, 0.0, 3.0]), phi=np.array([0.05, 0.05, 1e3, 1e3])),
                 _pack(2, np.concatenate(th_eta), 0.0, phi=np.concatenate(th_phi))]
        n = 0
        for p in parts:
            p['y'] = 1.0 + (n + np.arange(p['rho'].size)) % 7.0
            n += p['rho'].size
    elif family == 'negbin_disp':
        PHI, Y = np.array([0.3, 2.0, 15.0, 200.0, 3000.0]), np.array([0.0, 1.0, 7.0, 400.0])
        R0, S0 = np.array([-30.0, -12.0, -5.0, -2.0, 0.0, 2.5, 5.0, 12.0, 30.0]), np.array([0.0, 0.5, 3.0])
        raw0, s0, phi0, y0 = _grid(R0, S0, PHI, Y)                       # tests/test_glmm_dispersion_host_math.py: rho is the RAW predictor
        eta1, s1, phi1, y1 = _grid(RHO_EXT, S_EXT, PHI, Y)
        th = np.tile(around(0.0), 2)
        parts = [_pack(0, raw0 - np.log(phi0), s0, y=y0, trials=y0 + phi0, phi=phi0), _pack(1, eta1, s1, y=y1, trials=y1 + phi1, phi=phi1),
                 _pack(2, th, 0.0, y=np.repeat([0.0, 7.0], 5), trials=np.repeat([0.0, 7.0], 5) + 15.0, phi=15.0)]
    elif family in ('beta', 'beta_disp'):
        PHI, L = np.array([0.3, 2.0, 15.0, 200.0, 3000.0]), np.array([-8.0, -0.7, 0.4, 3.0])
        R0, S0 = np.array([-30.0, -12.0, -5.0, -2.0, 0.0, 2.5, 5.0, 12.0, 30.0]), np.array([0.0, 0.5, 3.0])
        rho0, s0, phi0, l0 = _grid(R0, S0, PHI, L)
        rho1, s1, phi1, l1 = _grid(np.union1d(R0, RHO_EXT), S_EXT, PHI, L)
        new = ~(np.isin(rho1, R0) & np.isin(s1, S0))
        th_t, th_phi = [around(0.0), around(0.0)], [np.full(5, 2.0), np.full(5, 3000.0)]
        # the z < 10 steps of polygamma: 1 + phi mu (t < 0 rows) and 1 + phi (1 - mu) (the mirrored t > 0 rows) on 1 .. 10 and 1e6,
        # -3 .. +3 ulp of phi around the landing point
        for t in (-3.0, 0.7):
            mu = 1.0 / (1.0 + np.exp(-t))
            for j in list(range(2, 11)) + [1e6]:
                phi = (j - 1.0) / mu
                for step in range(-3, 4):
                    p = phi
                    for _ in range(abs(step)):
                        p = np.nextafter(p, np.inf if step > 0 else -np.inf)
                    th_t += [np.array([t, -t])]; th_phi += [np.array([p, p])]
            for k in (1.0, 2.0, 3.0):                                    # 1 + k ulp
                th_t += [np.array([t, -t])]; th_phi += [np.full(2, k * 2.0 ** -52 / mu)]
        th_t += [np.array([-40.0, 40.0])]; th_phi += [np.full(2, 15.0)]  # 1 + phi mu = 1 exactly
        th_t, th_phi = np.concatenate(th_t), np.concatenate(th_phi)
        parts = [_pack(0, rho0, s0, y=l0, phi=phi0), _pack(1, rho1[new], s1[new], y=l1[new], phi=phi1[new]),
                 _pack(2, th_t, 0.0, y=np.where(np.arange(th_t.size) % 2 == 0, -0.7, 3.0), phi=th_phi)]
    else:
        raise ValueError(family)
    out = _cat(parts)
    # every entry refuses r = 0 ("r[g] is not positive", glmms_check of csrc/lrvb_api.hip): the s = 0 rows carry the smallest s the
    # entries accept, the smallest positive double.  sqrt(s) = 2.2e-162 moves no node off rho unless |rho| is itself below 1e-146
    # (the rows next to t = 0, whose twenty nodes then lie at +-1e-161 on BOTH sides of 0); the exact values are computed at that s.
    out['s'] = np.where(out['s'] == 0.0, S_MIN, out['s'])
    if out['rho'].size % 64 == 0:                                        # dead lanes next to the last rows
        out = _cat([out, {k: a[:1] for k, a in out.items()}])
    assert out['rho'].size % 64 != 0 and out['rho'].size <= 3000
    return out


def _logistic_expected(rho, s, trials):
    from lrvb_amd import glmm_hurdle
    from lrvb_amd.glmm_binomial import _nodes
    gx, gw = gh()
    t, wk = _nodes(rho, s, gx, gw)
    return np.stack([trials * (a * wk).sum(-1) for a in glmm_hurdle._logistic_node(t)])


def host(family, r):
    """The package's HOST restatement of the device policy at the rows r: E H^(k), k = 0..4 (5 x n; the four dispersion quantities,
    4 x n, for a dispersion family), and the response mean per trial where the policy has one of its own (else None)."""
    from lrvb_amd import glmm_beta, glmm_binomial, glmm_hurdle
    gx, gw = gh()
    rho, s, y, trials, phi = r['rho'], r['s'], r['y'], r['trials'], r['phi']
    with np.errstate(all='ignore'):
        if family in ('logistic', 'binomial', 'negbin'):
            return _logistic_expected(rho, s, trials), None
        if family in ('probit', 'cloglog'):
            mean = glmm_binomial.link_response_mean(family, rho, s, np.ones_like(rho), gx, gw)
            return glmm_binomial.link_expected_h(family, rho, s, y, trials, gx, gw), mean
        if family == 'poisson':
            return np.tile(np.exp(rho + 0.5 * s), (5, 1)), None
        if family == 'ztpoisson':
            return glmm_hurdle.ztp_expected_A(rho, s, gx, gw), glmm_hurdle.ztp_response_mean(rho, s, gx, gw)
        if family == 'ztnegbin':
            return glmm_hurdle.ztnb_expected_H(rho, s, y, phi, gx, gw), glmm_hurdle.ztnb_response_mean(rho, s, phi, gx, gw)
        if family == 'beta':
            return glmm_beta.beta_expected_h(rho, s, y, phi, gx, gw), glmm_beta.beta_response_mean(rho, s, gx, gw)
        if family == 'beta_disp':
            return glmm_beta.beta_expected_h_dispersion(rho, s, y, phi, gx, gw), None
        if family == 'negbin_disp':
            # `negbin_expected_h_dispersion` forms eta = rho - log phi itself; the rows hold eta, so its two steps are taken here: the
            # node sums of `_logistic_nodes` and the combination behind them
            t, wk = glmm_binomial._nodes(rho, s, gx, gw)
            v, e1, e2, e3 = [(a * wk).sum(-1) for a in glmm_binomial._logistic_nodes(t)]
            return np.stack([(phi * v - trials * e1) + y, phi * e1 - trials * e2, phi * e2 - trials * e3, phi * (v - 2.0 * e1) + trials * e2]), None
    raise ValueError(family)


def scale(family, r, exact):
    """The scale of the absolute measure, one row per order."""
    size = {'ztnegbin': r['y'] + r['phi'], 'negbin': r['trials'], 'binomial': r['trials'], 'probit': r['trials'], 'cloglog': r['trials'],
            'beta': r['phi'], 'beta_disp': r['phi'], 'negbin_disp': r['trials']}.get(family, np.ones_like(r['rho']))
    return np.maximum(np.maximum(1.0, np.abs(exact)), size[None, :])


def rel_err(got, exact):
    """|got - exact| / |exact|; 0 where they are equal (an exact 0 included), inf where exact is 0 and got is not."""
    err = np.abs(got - exact)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(err == 0.0, 0.0, err / np.abs(exact))


def host_figures(family, r, exact, mag):
    """(host_rel, host_abs, resolvable), one row per order, of the host formula.  An exact 0 (a value below the fp64 range) is
    resolvable where the host returns 0 too."""
    h, _ = host(family, r)
    rel = rel_err(h, exact)
    # the existing CPU grids of the Beta and the zero-truncated NB2 family are held pointwise WHOLE by their own host tests (the Beta
    # grid holds two entries where the third derivative is 2e-4 of its node terms): there the size condition is waived, which only
    # adds entries to the mask
    whole = (r['kind'] == 0) & (family in ('beta', 'ztnegbin'))
    resolvable = ((np.abs(exact) >= 1e-3 * mag) | whole[None, :]) & (rel <= CAP / 4.0)
    return rel, np.abs(h - exact) / scale(family, r, exact), resolvable


def abs_bounds(host_abs):
    """Per order: 8 x the host's own worst absolute figure, floor 64 x 2^-53."""
    return np.maximum(8.0 * np.max(host_abs, axis=-1), FLOOR)


def device_mask(family, fx):
    """`resolvable`, and at orders 0 and 1 of a canonical entry only where the subtracted y rho (y) leaves the entry resolvable."""
    m = fx['resolvable'].copy()
    if family in MINUS_Y and family not in DISPERSION:
        e = np.abs(fx['exact'])
        m[0] &= e[0] >= 1e-3 * (fx['mag'][0] + np.abs(fx['y'] * fx['rho']))
        m[1] &= e[1] >= 1e-3 * (fx['mag'][1] + np.abs(fx['y']))
    return m


def load(family):
    """The committed fixture of a family: the inputs of `rows`, deg, exact, mean, mag, host_rel, host_abs, resolvable."""
    with np.load(FIXTURE) as z:
        return {k[len(family) + 1:]: z[k] for k in z.files if k.startswith(family + '/')}


def undo(family, fx, sums, idx=None):
    """E H^(k), k = 1..4 (4 x n) of the rows idx from their K = 1 group sums [a1, a2, c11, c12, c22] at unit weight; also asserts
    that a2 and c11 carry the same E H''."""
    y = fx['y'] if idx is None else fx['y'][idx]
    a1 = sums[:, 0] + (y if family in MINUS_Y else 0.0)
    return np.stack([a1, 2.0 * sums[:, 1], 2.0 * sums[:, 3], 4.0 * sums[:, 4]]), sums[:, 2]

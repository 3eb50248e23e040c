"""Inputs, plain references, bounds and restated faults for the softmax pass (csrc/k_softmax.hip, `softmax_pass_kernel`), used
by tests/test_gpu_softmax_pass.py on the device and by tests/test_softmax_pass_reference_host_math.py on the CPU.

    gradient mode   p = softmax(X beta^T), value = sum w (lse - z_y), r = w (p - e_y), g = X^T r       `ctx.softmax_terms`
    product mode    t = X V^T, u = w p o (t - p . t), hv = X^T u                                       `ctx.softmax_hvp`
    rows-only mode  T = X A_q^T per output q, out[n, q] = sum_a (p_na - e_na) T_na                     `ctx.softmax_obs_influence`

NumPy only.  Two oracles:

  exact     K a power of two, small-integer X, w, V, A; beta non-zero in ONE column j* only, beta[a, j*] = 1000 (a + 1), and
            x[n, j*] in {-1, 0, +1}: a 0 row has all logits 0 and p = 1/K, a +1 row saturates to the one-hot of the last class
            (the maximum's exp argument is 0, every other one <= -1000), a -1 row to the reference class (m = 0, p = 0).  p is a
            multiple of 1/K, r and the influence rows of 1/K, u and the Hessian weight columns of 1/K^2: every partial sum is a
            dyadic rational far below 2^53 / K^2, so every summation order gives the same float64 and the device result must be
            BITWISE the int64 computation (scaled by K, K^2).  The value's term w log K of the 0 rows is not exact: the value
            is bitwise on the saturated-only variant and bounded otherwise.
  bounded   real data against the longdouble evaluation `ld_eval`, entry by entry: |got - ref| <= 1.01 2^-53 B, B a running
            first-order count in units of U = 2^-53 read off the kernel text (`bounds`):

              z, t, T     a dot product over the padded columns: one rounding per non-zero product (a wave adds its columns on
                          two matrix-core chains; a padding column or a zero of U adds an exact zero), the join of the two
                          chains and the gather of the NW partial tiles: nz + NW (nz, if nz <= 1), times sum |x| |u|
              p           relative: exp at E = 2 ulp = 4 U and the rounding of z - m on its argument (4 + |z - m|); s the same
                          p-weighted over the K classes, + 4 DPP levels + the add of exp(-m); the quotient 1; the error of z
                          itself through the softmax (|dz_a| + sum_b p_b |dz_b|: any common shift m cancels)
              r           |w| (abs(p) + 2 |p - e|): the subtraction and the product by w
              value term  |w| (sum_b p_b |dz_b| + rel(s) + 4 |log s| + |m + log s| + |dz_y| + |lse - z_y|) + |term|
              u           pt = p t (1), s = sum pt (4 DPP levels), t - s (1), w p (1), the product (1)
              step B      8 per chunk this workgroup takes (two 16 x 16 x 4 instructions per tile) + the reducer's depth
                          ceil(grid / 8) + 8 (`hvp_multi_reduce_kernel`: eight strided chains, then the eight sums)
              value       2 per trip (rows l4, l4 + 4 into the lane's running sum) + 6 (wave butterfly) + 8 (`sum_partials_kernel`)
              influence   per term (p - e) T: the subtraction, the product; one addition per further non-zero term
              reference   the longdouble evaluation's own rounding, unit 2^-64 = U / 2048: n / 2048 + 1 per sum of n terms
              underflow   a float64 result below 2^-1022 is a multiple of 2^-1074: 4 2^-1074 absolute on p and on every output

The restatement `f64_pass` / `f64_influence` is the kernel's order in float64 NumPy (workgroup g takes chunks g, g + grid, ..;
per chunk: clamped rows, zero-padded weights, labels and p; T by wave slices; the DPP rotate tree; step B per chunk; the fixed
order reducers).  It takes the restated faults of `PASS_MUTATIONS`: what it returns with one of them must leave a bound or
break bitwise equality in at least one case of the GPU file.
"""
import os

import numpy as np

import hvp_multi_reference as hr

LD = np.longdouble
assert np.finfo(LD).eps == 2.0 ** -63, 'the references need the 80-bit long double'
U_ROUND = hr.U_ROUND
SM_ROWS, SM_GRID = hr.HM_ROWS, hr.HM_MAX_GRID      # the same chunk and grid as the multi-vector pass
GRAD, HVP, ROWS = 'gradient', 'product', 'rows'
MODES = (GRAD, HVP, ROWS)
FOUR_WAVES = 4                                     # tuning bit 2
E_ULP = 4.0                                        # device exp / log: 2 ulp = 4 U (section 28)
TINY_U = 4.0 * 2.0 ** -1074 / U_ROUND              # the underflow floor, in units of U
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'softmax_pass_probes.npz')

n_chunks, grid, trips = hr.n_chunks, hr.grid, hr.chunks_per_workgroup
worst_entry = hr.worst_entry


def full_trips(N, min_rows=9):
    """The trips of the chunk loop that hold at least `min_rows` rows (more than one chunk, both T registers): a last trip of ONE
    row, as at N = 2049 or 4097, shows a stale half or a wrong row only if that row happens to differ."""
    return sum(1 for t in range(trips(N)) if min(max(N - t * SM_ROWS * SM_GRID, 0), SM_ROWS * SM_GRID) >= min_rows)


# ---- the dispatch table (sm_dispatch) --------------------------------------------------------------------------------------
def dispatch(P, aligned=True, mode=GRAD, four_waves=False):
    """(NB, NW, ODD) of the instance of softmax_pass_kernel that runs."""
    nb = hr.n_blocks(P)
    if P % 2 != 0 or not aligned:
        return nb, 4, True
    nw = 8 if nb % 2 == 0 and not four_waves else 4
    if mode == GRAD and nb == 8:
        nw = 4                                     # the gradient mode at NB = 8 runs 4 waves
    return nb, nw, False


def all_instances():
    """Every (mode, NB, NW, ODD) that sm_dispatch can launch."""
    out = set()
    for mode in MODES:
        for nb in range(1, 9):
            out.add((mode, nb, 4, True))
            out.add((mode, nb, 4, False))
            if nb % 2 == 0 and not (mode == GRAD and nb == 8):
                out.add((mode, nb, 8, False))
    return out


def wave_flags(P, aligned=True):
    """The tuning flags worth running: the four-wave bit changes the instance at an even, aligned, even-NB width only."""
    return (0, FOUR_WAVES) if (P % 2 == 0 and aligned and hr.n_blocks(P) % 2 == 0) else (0,)


# ---- shapes of the GPU file, replayed by the CPU file -------------------------------------------------------------------
N_GRID = [1, 7, 8, 9, 17, 2047, 2048, 2049, 4097, 6145]
P_EVEN = [2, 126, 128, 130, 254, 256, 258, 384, 512, 640, 768, 896, 1022, 1024]
P_ODD = [1, 3, 127, 129, 257, 511, 639, 767, 769, 1023]              # NB = 1, 1, 1, 2, 3, 4, 5, 6, 7, 8
P_ROWGRID = [2, 130, 129, 1024, 1023]
K_REAL = [2, 3, 5, 8, 16, 17]
K_EXACT = [2, 4, 8, 16]
N_TWO_TRIPS = 2121
UNALIGNED_P = 130                                  # one even P on a base offset by 8 bytes


def _cases(klist):
    """(N, P, K, aligned): every width at N = 9 (two chunks, a ragged one) and N = 2121 (workgroups 0 .. 9 take a second chunk,
    the last one ragged: at N = 2049 the second trip holds ONE row, and a stale half that happens to agree on it goes unseen);
    every N of the row grid at P_ROWGRID; the unaligned base at 9, 2049 and 4097.  K cycles through `klist`, with the widest
    classes kept off the largest matrices (the host reference is N P K longdouble operations)."""
    out, i = [], 0
    for P in P_EVEN + P_ODD:
        for N in (9, N_TWO_TRIPS):
            out.append((N, P, klist[i % len(klist)], True)); i += 1
    for P in P_ROWGRID:
        for N in N_GRID:
            if N == 9:
                continue
            K = klist[i % len(klist)]; i += 1
            if N * P > 3_000_000:
                K = klist[i % 3]
            out.append((N, P, K, True))
    for N in (9, N_TWO_TRIPS, 4097):
        out.append((N, UNALIGNED_P, klist[i % len(klist)], False)); i += 1
    return out


REAL_CASES = _cases(K_REAL) + [(2121, 130, 17, True), (4097, 129, 17, True), (4097, 130, 16, True), (6145, 2, 17, True)]
EXACT_CASES = _cases(K_EXACT) + [(4097, 130, 16, True), (4097, 129, 16, True), (6145, 2, 16, True)]

INFL_N = 4099
INFL_WINDOWS = [(0, 4099), (0, 1), (3, 12), (8, 16), (2041, 4099), (4091, 4099), (4098, 4099)]
INFL_CASES = [(130, 6, 7), (130, 17, 3), (2, 17, 2), (129, 4, 11), (384, 3, 9), (1024, 2, 17), (1023, 6, 4), (258, 9, 5)]   # (P, K, Q)
HESS_CASES = [(300, 66, 16), (300, 9, 16), (203, 66, 8), (77, 3, 4), (64, 130, 2)]                          # (N, P, K)
STATE_CASE = (2121, 130)
GOLDEN_CASES = [(17, 40, 5), (17, 40, 17), (12, 40, 2)]                  # (N, P, K): every row in mpmath


def is_cheap(N, P, K):
    """The cases the CPU file replays in full: the reference is N P K longdouble operations."""
    return N * P * (K - 1) <= 6_000_000


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def case_seed(N, P, K):
    return 1000003 * P + 7919 * N + 101 * K


def exact_case(N, P, K, Q=3, saturated_only=False):
    """Integer design of the exact oracle.  Column 0 is the constant 1 (P >= 2), column j* = P - 1 holds the row kind."""
    assert K in K_EXACT
    rng = np.random.default_rng(case_seed(N, P, K) + 17)
    Km = K - 1
    X = rng.integers(-3, 4, size=(N, P)).astype(np.float64)
    js = P - 1
    if P >= 2:
        X[:, 0] = 1.0
    kind = rng.integers(-1, 2, size=N)
    kind[N - 1] = 0                                # the last row is uniform: a clamped copy given weight cannot cancel
    if saturated_only:
        kind = np.where(kind == 0, 1, kind)
    X[:, js] = kind
    w = rng.integers(1, 5, size=N).astype(np.float64)
    y = rng.integers(0, K, size=N)
    beta = np.zeros((Km, P))
    beta[:, js] = 1000.0 * (np.arange(Km) + 1)
    V = rng.integers(-3, 4, size=(Km, P)).astype(np.float64)
    A = rng.integers(-3, 4, size=(Q, Km * P)).astype(np.float64)
    return dict(X=X, w=w, y=y, K=K, beta=beta, V=V, A=A, kind=kind, js=js)


def exact_outputs(c):
    """Every output of the exact design as float64 from int64 arithmetic: dict(p, value_sat (None unless saturated only), g,
    hv, infl (N x Q), r, u, coef(a, b)).  Asserts every scaled integer below 2^53."""
    X, K, kind = c['X'].astype(np.int64), c['K'], c['kind']
    assert np.array_equal(X, c['X'])
    N, P = X.shape
    Km = K - 1
    w, y = c['w'].astype(np.int64), c['y']
    pK = np.zeros((N, Km), dtype=np.int64)                     # K p
    pK[kind == 0] = 1
    pK[kind == 1, Km - 1] = K
    E = np.zeros((N, Km), dtype=np.int64)
    E[np.flatnonzero(y > 0), y[y > 0] - 1] = 1
    rK = w[:, None] * (pK - K * E)                             # K r
    gK = rK.T @ X
    V, A = c['V'].astype(np.int64), c['A'].astype(np.int64)
    t = X @ V.T
    sK = (pK * t).sum(axis=1)
    uKK = w[:, None] * pK * (K * t - sK[:, None])              # K^2 u
    hvKK = uKK.T @ X
    Q = A.shape[0]
    M = (X @ A.reshape(Q * Km, P).T).reshape(N, Q, Km)
    inflK = np.einsum('na,nqa->nq', pK - K * E, M)
    for v in (gK, hvKK, inflK, uKK):
        assert np.max(np.abs(v), initial=0) < 2 ** 52
    z_y = np.where(y > 0, kind * 1000 * y, 0)
    m = np.where(kind == 1, 1000 * Km, 0)
    out = dict(p=pK / K, g=(gK / K).ravel(), hv=(hvKK / K ** 2).ravel(), infl=inflK / K, r=rK / K, u=uKK / K ** 2,
               pK=pK, X=X, w=w)
    out['value_sat'] = float(np.sum(w * (m - z_y))) if not np.any(kind == 0) else None
    return out


def exact_hessian(c):
    """H (D x D) of the exact design: block (a, b) = X^T diag(w p_a (delta_ab - p_b)) X, from int64 scaled by K^2."""
    e = exact_outputs(c)
    X, w, pK, K = e['X'], e['w'], e['pK'], c['K']
    N, P = X.shape
    Km = K - 1
    H = np.empty((Km * P, Km * P))
    for a in range(Km):
        for b in range(a, Km):
            cKK = w * pK[:, a] * ((K if a == b else 0) - pK[:, b])
            blk = (X.T * cKK) @ X
            assert np.max(np.abs(blk), initial=0) < 2 ** 52
            H[a * P:(a + 1) * P, b * P:(b + 1) * P] = blk / K ** 2
            H[b * P:(b + 1) * P, a * P:(a + 1) * P] = blk / K ** 2
    return H


PROBE_ROWS = (0, 3, 4, 7, 2047, 2048, 4095, 4096)
EXTREME_ROWS = (1, 2, 5, 6, 9, 10, 11)
EXTREME_KINDS = ('ref max', 'lane0 max', 'last max', 'tie', 'all low', 'gap 30', 'gap 700')


def extreme_logits(kind, Km):
    a = np.arange(Km, dtype=np.float64)
    if kind == 'ref max':
        return -0.75 * (a + 1)
    if kind == 'lane0 max':
        z = -1.5 - 0.5 * a; z[0] = 4.25
        return z
    if kind == 'last max':
        z = -1.0 - 0.25 * a; z[Km - 1] = 3.75
        return z
    if kind == 'tie':                                          # an exact two-way tie at the maximum (with the reference class at Km = 1)
        if Km == 1:
            return np.zeros(1)
        z = np.full(Km, -1.0); z[0] = z[Km - 1] = 2.5
        return z
    if kind == 'all low':
        return -750.0 - 3.0 * a
    if kind == 'gap 30':
        z = np.zeros(Km); z[0] = 30.0
        return z
    if kind in ('gap 700', 'gap 700 last'):
        z = np.zeros(Km); z[Km - 1] = 700.0
        return z
    raise ValueError(kind)


def special_plan(N, P):
    """[(row, kind, column)]: rows read alone through an indicator column (x = 1 on that row only).  'probe' rows keep their
    ordinary entries; the others are zero outside the constant and their indicator column, whose beta holds the logits of
    the kind exactly.  The last row is extreme when N mod 8 != 0 (its clamped copies then run with weight 0).  As many as fit
    beside the constant column and one ordinary column, the last row first, columns from P - 1 downwards."""
    plan = []
    if N - 1 not in PROBE_ROWS and N - 1 not in EXTREME_ROWS:
        plan.append((N - 1, 'gap 700 last' if N % SM_ROWS else 'probe'))
    ext = [(r, k) for r, k in zip(EXTREME_ROWS, EXTREME_KINDS) if r < N]
    prb = [(r, 'probe') for r in PROBE_ROWS if r < N]
    while ext or prb:
        if prb:
            plan.append(prb.pop(0))
        if ext:
            plan.append(ext.pop(0))
    plan = plan[:max(0, P - 2)]
    return [(r, k, P - 1 - i) for i, (r, k) in enumerate(plan)]


def real_case(N, P, K, Q=3):
    """Normal X / sqrt(P) with a constant first column (P >= 2; its beta is 0, so it only serves the unit probes), beta with
    logits of a few units, w in [0.2, 2] with zeros on every fourth ordinary row and on probe row 7, labels covering 0, 1 and
    K - 1 on the probe rows, and the rows of `special_plan`."""
    rng = np.random.default_rng(case_seed(N, P, K) + 500000007)
    Km = K - 1
    X = rng.normal(size=(N, P)) / np.sqrt(P)
    beta = rng.normal(size=(Km, P)) * 2.0
    y = rng.integers(0, K, size=N)
    w = rng.uniform(0.2, 2.0, size=N)
    plan = special_plan(N, P)
    special = {r for r, _, _ in plan}
    zero = np.arange(N) % 4 == 1
    zero[list(special)] = False
    w[zero] = 0.0
    if P >= 2:
        X[:, 0] = 1.0
        beta[:, 0] = 0.0
    kinds = (0, 1, K - 1)
    for i, (r, kind, j) in enumerate(plan):
        X[:, j] = 0.0
        if kind != 'probe':
            X[r, 1:] = 0.0
            beta[:, j] = extreme_logits(kind, Km)
        X[r, j] = 1.0
        y[r] = kinds[i % 3]
    if 7 in special:
        w[7] = 0.0
    V = rng.normal(size=(Km, P))
    A = rng.normal(size=(Q, Km * P))
    return dict(X=X, w=w, y=y, K=K, beta=beta, V=V, A=A, plan=plan)


def unit_probes(P, Km):
    """A (Km x Km P): row a picks (a, the constant column 0).  With x[n, 0] = 1 the influence row is p_na - [y_n = a + 1]."""
    A = np.zeros((Km, Km * P))
    A[np.arange(Km), np.arange(Km) * P] = 1.0
    return A


def onehot(y, Km):
    E = np.zeros((y.size, Km))
    rows = np.flatnonzero(y > 0)
    E[rows, y[rows] - 1] = 1.0
    return E


# ---- the longdouble reference and the counted bounds ------------------------------------------------------------------------
def to_ld(v):
    return np.asarray(v, dtype=np.float64).astype(LD)


def ld_eval(c, want=(GRAD, HVP)):
    """All rows in longdouble: dict(z, m, s, p, lse, vterm, value, r, g, t, u, hv) (the product part if HVP in `want`)."""
    X, B, w, y = to_ld(c['X']), to_ld(c['beta']), to_ld(c['w']), c['y']
    N, Km = X.shape[0], c['K'] - 1
    z = X @ B.T
    zf = np.concatenate([np.zeros((N, 1), dtype=LD), z], axis=1)
    m = zf.max(axis=1)
    e = np.exp(zf - m[:, None])
    s = e.sum(axis=1)
    pf = e / s[:, None]
    lse = m + np.log(s)
    vterm = w * (lse - zf[np.arange(N), y])
    p = pf[:, 1:]
    r = w[:, None] * (p - to_ld(onehot(y, Km)))
    out = dict(z=z, zf=zf, m=m, s=s, pf=pf, p=p, lse=lse, vterm=vterm, value=vterm.sum(), r=r, g=(r.T @ X).ravel())
    if HVP in want:
        t = X @ to_ld(c['V']).T
        s2 = (p * t).sum(axis=1)
        u = w[:, None] * p * (t - s2[:, None])
        out.update(t=t, s2=s2, u=u, hv=(u.T @ X).ravel())
    return out


def dot_roundings(X, Uc, nw):
    """Roundings of the dot products x_n . u_q on the device: one per non-zero product, + NW (the join of the two chains and
    the gather over the waves) when there is more than one."""
    nz = (X != 0).astype(np.float64) @ (Uc != 0).astype(np.float64).T
    return np.where(nz > 1, nz + nw, nz)


def ref_units(n):
    return n / 2048.0 + 1.0


def step_b_roundings(N):
    g = grid(N)
    return 8 * trips(N) + -(-g // 8) + 8


def f64(v):
    return np.asarray(v, dtype=np.float64)


def bounds(c, ref, nw_grad=8, nw_hvp=8):
    """Entry-wise bounds in units of U (multiply by 1.01 2^-53): dict(p (N x Km, absolute), rel_p, g (D), value, hv (D)); the
    float64 magnitudes are inflated by 1e-9 to stay upper bounds."""
    X, w, y, K = c['X'], c['w'], c['y'], c['K']
    N, P = X.shape
    Km = K - 1
    aX, aw = np.abs(X), np.abs(w)
    up = 1.0 + 1e-9
    az = np.zeros((N, K))
    az[:, 1:] = (dot_roundings(X, c['beta'], nw_grad) + ref_units(P)) * (aX @ np.abs(c['beta']).T) * up
    pf, zf, m = f64(ref['pf']), f64(ref['zf']), f64(ref['m'])
    d = np.abs(zf - m[:, None])
    paz = (pf * az).sum(axis=1)
    rs = (pf * (E_ULP + d)).sum(axis=1) + 5.0
    rel_p = (E_ULP + d[:, 1:]) + rs[:, None] + 1.0 + az[:, 1:] + paz[:, None] + 1.0
    p = pf[:, 1:]
    ap = rel_p * p * up + TINY_U
    E = onehot(y, Km)
    r = np.abs(f64(ref['r']))
    ar = aw[:, None] * (ap + 2.0 * np.abs(p - E) * up)
    kB = step_b_roundings(N) + ref_units(N) + 1.0
    out = dict(p=ap, rel_p=rel_p, r=ar + r * up)
    out['g'] = ((ar + kB * r * up).T @ aX).ravel() * up
    lse, s = f64(ref['lse']), f64(ref['s'])
    vterm = np.abs(f64(ref['vterm']))
    av = aw * (paz + rs + E_ULP * np.abs(np.log(s)) + np.abs(lse) + az[np.arange(N), y] + np.abs(lse - zf[np.arange(N), y])) * up + vterm
    out['vterm'] = av + vterm
    out['value'] = float(av.sum() + (2 * trips(N) + 6 + 8 + ref_units(N) + 1.0) * vterm.sum()) * up
    if 't' in ref:
        t, s2 = f64(ref['t']), f64(ref['s2'])
        at = (dot_roundings(X, c['V'], nw_hvp) + ref_units(P)) * (aX @ np.abs(c['V']).T) * up
        apt = p * at + np.abs(t) * ap + np.abs(p * t)
        es = apt.sum(axis=1) + 4.0 * np.abs(p * t).sum(axis=1)
        dts = np.abs(t - s2[:, None])
        au = aw[:, None] * (p * (at + es[:, None] + dts) + dts * ap + 2.0 * p * dts) * up
        u = np.abs(f64(ref['u']))
        out['u'] = au + u * up
        out['hv'] = ((au + kB * u * up).T @ aX).ravel() * up
    return out


def ld_influence(c, ref, A, n0, n1):
    """(reference (rows x Q, longdouble), bound in units of U) of the influence rows of the window."""
    X, K = c['X'][n0:n1], c['K']
    Km, P, Q = K - 1, c['X'].shape[1], A.shape[0]
    pe = ref['p'][n0:n1] - to_ld(onehot(c['y'][n0:n1], Km))
    M = (to_ld(X) @ to_ld(A).reshape(Q * Km, P).T).reshape(n1 - n0, Q, Km)
    return np.einsum('na,nqa->nq', pe, M), pe, M


def influence_bound(c, bnd, pe, M, A, n0, n1, nw_rows=8):
    X, K = c['X'][n0:n1], c['K']
    Km, P, Q = K - 1, c['X'].shape[1], A.shape[0]
    up = 1.0 + 1e-9
    A2 = A.reshape(Q * Km, P)
    aM = ((dot_roundings(X, A2, nw_rows) + ref_units(P)) * (np.abs(X) @ np.abs(A2).T)).reshape(n1 - n0, Q, Km) * up
    pe, M = np.abs(f64(pe)), np.abs(f64(M))
    ap = bnd['p'][n0:n1]
    term = pe[:, None, :] * M
    err = M * (ap[:, None, :] + pe[:, None, :]) + pe[:, None, :] * aM + term
    adds = np.maximum((M != 0).sum(axis=2) - 1, 0) + ref_units(Km)
    return (err.sum(axis=2) + adds * term.sum(axis=2)) * up


def scale(B):
    """Units of U -> the absolute bound; every compared output is a float64, so none is held below the underflow floor."""
    return 1.01 * U_ROUND * np.asarray(B, dtype=np.float64) + 4.0 * 2.0 ** -1074


# ---- the kernel's order in float64 NumPy, with restated faults --------------------------------------------------------------
PASS_MUTATIONS = ('stale weights', 'stale labels', 'stale p', 'slot not flipped', 'rows l4 and l4 + 4 swapped', 'm not clamped',
                  'lane Km active', 'label off by one', 'phantom row weighted')


def _row16(v, op):
    """The row_ror 8, 4, 2, 1 tree over the 16 lanes (last axis): every lane ends with the full reduction in its own order."""
    for n in (8, 4, 2, 1):
        v = op(v, np.roll(v, n, axis=-1))
    return v


def _wave_dot(Xc, Uc, P, nw):
    """T = X_chunk U^T as the sum of the NW waves' column slices."""
    Ppad = hr.padded_cols(P)
    pw = Ppad // nw
    T = None
    for wv in range(nw):
        lo, hi = wv * pw, min((wv + 1) * pw, P)
        if lo >= P:
            break
        part = Xc[..., lo:hi] @ Uc[:, lo:hi].T
        T = part if T is None else T + part
    return T


def _sum_partials(part):
    sh = np.zeros(256)
    sh[:part.size] = part
    s = 128
    while s > 0:
        sh[:s] += sh[s:2 * s]
        s >>= 1
    return sh[0]


def _reduce_grid(Rpart):
    chains = [Rpart[r::8].sum(axis=0) if r < Rpart.shape[0] else 0.0 for r in range(8)]
    t = chains[0]
    for r in range(1, 8):
        t = t + chains[r]
    return t


def f64_pass(c, mode, nw=4, p_in=None, mut=None):
    """The pass in the kernel's order.  GRAD: (value, g (D), p (N x Km)); HVP: hv (D), reading `p_in`.  `mut`: one of
    PASS_MUTATIONS.  A stale staging half holds what the workgroup's previous chunk left there (the first trip is modelled as
    correct: the fault then shows at two or more trips only); uninitialised LDS of the slot fault is modelled as zero."""
    X, K = c['X'], c['K']
    N, P = X.shape
    Km = K - 1
    Uc = c['beta'] if mode == GRAD else c['V']
    G, nch = grid(N), n_chunks(N)
    wpad = np.concatenate([c['w'], np.zeros(SM_ROWS * G * trips(N) + 64)])
    ypad = np.concatenate([c['y'], np.zeros(SM_ROWS * G * trips(N) + 64, dtype=c['y'].dtype)])
    if mut == 'phantom row weighted':
        wpad[N:] = c['w'][N - 1] if c['w'][N - 1] != 0 else 1.0
        ypad[N:] = c['y'][N - 1]
    ppad = None
    if mode == HVP:
        ppad = np.concatenate([p_in, np.zeros((SM_ROWS * G * trips(N) + 64, Km))])
        if mut == 'phantom row weighted':
            ppad[N:] = p_in[N - 1]
    Rpart = np.zeros((G, Km, P))
    vacc = np.zeros((G, 4))
    p_out = np.zeros((N, Km))
    lanes = np.arange(16)
    prev = None
    for t in range(trips(N)):
        ch = t * G + np.arange(G)
        live = ch < nch
        rows = ch[:, None] * SM_ROWS + np.arange(SM_ROWS)
        Xc = X[np.minimum(rows, N - 1)]
        wc, yc = wpad[np.minimum(rows, wpad.size - 1)], ypad[np.minimum(rows, wpad.size - 1)]
        pc = ppad[np.minimum(rows, wpad.size - 1)] if mode == HVP else None
        T = _wave_dot(Xc, Uc, P, nw)                            # G x 8 x Km
        cur = dict(w=wc, y=yc, p=pc, T=T)
        if prev is not None:
            if mut == 'stale weights':
                wc = prev['w']
            if mut == 'stale labels' and mode == GRAD:
                yc = prev['y']
            if mut == 'stale p' and mode == HVP:
                pc = prev['p']
        if mut == 'slot not flipped':
            T = prev['T'] if prev is not None else np.zeros_like(T)
        if mut == 'rows l4 and l4 + 4 swapped':
            if mode == GRAD:
                yc = np.concatenate([yc[:, :4], yc[:, :4]], axis=1)
            else:
                pc = np.concatenate([pc[:, :4], pc[:, :4]], axis=1)
        prev = cur
        T16 = np.zeros(T.shape[:2] + (16,))
        T16[..., :Km] = T
        nact = Km + 1 if (mut == 'lane Km active' and Km < 16 and mode == GRAD) else Km
        act = lanes < nact
        if mode == GRAD:
            with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
                z = np.where(act, T16, -np.inf)
                zm = z if mut == 'm not clamped' else np.maximum(z, 0.0)
                m = _row16(zm, np.maximum)
                e = np.where(act, np.exp(z - m), 0.0)
                s = _row16(e, np.add) + np.exp(-m)
                p = e / s
                hit = act & (lanes == (yc[..., None] - (0 if mut == 'label off by one' else 1)))
                zy = _row16(np.where(hit, z, 0.0), np.add)
                vt = wc * (m[..., 0] + np.log(s[..., 0]) - zy[..., 0])          # G x 8
                mixed = wc[..., None] * (p - hit)
            vt = np.where(live[:, None], vt, 0.0)
            vacc = vacc + vt[:, :4]
            vacc = vacc + vt[:, 4:]
            ok = live[:, None] & (rows < N)
            p_out[rows[ok]] = p[..., :Km][ok]
        else:
            pq = np.zeros_like(T16)
            pq[..., :Km] = pc
            pt = np.where(act, pq * T16, 0.0)
            s = _row16(pt, np.add)
            mixed = np.where(act, wc[..., None] * pq * (T16 - s), 0.0)
        mixed = np.where(live[:, None, None], mixed[..., :Km], 0.0)
        Rpart = Rpart + np.einsum('gra,grp->gap', mixed, Xc)
    out = _reduce_grid(Rpart).ravel()
    if mode == HVP:
        return out
    vpart = (vacc[:, 0] + vacc[:, 2]) + (vacc[:, 1] + vacc[:, 3])
    return _sum_partials(vpart), out, p_out


ROWS_MUTATIONS = ('rows l4 and l4 + 4 swapped', 'label off by one', 'last row dropped')


def f64_influence(c, p, A, n0, n1, nw=4, mut=None):
    """The influence rows in the device's order: T = 1.0 (X A^T) by wave slices, then the sequential contraction over a."""
    X, y = c['X'][n0:n1], c['y'][n0:n1]
    Km, P, Q = c['K'] - 1, c['X'].shape[1], A.shape[0]
    rows = n1 - n0
    M = (1.0 * _wave_dot(X, A.reshape(Q * Km, P), P, nw)).reshape(rows, Q, Km)
    if mut == 'rows l4 and l4 + 4 swapped':
        idx = np.arange(rows)
        sw = idx + np.where(idx % 8 < 4, 4, -4)
        M = M[np.where(sw < rows, sw, idx)]
    out = np.zeros((rows, Q))
    for a in range(Km):
        e = (y == a + (0 if mut == 'label off by one' else 1)).astype(np.float64)
        out = out + (p[n0:n1, a] - e)[:, None] * M[:, :, a]
    if mut == 'last row dropped':
        out[rows - 1] = 0.0
    return out


def max_ratio(got, ref, B):
    return hr.max_ratio(got, ref, scale(B))


# ---- the assertions, shared by the device (tests/test_gpu_softmax_pass.py) and the float64 restatement (the CPU file) -------
class F64Backend(object):
    """The restatement behind the interface the checks use: terms(flags) -> (value, g), hvp(flags), influence(A, n0, n1, flags),
    hessian().  `mut` restates one fault."""

    def __init__(self, c, aligned=True, mut=None):
        self.c, self.aligned, self.mut, self.p = c, aligned, mut, None
        self.P = c['X'].shape[1]

    def _nw(self, mode, flags):
        return dispatch(self.P, self.aligned, mode, flags != 0)[1]

    def terms(self, flags=0):
        val, g, self.p = f64_pass(self.c, GRAD, self._nw(GRAD, flags), mut=self.mut)
        return val, g

    def hvp(self, flags=0):
        if self.p is None:
            self.terms(flags)
        return f64_pass(self.c, HVP, self._nw(HVP, flags), p_in=self.p, mut=self.mut)

    def influence(self, A, n0, n1, flags=0):
        if self.p is None:
            self.terms(flags)
        return f64_influence(self.c, self.p, A, n0, n1, self._nw(ROWS, flags), mut=self.mut if self.mut in ROWS_MUTATIONS else None)

    def hessian(self):
        c = self.c
        X, w, Km = c['X'], c['w'], c['K'] - 1
        P = X.shape[1]
        self.terms()
        H = np.empty((Km * P, Km * P))
        for a in range(Km):
            for b in range(Km):
                col = w * self.p[:, a] * ((1.0 if a == b else 0.0) - self.p[:, b])
                H[a * P:(a + 1) * P, b * P:(b + 1) * P] = (X.T * col) @ X
        return H

    def close(self):
        pass


def assert_exact(got, want, label):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, '{}: shape {} against {}'.format(label, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    first = tuple(int(i) for i in bad[0])
    raise AssertionError('{}: {} of {} entries differ; first {}: got {!r}, want {!r}'.format(
        label, len(bad), got.size, first, got[first], want[first]))


def assert_bounded(got, ref, B, label, ratios=None):
    """Every entry: |got - ref| <= 1.01 2^-53 B.  Records the worst ratio under the label's first word."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, '{}: shape {} against {}'.format(label, got.shape, ref.shape)
    entry, ratio = worst_entry(np.atleast_1d(got), np.atleast_1d(ref), np.atleast_1d(scale(B)))
    if ratios is not None:
        key = label.split()[0]
        ratios[key] = max(ratios.get(key, 0.0), ratio)
    assert ratio <= 1.0, '{}: entry {} is {:.3g} x its bound'.format(label, entry, ratio)


def exact_value_bound(c, N):
    """(reference, bound in units of U) of the value on the exact design: the saturated rows' terms are exact integers, a
    uniform row's is w log K with s = K exactly (rel(s) = 4 + 5: its exp(0) terms are exact, the count is kept), the log at
    E, the addition m + log s, the subtraction of z_y = 0 and the product by w; then the accumulation over all terms."""
    K, kind, w, y = c['K'], c['kind'], c['w'], c['y']
    Km = K - 1
    sat = np.where(kind == 1, 1000.0 * Km - 1000.0 * y, np.where(kind == -1, 1000.0 * y, 0.0))
    lk = np.log(LD(K))
    terms = to_ld(w) * np.where(kind == 0, lk, to_ld(sat))
    mag = float(np.abs(terms).sum())
    uni = float(np.sum(np.abs(w[kind == 0])))
    B = uni * (9.0 + (E_ULP + 3.0) * float(lk)) + (2 * trips(N) + 6 + 8 + ref_units(N) + 1.0) * mag
    return terms.sum(), B * (1.0 + 1e-9)


def check_exact_case(make, N, P, K, aligned=True, Q=3):
    """All three modes on the exact design, bitwise, with every wave flag that changes the instance; p of every row through
    the unit probes; the value bounded on the mixed design and bitwise on the saturated-only variant."""
    c = exact_case(N, P, K, Q)
    e = exact_outputs(c)
    vref, vB = exact_value_bound(c, N)
    E = onehot(c['y'], K - 1)
    be = make(c, aligned)
    label = 'exact N {} P {} K {} aligned {}'.format(N, P, K, aligned)
    try:
        for f in wave_flags(P, aligned):
            lf = '{} flags {}'.format(label, f)
            val, g = be.terms(f)
            assert_exact(g, e['g'], 'gradient ' + lf)
            assert_bounded(val, vref, vB, 'value ' + lf)
            assert_exact(be.hvp(f), e['hv'], 'product ' + lf)
            assert_exact(be.influence(c['A'], 0, N, f), e['infl'], 'influence ' + lf)
            if P >= 2:
                assert_exact(be.influence(unit_probes(P, K - 1), 0, N, f), e['p'] - E, 'p of every row ' + lf)
    finally:
        be.close()
    cs = exact_case(N, P, K, Q, saturated_only=True)
    es = exact_outputs(cs)
    be = make(cs, aligned)
    try:
        for f in wave_flags(P, aligned):
            val, g = be.terms(f)
            assert val == es['value_sat'], 'value (saturated rows only) {} flags {}: got {!r}, want {!r}'.format(label, f, val, es['value_sat'])
            assert_exact(g, es['g'], 'gradient (saturated rows only) {} flags {}'.format(label, f))
            assert_exact(be.hvp(f), es['hv'], 'product (saturated rows only) {} flags {}'.format(label, f))
    finally:
        be.close()


def check_real_case(make, N, P, K, aligned=True, Q=3):
    """All three modes on real data, every entry inside its bound, with every wave flag that changes the instance; p of every
    row through the unit probes under the bound on p.  Returns the worst ratios {value, gradient, product, influence, p}.
    The bounds count the waves of the instances with the flag clear (the four-wave instances gather fewer tiles)."""
    c = real_case(N, P, K, Q)
    ref = ld_eval(c)
    Km = K - 1
    bnd = bounds(c, ref, dispatch(P, aligned, GRAD)[1], dispatch(P, aligned, HVP)[1])
    iref, pe, M = ld_influence(c, ref, c['A'], 0, N)
    iB = influence_bound(c, bnd, pe, M, c['A'], 0, N, dispatch(P, aligned, ROWS)[1])
    peE = ref['p'] - to_ld(onehot(c['y'], Km))
    pB = bnd['p'] + 2.0 * np.abs(f64(peE)) * (1.0 + 1e-9)
    ratios = {}
    be = make(c, aligned)
    label = 'real N {} P {} K {} aligned {}'.format(N, P, K, aligned)
    try:
        for f in wave_flags(P, aligned):
            lf = '{} flags {}'.format(label, f)
            val, g = be.terms(f)
            assert_bounded(val, ref['value'], bnd['value'], 'value ' + lf, ratios)
            assert_bounded(g, ref['g'], bnd['g'], 'gradient ' + lf, ratios)
            assert_bounded(be.hvp(f), ref['hv'], bnd['hv'], 'product ' + lf, ratios)
            assert_bounded(be.influence(c['A'], 0, N, f), iref, iB, 'influence ' + lf, ratios)
            if P >= 2:
                assert_bounded(be.influence(unit_probes(P, Km), 0, N, f), peE, pB, 'p of every row ' + lf, ratios)
    finally:
        be.close()
    return ratios


def exact_k(K):
    """The power of two the exact oracle runs at beside a real-data K."""
    return min(k for k in K_EXACT if k >= min(K, 16))


def check_influence_windows(make, P, K, Q):
    """The influence rows at N = 4099 over windows on and off the chunk grid, exact (at the power of two beside K) and
    bounded, with every wave flag that changes the instance."""
    N = INFL_N
    ratios = {}
    Ke = exact_k(K)
    c = exact_case(N, P, Ke, Q)
    e = exact_outputs(c)
    be = make(c, True)
    try:
        for f in wave_flags(P):
            for (n0, n1) in INFL_WINDOWS:
                assert_exact(be.influence(c['A'], n0, n1, f), e['infl'][n0:n1], 'influence exact P {} K {} Q {} window ({}, {}) flags {}'.format(P, Ke, Q, n0, n1, f))
    finally:
        be.close()
    c = real_case(N, P, K, Q)
    ref = ld_eval(c, want=(GRAD,))
    bnd = bounds(c, ref, dispatch(P, True, GRAD)[1])
    iref, pe, M = ld_influence(c, ref, c['A'], 0, N)
    iB = influence_bound(c, bnd, pe, M, c['A'], 0, N, dispatch(P, True, ROWS)[1])
    be = make(c, True)
    try:
        for f in wave_flags(P):
            for (n0, n1) in INFL_WINDOWS:
                assert_bounded(be.influence(c['A'], n0, n1, f), iref[n0:n1], iB[n0:n1],
                               'influence real P {} K {} Q {} window ({}, {}) flags {}'.format(P, K, Q, n0, n1, f), ratios)
    finally:
        be.close()
    return ratios


def check_hessian(make, N, P, K):
    """The Hessian on the exact design, bitwise: the weight columns, the placement of block (a, b) at (a P, b P), its mirror
    and the batch boundary (K = 16: 120 blocks in batches of 64 and 56 where the batched route runs)."""
    c = exact_case(N, P, K)
    be = make(c, True)
    try:
        H = be.hessian()
    finally:
        be.close()
    want = exact_hessian(c)
    if not np.array_equal(H, want):
        Km = K - 1
        bad = [(a, b) for a in range(Km) for b in range(Km)
               if not np.array_equal(H[a * P:(a + 1) * P, b * P:(b + 1) * P], want[a * P:(a + 1) * P, b * P:(b + 1) * P])]
        raise AssertionError('Hessian N {} P {} K {}: {} of {} blocks differ, first {}'.format(N, P, K, len(bad), Km * Km, bad[:6]))


def _dedupe(cases):
    return list(dict.fromkeys(cases))


REAL_CASES, EXACT_CASES = _dedupe(REAL_CASES), _dedupe(EXACT_CASES)

// k_glmm_walk.h -- what every mixed-model kernel that walks the rows shares (DESIGN.md sections 27, 31 and 33): the tile size, the
// likelihood policies, the head of a tile of group-sorted rows (gs_stage_sorted_tile), the destination of a flushed segment
// (gs_flush_dst) and the grid of every walk (glmm_grid).  Included by k_glmm.hip (the random intercept: its own three kernels over
// the rows, on LogisticLik) and by k_glmm_slopes.hip (K <= 4 effects per group: the three walks templated over the policy).
// glmm_fixup_kernel and glmm_num_tiles keep their ONE definition in k_glmm.hip (a
// __global__ function in a header would be compiled into both code objects); k_kernels.h and lrvb_internal.h declare them.
#pragma once
#include "lrvb_internal.h"
#include "k_kernels.h"
#include <math.h>

constexpr int GLMM_T = 64;               // sorted rows per tile, for every walk, glmm_fixup_kernel and glmm_num_tiles

// ---- what the likelihood policies share ------------------------------------------------------------------------
// Neither infl nor moments is handed its row: in every kernel the four lanes of staged row r are the threads 4 r .. 4 r + 3.
__device__ __forceinline__ int gs_lane_row() { return (int)(threadIdx.x >> 2); }

// The Gauss-Hermite walk of a row: the four lanes of a row share the nodes, lane q4 takes the nodes q4, q4 + 4, .. of the tables
// q.sx, q.sw (LogisticLik::Lds) at t = rho + sqrt(max(s, 0)) x_k and hands (t, w_k) to f.  f accumulates in expressions of its
// own -- its sums, and how they contract, belong to the policy.  A lane that is not `on` (a dead row of the tile; an observed row of
// the censored policy) walks nothing and keeps its zeros.
template <class Q, class F>
__device__ __forceinline__ void gh_nodes(const Q& q, int nq, bool on, int q4, double rho, double s, F f)
{
    if (on) {
        const double sd = sqrt(fmax(s, 0.0));
        for (int k = q4; k < nq; k += 4) f(rho + sd * q.sx[k], q.sw[k]);
    }
}

// The N accumulators of a lane summed over the four lanes of its row, on all four: two xor shuffles in fixed order, no atomics.
// Stands outside every branch on the row's data, so that a quad never diverges around it.
template <int N>
__device__ __forceinline__ void gh_lane_sum(double* e)
{
#pragma unroll
    for (int off = 1; off <= 2; off <<= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) e[i] += __shfl_xor(e[i], off);
}
// the pair of an influence walk, which its caller holds in two variables
__device__ __forceinline__ void gh_lane_sum(double& e1, double& e2)
{
    double e[2] = {e1, e2};
    gh_lane_sum<2>(e);
    e1 = e[0]; e2 = e[1];
}

// The two coefficient layouts.  `kind` names one of the five coefficients: 0 = a1, 1 = a2, 2 = c11, 3 = c12, 4 = c22.
// Five rows, one per coefficient: every policy that integrates on the nodes.
struct FiveRowLayout {
    static constexpr int NCF = 5, NB = 4, DK = 16;
    static constexpr bool HAS_FACTOR = false;
    static __device__ __forceinline__ int cf_row(int kind) { return kind; }
    static __device__ __forceinline__ double cf_factor(int) { return 1.0; }                      // HAS_FACTOR is false: no flush multiplies by it
    static __device__ __forceinline__ int o_d(int b, int k, int Kz) { return b * Kz + k; }
    static __device__ __forceinline__ int d_stride(int) { return DK; }
};
// Two rows [a1 | h], every other coefficient a multiple cf_factor(kind) of h: the closed forms.  cf_factor is the policy's own.
struct TwoRowLayout {
    static constexpr int NCF = 2, NB = 2, DK = 8;
    static constexpr bool HAS_FACTOR = true;
    static __device__ __forceinline__ int cf_row(int kind) { return kind == 0 ? 0 : 1; }
    static __device__ __forceinline__ int o_d(int b, int k, int Kz) { return (b & 1) * Kz + k; }
    static __device__ __forceinline__ int d_stride(int Kz) { return 2 * Kz; }
};

// ---- the likelihood policies -------------------------------------------------------------------------------------------------------
struct LogisticLik : FiveRowLayout {
    struct Args { const double* gx; const double* gw; int nq; };         // Gauss-Hermite nodes and weights (device), 1 <= nq <= 128
    struct Lds { double sx[128], sw[128]; };                             // sqrt(2) x_k, w_k / sqrt(pi)
    struct Moments { double v, e1, e2, e3, e4; };
    static constexpr const char* LIMITS = "logistic mixed model with slopes: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return a.nq >= 1 && a.nq <= 128; }

    static __device__ __forceinline__ void init(Lds& L, const Args& a, int tid)
    {
        const double r2 = 1.4142135623730951, ispi = 0.5641895835477563;     // sqrt(2), 1 / sqrt(pi)
        if (tid < a.nq) { L.sx[tid] = r2 * a.gx[tid]; L.sw[tid] = ispi * a.gw[tid]; }
    }
    static __device__ __forceinline__ void stage_row(Lds&, const Args&, int, bool, i64) {}
    static __device__ __forceinline__ double row_shift(const Lds&, int) { return 0.0; }
    // e1 = psi_rho and e2 = E g2 = 2 psi_s (gi_psi_derivs of k_glmm.hip and gsi_psi_derivs of k_glmm_slopes.hip end in it)
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        e1 = 0.0; e2 = 0.0;
        gh_nodes(L, a.nq, live, q4, rho, s, [&](double t, double wk) {
            const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
            const double sg = t >= 0.0 ? ie : e * ie;
            e1 += wk * sg; e2 += wk * e * ie * ie;
        });
        gh_lane_sum(e1, e2);
    }
    // What the walk asks of a canonical likelihood: the influence kernels subtract y from e1, and the
    // response-scale mean of the predict walk is infl's e1.
    static constexpr bool MINUS_Y = true;
    static __device__ __forceinline__ void mean(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& mu)
    {
        double e2;
        infl(L, a, o, live, q4, rho, s, mu, e2);
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        gh_nodes(L, a.nq, live, q4, rho, s, [&](double t, double wk) {
            const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
            const double sp = (t > 0.0 ? t : 0.0) + log1p(e);
            const double sg = t >= 0.0 ? ie : e * ie;
            const double g2 = e * ie * ie;
            const double om = (1.0 - e) * ie;                            // |1 - 2 sigma|
            const double g3 = t >= 0.0 ? -g2 * om : g2 * om;
            m[0] += wk * sp; m[1] += wk * sg; m[2] += wk * g2; m[3] += wk * g3; m[4] += wk * g2 * (1.0 - 6.0 * g2);
        });
        gh_lane_sum<5>(m);
        return {m[0], m[1], m[2], m[3], m[4]};
    }
    static __device__ __forceinline__ double coefs(const Lds&, int, const Moments& mo, double wi, double yi, double rho, double,
                                                   double* k)
    {
        k[0] = wi * (mo.e1 - yi); k[1] = wi * 0.5 * mo.e2; k[2] = wi * mo.e2; k[3] = wi * 0.5 * mo.e3; k[4] = wi * 0.25 * mo.e4;
        return wi * (mo.v - yi * rho);
    }
};

// A policy that integrates on LogisticLik's nodes next to staged per-row data: its Args and its Lds begin with the node tables `q`.
struct NodeTableLik : FiveRowLayout {
    typedef LogisticLik::Moments Moments;
    template <class L, class A>
    static __device__ __forceinline__ void init(L& l, const A& a, int tid) { LogisticLik::init(l.q, a.q, tid); }
    // The coefficients of a likelihood that is not canonical, by Stein's identity from its finished moments (E H, E H', .. E H''''):
    // no "- y rho" and no "- y", y sits inside H.  A canonical one delegates to LogisticLik::coefs.
    static __device__ __forceinline__ double stein_coefs(const Moments& mo, double wi, double* k)
    {
        k[0] = wi * mo.e1; k[1] = wi * 0.5 * mo.e2; k[2] = wi * mo.e2; k[3] = wi * 0.5 * mo.e3; k[4] = wi * 0.25 * mo.e4;
        return wi * mo.v;
    }
};

struct PoissonLik : TwoRowLayout {
    typedef const double* __restrict__ Args;                             // the per-row offset (device, original row order) or nullptr
    struct Lds { double s_off[GLMM_T]; };                                  // the offsets of the tile's rows
    struct Moments {};
    static constexpr const char* LIMITS = "Poisson mixed model: P <= 64, 1 <= K <= 4";
    static bool args_ok(const Args&) { return true; }
    static __device__ __forceinline__ double cf_factor(int kind) { return kind == 4 ? 0.25 : ((kind & 1) ? 0.5 : 1.0); }   // rows [a1 | h]

    static __device__ __forceinline__ void init(Lds&, const Args&, int) {}
    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a && live) ? a[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }
    static __device__ __forceinline__ void infl(const Lds&, const Args&, double o, bool live, int, double rho, double s, double& e1,
                                                double& e2)
    {
        e1 = e2 = live ? exp((rho + o) + 0.5 * s) : 0.0;
    }
    // canonical: see LogisticLik
    static constexpr bool MINUS_Y = true;
    static __device__ __forceinline__ void mean(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& mu)
    {
        double e2;
        infl(L, a, o, live, q4, rho, s, mu, e2);
    }
    static __device__ __forceinline__ Moments moments(const Lds&, const Args&, bool, int, double, double) { return {}; }
    static __device__ __forceinline__ double coefs(const Lds& L, int row, const Moments&, double wi, double yi, double rho, double s,
                                                   double* k)
    {
        rho += L.s_off[row];
        const double psi = exp(rho + 0.5 * s);
        const double h = wi * psi;
        k[0] = h - wi * yi; k[1] = h;
        return wi * (psi - yi * rho);
    }
};

// Binomial with a per-row trial count m_n and a per-row offset o_n: the logistic quadrature at rho + o, its
// finished moments times m_n.  The data term is sum w [m E softplus(t) - y rho], t ~ N(rho, s), rho including the offset; with
// m = y + phi and the offset o - log phi it is the negative binomial (NB2) term for a known dispersion phi.  Nodes AND staged
// per-row data: the node tables and init are LogisticLik's, the staging is PoissonLik's with a second array.  The coefficient
// layout is the logistic one.  m = 1 and o = 0 (either pointer null, or the values themselves) give the logistic instantiation
// bit for bit: x * 1.0 and x + 0.0 are exact, and the products with m are kept out of every fused multiply-add, so that the
// sums behind them are contracted as LogisticLik's are.
struct BinomialLik : NodeTableLik {
    struct Args { LogisticLik::Args q; const double* __restrict__ off; const double* __restrict__ trials; };   // either may be nullptr
    struct Lds { LogisticLik::Lds q; double s_off[GLMM_T], s_m[GLMM_T]; };   // the node tables; the offsets and trials of the tile's rows
    static constexpr const char* LIMITS = "binomial mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q); }

    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a.off && live) ? a.off[src] : 0.0;
        L.s_m[t] = (a.trials && live) ? a.trials[src] : 1.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        const double mt = L.s_m[gs_lane_row()];
        LogisticLik::infl(L.q, a.q, 0.0, live, q4, rho + o, s, e1, e2);
        {
#pragma clang fp contract(off)
            e1 = e1 * mt; e2 = e2 * mt;
        }
    }
    // canonical: see LogisticLik
    static constexpr bool MINUS_Y = true;
    static __device__ __forceinline__ void mean(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& mu)
    {
        double e2;
        infl(L, a, o, live, q4, rho, s, mu, e2);
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double mt = L.s_m[row];
        Moments mo = LogisticLik::moments(L.q, a.q, live, q4, rho + L.s_off[row], s);
        {
#pragma clang fp contract(off)
            mo.v = mo.v * mt; mo.e1 = mo.e1 * mt; mo.e2 = mo.e2 * mt; mo.e3 = mo.e3 * mt; mo.e4 = mo.e4 * mt;
        }
        return mo;
    }
    static __device__ __forceinline__ double coefs(const Lds& L, int row, const Moments& mo, double wi, double yi, double rho, double s,
                                                   double* k)
    {
        return LogisticLik::coefs(L.q, row, mo, wi, yi, rho + L.s_off[row], s, k);
    }
};

// Binomial with a probit or a complementary log-log link: p = Phi(t) or p = 1 - exp(-e^t).  The first
// likelihoods here that are not canonical: with h1 = -log p, h0 = -log(1 - p) the row's term is E [y h1(t) + (m - y) h0(t)],
// t ~ N(rho, s), rho including the offset -- no "- y rho", success and failure with curvatures of their own, and a response mean
// that is not psi_rho.  So MINUS_Y is false (infl returns a1' = y E h1' + (m - y) E h0' whole) and `mean` is a function of its
// own.  Nodes, offsets and trials are staged as BinomialLik stages them, y from the same ORIGINAL row index behind them (a null
// y -- the predict walk, which needs none -- stages zeros).  Coefficients by Stein's identity on the nodes, in the logistic
// five-row layout:  value = E H, a1 = E H', a2 = E H'' / 2, c11 = E H'', c12 = E H''' / 2, c22 = E H'''' / 4  (times w).
//   probit   h1' = -lambda, lambda = phi / Phi = sqrt(2 / pi) / erfcx(-t / sqrt 2) (never phi / Phi: 0 / 0 below t = -38), and with
//            d = t + lambda, w = lambda d:  h1'' = w,  h1''' = w' = lambda (1 - w) - w d,  h1'''' = -w' (d + lambda) - 2 w (1 - w).
//            erfcx overflows to +inf for large t: lambda = 0 and every derivative is 0, no branch on data.  h0(t) = h1(-t): the
//            same rule at -t, odd derivatives negated.  -log Phi: t^2 / 2 - log(erfcx(-t / sqrt 2) / 2) for t < 0,
//            -log1p(-erfc(t / sqrt 2) / 2) for t >= 0.
//   cloglog  u = e^t, r = u / expm1(u):  h1' = -r,  r' = r q with q = 1 - u - r,  q' = -u - r', and so on by the product rule.
//            Past u = 700 (r < 1e-301) r is set to 0 and u to 700 in the polynomials, a select: u = +inf gives exact zeros, not
//            inf / inf.  h1 = -log(-expm1(-u)) up to u = log 2, -log1p(-exp(-u)) past it.  h0 = u EXACTLY integrable: E h0 and all its derivatives are exp(rho + s / 2), one
//            exp per row as in PoissonLik and not clamped -- where it overflows the non-finite value reaches the sums and the
//            entry refuses it.  Below t = -745 (u = 0) r is 0 / 0 and the row is refused in the same way.
// The products with y and m - y are formed per lane, inside the node function.
constexpr int GLMM_LINK_LOGIT = 0, GLMM_LINK_PROBIT = 1, GLMM_LINK_CLOGLOG = 2;     // LRVB_LINK_* of the C ABI

template <int LINK>
struct BinomialLinkLik : NodeTableLik {
    static_assert(LINK == GLMM_LINK_PROBIT || LINK == GLMM_LINK_CLOGLOG, "the logit link is BinomialLik");
    struct Args { LogisticLik::Args q; const double* __restrict__ off; const double* __restrict__ trials; const double* __restrict__ y; };
    struct Lds { LogisticLik::Lds q; double s_off[GLMM_T], s_m[GLMM_T], s_y[GLMM_T]; };
    static constexpr const char* LIMITS = "binomial mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q); }
    static constexpr bool MINUS_Y = false;

    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a.off && live) ? a.off[src] : 0.0;
        L.s_m[t] = (a.trials && live) ? a.trials[src] : 1.0;
        L.s_y[t] = (a.y && live) ? a.y[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }

    // Probit, left tail: below t = PROBIT_CF_BELOW the sum d = t + lambda cancels to -1 / t and carries t^2 times the error of erfcx, and
    // 1 - w and w' behind it t^4 times.  There d comes from the continued fraction sqrt(2 / pi) / erfcx(x) = sqrt 2 (x + K(x)),
    // K = (1/2) / (x + (2/2) / (x + (3/2) / (x + ..))), x = -t / sqrt 2: d = sqrt 2 K(x) without a cancellation and lambda = d - t.
    // PROBIT_CF_TERMS terms (5e-16 of K at x = 3.5) from the tail as one ratio cn / cd -- one division; past x = 1e8, where cd would
    // overflow, K = 1 / (2 x) to the last bit.  The cancellations of 1 - w and of w' themselves stay.
    static constexpr double PROBIT_CF_BELOW = -5.0;
    static constexpr int PROBIT_CF_TERMS = 24;

    // h1' and h1'' at t (N = 2), or h1 .. h1'''' (N = 5), into h[5 - N ..]: h[0] is the value wherever it is asked for
    template <int N>
    static __device__ __forceinline__ void h1(double t, double* h)
    {
        if constexpr (LINK == GLMM_LINK_PROBIT) {
            const double ex = erfcx(-0.7071067811865476 * t);
            double lam = 0.7978845608028654 / ex;                        // sqrt(2 / pi) / erfcx(-t / sqrt 2)
            double d = t + lam;
            if (t < PROBIT_CF_BELOW) {                                   // d = sqrt 2 K(x) from the continued fraction, lambda = d - t (above)
                const double x0 = -0.7071067811865476 * t, x = fmin(x0, 1e8);
                double cn = 0.5 * PROBIT_CF_TERMS, cd = x;
#pragma unroll
                for (int k = PROBIT_CF_TERMS - 1; k >= 1; --k) { const double nn = (0.5 * k) * cd; cd = x * cd + cn; cn = nn; }
                d = 1.4142135623730951 * (x0 > 1e8 ? 0.5 / x0 : cn / cd);
                lam = d - t;
            }
            const double w = lam * d;
            h[1] = -lam; h[2] = w;
            if constexpr (N == 5) {
                const double w1 = lam * (1.0 - w) - w * d;
                h[3] = w1; h[4] = -w1 * (d + lam) - 2.0 * w * (1.0 - w);
                if (t < 0.0) h[0] = 0.5 * t * t - log(0.5 * ex);
                else h[0] = -log1p(-0.5 * erfc(0.7071067811865476 * t));
            }
        } else {
            const double u = exp(t), uc = fmin(u, 700.0);
            const double r = u > 700.0 ? 0.0 : uc / expm1(uc);
            const double q = 1.0 - uc - r, r1 = r * q;
            h[1] = -r; h[2] = -r1;
            if constexpr (N == 5) {
                const double q1 = -uc - r1, r2 = r1 * q + r * q1, q2 = -uc - r2;
                h[3] = -r2; h[4] = -(r2 * q + 2.0 * r1 * q1 + r * q2);
                // past u = log 2 through log1p(-e^-u): 1 - e^-u rounds to 1 from u = 37 on and -log of it would lose e^-u whole
                h[0] = u > 0.6931471805599453 ? -log1p(-exp(-u)) : -log(-expm1(-u));
            }
        }
    }
    // a1' = y E h1' + (m - y) E h0' and E H'' = 2 a2' per unit weight, on all four lanes of a row
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        const int row = gs_lane_row();
        const double yt = L.s_y[row], ft = L.s_m[row] - yt;
        rho += o;
        e1 = 0.0; e2 = 0.0;
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double h[5];
            h1<2>(t, h);
            double g1 = yt * h[1], g2 = yt * h[2];
            if constexpr (LINK == GLMM_LINK_PROBIT) {
                h1<2>(-t, h);
                g1 -= ft * h[1]; g2 += ft * h[2];
            }
            e1 += wk * g1; e2 += wk * g2;
        });
        gh_lane_sum(e1, e2);
        if constexpr (LINK == GLMM_LINK_CLOGLOG) {
            const double eh = live ? ft * exp(rho + 0.5 * s) : 0.0;
            e1 += eh; e2 += eh;
        }
    }
    // the response-scale mean m p: probit in closed form, E Phi(t) = Phi(rho / sqrt(1 + s)); cloglog on the nodes
    static __device__ __forceinline__ void mean(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& mu)
    {
        const double mt = L.s_m[gs_lane_row()];
        rho += o;
        if constexpr (LINK == GLMM_LINK_PROBIT) {
            mu = live ? mt * (0.5 * erfc(-rho / sqrt(2.0 * (1.0 + fmax(s, 0.0))))) : 0.0;
        } else {
            double p = 0.0;
            gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) { p += wk * -expm1(-exp(t)); });
            gh_lane_sum<1>(&p);
            mu = mt * p;
        }
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double yt = L.s_y[row], ft = L.s_m[row] - yt;
        rho += L.s_off[row];
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double h[5], g[5];
            h1<5>(t, h);
#pragma unroll
            for (int i = 0; i < 5; ++i) g[i] = yt * h[i];
            if constexpr (LINK == GLMM_LINK_PROBIT) {
                h1<5>(-t, h);
#pragma unroll
                for (int i = 0; i < 5; ++i) g[i] += ft * ((i & 1) ? -h[i] : h[i]);
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] += wk * g[i];
        });
        gh_lane_sum<5>(e);
        if constexpr (LINK == GLMM_LINK_CLOGLOG) {
            const double eh = live ? ft * exp(rho + 0.5 * s) : 0.0;
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] += eh;
        }
        return {e[0], e[1], e[2], e[3], e[4]};
    }
    static __device__ __forceinline__ double coefs(const Lds&, int, const Moments& mo, double wi, double, double, double, double* k)
    {
        return stein_coefs(mo, wi, k);
    }
};

// Zero-truncated Poisson with a per-row offset: y in {1, 2, ..}, P(y | t) = e^{y t - u} / (y! (1 - e^{-u})),
// u = e^t -- the count part of a hurdle model.  Canonical in t: -log P = A(t) - y t + log y! with the log-partition
//   A(t) = log(e^u - 1) = u + log(-expm1(-u)),   A' = u + r (the response mean u / (1 - e^{-u})),   A^(k) = u + r^(k-1),  k >= 1,
// r = u / expm1(u) and its derivatives by the recurrences of BinomialLinkLik<CLOGLOG>::h1 (A = e^t - h1 of that link).  The data
// term is sum w [E A(t) - y rho], t ~ N(rho, s), rho including the offset; coefficients by Stein's identity in the logistic five-row
// layout, as LogisticLik::coefs forms them:
//   value = w (E A - y rho),  a1 = w (E A' - y),  a2 = w E A'' / 2,  c11 = w E A'',  c12 = w E A''' / 2,  c22 = w E A'''' / 4.
// The e^t part of every E A^(k) is exp(rho + s / 2) EXACTLY: one exp per row, added behind the shuffles and not clamped -- where it
// overflows the non-finite value reaches the sums and the entry refuses it, as for PoissonLik.  Only log(-expm1(-u)) and r^(k-1) go
// on the nodes.  Past u = 700 (r < 1e-301) r is set to 0 and u
// to 700 in the polynomials, a select; below t = -745 (u = 0) r is 0 / 0 and the row is refused in the same way.  Nodes AND a
// staged offset, no trials, and y from the walk (MINUS_Y): the response mean E A' is infl's e1.
struct TruncPoissonLik : NodeTableLik {
    struct Args { LogisticLik::Args q; const double* __restrict__ off; };                      // off may be nullptr
    struct Lds { LogisticLik::Lds q; double s_off[GLMM_T]; };               // the node tables; the offsets of the tile's rows
    static constexpr const char* LIMITS = "zero-truncated Poisson mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q); }
    static constexpr bool MINUS_Y = true;

    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a.off && live) ? a.off[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }

    // The node parts of A' and A'' at t (N = 2), or of A .. A'''' (N = 5), into g[5 - N ..]: g[0] = log(-expm1(-u)), g[k] = r^(k-1)
    template <int N>
    static __device__ __forceinline__ void node(double t, double* g)
    {
        const double u = exp(t), uc = fmin(u, 700.0);
        const double r = u > 700.0 ? 0.0 : uc / expm1(uc);
        const double q = 1.0 - uc - r, r1 = r * q;
        g[1] = r; g[2] = r1;
        if constexpr (N == 5) {
            const double q1 = -uc - r1, r2 = r1 * q + r * q1, q2 = -uc - r2;
            g[3] = r2; g[4] = r2 * q + 2.0 * r1 * q1 + r * q2;
            g[0] = log(-expm1(-u));
        }
    }
    // e1 = E A' (the response mean; the walk subtracts y) and e2 = E A'' = 2 psi_s, on all four lanes of a row
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        rho += o;
        e1 = 0.0; e2 = 0.0;
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double g[5];
            node<2>(t, g);
            e1 += wk * g[1]; e2 += wk * g[2];
        });
        gh_lane_sum(e1, e2);
        const double eu = live ? exp(rho + 0.5 * s) : 0.0;
        e1 += eu; e2 += eu;
    }
    static __device__ __forceinline__ void mean(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& mu)
    {
        double e2;
        infl(L, a, o, live, q4, rho, s, mu, e2);
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        rho += L.s_off[gs_lane_row()];
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double g[5];
            node<5>(t, g);
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] += wk * g[i];
        });
        gh_lane_sum<5>(e);
        const double eu = live ? exp(rho + 0.5 * s) : 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) e[i] += eu;
        return {e[0], e[1], e[2], e[3], e[4]};
    }
    static __device__ __forceinline__ double coefs(const Lds& L, int row, const Moments& mo, double wi, double yi, double rho, double s,
                                                   double* k)
    {
        return LogisticLik::coefs(L.q, row, mo, wi, yi, rho + L.s_off[row], s, k);
    }
};

// Zero-truncated negative binomial (NB2) with a known per-row dispersion phi and a per-row offset: y in
// {1, 2, ..}, the count part of a hurdle model for over-dispersed counts.  With eta = t - log phi (the staged offset is the SHIFTED
// one, o - log phi), sp = softplus and m = y + phi the row's term is, constants dropped,
//   H(eta) = m sp(eta) - y eta + g(eta),   g = log(1 - exp(-v)),   v = phi sp(eta)      (P(y = 0) = (1 + e^eta)^-phi = exp(-v)):
// the NB2 term of BinomialLik plus the log of 1 - P(0), which couples phi and eta inside a log and so is no binomial term.  The
// data term is sum w [E H(eta)], eta ~ N(rho, s), rho including the shifted offset; coefficients by Stein's identity in the
// logistic five-row layout, as LogisticLik::coefs forms them (MINUS_Y: infl returns e1 = m E sigma + E g', the walk subtracts y):
//   value = w (E[m sp + g] - y rho),  a1 = w (E[m sigma + g'] - y),  a2 = w E H'' / 2,  c11 = w E H'',  c12 = w E H''' / 2,  c22 = w E H'''' / 4.
// g by the chain rule in its FACTORED form, every intermediate O(1) down to eta = -745: with v_k = phi sp^(k), R = 1 / expm1(v),
//   a = v_1 R, b = v_2 R, d = v_3 R, c = v_1 + a           (dR/d eta = -a (1 + R))
//   g' = a,   g'' = b - a c,   b' = d - a (v_2 + b),   c' = v_2 + g'',   g''' = b' - g'' c - a c',
//   d' = v_4 R - a (v_3 + d),   b'' = d' - g'' (v_2 + b) - a (v_3 + b'),   g'''' = b'' - g''' c - 2 g'' c' - a (v_3 + g''').
// In the corner eta < log 1e-3, v < 0.01 the derivatives of order 2 to 4 come from two short series instead (at `node`).
// Past v = 700 (R < 1e-304) R is 0 by a select (the TruncPoissonLik rule): a huge v gives exact zeros, not inf * 0.  Where v
// underflows to 0 (eta below about -745) R is 1 / 0: the non-finite value reaches the sums and the entry refuses the point; no
// clamp.  The response mean of the truncated count is E[mu / (1 - P0)] = E[e^t (1 + R(v))], e^t = phi e^eta: its e^t part is
// phi exp(rho + s / 2) in closed form, one exp per row and not clamped; e^t R(v) goes on the nodes (-> 1 as t -> -inf, 0 by the
// same select).  Nodes, offsets, phi and y are staged as BinomialLinkLik stages offset, trials and y (a null y -- the predict
// walk -- stages zeros); m sp^(k) + g^(k) per node.
struct TruncNegBinLik : NodeTableLik {
    struct Args { LogisticLik::Args q; const double* __restrict__ off; const double* __restrict__ disp; const double* __restrict__ y; };   // off may be nullptr
    struct Lds { LogisticLik::Lds q; double s_off[GLMM_T], s_phi[GLMM_T], s_y[GLMM_T]; };
    static constexpr const char* LIMITS = "zero-truncated negative binomial mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q) && a.disp != nullptr; }
    static constexpr bool MINUS_Y = true;

    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a.off && live) ? a.off[src] : 0.0;
        L.s_phi[t] = live ? a.disp[src] : 1.0;
        L.s_y[t] = (a.y && live) ? a.y[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }

    // 1 / expm1(v), 0 past v = 700 by a select
    static __device__ __forceinline__ double recip_expm1(double v) { return v > 700.0 ? 0.0 : 1.0 / expm1(fmin(v, 700.0)); }

    // The corner eta < log 1e-3 and v < 0.01: there g'', g''', g'''' are O(e^eta) while a, b, c are O(1), and b - a c keeps an absolute
    // error of 2^-53 only -- 1e-3 of g'' at eta = -30.  With x = e^eta, g = log phi + eta + M(eta) + L(v),
    //   M = log(sp / x) = -x / 2 + 5 x^2 / 24 - x^3 / 8 + 251 x^4 / 2880 - 19 x^5 / 288,   L = log((1 - e^-v) / v) = -v / 2 + v^2 / 24 - v^4 / 2880,
    // and every term of g'' = M'' + L'' v_1^2 + L' v_2, g''' = M''' + L''' v_1^3 + 3 L'' v_1 v_2 + L' v_3,
    // g'''' = M'''' + L'''' v_1^4 + 6 L''' v_1^2 v_2 + L'' (3 v_2^2 + 4 v_1 v_3) + L' v_4 has the sign and size of the result.  The terms
    // left out are below 2e-13 (x^6) and 1e-15 (v^6) of it.  Outside the corner the factored form is good to 1e-13 of the result.
    static constexpr double ETA_SMALL = -6.907755278982137, V_SMALL = 0.01;
    // the J-th derivative in eta of M: sum_k c_k k^J x^k
    template <int J>
    static __device__ __forceinline__ double small_m(double x)
    {
        constexpr double p2 = J == 2 ? 4.0 : (J == 3 ? 8.0 : 16.0), p3 = J == 2 ? 9.0 : (J == 3 ? 27.0 : 81.0);
        constexpr double p4 = J == 2 ? 16.0 : (J == 3 ? 64.0 : 256.0), p5 = J == 2 ? 25.0 : (J == 3 ? 125.0 : 625.0);
        return x * (-0.5 + x * (p2 * (5.0 / 24.0) + x * (p3 * (-1.0 / 8.0) + x * (p4 * (251.0 / 2880.0) + x * (p5 * (-19.0 / 288.0))))));
    }

    // H' and H'' at eta = t (N = 2), or H + y eta, H' + y, H'' .. H'''' (N = 5), into h[5 - N ..]; mt = y + phi
    template <int N>
    static __device__ __forceinline__ void node(double t, double phi, double mt, double* h)
    {
        const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
        const double sp = (t > 0.0 ? t : 0.0) + log1p(e);
        const double sg = t >= 0.0 ? ie : e * ie;
        const double g2 = e * ie * ie;
        const double v = phi * sp, R = recip_expm1(v);
        const double v1 = phi * sg, v2 = phi * g2;
        const double a = v1 * R, b = v2 * R, c = v1 + a;
        // the corner (see above): t < 0 there, so e = e^eta
        const bool corner = t < ETA_SMALL && v < V_SMALL;
        const double lp = -0.5 + v * (1.0 / 12.0 - v * v * (1.0 / 720.0)), lpp = 1.0 / 12.0 - v * v * (1.0 / 240.0);
        const double gg2 = corner ? small_m<2>(e) + lpp * v1 * v1 + lp * v2 : b - a * c;
        h[1] = mt * sg + a; h[2] = mt * g2 + gg2;
        if constexpr (N == 5) {
            const double om = (1.0 - e) * ie;                            // |1 - 2 sigma|
            const double g3 = t >= 0.0 ? -g2 * om : g2 * om;
            const double g4 = g2 * (1.0 - 6.0 * g2);
            const double v3 = phi * g3, v4 = phi * g4;
            double gg3, gg4;
            if (corner) {
                const double lppp = v * (-1.0 / 120.0);
                gg3 = small_m<3>(e) + lppp * v1 * v1 * v1 + 3.0 * lpp * v1 * v2 + lp * v3;
                gg4 = small_m<4>(e) - (1.0 / 120.0) * (v1 * v1) * (v1 * v1) + 6.0 * lppp * v1 * v1 * v2 + lpp * (3.0 * v2 * v2 + 4.0 * v1 * v3)
                      + lp * v4;
            } else {
                const double d = v3 * R;
                const double b1 = d - a * (v2 + b), c1 = v2 + gg2;
                gg3 = b1 - gg2 * c - a * c1;
                const double d1 = v4 * R - a * (v3 + d);
                const double b2 = d1 - gg2 * (v2 + b) - a * (v3 + b1);
                gg4 = b2 - gg3 * c - 2.0 * gg2 * c1 - a * (v3 + gg3);
            }
            h[0] = mt * sp + log(-expm1(-v)); h[3] = mt * g3 + gg3; h[4] = mt * g4 + gg4;
        }
    }
    // e1 = m E sigma + E g' (the walk subtracts y) and e2 = E H'' = 2 psi_s, on all four lanes of a row
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], mt = L.s_y[row] + phi;
        rho += o;
        e1 = 0.0; e2 = 0.0;
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double h[5];
            node<2>(t, phi, mt, h);
            e1 += wk * h[1]; e2 += wk * h[2];
        });
        gh_lane_sum(e1, e2);
    }
    // the response mean of the truncated count: phi exp(rho + s / 2) in closed form plus E[e^t R(v)] on the nodes
    static __device__ __forceinline__ void mean(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& mu)
    {
        const double phi = L.s_phi[gs_lane_row()];
        rho += o;
        double p = 0.0;
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            const double e = exp(-fabs(t));
            const double v = phi * ((t > 0.0 ? t : 0.0) + log1p(e));
            p += wk * (v > 700.0 ? 0.0 : phi * exp(t) * recip_expm1(v));
        });
        gh_lane_sum<1>(&p);
        mu = live ? phi * exp(rho + 0.5 * s) + p : 0.0;
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], mt = L.s_y[row] + phi;
        rho += L.s_off[row];
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double h[5];
            node<5>(t, phi, mt, h);
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] += wk * h[i];
        });
        gh_lane_sum<5>(e);
        return {e[0], e[1], e[2], e[3], e[4]};
    }
    static __device__ __forceinline__ double coefs(const Lds& L, int row, const Moments& mo, double wi, double yi, double rho, double s,
                                                   double* k)
    {
        return LogisticLik::coefs(L.q, row, mo, wi, yi, rho + L.s_off[row], s, k);
    }
};

// Beta with a known per-row precision phi and a per-row offset: a proportion y strictly inside (0, 1),
// y ~ Beta(mu phi, (1 - mu) phi), mu = sigma(t).  The staged y is l = logit(y); with it the row's term is, constants dropped,
//   h(t) = lgamma(phi sigma(t)) + lgamma(phi sigma(-t)) - phi l sigma(t).
// Differentiated as it stands that is useless in the tails: psi^(j)(phi mu) ~ (phi mu)^-(j+1) meets mu'^j ~ mu^j and O(1) terms
// cancel to an O(mu) result.  Both arguments are therefore SHIFTED by one, lgamma(x) = lgamma(1 + x) - log x and
// -log sigma(+-t) = softplus(-+t):
//   h(t) = softplus(t) + softplus(-t) - 2 log phi + G(mu),   G(mu) = lgamma(1 + phi mu) + lgamma(1 + phi (1 - mu)) - phi l mu,
// G smooth with every polygamma argument >= 1.  The softplus pair gives |t| + 2 log1p(e), +-|1 - 2 sigma| and 2 sigma', 2 sigma'',
// 2 sigma''' (the g2, g3, g4 of LogisticLik::moments); G goes through Faa di Bruno with
//   G_j = phi^j [psi^(j-1)(1 + phi mu) + (-1)^j psi^(j-1)(1 + phi (1 - mu))] - [j = 1] phi l,
//   mu' = v,  mu'' = v (1 - 2 mu),  mu''' = v (1 - 6 v),  mu'''' = v (1 - 2 mu)(1 - 12 v),  v = mu (1 - mu),
// mu and 1 - mu both from e = exp(-|t|), never 1 - sigma by subtraction.  The data term is sum w E h(t), t ~ N(rho, s), rho
// including the offset; coefficients by Stein's identity in the logistic five-row layout.  Not canonical (the y-dependence sits
// inside h): MINUS_Y is false and coefs ignores the walk's yi, as BinomialLinkLik does.  -2 log phi is added once per row behind
// the shuffles (E of a constant).  NO finite point is refused: as |t| grows e underflows to 0, the arguments become 1 and 1 + phi
// and h grows like |t| -- unlike the Poisson-type policies there is no exp of t that could overflow.  The response mean is
// E sigma(t), the logistic one, whatever phi.  Nodes, offsets, phi and l are staged as TruncNegBinLik stages offset, dispersion and
// y.
struct BetaLik : NodeTableLik {
    struct Args { LogisticLik::Args q; const double* __restrict__ off; const double* __restrict__ disp; const double* __restrict__ y; };   // off may be nullptr; y holds logit(y)
    struct Lds { LogisticLik::Lds q; double s_off[GLMM_T], s_phi[GLMM_T], s_y[GLMM_T]; };
    static constexpr const char* LIMITS = "Beta mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q) && a.disp != nullptr; }
    static constexpr bool MINUS_Y = false;

    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a.off && live) ? a.off[src] : 0.0;
        L.s_phi[t] = live ? a.disp[src] : 1.0;
        L.s_y[t] = (a.y && live) ? a.y[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }

    // lgamma (N = 5 only), psi, psi' (p[1], p[2]) and psi'', psi''' (N = 5: p[3], p[4]) at x >= 1: nine unrolled steps of the
    // recurrence f(x) = f(x + 1) + .. wherever x is still below 10 -- selects, no data-dependent trip count and no indexed
    // array -- and then the Stirling / Bernoulli series to B_16 at z >= 10 (the first term left out is below 3e-17 of the result).
    template <int N>
    static __device__ __forceinline__ void polygamma(double x, double* p)
    {
        double z = x, prod = 1.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const bool lo = z < 10.0;
            const double r = lo ? 1.0 / z : 0.0, r2 = r * r;
            s1 += r; s2 += r2;
            if constexpr (N == 5) { s3 += r2 * r; s4 += r2 * r2; prod *= lo ? z : 1.0; }
            z = lo ? z + 1.0 : z;
        }
        const double w = 1.0 / z, w2 = w * w, lz = log(z);
        // sum_k B_2k w^2k / (2k),  sum_k B_2k w^2k,  sum_k B_2k (2k + 1) w^2k,  sum_k B_2k (2k + 1)(2k + 2) w^2k,  k = 1 .. 8
        p[1] = lz - 0.5 * w - s1
               - w2 * (1.0 / 12.0 + w2 * (-1.0 / 120.0 + w2 * (1.0 / 252.0 + w2 * (-1.0 / 240.0 + w2 * (1.0 / 132.0 + w2 * (-691.0 / 32760.0
                 + w2 * (1.0 / 12.0 + w2 * (-3617.0 / 8160.0))))))));
        p[2] = s2 + w * (1.0 + 0.5 * w
               + w2 * (1.0 / 6.0 + w2 * (-1.0 / 30.0 + w2 * (1.0 / 42.0 + w2 * (-1.0 / 30.0 + w2 * (5.0 / 66.0 + w2 * (-691.0 / 2730.0
                 + w2 * (7.0 / 6.0 + w2 * (-3617.0 / 510.0)))))))));
        if constexpr (N == 5) {
            p[3] = -2.0 * s3 - w2 * (1.0 + w
                   + w2 * (3.0 / 6.0 + w2 * (-5.0 / 30.0 + w2 * (7.0 / 42.0 + w2 * (-9.0 / 30.0 + w2 * (55.0 / 66.0 + w2 * (-13.0 * 691.0 / 2730.0
                     + w2 * (15.0 * 7.0 / 6.0 + w2 * (-17.0 * 3617.0 / 510.0)))))))));
            p[4] = 6.0 * s4 + w2 * w * (2.0 + 3.0 * w
                   + w2 * (12.0 / 6.0 + w2 * (-30.0 / 30.0 + w2 * (56.0 / 42.0 + w2 * (-90.0 / 30.0 + w2 * (660.0 / 66.0
                     + w2 * (-182.0 * 691.0 / 2730.0 + w2 * (240.0 * 7.0 / 6.0 + w2 * (-306.0 * 3617.0 / 510.0)))))))));
            // sum_k B_2k w^(2k-1) / (2k (2k - 1))
            p[0] = (z - 0.5) * lz - z + 0.9189385332046727 - log(prod)
                   + w * (1.0 / 12.0 + w2 * (-1.0 / 360.0 + w2 * (1.0 / 1260.0 + w2 * (-1.0 / 1680.0 + w2 * (1.0 / 1188.0 + w2 * (-691.0 / 360360.0
                     + w2 * (1.0 / 156.0 + w2 * (-3617.0 / 122400.0))))))));
        }
    }

    // h' and h'' at t (N = 2), or h + 2 log phi, h', h'' .. h'''' (N = 5), into h[5 - N ..]; l = logit(y)
    template <int N>
    static __device__ __forceinline__ void node(double t, double phi, double l, double* h)
    {
        const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
        const bool pos = t >= 0.0;
        const double mu = pos ? ie : e * ie, nu = pos ? e * ie : ie;      // sigma(t) and sigma(-t)
        const double g2 = e * ie * ie;                                   // v = mu (1 - mu)
        const double om = (1.0 - e) * ie;                                // |1 - 2 sigma|
        const double d = pos ? -om : om;                                 // 1 - 2 mu
        double pa[5], pb[5];
        polygamma<N>(1.0 + phi * mu, pa);
        polygamma<N>(1.0 + phi * nu, pb);
        const double G1 = phi * ((pa[1] - pb[1]) - l), G2 = phi * phi * (pa[2] + pb[2]);
        const double m1 = g2, m2 = g2 * d;
        h[1] = -d + G1 * m1;
        h[2] = 2.0 * g2 + G2 * m1 * m1 + G1 * m2;
        if constexpr (N == 5) {
            const double p3 = phi * phi * phi;
            const double G3 = p3 * (pa[3] - pb[3]), G4 = p3 * phi * (pa[4] + pb[4]);
            const double g3 = g2 * d, g4 = g2 * (1.0 - 6.0 * g2);         // sigma'' and sigma'''
            const double m3 = g4, m4 = g2 * d * (1.0 - 12.0 * g2);
            h[0] = fabs(t) + 2.0 * log1p(e) + pa[0] + pb[0] - phi * l * mu;
            h[3] = 2.0 * g3 + G3 * m1 * m1 * m1 + 3.0 * G2 * m1 * m2 + G1 * m3;
            h[4] = 2.0 * g4 + G4 * (m1 * m1) * (m1 * m1) + 6.0 * G3 * m1 * m1 * m2 + G2 * (3.0 * m2 * m2 + 4.0 * m1 * m3) + G1 * m4;
        }
    }
    // a1' = E h' and E h'' = 2 a2' per unit weight, on all four lanes of a row
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], l = L.s_y[row];
        rho += o;
        e1 = 0.0; e2 = 0.0;
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double h[5];
            node<2>(t, phi, l, h);
            e1 += wk * h[1]; e2 += wk * h[2];
        });
        gh_lane_sum(e1, e2);
    }
    // the response mean E sigma(t) does not depend on phi: the logistic quadrature at rho + o
    static __device__ __forceinline__ void mean(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& mu)
    {
        double e2;
        LogisticLik::infl(L.q, a.q, 0.0, live, q4, rho + o, s, mu, e2);
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], l = L.s_y[row];
        rho += L.s_off[row];
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double h[5];
            node<5>(t, phi, l, h);
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] += wk * h[i];
        });
        gh_lane_sum<5>(e);
        return {live ? e[0] - 2.0 * log(phi) : 0.0, e[1], e[2], e[3], e[4]};
    }
    static __device__ __forceinline__ double coefs(const Lds&, int, const Moments& mo, double wi, double, double, double, double* k)
    {
        return stein_coefs(mo, wi, k);
    }
};

// Gamma with a log link, a per-row shape phi and a per-row offset: y > 0, mean mu = e^t, the row's term,
// constants dropped,
//   h(t) = phi (y e^{-t} + t).
// The second likelihood after PoissonLik whose expectation under t ~ N(rho, s) is closed form: E h = g + phi rho with
//   g = phi exp((log y - rho) + s / 2),
// rho including the offset: ONE exp per row, no nodes.  The staged y is log y, so that g is one exp of a difference: a tiny or a huge
// y never overflows a product that the exponent would not.  Every derivative of E h is a multiple of g:
//   a1 = phi - g,  a2 = g / 2,  c11 = g,  c12 = -g / 2,  c22 = g / 4      (times w),
// PoissonLik's two coefficient rows [a1 | g] with the SIGN of c12 carried by cf_factor(3) = -0.5 (the host's two-row branch puts
// the same sign on the cross block).  Not canonical in the walk's sense (y sits inside g): MINUS_Y is false, coefs ignores the
// walk's yi and infl returns e1 = phi - g whole.  No clamp: where g overflows the non-finite value reaches the sums and the entry
// refuses the point, as for PoissonLik; where g underflows to 0 the row's term is phi rho, a legitimate point.  The response mean
// E e^t = exp(rho + s / 2) does not depend on phi: the Poisson predict walk serves this model, and `mean` is PoissonLik's formula.
// Offsets, phi and log y are staged as BetaLik stages offset, precision and logit y.  No shuffles, no atomics.
struct GammaLik : TwoRowLayout {
    struct Args { const double* __restrict__ off; const double* __restrict__ disp; const double* __restrict__ y; };   // off may be nullptr; y holds log(y)
    struct Lds { double s_off[GLMM_T], s_phi[GLMM_T], s_y[GLMM_T]; };
    struct Moments {};
    static constexpr const char* LIMITS = "Gamma mixed model: P <= 64, 1 <= K <= 4";
    static bool args_ok(const Args& a) { return a.disp != nullptr && a.y != nullptr; }
    static constexpr bool MINUS_Y = false;
    static __device__ __forceinline__ double cf_factor(int kind) { return kind == 4 ? 0.25 : (kind == 3 ? -0.5 : (kind == 1 ? 0.5 : 1.0)); }   // rows [a1 | g]

    static __device__ __forceinline__ void init(Lds&, const Args&, int) {}
    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a.off && live) ? a.off[src] : 0.0;
        L.s_phi[t] = live ? a.disp[src] : 1.0;
        L.s_y[t] = live ? a.y[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }
    // g = phi exp((log y - rho) + s / 2) at rho INCLUDING the offset
    static __device__ __forceinline__ double g_of(double phi, double ly, double rho, double s) { return phi * exp((ly - rho) + 0.5 * s); }
    // e1 = a1' = phi - g whole and e2 = E h'' = g, on all four lanes of a row
    static __device__ __forceinline__ void infl(const Lds& L, const Args&, double o, bool live, int, double rho, double s, double& e1,
                                                double& e2)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row];
        const double g = live ? g_of(phi, L.s_y[row], rho + o, s) : 0.0;
        e1 = live ? phi - g : 0.0; e2 = g;
    }
    // the response mean E e^t = exp(rho + s / 2), whatever phi
    static __device__ __forceinline__ void mean(const Lds&, const Args&, double o, bool live, int, double rho, double s, double& mu)
    {
        mu = live ? exp((rho + o) + 0.5 * s) : 0.0;
    }
    static __device__ __forceinline__ Moments moments(const Lds&, const Args&, bool, int, double, double) { return {}; }
    static __device__ __forceinline__ double coefs(const Lds& L, int row, const Moments&, double wi, double, double rho, double s, double* k)
    {
        rho += L.s_off[row];
        const double phi = L.s_phi[row];
        const double g = g_of(phi, L.s_y[row], rho, s);
        k[0] = wi * (phi - g); k[1] = wi * g;
        return wi * (g + phi * rho);
    }
};

// Censored Gaussian (Tobit) with a per-row precision phi, a per-row offset and a per-row status: the latent
// y* ~ N(t, 1 / phi), and the row says delta = 0 (y = y* observed), +1 (right-censored: y* > y) or -1 (left-censored: y* < y).  The
// first policy that is closed form OR quadrature per row, by the row's status.  With r = sqrt(phi) and u = rho - y (rho including the
// offset) the row's term under t ~ N(rho, s), constants dropped, is
//   observed   h(t) = phi (y - t)^2 / 2:   E h = phi (u^2 + s) / 2,  E h' = phi u,  E h'' = phi,  E h''' = E h'''' = 0      (no nodes);
//   censored   h(t) = H(a),  a = delta r (t - y),  H = -log Phi:   d_t^k h = (delta r)^k H^(k)(a) on the nodes t_k = rho + sqrt(s) x_k,
//              H .. H'''' from BinomialLinkLik<PROBIT>::h1<5> as it stands (h1<2> in the influence walk).
// What is STAGED is the fold d = o - y next to phi and delta (three arrays, the LDS of the probit policy): u = rho_x + d is one
// addition, a shift of y and o by a common constant leaves d -- and with it every result -- unchanged wherever the shifted values are
// exact, and the predict walk, which has no y (a null y stages zeros), reads d = o: `mean` is rho + d.  y, phi and delta are read
// from the ORIGINAL row index, as every staged array; a null status is "every row observed".  Coefficients in the logistic five-row
// layout as BinomialLinkLik forms them (MINUS_Y false: y sits inside u).  The four lanes of a row share the
// row's status, so a quad never diverges; gh_lane_sum stands outside the branch.  The powers of
// delta r multiply the FINISHED sums, outside every fused multiply-add: with sqrt(phi) a power of two an all-censored data set is
// the probit model on the design (r x, r z) with the offset r (o - y) to the last bit of a, and sum_k w_k H^(j)(a_k) is formed as the
// probit policy forms it.  No clamp: an observed row overflows with phi u^2, a censored one with a^2 / 2 in the left tail; the
// non-finite value reaches the sums and the entry refuses the point.
struct CensNormalLik : NodeTableLik {
    typedef BinomialLinkLik<GLMM_LINK_PROBIT> Probit;
    struct Args { LogisticLik::Args q; const double* __restrict__ off; const double* __restrict__ disp; const double* __restrict__ y;
                  const double* __restrict__ cens; };                       // off, y (predict) and cens (all observed) may be nullptr
    struct Lds { LogisticLik::Lds q; double s_d[GLMM_T], s_phi[GLMM_T], s_st[GLMM_T]; };     // o - y, phi, delta as a double
    static constexpr const char* LIMITS = "censored Gaussian mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q) && a.disp != nullptr && a.y != nullptr; }
    static constexpr bool MINUS_Y = false;

    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        const double o = (a.off && live) ? a.off[src] : 0.0;
        const double yy = (a.y && live) ? a.y[src] : 0.0;
        L.s_d[t] = o - yy;
        L.s_phi[t] = (a.disp && live) ? a.disp[src] : 1.0;
        L.s_st[t] = (a.cens && live) ? a.cens[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_d[row]; }

    // a1' = E h' and E h'' = 2 a2' per unit weight, on all four lanes of a row; o is the staged fold o - y
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double o, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], st = L.s_st[row];
        const double u = rho + o;
        const bool cens = live && st != 0.0;
        e1 = 0.0; e2 = 0.0;
        if (cens) {                                                      // the walk in its own text: see `moments`
            const double dr = st * sqrt(phi), sd = sqrt(fmax(s, 0.0));
            for (int k = q4; k < a.q.nq; k += 4) {
                const double tu = u + sd * L.q.sx[k], wk = L.q.sw[k];
                double av, h[5];
                {
#pragma clang fp contract(off)
                    av = dr * tu;
                }
                Probit::h1<2>(av, h);
                e1 += wk * h[1]; e2 += wk * h[2];
            }
        }
        gh_lane_sum(e1, e2);
        {
#pragma clang fp contract(off)
            if (cens) { e1 = e1 * (st * sqrt(phi)); e2 = e2 * phi; }
            else if (live) { e1 = phi * u; e2 = phi; }
        }
    }
    // the latent mean E y* = rho + o, whatever phi and whatever the variance (no y in the predict walk: the staged fold is o)
    static __device__ __forceinline__ void mean(const Lds&, const Args&, double o, bool live, int, double rho, double, double& mu)
    {
        mu = live ? rho + o : 0.0;
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], st = L.s_st[row];
        const double u = rho + L.s_d[row];
        const bool cens = live && st != 0.0;
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        // The walks of this policy and of CensNormalDispLik stand in their own text, not as calls of gh_nodes: through the helper
        // glmm_slopes_rows_kernel<CensNormalLik> measured 3 to 5 % slower at K = 4, outside the margin of DESIGN.md section 46, and
        // with delta r formed ahead of the helper every observed row paid its square root (2 % of the dispersion walk).
        if (cens) {
            const double dr = st * sqrt(phi), sd = sqrt(fmax(s, 0.0));
            for (int k = q4; k < a.q.nq; k += 4) {
                const double tu = u + sd * L.q.sx[k], wk = L.q.sw[k];
                double av, h[5];
                {
#pragma clang fp contract(off)
                    av = dr * tu;
                }
                Probit::h1<5>(av, h);
#pragma unroll
                for (int i = 0; i < 5; ++i) e[i] += wk * h[i];
            }
        }
        gh_lane_sum<5>(e);
        {
#pragma clang fp contract(off)
            if (cens) {
                const double dr = st * sqrt(phi);
                e[1] = e[1] * dr; e[2] = e[2] * phi; e[3] = e[3] * (dr * phi); e[4] = e[4] * (phi * phi);
            } else if (live) {
                const double q = u * u + s;
                e[0] = 0.5 * (phi * q); e[1] = phi * u; e[2] = phi;
            }
        }
        return {e[0], e[1], e[2], e[3], e[4]};
    }
    static __device__ __forceinline__ double coefs(const Lds&, int, const Moments& mo, double wi, double, double, double, double* k)
    {
        return stein_coefs(mo, wi, k);
    }
};

// Ordinal response with a cumulative logit link: y in {0 .. T}, cut points -inf = a_0 < a_1 < .. < a_T < a_T+1 = +inf,
//   P(y = j | t) = sigma(a_j+1 - t) - sigma(a_j - t) = sigma(hi - t) sigma(t - lo) (1 - e^-D),   hi = a_y+1, lo = a_y, D = hi - lo,
//   h(t) = -log P = softplus(t - hi) + softplus(lo - t) - log(-expm1(-D)):
// two logistic node functions at two shifts plus a term without t, no cancellation anywhere.  The node expressions are
// LogisticLik::moments' at a = t - hi and at b = lo - t (d/dt b = -1: the odd derivatives of the lo term are negated); a missing cut
// point of an end category is a sentinel +-inf, at which e = exp(-inf) = 0 and every expression is an exact zero -- no branch.  The
// D term is one closed form per LIVE row behind the shuffles, in the value only; at D = +inf it is -log1p(-0) = -0.
// The table of T + 2 cut points (both sentinels) is copied to LDS once per workgroup; per row the category, clamped to [0, T] as an
// INTEGER (a bound on an address: the host entries refuse such data before any walk), and the folds hi - o and lo - o are staged from
// the row's ORIGINAL index, so that t - hi = rho_x - (hi - o) is one subtraction and a common shift of the cut points and the offset
// changes nothing wherever the shifted values are exact.  Not canonical in the walk's sense (y picks the cut points): MINUS_Y is
// false, coefficients by Stein's identity in the five-row layout.  No clamp of values: a non-finite sum reaches the entry, which
// refuses it.  The predict walk is not instantiated for this policy (no `mean`): P(y <= j) is the binomial entry's at offset o - a_j+1.
struct OrdinalLik : NodeTableLik {
    static constexpr int MAX_T = 15;
    struct Args { LogisticLik::Args q; const double* __restrict__ off; const double* __restrict__ y; const double* __restrict__ thr; int T; };   // off may be nullptr; thr: T + 2 doubles
    struct Lds { LogisticLik::Lds q; double tab[MAX_T + 2], s_hi[GLMM_T], s_lo[GLMM_T]; int s_cat[GLMM_T]; };
    struct ThrMoments { double a0, a1, a2, b0, b1, b2; };                  // E sigma, E sigma', E sigma'' at t - hi and at lo - t
    static constexpr const char* LIMITS = "ordinal mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes, 1 to 15 thresholds";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q) && a.y != nullptr && a.thr != nullptr && a.T >= 1 && a.T <= MAX_T; }
    static constexpr bool MINUS_Y = false;

    static __device__ __forceinline__ void init(Lds& L, const Args& a, int tid)
    {
        LogisticLik::init(L.q, a.q, tid);
        if (tid < a.T + 2) L.tab[tid] = a.thr[tid];
    }
    // after the barrier that follows init: reads the table
    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        const double o = (a.off && live) ? a.off[src] : 0.0;
        const double yy = live ? a.y[src] : 0.0;
        const int j = yy >= 0.0 ? (yy <= (double)a.T ? (int)yy : a.T) : 0;   // a NaN compares false: 0
        L.s_cat[t] = j; L.s_hi[t] = L.tab[j + 1] - o; L.s_lo[t] = L.tab[j] - o;
    }
    static __device__ __forceinline__ double row_shift(const Lds&, int) { return 0.0; }   // the folds are read by gs_lane_row()
    // D = hi - lo from the TABLE, not from the two folds: those carry the rounding of a - o, which at a small D would be most of it
    static __device__ __forceinline__ double row_delta(const Lds& L, int row) { const int j = L.s_cat[row]; return L.tab[j + 1] - L.tab[j]; }

    // softplus, sigma, sigma' (N = 2: g[1], g[2] only) and sigma'', sigma''' (N = 5) at x, as LogisticLik::moments forms them
    template <int N>
    static __device__ __forceinline__ void node(double x, double* g)
    {
        const double e = exp(-fabs(x)), ie = 1.0 / (1.0 + e);
        const double g2 = e * ie * ie;
        g[1] = x >= 0.0 ? ie : e * ie; g[2] = g2;
        if constexpr (N == 5) {
            const double om = (1.0 - e) * ie;                            // |1 - 2 sigma|
            g[0] = (x > 0.0 ? x : 0.0) + log1p(e);
            g[3] = x >= 0.0 ? -g2 * om : g2 * om; g[4] = g2 * (1.0 - 6.0 * g2);
        }
    }
    // -log(1 - e^-D), D > 0: past log 2 through log1p (1 - e^-D rounds to 1 from D = 37 on)
    static __device__ __forceinline__ double delta_term(double D) { return D > 0.6931471805599453 ? -log1p(-exp(-D)) : -log(-expm1(-D)); }

    // a1' = E h' and E h'' = 2 a2' per unit weight, on all four lanes of a row
    static __device__ __forceinline__ void infl(const Lds& L, const Args& a, double, bool live, int q4, double rho, double s, double& e1,
                                                double& e2)
    {
        const int row = gs_lane_row();
        const double hi = L.s_hi[row], lo = L.s_lo[row];
        e1 = 0.0; e2 = 0.0;
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double ga[5], gb[5];
            node<2>(t - hi, ga);
            node<2>(lo - t, gb);
            e1 += wk * (ga[1] - gb[1]); e2 += wk * (ga[2] + gb[2]);
        });
        gh_lane_sum(e1, e2);
    }
    static __device__ __forceinline__ Moments moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double hi = L.s_hi[row], lo = L.s_lo[row];
        double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double ga[5], gb[5];
            node<5>(t - hi, ga);
            node<5>(lo - t, gb);
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] += wk * ((i & 1) ? ga[i] - gb[i] : ga[i] + gb[i]);
        });
        gh_lane_sum<5>(e);
        return {live ? e[0] + delta_term(row_delta(L, row)) : 0.0, e[1], e[2], e[3], e[4]};
    }
    static __device__ __forceinline__ double coefs(const Lds&, int, const Moments& mo, double wi, double, double, double, double* k)
    {
        return stein_coefs(mo, wi, k);
    }
    // the six node sums of the threshold pass (glmm_thr_rows_kernel), on all four lanes of a row
    static __device__ __forceinline__ ThrMoments thr_moments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double hi = L.s_hi[row], lo = L.s_lo[row];
        double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            double ga[5], gb[5];
            node<5>(t - hi, ga);                                         // the value and sigma''' are not read and fall to the compiler
            node<5>(lo - t, gb);
            e[0] += wk * ga[1]; e[1] += wk * ga[2]; e[2] += wk * ga[3];
            e[3] += wk * gb[1]; e[4] += wk * gb[2]; e[5] += wk * gb[3];
        });
        gh_lane_sum<6>(e);
        return {e[0], e[1], e[2], e[3], e[4], e[5]};
    }
};

// ---- the dispersion-derivative policies ----------------------------------------------------------------------
// The dispersion of the Beta and the NB2 model as phi_n = e^lambda phi0_n with ONE scalar lambda: every derivative below is in
// lambda at fixed t, d/d lambda = phi d/d phi.  A policy of this kind serves glmm_disp_rows_kernel (k_glmm_slopes.hip) and supplies
// the staging of its base policy and ONE function
//   dmoments(lik, la, live, q4, rho, s) -> (E h_l, E d_t h_l, E d_t^2 h_l, E h_ll) per unit weight, t ~ N(rho + offset, s),
// on all four lanes of a row, by gh_nodes and gh_lane_sum<4>.  By Stein's identity E d_t h_l is the derivative of E h_l in rho and E d_t^2 h_l / 2 the one in s: the two
// coefficient rows of the cross Hessian d^2 F / d theta d lambda.
struct DispMoments { double hl, t1, t2, hll; };

// Beta (the shifted form of BetaLik): a = phi mu, b = phi (1 - mu), v = mu (1 - mu), d = 1 - 2 mu, l = logit y,
//   h_l  = a psi(1 + a) + b psi(1 + b) - l a - 2,
//   h_ll = a psi(1 + a) + a^2 psi'(1 + a) + b psi(1 + b) + b^2 psi'(1 + b) - l a,
//   K1 = phi [psi(1 + a) + a psi'(1 + a) - psi(1 + b) - b psi'(1 + b) - l],   K2 = phi^2 [2 psi'(1 + a) + a psi''(1 + a) + 2 psi'(1 + b) + b psi''(1 + b)],
//   d_t h_l = K1 v,   d_t^2 h_l = K2 v^2 + K1 v d.
// mu and 1 - mu from e = exp(-|t|) as BetaLik::node forms them; psi, psi', psi'' from BetaLik::polygamma<5>, whose lgamma and psi'''
// are not read here and fall to the compiler (the function is inlined).  Every polygamma argument is >= 1.  The -2 is E of a
// constant: added once per row behind the shuffles.
struct BetaDispLik {
    typedef BetaLik::Args Args;
    typedef BetaLik::Lds Lds;
    static constexpr const char* LIMITS = BetaLik::LIMITS;
    static bool args_ok(const Args& a) { return BetaLik::args_ok(a); }
    static __device__ __forceinline__ void init(Lds& L, const Args& a, int tid) { BetaLik::init(L, a, tid); }
    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src) { BetaLik::stage_row(L, a, t, live, src); }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return BetaLik::row_shift(L, row); }

    static __device__ __forceinline__ DispMoments dmoments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], l = L.s_y[row];
        rho += L.s_off[row];
        double m[4] = {0.0, 0.0, 0.0, 0.0};
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
            const bool pos = t >= 0.0;
            const double mu = pos ? ie : e * ie, nu = pos ? e * ie : ie;      // sigma(t) and sigma(-t)
            const double g2 = e * ie * ie;                                   // v = mu (1 - mu)
            const double om = (1.0 - e) * ie;
            const double d = pos ? -om : om;                                 // 1 - 2 mu
            const double pa_ = phi * mu, pb_ = phi * nu;
            double pa[5], pb[5];
            BetaLik::polygamma<5>(1.0 + pa_, pa);
            BetaLik::polygamma<5>(1.0 + pb_, pb);
            const double first = pa_ * pa[1] + pb_ * pb[1] - l * pa_;        // h_l + 2
            const double ta = pa_ * pa[2], tb = pb_ * pb[2];                 // a psi'(1 + a), b psi'(1 + b)
            const double K1 = phi * (((pa[1] + ta) - (pb[1] + tb)) - l);
            const double K2 = phi * phi * ((2.0 * pa[2] + pa_ * pa[3]) + (2.0 * pb[2] + pb_ * pb[3]));
            const double K1v = K1 * g2;
            m[0] += wk * first; m[1] += wk * K1v; m[2] += wk * (K2 * g2 * g2 + K1v * d); m[3] += wk * (first + pa_ * ta + pb_ * tb);
        });
        gh_lane_sum<4>(m);
        return {live ? m[0] - 2.0 : 0.0, m[1], m[2], m[3]};
    }
};

// NB2 through the binomial context: eta = t - log phi is what that context integrates over (its offset is o - log phi), m = y + phi
// its trials.  On the logistic nodes, with sp = softplus(eta), sg = sigma(eta) and its derivatives g2, g3 (LogisticLik::moments),
//   h_l  = phi sp - m sg + y,   h_ll = phi sp - 2 phi sg + m g2,   d_t h_l = phi sg - m g2,   d_t^2 h_l = phi g2 - m g3.
// The shifted offset, the trials and phi ITSELF are staged (phi is never recovered as trials - y: at phi << y that loses it), and y
// from the context's responses.  The E sums of sp, sg, g2, g3 are formed per lane and combined with phi, m and y behind the
// shuffles (all four are linear in them).
struct NegBinDispLik {
    struct Args { LogisticLik::Args q; const double* __restrict__ off; const double* __restrict__ trials; const double* __restrict__ disp;
                  const double* __restrict__ y; };                          // off may be nullptr
    struct Lds { LogisticLik::Lds q; double s_off[GLMM_T], s_m[GLMM_T], s_phi[GLMM_T], s_y[GLMM_T]; };
    static constexpr const char* LIMITS = "negative binomial mixed model: P <= 64, 1 <= K <= 4, at most 128 nodes";
    static bool args_ok(const Args& a) { return LogisticLik::args_ok(a.q) && a.trials != nullptr && a.disp != nullptr && a.y != nullptr; }
    static __device__ __forceinline__ void init(Lds& L, const Args& a, int tid) { LogisticLik::init(L.q, a.q, tid); }
    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src)
    {
        L.s_off[t] = (a.off && live) ? a.off[src] : 0.0;
        L.s_m[t] = live ? a.trials[src] : 1.0;
        L.s_phi[t] = live ? a.disp[src] : 1.0;
        L.s_y[t] = live ? a.y[src] : 0.0;
    }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return L.s_off[row]; }

    static __device__ __forceinline__ DispMoments dmoments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], mt = L.s_m[row], yt = L.s_y[row];
        rho += L.s_off[row];
        double m[4] = {0.0, 0.0, 0.0, 0.0};                                  // E sp, E sg, E g2, E g3
        gh_nodes(L.q, a.q.nq, live, q4, rho, s, [&](double t, double wk) {
            const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
            const double sp = (t > 0.0 ? t : 0.0) + log1p(e);
            const double sg = t >= 0.0 ? ie : e * ie;
            const double g2 = e * ie * ie;
            const double om = (1.0 - e) * ie;                            // |1 - 2 sigma|
            const double g3 = t >= 0.0 ? -g2 * om : g2 * om;
            m[0] += wk * sp; m[1] += wk * sg; m[2] += wk * g2; m[3] += wk * g3;
        });
        gh_lane_sum<4>(m);
        if (!live) return {0.0, 0.0, 0.0, 0.0};
        return {(phi * m[0] - mt * m[1]) + yt, phi * m[1] - mt * m[2], phi * m[2] - mt * m[3], phi * (m[0] - 2.0 * m[1]) + mt * m[2]};
    }
};

// Gamma: h = phi (y e^{-t} + t) is LINEAR in phi, so that in lambda = log(phi / phi0)
//   h_l = h_ll = h,   d_t h_l = h',   d_t^2 h_l = h'':   (E h, phi - g, g, E h) with GammaLik's g and staging.
// The derivative of the data term in lambda is the data term, the cross Hessian its gradient -- formed here by a kernel of its own.
struct GammaDispLik {
    typedef GammaLik::Args Args;
    typedef GammaLik::Lds Lds;
    static constexpr const char* LIMITS = GammaLik::LIMITS;
    static bool args_ok(const Args& a) { return GammaLik::args_ok(a); }
    static __device__ __forceinline__ void init(Lds& L, const Args& a, int tid) { GammaLik::init(L, a, tid); }
    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src) { GammaLik::stage_row(L, a, t, live, src); }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return GammaLik::row_shift(L, row); }

    static __device__ __forceinline__ DispMoments dmoments(const Lds& L, const Args&, bool live, int, double rho, double s)
    {
        if (!live) return {0.0, 0.0, 0.0, 0.0};
        const int row = gs_lane_row();
        const double phi = L.s_phi[row];
        rho += L.s_off[row];
        const double g = GammaLik::g_of(phi, L.s_y[row], rho, s);
        const double eh = g + phi * rho;
        return {eh, phi - g, g, eh};
    }
};

// Censored Gaussian: the precision phi = e^lambda phi0, so r = sqrt(phi) and a = delta r (t - y) has d_l a = a / 2.
//   observed   h is linear in phi, as the Gamma term:  h_l = h_ll = h,  d_t h_l = h',  d_t^2 h_l = h'':  (E h, phi u, phi, E h);
//   censored   h_l = a H' / 2,   h_ll = a (a H'' + H') / 4,   d_t h_l = delta r (a H'' + H') / 2,   d_t^2 h_l = phi (a H''' + 2 H'') / 2
// on the nodes, H', H'', H''' from the probit h1<5> (its value and fourth derivative are not read and fall to the compiler).  None of
// the three sums cancels in a tail: as a -> -inf, a H'' + H' -> 2 a and a H''' + 2 H'' -> 2; as a -> +inf every term vanishes.  The
// halves, delta r and phi multiply the finished sums.  Staging, the fold u = rho + (o - y) and the status are CensNormalLik's.
struct CensNormalDispLik {
    typedef CensNormalLik::Args Args;
    typedef CensNormalLik::Lds Lds;
    static constexpr const char* LIMITS = CensNormalLik::LIMITS;
    static bool args_ok(const Args& a) { return CensNormalLik::args_ok(a); }
    static __device__ __forceinline__ void init(Lds& L, const Args& a, int tid) { CensNormalLik::init(L, a, tid); }
    static __device__ __forceinline__ void stage_row(Lds& L, const Args& a, int t, bool live, i64 src) { CensNormalLik::stage_row(L, a, t, live, src); }
    static __device__ __forceinline__ double row_shift(const Lds& L, int row) { return CensNormalLik::row_shift(L, row); }

    static __device__ __forceinline__ DispMoments dmoments(const Lds& L, const Args& a, bool live, int q4, double rho, double s)
    {
        const int row = gs_lane_row();
        const double phi = L.s_phi[row], st = L.s_st[row];
        const double u = rho + L.s_d[row];
        const bool cens = live && st != 0.0;
        double m[4] = {0.0, 0.0, 0.0, 0.0};
        if (cens) {                                                      // the walk in its own text: see CensNormalLik::moments
            const double dr = st * sqrt(phi), sd = sqrt(fmax(s, 0.0));
            for (int k = q4; k < a.q.nq; k += 4) {
                const double tu = u + sd * L.q.sx[k], wk = L.q.sw[k];
                double av, h[5];
                {
#pragma clang fp contract(off)
                    av = dr * tu;
                }
                CensNormalLik::Probit::h1<5>(av, h);
                const double b1 = av * h[2] + h[1];                          // a H'' + H'
                m[0] += wk * (av * h[1]); m[1] += wk * b1; m[2] += wk * (av * h[3] + 2.0 * h[2]); m[3] += wk * (av * b1);
            }
        }
        gh_lane_sum<4>(m);
        if (cens) return {0.5 * m[0], (0.5 * (st * sqrt(phi))) * m[1], (0.5 * phi) * m[2], 0.25 * m[3]};
        if (!live) return {0.0, 0.0, 0.0, 0.0};
        double eh;
        {
#pragma clang fp contract(off)
            const double q = u * u + s;
            eh = 0.5 * (phi * q);
        }
        return {eh, phi * u, phi, eh};
    }
};

// ---- what the kernels over group-sorted rows share ----------------------------------------------------------------------------------
// The head of a tile of sorted rows: thread t < GLMM_T finds row t0 + t's original position, its group (the last g with
// offs[g] <= i) and whether that group lies whole inside the tile; then the tile's rows of X and Z are gathered into xs (row
// stride XS, z behind the P columns of x).  HAS_Z = false is the unit design of the random intercept: no Z is read, and no division
// by Kz is emitted.  Ends on a barrier.
template <class Lik, int XS, bool HAS_Z = true>
__device__ __forceinline__ void gs_stage_sorted_tile(int tid, i64 t0, int rows, int P, int Kz, i64 G, const double* __restrict__ X,
                                                     const double* __restrict__ Z, const i64* __restrict__ perm,
                                                     const i64* __restrict__ offs, const typename Lik::Args& la, typename Lik::Lds& lik,
                                                     double* xs, i64* s_row, int* s_gid, int* s_whole)
{
    if (tid < GLMM_T) {
        int g = 0, whole = 0;
        i64 pr = 0;
        if (tid < rows) {
            const i64 i = t0 + tid;
            pr = perm[i];
            i64 lo = 0, hi = G;                                          // the last g with offs[g] <= i (its offs[g + 1] > i)
            while (hi - lo > 1) { const i64 mid = (lo + hi) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid; }
            g = (int)lo;
            whole = (offs[lo] >= t0 && offs[lo + 1] <= t0 + GLMM_T) ? 1 : 0;
        }
        s_row[tid] = pr; s_gid[tid] = g; s_whole[tid] = whole;
        Lik::stage_row(lik, la, tid, tid < rows, pr);
    }
    __syncthreads();
    for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * XS + cc] = X[s_row[rr] * P + cc]; }
    if constexpr (HAS_Z)
        for (int e = tid; e < rows * Kz; e += 256) { const int rr = e / Kz, cc = e - rr * Kz; xs[rr * XS + P + cc] = Z[s_row[rr] * Kz + cc]; }
    __syncthreads();
}

// Where the walk of a tile flushes the segment that ends at a change of group: the group's own row of the result where the group
// lies whole inside the tile, else one of the tile's two partial rows -- row 0 for the piece that began at the tile's first row
// (the tail of a group cut by the boundary before it), row 1 for the piece that runs to its end.
__device__ __forceinline__ double* gs_flush_dst(bool whole, int g, i64 tile, int run_start, int ncol, double* gsum, double* part)
{
    return whole ? gsum + (i64)g * ncol : part + (tile * 2 + (run_start == 0 ? 0 : 1)) * ncol;
}

// One grid for every walk over `rows` rows: a workgroup per tile, at most 2048 of them (a workgroup then walks several tiles).
inline unsigned glmm_grid(i64 rows) { const i64 n_tiles = glmm_num_tiles(rows); return (unsigned)(n_tiles < 1 ? 1 : (n_tiles < 2048 ? n_tiles : 2048)); }

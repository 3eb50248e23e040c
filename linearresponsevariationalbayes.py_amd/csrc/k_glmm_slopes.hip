// k_glmm_slopes.hip -- mixed models with K <= 4 independent random effects per group, q(beta_j) = N(m_j, v_j), q(u_gk) = N(e_gk, r_gk):
//   logistic:  y_n ~ Bernoulli(sigma(x_n . beta + z_n . u_g(n)))
//   Poisson  (DESIGN.md section 26):  y_n ~ Poisson(exp(o_n + x_n . beta + z_n . u_g(n)))
//   binomial:  y_n ~ Binomial(m_n, sigma(o_n + x_n . beta + z_n . u_g(n))), and through it NB2
//   binomial with a probit or cloglog link:  p = Phi(.) or 1 - exp(-exp(.)) in the place of sigma(.)
//   zero-truncated Poisson:  y_n >= 1,  P(y_n) = Poisson(y_n; lambda_n) / (1 - exp(-lambda_n)),  lambda_n as the Poisson one
//   zero-truncated NB2:  y_n >= 1,  P(y_n) = NB2(y_n; mu_n, phi_n) / (1 - (1 + mu_n / phi_n)^-phi_n),  mu_n as lambda_n
//   Beta:  0 < y_n < 1,  y_n ~ Beta(mu_n phi_n, (1 - mu_n) phi_n),  mu_n = sigma(o_n + x_n . beta + z_n . u_g(n))
//   Gamma:  y_n > 0,  y_n ~ Gamma(shape phi_n, mean exp(o_n + x_n . beta + z_n . u_g(n)))
//   censored Gaussian:  y*_n ~ N(o_n + x_n . beta + z_n . u_g(n), 1 / phi_n), observed, left- or right-censored at y_n
//   ordinal, cumulative logit:  P(y_n <= j) = sigma(alpha_j+1 - o_n - x_n . beta - z_n . u_g(n)),  y_n in {0 .. T}
// Per observation rho_n = x_n . m + z_n . e_g, s_n = (x_n o x_n) . v + (z_n o z_n) . r_g and five coefficients a1, a2, c11, c12, c22.
// Every kernel that walks the rows is written ONCE, as a template over a likelihood policy (k_glmm_walk.h, DESIGN.md sections 27 and
// 31): LogisticLik (the quadrature k_glmm.hip runs too; with K = 1 and z = 1 this is that model) and PoissonLik
// (psi = E exp(t) = exp(o + rho + s / 2) exactly: ONE exp per row, no nodes); BinomialLik is the first that needs both kinds of
// state, the nodes and staged per-row data.  A policy supplies
//   Args / Lds      what only its kernels are handed (the nodes, a struct | the offset, a __restrict__ pointer) and its LDS (node
//                   tables | the tile's offsets) -- nothing of the other's;
//   init, stage_row what it puts there, once per workgroup and once per staged row;
//   row_shift, infl (rho, s) -> (e1, e2) = (psi_rho, 2 psi_s) on all four lanes of a row, row_shift being what the row adds to rho
//                   (the staged offset), read ahead of the dot products: the two influence kernels;
//   MINUS_Y, mean   whether those two kernels subtract y from e1 (every canonical likelihood: a1' = psi_rho - y) or take e1 as the
//                   whole a1' (BinomialLinkLik, which stages y itself), and the response-scale mean of the predict walk
//                   (infl's e1 for the canonical ones; a function of its own for the two links);
//   moments, coefs  (rho, s) -> the row's value and its NCF coefficient rows: the rows kernel;
//   cf_row, HAS_FACTOR / cf_factor, NB / o_d / d_stride, DK
//                   rows kernel: where the five coefficients live.  The logistic model keeps five rows.  With h = w psi the
//                   Poisson ones are a1 = h - w y, a2 = h / 2, c11 = h, c12 = h / 2, c22 = h / 4: TWO rows (a1, h) and the constant
//                   factors 1, 1/2, 1, 1/2, 1/4.  A power of two is applied ONCE to a finished sum (at the flush of a segment; to
//                   a whole block in the host's terms body), bit for bit the sum of the scaled terms.  So its products table has
//                   NB = 2 blocks per component (h z_k, h z_k^2), stored densely, against the logistic 4 at stride 16.
//
// glmm_slopes_rows_kernel is ONE pass over the rows in group-sorted order, built like glmm_rows_kernel: a workgroup (4 waves) walks
// tiles of GLMM_T = 64 sorted rows.
//   1. the tile's rows of X are gathered through the permutation into LDS, and the row's K values of z behind them (columns
//      P .. P + K - 1 of the same LDS row, stride GS_XS);
//   2. four lanes share a row for the four dot products (lane q4 takes the x columns q4, q4 + 4, .. and the z column q4) and for
//      the quadrature nodes; xor shuffles add the quarters;
//   3. lane 0 of the four writes the coefficients to the ORIGINAL row position (global block and gradient by the library's
//      weighted products, unchanged) and to LDS;
//   4. the products of a row that P border columns each share (logistic: 4 K,
//        d[0 K + k] = c11 z_k,  d[1 K + k] = c12 z_k^2,  d[2 K + k] = c12 z_k,  d[3 K + k] = c22 z_k^2;
//      Poisson: the first 2 K of them with h for both coefficients, blocks 2 and 3 reading blocks 0 and 1)
//      are formed ONCE per row into LDS;
//   5. segmented sums from the tile still in LDS over the ncol = nsc + 4 K P columns of a group,
//        [ sum a1 z (K) | sum a2 z o z (K) | upper triangle, row-major, of the 2 K x 2 K block  sum c q q^T  (K (2 K + 1)) |
//          border: column nsc + (b K + k) P + j = sum d[b K + k] x_j (b = 0, 1) or d[b K + k] x_j^2 (b = 2, 3) ],
//      nsc = 2 K + K (2 K + 1), q = [z | z o z] and c = c11 / c12 / c22 by the halves the pair lies in.  Thread t owns the
//      border columns t, t + 256, t + 512, t + 768 (consecutive threads read consecutive LDS words of the staged row; the
//      factor d is a broadcast) and, for t < nsc, scalar column t.  The tile's rows are walked in order, flushing at every change
//      of group: a group inside one tile goes to its row of the result, the piece of a group cut by a tile boundary to one of
//      the tile's two partial rows, which glmm_fixup_kernel (k_glmm.hip) adds in tile order.
// No atomics anywhere: the result is a fixed-order sum, bitwise reproducible.  Empty groups keep the zeros the caller wrote.
// The launchers dispatch over K with gs_with_K and over the likelihood with gs_with_lik.
// The Poisson policy does not clamp: where o + rho + s / 2 overflows the exponent, psi = inf reaches the sums and the entry refuses
// the non-finite value (LRVB_ERR_INVALID).
#include "k_glmm_walk.h"
#include <type_traits>

constexpr int GS_XS = 68;                // LDS row stride in doubles: 64 columns of x + 4 of z; 68 = 4 mod 32, so the 8 rows x 4 lanes
                                         // of a 32-lane half read 32 different 8-byte bank pairs in the dot products
constexpr int GS_OWN = 4;                // border columns per thread: 4 K P <= 1024 = 4 x 256

template <class Lik>
__global__ __launch_bounds__(256)
void glmm_slopes_rows_kernel(i64 N, int P, int Kz, i64 G, const double* __restrict__ X, const double* __restrict__ Z,
                             const double* __restrict__ y, const double* __restrict__ w, const i64* __restrict__ perm,
                             const i64* __restrict__ offs, const double* __restrict__ m, const double* __restrict__ vb,
                             const double* __restrict__ eg, const double* __restrict__ rg, typename Lik::Args la,
                             double* __restrict__ coef, i64 NP, double* __restrict__ gsum, double* __restrict__ part,
                             double* __restrict__ vpart)
{
    __shared__ double xs[GLMM_T * GS_XS], dk[GLMM_T * Lik::DK], cf[Lik::NCF * GLMM_T], ms[64], vs[64], red[4];
    __shared__ typename Lik::Lds lik;
    __shared__ i64 s_row[GLMM_T];
    __shared__ int s_gid[GLMM_T], s_whole[GLMM_T];
    const int tid = threadIdx.x;
    const int K2 = 2 * Kz, ND = Lik::NB * Kz, DS = Lik::d_stride(Kz);
    const int nsc = K2 + Kz * (K2 + 1), nbord = 4 * Kz * P, ncol = nsc + nbord;
    Lik::init(lik, la, tid);
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    // the border columns of this thread: column t = tid + 256 i is block bk = t / P (b = bk / K, k = bk - b K) and x column
    // j = t - bk P; it reads the product o_d(b, k), squares x for b >= 2 and (Poisson) carries the factor of its coefficient
    int o_x[GS_OWN], o_d[GS_OWN];
    bool o_has[GS_OWN], o_sq[GS_OWN];
    double o_f[GS_OWN];
#pragma unroll
    for (int i = 0; i < GS_OWN; ++i) {
        const int t = tid + 256 * i;
        o_has[i] = t < nbord;
        const int bk = o_has[i] ? t / P : 0, b = bk / Kz, k = bk - b * Kz;
        o_d[i] = Lik::o_d(b, k, Kz); o_x[i] = o_has[i] ? t - bk * P : 0; o_sq[i] = bk >= K2;
        o_f[i] = Lik::cf_factor(b == 0 ? 2 : (b == 3 ? 4 : 3));
    }
    // the scalar column of this thread (tid < nsc): coefficient s_k times q[s_i] q[s_j] with q = [z | z o z | 1]
    const bool has_sc = tid < nsc;
    int s_k = 0, s_i = K2, s_j = K2;
    if (tid < Kz) { s_k = 0; s_i = tid; }
    else if (tid < K2) { s_k = 1; s_i = tid; }
    else if (has_sc) {
        int u = tid - K2, i = 0;
        while (u >= K2 - i) { u -= K2 - i; ++i; }
        s_i = i; s_j = i + u;
        s_k = s_j < Kz ? 2 : (s_i >= Kz ? 4 : 3);
    }
    const int s_c = Lik::cf_row(s_k);
    const double s_f = Lik::cf_factor(s_k);
    const int zi = P + (s_i < Kz ? s_i : s_i - Kz), zj = P + (s_j < Kz ? s_j : s_j - Kz);    // unused where the factor is 1
    const bool i_one = s_i >= K2, i_sq = s_i >= Kz, j_one = s_j >= K2, j_sq = s_j >= Kz;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(N - t0 < GLMM_T ? N - t0 : GLMM_T);
        __syncthreads();                                                 // the previous tile is consumed (and the nodes, m, v are in place)
        gs_stage_sorted_tile<Lik, GS_XS>(tid, t0, rows, P, Kz, G, X, Z, perm, offs, la, lik, xs, s_row, s_gid, s_whole);
        double rho = 0.0, s = 0.0;
        if (row < rows) {
            const double* xr = xs + row * GS_XS;
            for (int j = q4; j < P; j += 4) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
            if (q4 < Kz) {
                const i64 gk = (i64)s_gid[row] * Kz + q4;
                const double z = xr[P + q4];
                rho += z * eg[gk]; s += z * z * rg[gk];
            }
        }
        rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
        rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
        const typename Lik::Moments mo = Lik::moments(lik, la, row < rows, q4, rho, s);
        double contrib = 0.0;
        if (q4 == 0) {
            double k[Lik::NCF];
#pragma unroll
            for (int i = 0; i < Lik::NCF; ++i) k[i] = 0.0;
            if (row < rows) {
                const i64 pr = s_row[row];
                contrib = Lik::coefs(lik, row, mo, w[pr], y[pr], rho, s, k);
#pragma unroll
                for (int i = 0; i < Lik::NCF; ++i) coef[i * NP + pr] = k[i];
            }
#pragma unroll
            for (int i = 0; i < Lik::NCF; ++i) cf[i * GLMM_T + row] = k[i];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) contrib += __shfl_xor(contrib, off);
        if ((tid & 63) == 0) red[tid >> 6] = contrib;
        __syncthreads();
        if (tid == 0) vpart[tile] = (red[0] + red[1]) + (red[2] + red[3]);
        // the NB K products of a row that its border columns share
        for (int e = tid; e < rows * ND; e += 256) {
            const int rr = e / ND, bk = e - rr * ND, b = bk / Kz, k = bk - b * Kz;
            const double z = xs[rr * GS_XS + P + k];
            dk[rr * DS + bk] = cf[Lik::cf_row(b == 0 ? 2 : (b == 3 ? 4 : 3)) * GLMM_T + rr] * ((b & 1) ? z * z : z);
        }
        __syncthreads();
        // segmented sums over the tile's rows, in row order
        if (o_has[0] || has_sc) {
            double acc[GS_OWN] = {0.0, 0.0, 0.0, 0.0}, accs = 0.0;
            int run_start = 0;
            for (int rr = 0; rr < rows; ++rr) {
                const double* xr = xs + rr * GS_XS;
                const double* dr = dk + rr * DS;
#pragma unroll
                for (int i = 0; i < GS_OWN; ++i)
                    if (o_has[i]) { double x = xr[o_x[i]]; if (o_sq[i]) x *= x; acc[i] += dr[o_d[i]] * x; }
                if (has_sc) {
                    double fi = 1.0, fj = 1.0;
                    if (!i_one) { fi = xr[zi]; if (i_sq) fi *= fi; }
                    if (!j_one) { fj = xr[zj]; if (j_sq) fj *= fj; }
                    accs += cf[s_c * GLMM_T + rr] * (fi * fj);
                }
                const int g = s_gid[rr];
                if (rr == rows - 1 || s_gid[rr + 1] != g) {
                    double* dst = gs_flush_dst(s_whole[rr], g, tile, run_start, ncol, gsum, part);
#pragma unroll
                    for (int i = 0; i < GS_OWN; ++i)
                        if (o_has[i]) {
                            if constexpr (Lik::HAS_FACTOR) acc[i] = o_f[i] * acc[i];
                            dst[nsc + tid + 256 * i] = acc[i]; acc[i] = 0.0;
                        }
                    if (has_sc) {
                        if constexpr (Lik::HAS_FACTOR) accs = s_f * accs;
                        dst[tid] = accs;
                    }
                    accs = 0.0; run_start = rr + 1;
                }
            }
        }
    }
}

// The runtime Kz in 1..4 as a compile-time constant: f(std::integral_constant<int, Kz>); any other value is refused with `text`.
template <class F>
static int gs_with_K(int Kz, const char* text, F&& f) {
    switch (Kz) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    default: LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "%s", text);
    }
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// The likelihood of a GlmmLik as its policy: f(Lik(), la) with la the Lik::Args the kernels of that policy are handed.
template <class F>
static int gs_with_lik(const GlmmLik& lik, F&& f) {
    const LogisticLik::Args q{lik.gx, lik.gw, lik.n_nodes};
    if (lik.kind == GLMM_POISSON) return f(PoissonLik(), PoissonLik::Args(lik.off));
    if (lik.kind == GLMM_ZTPOISSON) return f(TruncPoissonLik(), TruncPoissonLik::Args{q, lik.off});
    if (lik.kind == GLMM_ZTNEGBIN) return f(TruncNegBinLik(), TruncNegBinLik::Args{q, lik.off, lik.trials, lik.y});
    if (lik.kind == GLMM_BETA) return f(BetaLik(), BetaLik::Args{q, lik.off, lik.trials, lik.y});
    if (lik.kind == GLMM_GAMMA) return f(GammaLik(), GammaLik::Args{lik.off, lik.trials, lik.y});
    if (lik.kind == GLMM_CENSNORMAL) return f(CensNormalLik(), CensNormalLik::Args{q, lik.off, lik.trials, lik.y, lik.cens});
    if (lik.kind == GLMM_ORDINAL) return f(OrdinalLik(), OrdinalLik::Args{q, lik.off, lik.y, lik.thr, lik.T});
    if (lik.kind == GLMM_BINOMIAL && lik.link == GLMM_LINK_PROBIT)
        return f(BinomialLinkLik<GLMM_LINK_PROBIT>(), BinomialLinkLik<GLMM_LINK_PROBIT>::Args{q, lik.off, lik.trials, lik.y});
    if (lik.kind == GLMM_BINOMIAL && lik.link == GLMM_LINK_CLOGLOG)
        return f(BinomialLinkLik<GLMM_LINK_CLOGLOG>(), BinomialLinkLik<GLMM_LINK_CLOGLOG>::Args{q, lik.off, lik.trials, lik.y});
    if (lik.kind == GLMM_BINOMIAL) return f(BinomialLik(), BinomialLik::Args{q, lik.off, lik.trials});
    return f(LogisticLik(), q);
}

// The link of a policy: 0 (logit, or no link at all) for every policy but BinomialLinkLik
template <class Lik> struct gs_link_of { static constexpr int value = GLMM_LINK_LOGIT; };
template <int LINK> struct gs_link_of<BinomialLinkLik<LINK>> { static constexpr int value = LINK; };

template <class Lik>
static int gs_launch_rows(lrvb_ctx* c, int Kz, const double* Z, typename Lik::Args la, const double* m, const double* vb, const double* eg,
                          const double* rg, double* coef, i64 NP, double* gsum, double* part, double* vpart) {
    const i64 N = c->N, G = c->n_groups;
    if (c->P > 64 || Kz < 1 || Kz > 4 || !Lik::args_ok(la)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "%s", Lik::LIMITS);
    const int ncol = glmm_slopes_ncol((int)c->P, Kz);
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    hipLaunchKernelGGL(glmm_slopes_rows_kernel<Lik>, dim3(glmm_grid(N)), dim3(256), 0, c->stream, N, (int)c->P, Kz, G, (const double*)c->X.p, Z,
                       (const double*)c->y.p, (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, la, coef, NP, gsum, part, vpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncol, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// Z = nullptr is the unit design: the logistic model with one effect per group on its own kernels (k_glmm.hip)
static int gs_unit_design(const GlmmLik& lik, int Kz) {
    if (lik.kind != GLMM_LOGISTIC || Kz != 1) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "the unit group design is the logistic mixed model with one effect per group");
    return LRVB_OK;
}

int launch_glmm_slopes_rows(lrvb_ctx* c, const GlmmLik& lik, int Kz, const double* Z, const double* m, const double* vb, const double* eg,
                            const double* rg, double* coef, i64 NP, double* gsum, double* part, double* vpart) {
    if (!Z) { LRVB_TRY(gs_unit_design(lik, Kz)); return launch_glmm_rows(c, m, vb, eg, rg, lik.gx, lik.gw, lik.n_nodes, coef, NP, gsum, part, vpart); }
    return gs_with_lik(lik, [&](auto L, auto la) { return gs_launch_rows<decltype(L)>(c, Kz, Z, la, m, vb, eg, rg, coef, NP, gsum, part, vpart); });
}
int glmm_slopes_ncol(int P, int Kz) { return 2 * Kz + Kz * (2 * Kz + 1) + 4 * Kz * P; }

// ---- the derivative in the log-dispersion (lrvb_glmm_beta_dispersion_terms / lrvb_glmm_negbin_dispersion_terms) ----
// ONE pass over the rows in group-sorted order on the head of glmm_slopes_rows_kernel: the same tiles, the same staging
// (gs_stage_sorted_tile), four lanes per row for rho and s by the same dot products, then DLik::dmoments.  Per row
//   d1 = w E d_t h_l   (the derivative in rho of the row's h_l term),   d2 = w E d_t^2 h_l / 2   (the one in s),
// written to the ORIGINAL row position (two coefficient rows: X^T d1 and (X o X)^T d2 are the library's weighted products) and to
// LDS; per group the 2 K segmented sums [sum d1 z_k | sum d2 z_k^2], thread t < 2 K owning column t, the tile's rows walked in
// order and flushed at every change of group as the rows kernel flushes (gs_flush_dst at ncol = 2 K; glmm_fixup_kernel adds the
// partial rows in tile order); per tile the two partial scalars sum w E h_l and sum w E h_ll (vpart[tile], vpart[n_tiles + tile]),
// finished in tile order by sum_partials_kernel.  No border, no local blocks, no products table.  No atomics: fixed-order sums,
// bitwise reproducible.  Empty groups keep the zeros the caller wrote; a row of weight zero contributes w x = 0 exactly.
template <class DLik>
__global__ __launch_bounds__(256)
void glmm_disp_rows_kernel(i64 N, int P, int Kz, i64 G, const double* __restrict__ X, const double* __restrict__ Z,
                           const double* __restrict__ w, const i64* __restrict__ perm, const i64* __restrict__ offs,
                           const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                           const double* __restrict__ rg, typename DLik::Args la, double* __restrict__ coef, i64 NP,
                           double* __restrict__ gsum, double* __restrict__ part, double* __restrict__ vpart)
{
    __shared__ double xs[GLMM_T * GS_XS], cf[2 * GLMM_T], ms[64], vs[64], red[8];
    __shared__ typename DLik::Lds lik;
    __shared__ i64 s_row[GLMM_T];
    __shared__ int s_gid[GLMM_T], s_whole[GLMM_T];
    const int tid = threadIdx.x;
    const int ncol = 2 * Kz;
    DLik::init(lik, la, tid);
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    // the column of this thread (tid < 2 K): d1 z_k for tid < K, d2 z_k^2 behind them
    const bool has_col = tid < ncol, c_sq = tid >= Kz;
    const int c_z = P + (c_sq ? tid - Kz : tid), c_row = c_sq ? 1 : 0;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(N - t0 < GLMM_T ? N - t0 : GLMM_T);
        __syncthreads();                                                 // the previous tile is consumed (and the nodes, m, v are in place)
        gs_stage_sorted_tile<DLik, GS_XS>(tid, t0, rows, P, Kz, G, X, Z, perm, offs, la, lik, xs, s_row, s_gid, s_whole);
        double rho = 0.0, s = 0.0;
        if (row < rows) {
            const double* xr = xs + row * GS_XS;
            for (int j = q4; j < P; j += 4) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
            if (q4 < Kz) {
                const i64 gk = (i64)s_gid[row] * Kz + q4;
                const double z = xr[P + q4];
                rho += z * eg[gk]; s += z * z * rg[gk];
            }
        }
        rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
        rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
        const DispMoments mo = DLik::dmoments(lik, la, row < rows, q4, rho, s);
        double c1 = 0.0, c2 = 0.0;
        if (q4 == 0) {
            double d1 = 0.0, d2 = 0.0;
            if (row < rows) {
                const i64 pr = s_row[row];
                const double wi = w[pr];
                d1 = wi * mo.t1; d2 = wi * 0.5 * mo.t2;
                c1 = wi * mo.hl; c2 = wi * mo.hll;
                coef[pr] = d1; coef[NP + pr] = d2;
            }
            cf[row] = d1; cf[GLMM_T + row] = d2;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { c1 += __shfl_xor(c1, off); c2 += __shfl_xor(c2, off); }
        if ((tid & 63) == 0) { red[tid >> 6] = c1; red[4 + (tid >> 6)] = c2; }
        __syncthreads();
        if (tid == 0) {
            vpart[tile] = (red[0] + red[1]) + (red[2] + red[3]);
            vpart[n_tiles + tile] = (red[4] + red[5]) + (red[6] + red[7]);
        }
        // segmented sums over the tile's rows, in row order
        if (has_col) {
            double acc = 0.0;
            int run_start = 0;
            for (int rr = 0; rr < rows; ++rr) {
                double z = xs[rr * GS_XS + c_z];
                if (c_sq) z *= z;
                acc += cf[c_row * GLMM_T + rr] * z;
                const int g = s_gid[rr];
                if (rr == rows - 1 || s_gid[rr + 1] != g) {
                    gs_flush_dst(s_whole[rr], g, tile, run_start, ncol, gsum, part)[tid] = acc;
                    acc = 0.0; run_start = rr + 1;
                }
            }
        }
    }
}

template <class DLik>
static int gs_launch_disp(lrvb_ctx* c, int Kz, typename DLik::Args la, const double* m, const double* vb, const double* eg, const double* rg,
                          double* coef, i64 NP, double* gsum, double* part, double* vpart) {
    const i64 N = c->N, G = c->n_groups;
    if (c->P > 64 || !DLik::args_ok(la)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "%s", DLik::LIMITS);
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    const double* Z = c->gz.p;
    LRVB_TRY(gs_with_K(Kz, DLik::LIMITS, [&](auto) {
        hipLaunchKernelGGL(glmm_disp_rows_kernel<DLik>, dim3(glmm_grid(N)), dim3(256), 0, c->stream, N, (int)c->P, Kz, G, (const double*)c->X.p, Z,
                           (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, la, coef, NP, gsum, part, vpart);
    }));
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, 2 * Kz, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// `lik` is the likelihood of the family's terms entry (GLMM_BETA, GLMM_GAMMA, GLMM_CENSNORMAL, or GLMM_BINOMIAL with the logit link: NB2), `disp` the resident
// dispersion; coef 2 x NP (zeroed by the caller), gsum G x 2 K (zeroed by the caller), part 2 x 2 K and vpart 2 doubles per tile.
int launch_glmm_disp_rows(lrvb_ctx* c, const GlmmLik& lik, const double* disp, int Kz, const double* m, const double* vb, const double* eg,
                          const double* rg, double* coef, i64 NP, double* gsum, double* part, double* vpart) {
    const LogisticLik::Args q{lik.gx, lik.gw, lik.n_nodes};
    if (lik.kind == GLMM_BETA)
        return gs_launch_disp<BetaDispLik>(c, Kz, BetaDispLik::Args{q, lik.off, disp, lik.y}, m, vb, eg, rg, coef, NP, gsum, part, vpart);
    if (lik.kind == GLMM_GAMMA)
        return gs_launch_disp<GammaDispLik>(c, Kz, GammaDispLik::Args{lik.off, disp, lik.y}, m, vb, eg, rg, coef, NP, gsum, part, vpart);
    if (lik.kind == GLMM_CENSNORMAL)
        return gs_launch_disp<CensNormalDispLik>(c, Kz, CensNormalDispLik::Args{q, lik.off, disp, lik.y, lik.cens}, m, vb, eg, rg, coef, NP, gsum, part, vpart);
    if (lik.kind == GLMM_BINOMIAL && lik.link == GLMM_LINK_LOGIT)
        return gs_launch_disp<NegBinDispLik>(c, Kz, NegBinDispLik::Args{q, lik.off, lik.trials, disp, lik.y}, m, vb, eg, rg, coef, NP, gsum, part, vpart);
    LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "the dispersion derivative is that of the Beta, the Gamma, the censored Gaussian and the negative binomial mixed model");
}

// ---- the derivatives in the thresholds of the ordinal model (lrvb_glmm_ordinal_threshold_terms) -------------
// ONE pass over the rows in group-sorted order on the head of glmm_disp_rows_kernel: the same tiles, the same staging, four lanes per
// row for rho and s by the same dot products, then OrdinalLik::thr_moments: E sigma, E sigma', E sigma'' at t - hi and at lo - t.
// A row of category y touches TWO of the T thresholds, its hi (index y, where y < T) and its lo (index y - 1, where y >= 1).  With
// r = 1 / expm1(D) and c = e^-D / expm1(-D)^2 (both 0 at the sentinel D = +inf of an end category) the row holds, times its weight,
//   g_hi = -E sigma(t - hi) - r,  g_lo = E sigma(lo - t) + r,  H_hi,hi = E sigma'(t - hi) + c,  H_lo,lo = E sigma'(lo - t) + c,  H_lo,hi = -c,
//   d1_hi = -E sigma'(t - hi),  d2_hi = -E sigma''(t - hi) / 2,  d1_lo = -E sigma'(lo - t),  d2_lo = +E sigma''(lo - t) / 2
// (d1 the derivative in rho of the row's threshold gradient, d2 the one in s, by Stein's identity).  Unlike a scalar dispersion there is
// no coefficient VECTOR per threshold to hand to the library's products: the products with x are formed here.
//   cross_global  T x 2 P accumulators per workgroup in LDS, [sum d1 x | sum d2 x o x] per threshold.  Thread c < 2 P owns column c of
//                 all T rows: it walks the tile's rows in order and adds to the rows of the two thresholds the row touches -- the
//                 threads of a wave write consecutive words of ONE accumulator row, whichever row the data picks.  The accumulators
//                 persist over the workgroup's tiles; each workgroup writes one block, glmm_thr_finish_kernel adds them in block order.
//   cross_local   per group the T x 2 K segmented sums [sum d1 z | sum d2 z o z], thread 128 + u owning column u = j 2 K + c, flushed
//                 at every change of group through gs_flush_dst at ncol = 2 K T, the partial rows added by glmm_fixup_kernel.
//   g, H          per tile 3 T partial scalars (g | H diagonal | H off-diagonal, the last slot of the third unused), thread q < 3 T
//                 summing the tile's rows in order; vpart[q n_tiles + tile], finished in tile order by sum_partials_kernel.
// No atomics: every sum has a fixed order for a given grid, bitwise reproducible.  A row of weight zero contributes exact zeros.
__global__ __launch_bounds__(256)
void glmm_thr_rows_kernel(i64 N, int P, int Kz, i64 G, const double* __restrict__ X, const double* __restrict__ Z,
                          const double* __restrict__ w, const i64* __restrict__ perm, const i64* __restrict__ offs,
                          const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                          const double* __restrict__ rg, OrdinalLik::Args la, double* __restrict__ gsum, double* __restrict__ part,
                          double* __restrict__ vpart, double* __restrict__ cpart)
{
    __shared__ double xs[GLMM_T * GS_XS], rv[9 * GLMM_T], acc[OrdinalLik::MAX_T * 128], ms[64], vs[64];
    __shared__ OrdinalLik::Lds lik;
    __shared__ i64 s_row[GLMM_T];
    __shared__ int s_gid[GLMM_T], s_whole[GLMM_T];
    const int tid = threadIdx.x;
    const int T = la.T, P2 = 2 * P, K2 = 2 * Kz, ncl = K2 * T;
    OrdinalLik::init(lik, la, tid);
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    for (int e = tid; e < T * P2; e += 256) acc[e] = 0.0;
    const i64 n_tiles = (N + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    // thread c < 2 P: column c of cross_global (x_c for c < P, x_{c-P}^2 behind them)
    const bool g_col = tid < P2, g_sq = tid >= P;
    const int g_x = g_sq ? tid - P : tid;
    // thread 128 + u, u < 2 K T: column u = j 2 K + c of cross_local (z_c for c < K, z_{c-K}^2 behind them)
    const int lu = tid - 128;
    const bool l_col = lu >= 0 && lu < ncl;
    const int l_j = l_col ? lu / K2 : 0, l_c = l_col ? lu - l_j * K2 : 0;
    const bool l_sq = l_c >= Kz;
    const int l_z = P + (l_sq ? l_c - Kz : l_c);
    // thread q < 3 T: scalar slot q = b T + j
    const int s_b = tid / T, s_j = tid - s_b * T;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(N - t0 < GLMM_T ? N - t0 : GLMM_T);
        __syncthreads();                                                 // the previous tile is consumed (and the nodes, the table, m, v are in place)
        gs_stage_sorted_tile<OrdinalLik, GS_XS>(tid, t0, rows, P, Kz, G, X, Z, perm, offs, la, lik, xs, s_row, s_gid, s_whole);
        double rho = 0.0, s = 0.0;
        if (row < rows) {
            const double* xr = xs + row * GS_XS;
            for (int j = q4; j < P; j += 4) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
            if (q4 < Kz) {
                const i64 gk = (i64)s_gid[row] * Kz + q4;
                const double z = xr[P + q4];
                rho += z * eg[gk]; s += z * z * rg[gk];
            }
        }
        rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
        rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
        const OrdinalLik::ThrMoments mo = OrdinalLik::thr_moments(lik, la, row < rows, q4, rho, s);
        if (q4 == 0) {
            double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (row < rows) {
                const double wi = w[s_row[row]];
                const double D = OrdinalLik::row_delta(lik, row);         // +inf on an end category: r = c = 0
                const double em = exp(-D), dm = expm1(-D);
                const double r = 1.0 / expm1(D), c = em / (dm * dm);      // in e^-D: e^D overflows at D = 710
                v[0] = -(wi * mo.a1); v[1] = -(wi * 0.5 * mo.a2); v[2] = -(wi * mo.b1); v[3] = wi * 0.5 * mo.b2;
                v[4] = wi * (-mo.a0 - r); v[5] = wi * (mo.b0 + r); v[6] = wi * (mo.a1 + c); v[7] = wi * (mo.b1 + c); v[8] = -(wi * c);
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) rv[i * GLMM_T + row] = v[i];
        }
        __syncthreads();
        if (g_col) {
            const double* dh = rv + (g_sq ? 1 : 0) * GLMM_T;
            const double* dl = rv + (g_sq ? 3 : 2) * GLMM_T;
            for (int rr = 0; rr < rows; ++rr) {
                double x = xs[rr * GS_XS + g_x];
                if (g_sq) x *= x;
                const int j = lik.s_cat[rr];                              // in [0, T]: clamped where it was staged
                if (j < T) acc[j * P2 + tid] += dh[rr] * x;
                if (j >= 1) acc[(j - 1) * P2 + tid] += dl[rr] * x;
            }
        } else if (l_col) {
            const double* dh = rv + (l_sq ? 1 : 0) * GLMM_T;
            const double* dl = rv + (l_sq ? 3 : 2) * GLMM_T;
            double a = 0.0;
            int run_start = 0;
            for (int rr = 0; rr < rows; ++rr) {
                double z = xs[rr * GS_XS + l_z];
                if (l_sq) z *= z;
                const int j = lik.s_cat[rr];
                if (j == l_j) a += dh[rr] * z;
                if (j == l_j + 1) a += dl[rr] * z;
                const int g = s_gid[rr];
                if (rr == rows - 1 || s_gid[rr + 1] != g) {
                    gs_flush_dst(s_whole[rr], g, tile, run_start, ncl, gsum, part)[lu] = a;
                    a = 0.0; run_start = rr + 1;
                }
            }
        }
        if (tid < 3 * T) {
            const double* vh = rv + (s_b == 0 ? 4 : 6) * GLMM_T;
            const double* vl = rv + (s_b == 0 ? 5 : 7) * GLMM_T;
            const double* vo = rv + 8 * GLMM_T;
            double a = 0.0;
            for (int rr = 0; rr < rows; ++rr) {
                const int j = lik.s_cat[rr];
                if (s_b < 2) {
                    if (j == s_j) a += vh[rr];
                    if (j == s_j + 1) a += vl[rr];
                } else if (j == s_j + 1 && j < T) a += vo[rr];           // the pair (alpha_j, alpha_j+1) of an interior category
            }
            vpart[(i64)tid * n_tiles + tile] = a;
        }
    }
    __syncthreads();
    for (int e = tid; e < T * P2; e += 256) cpart[(i64)blockIdx.x * (T * P2) + e] = acc[e];
}

// out[i] = sum over the nblk workgroup blocks, in block order
__global__ __launch_bounds__(256)
void glmm_thr_finish_kernel(int nblk, int n, const double* __restrict__ cpart, double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    for (int b = 0; b < nblk; ++b) a += cpart[(i64)b * n + i];
    out[i] = a;
}

unsigned glmm_thr_grid(i64 N) { return glmm_grid(N); }

// `lik` is the ordinal likelihood on the device (nodes, offset, y, the table); gsum G x 2 K T (zeroed by the caller), part 2 x 2 K T
// per tile, vpart 3 T per tile, cpart T x 2 P per workgroup of glmm_thr_grid(N), cross T x 2 P.
int launch_glmm_thr_rows(lrvb_ctx* c, const GlmmLik& lik, int Kz, const double* m, const double* vb, const double* eg, const double* rg,
                         double* gsum, double* part, double* vpart, double* cpart, double* cross) {
    const i64 N = c->N, G = c->n_groups;
    const OrdinalLik::Args la{{lik.gx, lik.gw, lik.n_nodes}, lik.off, lik.y, lik.thr, lik.T};
    if (lik.kind != GLMM_ORDINAL || c->P > 64 || Kz < 1 || Kz > 4 || !OrdinalLik::args_ok(la)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "%s", OrdinalLik::LIMITS);
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    const unsigned grid = glmm_thr_grid(N);
    const int ncl = 2 * Kz * lik.T, ncg = lik.T * 2 * (int)c->P;
    hipLaunchKernelGGL(glmm_thr_rows_kernel, dim3(grid), dim3(256), 0, c->stream, N, (int)c->P, Kz, G, (const double*)c->X.p, (const double*)c->gz.p,
                       (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, la, gsum, part, vpart, cpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncl, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_thr_finish_kernel, dim3((unsigned)((ncg + 255) / 256)), dim3(256), 0, c->stream, (int)grid, ncg, (const double*)cpart, cross);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// A = L L^T of one local block from its upper triangle a (row-major), L row-major into Ls; false where a pivot is not positive
// (the factor then continues with 1 in its place).  One thread; shared by the elimination and by the two substitution kernels
// of the solve below, so that all three see the same L bit for bit.
template <int K2>
__device__ __forceinline__ bool gs_local_chol(const double* __restrict__ a, double* __restrict__ Ls)
{
    double A[K2][K2];
    int t = 0;
#pragma unroll
    for (int i = 0; i < K2; ++i)
#pragma unroll
        for (int j = i; j < K2; ++j) A[i][j] = a[t++];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < K2; ++j) {                                       // column j of L, kept in A[j][j ..] (L_ij = A[j][i], i >= j)
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[k][j] * A[k][j];
        if (!(d > 0.0)) { ok = false; d = 1.0; }
        const double l = sqrt(d);
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < K2; ++i) {
            double sij = A[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) sij -= A[k][i] * A[k][j];
            A[j][i] = sij / l;
        }
    }
#pragma unroll
    for (int i = 0; i < K2; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Ls[i * K2 + j] = A[j][i];
    return ok;
}

// ---- elimination of the 2 K G local parameters ---------------------------------------------------------------------------------
// Per group g: A_g (2 K x 2 K, the complete local block in the coordinates that are eliminated, its K (2 K + 1) upper-triangle
// entries row-major from the host) = L L^T, and the 2 K border rows over the R = 2 P + 3 K coupled global coordinates
// [m (P) | v (P) | e_mu_0, a_0, b_0, .., e_mu_{K-1}, a_{K-1}, b_{K-1}]:
//   row e_gk = f_ek [sum c11 z_k x | sum c12 z_k x o x | closed (3) in the columns of k, zero in those of the other components]
//   row r_gk = f_rk [sum c12 z_k^2 x | sum c22 z_k^2 x o x | closed (3) ...]
// from the RESIDENT group sums.  Thread 0 factors A_g into LDS; thread c then takes column c through the forward substitution
// and writes U_g = L^-1 C_g (2 K x R), so that sum_g C_g^T A_g^-1 C_g = U^T U is one Gram over 2 K G rows.  A pivot that is not
// positive raises the flag.
template <int KZ>
__global__ __launch_bounds__(256)
void glmm_slopes_schur_rows_kernel(i64 G, int P, const double* __restrict__ gsum, const double* __restrict__ loc /* G x K (2 K + 1) */,
                                   const double* __restrict__ scale /* G x 2 K */, const double* __restrict__ closed /* G x 2 K x 3 */,
                                   double* __restrict__ U, int ldu, int* __restrict__ bad)
{
    constexpr int K2 = 2 * KZ, NT = KZ * (K2 + 1), nsc = K2 + NT;
    __shared__ double Ls[K2 * K2], fs[K2], cs[K2 * 3];
    const i64 g = blockIdx.x;
    if (g >= G) return;
    const int ncol = nsc + 4 * KZ * P, R = 2 * P + 3 * KZ;
    const int tid = threadIdx.x;
    if (tid == 0 && !gs_local_chol<K2>(loc + g * NT, Ls)) *bad = 1;
    if (tid >= 64 && tid < 64 + K2) fs[tid - 64] = scale[g * K2 + (tid - 64)];
    if (tid >= 128 && tid < 128 + K2 * 3) cs[tid - 128] = closed[g * K2 * 3 + (tid - 128)];
    __syncthreads();
    const double* gs = gsum + g * ncol + nsc;
    for (int c = tid; c < R; c += 256) {
        double u[K2];
#pragma unroll
        for (int i = 0; i < K2; ++i) {
            const int k = i < KZ ? i : i - KZ;
            double ce;
            if (c < P) ce = gs[((i < KZ ? 0 : KZ) + k) * P + c];
            else if (c < 2 * P) ce = gs[((i < KZ ? K2 : 3 * KZ) + k) * P + (c - P)];
            else { const int q = c - 2 * P, kc = q / 3; ce = kc == k ? cs[i * 3 + (q - 3 * kc)] : 0.0; }
            double t = fs[i] * ce;
#pragma unroll
            for (int j = 0; j < i; ++j) t -= Ls[i * K2 + j] * u[j];
            u[i] = t / Ls[i * K2 + i];
            U[(g * K2 + i) * ldu + c] = u[i];
        }
    }
}

int launch_glmm_slopes_schur_rows(lrvb_ctx* c, int Kz, const double* gsum, const double* loc, const double* scale, const double* closed,
                                  double* U, int ldu, int* bad) {
    const i64 G = c->n_groups;
    const dim3 grid((unsigned)G), block(256);
    const int P = (int)c->P;
    return gs_with_K(Kz, "logistic mixed model with slopes: 1 <= K <= 4", [&](auto k) {
        hipLaunchKernelGGL(glmm_slopes_schur_rows_kernel<decltype(k)::value>, grid, block, 0, c->stream, G, P, gsum, loc, scale, closed, U, ldu, bad);
    });
}

// ---- elimination with a dense closed border (lrvb_glmm_arrow_schur) -----------------------------------------
// The kernel above with the closed border generalised: R = 2 P + NC coupled coordinates [m (P) | v (P) | NC closed columns in the
// caller's order], and the closed entries of group g affine in its K-vector d_g,
//   closed_g[i][c] = A0[i][c] + sum_l A1[i][l][c] d_gl      (A0: 2 K x NC, A1: 2 K x K x NC, row-major, shared by all groups),
// so that G K doubles of d cross the bus and not G 2 K NC of closed rows.  The two tables and d_g are staged in LDS (at most
// 8 x 16 + 8 x 4 x 16 + 4 doubles) by the waves 1..3 while thread 0 of wave 0 factors the block (gs_local_chol: the same L, bit
// for bit); thread c then forms column c of the 2 K border rows -- the group sums for c < 2 P, the affine form in the order
// l = 0 .. K - 1 for the closed columns, both times the chain factor -- and takes it through the forward substitution.  The
// closed columns read LDS only: the tables as a broadcast per (i, l) row, consecutive threads consecutive doubles.
constexpr int GSA_NCMAX = 16;               // closed columns: K + 1 + K (K + 1) / 2 = 15 at K = 4

template <int KZ>
__global__ __launch_bounds__(256)
void glmm_arrow_schur_rows_kernel(i64 G, int P, int NC, const double* __restrict__ gsum, const double* __restrict__ loc /* G x K (2 K + 1) */,
                                  const double* __restrict__ scale /* G x 2 K */, const double* __restrict__ dloc /* G x K */,
                                  const double* __restrict__ A0 /* 2 K x NC */, const double* __restrict__ A1 /* 2 K x K x NC */,
                                  double* __restrict__ U, int ldu, int* __restrict__ bad)
{
    constexpr int K2 = 2 * KZ, NT = KZ * (K2 + 1), nsc = K2 + NT;
    __shared__ double Ls[K2 * K2], fs[K2], ds[KZ], A0s[K2 * GSA_NCMAX], A1s[K2 * KZ * GSA_NCMAX];
    const i64 g = blockIdx.x;
    if (g >= G) return;
    const int ncol = nsc + 4 * KZ * P, R = 2 * P + NC;
    const int tid = threadIdx.x;
    if (tid == 0 && !gs_local_chol<K2>(loc + g * NT, Ls)) *bad = 1;
    if (tid >= 64) {
        const int t = tid - 64;
        if (t < K2) fs[t] = scale[g * K2 + t];
        if (t < KZ) ds[t] = dloc[g * KZ + t];
        for (int q = t; q < K2 * NC; q += 192) A0s[q] = A0[q];
        for (int q = t; q < K2 * KZ * NC; q += 192) A1s[q] = A1[q];
    }
    __syncthreads();
    const double* gs = gsum + g * ncol + nsc;
    for (int c = tid; c < R; c += 256) {
        double u[K2];
#pragma unroll
        for (int i = 0; i < K2; ++i) {
            const int k = i < KZ ? i : i - KZ;
            double ce;
            if (c < P) ce = gs[((i < KZ ? 0 : KZ) + k) * P + c];
            else if (c < 2 * P) ce = gs[((i < KZ ? K2 : 3 * KZ) + k) * P + (c - P)];
            else {
                const int q = c - 2 * P;
                ce = A0s[i * NC + q];
#pragma unroll
                for (int l = 0; l < KZ; ++l) ce += A1s[(i * KZ + l) * NC + q] * ds[l];
            }
            double t = fs[i] * ce;
#pragma unroll
            for (int j = 0; j < i; ++j) t -= Ls[i * K2 + j] * u[j];
            u[i] = t / Ls[i * K2 + i];
            U[(g * K2 + i) * ldu + c] = u[i];
        }
    }
}

int launch_glmm_arrow_schur_rows(lrvb_ctx* c, int Kz, int NC, const double* gsum, const double* loc, const double* scale, const double* dloc,
                                 const double* A0, const double* A1, double* U, int ldu, int* bad) {
    const i64 G = c->n_groups;
    const dim3 grid((unsigned)G), block(256);
    const int P = (int)c->P;
    if (NC < Kz || NC > GSA_NCMAX) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "mixed model with a dense closed border: K <= NC <= 16");
    return gs_with_K(Kz, "mixed model with a dense closed border: 1 <= K <= 4", [&](auto k) {
        hipLaunchKernelGGL(glmm_arrow_schur_rows_kernel<decltype(k)::value>, grid, block, 0, c->stream, G, P, NC, gsum, loc, scale, dloc, A0, A1,
                           U, ldu, bad);
    });
}

// ---- the two substitution passes of the device-resident block-arrow solve ---------------------------------
// One workgroup per group.  Thread 0 re-derives L_g from the resident copy of the uploaded block (gs_local_chol: the L that
// U_g = L_g^-1 C_g was formed with) into LDS; thread t then owns the columns q = t, t + blockDim.x, .. of the group's 2 K x Q
// slab (row-major: consecutive threads touch consecutive doubles of each of its 2 K rows), keeps the 2 K values of a column
// in registers and runs one triangular substitution on them.  The contractions over the groups (U^T T) and over the coupled
// rows (U x) are the library's GEMM on the fp64 matrix cores, launched by the entry points.  Only blocks whose factorisation
// succeeded get here (the entry points ask for a valid resident factor).  No atomics; every output has one writer.
template <int KZ>
__global__ __launch_bounds__(256)
void glmm_slopes_solve_forward_kernel(i64 G, i64 Q, const double* __restrict__ loc /* G x K (2 K + 1) */,
                                      double* __restrict__ T /* G x 2 K x Q: R_local in, L^-1 R_local out */)
{
    constexpr int K2 = 2 * KZ, NT = KZ * (K2 + 1);
    __shared__ double Ls[K2 * K2];
    const i64 g = blockIdx.x;
    if (g >= G) return;
    if (threadIdx.x == 0) gs_local_chol<K2>(loc + g * NT, Ls);
    __syncthreads();
    double* tg = T + g * K2 * Q;
    for (i64 q = threadIdx.x; q < Q; q += blockDim.x) {
        double t[K2];
#pragma unroll
        for (int i = 0; i < K2; ++i) {
            double v = tg[i * Q + q];
#pragma unroll
            for (int j = 0; j < i; ++j) v -= Ls[i * K2 + j] * t[j];
            t[i] = v / Ls[i * K2 + i];
            tg[i * Q + q] = t[i];
        }
    }
}

template <int KZ>
__global__ __launch_bounds__(256)
void glmm_slopes_solve_back_kernel(i64 G, i64 Q, const double* __restrict__ loc, const double* __restrict__ T /* G x 2 K x Q */,
                                   double* __restrict__ W /* G x 2 K x Q: U_g x in, L^-T (T_g - U_g x) out */)
{
    constexpr int K2 = 2 * KZ, NT = KZ * (K2 + 1);
    __shared__ double Ls[K2 * K2];
    const i64 g = blockIdx.x;
    if (g >= G) return;
    if (threadIdx.x == 0) gs_local_chol<K2>(loc + g * NT, Ls);
    __syncthreads();
    const double* tg = T + g * K2 * Q;
    double* wg = W + g * K2 * Q;
    for (i64 q = threadIdx.x; q < Q; q += blockDim.x) {
        double x[K2];
#pragma unroll
        for (int i = 0; i < K2; ++i) x[i] = tg[i * Q + q] - wg[i * Q + q];
#pragma unroll
        for (int i = K2 - 1; i >= 0; --i) {
            double v = x[i];
#pragma unroll
            for (int j = i + 1; j < K2; ++j) v -= Ls[j * K2 + i] * x[j];
            x[i] = v / Ls[i * K2 + i];
            wg[i * Q + q] = x[i];
        }
    }
}

int launch_glmm_slopes_solve(lrvb_ctx* c, int Kz, bool back, i64 Q, const double* loc, double* T, double* W) {
    const i64 G = c->n_groups;
    const dim3 grid((unsigned)G), block(Q <= 64 ? 64 : (Q <= 128 ? 128 : 256));
    return gs_with_K(Kz, "logistic mixed model with slopes: 1 <= K <= 4", [&](auto k) {
        constexpr int KK = decltype(k)::value;
        if (back) hipLaunchKernelGGL(glmm_slopes_solve_back_kernel<KK>, grid, block, 0, c->stream, G, Q, loc, (const double*)T, W);
        else hipLaunchKernelGGL(glmm_slopes_solve_forward_kernel<KK>, grid, block, 0, c->stream, G, Q, loc, T);
    });
}

// ---- streamed weight influence (lrvb_glmm_slopes_obs_influence / lrvb_glmm_poisson_obs_influence) ---------
// out[n - n0][q] = a1' (x_n . A_m[q] + sum_k z_nk A_e[q, g(n), k]) + a2' ((x_n o x_n) . A_v[q] + sum_k z_nk^2 A_r[q, g(n), k]),
// a1' = psi_rho - y_n (Lik::MINUS_Y; the two links hand over a1' = E H' whole), a2' = psi_s PER UNIT WEIGHT (w_n does not enter).  Built like glmm_infl_rows_kernel (k_glmm.hip): ONE pass
// over the rows n0..n1 in their original order, X and Z read once for any Q; a workgroup (4 waves) walks tiles of GLMM_T = 64 rows:
//   1. the tile (contiguous in X) is staged in LDS, row stride GSI_XS, the row's K values of z behind its x columns (columns
//      P .. P + K - 1, as glmm_slopes_rows_kernel stages them);
//   2. four lanes share a row for the two dot products (lane q4 also takes the z column q4) and the likelihood's Lik::infl (the
//      quadrature: only E g1 and E g2 are formed; or one exp), and a1', a2' go to LDS;
//   3. wave w owns the rows 16 w .. 16 w + 15.  Per block of 16 outputs the contractions X A_m^T and (X o X) A_v^T run as
//      16 x 16 x 4 fp64 MFMA tiles, two accumulator chains each, x o x squared in a register.  The B operand is zero past Q and
//      past P, so the staged z columns (and whatever lies behind them) that the last k-step reads meet zeros;
//   4. epilogue, in the D layout (register r <-> row (l >> 4) + 4 r, column l & 15): the 2 K gathered values of A_local
//      (G x 2 K x Q: 16 consecutive doubles for the 16 lanes of a block), weighted by z_nk and z_nk^2 from the staged row, are
//      added, the two halves are combined with a1', a2', and 16 consecutive doubles per row are written.
// The group-dependent term CANNOT go through the matrix cores: the B operand of an MFMA tile is shared by its 16 rows, and those
// rows belong to different groups.  K is a runtime value: the epilogue is a loop over scalars, no indexed register array.
// With Q <= 16 the B fragments are loaded once per workgroup and stay in registers; with more outputs the blocks of 16 are a
// loop INSIDE the tile.  No atomics, no group walk.
//
// GSI_XS.  Bank of a double at index a: a mod 32 (ds_read_b64: 64 dword banks, the two 32-lane halves separately).
//   (a) MFMA operand: lane (i = l & 15, k = l >> 4) reads row i, column 4 kk + k; a half holds i = 0..15, k in {0, 1} (or
//       {2, 3}): banks i S + k (+ const) must be 32 different values, so S mod 32 = 2 x an odd number: i S runs through the
//       16 even residues.  Stride 66 of k_glmm.hip is too short for 64 + 4 columns; 68 puts rows i and i + 8 on one bank (2-way).
//   (b) dot products: a half holds 8 rows x 4 lanes.  With lane q4 on the columns q4, q4 + 4, .. (k_glmm.hip) the banks are
//       row S + q4: different only if S = 4 mod 8 -- never together with (a) (stride 66 is 2-way there).
//   S = 70 = 6 mod 32 meets (a); the row offsets 6 row mod 32, row = 0..7, are {0, 6, 12, 18, 24, 30, 4, 10}: all even, and no
//   two of them 16 apart.  So the four lanes of a row take the columns c0 + 2 t + 32 h, c0 = {0, 1, 16, 17}[q4], t = 0..7,
//   h = 0, 1: at every step the 32 lanes read row S + {0, 1, 16, 17} + 2 t -- 32 different banks.  Both patterns are free of
//   conflicts.  (The single read of z, column P + q4, may be 2-way; it happens once per row.)
constexpr int GSI_XS = 70;

typedef double gsi_d4 __attribute__((ext_vector_type(4)));

// The per-row part both influence kernels share, with the z terms and the column map of GSI_XS: every one of the four lanes of the
// staged row xr returns e1 = psi_rho and e2 = 2 psi_s of the likelihood.  Called by all lanes.
template <class Lik>
__device__ __forceinline__ void gsi_psi_derivs(const double* xr, int row, bool live, int g, int q4, int P, int Kz, const double* ms,
                                               const double* vs, const double* __restrict__ eg, const double* __restrict__ rg,
                                               const typename Lik::Lds& lik, const typename Lik::Args& la, double& e1, double& e2)
{
    const double o = Lik::row_shift(lik, row);                          // read ahead of the dot products, which hide its latency
    double rho = 0.0, s = 0.0;
    if (live) {
        for (int h = (q4 & 1) + 16 * (q4 >> 1); h < P; h += 32)
            for (int j = h; j < h + 16 && j < P; j += 2) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
        if (q4 < Kz) {
            const i64 gk = (i64)g * Kz + q4;
            const double z = xr[P + q4];
            rho += z * eg[gk]; s += z * z * rg[gk];
        }
    }
    rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
    rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
    Lik::infl(lik, la, o, live, q4, rho, s, e1, e2);
}

template <class Lik>
__device__ __forceinline__
void gsi_infl_rows(i64 n0, i64 R /* rows of the window */, int P, int Kz, const double* __restrict__ X,
                   const double* __restrict__ Z, const double* __restrict__ y, const int* __restrict__ gid,
                   const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                   const double* __restrict__ rg, typename Lik::Args la,
                   const double* __restrict__ Ag /* Q x 2 P */, const double* __restrict__ Al /* G x 2 K x Q */, int Q,
                   double* __restrict__ out /* R x Q */)
{
    __shared__ double xs[GLMM_T * GSI_XS], a1s[GLMM_T], a2s[GLMM_T], ms[64], vs[64];
    __shared__ typename Lik::Lds lik;
    __shared__ int s_gid[GLMM_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    Lik::init(lik, la, tid);
    if (tid < 64) { ms[tid] = tid < P ? m[tid] : 0.0; vs[tid] = tid < P ? vb[tid] : 0.0; }
    for (int e = tid; e < GLMM_T * GSI_XS; e += 256) xs[e] = 0.0;          // what no tile writes stays zero (finite) for the whole kernel
    const int KS = (P + 3) >> 2;                                         // k-steps of the contractions
    const int nqb = (Q + 15) >> 4;
    const int K2 = 2 * Kz;
    double bm[16], bv[16];
    auto load_b = [&](int qb) {
        const int q = 16 * qb + l15;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int k = 4 * kk + l4;
            const bool ok = q < Q && k < P;
            bm[kk] = ok ? Ag[(i64)q * 2 * P + k] : 0.0;
            bv[kk] = ok ? Ag[(i64)q * 2 * P + P + k] : 0.0;
        }
    };
    if (nqb == 1) load_b(0);
    const i64 n_tiles = (R + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(R - t0 < GLMM_T ? R - t0 : GLMM_T);
        __syncthreads();                                                 // the previous tile is consumed (and the nodes, m, v are in place)
        if (tid < GLMM_T) {
            s_gid[tid] = tid < rows ? gid[n0 + t0 + tid] : 0;
            Lik::stage_row(lik, la, tid, tid < rows, n0 + t0 + tid);
        }
        {
            const double* src = X + (n0 + t0) * (i64)P;
            for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * GSI_XS + cc] = src[e]; }
            const double* zsrc = Z + (n0 + t0) * (i64)Kz;
            for (int e = tid; e < rows * Kz; e += 256) { const int rr = e / Kz, cc = e - rr * Kz; xs[rr * GSI_XS + P + cc] = zsrc[e]; }
        }
        __syncthreads();
        double e1, e2;
        gsi_psi_derivs<Lik>(xs + row * GSI_XS, row, row < rows, s_gid[row], q4, P, Kz, ms, vs, eg, rg, lik, la, e1, e2);
        if (q4 == 0) {
            double k1 = 0.0, k2 = 0.0;
            if (row < rows) {
                if constexpr (Lik::MINUS_Y) k1 = e1 - y[n0 + t0 + row];
                else k1 = e1;                                            // a1' whole: the policy staged y itself
                k2 = 0.5 * e2;
            }
            a1s[row] = k1; a2s[row] = k2;
        }
        __syncthreads();
        // the two contractions of this wave's 16 rows
        const double* xa = xs + (16 * wave + l15) * GSI_XS + l4;
        for (int qb = 0; qb < nqb; ++qb) {
            if (nqb > 1) load_b(qb);
            gsi_d4 am0 = {0.0, 0.0, 0.0, 0.0}, am1 = am0, av0 = am0, av1 = am0;
#pragma unroll
            for (int kk = 0; kk < 16; kk += 2) {
                if (kk < KS) {
                    const double x = xa[4 * kk];
                    am0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, bm[kk], am0, 0, 0, 0);
                    av0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x * x, bv[kk], av0, 0, 0, 0);
                }
                if (kk + 1 < KS) {
                    const double x = xa[4 * kk + 4];
                    am1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, bm[kk + 1], am1, 0, 0, 0);
                    av1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x * x, bv[kk + 1], av1, 0, 0, 0);
                }
            }
            const int q = 16 * qb + l15;
            if (q < Q) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = 16 * wave + l4 + 4 * r;
                    if (rr < rows) {
                        const double* zr = xs + rr * GSI_XS + P;
                        const double* al = Al + (i64)s_gid[rr] * K2 * Q + q;
                        double le = 0.0, lr = 0.0;
                        for (int k = 0; k < Kz; ++k) {
                            const double z = zr[k];
                            le += z * al[(i64)k * Q]; lr += z * z * al[(i64)(Kz + k) * Q];
                        }
                        out[(t0 + rr) * (i64)Q + q] = a1s[rr] * ((am0[r] + am1[r]) + le) + a2s[rr] * ((av0[r] + av1[r]) + lr);
                    }
                }
            }
        }
    }
}

// The three entries of the walk above.  Each has its likelihood's arguments where that likelihood's kernel has always had them (the
// offset behind Z, the nodes behind rg): with ONE templated signature the Poisson instantiation loaded its kernel arguments and
// spilled its SGPRs differently and ran 0.7 to 1 % slower than before the merge.
__global__ __launch_bounds__(256)
void glmm_slopes_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                  const double* __restrict__ y, const int* __restrict__ gid, const double* __restrict__ m,
                                  const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                                  const double* __restrict__ gx, const double* __restrict__ gw, int nq, const double* __restrict__ Ag,
                                  const double* __restrict__ Al, int Q, double* __restrict__ out)
{
    gsi_infl_rows<LogisticLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {gx, gw, nq}, Ag, Al, Q, out);
}

__global__ __launch_bounds__(256)
void glmm_poisson_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                   const double* __restrict__ off, const double* __restrict__ y, const int* __restrict__ gid,
                                   const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                                   const double* __restrict__ rg, const double* __restrict__ Ag, const double* __restrict__ Al, int Q,
                                   double* __restrict__ out)
{
    gsi_infl_rows<PoissonLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, off, Ag, Al, Q, out);
}

__global__ __launch_bounds__(256)
void glmm_binomial_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                    const double* __restrict__ off, const double* __restrict__ trials, const double* __restrict__ y,
                                    const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                    const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ gx,
                                    const double* __restrict__ gw, int nq, const double* __restrict__ Ag, const double* __restrict__ Al,
                                    int Q, double* __restrict__ out)
{
    gsi_infl_rows<BinomialLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {{gx, gw, nq}, off, trials}, Ag, Al, Q, out);
}

// The probit and the cloglog link: the arguments of the binomial entry; y is also what the policy stages.
template <int LINK>
__global__ __launch_bounds__(256)
void glmm_link_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                const double* __restrict__ off, const double* __restrict__ trials, const double* __restrict__ y,
                                const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ gx,
                                const double* __restrict__ gw, int nq, const double* __restrict__ Ag, const double* __restrict__ Al,
                                int Q, double* __restrict__ out)
{
    gsi_infl_rows<BinomialLinkLik<LINK>>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {{gx, gw, nq}, off, trials, y}, Ag, Al, Q, out);
}

// The zero-truncated Poisson model: the arguments of the binomial entry without the trials.
__global__ __launch_bounds__(256)
void glmm_ztpoisson_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                     const double* __restrict__ off, const double* __restrict__ y, const int* __restrict__ gid,
                                     const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                                     const double* __restrict__ rg, const double* __restrict__ gx, const double* __restrict__ gw, int nq,
                                     const double* __restrict__ Ag, const double* __restrict__ Al, int Q, double* __restrict__ out)
{
    gsi_infl_rows<TruncPoissonLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {{gx, gw, nq}, off}, Ag, Al, Q, out);
}

// The zero-truncated NB2 model: the arguments of the link entry, the dispersion in the place of the trials.
__global__ __launch_bounds__(256)
void glmm_ztnegbin_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                    const double* __restrict__ off, const double* __restrict__ disp, const double* __restrict__ y,
                                    const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                    const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ gx,
                                    const double* __restrict__ gw, int nq, const double* __restrict__ Ag, const double* __restrict__ Al,
                                    int Q, double* __restrict__ out)
{
    gsi_infl_rows<TruncNegBinLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {{gx, gw, nq}, off, disp, y}, Ag, Al, Q, out);
}

// The Beta model: the arguments of the zero-truncated NB2 entry; y holds logit(y).
__global__ __launch_bounds__(256)
void glmm_beta_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                const double* __restrict__ off, const double* __restrict__ disp, const double* __restrict__ y,
                                const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ gx,
                                const double* __restrict__ gw, int nq, const double* __restrict__ Ag, const double* __restrict__ Al,
                                int Q, double* __restrict__ out)
{
    gsi_infl_rows<BetaLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {{gx, gw, nq}, off, disp, y}, Ag, Al, Q, out);
}

// The Gamma model: the arguments of the Beta entry without the nodes; y holds log(y).
__global__ __launch_bounds__(256)
void glmm_gamma_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                 const double* __restrict__ off, const double* __restrict__ disp, const double* __restrict__ y,
                                 const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                 const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ Ag,
                                 const double* __restrict__ Al, int Q, double* __restrict__ out)
{
    gsi_infl_rows<GammaLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {off, disp, y}, Ag, Al, Q, out);
}

// The censored Gaussian model: the arguments of the Beta entry, the status behind y; y holds the responses.
__global__ __launch_bounds__(256)
void glmm_censnormal_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                      const double* __restrict__ off, const double* __restrict__ disp, const double* __restrict__ y,
                                      const double* __restrict__ cens, const int* __restrict__ gid, const double* __restrict__ m,
                                      const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                                      const double* __restrict__ gx, const double* __restrict__ gw, int nq, const double* __restrict__ Ag,
                                      const double* __restrict__ Al, int Q, double* __restrict__ out)
{
    gsi_infl_rows<CensNormalLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {{gx, gw, nq}, off, disp, y, cens}, Ag, Al, Q, out);
}

// The ordinal model: the offset, the categories (y) and the table of T + 2 cut points behind Z.
__global__ __launch_bounds__(256)
void glmm_ordinal_infl_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                   const double* __restrict__ off, const double* __restrict__ y, const double* __restrict__ thr, int T,
                                   const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                   const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ gx,
                                   const double* __restrict__ gw, int nq, const double* __restrict__ Ag, const double* __restrict__ Al,
                                   int Q, double* __restrict__ out)
{
    gsi_infl_rows<OrdinalLik>(n0, R, P, Kz, X, Z, y, gid, m, vb, eg, rg, {{gx, gw, nq}, off, y, thr, T}, Ag, Al, Q, out);
}

template <class Lik>
static int gs_launch_infl_rows(lrvb_ctx* c, int Kz, const double* Z, typename Lik::Args la, i64 n0, i64 n1, const int* gid, const double* m,
                               const double* vb, const double* eg, const double* rg, const double* Ag, const double* Al, i64 Q,
                               double* out) {
    if (c->P > 64 || Kz < 1 || Kz > 4 || !Lik::args_ok(la)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "%s", Lik::LIMITS);
    const i64 R = n1 - n0;
    if (R <= 0) return LRVB_OK;
    if constexpr (std::is_same<Lik, PoissonLik>::value)
        hipLaunchKernelGGL(glmm_poisson_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la, (const double*)c->y.p, gid, m, vb, eg, rg, Ag, Al, (int)Q, out);
    else if constexpr (std::is_same<Lik, BinomialLik>::value)
        hipLaunchKernelGGL(glmm_binomial_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la.off, (const double*)la.trials, (const double*)c->y.p, gid, m, vb, eg, rg, la.q.gx, la.q.gw,
                           la.q.nq, Ag, Al, (int)Q, out);
    else if constexpr (std::is_same<Lik, TruncPoissonLik>::value)
        hipLaunchKernelGGL(glmm_ztpoisson_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la.off, (const double*)c->y.p, gid, m, vb, eg, rg, la.q.gx, la.q.gw, la.q.nq, Ag, Al, (int)Q, out);
    else if constexpr (std::is_same<Lik, TruncNegBinLik>::value)
        hipLaunchKernelGGL(glmm_ztnegbin_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la.off, (const double*)la.disp, (const double*)la.y, gid, m, vb, eg, rg, la.q.gx, la.q.gw, la.q.nq,
                           Ag, Al, (int)Q, out);
    else if constexpr (std::is_same<Lik, BetaLik>::value)
        hipLaunchKernelGGL(glmm_beta_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la.off, (const double*)la.disp, (const double*)la.y, gid, m, vb, eg, rg, la.q.gx, la.q.gw, la.q.nq,
                           Ag, Al, (int)Q, out);
    else if constexpr (std::is_same<Lik, GammaLik>::value)
        hipLaunchKernelGGL(glmm_gamma_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la.off, (const double*)la.disp, (const double*)la.y, gid, m, vb, eg, rg, Ag, Al, (int)Q, out);
    else if constexpr (std::is_same<Lik, CensNormalLik>::value)
        hipLaunchKernelGGL(glmm_censnormal_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la.off, (const double*)la.disp, (const double*)la.y, (const double*)la.cens, gid, m, vb, eg, rg,
                           la.q.gx, la.q.gw, la.q.nq, Ag, Al, (int)Q, out);
    else if constexpr (std::is_same<Lik, OrdinalLik>::value)
        hipLaunchKernelGGL(glmm_ordinal_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)la.off, (const double*)la.y, (const double*)la.thr, la.T, gid, m, vb, eg, rg, la.q.gx, la.q.gw,
                           la.q.nq, Ag, Al, (int)Q, out);
    else if constexpr (gs_link_of<Lik>::value != GLMM_LINK_LOGIT)
        hipLaunchKernelGGL(glmm_link_infl_rows_kernel<gs_link_of<Lik>::value>, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz,
                           (const double*)c->X.p, Z, (const double*)la.off, (const double*)la.trials, (const double*)la.y, gid, m, vb, eg, rg,
                           la.q.gx, la.q.gw, la.q.nq, Ag, Al, (int)Q, out);
    else
        hipLaunchKernelGGL(glmm_slopes_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                           (const double*)c->y.p, gid, m, vb, eg, rg, la.gx, la.gw, la.nq, Ag, Al, (int)Q, out);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

int launch_glmm_slopes_infl_rows(lrvb_ctx* c, const GlmmLik& lik, int Kz, const double* Z, i64 n0, i64 n1, const int* gid, const double* m,
                                 const double* vb, const double* eg, const double* rg, const double* Ag, const double* Al, i64 Q,
                                 double* out) {
    if (!Z) { LRVB_TRY(gs_unit_design(lik, Kz)); return launch_glmm_infl_rows(c, n0, n1, gid, m, vb, eg, rg, lik.gx, lik.gw, lik.n_nodes, Ag, Al, Q, out); }
    return gs_with_lik(lik, [&](auto L, auto la) { return gs_launch_infl_rows<decltype(L)>(c, Kz, Z, la, n0, n1, gid, m, vb, eg, rg, Ag, Al, Q, out); });
}

// ---- group blocks of H^-1 and fitted values with their linear-response variance ---------------------------
// From the factor lrvb_glmm_slopes_schur left resident (the blocks as uploaded, U_g = L_g^-1 C_g), W = (S^-1)[rows, rows] (R x R)
// and the scaling s of the coupled rows, one workgroup per group writes the two blocks of H^-1 that a prediction in that group
// needs, row g of a G + 1 row buffer of K K + K P doubles, [Sigma_uu (K x K, row-major) | Sigma_ubeta (K x P, k-major)]:
//   1. thread 0: L_g by gs_local_chol (the L of the solve kernels, bit for bit);
//   2. thread c < R: column c of Y_g = L_g^-T (U_g diag(s)) by back substitution; its K leading rows (the rows of e_g.) go to LDS.
//      Threads 192 .. 192 + K - 1: column k of A_g^-1 = L^-T L^-1, its K leading entries to LDS;
//   3. thread c < R: column c of E_g = Y_g[:K] W, a sum over the R rows of W in their order (consecutive threads read consecutive
//      doubles of a row of W, R R <= 157 KB and so expected in L2; Y is an LDS broadcast);  Sigma_ubeta[k][j] = -E_g[k][j], j < P;
//   4. thread t < K K: Sigma_uu[k][l] = A_g^-1[k][l] + sum_c E_g[k][c] Y_g[l][c], in the order of c.
// Workgroup G writes the pseudo-group of a population-level prediction (u = mu): Sigma_uu = W[mu rows, mu rows], Sigma_ubeta =
// W[mu rows, :P].  E_g is formed here and not by the library's GEMM: Y_g would have to be written out (K G x ld(R) doubles, the
// size of half of U) and read back for 2 K R^2 flops per group, and the kernel would still be needed around it (a choice on
// these counts; the GEMM variant was not built or timed).  No atomics, one
// writer per output, fixed order: two calls give equal bits.
constexpr int GSP_RMAX = 2 * 64 + 3 * 4;   // coupled rows at P = 64, K = 4

template <int KZ>
__global__ __launch_bounds__(256)
void glmm_slopes_group_cov_kernel(i64 G, int P, const double* __restrict__ loc /* G x K (2 K + 1) */, const double* __restrict__ U,
                                  int ldu, const double* __restrict__ W /* R x R */, const double* __restrict__ s /* R */,
                                  double* __restrict__ out /* (G + 1) x (K K + K P) */)
{
    constexpr int K2 = 2 * KZ, NT = KZ * (K2 + 1), KK = KZ * KZ;
    __shared__ double Ls[K2 * K2], Ys[KZ * GSP_RMAX], Es[KZ * GSP_RMAX], Ai[KK];
    const i64 g = blockIdx.x;
    if (g > G) return;
    const int R = 2 * P + 3 * KZ, ncg = KK + KZ * P;
    const int tid = threadIdx.x;
    double* og = out + g * ncg;
    if (g == G) {
        for (int t = tid; t < ncg; t += 256) {
            if (t < KK) { const int k = t / KZ, l = t - k * KZ; og[t] = W[(i64)(2 * P + 3 * k) * R + 2 * P + 3 * l]; }
            else { const int u = t - KK, k = u / P, j = u - k * P; og[t] = W[(i64)(2 * P + 3 * k) * R + j]; }
        }
        return;
    }
    if (tid == 0) gs_local_chol<K2>(loc + g * NT, Ls);
    __syncthreads();
    for (int c = tid; c < R; c += 256) {
        double y[K2];
        const double sc = s[c];
#pragma unroll
        for (int i = 0; i < K2; ++i) y[i] = U[(g * K2 + i) * ldu + c] * sc;
#pragma unroll
        for (int i = K2 - 1; i >= 0; --i) {
            double v = y[i];
#pragma unroll
            for (int j = i + 1; j < K2; ++j) v -= Ls[j * K2 + i] * y[j];
            y[i] = v / Ls[i * K2 + i];
        }
#pragma unroll
        for (int k = 0; k < KZ; ++k) Ys[k * GSP_RMAX + c] = y[k];
    }
    if (tid >= 192 && tid < 192 + KZ) {
        const int k = tid - 192;
        double x[K2];
#pragma unroll
        for (int i = 0; i < K2; ++i) {
            double v = i == k ? 1.0 : 0.0;
#pragma unroll
            for (int j = 0; j < i; ++j) v -= Ls[i * K2 + j] * x[j];
            x[i] = v / Ls[i * K2 + i];
        }
#pragma unroll
        for (int i = K2 - 1; i >= 0; --i) {
            double v = x[i];
#pragma unroll
            for (int j = i + 1; j < K2; ++j) v -= Ls[j * K2 + i] * x[j];
            x[i] = v / Ls[i * K2 + i];
        }
#pragma unroll
        for (int l = 0; l < KZ; ++l) Ai[l * KZ + k] = x[l];
    }
    __syncthreads();
    for (int c = tid; c < R; c += 256) {
        double acc[KZ];
#pragma unroll
        for (int k = 0; k < KZ; ++k) acc[k] = 0.0;
        for (int cp = 0; cp < R; ++cp) {
            const double w = W[(i64)cp * R + c];
#pragma unroll
            for (int k = 0; k < KZ; ++k) acc[k] += Ys[k * GSP_RMAX + cp] * w;
        }
#pragma unroll
        for (int k = 0; k < KZ; ++k) {
            Es[k * GSP_RMAX + c] = acc[k];
            if (c < P) og[KK + k * P + c] = -acc[k];
        }
    }
    __syncthreads();
    if (tid < KK) {
        const int k = tid / KZ, l = tid - k * KZ;
        double acc = 0.0;
        for (int c = 0; c < R; ++c) acc += Es[k * GSP_RMAX + c] * Ys[l * GSP_RMAX + c];
        og[tid] = Ai[tid] + acc;
    }
}

// The same for a factor of lrvb_glmm_arrow_schur: R = 2 P + NC coupled rows, the LDS rows sized for
// R <= 2 x 64 + 16, and the means of mu in the FIRST K closed columns (rows 2 P + k of W) for the pseudo-group.  A kernel of its
// own, so that the one above keeps its text and its machine code.
constexpr int GSA_RMAX = 2 * 64 + GSA_NCMAX;

template <int KZ>
__global__ __launch_bounds__(256)
void glmm_arrow_group_cov_kernel(i64 G, int P, int NC, const double* __restrict__ loc /* G x K (2 K + 1) */, const double* __restrict__ U,
                                 int ldu, const double* __restrict__ W /* R x R */, const double* __restrict__ s /* R */,
                                 double* __restrict__ out /* (G + 1) x (K K + K P) */)
{
    constexpr int K2 = 2 * KZ, NT = KZ * (K2 + 1), KK = KZ * KZ;
    __shared__ double Ls[K2 * K2], Ys[KZ * GSA_RMAX], Es[KZ * GSA_RMAX], Ai[KK];
    const i64 g = blockIdx.x;
    if (g > G) return;
    const int R = 2 * P + NC, ncg = KK + KZ * P;
    const int tid = threadIdx.x;
    double* og = out + g * ncg;
    if (g == G) {
        for (int t = tid; t < ncg; t += 256) {
            if (t < KK) { const int k = t / KZ, l = t - k * KZ; og[t] = W[(i64)(2 * P + k) * R + 2 * P + l]; }
            else { const int u = t - KK, k = u / P, j = u - k * P; og[t] = W[(i64)(2 * P + k) * R + j]; }
        }
        return;
    }
    if (tid == 0) gs_local_chol<K2>(loc + g * NT, Ls);
    __syncthreads();
    for (int c = tid; c < R; c += 256) {
        double y[K2];
        const double sc = s[c];
#pragma unroll
        for (int i = 0; i < K2; ++i) y[i] = U[(g * K2 + i) * ldu + c] * sc;
#pragma unroll
        for (int i = K2 - 1; i >= 0; --i) {
            double v = y[i];
#pragma unroll
            for (int j = i + 1; j < K2; ++j) v -= Ls[j * K2 + i] * y[j];
            y[i] = v / Ls[i * K2 + i];
        }
#pragma unroll
        for (int k = 0; k < KZ; ++k) Ys[k * GSA_RMAX + c] = y[k];
    }
    if (tid >= 192 && tid < 192 + KZ) {
        const int k = tid - 192;
        double x[K2];
#pragma unroll
        for (int i = 0; i < K2; ++i) {
            double v = i == k ? 1.0 : 0.0;
#pragma unroll
            for (int j = 0; j < i; ++j) v -= Ls[i * K2 + j] * x[j];
            x[i] = v / Ls[i * K2 + i];
        }
#pragma unroll
        for (int i = K2 - 1; i >= 0; --i) {
            double v = x[i];
#pragma unroll
            for (int j = i + 1; j < K2; ++j) v -= Ls[j * K2 + i] * x[j];
            x[i] = v / Ls[i * K2 + i];
        }
#pragma unroll
        for (int l = 0; l < KZ; ++l) Ai[l * KZ + k] = x[l];
    }
    __syncthreads();
    for (int c = tid; c < R; c += 256) {
        double acc[KZ];
#pragma unroll
        for (int k = 0; k < KZ; ++k) acc[k] = 0.0;
        for (int cp = 0; cp < R; ++cp) {
            const double w = W[(i64)cp * R + c];
#pragma unroll
            for (int k = 0; k < KZ; ++k) acc[k] += Ys[k * GSA_RMAX + cp] * w;
        }
#pragma unroll
        for (int k = 0; k < KZ; ++k) {
            Es[k * GSA_RMAX + c] = acc[k];
            if (c < P) og[KK + k * P + c] = -acc[k];
        }
    }
    __syncthreads();
    if (tid < KK) {
        const int k = tid / KZ, l = tid - k * KZ;
        double acc = 0.0;
        for (int c = 0; c < R; ++c) acc += Es[k * GSA_RMAX + c] * Ys[l * GSA_RMAX + c];
        og[tid] = Ai[tid] + acc;
    }
}

// NC = 0: the legacy layout of lrvb_glmm_slopes_group_cov (3 K closed columns, the mean of mu_k at 2 P + 3 k).
int launch_glmm_slopes_group_cov(lrvb_ctx* c, int Kz, int NC, const double* loc, const double* U, int ldu, const double* W, const double* s,
                                 double* out) {
    const i64 G = c->n_groups;
    const dim3 grid((unsigned)(G + 1)), block(256);
    const int P = (int)c->P;
    if (P > 64) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "mixed model with slopes: P <= 64");
    if (NC != 0 && (NC < Kz || NC > GSA_NCMAX)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "mixed model with a dense closed border: K <= NC <= 16");
    return gs_with_K(Kz, "mixed model with slopes: 1 <= K <= 4", [&](auto k) {
        constexpr int KK = decltype(k)::value;
        if (NC == 0) hipLaunchKernelGGL(glmm_slopes_group_cov_kernel<KK>, grid, block, 0, c->stream, G, P, loc, U, ldu, W, s, out);
        else hipLaunchKernelGGL(glmm_arrow_group_cov_kernel<KK>, grid, block, 0, c->stream, G, P, NC, loc, U, ldu, W, s, out);
    });
}

// gsp_predict_rows: the streaming sibling of gsi_infl_rows -- the same tile of 64 rows in their original order, the same staging
// of x | z at stride GSI_XS, the same Lik::init / stage_row / row_shift -- for five columns of n doubles,
//   rho = o + x . m + z . e_g,   var_mf = (x o x) . v + (z o z) . r_g,
//   var_lrvb = x^T S_bb x + 2 sum_k z_k (x . S_ubeta[g][k]) + z^T S_uu[g] z,
//   mean_mf, mean_lrvb = the policy's `mean` (E sigma(t), exp(rho + ./2), m E sigma(t): its e1; m Phi(rho / sqrt(1 + .)) and
//   m E [1 - exp(-e^t)] for the two links) at (rho, var_mf) and at (rho, var_lrvb).
//   1. four lanes per row form rho and var_mf with the column map of gsi_psi_derivs and keep them in registers;
//   2. wave w owns the rows 16 w .. 16 w + 15: per block of 16 columns of S_bb (P x P, the B operand, zero past P) the product
//      X S_bb runs as 16 x 16 x 4 fp64 MFMA tiles, two accumulator chains; in the D layout (register r <-> row (l >> 4) + 4 r,
//      column l & 15) every entry is multiplied by the staged x of its row and column and added to the lane's partial sum of
//      that row;
//   3. behind it the lane adds its share of the cross term: the K P values of S_ubeta of the row's OWN group are gathered, 16
//      consecutive doubles per step for the 16 lanes of a row, against the staged x, times z_k.  The rows of a tile belong to
//      different groups, so this cannot be an MFMA operand;
//   4. xor shuffles over the 16 lanes of a row add the partial sums in a fixed order; z^T S_uu z (K K gathered values) is added
//      and the row's variance goes to LDS;
//   5. the four lanes of a row run Lik::mean twice, and lane 0 writes the five values.
// With P <= 16 the B fragments are loaded once per workgroup.  A row's result depends on nothing but the row: a window equals
// the same rows of the full result bitwise.  No atomics.
template <class Lik>
__device__ __forceinline__
void gsp_predict_rows(i64 n0, i64 R /* rows of the window */, int P, int Kz, const double* __restrict__ X,
                      const double* __restrict__ Z, const int* __restrict__ gid, const double* __restrict__ m,
                      const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                      typename Lik::Args la, const double* __restrict__ Sbb /* P x P */,
                      const double* __restrict__ gcov /* G' x (K K + K P) */, double* __restrict__ out /* 5 x ldo */, i64 ldo)
{
    __shared__ double xs[GLMM_T * GSI_XS], vq[GLMM_T], ms[64], vs[64];
    __shared__ typename Lik::Lds lik;
    __shared__ int s_gid[GLMM_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    Lik::init(lik, la, tid);
    if (tid < 64) { ms[tid] = tid < P ? m[tid] : 0.0; vs[tid] = tid < P ? vb[tid] : 0.0; }
    for (int e = tid; e < GLMM_T * GSI_XS; e += 256) xs[e] = 0.0;          // what no tile writes stays zero (finite) for the whole kernel
    const int KS = (P + 3) >> 2;                                         // k-steps of the contraction
    const int ncb = (P + 15) >> 4;
    const int KK = Kz * Kz, ncg = KK + Kz * P;
    double bm[16];
    auto load_b = [&](int cb) {
        const int q = 16 * cb + l15;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int k = 4 * kk + l4;
            bm[kk] = (q < P && k < P) ? Sbb[k * P + q] : 0.0;
        }
    };
    if (ncb == 1) load_b(0);
    const i64 n_tiles = (R + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(R - t0 < GLMM_T ? R - t0 : GLMM_T);
        __syncthreads();                                                 // the previous tile is consumed (and the nodes, m, v are in place)
        if (tid < GLMM_T) {
            s_gid[tid] = tid < rows ? gid[n0 + t0 + tid] : 0;
            Lik::stage_row(lik, la, tid, tid < rows, n0 + t0 + tid);
        }
        {
            const double* src = X + (n0 + t0) * (i64)P;
            for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * GSI_XS + cc] = src[e]; }
            const double* zsrc = Z + (n0 + t0) * (i64)Kz;
            for (int e = tid; e < rows * Kz; e += 256) { const int rr = e / Kz, cc = e - rr * Kz; xs[rr * GSI_XS + P + cc] = zsrc[e]; }
        }
        __syncthreads();
        // rho and the mean-field variance: the dot products of gsi_psi_derivs
        const bool live = row < rows;
        const double o = Lik::row_shift(lik, row);
        double rho = 0.0, s = 0.0;
        if (live) {
            const double* xr = xs + row * GSI_XS;
            for (int h = (q4 & 1) + 16 * (q4 >> 1); h < P; h += 32)
                for (int j = h; j < h + 16 && j < P; j += 2) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
            if (q4 < Kz) {
                const i64 gk = (i64)s_gid[row] * Kz + q4;
                const double z = xr[P + q4];
                rho += z * eg[gk]; s += z * z * rg[gk];
            }
        }
        rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
        rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
        // the quadratic form of this wave's 16 rows
        const double* xa = xs + (16 * wave + l15) * GSI_XS + l4;
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int cb = 0; cb < ncb; ++cb) {
            if (ncb > 1) load_b(cb);
            gsi_d4 a0 = {0.0, 0.0, 0.0, 0.0}, a1 = a0;
#pragma unroll
            for (int kk = 0; kk < 16; kk += 2) {
                if (kk < KS) a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[4 * kk], bm[kk], a0, 0, 0, 0);
                if (kk + 1 < KS) a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[4 * kk + 4], bm[kk + 1], a1, 0, 0, 0);
            }
            const int q = 16 * cb + l15;
            if (q < P) {
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] += (a0[r] + a1[r]) * xs[(16 * wave + l4 + 4 * r) * GSI_XS + q];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = 16 * wave + l4 + 4 * r;
            const double* xr = xs + rr * GSI_XS;
            const double* gc = gcov + (i64)s_gid[rr] * ncg;
            if (rr < rows) {
                double cr = 0.0;
                for (int k = 0; k < Kz; ++k) {
                    const double* sub = gc + KK + k * P;
                    double a = 0.0;
                    for (int j = l15; j < P; j += 16) a += xr[j] * sub[j];
                    cr += xr[P + k] * a;
                }
                t[r] += 2.0 * cr;
            }
            double tv = t[r];
            tv += __shfl_xor(tv, 1); tv += __shfl_xor(tv, 2); tv += __shfl_xor(tv, 4); tv += __shfl_xor(tv, 8);
            if (l15 == 0) {
                double uu = 0.0;
                if (rr < rows)
                    for (int k = 0; k < Kz; ++k)
                        for (int l = 0; l < Kz; ++l) uu += xr[P + k] * xr[P + l] * gc[k * Kz + l];
                vq[rr] = rr < rows ? tv + uu : 0.0;
            }
        }
        __syncthreads();
        const double v_lr = vq[row];
        double m_mf, m_lr;
        Lik::mean(lik, la, o, live, q4, rho, s, m_mf);
        Lik::mean(lik, la, o, live, q4, rho, v_lr, m_lr);
        if (live && q4 == 0) {
            double* dst = out + t0 + row;
            dst[0] = rho + o; dst[ldo] = s; dst[2 * ldo] = v_lr; dst[3 * ldo] = m_mf; dst[4 * ldo] = m_lr;
        }
    }
}

// The three entries of the walk above, with flat arguments in the order of their influence siblings.
__global__ __launch_bounds__(256)
void glmm_slopes_predict_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                     const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                     const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ gx,
                                     const double* __restrict__ gw, int nq, const double* __restrict__ Sbb,
                                     const double* __restrict__ gcov, double* __restrict__ out, i64 ldo)
{
    gsp_predict_rows<LogisticLik>(n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, {gx, gw, nq}, Sbb, gcov, out, ldo);
}

__global__ __launch_bounds__(256)
void glmm_poisson_predict_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                      const double* __restrict__ off, const int* __restrict__ gid, const double* __restrict__ m,
                                      const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                                      const double* __restrict__ Sbb, const double* __restrict__ gcov, double* __restrict__ out, i64 ldo)
{
    gsp_predict_rows<PoissonLik>(n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, off, Sbb, gcov, out, ldo);
}

__global__ __launch_bounds__(256)
void glmm_binomial_predict_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                       const double* __restrict__ off, const double* __restrict__ trials, const int* __restrict__ gid,
                                       const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                                       const double* __restrict__ rg, const double* __restrict__ gx, const double* __restrict__ gw,
                                       int nq, const double* __restrict__ Sbb, const double* __restrict__ gcov,
                                       double* __restrict__ out, i64 ldo)
{
    gsp_predict_rows<BinomialLik>(n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, {{gx, gw, nq}, off, trials}, Sbb, gcov, out, ldo);
}

// The probit and the cloglog link: the arguments of the binomial entry.  No y: the response mean needs none, and new rows have none.
template <int LINK>
__global__ __launch_bounds__(256)
void glmm_link_predict_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                   const double* __restrict__ off, const double* __restrict__ trials, const int* __restrict__ gid,
                                   const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                                   const double* __restrict__ rg, const double* __restrict__ gx, const double* __restrict__ gw,
                                   int nq, const double* __restrict__ Sbb, const double* __restrict__ gcov,
                                   double* __restrict__ out, i64 ldo)
{
    gsp_predict_rows<BinomialLinkLik<LINK>>(n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, {{gx, gw, nq}, off, trials, nullptr}, Sbb, gcov, out, ldo);
}

// The zero-truncated Poisson model: the arguments of the binomial entry without the trials; the mean is E A' = exp(rho + . / 2) + E r.
__global__ __launch_bounds__(256)
void glmm_ztpoisson_predict_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                        const double* __restrict__ off, const int* __restrict__ gid, const double* __restrict__ m,
                                        const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                                        const double* __restrict__ gx, const double* __restrict__ gw, int nq,
                                        const double* __restrict__ Sbb, const double* __restrict__ gcov, double* __restrict__ out, i64 ldo)
{
    gsp_predict_rows<TruncPoissonLik>(n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, {{gx, gw, nq}, off}, Sbb, gcov, out, ldo);
}

// The zero-truncated NB2 model: the arguments of the binomial entry, the dispersion in the place of the trials.  No y, as for the links.
__global__ __launch_bounds__(256)
void glmm_ztnegbin_predict_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                       const double* __restrict__ off, const double* __restrict__ disp, const int* __restrict__ gid,
                                       const double* __restrict__ m, const double* __restrict__ vb, const double* __restrict__ eg,
                                       const double* __restrict__ rg, const double* __restrict__ gx, const double* __restrict__ gw,
                                       int nq, const double* __restrict__ Sbb, const double* __restrict__ gcov,
                                       double* __restrict__ out, i64 ldo)
{
    gsp_predict_rows<TruncNegBinLik>(n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, {{gx, gw, nq}, off, disp, nullptr}, Sbb, gcov, out, ldo);
}

// The censored Gaussian model: the arguments of the zero-truncated Poisson entry.  No y, no status and no
// precision: the latent mean rho + o needs none of them, and new rows have none (the policy's staged fold o - y is then o).
__global__ __launch_bounds__(256)
void glmm_censnormal_predict_rows_kernel(i64 n0, i64 R, int P, int Kz, const double* __restrict__ X, const double* __restrict__ Z,
                                         const double* __restrict__ off, const int* __restrict__ gid, const double* __restrict__ m,
                                         const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                                         const double* __restrict__ gx, const double* __restrict__ gw, int nq,
                                         const double* __restrict__ Sbb, const double* __restrict__ gcov, double* __restrict__ out, i64 ldo)
{
    gsp_predict_rows<CensNormalLik>(n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, {{gx, gw, nq}, off, nullptr, nullptr, nullptr}, Sbb, gcov, out, ldo);
}

int launch_glmm_slopes_predict_rows(lrvb_ctx* c, const GlmmLik& lik, int Kz, const double* X, const double* Z, i64 n0, i64 n1,
                                    const int* gid, const double* m, const double* vb, const double* eg, const double* rg,
                                    const double* Sbb, const double* gcov, double* out, i64 ldo) {
    if (c->P > 64 || Kz < 1 || Kz > 4 || !X || !Z) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "mixed-model prediction: P <= 64, 1 <= K <= 4, a group design");
    const bool closed_form = lik.kind == GLMM_POISSON || lik.kind == GLMM_GAMMA;     // no nodes; E e^t = exp(rho + s / 2) for both
    if (!closed_form && (lik.n_nodes < 1 || lik.n_nodes > 128)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "1 to 128 quadrature nodes");
    const i64 R = n1 - n0;
    if (R <= 0) return LRVB_OK;
    const dim3 grid(glmm_grid(R)), block(256);
    const int P = (int)c->P;
    if (closed_form)
        hipLaunchKernelGGL(glmm_poisson_predict_rows_kernel, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, lik.off, gid, m, vb, eg, rg, Sbb,
                           gcov, out, ldo);
    else if (lik.kind == GLMM_ZTPOISSON)
        hipLaunchKernelGGL(glmm_ztpoisson_predict_rows_kernel, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, lik.off, gid, m, vb, eg, rg,
                           lik.gx, lik.gw, lik.n_nodes, Sbb, gcov, out, ldo);
    else if (lik.kind == GLMM_CENSNORMAL)
        hipLaunchKernelGGL(glmm_censnormal_predict_rows_kernel, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, lik.off, gid, m, vb, eg, rg,
                           lik.gx, lik.gw, lik.n_nodes, Sbb, gcov, out, ldo);
    else if (lik.kind == GLMM_ZTNEGBIN) {
        if (!lik.trials) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "%s", TruncNegBinLik::LIMITS);
        hipLaunchKernelGGL(glmm_ztnegbin_predict_rows_kernel, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, lik.off, lik.trials, gid, m, vb,
                           eg, rg, lik.gx, lik.gw, lik.n_nodes, Sbb, gcov, out, ldo);
    } else if (lik.kind == GLMM_BINOMIAL && lik.link == GLMM_LINK_PROBIT)
        hipLaunchKernelGGL(glmm_link_predict_rows_kernel<GLMM_LINK_PROBIT>, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, lik.off, lik.trials, gid,
                           m, vb, eg, rg, lik.gx, lik.gw, lik.n_nodes, Sbb, gcov, out, ldo);
    else if (lik.kind == GLMM_BINOMIAL && lik.link == GLMM_LINK_CLOGLOG)
        hipLaunchKernelGGL(glmm_link_predict_rows_kernel<GLMM_LINK_CLOGLOG>, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, lik.off, lik.trials, gid,
                           m, vb, eg, rg, lik.gx, lik.gw, lik.n_nodes, Sbb, gcov, out, ldo);
    else if (lik.kind == GLMM_BINOMIAL)
        hipLaunchKernelGGL(glmm_binomial_predict_rows_kernel, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, lik.off, lik.trials, gid, m, vb,
                           eg, rg, lik.gx, lik.gw, lik.n_nodes, Sbb, gcov, out, ldo);
    else
        hipLaunchKernelGGL(glmm_slopes_predict_rows_kernel, grid, block, 0, c->stream, n0, R, P, Kz, X, Z, gid, m, vb, eg, rg, lik.gx, lik.gw,
                           lik.n_nodes, Sbb, gcov, out, ldo);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// ---- group influence (lrvb_glmm_slopes_group_influence / lrvb_glmm_poisson_group_influence) --------------------------------------
// Per group the WEIGHTED sums  [sum a1 z (K) | sum a2 z o z (K) | sum a1 x (P) | sum a2 x o x (P)],  a1 = w (psi_rho - y),
// a2 = w psi_s  (2 K + 2 P columns): glmm_slopes_rows_kernel cut down to them -- group-sorted rows, two coefficients from
// Lik::infl, the same in-order walk of the tile (thread t owns column t), the pieces of a cut group in the tile's two partial
// rows, added by glmm_fixup_kernel in tile order.  The staging is that of the rows kernel, stride and column map of the dot
// products those of the row kernel above.  The contraction with the operand is N-independent: a (G x 2 P) (2 P x Q) product on the
// library's GEMM and glmm_slopes_infl_local_kernel for the 2 K local columns.  Fixed order everywhere, no atomics.
template <class Lik>
__global__ __launch_bounds__(256)
void glmm_slopes_infl_gsum_kernel(i64 N, int P, int Kz, i64 G, const double* __restrict__ X, const double* __restrict__ Z,
                                  const double* __restrict__ y, const double* __restrict__ w, const i64* __restrict__ perm,
                                  const i64* __restrict__ offs, const double* __restrict__ m, const double* __restrict__ vb,
                                  const double* __restrict__ eg, const double* __restrict__ rg, typename Lik::Args la,
                                  double* __restrict__ gsum, double* __restrict__ part)
{
    __shared__ double xs[GLMM_T * GSI_XS], cf[2 * GLMM_T], ms[64], vs[64];
    __shared__ typename Lik::Lds lik;
    __shared__ i64 s_row[GLMM_T];
    __shared__ int s_gid[GLMM_T], s_whole[GLMM_T];
    const int tid = threadIdx.x;
    const int K2 = 2 * Kz, ncol = K2 + 2 * P;
    Lik::init(lik, la, tid);
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    // output column tid (< ncol): a1 z_k | a2 z_k^2 | a1 x_j | a2 x_j^2 -- the staged column jc, squared or not
    const bool has_col = tid < ncol;
    const bool sq = has_col && (tid < K2 ? tid >= Kz : tid >= K2 + P);
    const int jc = !has_col ? 0 : (tid < Kz ? P + tid : (tid < K2 ? P + tid - Kz : (tid < K2 + P ? tid - K2 : tid - K2 - P)));
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(N - t0 < GLMM_T ? N - t0 : GLMM_T);
        __syncthreads();
        gs_stage_sorted_tile<Lik, GSI_XS>(tid, t0, rows, P, Kz, G, X, Z, perm, offs, la, lik, xs, s_row, s_gid, s_whole);
        double e1, e2;
        gsi_psi_derivs<Lik>(xs + row * GSI_XS, row, row < rows, s_gid[row], q4, P, Kz, ms, vs, eg, rg, lik, la, e1, e2);
        if (q4 == 0) {
            double k1 = 0.0, k2 = 0.0;
            if (row < rows) {
                const i64 pr = s_row[row];
                const double wi = w[pr];
                if constexpr (Lik::MINUS_Y) k1 = wi * (e1 - y[pr]);
                else k1 = wi * e1;
                k2 = wi * 0.5 * e2;
            }
            cf[row] = k1; cf[GLMM_T + row] = k2;
        }
        __syncthreads();
        if (has_col) {
            double acc = 0.0;
            int run_start = 0;
            for (int rr = 0; rr < rows; ++rr) {
                double x = xs[rr * GSI_XS + jc];
                if (sq) x *= x;
                acc += cf[(sq ? GLMM_T : 0) + rr] * x;
                const int g = s_gid[rr];
                if (rr == rows - 1 || s_gid[rr + 1] != g) {
                    gs_flush_dst(s_whole[rr], g, tile, run_start, ncol, gsum, part)[tid] = acc;
                    acc = 0.0; run_start = rr + 1;
                }
            }
        }
    }
}

// out[g][q] += sum_c S[g][c] A_local[g][c][q], c = 0 .. 2 K - 1   (S: the group sums, leading dimension ncol)
__global__ __launch_bounds__(256)
void glmm_slopes_infl_local_kernel(i64 G, int Q, int K2, int ncol, const double* __restrict__ S, const double* __restrict__ Al,
                                   double* __restrict__ out)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= G * Q) return;
    const i64 g = i / Q;
    const int q = (int)(i - g * Q);
    const double* s = S + g * ncol;
    const double* al = Al + g * K2 * Q + q;
    double acc = 0.0;
    for (int c = 0; c < K2; ++c) acc += s[c] * al[(i64)c * Q];
    out[i] += acc;
}


template <class Lik>
static int gs_launch_infl_gsum(lrvb_ctx* c, int Kz, const double* Z, typename Lik::Args la, const double* m, const double* vb,
                               const double* eg, const double* rg, double* gsum, double* part) {
    const i64 N = c->N, G = c->n_groups;
    if (c->P > 64 || Kz < 1 || Kz > 4 || !Lik::args_ok(la)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "%s", Lik::LIMITS);
    const int ncol = 2 * Kz + 2 * (int)c->P;
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    hipLaunchKernelGGL(glmm_slopes_infl_gsum_kernel<Lik>, dim3(glmm_grid(N)), dim3(256), 0, c->stream, N, (int)c->P, Kz, G, (const double*)c->X.p, Z,
                       (const double*)c->y.p, (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, la, gsum, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncol, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

int launch_glmm_slopes_infl_gsum(lrvb_ctx* c, const GlmmLik& lik, int Kz, const double* Z, const double* m, const double* vb,
                                 const double* eg, const double* rg, double* gsum, double* part) {
    if (!Z) { LRVB_TRY(gs_unit_design(lik, Kz)); return launch_glmm_infl_gsum(c, m, vb, eg, rg, lik.gx, lik.gw, lik.n_nodes, gsum, part); }
    return gs_with_lik(lik, [&](auto L, auto la) { return gs_launch_infl_gsum<decltype(L)>(c, Kz, Z, la, m, vb, eg, rg, gsum, part); });
}

int launch_glmm_slopes_infl_local(lrvb_ctx* c, int Kz, i64 Q, const double* S, const double* Al, double* out) {
    const i64 G = c->n_groups, n = G * Q;
    hipLaunchKernelGGL(glmm_slopes_infl_local_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, G, (int)Q, 2 * Kz,
                       2 * Kz + 2 * (int)c->P, S, Al, out);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}


// The three global blocks of the Poisson model were all formed with the one coefficient vector h: [X^T h X | X^T h X2 | X2^T h X2].
// c12 = h / 2 and c22 = h / 4: the second and third block take their factor here (exact).
__global__ void glmm_poisson_scale_blocks_kernel(i64 PP, double* __restrict__ Hb)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= PP) return;
    Hb[PP + i] *= 0.5;
    Hb[2 * PP + i] *= 0.25;
}

// The Gamma model's blocks likewise, with c12 = -g / 2: the cross block takes the sign with its factor (exact).
__global__ void glmm_gamma_scale_blocks_kernel(i64 PP, double* __restrict__ Hb)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= PP) return;
    Hb[PP + i] *= -0.5;
    Hb[2 * PP + i] *= 0.25;
}

int launch_glmm_gamma_scale_blocks(lrvb_ctx* c, double* Hb) {
    const i64 PP = c->P * c->P;
    hipLaunchKernelGGL(glmm_gamma_scale_blocks_kernel, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, c->stream, PP, Hb);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

int launch_glmm_poisson_scale_blocks(lrvb_ctx* c, double* Hb) {
    const i64 PP = c->P * c->P;
    hipLaunchKernelGGL(glmm_poisson_scale_blocks_kernel, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, c->stream, PP, Hb);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

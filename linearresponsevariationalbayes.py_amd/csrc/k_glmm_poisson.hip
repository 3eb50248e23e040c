// k_glmm_poisson.hip -- Poisson mixed model with K <= 4 independent random effects per group:
//   y_n ~ Poisson(exp(o_n + x_n . beta + z_n . u_g(n))),   q(beta_j) = N(m_j, v_j),   q(u_gk) = N(e_gk, r_gk).
// Per observation rho_n = o_n + x_n . m + z_n . e_g, s_n = (x_n o x_n) . v + (z_n o z_n) . r_g and
//   psi_n = E exp(t) = exp(rho_n + s_n / 2),  t ~ N(rho_n, s_n)      -- exact, no quadrature: ONE exp per row.
// With h = w psi the five coefficients of k_glmm_slopes.hip are a1 = h - w y, a2 = h / 2, c11 = h, c12 = h / 2, c22 = h / 4: two
// distinct numbers per row and the constant factors 1, 1/2, 1/2, 1/4.  Multiplying by a power of two is exact, so every factor
// is applied ONCE to a finished sum (at the flush of a segment here, to a whole block in lrvb_glmm_poisson_terms) and the result
// is bit for bit the sum of the scaled terms.
//
// The kernels are the siblings of glmm_slopes_rows_kernel, glmm_slopes_infl_rows_kernel and glmm_slopes_infl_gsum_kernel: the
// same tiles of GP_T = 64 rows, the same staging, the same in-order segmented walk, the same two partial rows per tile added by
// glmm_fixup_kernel (k_glmm.hip), the same output layouts (include/lrvb_hip.h, lrvb_glmm_slopes_terms).  The tile walk is
// DUPLICATED from k_glmm_slopes.hip on purpose: that file's object code stays what it was (known cost).
// What the simpler likelihood changes in glmm_poisson_rows_kernel:
//   * no node tables in LDS, no quadrature loop: lane 0 of a row's four lanes takes one exp;
//   * two coefficient rows in LDS (a1, h) instead of five, and two coefficient vectors for the library's weighted products
//     (coef[0] = a1, coef[NP] = h): the gradient in v is 1/2 X2^T h and the three global blocks are X^T h X, 1/2 X^T h X2,
//     1/4 X2^T h X2 (launch_glmm_poisson_scale_blocks);
//   * the shared products of a row are the 2 K numbers d[k] = h z_k, d[K + k] = h z_k^2, stored densely (row stride 2 K); border
//     block b = 0..3 of component k reads d[(b & 1) K + k] and carries the factor {1, 1/2, 1/2, 1/4}[b].
// No atomics anywhere: every result is a fixed-order sum, bitwise reproducible.  Empty groups keep the zeros the caller wrote.
// The kernels do not clamp: where rho + s / 2 overflows the exponent, psi = inf reaches the sums and the entry refuses the
// non-finite value (LRVB_ERR_INVALID).
//
// LDS strides.  Bank of a double at index a: a mod 32 (ds_read_b64: 64 dword banks, the two 32-lane halves separately).
//   GP_XS = 68 (rows kernel; 64 columns of x + 4 of z).  (a) dot products: a half holds 8 rows x 4 lanes, lane q4 on the columns
//     q4, q4 + 4, ..: banks 68 row + q4 + 4 i = 4 row + q4 (+ 4 i) mod 32, row = 0..7, q4 = 0..3 -- 32 different values.
//     (b) the walk: thread t reads word o_x of row rr, o_x = (t + 256 i) mod P -- the lanes of a half read consecutive words of one
//     row (wrapping to its start at a multiple of P: a second run of consecutive words, overlapping the first only where two
//     lanes read the SAME word, which is a broadcast), the factor d[.] is one word or two for the half: broadcasts.
//     (c) the products table is written and read at dense indices (thread e writes word e): conflict-free.
//   GPI_XS = 70 (the two influence kernels): the argument of GSI_XS in k_glmm_slopes.hip, unchanged -- MFMA operand reads
//     (lane (i, k) on row i, column 4 kk + k: 70 i = 6 i mod 32 runs through 16 different even residues) and the dot products on
//     the columns c0 + 2 t + 32 h, c0 = {0, 1, 16, 17}[q4].
#include "lrvb_internal.h"
#include "k_kernels.h"
#include <math.h>

constexpr int GP_T = 64;                 // sorted rows per tile (= GL_T of k_glmm.hip: glmm_fixup_kernel and glmm_num_tiles are shared)
constexpr int GP_XS = 68;
constexpr int GP_OWN = 4;                // border columns per thread: 4 K P <= 1024 = 4 x 256
constexpr int GPI_XS = 70;

__global__ __launch_bounds__(256)
void glmm_poisson_rows_kernel(i64 N, int P, int Kz, i64 G, const double* __restrict__ X, const double* __restrict__ Z,
                              const double* __restrict__ off, const double* __restrict__ y, const double* __restrict__ w,
                              const i64* __restrict__ perm, const i64* __restrict__ offs, const double* __restrict__ m,
                              const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                              double* __restrict__ coef, i64 NP, double* __restrict__ gsum, double* __restrict__ part,
                              double* __restrict__ vpart)
{
    __shared__ double xs[GP_T * GP_XS], dk[GP_T * 8], cf[2 * GP_T], s_off[GP_T], ms[64], vs[64], red[4];
    __shared__ i64 s_row[GP_T];
    __shared__ int s_gid[GP_T], s_whole[GP_T];
    const int tid = threadIdx.x;
    const int K2 = 2 * Kz, K4 = 4 * Kz;
    const int nsc = K2 + Kz * (K2 + 1), nbord = K4 * P, ncol = nsc + nbord;
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GP_T - 1) / GP_T;
    const int row = tid >> 2, q4 = tid & 3;
    // the border columns of this thread: column t = tid + 256 i is block bk = t / P (b = bk / K, k = bk - b K) and x column
    // j = t - bk P; it reads d[(b & 1) K + k], squares x for b >= 2 and carries the factor o_f
    int o_x[GP_OWN], o_d[GP_OWN];
    bool o_has[GP_OWN], o_sq[GP_OWN];
    double o_f[GP_OWN];
#pragma unroll
    for (int i = 0; i < GP_OWN; ++i) {
        const int t = tid + 256 * i;
        o_has[i] = t < nbord;
        const int bk = o_has[i] ? t / P : 0, b = bk / Kz, k = bk - b * Kz;
        o_d[i] = (b & 1) * Kz + k; o_x[i] = o_has[i] ? t - bk * P : 0; o_sq[i] = b >= 2;
        o_f[i] = b == 0 ? 1.0 : (b == 3 ? 0.25 : 0.5);
    }
    // the scalar column of this thread (tid < nsc): s_f cf[s_c] q[s_i] q[s_j] with q = [z | z o z | 1], cf = [a1 | h]
    const bool has_sc = tid < nsc;
    int s_c = 1, s_i = K2, s_j = K2;
    double s_f = 1.0;
    if (tid < Kz) { s_c = 0; s_i = tid; }                                 // sum a1 z_k
    else if (tid < K2) { s_i = tid; s_f = 0.5; }                          // sum a2 z_k^2, a2 = h / 2
    else if (has_sc) {
        int u = tid - K2, i = 0;
        while (u >= K2 - i) { u -= K2 - i; ++i; }
        s_i = i; s_j = i + u;
        s_f = s_j < Kz ? 1.0 : (s_i >= Kz ? 0.25 : 0.5);                  // c11 = h, c22 = h / 4, c12 = h / 2
    }
    const int zi = P + (s_i < Kz ? s_i : s_i - Kz), zj = P + (s_j < Kz ? s_j : s_j - Kz);    // unused where the factor is 1
    const bool i_one = s_i >= K2, i_sq = s_i >= Kz, j_one = s_j >= K2, j_sq = s_j >= Kz;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GP_T;
        const int rows = (int)(N - t0 < GP_T ? N - t0 : GP_T);
        __syncthreads();                                                 // the previous tile is consumed (and m, v are in place)
        if (tid < GP_T) {
            int g = 0, whole = 0;
            i64 pr = 0;
            double o = 0.0;
            if (tid < rows) {
                const i64 i = t0 + tid;
                pr = perm[i];
                if (off) o = off[pr];
                i64 lo = 0, hi = G;                                      // the last g with offs[g] <= i (its offs[g + 1] > i)
                while (hi - lo > 1) { const i64 mid = (lo + hi) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid; }
                g = (int)lo;
                whole = (offs[lo] >= t0 && offs[lo + 1] <= t0 + GP_T) ? 1 : 0;
            }
            s_row[tid] = pr; s_gid[tid] = g; s_whole[tid] = whole; s_off[tid] = o;
        }
        __syncthreads();
        for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * GP_XS + cc] = X[s_row[rr] * P + cc]; }
        for (int e = tid; e < rows * Kz; e += 256) { const int rr = e / Kz, cc = e - rr * Kz; xs[rr * GP_XS + P + cc] = Z[s_row[rr] * Kz + cc]; }
        __syncthreads();
        double rho = 0.0, s = 0.0;
        if (row < rows) {
            const double* xr = xs + row * GP_XS;
            for (int j = q4; j < P; j += 4) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
            if (q4 < Kz) {
                const i64 gk = (i64)s_gid[row] * Kz + q4;
                const double z = xr[P + q4];
                rho += z * eg[gk]; s += z * z * rg[gk];
            }
        }
        rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
        rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
        double contrib = 0.0;
        if (q4 == 0) {
            double k1 = 0.0, h = 0.0;
            if (row < rows) {
                const i64 pr = s_row[row];
                const double wi = w[pr], yi = y[pr];
                rho += s_off[row];
                const double psi = exp(rho + 0.5 * s);
                contrib = wi * (psi - yi * rho);
                h = wi * psi; k1 = h - wi * yi;
                coef[pr] = k1; coef[NP + pr] = h;
            }
            cf[row] = k1; cf[GP_T + row] = h;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o);
        if ((tid & 63) == 0) red[tid >> 6] = contrib;
        __syncthreads();
        if (tid == 0) vpart[tile] = (red[0] + red[1]) + (red[2] + red[3]);
        // the 2 K products of a row that its border columns share: dk[rr 2 K + k] = h z_k, dk[rr 2 K + K + k] = h z_k^2
        for (int e = tid; e < rows * K2; e += 256) {
            const int rr = e / K2, bk = e - rr * K2;
            const double z = xs[rr * GP_XS + P + (bk < Kz ? bk : bk - Kz)];
            dk[e] = cf[GP_T + rr] * (bk < Kz ? z : z * z);
        }
        __syncthreads();
        // segmented sums over the tile's rows, in row order
        if (o_has[0] || has_sc) {
            double acc[GP_OWN] = {0.0, 0.0, 0.0, 0.0}, accs = 0.0;
            int run_start = 0;
            for (int rr = 0; rr < rows; ++rr) {
                const double* xr = xs + rr * GP_XS;
                const double* dr = dk + rr * K2;
#pragma unroll
                for (int i = 0; i < GP_OWN; ++i)
                    if (o_has[i]) { double x = xr[o_x[i]]; if (o_sq[i]) x *= x; acc[i] += dr[o_d[i]] * x; }
                if (has_sc) {
                    double fi = 1.0, fj = 1.0;
                    if (!i_one) { fi = xr[zi]; if (i_sq) fi *= fi; }
                    if (!j_one) { fj = xr[zj]; if (j_sq) fj *= fj; }
                    accs += cf[s_c * GP_T + rr] * (fi * fj);
                }
                const int g = s_gid[rr];
                if (rr == rows - 1 || s_gid[rr + 1] != g) {
                    double* dst = s_whole[rr] ? gsum + (i64)g * ncol : part + (tile * 2 + (run_start == 0 ? 0 : 1)) * ncol;
#pragma unroll
                    for (int i = 0; i < GP_OWN; ++i)
                        if (o_has[i]) { dst[nsc + tid + 256 * i] = o_f[i] * acc[i]; acc[i] = 0.0; }
                    if (has_sc) dst[tid] = s_f * accs;
                    accs = 0.0; run_start = rr + 1;
                }
            }
        }
    }
}

int launch_glmm_poisson_rows(lrvb_ctx* c, int Kz, const double* Z, const double* off, const double* m, const double* vb, const double* eg,
                             const double* rg, double* coef, i64 NP, double* gsum, double* part, double* vpart) {
    const i64 N = c->N, G = c->n_groups;
    if (c->P > 64 || Kz < 1 || Kz > 4) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "Poisson mixed model: P <= 64, 1 <= K <= 4");
    const int ncol = glmm_slopes_ncol((int)c->P, Kz);
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    const i64 n_tiles = glmm_num_tiles(N);
    const unsigned grid = (unsigned)(n_tiles < 2048 ? (n_tiles < 1 ? 1 : n_tiles) : 2048);
    hipLaunchKernelGGL(glmm_poisson_rows_kernel, dim3(grid), dim3(256), 0, c->stream, N, (int)c->P, Kz, G, (const double*)c->X.p, Z, off,
                       (const double*)c->y.p, (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, coef, NP, gsum, part, vpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncol, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// The three global blocks were all formed with the one coefficient vector h: [X^T h X | X^T h X2 | X2^T h X2].  c12 = h / 2 and
// c22 = h / 4: the second and third block take their factor here (exact).
__global__ void glmm_poisson_scale_blocks_kernel(i64 PP, double* __restrict__ Hb)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= PP) return;
    Hb[PP + i] *= 0.5;
    Hb[2 * PP + i] *= 0.25;
}

int launch_glmm_poisson_scale_blocks(lrvb_ctx* c, double* Hb) {
    const i64 PP = c->P * c->P;
    hipLaunchKernelGGL(glmm_poisson_scale_blocks_kernel, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, c->stream, PP, Hb);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// ---- streamed weight influence (lrvb_glmm_poisson_obs_influence) -----------------------------------------------------------------
// out[n - n0][q] = a1' (x_n . A_m[q] + sum_k z_nk A_e[q, g(n), k]) + a2' ((x_n o x_n) . A_v[q] + sum_k z_nk^2 A_r[q, g(n), k]),
// a1' = psi - y_n, a2' = psi / 2 PER UNIT WEIGHT (w_n does not enter): glmm_slopes_infl_rows_kernel with the quadrature replaced
// by one exp -- rows in their original order, the tile staged once for any Q, the two P x Q contractions as 16 x 16 x 4 fp64
// MFMA tiles with two accumulator chains each, the 2 K local terms added behind them in the D layout.

typedef double gpi_d4 __attribute__((ext_vector_type(4)));

// The per-row part both influence kernels share: every one of the four lanes of the staged row xr returns psi.
__device__ __forceinline__ double gpi_psi(const double* xr, bool live, double o, int g, int q4, int P, int Kz, const double* ms,
                                          const double* vs, const double* __restrict__ eg, const double* __restrict__ rg)
{
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
    return live ? exp((rho + o) + 0.5 * s) : 0.0;
}

__global__ __launch_bounds__(256)
void glmm_poisson_infl_rows_kernel(i64 n0, i64 R /* rows of the window */, int P, int Kz, const double* __restrict__ X,
                                   const double* __restrict__ Z, const double* __restrict__ off, const double* __restrict__ y,
                                   const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                                   const double* __restrict__ eg, const double* __restrict__ rg,
                                   const double* __restrict__ Ag /* Q x 2 P */, const double* __restrict__ Al /* G x 2 K x Q */, int Q,
                                   double* __restrict__ out /* R x Q */)
{
    __shared__ double xs[GP_T * GPI_XS], a1s[GP_T], a2s[GP_T], s_off[GP_T], ms[64], vs[64];
    __shared__ int s_gid[GP_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    if (tid < 64) { ms[tid] = tid < P ? m[tid] : 0.0; vs[tid] = tid < P ? vb[tid] : 0.0; }
    for (int e = tid; e < GP_T * GPI_XS; e += 256) xs[e] = 0.0;          // what no tile writes stays zero (finite) for the whole kernel
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
    const i64 n_tiles = (R + GP_T - 1) / GP_T;
    const int row = tid >> 2, q4 = tid & 3;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GP_T;
        const int rows = (int)(R - t0 < GP_T ? R - t0 : GP_T);
        __syncthreads();                                                 // the previous tile is consumed (and m, v are in place)
        if (tid < GP_T) {
            s_gid[tid] = tid < rows ? gid[n0 + t0 + tid] : 0;
            s_off[tid] = (off && tid < rows) ? off[n0 + t0 + tid] : 0.0;
        }
        {
            const double* src = X + (n0 + t0) * (i64)P;
            for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * GPI_XS + cc] = src[e]; }
            const double* zsrc = Z + (n0 + t0) * (i64)Kz;
            for (int e = tid; e < rows * Kz; e += 256) { const int rr = e / Kz, cc = e - rr * Kz; xs[rr * GPI_XS + P + cc] = zsrc[e]; }
        }
        __syncthreads();
        const double psi = gpi_psi(xs + row * GPI_XS, row < rows, s_off[row], s_gid[row], q4, P, Kz, ms, vs, eg, rg);
        if (q4 == 0) {
            double k1 = 0.0, k2 = 0.0;
            if (row < rows) { k1 = psi - y[n0 + t0 + row]; k2 = 0.5 * psi; }
            a1s[row] = k1; a2s[row] = k2;
        }
        __syncthreads();
        // the two contractions of this wave's 16 rows
        const double* xa = xs + (16 * wave + l15) * GPI_XS + l4;
        for (int qb = 0; qb < nqb; ++qb) {
            if (nqb > 1) load_b(qb);
            gpi_d4 am0 = {0.0, 0.0, 0.0, 0.0}, am1 = am0, av0 = am0, av1 = am0;
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
                        const double* zr = xs + rr * GPI_XS + P;
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

int launch_glmm_poisson_infl_rows(lrvb_ctx* c, int Kz, const double* Z, const double* off, i64 n0, i64 n1, const int* gid, const double* m,
                                  const double* vb, const double* eg, const double* rg, const double* Ag, const double* Al, i64 Q,
                                  double* out) {
    if (c->P > 64 || Kz < 1 || Kz > 4) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "Poisson mixed model: P <= 64, 1 <= K <= 4");
    const i64 R = n1 - n0;
    if (R <= 0) return LRVB_OK;
    const i64 n_tiles = (R + GP_T - 1) / GP_T;
    const unsigned grid = (unsigned)(n_tiles < 2048 ? n_tiles : 2048);
    hipLaunchKernelGGL(glmm_poisson_infl_rows_kernel, dim3(grid), dim3(256), 0, c->stream, n0, R, (int)c->P, Kz, (const double*)c->X.p, Z,
                       off, (const double*)c->y.p, gid, m, vb, eg, rg, Ag, Al, (int)Q, out);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// ---- group influence (lrvb_glmm_poisson_group_influence) ---------------------------------------------------------------------------
// Per group the WEIGHTED sums  [sum a1 z (K) | sum a2 z o z (K) | sum a1 x (P) | sum a2 x o x (P)],  a1 = w (psi - y), a2 = w psi / 2
// (2 K + 2 P columns): glmm_slopes_infl_gsum_kernel with one exp -- group-sorted rows, the in-order walk of the tile (thread t owns
// column t), the pieces of a cut group in the tile's two partial rows, added by glmm_fixup_kernel in tile order.  The contraction
// with the operand is the library's GEMM and glmm_slopes_infl_local_kernel, as for the logistic model.
__global__ __launch_bounds__(256)
void glmm_poisson_infl_gsum_kernel(i64 N, int P, int Kz, i64 G, const double* __restrict__ X, const double* __restrict__ Z,
                                   const double* __restrict__ off, const double* __restrict__ y, const double* __restrict__ w,
                                   const i64* __restrict__ perm, const i64* __restrict__ offs, const double* __restrict__ m,
                                   const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                                   double* __restrict__ gsum, double* __restrict__ part)
{
    __shared__ double xs[GP_T * GPI_XS], cf[2 * GP_T], s_off[GP_T], ms[64], vs[64];
    __shared__ i64 s_row[GP_T];
    __shared__ int s_gid[GP_T], s_whole[GP_T];
    const int tid = threadIdx.x;
    const int K2 = 2 * Kz, ncol = K2 + 2 * P;
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GP_T - 1) / GP_T;
    const int row = tid >> 2, q4 = tid & 3;
    // output column tid (< ncol): a1 z_k | a2 z_k^2 | a1 x_j | a2 x_j^2 -- the staged column jc, squared or not
    const bool has_col = tid < ncol;
    const bool sq = has_col && (tid < K2 ? tid >= Kz : tid >= K2 + P);
    const int jc = !has_col ? 0 : (tid < Kz ? P + tid : (tid < K2 ? P + tid - Kz : (tid < K2 + P ? tid - K2 : tid - K2 - P)));
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GP_T;
        const int rows = (int)(N - t0 < GP_T ? N - t0 : GP_T);
        __syncthreads();
        if (tid < GP_T) {
            int g = 0, whole = 0;
            i64 pr = 0;
            double o = 0.0;
            if (tid < rows) {
                const i64 i = t0 + tid;
                pr = perm[i];
                if (off) o = off[pr];
                i64 lo = 0, hi = G;                                      // the last g with offs[g] <= i (its offs[g + 1] > i)
                while (hi - lo > 1) { const i64 mid = (lo + hi) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid; }
                g = (int)lo;
                whole = (offs[lo] >= t0 && offs[lo + 1] <= t0 + GP_T) ? 1 : 0;
            }
            s_row[tid] = pr; s_gid[tid] = g; s_whole[tid] = whole; s_off[tid] = o;
        }
        __syncthreads();
        for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * GPI_XS + cc] = X[s_row[rr] * P + cc]; }
        for (int e = tid; e < rows * Kz; e += 256) { const int rr = e / Kz, cc = e - rr * Kz; xs[rr * GPI_XS + P + cc] = Z[s_row[rr] * Kz + cc]; }
        __syncthreads();
        const double psi = gpi_psi(xs + row * GPI_XS, row < rows, s_off[row], s_gid[row], q4, P, Kz, ms, vs, eg, rg);
        if (q4 == 0) {
            double k1 = 0.0, k2 = 0.0;
            if (row < rows) { const i64 pr = s_row[row]; const double wi = w[pr]; k1 = wi * (psi - y[pr]); k2 = wi * 0.5 * psi; }
            cf[row] = k1; cf[GP_T + row] = k2;
        }
        __syncthreads();
        if (has_col) {
            double acc = 0.0;
            int run_start = 0;
            for (int rr = 0; rr < rows; ++rr) {
                double x = xs[rr * GPI_XS + jc];
                if (sq) x *= x;
                acc += cf[(sq ? GP_T : 0) + rr] * x;
                const int g = s_gid[rr];
                if (rr == rows - 1 || s_gid[rr + 1] != g) {
                    double* dst = s_whole[rr] ? gsum + (i64)g * ncol : part + (tile * 2 + (run_start == 0 ? 0 : 1)) * ncol;
                    dst[tid] = acc;
                    acc = 0.0; run_start = rr + 1;
                }
            }
        }
    }
}

int launch_glmm_poisson_infl_gsum(lrvb_ctx* c, int Kz, const double* Z, const double* off, const double* m, const double* vb,
                                  const double* eg, const double* rg, double* gsum, double* part) {
    const i64 N = c->N, G = c->n_groups;
    if (c->P > 64 || Kz < 1 || Kz > 4) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "Poisson mixed model: P <= 64, 1 <= K <= 4");
    const int ncol = 2 * Kz + 2 * (int)c->P;
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    const i64 n_tiles = glmm_num_tiles(N);
    const unsigned grid = (unsigned)(n_tiles < 2048 ? (n_tiles < 1 ? 1 : n_tiles) : 2048);
    hipLaunchKernelGGL(glmm_poisson_infl_gsum_kernel, dim3(grid), dim3(256), 0, c->stream, N, (int)c->P, Kz, G, (const double*)c->X.p, Z, off,
                       (const double*)c->y.p, (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, gsum, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncol, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// k_logitmvn.hip -- logistic regression with a full-covariance Gaussian posterior q(beta) = N(m, Sigma), Sigma = Lambda^-1.
// Per observation mu_n = x_n . m and s_n = x_n^T Sigma x_n; psi(mu, s) = E log(1 + e^z), z ~ N(mu, s), by Gauss-Hermite.
// The kernels here are the O(N) element-wise and row pieces; the products over observations are the existing MFMA kernels
// (the weighted TN product, the packed-triangle Kronecker SYRK wsyrk_kron_kernel) except the cross block, which has its own
// MFMA kernel here, and the chain to vech Lambda is GEMMs (lrvb_api.hip, lrvb_logitnormal_mvn_*).
#include "lrvb_internal.h"
#include "k_kernels.h"
#include <math.h>

typedef double lmvn_d4 __attribute__((ext_vector_type(4)));

// vech index v = a (a + 1) / 2 + b (b <= a) -> is it a diagonal entry?
__device__ __forceinline__ bool lmvn_vech_diag(i64 v) {
    i64 a = (i64)((sqrt(8.0 * (double)v + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > v) --a;
    while ((a + 1) * (a + 2) / 2 <= v) ++a;
    return v - a * (a + 1) / 2 == a;
}

// Derivatives of psi in the VARIANCE s (Stein's identity on z ~ N(mu, s)): d_s E g = 1/2 E g'', d_mu d_s E g = 1/2 E g''',
// d_s^2 E g = 1/4 E g'''', each expectation by the same nodes.  No division by sd: a design row of zeros (s = 0) is regular.
// g = log(1 + e^t): g' = sigma, g'' = sigma (1 - sigma), g''' = g'' (1 - 2 sigma), g'''' = g'' (1 - 6 g''), all in the
// overflow-free form of e = exp(-|t|).
// Outputs (zero padding past n is the caller's): a1 = w (psi_mu - y), a2 = w psi_s, c11 = w psi_mumu, c12 = w psi_mus,
// c22 = w psi_ss, and the block sums of w (psi - y mu).
__global__ __launch_bounds__(256)
void lmvn_coef_kernel(i64 n, const double* __restrict__ mu, const double* __restrict__ s, const double* __restrict__ y,
                      const double* __restrict__ w, const double* __restrict__ gx, const double* __restrict__ gw, int K,
                      double* __restrict__ a1, double* __restrict__ a2, double* __restrict__ c11, double* __restrict__ c12,
                      double* __restrict__ c22, double* __restrict__ vpart)
{
    __shared__ double sx[128], sw[128], red[4];
    const double r2 = 1.4142135623730951, ispi = 0.5641895835477563;     // sqrt(2), 1 / sqrt(pi)
    if ((int)threadIdx.x < K) { sx[threadIdx.x] = r2 * gx[threadIdx.x]; sw[threadIdx.x] = ispi * gw[threadIdx.x]; }
    __syncthreads();
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    double contrib = 0.0;
    if (i < n) {
        const double m = mu[i], sd = sqrt(fmax(s[i], 0.0)), wi = w[i], yi = y[i];
        double v = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0, e4 = 0.0;
        for (int k = 0; k < K; ++k) {
            const double t = m + sd * sx[k], wk = sw[k];
            const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
            const double sp = (t > 0.0 ? t : 0.0) + log1p(e);
            const double sg = t >= 0.0 ? ie : e * ie;
            const double g2 = e * ie * ie;
            const double om = (1.0 - e) * ie;                            // |1 - 2 sigma|
            const double g3 = t >= 0.0 ? -g2 * om : g2 * om;
            v += wk * sp; e1 += wk * sg; e2 += wk * g2; e3 += wk * g3; e4 += wk * g2 * (1.0 - 6.0 * g2);
        }
        contrib = wi * (v - yi * m);
        a1[i] = wi * (e1 - yi);
        a2[i] = wi * 0.5 * e2;
        c11[i] = wi * e2;
        c12[i] = wi * 0.5 * e3;
        c22[i] = wi * 0.25 * e4;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) contrib += __shfl_xor(contrib, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = contrib;
    __syncthreads();
    if (threadIdx.x == 0) vpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The Sigma-Sigma block in vech Sigma coordinates: H[P + r, P + c] *= delta_r delta_c (delta = 1 on the diagonal, 2 off it)
__global__ void lmvn_dup_scale_kernel(i64 total, i64 Pv, int P, double* __restrict__ H, i64 ld)
{
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;                                  // total = Pv^2
    const i64 r = k / Pv, c = k - r * Pv;
    const double f = (lmvn_vech_diag(r) ? 1.0 : 2.0) * (lmvn_vech_diag(c) ? 1.0 : 2.0);
    H[(P + r) * ld + P + c] *= f;
}

// g[v] = delta_v G[a, b] for the vech coordinate v = (a, b): the gradient in vech Sigma of tr(G Sigma)
__global__ void lmvn_vech_grad_kernel(i64 total, int P, const double* __restrict__ G, double* __restrict__ g)
{
    const i64 v = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= total) return;
    i64 a = (i64)((sqrt(8.0 * (double)v + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > v) --a;
    while ((a + 1) * (a + 2) / 2 <= v) ++a;
    const i64 b = v - a * (a + 1) / 2;
    g[v] = G[a * P + b] * (a == b ? 1.0 : 2.0);
}

// H[P + v, a] = H[a, P + v]: the lower-left block from the upper-right one
__global__ void lmvn_mirror_kernel(i64 total, i64 Pv, int P, double* __restrict__ H, i64 ld)
{
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;                                  // total = P Pv
    const i64 a = k / Pv, v = k - a * Pv;
    H[(P + v) * ld + a] = H[a * ld + P + v];
}

// dst[r, c] = src[r, c] for an R x C block (strided)
__global__ void lmvn_copy_block_kernel(i64 total, i64 C, const double* __restrict__ src, i64 lds, double* __restrict__ dst, i64 ldd)
{
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    const i64 r = k / C, c = k - r * C;
    dst[r * ldd + c] = src[r * lds + c];
}

// J[r, c] = -S[r, c] / delta_r in place: d vech(Sigma) / d vech(Lambda) from S = symkron(Sigma, Sigma)
__global__ void lmvn_jac_rows_kernel(i64 total, i64 Pv, double* __restrict__ S)
{
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;
    const i64 r = k / Pv;
    S[k] *= lmvn_vech_diag(r) ? -1.0 : -0.5;
}

// Matrix-free product: per observation the directional changes (dmu, ds) -> e_m = c11 dmu + c12 ds, e_s = c12 dmu + c22 ds
__global__ void lmvn_hvp_coef_kernel(i64 n, const double* __restrict__ c11, const double* __restrict__ c12, const double* __restrict__ c22,
                                     const double* __restrict__ dmu, const double* __restrict__ ds, double* __restrict__ em,
                                     double* __restrict__ es)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = dmu[i], b = ds[i], k12 = c12[i];
    em[i] = c11[i] * a + k12 * b;
    es[i] = k12 * a + c22[i] * b;
}

// ---- row pass: r_n = x_n^T A x_n and t_n = x_n . b, A (P x P, P <= 64) resident in LDS, X streamed once ---------------------
// A workgroup walks tiles of 32 rows: the tile (32 P contiguous doubles) is loaded coalesced into LDS, then 8 lanes share a row,
// lane `part` forming y_j = (A x)_j for j = part, part + 8, ... and its share of x . y and x . b; three xor shuffles add the 8.
// LDS strides P + 1 / 65: the 8 parts read 8 different rows of A, the 8 rows of a wave 8 different rows of the tile, in
// different banks.  No P x N intermediate goes through HBM (DESIGN.md section 14 has the measurement against an A X^T GEMM).
constexpr int LMVN_RT = 32;              // rows per tile
constexpr int LMVN_XS = 65;              // LDS row stride of the tile
__global__ __launch_bounds__(256)
void lmvn_rowpass_kernel(i64 N, int P, const double* __restrict__ X, const double* __restrict__ A, const double* __restrict__ b,
                         double* __restrict__ r, double* __restrict__ t)
{
    __shared__ double As[64 * 65], xs[LMVN_RT * LMVN_XS], bs[64];
    const int tid = threadIdx.x, P1 = P + 1;
    for (int e = tid; e < P * P; e += 256) { const int j = e / P, k = e - j * P; As[j * P1 + k] = A[e]; }
    if (tid < P) bs[tid] = b[tid];
    const int row = tid >> 3, part = tid & 7;
    for (i64 t0 = (i64)blockIdx.x * LMVN_RT; t0 < N; t0 += (i64)gridDim.x * LMVN_RT) {
        const i64 rows = N - t0 < LMVN_RT ? N - t0 : LMVN_RT;
        __syncthreads();                                     // the previous tile is consumed (and A, b are in place)
        const double* src = X + t0 * P;
        for (int e = tid; e < (int)rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * LMVN_XS + cc] = src[e]; }
        __syncthreads();
        double rs = 0.0, ts = 0.0;
        if (row < rows) {
            const double* xr = xs + row * LMVN_XS;
            for (int j = part; j < P; j += 8) {
                const double* aj = As + j * P1;
                double y = 0.0;
                for (int k = 0; k < P; ++k) y += aj[k] * xr[k];
                rs += xr[j] * y;
                ts += xr[j] * bs[j];
            }
        }
        rs += __shfl_xor(rs, 1); ts += __shfl_xor(ts, 1);
        rs += __shfl_xor(rs, 2); ts += __shfl_xor(ts, 2);
        rs += __shfl_xor(rs, 4); ts += __shfl_xor(ts, 4);
        if (part == 0 && row < rows) { r[t0 + row] = rs; t[t0 + row] = ts; }
    }
}

int launch_lmvn_rowpass(lrvb_ctx* c, const double* A, const double* b, double* r, double* t) {
    const i64 N = c->N;
    if (c->P > 64) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "row pass: P <= 64");
    i64 tiles = (N + LMVN_RT - 1) / LMVN_RT;
    const unsigned grid = (unsigned)(tiles < 4096 ? (tiles < 1 ? 1 : tiles) : 4096);
    hipLaunchKernelGGL(lmvn_rowpass_kernel, dim3(grid), dim3(256), 0, c->stream, N, (int)c->P, (const double*)c->X.p, A, b, r, t);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// ---- cross block H_mSigma[a, v] = sum_n c_n x_na u_nv,  u_nv = x_nb x_ne for v = b (b + 1) / 2 + e (e <= b) ----------------------
// The operand U (N x Pv) is generated on chip and never touches HBM.  A workgroup owns a 64 x 64 output tile (rows a < 64: all of
// P; columns v of one 64-column slice of the packed triangle) over one split of the rows.  Each stage puts 16 rows of X and of
// c o X in LDS (zero past P and past N); wave w forms rows 16 w .. 16 w + 15 on v_mfma_f64_16x16x4_f64, the A operand c_n x_na read
// from LDS, the B operand the product of two LDS reads x_nb x_ne at per-lane column pairs computed once.  Columns past Pv read the
// zero slot.  Partial tiles per split; lmvn_cross_finish_kernel adds them in a fixed order and writes both triangles of H.
constexpr int LMVN_KC = 16;              // observations per stage
constexpr int LMVN_CS = 72;              // LDS row stride: [0, 64) x (zero past P), [64] = 0.0
constexpr int LMVN_ZERO = 64;
__global__ __launch_bounds__(256)
void lmvn_cross_kernel(const double* __restrict__ X, i64 N, int P, int pv, const double* __restrict__ cvec, int ntile,
                       i64 rows_per_split, double* __restrict__ partial)
{
    __shared__ double xs[LMVN_KC * LMVN_CS], cx[LMVN_KC * LMVN_CS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int tile = blockIdx.x % ntile, split = blockIdx.x / ntile;
    i64 r0 = (i64)split * rows_per_split, r1 = r0 + rows_per_split;
    if (r1 > N) r1 = N;
    // this lane's four B-operand columns v = 64 tile + 16 j + l15 as LDS column pairs
    int cb[4], ce[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = tile * 64 + 16 * j + l15;
        if (v >= pv) { cb[j] = ce[j] = LMVN_ZERO; continue; }
        int a = (int)((sqrtf(8.f * (float)v + 1.f) - 1.f) * 0.5f);
        while (a * (a + 1) / 2 > v) --a;
        while ((a + 1) * (a + 2) / 2 <= v) ++a;
        cb[j] = a; ce[j] = v - a * (a + 1) / 2;
    }
    const int arow = 16 * wave + l15;                        // A-operand row (output row a); rows >= P read zeros
    lmvn_d4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (lmvn_d4){0.0, 0.0, 0.0, 0.0};
    const int srow = tid >> 4, seg = tid & 15;               // stage: row srow, columns 4 seg .. 4 seg + 3
    for (i64 n0 = r0; n0 < r1; n0 += LMVN_KC) {
        const i64 n = n0 + srow;
        const bool live = n < r1;
        const double cn = live ? cvec[n] : 0.0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 4 * seg + q;
            const double xv = (live && col < P) ? X[n * P + col] : 0.0;
            xs[srow * LMVN_CS + col] = xv;
            cx[srow * LMVN_CS + col] = cn * xv;
        }
        if (seg == 0) { xs[srow * LMVN_CS + LMVN_ZERO] = 0.0; cx[srow * LMVN_CS + LMVN_ZERO] = 0.0; }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < LMVN_KC / 4; ++kk) {
            const int k = kk * 4 + l4;
            const double af = cx[k * LMVN_CS + arow];
            const double* xr = xs + k * LMVN_CS;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, xr[cb[j]] * xr[ce[j]], acc[j], 0, 0, 0);
        }
    }
    double* out = partial + ((i64)split * ntile + tile) * 4096;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(16 * wave + l4 + 4 * q) * 64 + 16 * j + l15] = acc[j][q];
}

// H[a, P + v] = H[P + v, a] = delta_v sum_s partial[s][tile(v)][a][v mod 64]  (a < P, v < Pv; fixed order over the splits)
__global__ void lmvn_cross_finish_kernel(i64 total, int P, i64 pv, int ntile, int n_splits, const double* __restrict__ partial,
                                         double* __restrict__ H, i64 ld)
{
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= total) return;                                  // total = P pv
    const i64 a = k / pv, v = k - a * pv;
    const i64 tile = v >> 6, col = v & 63;
    double s = 0.0;
    for (int sp = 0; sp < n_splits; ++sp) s += partial[(((i64)sp * ntile + tile) * 64 + a) * 64 + col];
    i64 b = (i64)((sqrt(8.0 * (double)v + 1.0) - 1.0) * 0.5);
    while (b * (b + 1) / 2 > v) --b;
    while ((b + 1) * (b + 2) / 2 <= v) ++b;
    if (v - b * (b + 1) / 2 != b) s *= 2.0;
    H[a * ld + P + v] = s;
    H[(P + v) * ld + a] = s;
}

int launch_lmvn_cross(lrvb_ctx* c, const double* cvec, double* H, i64 ld) {
    const i64 N = c->N, P = c->P, pv = P * (P + 1) / 2;
    if (P > 64) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "cross block: P <= 64");
    const int ntile = (int)((pv + 63) / 64);
    // ~2048 workgroups; every split at least 256 rows
    i64 S = (2048 + ntile - 1) / ntile;
    const i64 max_by_rows = N / 256;
    if (S > max_by_rows) S = max_by_rows;
    if (S < 1) S = 1;
    i64 rps = (N + S - 1) / S;
    rps = ((rps + LMVN_KC - 1) / LMVN_KC) * LMVN_KC;
    S = (N + rps - 1) / rps;
    if (S < 1) S = 1;
    LRVB_TRY(buf_reserve(c, c->tile_part, (size_t)(S * ntile * 4096)));
    hipLaunchKernelGGL(lmvn_cross_kernel, dim3((unsigned)(S * ntile)), dim3(256), 0, c->stream, (const double*)c->X.p, N, (int)P,
                       (int)pv, cvec, ntile, rps, c->tile_part.p);
    HIP_TRY(hipGetLastError());
    const i64 total = P * pv;
    hipLaunchKernelGGL(lmvn_cross_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, total, (int)P, pv, ntile,
                       (int)S, (const double*)c->tile_part.p, H, ld);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

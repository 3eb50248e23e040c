// k_glmm.hip -- logistic mixed model with a random intercept: y_n ~ Bernoulli(sigma(x_n . beta + u_g(n))), mean-field Gaussian
// q(beta_j) = N(m_j, v_j), q(u_g) = N(e_g, r_g).  Per observation rho_n = x_n . m + e_g(n), s_n = (x_n o x_n) . v + r_g(n) and
// psi(rho, s) = E log(1 + e^z), z ~ N(rho, s), by Gauss-Hermite with the derivative convention of lmvn_coef_kernel
// (k_logitmvn.hip: Stein's identity on the same nodes, no division by sd).
//
// glmm_rows_kernel is ONE pass over the rows in group-sorted order.  A workgroup (4 waves) walks tiles of GLMM_T = 64 sorted rows:
//   1. the tile's rows are gathered through the permutation into LDS (a row is contiguous in X, so the gather is row-granular;
//      any P, no alignment requirement -- there is no separate odd-P route);
//   2. four lanes share a row: each forms a quarter of the two dot products (m and v live in LDS), two xor shuffles add them,
//      then each lane evaluates a quarter of the quadrature nodes and two more shuffles add the five expectations -- all 256
//      lanes stay busy in the exp-class work;
//   3. lane 0 of the four writes the five coefficients a1, a2, c11, c12, c22 to the ORIGINAL row position (for the weighted
//      products X^T D X of the global block) and to LDS;
//   4. segmented sums from the tile still in LDS: thread c owns output column c of
//        [sum a1, sum a2, sum c11, sum c12, sum c22 | sum c11 x | sum c12 x | sum c12 x o x | sum c22 x o x]     (5 + 4 P columns)
//      and walks the tile's rows in order, flushing at every change of group.  A group that lies inside one tile is written
//      to its row of the result; the piece of a group cut by a tile boundary goes to one of the tile's two partial rows (slot 0:
//      the run that starts at the tile's first row, slot 1: the run that leaves through its last row) and glmm_fixup_kernel adds
//      the pieces of such a group in tile order.  No atomics anywhere: the result is a fixed-order sum, bitwise reproducible.
// Empty groups keep the zeros the caller wrote.
//
// This is the K-effect model of k_glmm_slopes.hip at K = 1 with z = 1, and everything that does not depend on the geometry of the
// walk is that file's (k_glmm_walk.h): the quadrature is LogisticLik (init, moments, coefs, infl), the head
// of a tile is gs_stage_sorted_tile without a design, the destination of a flush is gs_flush_dst.  What stays here is what makes
// this walk faster than the K = 1 instantiation: dot products that add a single e_g, r_g, the strides 65 and 66, one border column
// per thread (gl_walk_tile) and the MFMA loop of glmm_infl_rows_kernel.
#include "k_glmm_walk.h"

constexpr int GL_XS = 65;                // LDS row stride of the tile (odd: the four lanes of a row and 16 rows hit different banks)

// The segmented sums of one tile, in row order: thread tid owns output column NSC + tid (has_col: the staged column jc, squared
// where sq, times coefficient row ci) and, for tid < NSC, scalar column tid (the sum of coefficient row tid); a flush at every
// change of group, to gs_flush_dst.
template <int NSC>
__device__ __forceinline__ void gl_walk_tile(int tid, i64 tile, int rows, int ncol, bool has_col, int jc, int ci, bool sq, const double* xs,
                                             const double* cf, const int* s_gid, const int* s_whole, double* __restrict__ gsum,
                                             double* __restrict__ part)
{
    if (has_col || tid < NSC) {
        double acc = 0.0, accs = 0.0;
        int run_start = 0;
        for (int rr = 0; rr < rows; ++rr) {
            if (has_col) { double x = xs[rr * GL_XS + jc]; if (sq) x *= x; acc += cf[ci * GLMM_T + rr] * x; }
            if (tid < NSC) accs += cf[tid * GLMM_T + rr];
            const int g = s_gid[rr];
            if (rr == rows - 1 || s_gid[rr + 1] != g) {
                double* dst = gs_flush_dst(s_whole[rr], g, tile, run_start, ncol, gsum, part);
                if (has_col) dst[NSC + tid] = acc;
                if (tid < NSC) dst[tid] = accs;
                acc = 0.0; accs = 0.0; run_start = rr + 1;
            }
        }
    }
}

__global__ __launch_bounds__(256)
void glmm_rows_kernel(i64 N, int P, i64 G, const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w,
                      const i64* __restrict__ perm, const i64* __restrict__ offs, const double* __restrict__ m,
                      const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                      const double* __restrict__ gx, const double* __restrict__ gw, int K, double* __restrict__ coef, i64 NP,
                      double* __restrict__ gsum, double* __restrict__ part, double* __restrict__ vpart)
{
    __shared__ double xs[GLMM_T * GL_XS], cf[5 * GLMM_T], ms[64], vs[64], red[4];
    __shared__ LogisticLik::Lds lik;
    __shared__ i64 s_row[GLMM_T];
    __shared__ int s_gid[GLMM_T], s_whole[GLMM_T];
    const int tid = threadIdx.x;
    const int ncol = 5 + 4 * P;
    const LogisticLik::Args la{gx, gw, K};
    LogisticLik::init(lik, la, tid);
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    // the output column of this thread in the segmented sums: 5 + tid (tid < 4 P); threads 0..4 also carry scalar column tid
    const int blk = tid / P, jc = tid - blk * P;
    const bool has_col = tid < 4 * P;
    const int ci = blk == 0 ? 2 : (blk == 3 ? 4 : 3);                    // c11 | c12 | c12 | c22
    const bool sq = blk >= 2;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(N - t0 < GLMM_T ? N - t0 : GLMM_T);
        __syncthreads();                                                 // the previous tile is consumed (and the nodes are in place)
        gs_stage_sorted_tile<LogisticLik, GL_XS, false>(tid, t0, rows, P, 0, G, X, nullptr, perm, offs, la, lik, xs, s_row, s_gid, s_whole);
        double rho = 0.0, s = 0.0;
        if (row < rows) {
            const double* xr = xs + row * GL_XS;
            for (int j = q4; j < P; j += 4) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
        }
        rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
        rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
        if (row < rows) { const int g = s_gid[row]; rho += eg[g]; s += rg[g]; }
        const LogisticLik::Moments mo = LogisticLik::moments(lik, la, row < rows, q4, rho, s);
        double contrib = 0.0;
        if (q4 == 0) {
            double k[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (row < rows) {
                const i64 pr = s_row[row];
                contrib = LogisticLik::coefs(lik, row, mo, w[pr], y[pr], rho, s, k);
#pragma unroll
                for (int i = 0; i < 5; ++i) coef[i * NP + pr] = k[i];
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) cf[i * GLMM_T + row] = k[i];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) contrib += __shfl_xor(contrib, off);
        if ((tid & 63) == 0) red[tid >> 6] = contrib;
        __syncthreads();
        if (tid == 0) vpart[tile] = (red[0] + red[1]) + (red[2] + red[3]);
        // segmented sums over the tile's rows, in row order
        gl_walk_tile<5>(tid, tile, rows, ncol, has_col, jc, ci, sq, xs, cf, s_gid, s_whole, gsum, part);
    }
}

// the groups cut by tile boundaries: their pieces, one per tile they touch, added in tile order
__global__ __launch_bounds__(256)
void glmm_fixup_kernel(i64 G, int ncol, const i64* __restrict__ offs, const double* __restrict__ part, double* __restrict__ gsum)
{
    const i64 g = blockIdx.x;
    if (g >= G) return;
    const i64 gs = offs[g], ge = offs[g + 1];
    if (ge <= gs) return;
    const i64 tf = gs / GLMM_T, tl = (ge - 1) / GLMM_T;
    if (tf == tl) return;                                                // written by the rows kernel
    const int first_slot = (gs % GLMM_T) != 0 ? 1 : 0;
    for (int c = threadIdx.x; c < ncol; c += 256) {
        double acc = part[(tf * 2 + first_slot) * ncol + c];
#pragma unroll 4
        for (i64 t = tf + 1; t <= tl; ++t) acc += part[(t * 2) * ncol + c];
        gsum[g * ncol + c] = acc;
    }
}

int launch_glmm_rows(lrvb_ctx* c, const double* m, const double* vb, const double* eg, const double* rg, const double* gx,
                     const double* gw, int K, double* coef, i64 NP, double* gsum, double* part, double* vpart) {
    const i64 N = c->N, G = c->n_groups;
    if (c->P > 64) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "logistic mixed model: P <= 64");
    const int ncol = 5 + 4 * (int)c->P;
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    hipLaunchKernelGGL(glmm_rows_kernel, dim3(glmm_grid(N)), dim3(256), 0, c->stream, N, (int)c->P, G, (const double*)c->X.p,
                       (const double*)c->y.p, (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, gx, gw, K, coef, NP, gsum, part, vpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncol, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}
i64 glmm_num_tiles(i64 N) { return (N + GLMM_T - 1) / GLMM_T; }

// ---- streamed weight influence (lrvb_glmm_obs_influence) ----------------------------------------------------------------------
// out[n - n0][q] = a1' (x_n . A_m[q] + A_e[q, g(n)]) + a2' ((x_n o x_n) . A_v[q] + A_r[q, g(n)]),  a1' = psi_rho - y_n, a2' = psi_s
// PER UNIT WEIGHT (w_n does not enter: a row of weight zero gets the influence of adding it).  ONE pass over the rows n0..n1 in
// their original order, X read once for any Q.  A workgroup (4 waves) walks tiles of GLMM_T = 64 rows:
//   1. the tile (contiguous in X) is staged in LDS, row stride GI_XS; the columns P .. 4 ceil(P / 4) hold zeros;
//   2. four lanes share a row for the two dot products and the quadrature, as in glmm_rows_kernel, but only the two sums E g1
//      and E g2 are formed (no value, no second derivatives), and a1', a2' go to LDS;
//   3. wave w owns the rows 16 w .. 16 w + 15 of the tile.  Per block of 16 outputs it runs the two contractions
//      X A_m^T and (X o X) A_v^T as 16 x 16 x 4 fp64 MFMA tiles (A operand: lane (i = l & 15, k = l >> 4) reads one staged x and
//      squares it in a register -- X o X is never read from memory; B operand: A_global, zero past Q and past P), two
//      accumulator chains each, then combines them with a1', a2' and the gathered 2 Q-row of A_local in the D layout
//      (register r <-> row (l >> 4) + 4 r, column l & 15) and writes 16 consecutive doubles per row.
// With Q <= 16 the B fragments are loaded once per workgroup and stay in registers; with more outputs the blocks of 16 are a
// loop INSIDE the tile (the quadrature is shared, the fragments come from L2).  No atomics, no group walk.
constexpr int GI_XS = 66;                // LDS row stride: lanes (i, k) of an MFMA operand read banks 2 i + k

typedef double gi_d4 __attribute__((ext_vector_type(4)));

// The per-row part both influence kernels share: four lanes share the staged row xr -- each a quarter of the two dot products, then
// (LogisticLik::infl) a quarter of the nodes -- and every one of them returns e1 = psi_rho and e2 = E g2 = 2 psi_s of group g's row.
// Called by all lanes (xor shuffles); a lane whose row is not live returns zeros.
__device__ __forceinline__ void gi_psi_derivs(const double* xr, bool live, int g, int q4, int P, const double* ms, const double* vs,
                                              const double* __restrict__ eg, const double* __restrict__ rg, const LogisticLik::Lds& lik,
                                              const LogisticLik::Args& la, double& e1, double& e2)
{
    double rho = 0.0, s = 0.0;
    if (live) for (int j = q4; j < P; j += 4) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
    rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
    rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
    if (live) { rho += eg[g]; s += rg[g]; }
    LogisticLik::infl(lik, la, 0.0, live, q4, rho, s, e1, e2);
}

__global__ __launch_bounds__(256)
void glmm_infl_rows_kernel(i64 n0, i64 R /* rows of the window */, int P, const double* __restrict__ X, const double* __restrict__ y,
                           const int* __restrict__ gid, const double* __restrict__ m, const double* __restrict__ vb,
                           const double* __restrict__ eg, const double* __restrict__ rg, const double* __restrict__ gx,
                           const double* __restrict__ gw, int K, const double* __restrict__ Ag /* Q x 2 P */,
                           const double* __restrict__ Al /* G x 2 Q */, int Q, double* __restrict__ out /* R x Q */)
{
    __shared__ double xs[GLMM_T * GI_XS], a1s[GLMM_T], a2s[GLMM_T], ms[64], vs[64];
    __shared__ LogisticLik::Lds lik;
    __shared__ int s_gid[GLMM_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const LogisticLik::Args la{gx, gw, K};
    LogisticLik::init(lik, la, tid);
    if (tid < 64) { ms[tid] = tid < P ? m[tid] : 0.0; vs[tid] = tid < P ? vb[tid] : 0.0; }
    for (int e = tid; e < GLMM_T * GI_XS; e += 256) xs[e] = 0.0;           // the padding columns stay zero for the whole kernel
    const int KS = (P + 3) >> 2;                                         // k-steps of the contractions
    const int nqb = (Q + 15) >> 4;
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
        __syncthreads();                                                 // the previous tile is consumed (and the nodes are in place)
        if (tid < GLMM_T) s_gid[tid] = tid < rows ? gid[n0 + t0 + tid] : 0;
        {
            const double* src = X + (n0 + t0) * (i64)P;
            for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * GI_XS + cc] = src[e]; }
        }
        __syncthreads();
        double e1, e2;
        gi_psi_derivs(xs + row * GI_XS, row < rows, s_gid[row], q4, P, ms, vs, eg, rg, lik, la, e1, e2);
        if (q4 == 0) {
            double k1 = 0.0, k2 = 0.0;
            if (row < rows) { k1 = e1 - y[n0 + t0 + row]; k2 = 0.5 * e2; }
            a1s[row] = k1; a2s[row] = k2;
        }
        __syncthreads();
        // the two contractions of this wave's 16 rows
        const double* xa = xs + (16 * wave + l15) * GI_XS + l4;
        for (int qb = 0; qb < nqb; ++qb) {
            if (nqb > 1) load_b(qb);
            gi_d4 am0 = {0.0, 0.0, 0.0, 0.0}, am1 = am0, av0 = am0, av1 = am0;
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
                        const double* al = Al + (i64)s_gid[rr] * 2 * Q;
                        out[(t0 + rr) * (i64)Q + q] = a1s[rr] * ((am0[r] + am1[r]) + al[q]) + a2s[rr] * ((av0[r] + av1[r]) + al[Q + q]);
                    }
                }
            }
        }
    }
}

int launch_glmm_infl_rows(lrvb_ctx* c, i64 n0, i64 n1, const int* gid, const double* m, const double* vb, const double* eg,
                          const double* rg, const double* gx, const double* gw, int K, const double* Ag, const double* Al, i64 Q,
                          double* out) {
    if (c->P > 64) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "logistic mixed model: P <= 64");
    const i64 R = n1 - n0;
    if (R <= 0) return LRVB_OK;
    hipLaunchKernelGGL(glmm_infl_rows_kernel, dim3(glmm_grid(R)), dim3(256), 0, c->stream, n0, R, (int)c->P, (const double*)c->X.p,
                       (const double*)c->y.p, gid, m, vb, eg, rg, gx, gw, K, Ag, Al, (int)Q, out);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// ---- group influence (lrvb_glmm_group_influence) ------------------------------------------------------------------------------
// Per group the WEIGHTED sums  [sum a1, sum a2 | sum a1 x (P) | sum a2 x o x (P)],  a1 = w (psi_rho - y), a2 = w psi_s  (2 + 2 P
// columns), by the pass of glmm_rows_kernel cut down to them: group-sorted rows, two quadrature sums, the same in-order walk of
// the tile with the pieces of a cut group in the tile's two partial rows, added by glmm_fixup_kernel in tile order.  The
// contraction with the operand is N-independent: a (G x 2 P) (2 P x Q) product on the library's GEMM and glmm_infl_local_kernel
// for the two local columns.  Fixed order everywhere, no atomics.
__global__ __launch_bounds__(256)
void glmm_infl_gsum_kernel(i64 N, int P, i64 G, const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w,
                           const i64* __restrict__ perm, const i64* __restrict__ offs, const double* __restrict__ m,
                           const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                           const double* __restrict__ gx, const double* __restrict__ gw, int K, double* __restrict__ gsum,
                           double* __restrict__ part)
{
    __shared__ double xs[GLMM_T * GL_XS], cf[2 * GLMM_T], ms[64], vs[64];
    __shared__ LogisticLik::Lds lik;
    __shared__ i64 s_row[GLMM_T];
    __shared__ int s_gid[GLMM_T], s_whole[GLMM_T];
    const int tid = threadIdx.x;
    const int ncol = 2 + 2 * P;
    const LogisticLik::Args la{gx, gw, K};
    LogisticLik::init(lik, la, tid);
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GLMM_T - 1) / GLMM_T;
    const int row = tid >> 2, q4 = tid & 3;
    const bool has_col = tid < 2 * P;                                    // output column 2 + tid; threads 0, 1 also a scalar column
    const bool sq = tid >= P;
    const int jc = sq ? tid - P : tid;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GLMM_T;
        const int rows = (int)(N - t0 < GLMM_T ? N - t0 : GLMM_T);
        __syncthreads();
        gs_stage_sorted_tile<LogisticLik, GL_XS, false>(tid, t0, rows, P, 0, G, X, nullptr, perm, offs, la, lik, xs, s_row, s_gid, s_whole);
        double e1, e2;
        gi_psi_derivs(xs + row * GL_XS, row < rows, s_gid[row], q4, P, ms, vs, eg, rg, lik, la, e1, e2);
        if (q4 == 0) {
            double k1 = 0.0, k2 = 0.0;
            if (row < rows) { const i64 pr = s_row[row]; const double wi = w[pr]; k1 = wi * (e1 - y[pr]); k2 = wi * 0.5 * e2; }
            cf[row] = k1; cf[GLMM_T + row] = k2;
        }
        __syncthreads();
        gl_walk_tile<2>(tid, tile, rows, ncol, has_col, jc, sq ? 1 : 0, sq, xs, cf, s_gid, s_whole, gsum, part);
    }
}

// out[g][q] += S[g][0] A_e[q, g] + S[g][1] A_r[q, g]   (S: the group sums, leading dimension ncol; A_local: G x 2 Q)
__global__ __launch_bounds__(256)
void glmm_infl_local_kernel(i64 G, int Q, int ncol, const double* __restrict__ S, const double* __restrict__ Al, double* __restrict__ out)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= G * Q) return;
    const i64 g = i / Q;
    const int q = (int)(i - g * Q);
    out[i] += S[g * ncol] * Al[g * 2 * Q + q] + S[g * ncol + 1] * Al[g * 2 * Q + Q + q];
}

int launch_glmm_infl_gsum(lrvb_ctx* c, const double* m, const double* vb, const double* eg, const double* rg, const double* gx,
                          const double* gw, int K, double* gsum, double* part) {
    const i64 N = c->N, G = c->n_groups;
    if (c->P > 64) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "logistic mixed model: P <= 64");
    const int ncol = 2 + 2 * (int)c->P;
    const i64* gdev = reinterpret_cast<const i64*>(c->groups.p);
    hipLaunchKernelGGL(glmm_infl_gsum_kernel, dim3(glmm_grid(N)), dim3(256), 0, c->stream, N, (int)c->P, G, (const double*)c->X.p,
                       (const double*)c->y.p, (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, gx, gw, K, gsum, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncol, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

int launch_glmm_infl_local(lrvb_ctx* c, i64 Q, const double* S, const double* Al, double* out) {
    const i64 G = c->n_groups, n = G * Q;
    hipLaunchKernelGGL(glmm_infl_local_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, G, (int)Q,
                       2 + 2 * (int)c->P, S, Al, out);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

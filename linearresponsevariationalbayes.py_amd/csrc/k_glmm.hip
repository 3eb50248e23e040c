// k_glmm.hip -- logistic mixed model with a random intercept: y_n ~ Bernoulli(sigma(x_n . beta + u_g(n))), mean-field Gaussian
// q(beta_j) = N(m_j, v_j), q(u_g) = N(e_g, r_g).  Per observation rho_n = x_n . m + e_g(n), s_n = (x_n o x_n) . v + r_g(n) and
// psi(rho, s) = E log(1 + e^z), z ~ N(rho, s), by Gauss-Hermite with the derivative convention of lmvn_coef_kernel
// (k_logitmvn.hip: Stein's identity on the same nodes, no division by sd).
//
// glmm_rows_kernel is ONE pass over the rows in group-sorted order.  A workgroup (4 waves) walks tiles of GL_T = 64 sorted rows:
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
#include "lrvb_internal.h"
#include "k_kernels.h"
#include <math.h>

constexpr int GL_T = 64;                 // sorted rows per tile
constexpr int GL_XS = 65;                // LDS row stride of the tile (odd: the four lanes of a row and 16 rows hit different banks)

__global__ __launch_bounds__(256)
void glmm_rows_kernel(i64 N, int P, i64 G, const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w,
                      const i64* __restrict__ perm, const i64* __restrict__ offs, const double* __restrict__ m,
                      const double* __restrict__ vb, const double* __restrict__ eg, const double* __restrict__ rg,
                      const double* __restrict__ gx, const double* __restrict__ gw, int K, double* __restrict__ coef, i64 NP,
                      double* __restrict__ gsum, double* __restrict__ part, double* __restrict__ vpart)
{
    __shared__ double xs[GL_T * GL_XS], cf[5 * GL_T], ms[64], vs[64], sx[128], sw[128], red[4];
    __shared__ i64 s_row[GL_T];
    __shared__ int s_gid[GL_T], s_whole[GL_T];
    const int tid = threadIdx.x;
    const int ncol = 5 + 4 * P;
    const double r2 = 1.4142135623730951, ispi = 0.5641895835477563;     // sqrt(2), 1 / sqrt(pi)
    if (tid < K) { sx[tid] = r2 * gx[tid]; sw[tid] = ispi * gw[tid]; }
    if (tid < P) { ms[tid] = m[tid]; vs[tid] = vb[tid]; }
    const i64 n_tiles = (N + GL_T - 1) / GL_T;
    const int row = tid >> 2, q4 = tid & 3;
    // the output column of this thread in the segmented sums: 5 + tid (tid < 4 P); threads 0..4 also carry scalar column tid
    const int blk = tid / P, jc = tid - blk * P;
    const bool has_col = tid < 4 * P;
    const int ci = blk == 0 ? 2 : (blk == 3 ? 4 : 3);                    // c11 | c12 | c12 | c22
    const bool sq = blk >= 2;
    for (i64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const i64 t0 = tile * GL_T;
        const int rows = (int)(N - t0 < GL_T ? N - t0 : GL_T);
        __syncthreads();                                                 // the previous tile is consumed (and the nodes are in place)
        if (tid < GL_T) {
            int g = 0, whole = 0;
            i64 pr = 0;
            if (tid < rows) {
                const i64 i = t0 + tid;
                pr = perm[i];
                i64 lo = 0, hi = G;                                      // the last g with offs[g] <= i (its offs[g + 1] > i)
                while (hi - lo > 1) { const i64 mid = (lo + hi) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid; }
                g = (int)lo;
                whole = (offs[lo] >= t0 && offs[lo + 1] <= t0 + GL_T) ? 1 : 0;
            }
            s_row[tid] = pr; s_gid[tid] = g; s_whole[tid] = whole;
        }
        __syncthreads();
        for (int e = tid; e < rows * P; e += 256) { const int rr = e / P, cc = e - rr * P; xs[rr * GL_XS + cc] = X[s_row[rr] * P + cc]; }
        __syncthreads();
        double rho = 0.0, s = 0.0;
        if (row < rows) {
            const double* xr = xs + row * GL_XS;
            for (int j = q4; j < P; j += 4) { const double x = xr[j]; rho += x * ms[j]; s += x * x * vs[j]; }
        }
        rho += __shfl_xor(rho, 1); s += __shfl_xor(s, 1);
        rho += __shfl_xor(rho, 2); s += __shfl_xor(s, 2);
        double v = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0, e4 = 0.0;
        if (row < rows) {
            const int g = s_gid[row];
            rho += eg[g]; s += rg[g];
            const double sd = sqrt(fmax(s, 0.0));
            for (int k = q4; k < K; k += 4) {
                const double t = rho + sd * sx[k], wk = sw[k];
                const double e = exp(-fabs(t)), ie = 1.0 / (1.0 + e);
                const double sp = (t > 0.0 ? t : 0.0) + log1p(e);
                const double sg = t >= 0.0 ? ie : e * ie;
                const double g2 = e * ie * ie;
                const double om = (1.0 - e) * ie;                        // |1 - 2 sigma|
                const double g3 = t >= 0.0 ? -g2 * om : g2 * om;
                v += wk * sp; e1 += wk * sg; e2 += wk * g2; e3 += wk * g3; e4 += wk * g2 * (1.0 - 6.0 * g2);
            }
        }
#pragma unroll
        for (int off = 1; off <= 2; off <<= 1) {
            v += __shfl_xor(v, off); e1 += __shfl_xor(e1, off); e2 += __shfl_xor(e2, off);
            e3 += __shfl_xor(e3, off); e4 += __shfl_xor(e4, off);
        }
        double contrib = 0.0;
        if (q4 == 0) {
            double k1 = 0.0, k2 = 0.0, k11 = 0.0, k12 = 0.0, k22 = 0.0;
            if (row < rows) {
                const i64 pr = s_row[row];
                const double wi = w[pr], yi = y[pr];
                contrib = wi * (v - yi * rho);
                k1 = wi * (e1 - yi); k2 = wi * 0.5 * e2; k11 = wi * e2; k12 = wi * 0.5 * e3; k22 = wi * 0.25 * e4;
                coef[pr] = k1; coef[NP + pr] = k2; coef[2 * NP + pr] = k11; coef[3 * NP + pr] = k12; coef[4 * NP + pr] = k22;
            }
            cf[row] = k1; cf[GL_T + row] = k2; cf[2 * GL_T + row] = k11; cf[3 * GL_T + row] = k12; cf[4 * GL_T + row] = k22;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) contrib += __shfl_xor(contrib, off);
        if ((tid & 63) == 0) red[tid >> 6] = contrib;
        __syncthreads();
        if (tid == 0) vpart[tile] = (red[0] + red[1]) + (red[2] + red[3]);
        // segmented sums over the tile's rows, in row order
        if (has_col || tid < 5) {
            double acc = 0.0, accs = 0.0;
            int run_start = 0;
            for (int rr = 0; rr < rows; ++rr) {
                if (has_col) { double x = xs[rr * GL_XS + jc]; if (sq) x *= x; acc += cf[ci * GL_T + rr] * x; }
                if (tid < 5) accs += cf[tid * GL_T + rr];
                const int g = s_gid[rr];
                if (rr == rows - 1 || s_gid[rr + 1] != g) {
                    double* dst = s_whole[rr] ? gsum + (i64)g * ncol : part + (tile * 2 + (run_start == 0 ? 0 : 1)) * ncol;
                    if (has_col) dst[5 + tid] = acc;
                    if (tid < 5) dst[tid] = accs;
                    acc = 0.0; accs = 0.0; run_start = rr + 1;
                }
            }
        }
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
    const i64 tf = gs / GL_T, tl = (ge - 1) / GL_T;
    if (tf == tl) return;                                                // written by the rows kernel
    const int first_slot = (gs % GL_T) != 0 ? 1 : 0;
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
    const i64 n_tiles = (N + GL_T - 1) / GL_T;
    const unsigned grid = (unsigned)(n_tiles < 2048 ? (n_tiles < 1 ? 1 : n_tiles) : 2048);
    hipLaunchKernelGGL(glmm_rows_kernel, dim3(grid), dim3(256), 0, c->stream, N, (int)c->P, G, (const double*)c->X.p,
                       (const double*)c->y.p, (const double*)c->w.p, gdev, gdev + N, m, vb, eg, rg, gx, gw, K, coef, NP, gsum, part, vpart);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(glmm_fixup_kernel, dim3((unsigned)G), dim3(256), 0, c->stream, G, ncol, gdev + N, (const double*)part, gsum);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}
i64 glmm_num_tiles(i64 N) { return (N + GL_T - 1) / GL_T; }

// ---- elimination of the 2 G local parameters -------------------------------------------------------------------------------
// Per group g: A_g = [a11 a12; a12 a22] (the complete local block in free coordinates, from the host) = L L^T, and the two
// border rows over the R = 2 P + 3 coupled global coordinates [m (P) | v (P) | e_mu, a, b]
//   c_e = f_e [sum c11 x | sum c12 x o x | closed_e (3)],   c_r = f_r [sum c12 x | sum c22 x o x | closed_r (3)]
// from the RESIDENT group sums.  The kernel writes U_g = L^-1 [c_e; c_r] (2 x R), so that sum_g C_g A_g^-1 C_g^T = U^T U is one
// Gram over 2 G rows.  A block that is not positive definite raises the flag.
__global__ __launch_bounds__(128)
void glmm_schur_rows_kernel(i64 G, int P, const double* __restrict__ gsum, const double* __restrict__ loc /* G x 3 */,
                            const double* __restrict__ scale /* G x 2 */, const double* __restrict__ closed /* G x 6 */,
                            double* __restrict__ U, int ldu, int* __restrict__ bad)
{
    const i64 g = blockIdx.x;
    if (g >= G) return;
    const int ncol = 5 + 4 * P, R = 2 * P + 3;
    const double a11 = loc[g * 3], a12 = loc[g * 3 + 1], a22 = loc[g * 3 + 2];
    const bool ok1 = a11 > 0.0;
    const double l11 = sqrt(ok1 ? a11 : 1.0), l21 = a12 / l11, d = a22 - l21 * l21;
    const bool ok = ok1 && d > 0.0;
    if (!ok && threadIdx.x == 0) *bad = 1;
    const double l22 = sqrt(ok ? d : 1.0);
    const double fe = scale[g * 2], fr = scale[g * 2 + 1];
    const double* gs = gsum + g * ncol;
    for (int c = threadIdx.x; c < R; c += 128) {
        double ce, cr;
        if (c < P) { ce = gs[5 + c]; cr = gs[5 + P + c]; }
        else if (c < 2 * P) { ce = gs[5 + 2 * P + (c - P)]; cr = gs[5 + 3 * P + (c - P)]; }
        else { ce = closed[g * 6 + (c - 2 * P)]; cr = closed[g * 6 + 3 + (c - 2 * P)]; }
        const double u1 = fe * ce / l11;
        const double u2 = (fr * cr - l21 * u1) / l22;
        U[(2 * g) * ldu + c] = u1;
        U[(2 * g + 1) * ldu + c] = u2;
    }
}

int launch_glmm_schur_rows(lrvb_ctx* c, const double* gsum, const double* loc, const double* scale, const double* closed,
                           double* U, int ldu, int* bad) {
    const i64 G = c->n_groups;
    hipLaunchKernelGGL(glmm_schur_rows_kernel, dim3((unsigned)G), dim3(128), 0, c->stream, G, (int)c->P, gsum, loc, scale, closed, U, ldu, bad);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// k_softmax.hip -- multinomial (softmax) regression: the fused observation pass, the Hessian weight columns and the
// streamed weight-sensitivity rows.
//
// K classes, class 0 the reference, B = beta ((K-1) x P, row a = class a + 1), z_na = x_n . beta_a, z_n0 = 0,
// p_n = softmax(z_n), r_na = w_n (p_na - [y_n = a + 1]).  With Km = K - 1 <= 16 one row's Km columns are one 16-lane DPP row
// of the T tile of hvp_multi_kernel (k_hvp_multi.hip), whose structure this pass keeps:
//
//   chunk = 8 observations x P columns, staged by LDS-DMA (double buffered), with its weights, labels and p rows
//   step A:  T (8 x 16)   = X_chunk U                     U = beta (gradient mode) or the product vectors V (product mode)
//   mix  :  per row, across the 16 lanes that hold it      (DPP row_ror reductions: max, sums)
//            gradient mode: p = softmax(t), value += w (lse - z_y), t <- w (p - e_y), p written out
//            product  mode: t <- w p o (t - p . t)        (p of the point, staged with the chunk)
//   step B:  R (P x 16)  += X_chunk^T (mixed T)
//
// One read of X per pass.  Any 1 <= P <= 1024: even P with 16-byte aligned rows stages by 16-byte DMA (as k_hvp_multi.hip),
// odd P (or unaligned X) by 4-byte DMA into the same LDS image (four times the instructions; the parity-preserving clamp
// keeps padding columns finite, and they meet zeros of U).
#include "lrvb_internal.h"
#include "k_kernels.h"
#include <math.h>

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

#define SM_GLDS16_S(sbase, voff, ldsaddr) asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1 nt" \
    :: "v"(voff), "s"(sbase), "s"(ldsaddr) : "memory")
#define SM_GLDS4_S(sbase, voff, ldsaddr) asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dword %0, %1" \
    :: "v"(voff), "s"(sbase), "s"(ldsaddr) : "memory")

constexpr int SM_ROWS = 8;                 // observations per chunk
constexpr int SM_GRID = 256;               // one workgroup per CU

// defined in k_hvp_multi.hip: Out[q][off + p] = sum over workgroups of Rpart[g][p][q] (fixed order)
__global__ __launch_bounds__(256)
void hvp_multi_reduce_kernel(const double* __restrict__ Rpart, int G, int P, int Ppad, int Q, i64 ldo, i64 off,
                             double* __restrict__ Out, const double* __restrict__ live);

// ---- one DPP row (16 lanes) --------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// row_ror:8, 4, 2, 1 -- every lane of the row ends with the full reduction
__device__ __forceinline__ double row16_sum(double v) {
    v += dpp_d<0x128>(v); v += dpp_d<0x124>(v); v += dpp_d<0x122>(v); v += dpp_d<0x121>(v);
    return v;
}
__device__ __forceinline__ double row16_max(double v) {
    v = fmax(v, dpp_d<0x128>(v)); v = fmax(v, dpp_d<0x124>(v)); v = fmax(v, dpp_d<0x122>(v)); v = fmax(v, dpp_d<0x121>(v));
    return v;
}

enum { SM_GRAD = 0, SM_HVP = 1 };

// a wave-uniform address in SGPRs (the scalar base of an LDS-DMA instruction), computed before a lane-divergent branch
__device__ __forceinline__ const char* sm_uniform(const void* p) {
    const uintptr_t a = (uintptr_t)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return reinterpret_cast<const char*>(((uintptr_t)hi << 32) | lo);
}

// NB = ceil(P / 128); TONLY: step A only, Tout[n][q] = w_n (X U)[n][q] (the streamed influence rows); NW waves; ODD: 4-byte staging;
// MODE = SM_GRAD or SM_HVP, a compile-time choice: with one runtime kernel for both modes the 8-wave P = 1024 instance kept
// both modes' row state live and spilled (256 VGPRs + 92 bytes of scratch per lane, reloaded inside the chunk loop)
template <int NB, bool TONLY, int NW, bool ODD, int MODE>
__global__ __launch_bounds__(64 * NW, 1)
void softmax_pass_kernel(const double* __restrict__ X, int Preal, i64 N, const double* __restrict__ cw /* N + 64, zero padded */,
                         const int* __restrict__ labels /* N + 64, zero padded */, double* __restrict__ pbuf /* N Km + pad */,
                         const double* __restrict__ U, i64 ldu, int Q, double* __restrict__ Rpart,
                         double* __restrict__ valpart, double* __restrict__ Tout, i64 ldt)
{
    constexpr int P = NB * 128;
    constexpr int PW = P / NW;
    constexpr int NBW = PW / 32;
    constexpr int RPW = SM_ROWS / NW;
    constexpr int STRIDE = P + 2;
    constexpr int NT = PW / 16;
    constexpr int OFF_T = 2 * SM_ROWS * STRIDE;              // [2][NW][2][64] partial T tiles
    constexpr int OFF_C = OFF_T + 2 * NW * 2 * 64;           // [2][8] weights
    constexpr int OFF_Y = OFF_C + 2 * SM_ROWS;               // [2][8 doubles] labels (8 int32 used)
    constexpr int OFF_P = OFF_Y + 2 * SM_ROWS;               // [2][128] p rows of the chunk (8 x Km)
    extern __shared__ double lds[];
    double* Tpart = lds + OFF_T;
    const double* Cst = lds + OFF_C;
    const int* Yst = reinterpret_cast<const int*>(lds + OFF_Y);
    const double* Pst = lds + OFF_P;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int pc0 = wave * PW;
    const int Km = Q;
    constexpr bool grad = (MODE == SM_GRAD);

    double uf[NBW][8];
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = pc0 + 32 * b + 8 * l4 + t;
            uf[b][t] = (l15 < Q && k < Preal) ? U[(i64)l15 * ldu + k] : 0.0;
        }
    d4 acc[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m) acc[m] = (d4){0.0, 0.0, 0.0, 0.0};

    const i64 nchunks = (N + SM_ROWS - 1) / SM_ROWS;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)lds;
    constexpr int NI = ODD ? 4 * NB : NB;                     // DMA instructions per row
    unsigned voff[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        if (ODD) {
            int d = 64 * j + lane;                            // 4-byte word of the row
            if (d > 2 * Preal - 1) d = 2 * Preal - 2 + (d & 1);   // stays on the last column: finite, meets zeros of U
            voff[j] = (unsigned)d * 4u;
        } else {
            int col = 128 * j + 2 * lane; if (col > Preal - 2) col = Preal - 2;
            voff[j] = (unsigned)col * 8u;
        }
    }
    auto issue = [&](i64 ch, int buf) {
        const unsigned base = lds0 + (unsigned)(buf * (SM_ROWS * STRIDE)) * 8u;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int row = RPW * wave + rr;
            i64 n = ch * SM_ROWS + row; if (n > N - 1) n = N - 1;
            const char* rowp = reinterpret_cast<const char*>(X + n * (i64)Preal);
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                if (ODD) SM_GLDS4_S(rowp, voff[j], base + (unsigned)(row * STRIDE + 32 * j) * 8u);
                else     SM_GLDS16_S(rowp, voff[j], base + (unsigned)(row * STRIDE + 128 * j) * 8u);
            }
        }
        const char* cwp = sm_uniform(cw + ch * SM_ROWS);
        if (wave == 0 && lane < 16)            // the chunk's 8 weights
            SM_GLDS4_S(cwp, (unsigned)lane * 4u, lds0 + (unsigned)(OFF_C + buf * SM_ROWS) * 8u);
        if (!TONLY) {
            if constexpr (grad) {
                const char* yp = sm_uniform(labels + ch * SM_ROWS);
                if (wave == 1 && lane < SM_ROWS)   // its 8 labels
                    SM_GLDS4_S(yp, (unsigned)lane * 4u, lds0 + (unsigned)(OFF_Y + buf * SM_ROWS) * 8u);
            } else {
                const char* pp = sm_uniform(pbuf + ch * SM_ROWS * Km);
                if (wave == 1 && lane < 4 * Km)    // its 8 x Km probabilities (contiguous in pbuf)
                    SM_GLDS16_S(pp, (unsigned)lane * 16u, lds0 + (unsigned)(OFF_P + buf * 128) * 8u);
            }
        }
    };

    const i64 cend = nchunks;
    i64 ch = blockIdx.x;
    const i64 step = gridDim.x;
    int buf = 0;
    auto step_a = [&](const double* Xs, double (&tp)[2]) {
        const double* arow = Xs + (lane & 3) * STRIDE + pc0 + 8 * l4;
        double tpa[2] = {0.0, 0.0}, tpb[2] = {0.0, 0.0};
        d2 fr[2][8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fr[0][i] = *reinterpret_cast<const d2*>(arow + 2 * i);
            fr[0][4 + i] = *reinterpret_cast<const d2*>(arow + 4 * STRIDE + 2 * i);
        }
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
            const int cur = b & 1;
            if (b + 1 < NBW) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    fr[cur ^ 1][i] = *reinterpret_cast<const d2*>(arow + 32 * (b + 1) + 2 * i);
                    fr[cur ^ 1][4 + i] = *reinterpret_cast<const d2*>(arow + 4 * STRIDE + 32 * (b + 1) + 2 * i);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 8; t += 2) {
                tpa[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(fr[cur][t >> 1][0], uf[b][t], tpa[0], 0, 0, 0);
                tpa[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(fr[cur][4 + (t >> 1)][0], uf[b][t], tpa[1], 0, 0, 0);
                tpb[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(fr[cur][t >> 1][1], uf[b][t + 1], tpb[0], 0, 0, 0);
                tpb[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(fr[cur][4 + (t >> 1)][1], uf[b][t + 1], tpb[1], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        tp[0] = tpa[0] + tpb[0]; tp[1] = tpa[1] + tpb[1];
    };
    // T of a chunk (raw, unscaled) from the partial tiles in LDS: register s <-> row l4 + 4 s, lane l15 <-> column q
    auto gather_raw = [&](const double* Tp, double& t0, double& t1) {
        double pa[NW], pb[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) { pa[w] = Tp[(w * 2 + 0) * 64 + lane]; pb[w] = Tp[(w * 2 + 1) * 64 + lane]; }
        __builtin_amdgcn_sched_barrier(0);
        t0 = pa[0]; t1 = pb[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) { t0 += pa[w]; t1 += pb[w]; }
    };

    if (TONLY) {
        if (ch < cend) issue(ch, 0);
        for (; ch < cend; ch += step) {
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __syncthreads();
            const double c0 = Cst[buf * SM_ROWS + l4], c1 = Cst[buf * SM_ROWS + 4 + l4];
            const i64 nxt = ch + step;
            if (nxt < cend) issue(nxt, buf ^ 1);
            double tp[2];
            step_a(lds + buf * (SM_ROWS * STRIDE), tp);
            Tpart[(wave * 2 + 0) * 64 + lane] = tp[0];
            Tpart[(wave * 2 + 1) * 64 + lane] = tp[1];
            __builtin_amdgcn_s_waitcnt(0xC07F);               // lgkmcnt(0)
            __builtin_amdgcn_s_barrier();
            double t0, t1;
            gather_raw(Tpart, t0, t1);
            if (wave == 0 && l15 < Q) {
                const i64 n = ch * SM_ROWS + l4;
                if (n < N) Tout[n * ldt + l15] = c0 * t0;
                if (n + 4 < N) Tout[(n + 4) * ldt + l15] = c1 * t1;
            }
            buf ^= 1;
        }
        return;
    }

    // per-row mixing of one T register (row n, weight cw, label y or probability pq of this lane's class)
    double vacc = 0.0;
    auto mix = [&](double t, double w, int y, double pq, i64 n) -> double {
        const bool act = l15 < Km;
        if constexpr (grad) {
            const double z = act ? t : -INFINITY;
            const double m = row16_max(fmax(z, 0.0));
            const double e = act ? exp(z - m) : 0.0;
            const double s = row16_sum(e) + exp(-m);
            const double p = e / s;
            const bool hit = act && (l15 == y - 1);
            const double zy = row16_sum(hit ? z : 0.0);
            if (wave == 0) {
                if (l15 == 0) vacc += w * (m + log(s) - zy);
                if (act && n < N) pbuf[n * Km + l15] = p;
            }
            return w * (p - (hit ? 1.0 : 0.0));
        } else {
            const double pt = act ? pq * t : 0.0;
            const double s = row16_sum(pt);
            return act ? w * pq * (t - s) : 0.0;
        }
    };
    struct RowInfo { double c0, c1, p0, p1; int y0, y1; };
    auto load_info = [&](int b, RowInfo& ri) {
        ri.c0 = Cst[b * SM_ROWS + l4]; ri.c1 = Cst[b * SM_ROWS + 4 + l4];
        ri.y0 = 0; ri.y1 = 0; ri.p0 = 0.0; ri.p1 = 0.0;
        if constexpr (grad) { ri.y0 = Yst[b * 2 * SM_ROWS + l4]; ri.y1 = Yst[b * 2 * SM_ROWS + 4 + l4]; }
        else if (l15 < Km) { ri.p0 = Pst[b * 128 + l4 * Km + l15]; ri.p1 = Pst[b * 128 + (4 + l4) * Km + l15]; }
    };

    const double* brow0_0 = lds + l4 * STRIDE + pc0 + 2 * l15;
    d2 xb[NT / 2][2];
    RowInfo prev{};
    i64 chprev = 0;
    bool have_prev = false;
    int slot = 0;
    auto step_b = [&](double t0, double t1) {
#pragma unroll
        for (int h = 0; h < NT / 2; ++h) {
            acc[2 * h]     = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[h][0][0], t0, acc[2 * h], 0, 0, 0);
            acc[2 * h + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[h][0][1], t0, acc[2 * h + 1], 0, 0, 0);
            acc[2 * h]     = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[h][1][0], t1, acc[2 * h], 0, 0, 0);
            acc[2 * h + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[h][1][1], t1, acc[2 * h + 1], 0, 0, 0);
        }
    };
    auto mix_and_b = [&](const double* Tp) {
        double t0, t1;
        gather_raw(Tp, t0, t1);
        const i64 n = chprev * SM_ROWS + l4;
        t0 = mix(t0, prev.c0, prev.y0, prev.p0, n);
        t1 = mix(t1, prev.c1, prev.y1, prev.p1, n + 4);
        step_b(t0, t1);
    };
    if (ch < cend) issue(ch, 0);
    for (; ch < cend; ch += step) {
        __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0)
        __syncthreads();
        RowInfo cur;
        load_info(buf, cur);
        const i64 nxt = ch + step;
        if (nxt < cend) issue(nxt, buf ^ 1);
        if (have_prev) mix_and_b(Tpart + (slot ^ 1) * (NW * 2 * 64));
        const double* Xs = lds + buf * (SM_ROWS * STRIDE);
        double tp[2];
        step_a(Xs, tp);
        double* Tp = Tpart + slot * (NW * 2 * 64);
        Tp[(wave * 2 + 0) * 64 + lane] = tp[0];
        Tp[(wave * 2 + 1) * 64 + lane] = tp[1];
        const double* b0 = brow0_0 + buf * (SM_ROWS * STRIDE);
#pragma unroll
        for (int h = 0; h < NT / 2; ++h) {
            xb[h][0] = *reinterpret_cast<const d2*>(b0 + 32 * h);
            xb[h][1] = *reinterpret_cast<const d2*>(b0 + 4 * STRIDE + 32 * h);
        }
        prev = cur; chprev = ch; have_prev = true;
        slot ^= 1; buf ^= 1;
    }
    if (have_prev) {
        __syncthreads();
        mix_and_b(Tpart + (slot ^ 1) * (NW * 2 * 64));
    }
    double* out = Rpart + (i64)blockIdx.x * P * 16;
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = pc0 + 32 * (m >> 1) + 2 * (l4 + 4 * r) + (m & 1);
            out[p * 16 + l15] = acc[m][r];
        }
    if (wave == 0) {                                          // value partial of this workgroup (lanes l15 == 0 hold it)
        double v = vacc;
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) valpart[blockIdx.x] = v;
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------
static bool sm_odd(const lrvb_ctx* c) { return (c->P % 2) != 0 || ((((uintptr_t)c->X.p) & 15) != 0); }
static size_t sm_lds_bytes(int Ppad, int NW) {
    return (size_t)(2 * SM_ROWS * (Ppad + 2) + 2 * NW * 2 * 64 + 2 * SM_ROWS + 2 * SM_ROWS + 2 * 128) * sizeof(double);
}

template <int NB, bool TONLY, int NW, bool ODD, int MODE>
static int sm_launch(lrvb_ctx* c, int grid, const double* X, i64 N, const double* cw, const int* labels, double* pbuf,
                     const double* U, i64 ldu, int Q, double* Rpart, double* valpart, double* Tout, i64 ldt) {
    const size_t lds = sm_lds_bytes(NB * 128, NW);
    auto k = &softmax_pass_kernel<NB, TONLY, NW, ODD, MODE>;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64 * NW), lds, c->stream, X, (int)c->P, N, cw, labels, pbuf, U, ldu, Q,
                       Rpart, valpart, Tout, ldt);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

template <bool TONLY>
static int sm_dispatch(lrvb_ctx* c, int grid, const double* X, i64 N, const double* cw, const int* labels, double* pbuf,
                       const double* U, i64 ldu, int Q, int mode, double* Rpart, double* valpart, double* Tout, i64 ldt) {
    const int nb = (int)((c->P + 127) / 128);
    const bool odd = sm_odd(c);
    const bool eight = !odd && (nb % 2 == 0) && !c->hm_four_waves;
#define SM_ARGS c, grid, X, N, cw, labels, pbuf, U, ldu, Q, Rpart, valpart, Tout, ldt
// The gradient mode at P = 1024 runs 4 waves: with 8 its exp / log temporaries on top of the resident U slice, accumulators
// and step-B fragments took 256 VGPRs and 60 bytes of scratch per lane (reloaded inside the chunk loop); the 4-wave
// instance fits in 256 with none.  Every instance launched here has ScratchSize 0 (-Rpass-analysis=kernel-resource-usage).
#define SM_MODE(NB, NW, ODD) do { \
        if (TONLY || mode == SM_GRAD) return sm_launch<NB, TONLY, ((NB == 8 && !TONLY) ? 4 : NW), ODD, SM_GRAD>(SM_ARGS); \
        return sm_launch<NB, TONLY, NW, ODD, (TONLY ? SM_GRAD : SM_HVP)>(SM_ARGS); } while (0)
#define SM_CASE(NB) case NB: \
        if (odd) SM_MODE(NB, 4, true); \
        if (eight) SM_MODE((NB % 2 == 0 ? NB : 2), 8, false); \
        SM_MODE(NB, 4, false);
    switch (nb) {
    SM_CASE(1) SM_CASE(2) SM_CASE(3) SM_CASE(4) SM_CASE(5) SM_CASE(6) SM_CASE(7) SM_CASE(8)
    default: break;
    }
#undef SM_CASE
#undef SM_MODE
#undef SM_ARGS
    LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "softmax pass: 1 <= P <= 1024");
}

bool softmax_supported(i64 K, i64 P) { return K >= 2 && K <= 17 && P >= 1 && P <= 1024; }

// mode SM_GRAD: out (Km x P, row-major) = X^T R, value_dev[0] = sum_n w_n (lse_n - z_{n, y_n}), p written to pbuf
// mode SM_HVP:  out = X^T (w p o (X V^T - p . X V^T)) with p read from pbuf.  U: Km rows of P (device).
int launch_softmax_pass(lrvb_ctx* c, int mode, int Km, const double* U_dev, const double* cw_pad, const int* labels_pad,
                        double* pbuf, double* out_dev, double* value_dev) {
    if (!softmax_supported(Km + 1, c->P)) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "softmax pass: 2 <= K <= 17, 1 <= P <= 1024");
    const int Ppad = (int)(((c->P + 127) / 128) * 128);
    const i64 nchunks = (c->N + SM_ROWS - 1) / SM_ROWS;
    const int grid = (int)(nchunks < SM_GRID ? nchunks : SM_GRID);
    LRVB_TRY(buf_reserve(c, c->part_vec, (size_t)grid * (size_t)Ppad * 16));
    LRVB_TRY(buf_reserve(c, c->part_val, (size_t)SM_GRID));
    if (c->prof_on) LRVB_TRY(prof_mark(c, PROF_PASS));
    LRVB_TRY(sm_dispatch<false>(c, grid, c->X.p, c->N, cw_pad, labels_pad, pbuf, U_dev, c->P, Km, mode, c->part_vec.p,
                                c->part_val.p, nullptr, 0));
    hipLaunchKernelGGL(hvp_multi_reduce_kernel, dim3((unsigned)((c->P * 16 + 31) / 32)), dim3(256), 0, c->stream,
                       (const double*)c->part_vec.p, grid, (int)c->P, Ppad, Km, (i64)c->P, (i64)0, out_dev, (const double*)nullptr);
    HIP_TRY(hipGetLastError());
    if (value_dev) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)c->part_val.p, (i64)grid, value_dev);
        HIP_TRY(hipGetLastError());
    }
    if (c->prof_on) {
        LRVB_TRY(prof_mark(c, PROF_PASS));
        c->prof.pass_bytes = 8.0 * (double)c->N * (double)c->P;
    }
    return LRVB_OK;
}

// Tout[n - n0][j] = w_n x_n . Zt[j]  for n0 <= n < n1 and j < Q <= 16 (Zt: Q rows of P, stride ldz)
int launch_softmax_rows(lrvb_ctx* c, i64 n0, i64 n1, int Q, const double* Zt_dev, i64 ldz, const double* cw_pad,
                        double* Tout_dev, i64 ldt) {
    const i64 rows = n1 - n0;
    if (rows <= 0) return LRVB_OK;
    if (Q < 1 || Q > 16) LRVB_FAIL(LRVB_ERR_UNSUPPORTED, "softmax rows: 1 to 16 columns per launch");
    const i64 nchunks = (rows + SM_ROWS - 1) / SM_ROWS;
    const int grid = (int)(nchunks < SM_GRID ? nchunks : SM_GRID);
    return sm_dispatch<true>(c, grid, c->X.p + n0 * c->P, rows, cw_pad + n0, nullptr, nullptr, Zt_dev, ldz, Q, SM_GRAD,
                             nullptr, nullptr, Tout_dev, ldt);
}

// col[n] = w_n p_na (delta_ab - p_nb) for n < N (the padding past N stays zero): Hessian weight column of block (a, b)
__global__ void softmax_hess_coef_kernel(i64 n, int Km, int a, int b, const double* __restrict__ w, const double* __restrict__ p,
                                         double* __restrict__ col) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double pa = p[i * Km + a], pb = p[i * Km + b];
    col[i] = w[i] * pa * ((a == b ? 1.0 : 0.0) - pb);
}
int launch_softmax_hess_coef(lrvb_ctx* c, int Km, int a, int b, const double* w, const double* p, double* col) {
    const i64 n = c->N;
    hipLaunchKernelGGL(softmax_hess_coef_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, Km, a, b, w, p, col);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

// out[i][q0 + g] = sum_a (p_{n,a} - [y_n = a + 1]) T[i][g Km + a],  n = n0 + i, g < G (one launch of the influence rows)
__global__ void softmax_influence_contract_kernel(i64 total, int G, int Km, i64 n0, const double* __restrict__ p,
                                                  const int* __restrict__ labels, const double* __restrict__ T, i64 ldt,
                                                  double* __restrict__ out, i64 ldo, i64 q0) {
    const i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const i64 i = e / G; const int g = (int)(e % G);
    const i64 n = n0 + i;
    const int y = labels[n];
    double s = 0.0;
    for (int a = 0; a < Km; ++a) s += (p[n * Km + a] - (y == a + 1 ? 1.0 : 0.0)) * T[i * ldt + g * Km + a];
    out[i * ldo + q0 + g] = s;
}
int launch_softmax_influence_contract(lrvb_ctx* c, i64 n0, i64 rows, int G, int Km, const double* p, const int* labels,
                                      const double* T, i64 ldt, double* out, i64 ldo, i64 q0) {
    const i64 total = rows * G;
    if (total <= 0) return LRVB_OK;
    hipLaunchKernelGGL(softmax_influence_contract_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       total, G, Km, n0, p, labels, T, ldt, out, ldo, q0);
    HIP_TRY(hipGetLastError());
    return LRVB_OK;
}

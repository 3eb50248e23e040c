/*
 * lrvb_hip.h -- C ABI of liblrvb_hip.so, the MI355X (gfx950) implementation of the
 * LinearResponseVariationalBayes hot path: dense ELBO-Hessian assembly, Hessian-vector
 * product, per-observation gradient matrix G / Gram G^T G, and the linear-response solve
 * (Cholesky and conjugate gradient).
 *
 * The reference (pure Python on autograd) has no FFI; the boundary this library slots in
 * behind is the callable surface of `Objective` / `TwoParameterObjective` /
 * `ParametricSensitivityLinearApproximation` / `ConjugateGradientSolver`.  Every entry point
 * below cites the reference interface it replaces (paths relative to the reference checkout,
 * LRVB/ = LinearResponseVariationalBayes/).
 *
 * Conventions
 *   - Every function returns an int status: 0 = OK, negative = error; the message is then
 *     available from lrvb_last_error() (thread-local string).
 *   - All matrices are C-contiguous (row-major) IEEE fp64.
 *   - Pointers are caller-owned HOST pointers unless the parameter name ends in `_dev`
 *     (then it is a device pointer valid on the context's device).  The library owns only
 *     what lives inside the opaque context.
 *   - A context is bound to one HIP device and one HIP stream; one in-flight call per
 *     context (the reference's Objective is equally non-re-entrant:
 *     LRVB/SparseObjectives.py:131-150).
 *   - "free" = unconstrained flat vector theta (length D); "vector" = constrained flat
 *     vector eta (length V).  Layout = concatenation of blocks in push order
 *     (LRVB/ParameterDictionary.py:39-46, 55-65, 88-99).
 */
#ifndef LRVB_HIP_H
#define LRVB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared below are exported. */
#pragma GCC visibility push(default)


#define LRVB_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------------------- */
#define LRVB_OK                0
#define LRVB_ERR_INVALID      -1   /* bad argument (maps to ValueError on the Python side)  */
#define LRVB_ERR_SIZE         -2   /* wrong vector length (ValueError,
                                      LRVB/ParameterDictionary.py:56-60, 89-93)            */
#define LRVB_ERR_HIP          -3   /* HIP runtime error                                     */
#define LRVB_ERR_STATE        -4   /* call sequence error (e.g. solve before factor)        */
#define LRVB_ERR_NOT_POSDEF   -5   /* Cholesky breakdown (scipy raises LinAlgError)         */
#define LRVB_ERR_UNSUPPORTED  -6   /* layout/model combination not built                    */

/* ---- packing layout (free <-> vector maps) --------------------------------------------
 * One descriptor per parameter block, in ModelParamsDict push order.                     */
#define LRVB_BLOCK_BOX      0  /* ScalarParam/VectorParam/ArrayParam: elementwise box
                                  constraint, LRVB/Parameters.py:31-61                     */
#define LRVB_BLOCK_PSD      1  /* PosDefMatrixParam: log-Cholesky,
                                  LRVB/MatrixParameters.py:101-112                          */
#define LRVB_BLOCK_SIMPLEX  2  /* SimplexParam: row softmax with reference category 0,
                                  LRVB/SimplexParams.py:11-23                               */

typedef struct lrvb_block_desc {
    int32_t kind;        /* LRVB_BLOCK_*                                                    */
    int32_t reserved;
    int64_t free_off;    /* first index in theta                                            */
    int64_t vec_off;     /* first index in eta                                              */
    int64_t free_size;   /* box: n; psd: k(k+1)/2; simplex: rows*(K-1)                       */
    int64_t vec_size;    /* box: n; psd: k(k+1)/2; simplex: rows*K                           */
    int64_t dim0;        /* psd: k; simplex: rows; box: n                                    */
    int64_t dim1;        /* simplex: K; otherwise 0                                          */
    double  lb;          /* box lower bound (-inf allowed); psd: diag_lb                     */
    double  ub;          /* box upper bound (+inf allowed)                                   */
} lrvb_block_desc;

/* ---- model description -----------------------------------------------------------------
 * The objective the context differentiates, written in VECTOR coordinates:
 *
 *   f(eta) = sum_n w_n * loss(y_n, x_n . eta[glm_off : glm_off+n_cols])      (data term)
 *          + quad_scale * ( 1/2 (eta-m)^T A (eta-m) + b^T eta )             (quadratic term)
 *
 * and f_free(theta) = f(eta(theta)).  This replaces the opaque zero-argument closure `fun`
 * of LRVB/SparseObjectives.py:95-129 with a declared model, because a device kernel cannot
 * trace Python.                                                                          */
#define LRVB_LOSS_NONE      0
#define LRVB_LOSS_GAUSSIAN  1  /* loss = 1/2 * lik_info * (y - z)^2                         */
#define LRVB_LOSS_LOGISTIC  2  /* loss = log(1 + e^z) - y z                                  */
#define LRVB_LOSS_POISSON   3  /* loss = e^z - y z                                           */
#define LRVB_LOSS_DATA_ONLY 4  /* no GLM term: the context only holds the weighted data matrix Z
                                  (slot X, n_obs x n_cols) for objectives that are QUADRATIC IN
                                  THE DATA, f = 1/2 tr(Q(eta) Z^T diag(w) Z) + W c(eta) + R(eta)
                                  (Example.ipynb:247-274 and the conjugate-normal configs): the
                                  O(N) work is lrvb_weighted_gram / lrvb_obs_quadform, the
                                  N-independent closed forms stay with the caller.              */

#define LRVB_QUAD_NONE      0
#define LRVB_QUAD_DIAG      1  /* A = diag(a), a has length V                                */
#define LRVB_QUAD_DENSE     2  /* A is V x V symmetric                                       */

typedef struct lrvb_model_desc {
    int32_t n_blocks;
    int32_t loss;                  /* LRVB_LOSS_*                                           */
    const lrvb_block_desc* blocks; /* n_blocks entries                                       */
    int64_t n_obs;                 /* rows of X held by THIS context (its shard)             */
    int64_t n_cols;                /* columns of X                                           */
    int64_t glm_off;               /* offset of the coefficient slice inside eta             */
    double  lik_info;              /* Gaussian precision                                     */
    int32_t quad_kind;             /* LRVB_QUAD_*                                            */
    int32_t reserved;
} lrvb_model_desc;

typedef struct lrvb_ctx lrvb_ctx;

/* data slots for lrvb_set_data */
#define LRVB_SLOT_X        0   /* n_obs x n_cols design                                     */
#define LRVB_SLOT_Y        1   /* n_obs responses                                           */
#define LRVB_SLOT_QUAD_A   2   /* V (diag) or V x V (dense)                                  */
#define LRVB_SLOT_QUAD_M   3   /* V, centre of the quadratic term (default 0)               */
#define LRVB_SLOT_QUAD_B   4   /* V, linear tilt (default 0)                                 */

/* ---- library ------------------------------------------------------------------------- */
int         lrvb_version(void);
const char* lrvb_last_error(void);
int         lrvb_device_count(int* out);

/* ---- context: replaces Objective.__init__ (LRVB/SparseObjectives.py:96-116) ----------- */
int lrvb_ctx_create (lrvb_ctx** out, int device_id, const lrvb_model_desc* model);
int lrvb_ctx_destroy(lrvb_ctx* ctx);
int lrvb_ctx_sync   (lrvb_ctx* ctx);                 /* hipStreamSynchronize on the ctx stream */
/* ---- STREAM ORDERING (the contract of every entry point that takes or returns a DEVICE pointer: the `_dev`
 * functions, lrvb_set_data_dev / lrvb_set_weights_dev, lrvb_allreduce_hessian, the reduce hook) -------------------
 * All device work of a context is issued on ONE HIP stream, "the context's stream", and `_dev` entry points return
 * as soon as that work is queued.  A device operand is read, and a device result written, IN THE ORDER OF THAT
 * STREAM and in no other order.  The caller is responsible for ordering its own producers and consumers against it:
 *   (1) By default the context's stream is a private BLOCKING stream (hipStreamDefault): HIP orders it after all
 *       work already queued on the legacy default stream (handle NULL -- torch's current stream unless the caller
 *       changed it), and orders later default-stream work after it.  A caller that works on the default stream
 *       therefore needs nothing else: operands written by default-stream kernels are visible, results are complete
 *       before a later default-stream kernel or copy reads them.
 *   (2) A caller that works on ANY OTHER stream (torch side streams, hipStreamNonBlocking streams, per-thread
 *       default streams) must do one of: lrvb_ctx_set_stream(ctx, its stream, 1) -- the context then runs ON that
 *       stream; or bracket the calls with lrvb_ctx_wait_stream (before: the context's stream waits for everything
 *       queued so far on the caller's stream) and lrvb_stream_wait_ctx (after: the caller's stream waits for
 *       everything the context has queued); or synchronise on the host (its own stream before, lrvb_ctx_sync after).
 *   (3) Host-pointer entry points (no `_dev` suffix) synchronise the context's stream before they return: their
 *       outputs are complete on return, and their inputs may be reused at once.
 * Buffers adopted with lrvb_set_data_dev / lrvb_set_weights_dev are read by every later call: a caller that
 * overwrites them must order that write after the context's queued work (rule 1 or 2) like any other consumer.
 *
 * lrvb_ctx_set_stream: use_caller_stream != 0 runs the context on the caller-owned HIP stream `hip_stream` (e.g.
 * torch's current stream -- whose handle is NULL for the legacy default stream -- so that kernels, RCCL collectives
 * and the caller's own work are ordered without host synchronisation).  use_caller_stream == 0: back to a private
 * blocking stream.  The previous stream is drained first.                                                          */
int lrvb_ctx_set_stream(lrvb_ctx* ctx, void* hip_stream, int use_caller_stream);
/* Event hand-offs, no host synchronisation: the context's stream waits for the work queued so far on `hip_stream`
 * (call before handing the context operands produced there) ...                                                    */
int lrvb_ctx_wait_stream(lrvb_ctx* ctx, void* hip_stream);
/* ... and `hip_stream` waits for the work the context has queued so far (call before consuming results there).     */
int lrvb_stream_wait_ctx(lrvb_ctx* ctx, void* hip_stream);
int lrvb_ctx_sizes  (lrvb_ctx* ctx, int64_t* D, int64_t* V, int64_t* n_obs);

/* Observations / constants: uploaded once, resident in HBM afterwards.  rows/cols must
 * match the model description.  The `_dev` form adopts (does not copy, does not free) a
 * device buffer, e.g. one a torch tensor owns.                                             */
int lrvb_set_data    (lrvb_ctx* ctx, int slot, const double* host, int64_t rows, int64_t cols);
int lrvb_set_data_dev(lrvb_ctx* ctx, int slot, const double* data_dev, int64_t rows, int64_t cols);
/* Per-observation weights w (Example.ipynb:254, `self.weights`); default all ones.        */
int lrvb_set_weights    (lrvb_ctx* ctx, const double* w, int64_t n);
int lrvb_set_weights_dev(lrvb_ctx* ctx, const double* w_dev, int64_t n);
/* Multiplier of the quadratic term (the `z*y` keyword pass-through of
 * LRVB/test_objectives.py:161-217).                                                        */
int lrvb_set_quad_scale (lrvb_ctx* ctx, double scale);
/* Precision tau of the Gaussian loss 1/2 tau (y - z)^2 (the `lik_info` of the model description) as a settable
 * hyper-parameter: LRVB/ModelSensitivity.py:555-612 takes ANY hyper_par, and a likelihood precision is one of the
 * reference's own examples of it (regression_utils.py:59-132 carries `lik_info` as an argument).                    */
int lrvb_set_lik_info   (lrvb_ctx* ctx, double lik_info);

/* ---- packing: A15-A18 forward maps ---------------------------------------------------- */
/* eta = constrain(theta): ModelParamsDict.set_free + get_vector
 * (LRVB/ParameterDictionary.py:55-63, 97-99)                                               */
int lrvb_constrain  (lrvb_ctx* ctx, const double* free_in, int64_t D, double* vec_out, int64_t V);
/* theta = unconstrain(eta): set_vector + get_free (LRVB/ParameterDictionary.py:64-65, 88-96);
 * LRVB_ERR_INVALID if a value is out of bounds (LRVB/Parameters.py:15-28)                   */
int lrvb_unconstrain(lrvb_ctx* ctx, const double* vec_in, int64_t V, double* free_out, int64_t D);
/* Dense Jacobian d eta / d theta (V x D): ModelParamsDict.free_to_vector_jac(...).todense()
 * (LRVB/ParameterDictionary.py:70-78)                                                       */
int lrvb_free_to_vector_jac(lrvb_ctx* ctx, const double* free_in, int64_t D, double* jac_out);
/* H_free = J^T H_vec J + sum_k g_k d2 eta_k : convert_vector_to_free_hessian
 * (LRVB/Parameters.py:397-424)                                                              */
int lrvb_free_hessian_from_vector(lrvb_ctx* ctx, const double* free_in, const double* g_vec,
                                  const double* H_vec, double* H_free_out);

/* ---- objective in free coordinates ---------------------------------------------------- */
/* Objective.fun_free (LRVB/SparseObjectives.py:120-125)                                    */
int lrvb_value  (lrvb_ctx* ctx, const double* free_in, int64_t D, double* out);
/* Objective.fun_free_grad (LRVB/SparseObjectives.py:152-154); value_out may be NULL        */
int lrvb_grad   (lrvb_ctx* ctx, const double* free_in, int64_t D, double* value_out, double* g_out);
/* Objective.fun_free_hessian (LRVB/SparseObjectives.py:156-158, autograd.hessian at :103).
 * H_out is D x D with leading dimension ld (>= D).  Both triangles are written.            */
int lrvb_hessian(lrvb_ctx* ctx, const double* free_in, int64_t D, double* H_out, int64_t ld);
/* Objective.fun_free_hvp (LRVB/SparseObjectives.py:183-187): out = H(theta) v.  Host-callback optimisers
 * (scipy's cg and trust-ncg, as the reference drives them) call this many times at one point: the point state
 * (eta, packing Jacobian, per-observation curvature) of the last lrvb_hvp / lrvb_hvp_vec call is kept and reused
 * when the next call names the same point and no other entry point of this context ran in between (lrvb_cg_solve and
 * lrvb_cg_solve_multi keep and reuse the state the same way: the reference's ConjugateGradientSolver is built for ONE
 * point and solves for many right-hand sides there, LRVB/ConjugateGradient.py:63-105).  Data
 * installed zero-copy with lrvb_set_data_dev must be installed again after its contents change.               */
int lrvb_hvp    (lrvb_ctx* ctx, const double* free_in, const double* v, int64_t D, double* out);

/* ---- objective in vector coordinates: Objective.fun_vector* (:127-129, 164-174, 189-193) */
int lrvb_value_vec  (lrvb_ctx* ctx, const double* vec_in, int64_t V, double* out);
int lrvb_grad_vec   (lrvb_ctx* ctx, const double* vec_in, int64_t V, double* value_out, double* g_out);
int lrvb_hessian_vec(lrvb_ctx* ctx, const double* vec_in, int64_t V, double* H_out, int64_t ld);
int lrvb_hvp_vec    (lrvb_ctx* ctx, const double* vec_in, const double* v, int64_t V, double* out);

/* Vector-coordinate Hessian assembled ON THE DEVICE from small host blocks, then converted to free
 * coordinates (convert_vector_to_free_hessian, LRVB/Parameters.py:397-424) without a V x V host matrix:
 * the N-independent closed forms of the normal-family ELBOs (LRVB/NormalParams.py, WishartParams.py,
 * ExponentialFamilies.py) are sums of blocks  coef * D^T (A (x) B) D  with k x k matrices A, B and the
 * duplication matrix D of the symmetric-matrix vector form (MatrixParameters.py:16-41), plus small dense
 * blocks.  begin -> add_* ... -> finish.  `mirror` also adds the transposed block at the mirrored position
 * (off-diagonal blocks of a symmetric matrix).  finish: is_free = 1 returns J^T H J + sum_k g_k d2 eta_k
 * (H_out may be NULL: the result stays resident for lrvb_chol_factor_last), is_free = 0 returns H itself. */
int lrvb_hvec_begin(lrvb_ctx* ctx);
int lrvb_hvec_add_block(lrvb_ctx* ctx, const double* block, int64_t rows, int64_t cols, int64_t row_off,
                        int64_t col_off, int mirror);
/* H[rows[a], cols[b]] += block[a, b] (nr x nc, row-major): a dense block scattered over index lists -- the coupled
 * rows of an arrow Hessian are not contiguous.  No index may appear twice in one list.                               */
int lrvb_hvec_add_indexed(lrvb_ctx* ctx, const double* block, int64_t nr, int64_t nc, const int64_t* rows, const int64_t* cols);
int lrvb_hvec_add_symkron(lrvb_ctx* ctx, const double* A, const double* B, int64_t k, double coef,
                          int64_t row_off, int64_t col_off, int mirror);
int lrvb_hvec_finish(lrvb_ctx* ctx, const double* point, int64_t n_in, int is_free, const double* g_vec,
                     double* H_out);
/* The same assembly as ONE call (round 3: a begin / add / add / ... / finish sequence cost a binding call, an upload and a
 * launch per block -- more than the kernels of the small configurations).  `ops` holds n_ops records of 8 int64:
 *   [kind, off, a, b, c, d, e, f]   with `off` the position of the record's operands in `data` (n_data doubles, uploaded once),
 *   kind 0  add_block:    block at off (a x b, row-major), row_off c, col_off d, mirror e;
 *   kind 1  add_indexed:  block at off (a x b), then a row indices and b column indices stored as doubles;
 *   kind 2  add_symkron:  A at off, B at f (both a x a; two records may share an operand), row_off c, col_off d, mirror e,
 *                         the coefficient at data[b].
 * Then exactly lrvb_hvec_finish(point, n_in, is_free, g_vec, H_out).                                                       */
int lrvb_hvec_program(lrvb_ctx* ctx, const int64_t* ops, int64_t n_ops, const double* data, int64_t n_data,
                      const double* point, int64_t n_in, int is_free, const double* g_vec, double* H_out);

/* ---- cross Hessians: TwoParameterObjective.fun_hessian_free1_vector2
 * (LRVB/SparseObjectives.py:429-438) for the two hyper-parameters a declared model has ---- */
/* Rows n0..n1 of G (shape (n1-n0) x D): G[n,:] = d/dtheta of d f/d w_n, i.e. the transpose
 * of the D x N cross Hessian w.r.t. the observation weights (Example.ipynb:425-441).        */
int lrvb_obs_grad(lrvb_ctx* ctx, const double* free_in, int64_t D, int64_t n0, int64_t n1,
                  double* G_out);
/* l(y_n, z_n) for rows n0..n1: the gradient of the objective with respect to the observation weights,
 * TwoParameterObjective.fun_grad2 (LRVB/SparseObjectives.py:381-387) with par2 = the weights in vector
 * coordinates; `point` is the free vector (is_free != 0) or the vector-coordinate point.             */
int lrvb_obs_loss(lrvb_ctx* ctx, const double* point, int64_t n_in, int is_free, int64_t n0, int64_t n1,
                  double* out);
/* Same in vector coordinates ((n1-n0) x V): TwoParameterObjective.fun_vector_hessian21
 * (LRVB/SparseObjectives.py:418-427) with par2 = the weights.                               */
int lrvb_obs_grad_vec(lrvb_ctx* ctx, const double* vec_in, int64_t V, int64_t n0, int64_t n1,
                      double* G_out);
/* Weight sensitivity of moments by linear response, streamed over the observations:
 *   out[n - n0, q] = d m_q / d w_n = -(M H^-1 G^T)[q, n]       ((n1 - n0) x Q, row-major)
 * -- `moment_jac @ ParametricSensitivityLinearApproximation.get_dinput_dhyper()` with
 * hyper_par = the observation weights (LRVB/ModelSensitivity.py:596-606, Example.ipynb:425-441),
 * transposed, without forming the D x N cross Hessian or the D x N sensitivity.  M is Q x D
 * (free) / Q x V (vector) row-major; H is the factor left by lrvb_chol_factor (same coordinates).
 * With M = I (Q = D) the result is the whole sensitivity matrix, transposed.                   */
int lrvb_obs_influence(lrvb_ctx* ctx, const double* free_in, int64_t D, const double* M, int64_t Q,
                       int64_t n0, int64_t n1, double* out);
int lrvb_obs_influence_vec(lrvb_ctx* ctx, const double* vec_in, int64_t V, const double* M, int64_t Q,
                           int64_t n0, int64_t n1, double* out);
/* The row product inside lrvb_obs_influence and lrvb_obs_loss on its own:
 *   out[n - n0, q] = rowscale[n] * x_n . Zt[q]                  ((n1 - n0) x Q, row-major)
 * for the rows n0 <= n < n1 of the observation matrix; Zt is Q x n_cols row-major, rowscale has n_obs entries
 * (NULL = ones).  Where the fused multi-vector pass applies (even n_cols <= 1024, 16-byte aligned rows) the rows stream
 * through it 16 columns of the result at a time; otherwise, or with tuning bit 0 set, a GEMM and a row scaling.
 * Row range and data checks as lrvb_obs_loss.                                                */
int lrvb_rows_times_matrix(lrvb_ctx* ctx, const double* Zt, int64_t Q, const double* rowscale /*nullable*/,
                           int64_t n0, int64_t n1, double* out);
/* D x V cross Hessian w.r.t. the linear tilt b of the quadratic term
 * (the `hyper_param @ theta` term of LRVB/test_model_sensitivity.py:56-66).                 */
int lrvb_cross_hessian_tilt(lrvb_ctx* ctx, const double* free_in, int64_t D, double* C_out);
/* ---- cross Hessians and gradients with respect to the OTHER hyper-parameters of the declared objective:
 * TwoParameterObjective.fun_hessian_free1_vector2 / fun_vector_hessian12 / fun_grad2 (LRVB/SparseObjectives.py:381-449)
 * and the `hyper_par` of ParametricSensitivityLinearApproximation (LRVB/ModelSensitivity.py:555-612, whose defining use
 * is PRIOR sensitivity) for eps in
 *   LRVB_HYPER_TILT        b                 (Ph = V)
 *   LRVB_HYPER_QUAD_M      m, the centre / prior mean of the quadratic term (Ph = V)
 *   LRVB_HYPER_QUAD_A      A: its diagonal (LRVB_QUAD_DIAG, Ph = V) or the row-major lower triangle of the symmetric
 *                          matrix (LRVB_QUAD_DENSE, Ph = V (V + 1) / 2, the vector form of LRVB/MatrixParameters.py:16-41)
 *   LRVB_HYPER_QUAD_SCALE  s                 (Ph = 1)
 *   LRVB_HYPER_LIK_INFO    tau of the Gaussian loss (Ph = 1; one pass over the observations, summed over the ranks)
 * all in VECTOR coordinates of the hyper-parameter (a free hyper-parameter chains through its own packing Jacobian on
 * the caller's side: the objective is differentiated once in eps).  `point` is the free vector (is_free != 0) or the
 * vector-coordinate point of the input parameter; C_out is n x Ph row-major (n = D or V), g_out has Ph entries.
 * Closed forms in r = eta - m, A r, b and the data gradient, evaluated on the device with the packing Jacobian of the
 * input applied there.                                                                                              */
#define LRVB_HYPER_TILT        0
#define LRVB_HYPER_QUAD_M      1
#define LRVB_HYPER_QUAD_A      2
#define LRVB_HYPER_QUAD_SCALE  3
#define LRVB_HYPER_LIK_INFO    4
int lrvb_hyper_size(lrvb_ctx* ctx, int kind, int64_t* n_hyper);
int lrvb_cross_hessian_hyper(lrvb_ctx* ctx, int kind, const double* point, int64_t n_in, int is_free,
                             double* C_out, int64_t n_hyper);
int lrvb_hyper_grad(lrvb_ctx* ctx, int kind, const double* point, int64_t n_in, int is_free,
                    double* g_out, int64_t n_hyper);
/* out (D x Q, row-major) = J(theta)^T B for a host matrix B (V x Q): the chain rule d/d theta = J^T d/d eta for cross
 * Hessians whose vector-coordinate form is an N-independent closed form of the caller's (the priors of the model
 * families: LRVB/ExponentialFamilies.py:186-204 `mvn_prior`, `gamma_prior`, `dirichlet_prior`).                       */
int lrvb_jac_t_matmul(lrvb_ctx* ctx, const double* free_in, int64_t D, const double* B, int64_t Q, double* out);
/* Gram matrix G^T G (D x D) of the per-observation gradient matrix; G is generated on chip
 * and never materialised.                                                                   */
int lrvb_gram(lrvb_ctx* ctx, const double* free_in, int64_t D, double* GtG_out, int64_t ld);

/* ---- the non-conjugate logistic term (LRVB/Modeling.py) -----------------------------------
 * Per element i: phi_i = sum_k gh_w[k] log(1 + exp(z_mean[i] + sqrt(2) z_sd[i] gh_x[k])) / sqrt(pi), the Gauss-Hermite
 * value of E log(1 + e^z), z ~ N(z_mean, z_sd^2): get_e_logistic_term_guass_hermite(..., aggregate_all=False),
 * LRVB/Modeling.py:36-52 (log(1 + e^t) in the overflow-free form; the reference's log1p(exp(t)) is inf past t = 709).
 * order >= 1: d1 (n x 2) = [d/dz_mean, d/dz_sd]; order >= 2: d2 (n x 3) = [mean mean, mean sd, sd sd] -- derivatives of
 * the quadrature SUM, i.e. what autograd returns for the reference's expression.  1 <= n_nodes <= 128.
 * get_e_logistic_term (:16-32) is the same sum with nodes draws / sqrt(2) and weights sqrt(pi) / n_draws.             */
int lrvb_gh_logistic(lrvb_ctx* ctx, int64_t n, const double* z_mean, const double* z_sd, const double* gh_x,
                     const double* gh_w, int32_t n_nodes, int32_t order, double* val, double* d1, double* d2);
/* The model that expectation is written for: logistic regression with q(beta_j) = N(mean_j, var_j).  Data term
 *   sum_n w_n ( phi(x_n . mean, sqrt(x_n^2 . var)) - y_n x_n . mean )
 * of the context's X (n_obs x n_cols = P), y and weights, in the coordinates (mean, var): value, gradient (2 P, nullable)
 * and the three P x P blocks [d2/dmean2 | d2/dmean dvar | d2/dvar2] of the Hessian (3 P^2, row-major, nullable):
 * X^T D11 X, X^T D12 (X o X), (X o X)^T D22 (X o X) on the fp64 matrix cores with the per-observation second
 * derivatives of the quadrature sum as weights.  The context must hold X and y (any GLM loss).                       */
int lrvb_logitnormal_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* gh_x,
                           const double* gh_w, int32_t n_nodes, double* value_out, double* grad_out, double* H_blocks_out);
/* The same model with a full-covariance posterior q(beta) = N(mean, cov), P = n_cols <= 64 (LRVB_ERR_UNSUPPORTED above:
 * the Sigma-Sigma block is the packed-triangle Kronecker SYRK, whose stage holds 64 columns).  Data term
 *   sum_n w_n ( psi(x_n . mean, x_n^T cov x_n) - y_n x_n . mean ),   psi(mu, s) = E log(1 + e^z), z ~ N(mu, s)  (Gauss-Hermite)
 * in the D = P + P (P + 1) / 2 coordinates (mean, vech cov), vech = row-major lower triangle, an off-diagonal coordinate
 * standing for both entries: value, gradient (D, nullable) and Hessian (D x D, row-major, nullable).  Derivatives in the
 * variance s are Stein's identity on the same nodes (d_s E g = E g'' / 2, ...), so a zero design row is regular.       */
int lrvb_logitnormal_mvn_terms(lrvb_ctx* ctx, const double* mean, const double* cov, int64_t P, const double* gh_x,
                               const double* gh_w, int32_t n_nodes, double* value_out, double* grad_out, double* H_out);
/* Matrix-free product of that data-term Hessian with v (D, coordinates (mean, vech cov)) -> out (D): two row passes, one
 * gemv and one weighted SYRK of X; no D x D matrix is formed.                                                          */
int lrvb_logitnormal_mvn_hvp(lrvb_ctx* ctx, const double* mean, const double* cov, int64_t P, const double* gh_x,
                             const double* gh_w, int32_t n_nodes, const double* v, double* out);
/* Chain of a Hessian H_in (D x D) in (mean, vech Sigma) to (mean, vech Lambda), Lambda = Sigma^-1, on the device:
 *   H_out = J^T H_in J + [0, 0; 0, 2 symkron(M, Sigma) - 1/2 symkron(Sigma, Sigma)],  J = d vech Sigma / d vech Lambda,
 * where M = Sigma G Sigma for the symmetric matrix gradient G of the objective in Sigma (the second-order term of
 * Lambda -> Lambda^-1) and the last term is the Hessian of +1/2 log det Lambda (minus the entropy).  No observations are involved.          */
int lrvb_logitnormal_mvn_chain(lrvb_ctx* ctx, int64_t P, const double* cov, const double* M, const double* H_in, double* H_out);

/* ---- logistic mixed model with a random intercept ------------------------------------------------
 * y_n ~ Bernoulli(sigma(x_n . beta + u_g(n))), q(beta_j) = N(mean_j, var_j), q(u_g) = N(e_g, r_g).  The context holds X
 * (n_obs x P, P <= 64), y, the weights and the groups (lrvb_set_groups, G groups).  Data term
 *   f = sum_n w_n ( psi(rho_n, s_n) - y_n rho_n ),  rho_n = x_n . mean + e_g(n),  s_n = (x_n o x_n) . var + r_g(n),
 * psi(rho, s) = E log(1 + e^z), z ~ N(rho, s), by Gauss-Hermite; derivatives in s by Stein's identity on the same nodes
 * (d_s = 1/2 E g2, d_rho d_s = 1/2 E g3, d_s^2 = 1/4 E g4, gk the k-th derivative of log(1 + e^t)), as
 * lrvb_logitnormal_mvn_terms.  Per observation a1 = w (psi_rho - y), a2 = w psi_s, c11 = w psi_rhorho, c12 = w psi_rhos,
 * c22 = w psi_ss.  Coordinates (mean, var, e, r).
 * One pass over the group-sorted rows forms the coefficients and, per group, the fixed-order sums (no atomics: two calls at
 * one point return bitwise equal results)
 *   [sum a1, sum a2 | sum c11, sum c12, sum c22 | sum c11 x | sum c12 x | sum c12 x o x | sum c22 x o x]   (5 + 4 P numbers);
 * the global gradient [X^T a1 | (X o X)^T a2] and the blocks X^T D11 X, X^T D12 (X o X), (X o X)^T D22 (X o X) follow on the
 * kernels of lrvb_logitnormal_terms.  Outputs (host; all but value_out nullable): value, grad_global (2 P), grad_local
 * (G x 2: sum a1, sum a2), H_blocks (3 P^2), border (G x 4 P: the four P-vectors above) and local (G x 3: sum c11, c12, c22).
 * Reduce hook: every sum over observations of the call lies in ONE device buffer
 *   [H blocks (3 P^2, only when asked for) | group sums (G x (5 + 4 P)) | gradient (2 P) | value (1)]
 * and goes through the hook exactly once (groups may straddle ranks: their sums add).  The group sums stay resident in the
 * context for lrvb_glmm_schur until the next lrvb_glmm_terms or lrvb_set_groups.
 * ONE resident buffer serves this entry and the K-effect terms entries below (lrvb_glmm_slopes_terms, lrvb_glmm_poisson_terms,
 * lrvb_glmm_binomial_terms): on one context a call of this entry drops the resident K-effect sums and the factor of
 * lrvb_glmm_slopes_schur, and a K-effect terms call drops the sums of this entry.  Either family's elimination refuses the
 * other's sums (LRVB_ERR_STATE): use one context per model.
 * P > 64 or more than 128 nodes: LRVB_ERR_UNSUPPORTED; groups, X or y not set: LRVB_ERR_STATE; var_j <= 0 or r_g <= 0:
 * LRVB_ERR_INVALID.                                                                                                     */
int lrvb_glmm_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r, int64_t G,
                    const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out, double* grad_global_out,
                    double* grad_local_out, double* H_blocks_out, double* border_out, double* local_out);
/* Elimination of the 2 G local parameters on the device, from the group sums of the last lrvb_glmm_terms (the border is not
 * copied to the host).  Per group the host sends the COMPLETE 2 x 2 local block in the coordinates it eliminates in
 * (local_2x2, G x 3: [a11, a12, a22] -- data part, N-independent terms and chain terms added by the host), the two chain
 * factors of those coordinates (border_scale, G x 2: d e / d coordinate, d r / d coordinate) and the closed-form border
 * rows of the three scalar parameters (closed_rows, G x 6: rows [e_mu, a, b] against e_g, then against r_g).  With
 *   C_g = [ f_e [sum c11 x | sum c12 x o x | closed_e] ; f_r [sum c12 x | sum c22 x o x | closed_r] ]      (2 x (2 P + 3))
 * M_out ((2 P + 3)^2, row-major) = sum_g C_g^T A_g^-1 C_g over the coupled coordinates [mean (P) | var (P) | e_mu, a, b]:
 * rows scaled by the 2 x 2 Cholesky factors, then one Gram over 2 G rows.  A block that is not positive definite:
 * LRVB_ERR_NOT_POSDEF; no resident group sums: LRVB_ERR_STATE.                                                           */
int lrvb_glmm_schur(lrvb_ctx* ctx, const double* local_2x2, const double* border_scale, const double* closed_rows, int64_t G,
                    double* M_out);

/* Logistic mixed model with K <= 4 independent random effects per group (random slopes):
 *   y_n ~ Bernoulli(sigma(x_n . beta + z_n . u_g(n))),  q(beta_j) = N(mean_j, var_j),  q(u_gk) = N(e_gk, r_gk).
 * The group design z (n x K, row-major: a column of ones for an intercept, columns of X for slopes) lives in its own device
 * buffer.  It is replaced by the next call and dropped by a later lrvb_set_groups whose row count differs from n.
 * z == NULL: LRVB_ERR_INVALID; K < 1 or K > 4: LRVB_ERR_UNSUPPORTED; n < 1: LRVB_ERR_SIZE.                                */
int lrvb_set_group_design(lrvb_ctx* ctx, const double* z, int64_t n, int64_t K);
/* Data term of that model at (mean, var (P each), e, r (G x K each, row-major: group-major)):
 *   rho_n = x_n . mean + z_n . e_g(n),  s_n = (x_n o x_n) . var + (z_n o z_n) . r_g(n),  sum_n w_n [psi(rho_n, s_n) - y_n rho_n]
 * with psi and the per-row coefficients a1, a2, c11, c12, c22 of lrvb_glmm_terms (same nodes, same derivative rule).
 *   value_out (1), grad_global_out (2 P: d/d mean, d/d var; may be NULL), H_blocks_out (3 P^2: mean-mean, mean-var, var-var;
 *   may be NULL) as lrvb_glmm_terms.
 *   group_sums_out (may be NULL): per group the ncol = nsc + 4 K P sums, nsc = 2 K + K (2 K + 1),
 *     [ sum a1 z (K) | sum a2 z o z (K) |
 *       upper triangle, row-major, of the 2 K x 2 K local block  sum c q q^T,  q = [z | z o z],  c = c11 on the z-z quarter,
 *       c12 on the z-(z o z) quarter, c22 on the (z o z)-(z o z) quarter  (K (2 K + 1)) |
 *       border, four blocks of K x P, entry (b K + k) P + j:
 *         b = 0: sum c11 z_k x_j,  b = 1: sum c12 z_k^2 x_j,  b = 2: sum c12 z_k x_j^2,  b = 3: sum c22 z_k^2 x_j^2 ]
 *   want_border != 0: G x ncol doubles; want_border == 0: G x nsc doubles (the scalar columns; the border is not copied to
 *   the host).  At K = 1 with z = 1 these are the columns of lrvb_glmm_terms in its order.
 * Fixed summation order, no atomics: two calls at one point are bitwise equal.
 * Reduce hook: every sum over observations of the call lies in ONE device buffer
 *   [H blocks (3 P^2, only when asked for) | group sums (G x ncol) | gradient (2 P) | value (1)]
 * and goes through the hook exactly once.  The group sums stay resident for lrvb_glmm_slopes_schur until the next
 * lrvb_glmm_slopes_terms, lrvb_set_group_design or lrvb_set_groups -- or the next lrvb_glmm_terms, which shares the buffer (see there).
 * P > 64, K < 1, K > 4 or more than 128 nodes: LRVB_ERR_UNSUPPORTED; groups, the group design, X or y not set, or a group
 * design that is not n_obs x K: LRVB_ERR_STATE; var_j <= 0 or r_gk <= 0: LRVB_ERR_INVALID; G is not the number of groups:
 * LRVB_ERR_SIZE.                                                                                                          */
int lrvb_glmm_slopes_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r, int64_t G,
                           int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out,
                           double* grad_global_out, double* H_blocks_out, double* group_sums_out, int32_t want_border);
/* Elimination of the 2 K G local parameters on the device from the group sums of the last lrvb_glmm_slopes_terms.  Per group
 * the host sends the COMPLETE local block in the coordinates it eliminates in, ordered [e_g0 .. e_g,K-1 | r_g0 .. r_g,K-1]
 * (local_blocks, G x K (2 K + 1): upper triangle, row-major), the 2 K chain factors of those coordinates (border_scale,
 * G x 2 K) and the closed-form border entries of every local coordinate against [e_mu_k, a_k, b_k] of its own component k
 * (closed_rows, G x 2 K x 3; the entries against the other components are zero).
 * M_out (R x R, R = 2 P + 3 K, row-major) = sum_g C_g^T A_g^-1 C_g over the coupled coordinates
 * [mean (P) | var (P) | e_mu_0, a_0, b_0, .., e_mu_{K-1}, a_{K-1}, b_{K-1}]: each block is factored A_g = L L^T, the rows
 * U_g = L^-1 C_g are written, then one Gram over 2 K G rows.  A block that is not positive definite: LRVB_ERR_NOT_POSDEF;
 * no resident group sums of K effects: LRVB_ERR_STATE; K < 1 or K > 4: LRVB_ERR_UNSUPPORTED.  No reduce-hook call.
 * On success the uploaded blocks and U stay resident for lrvb_glmm_slopes_solve_forward / _back (below).                   */
int lrvb_glmm_slopes_schur(lrvb_ctx* ctx, const double* local_blocks, const double* border_scale, const double* closed_rows,
                           int64_t G, int64_t K, double* M_out);
/* The block-arrow solve H^-1 [R_g ; R_l] with the local half on the device.  A successful lrvb_glmm_slopes_schur leaves its
 * factor resident in a buffer of its own: the local blocks as uploaded (L_g is re-derived from them on chip, by the same
 * operations in the same order, wherever it is needed) and U_g = L_g^-1 C_g.  The factor is dropped by the next
 * lrvb_glmm_slopes_terms, lrvb_set_group_design or lrvb_set_groups, and replaced by the next lrvb_glmm_slopes_schur.  With
 * S = H_gg - M on the host (M scaled to the caller's coordinates; s below is that scaling of the coupled rows):
 *   forward:  T_g = L_g^-1 R_local,g  (kept resident),   red_out (R x Q, row-major) = sum_g U_g^T T_g;
 *   host:     rhs = R_g,  rhs[coupled rows] -= s o red,  x = S^-1 rhs;
 *   back:     X_local_out,g = L_g^-T (T_g - U_g x_coupled),   x_coupled (R x Q, row-major) = s o x[coupled rows].
 * R_local and X_local_out are G x 2 K x Q, row-major: group g holds 2 K vectors of Q contiguous values in the order
 * [e_g0 .. e_g,K-1 | r_g0 .. r_g,K-1] -- the layout of A_local of lrvb_glmm_slopes_obs_influence; the coupled rows are in the
 * order of M_out.  One workgroup per group runs the triangular substitution, one thread per column q (any Q >= 1); the
 * contractions U^T T (over 2 K G rows) and U x (over R) are GEMMs on the fp64 matrix cores.  Fixed summation order, no
 * atomics: two calls with the same inputs are bitwise equal.  No reduce-hook call: after lrvb_glmm_slopes_terms every rank
 * holds the complete group sums, so the solve is replicated, as the elimination is.
 * Memory: the factor holds 2 K G x ld(R) doubles of U, ld(R) = R rounded up to a multiple of 8 (G = 1e4, K = 4, P = 64:
 * 8e4 x 144 doubles = 92 MB), and K (2 K + 1) G doubles of blocks; a forward pass adds 2 K G x Q doubles of T, a back pass
 * as many of scratch.
 * No resident factor of K effects, or lrvb_glmm_slopes_solve_back without a forward pass since the factor was built:
 * LRVB_ERR_STATE; back with another Q than the forward pass before it, or G not the number of groups: LRVB_ERR_SIZE; K < 1 or
 * K > 4: LRVB_ERR_UNSUPPORTED; Q < 1 or a null pointer: LRVB_ERR_INVALID.                                                    */
int lrvb_glmm_slopes_solve_forward(lrvb_ctx* ctx, const double* R_local, int64_t G, int64_t K, int64_t Q, double* red_out);
int lrvb_glmm_slopes_solve_back(lrvb_ctx* ctx, const double* x_coupled, int64_t G, int64_t K, int64_t Q, double* X_local_out);
/* The elimination and the solve for a DENSE closed border: a K-effect model whose local coordinates couple to NC closed global
 * coordinates of any meaning (correlated random effects with a Wishart precision: [e_mu (K) | n | vech V], NC = K + 1 + K (K + 1) / 2).
 * After any K-effect terms entry (lrvb_glmm_slopes_terms, lrvb_glmm_poisson_terms, lrvb_glmm_binomial_terms):
 *   local_blocks (G x K (2 K + 1)) and border_scale (G x 2 K) as lrvb_glmm_slopes_schur;
 *   the closed border entries of group g are AFFINE in its K-vector d_g (d_loc, G x K, row-major):
 *     closed_g[i][c] = A0[i][c] + sum_l A1[i][l][c] d_gl,   i over the 2 K local coordinates [e_g. | r_g.], c over the NC columns,
 *   A0 (2 K x NC) and A1 (2 K x K x NC) row-major, shared by all groups, in the coordinates of the caller's choice on the closed
 *   side (the chain factor border_scale[g][i] multiplies row i as it does the group sums).
 * M_out (R x R, R = 2 P + NC <= 144, row-major) = sum_g C_g^T A_g^-1 C_g over [mean (P) | var (P) | the NC closed columns in the
 * caller's order].  The factor stays resident as after lrvb_glmm_slopes_schur, with NC recorded: lrvb_glmm_arrow_solve_forward / _back
 * are lrvb_glmm_slopes_solve_forward / _back on R = 2 P + NC coupled rows.  A factor answers only the entries of its own coupled
 * layout: an arrow entry asked for another NC than the factor's, or a legacy entry (lrvb_glmm_slopes_solve_forward / _back,
 * lrvb_glmm_slopes_group_cov) on a factor whose NC is not 3 K, is LRVB_ERR_STATE, and so is the reverse.  Whatever drops the
 * factor of lrvb_glmm_slopes_schur drops this one.  Fixed order, no atomics: two calls give equal bits.
 * K < 1, K > 4, NC < K or NC > 16: LRVB_ERR_UNSUPPORTED; a null pointer or Q < 1: LRVB_ERR_INVALID; G not the number of groups:
 * LRVB_ERR_SIZE; no resident group sums of K effects: LRVB_ERR_STATE; a block that is not positive definite:
 * LRVB_ERR_NOT_POSDEF (no factor is left).  No reduce-hook call.                                                            */
int lrvb_glmm_arrow_schur(lrvb_ctx* ctx, const double* local_blocks, const double* border_scale, const double* d_loc, const double* A0,
                          const double* A1, int64_t G, int64_t K, int64_t NC, double* M_out);
int lrvb_glmm_arrow_solve_forward(lrvb_ctx* ctx, const double* R_local, int64_t G, int64_t K, int64_t NC, int64_t Q, double* red_out);
int lrvb_glmm_arrow_solve_back(lrvb_ctx* ctx, const double* x_coupled, int64_t G, int64_t K, int64_t NC, int64_t Q, double* X_local_out);

/* Streamed weight influence of the logistic mixed model.  Point arguments as lrvb_glmm_terms.  Per observation, PER UNIT WEIGHT,
 *   a1' = psi_rho(rho_n, s_n) - y_n,   a2' = psi_s(rho_n, s_n)
 * and the gradient of row n's term in (mean, var, e, r) is [a1' x_n | a2' x_n o x_n | at g(n): a1', a2'].  For an operand A
 * (Q x (2 P + 2 G), columns [A_m | A_v | A_e | A_r]) given as
 *   A_global (Q x 2 P, row-major: row q = [A_m[q] | A_v[q]])   and
 *   A_local  (G x 2 Q, row-major: row g = [A_e[0..Q-1, g] | A_r[0..Q-1, g]] -- one contiguous read per observation)
 * the entry writes, for n0 <= n < n1,
 *   out[n - n0][q] = a1' (x_n . A_m[q] + A_e[q, g(n)]) + a2' ((x_n o x_n) . A_v[q] + A_r[q, g(n)])        ((n1 - n0) x Q, host)
 * i.e. A times column n of the weight cross Hessian, which is never formed.  The weights do not enter: a row of weight zero
 * gets the influence of adding it.  ONE pass over the rows of the window in their original order for any Q >= 1: a tile of 64
 * rows is staged on chip, the quadrature (two of the five derivative sums of lrvb_glmm_terms) is done once per row, and the
 * two contractions run on the fp64 matrix cores in blocks of 16 outputs inside the tile (x o x is formed on chip).  A window
 * equals the same rows of the full result bitwise.  Per-observation rows: rank-local, NO reduce-hook call.
 * Memory: nothing is chunked inside the call.  The device holds the (n1 - n0) x Q result and the G x 2 Q operand in one piece
 * each, so "any Q" is bounded by (n1 - n0) Q + 2 G Q doubles of free device memory (N = 1e6, G = 1e4, Q = 16: 128 MB + 2.6 MB;
 * Q = D = 20132 needs 3.2 GB for A_local alone and 161 GB for all rows at once): a caller with a wide operand walks row
 * windows, and one whose A_local does not fit walks blocks of outputs.  A device allocation that fails is LRVB_ERR_HIP.
 * Errors as lrvb_glmm_terms (P > 64 or more than 128 nodes: LRVB_ERR_UNSUPPORTED; groups, X or y not set: LRVB_ERR_STATE;
 * var_j <= 0 or r_g <= 0: LRVB_ERR_INVALID); n0 > n1 or n1 > n_obs: LRVB_ERR_INVALID, as lrvb_obs_influence.                */
int lrvb_glmm_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                            int64_t G, const double* gh_x, const double* gh_w, int32_t n_nodes, const double* A_global,
                            const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence: out[g][q] = sum over the rows n of group g of w_n * (the row of lrvb_glmm_obs_influence)   (G x Q, host) --
 * the derivative with respect to a common multiplier on the weights of group g's rows (leave one cluster out).  The group's
 * own prior term on u_g is NOT part of it.  One pass over the group-sorted rows forms, per group and in a fixed order (no
 * atomics: two calls at one point are bitwise equal), [sum w a1', sum w a2' | sum w a1' x | sum w a2' x o x] (2 + 2 P numbers);
 * the contraction with A is a (G x 2 P)(2 P x Q) product and does not touch the observations again.  An empty group gives a
 * zero row.  Reduce hook: the G x Q result is a sum over observations (a group may straddle ranks) and goes through the hook
 * exactly once, as one buffer of G Q doubles.  Errors as lrvb_glmm_obs_influence.                                          */
int lrvb_glmm_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                              int64_t G, const double* gh_x, const double* gh_w, int32_t n_nodes, const double* A_global,
                              const double* A_local, int64_t Q, double* out);

/* Streamed weight influence of the logistic mixed model with K <= 4 effects per group.  Point arguments as
 * lrvb_glmm_slopes_terms (e, r: G x K, group-major).  Per observation, PER UNIT WEIGHT, with a1', a2' as above at
 *   rho_n = x_n . mean + z_n . e_g(n),   s_n = (x_n o x_n) . var + (z_n o z_n) . r_g(n),
 * the gradient of row n's term in (mean, var, e, r) is [a1' x_n | a2' x_n o x_n | at g(n): a1' z_n (K), a2' z_n o z_n (K)].
 * For an operand A (Q x (2 P + 2 G K), columns [A_m | A_v | A_e (G K, group-major) | A_r (G K)]) given as
 *   A_global (Q x 2 P, row-major: row q = [A_m[q] | A_v[q]])   and
 *   A_local  (G x 2 K x Q, row-major: group g holds 2 K vectors of Q contiguous outputs in the order
 *             [A_e[., g, 0] .. A_e[., g, K-1] | A_r[., g, 0] .. A_r[., g, K-1]]; at K = 1 the G x 2 Q layout above)
 * the entry writes, for n0 <= n < n1,
 *   out[n - n0][q] = a1' (x_n . A_m[q] + sum_k z_nk A_e[q, g(n), k]) + a2' ((x_n o x_n) . A_v[q] + sum_k z_nk^2 A_r[q, g(n), k])
 * ((n1 - n0) x Q, host).  At K = 1 with z = 1 this is the row of lrvb_glmm_obs_influence.  The weights do not enter.  ONE pass
 * over the rows of the window in their original order for any Q >= 1, the quadrature once per row, the two global contractions
 * on the fp64 matrix cores in blocks of 16 outputs; the 2 K local values of a row are gathered (16 consecutive doubles per
 * coordinate and block) and added behind the matrix product, because the rows of one tile belong to different groups.  A window
 * equals the same rows of the full result bitwise.  Per-observation rows: rank-local, NO reduce-hook call.
 * Memory: nothing is chunked inside the call; Q is bounded by (n1 - n0) Q + 2 G K Q doubles of free device memory (N = 1e6,
 * G = 1e4, K = 4, Q = 16: 128 MB + 10 MB): a caller with a wide operand walks row windows or blocks of outputs.
 * Errors as lrvb_glmm_slopes_terms (P > 64, K < 1, K > 4 or more than 128 nodes: LRVB_ERR_UNSUPPORTED; groups, the group design,
 * X or y not set, or a group design that is not n_obs x K: LRVB_ERR_STATE; var_j <= 0 or r_gk <= 0: LRVB_ERR_INVALID; G is not
 * the number of groups: LRVB_ERR_SIZE); n0 > n1 or n1 > n_obs: LRVB_ERR_INVALID, as lrvb_glmm_obs_influence.                 */
int lrvb_glmm_slopes_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                   int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                   const double* A_global, const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence of that model: out[g][q] = sum over the rows n of group g of w_n * (the row of lrvb_glmm_slopes_obs_influence)
 * (G x Q, host): leave one cluster out; the group's own prior terms on u_g. are NOT part of it.  One pass over the group-sorted
 * rows forms, per group and in a fixed order (no atomics: two calls at one point are bitwise equal),
 *   [sum w a1' z (K) | sum w a2' z o z (K) | sum w a1' x (P) | sum w a2' x o x (P)]        (2 K + 2 P numbers);
 * the contraction with A is a (G x 2 P)(2 P x Q) product plus the 2 K local columns and does not touch the observations again.
 * An empty group gives an exact zero row.  Reduce hook: the G x Q result is a sum over observations (a group may straddle
 * ranks) and goes through the hook exactly once, as one buffer of G Q doubles.  Errors as lrvb_glmm_slopes_obs_influence.     */
int lrvb_glmm_slopes_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                     const double* r, int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                     const double* A_global, const double* A_local, int64_t Q, double* out);

/* ---- Poisson mixed model with K <= 4 independent random effects per group ---------------------------
 *   y_n ~ Poisson(exp(o_n + x_n . beta + z_n . u_g(n))),  q(beta_j) = N(mean_j, var_j),  q(u_gk) = N(e_gk, r_gk).
 * The per-row offset o (log exposure; n doubles) lives in one device buffer of its own.  offset == NULL clears it (the offset is
 * then zero); it is replaced by the next call.  The lrvb_glmm_poisson_*, lrvb_glmm_binomial_* and lrvb_glmm_ztpoisson_* entries read
 * it; no other entry looks at it (the logistic lrvb_glmm_slopes_* entries in particular do not).  The call drops the resident
 * group sums and factor (they were formed under another offset).  A length other than n_obs is found when a Poisson or binomial
 * entry runs: LRVB_ERR_STATE there.  n < 1 with a non-null offset: LRVB_ERR_SIZE.                                             */
int lrvb_set_offset(lrvb_ctx* ctx, const double* offset, int64_t n);
/* Data term of that model at (mean, var (P each), e, r (G x K each, group-major)), the group design of lrvb_set_group_design:
 *   rho_n = o_n + x_n . mean + z_n . e_g(n),  s_n = (x_n o x_n) . var + (z_n o z_n) . r_g(n),  psi_n = exp(rho_n + s_n / 2)
 *   value = sum_n w_n [psi_n - y_n rho_n]          (E exp(t), t ~ N(rho, s), is exact: no quadrature; log y! is dropped)
 * and, with h = w psi, the per-row coefficients a1 = h - w y, a2 = h / 2, c11 = h, c12 = h / 2, c22 = h / 4.  Outputs, the
 * column layout of group_sums_out, want_border, the fixed summation order (two calls at one point are bitwise equal) and the
 * reduce-hook contract (ONE buffer [H blocks, when asked for | group sums | gradient | value], one hook call) are those of
 * lrvb_glmm_slopes_terms.  The group sums stay resident exactly as that entry leaves them: lrvb_glmm_slopes_schur,
 * lrvb_glmm_slopes_solve_forward and lrvb_glmm_slopes_solve_back work on them unchanged.
 * Errors as lrvb_glmm_slopes_terms without the node count (P > 64, K < 1 or K > 4: LRVB_ERR_UNSUPPORTED; groups, the group
 * design, X or y not set, a group design that is not n_obs x K, or an offset whose length is not n_obs: LRVB_ERR_STATE;
 * var_j <= 0 or r_gk <= 0: LRVB_ERR_INVALID; G is not the number of groups: LRVB_ERR_SIZE).  The kernel does not clamp: where
 * exp(rho + s / 2) overflows, the value after the reduction is not finite and the call returns LRVB_ERR_INVALID; the other
 * outputs are then unspecified and no sums stay resident.  y is not validated here (the Python layer asks for y >= 0).      */
int lrvb_glmm_poisson_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                            int64_t G, int64_t K, double* value_out, double* grad_global_out, double* H_blocks_out,
                            double* group_sums_out, int32_t want_border);
/* Streamed weight influence of the Poisson mixed model: lrvb_glmm_slopes_obs_influence with, per unit weight,
 *   a1' = psi_n - y_n,   a2' = psi_n / 2
 * from one exp per row.  Operand layouts, the row window [n0, n1), the output, "a window equals the same rows of the full
 * result bitwise" and "no reduce-hook call" as there; errors as lrvb_glmm_poisson_terms, and n0 > n1 or n1 > n_obs:
 * LRVB_ERR_INVALID.                                                                                                          */
int lrvb_glmm_poisson_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                    int64_t G, int64_t K, const double* A_global, const double* A_local, int64_t Q, int64_t n0,
                                    int64_t n1, double* out);
/* Group influence of that model: out[g][q] = sum over the rows n of group g of w_n * (the row of lrvb_glmm_poisson_obs_influence)
 * (G x Q, host), as lrvb_glmm_slopes_group_influence: a fixed-order sum of 2 K + 2 P columns per group, an exact zero row for
 * an empty group, ONE reduce-hook call on the G x Q result.  Errors as lrvb_glmm_poisson_obs_influence.                       */
int lrvb_glmm_poisson_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                      const double* r, int64_t G, int64_t K, const double* A_global, const double* A_local,
                                      int64_t Q, double* out);

/* ---- binomial mixed model with K <= 4 independent random effects per group, per-row trials and offset ----
 *   y_n ~ Binomial(m_n, sigma(o_n + x_n . beta + z_n . u_g(n))),  q(beta_j) = N(mean_j, var_j),  q(u_gk) = N(e_gk, r_gk).
 * The per-row trial counts m (n doubles; real values are accepted) live in one device buffer of their own, the sibling of the
 * offset's: trials == NULL clears it (one trial per row); it is replaced by the next call; only the three lrvb_glmm_binomial_*
 * entries read it; the call drops the resident group sums and factor.  A length other than n_obs is found when a binomial entry
 * runs: LRVB_ERR_STATE there.  n < 1 with non-null trials: LRVB_ERR_SIZE.                                                     */
int lrvb_set_trials(lrvb_ctx* ctx, const double* trials, int64_t n);
/* The link of the binomial mixed model, a sibling of lrvb_set_trials:
 *   LRVB_LINK_LOGIT (the default)  p = sigma(t)           every lrvb_glmm_binomial_* entry exactly as documented below
 *   LRVB_LINK_PROBIT               p = Phi(t)
 *   LRVB_LINK_CLOGLOG              p = 1 - exp(-e^t)
 * Any other value: LRVB_ERR_UNSUPPORTED, the state untouched.  Only the four lrvb_glmm_binomial_* entries (terms, obs_influence,
 * group_influence, predict) read it; the logistic lrvb_glmm_slopes_*, the Poisson and the lrvb_glmm_arrow_* entries do not.  The call
 * drops the resident group sums, the factor and the group covariance, as lrvb_set_trials does (a following
 * lrvb_glmm_slopes_schur: LRVB_ERR_STATE).  Under the probit and the cloglog link, with h1 = -log p, h0 = -log(1 - p),
 * H_n = y_n h1 + (m_n - y_n) h0 and t ~ N(rho_n, s_n), rho_n including the offset:
 *   value = sum_n w_n E H_n(t)                                                            (log C(m_n, y_n) is dropped)
 *   a1 = w E H', a2 = w E H'' / 2, c11 = w E H'', c12 = w E H''' / 2, c22 = w E H'''' / 4   (Stein's identity on the nodes)
 * in the five-row layout, the scratch sizes and the summation order of the logit entries; E h1^(k) by the Gauss-Hermite rule of
 * the caller's nodes, probit E h0^(k) by the same rule at -t, cloglog E h0^(k) = exp(rho + s / 2) exactly and NOT clamped: a point
 * where it overflows is refused with LRVB_ERR_INVALID, as by lrvb_glmm_poisson_terms.  The influence entries use, per unit weight,
 * a1' = E H' (there is no "- y_n") and a2' = E H'' / 2.  The predict entry returns the response-scale means m Phi(rho / sqrt(1 + var))
 * (probit, closed form) and m E [1 - exp(-e^t)] (cloglog, on the nodes).  y is read from LRVB_SLOT_Y in the original row order.  */
#define LRVB_LINK_LOGIT 0
#define LRVB_LINK_PROBIT 1
#define LRVB_LINK_CLOGLOG 2
int lrvb_set_link(lrvb_ctx* ctx, int32_t link);
/* Data term of that model at (mean, var (P each), e, r (G x K each, group-major)), with the Gauss-Hermite rule of
 * lrvb_glmm_slopes_terms, the offset of lrvb_set_offset (none: 0) and the trials of lrvb_set_trials (none: 1):
 *   rho_n = o_n + x_n . mean + z_n . e_g(n),  s_n as there,  psi = E softplus(t), t ~ N(rho_n, s_n)
 *   value = sum_n w_n [m_n psi(rho_n, s_n) - y_n rho_n]                                  (log C(m_n, y_n) is dropped)
 * and the five per-row coefficients of lrvb_glmm_slopes_terms with every derivative of psi times m_n.  With no trials and no
 * offset (or ones and zeros) every output equals that of lrvb_glmm_slopes_terms bit for bit.  With m_n = y_n + phi and the offset
 * o_n - log phi the value is the parameter-dependent part of the negative-binomial (NB2) term with dispersion phi.  Arguments,
 * outputs, the column layout of group_sums_out, want_border, the fixed summation order and the reduce-hook contract (ONE buffer
 * [H blocks, when asked for | group sums | gradient | value], one hook call) are those of lrvb_glmm_slopes_terms; the group sums
 * stay resident for lrvb_glmm_slopes_schur, lrvb_glmm_slopes_solve_forward and lrvb_glmm_slopes_solve_back.  Errors as
 * lrvb_glmm_slopes_terms, and an offset or trials buffer whose length is not n_obs: LRVB_ERR_STATE.  y, the trials and the offset
 * are not validated here (the Python layer asks for finite values, trials >= 0 and 0 <= y <= trials).                        */
int lrvb_glmm_binomial_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                             int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out,
                             double* grad_global_out, double* H_blocks_out, double* group_sums_out, int32_t want_border);
/* Streamed weight influence of the binomial mixed model: lrvb_glmm_slopes_obs_influence with, per unit weight,
 *   a1' = m_n psi_rho(rho_n, s_n) - y_n,   a2' = m_n psi_s(rho_n, s_n),   rho_n including the offset.
 * Operand layouts, the row window, the output, "a window equals the same rows of the full result bitwise" and "no reduce-hook
 * call" as there; errors as lrvb_glmm_binomial_terms, and n0 > n1 or n1 > n_obs: LRVB_ERR_INVALID.                            */
int lrvb_glmm_binomial_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                     int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                     const double* A_global, const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence of that model: out[g][q] = sum over the rows n of group g of w_n * (the row of lrvb_glmm_binomial_obs_influence)
 * (G x Q, host), as lrvb_glmm_slopes_group_influence: a fixed-order sum of 2 K + 2 P columns per group, an exact zero row for
 * an empty group, ONE reduce-hook call on the G x Q result.  Errors as lrvb_glmm_binomial_obs_influence.                      */
int lrvb_glmm_binomial_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                       const double* r, int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                       const double* A_global, const double* A_local, int64_t Q, double* out);

/* ---- zero-truncated Poisson mixed model with K <= 4 independent random effects per group ---------------
 *   y_n in {1, 2, ..},  P(y_n | t_n) = e^{y_n t_n - u_n} / (y_n! (1 - e^{-u_n})),  u_n = e^{t_n},  t_n = o_n + x_n . beta + z_n . u_g(n):
 * the count part of a hurdle model (the zero part is the binomial model on 1[y > 0] under any link).  Canonical in t with the
 * log-partition A(t) = log(e^u - 1) = u + log(-expm1(-u)); A' = u + r is the response mean u / (1 - e^{-u}), r = u / expm1(u).
 * Data term at (mean, var (P each), e, r (G x K each, group-major)), with the Gauss-Hermite rule of lrvb_glmm_slopes_terms and the
 * offset of lrvb_set_offset (none: 0):
 *   rho_n = o_n + x_n . mean + z_n . e_g(n),  s_n as there,  t ~ N(rho_n, s_n)
 *   value = sum_n w_n [E A(t) - y_n rho_n]                                                       (log y_n! is dropped)
 *   a1 = w (E A' - y), a2 = w E A'' / 2, c11 = w E A'', c12 = w E A''' / 2, c22 = w E A'''' / 4    (Stein's identity on the nodes)
 * in the five-row layout, the scratch sizes and the summation order of the logistic entries.  The e^t part of every E A^(k) is
 * exp(rho + s / 2) exactly and NOT clamped; log(-expm1(-u)) and the derivatives of r go on the caller's nodes.  A point where
 * exp(rho + s / 2) overflows, or where e^t underflows to 0 on a node, gives a value that is not finite after the reduction: the
 * call returns LRVB_ERR_INVALID, the other outputs are then unspecified and no sums stay resident.  Arguments, outputs, the column
 * layout of group_sums_out, want_border, the fixed summation order (two calls at one point are bitwise equal) and the reduce-hook
 * contract are those of lrvb_glmm_slopes_terms; the group sums stay resident for lrvb_glmm_slopes_schur,
 * lrvb_glmm_slopes_solve_forward, lrvb_glmm_slopes_solve_back and lrvb_glmm_slopes_group_cov.  The entries read neither
 * lrvb_set_trials nor lrvb_set_link.  Errors as lrvb_glmm_slopes_terms (P > 64, K < 1, K > 4 or more than 128 nodes:
 * LRVB_ERR_UNSUPPORTED), and an offset whose length is not n_obs: LRVB_ERR_STATE.  y is not validated here (the Python layer
 * asks for finite y >= 1).                                                                                                    */
int lrvb_glmm_ztpoisson_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                              int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out,
                              double* grad_global_out, double* H_blocks_out, double* group_sums_out, int32_t want_border);
/* Streamed weight influence of the zero-truncated Poisson mixed model: lrvb_glmm_slopes_obs_influence with, per unit weight,
 *   a1' = E A' - y_n = exp(rho_n + s_n / 2) + E r(t) - y_n,   a2' = E A'' / 2,   rho_n including the offset.
 * Operand layouts, the row window, the output, "a window equals the same rows of the full result bitwise" and "no reduce-hook
 * call" as there; errors as lrvb_glmm_ztpoisson_terms, and n0 > n1 or n1 > n_obs: LRVB_ERR_INVALID.                           */
int lrvb_glmm_ztpoisson_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                      int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                      const double* A_global, const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence of that model: out[g][q] = sum over the rows n of group g of w_n * (the row of lrvb_glmm_ztpoisson_obs_influence)
 * (G x Q, host), as lrvb_glmm_slopes_group_influence: a fixed-order sum of 2 K + 2 P columns per group, an exact zero row for
 * an empty group, ONE reduce-hook call on the G x Q result.  Errors as lrvb_glmm_ztpoisson_obs_influence.                     */
int lrvb_glmm_ztpoisson_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                        const double* r, int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                        const double* A_global, const double* A_local, int64_t Q, double* out);

/* ---- zero-truncated negative binomial (NB2) mixed model with K <= 4 independent random effects per group --
 *   y_n in {1, 2, ..},  P(y_n | t_n) = NB2(y_n; mu_n = e^{t_n}, phi_n) / (1 - (1 + mu_n / phi_n)^{-phi_n}),  t_n = o_n + x_n . beta + z_n . u_g(n):
 * the count part of a hurdle model for over-dispersed counts, with a KNOWN per-row dispersion phi_n > 0.
 * lrvb_set_dispersion, a sibling of lrvb_set_trials: n_obs positive finite values in one device buffer of their own, or NULL to
 * clear them; replaced by the next call.  Only the lrvb_glmm_ztnegbin_*, lrvb_glmm_beta_*, lrvb_glmm_gamma_* and lrvb_glmm_censnormal_* entries read it.  The call drops the resident group sums,
 * the factor and the group covariance.  A value that is not positive and finite: LRVB_ERR_INVALID, checked on the host ahead of
 * everything else (the state is left as it was); n < 1 with a non-null pointer: LRVB_ERR_SIZE (the dispersion is then cleared, as
 * lrvb_set_trials clears the trials); a length other than n_obs is found when an entry runs: LRVB_ERR_STATE.                    */
int lrvb_set_dispersion(lrvb_ctx* ctx, const double* phi, int64_t n);
/* Data term.  The offset of lrvb_set_offset is the SHIFTED one, o_n - log phi_n (as for the NB2 model on the binomial entries),
 * so that eta = t - log phi ~ N(rho_n, s_n) with rho_n = offset_n + x_n . mean + z_n . e_g(n) and s_n as in lrvb_glmm_slopes_terms.
 * With sp = softplus, v = phi sp(eta) and g = log(1 - exp(-v)) (the log of 1 - P(y = 0)):
 *   H(eta) = (y + phi) sp(eta) - y eta + g(eta)                         (lgamma(y + phi) - lgamma(phi) - log y! is dropped)
 *   value = sum_n w_n E H,  a1 = w E H',  a2 = w E H'' / 2,  c11 = w E H'',  c12 = w E H''' / 2,  c22 = w E H'''' / 4
 * (Stein's identity on the caller's Gauss-Hermite nodes) in the five-row layout, the scratch sizes and the summation order of the
 * logistic entries.  Past v = 700 the derivatives of g are exact zeros; where v underflows to 0 on a node (eta below about -745)
 * the value is not finite after the reduction: the call returns LRVB_ERR_INVALID, the other outputs are then unspecified and no
 * sums stay resident.  Arguments, outputs, the column layout of group_sums_out, want_border, the fixed summation order (two calls
 * at one point are bitwise equal) and the reduce-hook contract are those of lrvb_glmm_slopes_terms; the group sums stay resident
 * for lrvb_glmm_slopes_schur, lrvb_glmm_slopes_solve_forward, lrvb_glmm_slopes_solve_back and lrvb_glmm_slopes_group_cov.  The
 * entries read neither lrvb_set_trials nor lrvb_set_link.  No dispersion set: LRVB_ERR_STATE ("no dispersion").  The other errors
 * are those of lrvb_glmm_ztpoisson_terms.  y is not validated here (the Python layer asks for finite y >= 1).                   */
int lrvb_glmm_ztnegbin_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                             int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out,
                             double* grad_global_out, double* H_blocks_out, double* group_sums_out, int32_t want_border);
/* Streamed weight influence of that model: lrvb_glmm_slopes_obs_influence with, per unit weight,
 *   a1' = (y_n + phi_n) E sigma(eta) + E g'(eta) - y_n,   a2' = E H'' / 2.
 * Operand layouts, the row window, the output, "a window equals the same rows of the full result bitwise" and "no reduce-hook
 * call" as there; errors as lrvb_glmm_ztnegbin_terms, and n0 > n1 or n1 > n_obs: LRVB_ERR_INVALID.                             */
int lrvb_glmm_ztnegbin_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                     int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                     const double* A_global, const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence of that model, as lrvb_glmm_ztpoisson_group_influence.  Errors as lrvb_glmm_ztnegbin_obs_influence.          */
int lrvb_glmm_ztnegbin_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                       const double* r, int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                       const double* A_global, const double* A_local, int64_t Q, double* out);

/* ---- Beta mixed model with K <= 4 independent random effects per group ------------------------------------
 *   0 < y_n < 1,  y_n ~ Beta(mu_n phi_n, (1 - mu_n) phi_n),  mu_n = sigma(t_n),  t_n = o_n + x_n . beta + z_n . u_g(n):
 * continuous proportions with a KNOWN per-row precision phi_n > 0 (lrvb_set_dispersion) and the RAW offset of lrvb_set_offset
 * (no log phi shift).  The context's y (LRVB_SLOT_Y) holds l_n = logit(y_n) = log y_n - log(1 - y_n).  With
 *   h(t) = lgamma(phi sigma(t)) + lgamma(phi sigma(-t)) - phi l sigma(t)
 *        = softplus(t) + softplus(-t) - 2 log phi + lgamma(1 + phi sigma(t)) + lgamma(1 + phi sigma(-t)) - phi l sigma(t)
 * (the second form is the one evaluated; lgamma(phi) + (phi - 1) log(1 - y) - log y is dropped), t ~ N(rho_n, s_n) with
 * rho_n = offset_n + x_n . mean + z_n . e_g(n) and s_n as in lrvb_glmm_slopes_terms:
 *   value = sum_n w_n E h,  a1 = w E h',  a2 = w E h'' / 2,  c11 = w E h'',  c12 = w E h''' / 2,  c22 = w E h'''' / 4
 * (Stein's identity on the caller's Gauss-Hermite nodes) in the five-row layout, the scratch sizes and the summation order of the
 * logistic entries.  No finite point is refused: as |t| grows h grows like |t| and nothing overflows.  A value that is not finite
 * after the reduction (a non-finite point, offset or l): LRVB_ERR_INVALID, the other outputs are then unspecified and no sums stay
 * resident.  Arguments, outputs, the column layout of group_sums_out, want_border, the fixed summation order (two calls at one
 * point are bitwise equal) and the reduce-hook contract are those of lrvb_glmm_slopes_terms; the group sums stay resident for
 * lrvb_glmm_slopes_schur, lrvb_glmm_slopes_solve_forward, lrvb_glmm_slopes_solve_back and lrvb_glmm_slopes_group_cov.  The
 * entries read neither lrvb_set_trials nor lrvb_set_link.  No dispersion set, or one of another length than n_obs:
 * LRVB_ERR_STATE.  The other errors are those of lrvb_glmm_ztpoisson_terms.  y is not validated here (the Python layer asks for
 * y strictly inside (0, 1)).  The fitted mean E sigma(t) does not depend on phi: lrvb_glmm_binomial_predict on a context without
 * trials and with the logit link is the predict entry of this model.                                                          */
int lrvb_glmm_beta_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                         int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out,
                         double* grad_global_out, double* H_blocks_out, double* group_sums_out, int32_t want_border);
/* Streamed weight influence of that model: lrvb_glmm_slopes_obs_influence with, per unit weight, a1' = E h' (there is no "- y":
 * the response sits inside h) and a2' = E h'' / 2.  Operand layouts, the row window, the output, "a window equals the same rows
 * of the full result bitwise" and "no reduce-hook call" as there; errors as lrvb_glmm_beta_terms, and n0 > n1 or n1 > n_obs:
 * LRVB_ERR_INVALID.                                                                                                            */
int lrvb_glmm_beta_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                 int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                 const double* A_global, const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence of that model, as lrvb_glmm_ztpoisson_group_influence.  Errors as lrvb_glmm_beta_obs_influence.              */
int lrvb_glmm_beta_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                   const double* r, int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                   const double* A_global, const double* A_local, int64_t Q, double* out);

/* ---- the derivative in the log-dispersion of the Beta and the NB2 mixed model -----------------------------
 * The dispersion of either model as phi_n = e^lambda phi0_n with ONE scalar lambda; d/d lambda = phi_n d/d phi_n at a fixed point.
 * With h the row term of the family's terms entry (lrvb_glmm_beta_terms; lrvb_glmm_binomial_terms with the logit link, the
 * trials y + phi and the offset o - log phi: NB2) and h_l, h_ll its first and second derivative in lambda at fixed t:
 *   d_out[0] = sum_n w_n E h_l,   d_out[1] = sum_n w_n E h_ll                                   (data terms only: the constant that the
 *                                                                                            value drops depends on phi too and is the caller's),
 *   cross_global_out (2 P) = [sum_n d1_n x_n | sum_n d2_n x_n o x_n],   d1 = w E d_t h_l,  d2 = w E d_t^2 h_l / 2,
 *   cross_local_out (G x 2 K, row-major) = per group [sum d1 z_k (K) | sum d2 z_k^2 (K)],
 * the derivative in lambda of the gradient of the data term in the coordinates (mean, var, e, r) of the terms entries.  Beta:
 *   h_l = a psi(1 + a) + b psi(1 + b) - l a - 2,  a = phi sigma(t), b = phi sigma(-t), l = logit y;  NB2, eta = t - log phi, m = y + phi:
 *   h_l = phi softplus(eta) - m sigma(eta) + y.
 * The context's state is that of the family's terms entry, and the dispersion of lrvb_set_dispersion for BOTH (the binomial
 * entries themselves never read it: results of lrvb_glmm_binomial_* are unchanged by that call).  No dispersion, or one of another
 * length than n_obs (NB2 also: no trials): LRVB_ERR_STATE.  P > 64, K outside 1..4, n_nodes outside 1..128, and for the NB2 entry a
 * link other than logit: LRVB_ERR_UNSUPPORTED.  A result that is not finite after the reduction: LRVB_ERR_INVALID.  The other
 * errors are those of lrvb_glmm_beta_terms.  One pass over the group-sorted rows; no atomics, a fixed summation order: two calls
 * at one point are bitwise equal; an empty group's row is zero and a row of weight zero contributes exact zeros.  The entries
 * write NEITHER the resident group sums NOR the factor NOR the group covariance of the context and drop none of them.  With a
 * reduce hook installed the packed result [cross_local | cross_global | d] goes through it in ONE call.                        */
int lrvb_glmm_beta_dispersion_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                    int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* d_out,
                                    double* cross_global_out, double* cross_local_out);
int lrvb_glmm_negbin_dispersion_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                      int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* d_out,
                                      double* cross_global_out, double* cross_local_out);

/* ---- Gamma mixed model with a log link and K <= 4 independent random effects per group -------------------
 *   y_n > 0,  y_n ~ Gamma(shape phi_n, mean mu_n),  mu_n = exp(t_n),  t_n = o_n + x_n . beta + z_n . u_g(n):
 * positive continuous responses with a KNOWN per-row shape phi_n > 0 (lrvb_set_dispersion) and the RAW offset of lrvb_set_offset.
 * The context's y (LRVB_SLOT_Y) holds log y_n.  With h(t) = phi (y e^{-t} + t) (phi log phi - lgamma(phi) + (phi - 1) log y is
 * dropped), t ~ N(rho_n, s_n) with rho_n = offset_n + x_n . mean + z_n . e_g(n) and s_n as in lrvb_glmm_slopes_terms, the
 * expectation is closed form, g = phi exp((log y - rho) + s / 2), ONE exp per row and no quadrature nodes:
 *   value = sum_n w_n (g + phi rho),  a1 = w (phi - g),  a2 = w g / 2,  c11 = w g,  c12 = -w g / 2,  c22 = w g / 4
 * in the two-row layout, the scratch sizes and the summation order of the Poisson entries (the sign of c12 rides on the factor of
 * its sums).  The kernel does not clamp: where g overflows for some row the value is not finite after the reduction:
 * LRVB_ERR_INVALID, the other outputs are then unspecified and no sums stay resident.  g underflowing to 0 is a legitimate point
 * (the row's term is phi rho).  Arguments, outputs, the column layout of group_sums_out, want_border, the fixed summation order
 * (two calls at one point are bitwise equal) and the reduce-hook contract are those of lrvb_glmm_poisson_terms; the group sums
 * stay resident for lrvb_glmm_slopes_schur, lrvb_glmm_slopes_solve_forward, lrvb_glmm_slopes_solve_back and
 * lrvb_glmm_slopes_group_cov.  The entries read neither lrvb_set_trials nor lrvb_set_link.  No dispersion set, or one of another
 * length than n_obs: LRVB_ERR_STATE.  The other errors are those of lrvb_glmm_poisson_terms.  y is not validated here (the Python
 * layer asks for finite y > 0).  The fitted mean E e^t = exp(rho + s / 2) does not depend on phi: lrvb_glmm_poisson_predict is
 * the predict entry of this model (it reads the offset and never y).                                                            */
int lrvb_glmm_gamma_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                          int64_t G, int64_t K, double* value_out, double* grad_global_out, double* H_blocks_out,
                          double* group_sums_out, int32_t want_border);
/* Streamed weight influence of that model: lrvb_glmm_poisson_obs_influence with, per unit weight, a1' = phi - g (there is no
 * "- y": the response sits inside g) and a2' = g / 2.  Operand layouts, the row window, the output, "a window equals the same
 * rows of the full result bitwise" and "no reduce-hook call" as there; errors as lrvb_glmm_gamma_terms, and n0 > n1 or
 * n1 > n_obs: LRVB_ERR_INVALID.                                                                                                 */
int lrvb_glmm_gamma_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                  int64_t G, int64_t K, const double* A_global, const double* A_local, int64_t Q, int64_t n0,
                                  int64_t n1, double* out);
/* Group influence of that model, as lrvb_glmm_poisson_group_influence.  Errors as lrvb_glmm_gamma_obs_influence.                */
int lrvb_glmm_gamma_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                    const double* r, int64_t G, int64_t K, const double* A_global, const double* A_local, int64_t Q,
                                    double* out);
/* The derivative in the log-dispersion lambda (phi_n = e^lambda phi0_n) of that model, as lrvb_glmm_beta_dispersion_terms without
 * the nodes.  h is linear in phi, so h_l = h_ll = h: d_out[0] = d_out[1] = the data term of lrvb_glmm_gamma_terms and the cross
 * terms are its gradient, here formed by a kernel of their own.  Reads the state of lrvb_glmm_gamma_terms; writes NEITHER the
 * resident group sums NOR the factor NOR the group covariance and drops none of them.  Errors as lrvb_glmm_gamma_terms.         */
int lrvb_glmm_gamma_dispersion_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                     int64_t G, int64_t K, double* d_out, double* cross_global_out, double* cross_local_out);

/* ---- censored Gaussian (Tobit) mixed model with K <= 4 independent random effects per group --------------
 *   y*_n ~ N(t_n, 1 / phi_n),  t_n = o_n + x_n . beta + z_n . u_g(n),  and a status delta_n per row: 0, y_n = y*_n is observed;
 *   +1, right-censored (y*_n > y_n); -1, left-censored (y*_n < y_n).  On log-times it is the log-normal accelerated-failure-time
 * model with shared frailties.  The precision phi_n > 0 is KNOWN per row (lrvb_set_dispersion), the offset the RAW one of
 * lrvb_set_offset, and the context's y (LRVB_SLOT_Y) holds y_n.
 * lrvb_set_censoring, a sibling of lrvb_set_dispersion: n_obs values in {-1, 0, +1}, kept in one device buffer of their own, or
 * NULL to clear them; replaced by the next call.  Only the lrvb_glmm_censnormal_* entries read it.  The call drops the resident
 * group sums, the factor and the group covariance.  Any other value: LRVB_ERR_INVALID, checked on the host ahead of everything else
 * (the state is left as it was); n < 1 with a non-null pointer: LRVB_ERR_SIZE (the status is then cleared); a length other than
 * n_obs is found when an entry runs: LRVB_ERR_STATE.                                                                            */
int lrvb_set_censoring(lrvb_ctx* ctx, const int32_t* status, int64_t n);
/* Data term.  With r = sqrt(phi), t ~ N(rho_n, s_n), rho_n = offset_n + x_n . mean + z_n . e_g(n) and s_n as in
 * lrvb_glmm_slopes_terms, the row term is
 *   observed   h(t) = phi (y - t)^2 / 2            (1/2 log phi - 1/2 log 2 pi is dropped): closed form, no nodes,
 *              E h = phi ((y - rho)^2 + s) / 2,  E h' = -phi (y - rho),  E h'' = phi,  E h''' = E h'''' = 0;
 *   censored   h(t) = -log Phi(a),  a = delta r (t - y): d_t^k h = (delta r)^k H^(k)(a), H = -log Phi, on the caller's Gauss-Hermite
 *              nodes with the inverse-Mills evaluation of the probit link (lrvb_glmm_binomial_terms under LRVB_LINK_PROBIT);
 *   value = sum_n w_n E h,  a1 = w E h',  a2 = w E h'' / 2,  c11 = w E h'',  c12 = w E h''' / 2,  c22 = w E h'''' / 4
 * in the five-row layout, the scratch sizes and the summation order of the logistic entries.  The kernel does not clamp: a value
 * that is not finite after the reduction (phi (rho - y)^2 overflows, or a^2 / 2 in the tail of a censored row): LRVB_ERR_INVALID,
 * the other outputs are then unspecified and no sums stay resident.  Arguments, outputs, the column layout of group_sums_out,
 * want_border, the fixed summation order (two calls at one point are bitwise equal) and the reduce-hook contract are those of
 * lrvb_glmm_slopes_terms; the group sums stay resident for lrvb_glmm_slopes_schur, the two solves and lrvb_glmm_slopes_group_cov.
 * The entries read neither lrvb_set_trials nor lrvb_set_link.  No dispersion or no status set, or one of another length than
 * n_obs: LRVB_ERR_STATE.  The other errors are those of lrvb_glmm_ztpoisson_terms.  y is not validated here (the Python layer
 * asks for finite y).                                                                                                           */
int lrvb_glmm_censnormal_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                               int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out,
                               double* grad_global_out, double* H_blocks_out, double* group_sums_out, int32_t want_border);
/* Streamed weight influence of that model: lrvb_glmm_slopes_obs_influence with, per unit weight, a1' = E h' (there is no "- y":
 * the response sits inside h) and a2' = E h'' / 2.  Operand layouts, the row window, the output, "a window equals the same rows
 * of the full result bitwise" and "no reduce-hook call" as there; errors as lrvb_glmm_censnormal_terms, and n0 > n1 or
 * n1 > n_obs: LRVB_ERR_INVALID.                                                                                                 */
int lrvb_glmm_censnormal_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                       int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                       const double* A_global, const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence of that model, as lrvb_glmm_ztpoisson_group_influence.  Errors as lrvb_glmm_censnormal_obs_influence.         */
int lrvb_glmm_censnormal_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                         const double* r, int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                         const double* A_global, const double* A_local, int64_t Q, double* out);
/* The derivative in the log-precision lambda (phi_n = e^lambda phi0_n, so d a / d lambda = a / 2) of that model, as
 * lrvb_glmm_beta_dispersion_terms.  Observed rows are linear in phi: h_l = h_ll = h, d_t h_l = h', d_t^2 h_l = h''.  Censored rows:
 *   h_l = a H' / 2,  h_ll = a (a H'' + H') / 4,  d_t h_l = delta r (a H'' + H') / 2,  d_t^2 h_l = phi (a H''' + 2 H'') / 2.
 * Reads the state of lrvb_glmm_censnormal_terms; writes NEITHER the resident group sums NOR the factor NOR the group covariance
 * and drops none of them.  Errors as lrvb_glmm_censnormal_terms.                                                                */
int lrvb_glmm_censnormal_dispersion_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e,
                                          const double* r, int64_t G, int64_t K, const double* gh_x, const double* gh_w,
                                          int32_t n_nodes, double* d_out, double* cross_global_out, double* cross_local_out);

/* ---- ordinal mixed model, cumulative logit link, K <= 4 independent random effects per group --------------
 *   y_n in {0 .. T},  P(y_n <= j | t_n) = sigma(alpha_{j+1} - t_n),  t_n = o_n + x_n . beta + z_n . u_g(n),
 * with T cut points alpha_1 < .. < alpha_T (2 <= T + 1 <= 16 ordered categories).  The offset is the RAW one of lrvb_set_offset and the
 * context's y (LRVB_SLOT_Y) holds the categories as doubles.
 * lrvb_set_thresholds: T finite, strictly increasing values, 1 <= T <= 15, kept with both sentinels -inf and +inf in one device
 * table of 17 doubles; replaced by the next call, which touches nothing of length n_obs.  Only the lrvb_glmm_ordinal_* entries read
 * it.  The call drops the resident group sums, the factor and the group covariance.  A null pointer, a T outside 1 .. 15, a value that
 * is not finite or not above the one before it: LRVB_ERR_INVALID, checked on the host ahead of everything else (the state is left as
 * it was).                                                                                                                       */
int lrvb_set_thresholds(lrvb_ctx* ctx, const double* alpha, int64_t T);
/* Data term.  With lo = alpha_y, hi = alpha_{y+1} (alpha_0 = -inf, alpha_{T+1} = +inf), D = hi - lo, t ~ N(rho_n, s_n),
 * rho_n = offset_n + x_n . mean + z_n . e_g(n) and s_n as in lrvb_glmm_slopes_terms, the row term is
 *   h(t) = -log[sigma(hi - t) - sigma(lo - t)] = softplus(t - hi) + softplus(lo - t) - log(1 - e^-D)
 * whole (nothing is dropped: the last term depends on the thresholds), the two softplus terms on the caller's Gauss-Hermite nodes with
 * the expressions of the logistic entries, the third in closed form per row;
 *   value = sum_n w_n E h,  a1 = w E h',  a2 = w E h'' / 2,  c11 = w E h'',  c12 = w E h''' / 2,  c22 = w E h'''' / 4
 * in the five-row layout, the scratch sizes and the summation order of the logistic entries.  The kernel does not clamp values: one
 * that is not finite after the reduction: LRVB_ERR_INVALID, the other outputs are then unspecified and no sums stay resident.
 * Arguments, outputs, the column layout of group_sums_out, want_border, the fixed summation order (two calls at one point are bitwise
 * equal) and the reduce-hook contract are those of lrvb_glmm_slopes_terms; the group sums stay resident for lrvb_glmm_slopes_schur,
 * the two solves and lrvb_glmm_slopes_group_cov.  The entries read neither trials, link, dispersion nor censoring status.  No
 * thresholds set: LRVB_ERR_STATE.  A y that is not an integer in 0 .. T: LRVB_ERR_INVALID, found on the host before any kernel over
 * the rows is launched (y is read back once per lrvb_set_data and T; the kernels clamp the table index besides).  The other errors
 * are those of lrvb_glmm_ztpoisson_terms.                                                                                        */
int lrvb_glmm_ordinal_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                            int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* value_out,
                            double* grad_global_out, double* H_blocks_out, double* group_sums_out, int32_t want_border);
/* Streamed weight influence of that model: lrvb_glmm_slopes_obs_influence with, per unit weight, a1' = E h' (there is no "- y":
 * the response picks the cut points) and a2' = E h'' / 2.  Errors as lrvb_glmm_ordinal_terms, and n0 > n1 or n1 > n_obs:
 * LRVB_ERR_INVALID.                                                                                                              */
int lrvb_glmm_ordinal_obs_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                    int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                    const double* A_global, const double* A_local, int64_t Q, int64_t n0, int64_t n1, double* out);
/* Group influence of that model, as lrvb_glmm_ztpoisson_group_influence.  Errors as lrvb_glmm_ordinal_obs_influence.             */
int lrvb_glmm_ordinal_group_influence(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                      int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes,
                                      const double* A_global, const double* A_local, int64_t Q, double* out);
/* The derivatives of that data term in the thresholds alpha at fixed (mean, var, e, r): one pass over the rows, which forms its
 * products with x and z itself (a row touches two of the T thresholds).  With r = 1 / expm1(D), c = e^-D / expm1(-D)^2 (0 on an end
 * category) a row adds, times w, -E sigma(t - hi) - r to g[hi], E sigma(lo - t) + r to g[lo], E sigma'(t - hi) + c and
 * E sigma'(lo - t) + c to the diagonal and -c to the off-diagonal entry of (lo, hi): the Hessian in alpha is tridiagonal.
 *   g_out (T), h_diag_out (T), h_off_out (T - 1: entry j couples alpha_j+1 and alpha_j+2; untouched where T = 1),
 *   cross_global_out (T x 2 P, row j = [d/d mean | d/d var] of g[j]),  cross_local_out (G x T x 2 K, [d/d e | d/d r] of g[j]).
 * Fixed summation order for a given n_obs, no atomics: two calls at one point are bitwise equal.  Reads the state of
 * lrvb_glmm_ordinal_terms; writes NEITHER the resident group sums NOR the factor NOR the group covariance and drops none of them.
 * A sum that is not finite: LRVB_ERR_INVALID.  The other errors as lrvb_glmm_ordinal_terms.                                      */
int lrvb_glmm_ordinal_threshold_terms(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                      int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, double* g_out,
                                      double* h_diag_out, double* h_off_out, double* cross_global_out, double* cross_local_out);

/* ---- group blocks of H^-1, fitted values and predictions with their linear-response variance ------------
 * For every mixed model with K <= 4 effects per group.  After a successful lrvb_glmm_slopes_schur (the factor L_g, U_g resident)
 * and a factored free Schur complement S on the caller's side, with
 *   W (R x R, row-major) = (S^-1)[coupled rows, coupled rows], R = 2 P + 3 K in the order of M_out of lrvb_glmm_slopes_schur, and
 *   s (R) the scaling of the coupled rows of lrvb_glmm_slopes_solve_forward / _back (the border is Hx[r, l] = s_r C_g[l, r]),
 * Y_g = L_g^-T (U_g diag(s)) (2 K x R) gives the blocks of H^-1 of group g:
 *   Cov(coupled rows, l_g) = -W Y_g^T,   Cov(l_g, l_g) = A_g^-1 + Y_g W Y_g^T.
 * One workgroup per group writes the K leading rows (the means e_g. of the effects) into a RESIDENT buffer of G + 1 rows of
 * K K + K P doubles, [Sigma_uu (K x K, row-major) | Sigma_ubeta (K x P, k-major: the P values against the means of beta
 * contiguous)]; row G is the pseudo-group of a population-level prediction (u = mu): W[mu rows, mu rows] | W[mu rows, :P].
 * out (host, (G + 1) x (K K + K P); may be NULL) receives a copy.  Fixed order, no atomics: two calls give equal bits.  The
 * upload is R^2 + R doubles.  The buffer is dropped wherever the factor is (lrvb_glmm_slopes_terms and its siblings,
 * lrvb_set_group_design, lrvb_set_groups, lrvb_set_offset, lrvb_set_trials, the next lrvb_glmm_slopes_schur).
 * No reduce-hook call.  Errors as lrvb_glmm_slopes_solve_forward: a null W or s: LRVB_ERR_INVALID; K < 1 or K > 4:
 * LRVB_ERR_UNSUPPORTED; no resident factor of K effects: LRVB_ERR_STATE; G not the number of groups, P not n_cols: LRVB_ERR_SIZE. */
int lrvb_glmm_slopes_group_cov(lrvb_ctx* ctx, const double* W, const double* s, int64_t P, int64_t G, int64_t K, double* out);
/* The same on a factor of lrvb_glmm_arrow_schur: W is R x R and s has R entries, R = 2 P + NC in the order of its M_out.
 * Convention: THE FIRST K CLOSED COLUMNS ARE e_mu_0 .. e_mu_{K-1} (the pseudo-group reads the rows 2 P + k).  The buffer it leaves
 * resident is that of lrvb_glmm_slopes_group_cov, and the predict entries read it unchanged.  Errors as lrvb_glmm_arrow_solve_forward. */
int lrvb_glmm_arrow_group_cov(lrvb_ctx* ctx, const double* W, const double* s, int64_t P, int64_t G, int64_t K, int64_t NC, double* out);
/* Fitted values and predictions: the streaming sibling of lrvb_glmm_slopes_obs_influence.  Point arguments as there, except that
 * e and r are G' x K with G' = G or G + 1 (row G: the pseudo-group, e_mu and 1 / i_mu); cov_beta (P x P, row-major, host) is
 * Sigma_bb = W[:P, :P].  Per row with design (x, z), group g and offset o,
 *   rho = o + x . mean + z . e_g,   var_mf = (x o x) . var + (z o z) . r_g,
 *   var_lrvb = x^T Sigma_bb x + 2 sum_k z_k (x . Sigma_ubeta[g][k]) + z^T Sigma_uu[g] z      (blocks of the resident buffer),
 *   mean_mf, mean_lrvb = the response-scale mean of the likelihood at (rho, var_mf) and at (rho, var_lrvb): E sigma(t),
 *   t ~ N(rho, .), by the Gauss-Hermite rule (logistic); exp(rho + . / 2) (Poisson); m E sigma(t) (binomial, m the trials).
 * out (host, 5 x n row-major: rho | var_mf | var_lrvb | mean_mf | mean_lrvb).  The rows are
 *   x_new == NULL: the window [n0, n1) of the context's rows, groups, group design (and offset, trials), n = n1 - n0;
 *   x_new != NULL: n = n_new new rows x_new (n x P), z_new (n x K), gid_new (n int32 in [0, G')), offset_new and trials_new (n
 *   each; NULL: zero, one), uploaded to scratch; n0 and n1 are ignored.  A gid_new outside [0, G') is refused here, before
 *   anything is launched: LRVB_ERR_INVALID.
 * ONE pass over the rows in their order: a tile of 64 rows is staged on chip, x^T Sigma_bb x runs on the fp64 matrix cores, the
 * K P + K K values of the row's own group are gathered and added behind it.  A window equals the same rows of the full result
 * bitwise, and new rows that are copies of the context's rows give the context's bits.  Rank-local: NO reduce-hook call.
 * The resident blocks belong to the weights, offset and point at the time of lrvb_glmm_slopes_schur.  lrvb_set_weights does NOT
 * drop the resident mixed-model state (it never has): after a direct call of it these entries still return LRVB_OK, with blocks of the
 * OLD weights.  A caller who changes the weights runs the terms, lrvb_glmm_slopes_schur and lrvb_glmm_slopes_group_cov again (the
 * Python classes do, through the key of the point).
 * Errors as the _obs_influence sibling, and: no resident group covariance of K effects: LRVB_ERR_STATE; G' not G or G + 1:
 * LRVB_ERR_SIZE; a null cov_beta, out, z_new or gid_new, n_new < 0, a bad window: LRVB_ERR_INVALID.                              */
int lrvb_glmm_slopes_predict(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                             int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, const double* cov_beta,
                             int64_t n0, int64_t n1, const double* x_new, const double* z_new, const int32_t* gid_new, int64_t n_new,
                             double* out);
int lrvb_glmm_poisson_predict(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                              int64_t G, int64_t K, const double* cov_beta, int64_t n0, int64_t n1, const double* x_new,
                              const double* z_new, const int32_t* gid_new, const double* offset_new, int64_t n_new, double* out);
int lrvb_glmm_binomial_predict(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                               int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, const double* cov_beta,
                               int64_t n0, int64_t n1, const double* x_new, const double* z_new, const int32_t* gid_new,
                               const double* offset_new, const double* trials_new, int64_t n_new, double* out);
/* The zero-truncated Poisson model: the arguments of lrvb_glmm_binomial_predict without trials_new; the
 * response-scale mean is that of the TRUNCATED count, E A'(t) = exp(rho + . / 2) + E r(t), r = u / expm1(u) on the nodes.      */
int lrvb_glmm_ztpoisson_predict(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, const double* cov_beta,
                                int64_t n0, int64_t n1, const double* x_new, const double* z_new, const int32_t* gid_new,
                                const double* offset_new, int64_t n_new, double* out);
/* The zero-truncated NB2 model: the arguments of lrvb_glmm_binomial_predict with the dispersion of the new
 * rows (dispersion_new, n_new positive finite values, REQUIRED with new rows: LRVB_ERR_INVALID) in the place of trials_new;
 * offset_new is the shifted offset o - log phi of the new rows.  The response-scale mean is that of the TRUNCATED count,
 * E[e^t (1 + R(v))], R = 1 / expm1(v): phi exp(rho + . / 2) in closed form and not clamped, e^t R(v) on the nodes.               */
int lrvb_glmm_ztnegbin_predict(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                               int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, const double* cov_beta,
                               int64_t n0, int64_t n1, const double* x_new, const double* z_new, const int32_t* gid_new,
                               const double* offset_new, const double* dispersion_new, int64_t n_new, double* out);
/* The censored Gaussian model: the arguments of lrvb_glmm_ztpoisson_predict.  The response-scale mean is the
 * LATENT mean E y* = rho, whatever the precision and under either variance; neither y nor the status nor the precision of new
 * rows is asked for.                                                                                                            */
int lrvb_glmm_censnormal_predict(lrvb_ctx* ctx, const double* mean, const double* var, int64_t P, const double* e, const double* r,
                                 int64_t G, int64_t K, const double* gh_x, const double* gh_w, int32_t n_nodes, const double* cov_beta,
                                 int64_t n0, int64_t n1, const double* x_new, const double* z_new, const int32_t* gid_new,
                                 const double* offset_new, int64_t n_new, double* out);

/* ---- multinomial (softmax) regression ---------------------------------------------------------
 * K classes (2 <= K <= 17), labels y_n in {0 .. K-1}, class 0 the reference; coefficients beta ((K-1) x P, row-major, row a
 * belongs to class a + 1, P = n_cols <= 1024), z_na = x_n . beta_a, z_n0 = 0, p_n = softmax(z_n).  The data term
 *   f(beta) = sum_n w_n [ log sum_k exp(z_nk) - z_{n,y_n} ]
 * in vector coordinates eta = vec(beta) (D = (K-1) P entries).  Any context with a design matrix holds it
 * (LRVB_LOSS_DATA_ONLY is the natural choice: X and the weights, no GLM term); the existing entry points of that context keep
 * their meaning.  Every call runs on the context's stream and returns with its results on the host.
 * K > 17 or P > 1024: LRVB_ERR_UNSUPPORTED.  A softmax call before lrvb_softmax_set_labels: LRVB_ERR_STATE.
 * Reduce hook (lrvb_set_reduce_hook / lrvb_comm_init): every sum over observations of one call goes through the hook exactly
 * once, in one device buffer -- lrvb_softmax_terms: [H (D x D, only when hess is asked for) | gradient (D) | value (1)];
 * lrvb_softmax_hvp: the product (D).  lrvb_softmax_obs_influence forms per-row results only and makes no hook call.
 * The class probabilities of the last point are kept in the context (N x (K-1)); any change of data, weights, labels or hook
 * drops them, and a product or influence call at another point forms them again first (one more pass over X).           */
/* Uploads the labels (n = n_obs int32), checks 0 <= y < K (else LRVB_ERR_INVALID) and fixes K for the context.           */
int lrvb_softmax_set_labels(lrvb_ctx* ctx, const int32_t* labels, int64_t n, int32_t K);
/* Value, gradient (D, nullable) and Hessian (D x D, leading dimension ldh >= D, nullable) of the data term at beta.  One fused
 * pass over X (value, gradient, p), then K(K-1)/2 weighted SYRKs X^T diag(w p_a (delta_ab - p_b)) X, block (a, b) at rows
 * a P, columns b P, mirrored.                                                                                             */
int lrvb_softmax_terms(lrvb_ctx* ctx, const double* beta, int64_t K, int64_t P, double* value_out, double* grad_out,
                       double* hess_out, int64_t ldh);
/* out = H v (D) at beta, matrix-free: (H v)_a = sum_n w_n p_na (t_na - sum_b p_nb t_nb) x_n, t_nb = x_n . v_b; one pass over X
 * (two at a point whose p the context does not hold).                                                                    */
int lrvb_softmax_hvp(lrvb_ctx* ctx, const double* beta, int64_t K, int64_t P, const double* v, double* out);
/* Streamed weight-sensitivity rows: out[n - n0][q] = sum_a (p_na - [y_n = a + 1]) (A[q, a P : (a + 1) P] . x_n) for
 * n0 <= n < n1, i.e. A times d2 f / d beta d w_n (column n of the cross Hessian, never formed); A is Q x D row-major (host),
 * out (n1 - n0) x Q.  Step A of the pass with up to 16 columns per launch, then a per-row contraction over the classes.     */
int lrvb_softmax_obs_influence(lrvb_ctx* ctx, const double* beta, int64_t K, int64_t P, const double* A, int64_t Q,
                               int64_t n0, int64_t n1, double* out);

/* ---- objectives that are quadratic in the data ------------------------------------------
 * S = Z^T diag(w) Z (n_cols x n_cols, both triangles) with the context's current weights: the
 * weighted sufficient statistics sum_n w_n z_n z_n^T that `np.einsum('ni,ij,nj,n', ...)` at
 * Example.ipynb:262 and LRVB/regression_utils.py:59-88 contract on the host.                  */
int lrvb_weighted_gram(lrvb_ctx* ctx, double* S_out, int64_t ld);
/* The same with the sum of the weights, W = sum_n w_n (the -1/2 W log|Lambda| term of Example.ipynb:247-274), formed on the
 * device and summed over the ranks in the SAME reduction as S.                                                       */
int lrvb_weighted_gram_sum(lrvb_ctx* ctx, double* S_out, int64_t ld, double* wsum_out);
/* out[n - n0, k] = 1/2 z_n^T M_k z_n + c_k for K symmetric matrices M_k (K x n_cols x n_cols)
 * and offsets c (K): rows of the cross Hessian d2 f / d w_n d eta_k of such an objective
 * (TwoParameterObjective.fun_vector_hessian21 with par2 = weights,
 * LRVB/SparseObjectives.py:418-427; Example.ipynb:425-441).                                   */
int lrvb_obs_quadform(lrvb_ctx* ctx, const double* M, const double* c, int64_t K,
                      int64_t n0, int64_t n1, double* out);

/* Grouped sufficient statistics for hierarchical models (doc/lmm.lyx:105-160): group ids are set
 * once (0 <= gid < n_groups); lrvb_group_sums returns, with the current weights, an
 * n_groups x (1 + n_cols) matrix [ sum_g w | sum_g w z ].  n_cols <= 64.                        */
int lrvb_set_groups(lrvb_ctx* ctx, const int32_t* gid, int64_t n, int64_t n_groups);
int lrvb_group_sums(lrvb_ctx* ctx, double* out);
/* Both statistics of a hierarchical model in one call, [S = Z^T diag(w) Z (q x q) | group sums (G x (1 + q))], in ONE
 * device buffer that goes to the sum-over-ranks hook once and stays resident for lrvb_lmm_group_terms.  Either host
 * copy may be NULL.  For an even n_cols the rows are read from a group-sorted copy that is built when the group ids and
 * the data are set (one pass instead of two): data adopted with lrvb_set_data_dev must be installed again after its
 * contents change (as for the point state of lrvb_hvp); weights adopted with lrvb_set_weights_dev are re-read by
 * every call.                                                                                                         */
int lrvb_grouped_stats(lrvb_ctx* ctx, double* S_out, double* gs_out);
/* The hierarchical linear mixed model of doc/lmm.lyx:77-160 (y_i ~ N(x_i.beta + u_g[i], 1/tau_y), u_g ~ N(mu, 1/tau_mu),
 * q(u_g) = N(e_g, 1/i_g)): elimination of the 2 G local parameters on the device, from the resident grouped
 * statistics (Z = [x | y], q = p + 1).  par (8 + p) = [E tau_y, E tau_mu, E mu, d E tau_y / d (a_y, b_y), d E tau_mu / d
 * (a_mu, b_mu), lower bound of the i_g, mean of q(beta) (p)]; f_local (2 G) = FREE local parameters [e_g | log(i_g - lb)].
 * out (128 + (p + 5)^2): out[0 .. p) = sum_g e_g sum_g w x; out[64 ..] = sum e_g r_g, sum W_g (e_g^2 + 1/i_g),
 * sum (e_g - E mu)^2 + 1/i_g, sum (e_g - E mu), sum log i_g, sum W_g, squared norm of the free local gradient
 * (r_g = sum_g w y - m . sum_g w x); then M = H_gl H_ll^-1 H_lg on the p + 5 coupled rows [mean of q(beta) | E mu | a_y |
 * b_y | a_mu | b_mu] in vector coordinates of those rows and free coordinates of the local parameters (H_ll is
 * diagonal for this model) -- what the reference would obtain from the D x D autograd Hessian and a sparse solve
 * (LRVB/SparseObjectives.py:581-657).                                                                                  */
int lrvb_lmm_group_terms(lrvb_ctx* ctx, const double* par, int64_t n_par, const double* f_local, int64_t n_local, double* out);
/* ---- a whole step of configurations 2 and 4 as ONE call (round 4) --------------------------------------------------------
 * The N-independent closed forms of these models are affine in the sufficient statistics, with coefficients that depend on
 * theta only.  The caller sends those coefficients (`hp`: P = Lambda^-1, polygamma values, priors -- see csrc/k_lmm.hip for
 * the layout) together with theta in ONE upload; the library forms the statistics (summed over the ranks), combines them
 * with the coefficients in a single-workgroup kernel where they lie, writes the Kronecker block of the information matrix,
 * and converts to free coordinates (LRVB/Parameters.py:397-424) -- no device-to-host copy inside the call.  The result
 * stays in HBM (lrvb_chol_factor_last factors it); H_out / value_out / sums_out may be NULL.
 *
 * lrvb_mvnreg_hessian: MVNParam regression (configuration 2; LRVB/NormalParams.py:6-23, GammaParams.py:4-16,
 *   regression_utils.py:59-132), the context holds the rows [x | y]; idx = vector positions of [mean, vech(information),
 *   shape, rate].  From the third call of one shape on, the launch chain behind the upload is replayed as a captured
 *   hipGraph (a dozen dependent kernels of ~5 us: 117 -> 92 us per step); plain launches under lrvb_profile_enable, a
 *   sum-over-ranks hook or tuning bit 0, and after any change of stream, shape or buffer addresses (re-captured).
 * lrvb_lmm_global_hessian: hierarchical LMM (configuration 4; doc/lmm.lyx:77-160): `data_ctx` holds the rows [x | y] and the
 *   groups, `global_ctx` the packing of the global parameters; idx = vector positions of [mean, vech(information), e_mu,
 *   i_mu, a_y, b_y, a_mu, b_mu]; free_val = [global free parameters | e_1..e_G | log(i_g - info_lb)].  Result: the Schur
 *   complement of the arrow Hessian onto the global block, in free coordinates, in global_ctx.  Both contexts' launches
 *   are queued on data_ctx's stream for the length of the call; global_ctx's own stream waits for it before and after.  */
int lrvb_mvnreg_hessian(lrvb_ctx* ctx, const double* free_in, int64_t D, const double* hp, int64_t n_hp, const int32_t* idx,
                        double* value_out, double* H_out);
int lrvb_lmm_global_hessian(lrvb_ctx* data_ctx, lrvb_ctx* global_ctx, const double* free_val, int64_t n_free, const double* hp,
                            int64_t n_hp, const int32_t* idx, double info_lb, double* sums_out, double* H_out);

/* Mixture models with a SimplexParam row per observation (LRVB/SimplexParams.py:69-175): for every
 * row, on one wavefront, the simplex map and its closed-form Jacobian / Hessian (:33-63), the local
 * (K-1) x (K-1) free Hessian block, its Cholesky factor and A_n = J_n H_nn^-1 J_n^T; then the
 * Schur-complement operand R = sum_n w_n^2 (x~_n (x) x~_n) vec(A_n)^T ((V+1)^2 x K^2) by an MFMA GEMM,
 * the sufficient statistics S64 = [x~ | z]^T diag(w) [x~ | z] (64 x 64, x~ padded to 32, z to 32),
 * val2 = [-sum w z.s, sum w z log z] and the free local gradient (N x (K-1); may be NULL, as may
 * R_out).  s_n = x~_n Lam, Lam = [E log pi; E log phi] ((V+1) x K), x~_n = (1, x_n).
 * V + 1 <= 32, 2 <= K <= 32.  theta_z == NULL evaluates at the simplex logits of the previous call, which
 * stay resident in HBM (the local part of the evaluation point: N (K-1) doubles).                    */
int lrvb_mixture_rows(lrvb_ctx* ctx, int32_t K, const double* theta_z, const double* Lam,
                      double* val2_out, double* gfree_out, double* S64_out, double* R_out);

/* Schur complement of the mixture's global (Dirichlet) block onto itself, assembled on the device:
 *   H_out = diag(scale) Hgg diag(scale) + diag(diag_add) - sym(Jlam^T Rm Jlam),
 * Rm[(j K + k), (j' K + k')] = R[(j q + j'), (k K + k')], n = q K.  R is the (q^2 x K^2) operand of
 * lrvb_mixture_rows (after the all-reduce over shards when there is one); NULL = the result of the last
 * lrvb_mixture_rows call on this context, still resident.  Jlam (n x n) = d vec(Lam) / d free with rows
 * ordered (j, k); Hgg (n x n) the global block without the Schur term; scale / diag_add (n, nullable)
 * the free-coordinate chain rule of a box block (LRVB/Parameters.py:397-424).  Two n^3 MFMA GEMMs
 * replace the host contraction the reference would do with sparse Jacobian lists.  All host pointers. */
int lrvb_mixture_schur(lrvb_ctx* ctx, int32_t K, int32_t q, const double* R, const double* Jlam,
                       const double* Hgg, const double* scale, const double* diag_add, double* H_out);
/* lrvb_mixture_rows without the per-row gradient and WITHOUT copying the Schur operand to the host: it is summed over
 * the ranks (with the other statistics, in one reduction) and stays resident for the Schur assembly below.          */
int lrvb_mixture_stats(lrvb_ctx* ctx, int32_t K, const double* theta_z, const double* Lam, int32_t want_schur,
                       double* val2_out, double* S64_out);
/* lrvb_mixture_schur with both n x n inputs generated on the device from their O(n) description.  The Dirichlet
 * blocks make d vec(Lam) / d alpha and the global Hessian block "diagonal plus a constant per Dirichlet"
 * (LRVB/ExponentialFamilies.py:114-120, DirichletParams.py:19-26): vecs (4 n) = [diagonal of d Lam | diagonal of Hgg |
 * scale | diag_add], consts (2 (K + 1)) = [constant of d Lam per Dirichlet | constant of Hgg per Dirichlet]
 * (Dirichlet 0 = the K mixture weights at indices 0 .. K-1, Dirichlet 1 + k = column k of the (V, K) array at
 * indices K + v K + k).  Uses the operand the last lrvb_mixture_rows / lrvb_mixture_stats call left on the device;
 * the result stays on the device for lrvb_chol_factor_last, H_out may be NULL.                                      */
int lrvb_mixture_schur_dirichlet(lrvb_ctx* ctx, int32_t K, int32_t q, const double* vecs, const double* consts, double* H_out);

/* Gram matrix G^T G (D x D, free coordinates) of the per-observation gradients
 * g_n[k] = 1/2 z_n^T M_k z_n + c_k (K = V matrices, one per vector coordinate, not necessarily symmetric): the Kronecker
 * rows -- the packed lower triangle of z_n z_n^T, q (q + 1) / 2 virtual columns, the matrices folded onto it -- are generated
 * on chip and contracted on the fp64 matrix cores; G (N x D) is never materialised (BASELINE.json config 5).  n_cols <= 64. */
int lrvb_quadform_gram(lrvb_ctx* ctx, const double* M, const double* c, int64_t K,
                       const double* free_in, double* GtG_out, int64_t ld);
/* The same Gram matrix for the Wishart + MVN model (BASELINE.json configuration 5: y_n ~ N(mu, Lambda^-1), q(mu) = MVNParam(d),
 * q(Lambda) = WishartParam(d); LRVB/NormalParams.py:6-23, WishartParams.py:6-35) with the V matrices M_k described by
 * (nu, m, V) alone: they are 0.2 % dense (64 entries per mean coordinate, four per coordinate of V, one dense matrix for nu) and
 * enter the contraction as gathers -- the 8 V (d + 1)^2-byte operand (134 MB at d = 63) is never formed, on either side of PCIe --
 * and with GtG_out == NULL the result stays in HBM as well (lrvb_chol_factor_last factors it; a sharded step then moves
 * nothing over PCIe but c and theta).
 * offsets = vector-coordinate positions of [mean of q(mu), vech(information of q(mu)), nu, vech(V)]; v is d x d row-major;
 * cvec (V) the constants c_k of the per-observation gradient, as for lrvb_quadform_gram.                                  */
int lrvb_wishart_gram(lrvb_ctx* ctx, int64_t d, const int64_t* offsets, double nu, const double* m, const double* v,
                      const double* cvec, const double* free_in, double* GtG_out, int64_t ld);
/* The Kronecker SYRK behind both on its own: K4 = sum_n c_n u_n u_n^T (Pv x Pv, Pv = n_cols (n_cols + 1) / 2, leading dimension
 * ld >= Pv, both triangles), u_n the packed lower triangle of z_n z_n^T (column a (a + 1) / 2 + b <-> z_na z_nb, b <= a), z the
 * context's data matrix.  cvec: n_obs weights, NULL = ones.  Rank-local (no sum over ranks); n_cols <= 64.  The split of the
 * observation axis is the kernel's own (lrvb_set_tuning does not reach it).                                                  */
int lrvb_kron_gram(lrvb_ctx* ctx, const double* cvec /*n_obs entries, NULL = ones*/, double* K4_out, int64_t ld);
/* C = A^T diag(c) B over N rows from host operands (row-major; cvec NULL = ones), on the two-operand matrix-core kernel the
 * models use, whatever the shape (no dispatch to the small-product kernels).  The context only lends its stream and scratch.
 *   mode 0  A (N x PA), B (N x PB), PA and PB even; C is PA x PB.
 *   mode 1  the same with 16 zero rows kept behind both operands on the device: at PA = PB = 528 the 16-column slivers ride on
 *           the 16 interior workgroups and the edge entries are sums of four k-quarters.
 *   mode 2  A is the N x 31 matrix x (PA = 31), B is N x 528: C (528 x 528) = sum_n c_n tri([1, x_n][1, x_n]^T) B[n, :], the
 *           left operand (the packed lower triangle, column a (a + 1) / 2 + b) generated on chip.
 * Odd widths, a mode-2 shape other than (31, 528) and N < 1 are errors (LRVB_ERR_UNSUPPORTED / LRVB_ERR_SIZE).              */
int lrvb_weighted_atb(lrvb_ctx* ctx, const double* A, int64_t PA, const double* B, int64_t PB, int64_t N,
                      const double* cvec /*nullable*/, int32_t mode, double* C_out);

/* ---- linear-response solve ------------------------------------------------------------ */
/* scipy.linalg.cho_factor at LRVB/ModelSensitivity.py:594 / SparseObjectives.py:539.
 * The factor stays on the device inside the context.  Only the lower triangle of H (row-major, j <= i) is read: whatever
 * lies above the diagonal -- NaN included -- has no effect, which is what lrvb_chol_factor_last relies on for resident
 * Hessians whose builders write lower tiles only.  A pivot that is not a positive finite number (<= 0, NaN, +Inf) fails with
 * LRVB_ERR_NOT_POSDEF and its 1-based position; after a failed call the context holds no factor.  */
int lrvb_chol_factor(lrvb_ctx* ctx, const double* H, int64_t D);
/* Factor the Hessian the context last built on the device (no host round trip).            */
int lrvb_chol_factor_last(lrvb_ctx* ctx);
/* scipy.linalg.cho_solve at LRVB/ModelSensitivity.py:600-602: X = H^{-1} B, B is D x nrhs   */
int lrvb_chol_solve (lrvb_ctx* ctx, const double* B, int64_t D, int64_t nrhs, double* X_out);
/* Device-resident forms (H_dev has leading dimension ld; B_dev is D x nrhs, overwritten
 * with the solution; cov_dev is Q x Q).                                                     */
int lrvb_chol_factor_dev(lrvb_ctx* ctx, const double* H_dev, int64_t D, int64_t ld);
int lrvb_chol_solve_dev (lrvb_ctx* ctx, double* B_dev, int64_t D, int64_t nrhs);
int lrvb_lrvb_cov_dev   (lrvb_ctx* ctx, const double* M_dev, int64_t Q, int64_t D, double* cov_dev);
/* LRVB covariance M H^{-1} M^T (Q x Q) for a moment Jacobian M (Q x D)
 * (Example.ipynb:398-415; LRVB/SparseObjectives.py:541-558)                                 */
int lrvb_lrvb_cov   (lrvb_ctx* ctx, const double* M, int64_t Q, int64_t D, double* cov_out);
/* ConjugateGradientSolver.get_hinv_vec (LRVB/ConjugateGradient.py:81-85): solves
 * H(theta) x = b by CG on device HVPs.  Stopping rule of scipy cg with tol (legacy) =
 * rtol, atol = 0: ||b - Hx|| <= tol*||b||; x0 NULL = zeros; Minv NULL = no preconditioner
 * (else a dense D x D approximate inverse, applied as z = Minv r); maxiter <= 0 = 10*D.
 * info_out: 0 converged, >0 = iterations at which it stopped unconverged (scipy's code).    */
int lrvb_cg_solve(lrvb_ctx* ctx, const double* free_in, const double* b, const double* x0,
                  const double* Minv, double tol, int64_t maxiter, int64_t D,
                  double* x_out, int* info_out, int64_t* iters_out);
/* Blocked variant: Q right-hand sides (rows of B, Q x D row-major) advance in lockstep -- the loop over
 * masks of ConjugateGradientSolver.get_hinv_vec_subsets (LRVB/ConjugateGradient.py:87-105) -- so that the
 * Q Hessian-vector products of an iteration share one pair of passes over the observations.  Each row
 * follows exactly the recurrence and stopping rule of lrvb_cg_solve; info_out / iters_out have Q entries. */
int lrvb_cg_solve_multi(lrvb_ctx* ctx, const double* free_in, const double* B, const double* X0 /*nullable*/,
                        const double* Minv /*nullable D x D*/, double tol, int64_t maxiter, int64_t D, int64_t Q,
                        double* X_out, int* info_out, int64_t* iters_out);
/* The block product of lrvb_cg_solve_multi on its own: row q of out (Q x D) = H(theta) Vb[q], computed exactly as the
 * warm-start product of that solver (the fused multi-vector pass 16 rows at a time; the two-GEMM route with tuning bit 0,
 * four waves per workgroup with bit 2; the resident Hessian of this point when there is one and bit 3 is clear).  Any
 * Q >= 1.  Keeps and reuses the point state like the solvers.                                 */
int lrvb_hvp_multi(lrvb_ctx* ctx, const double* free_in, int64_t D, const double* Vb, int64_t Q, double* out);

/* The same conjugate-gradient loop on a dense symmetric D x D matrix kept on the device (Hessians
 * assembled from sufficient statistics).  H == NULL reuses the matrix of the previous call.   */
int lrvb_cg_solve_matrix(lrvb_ctx* ctx, const double* H, const double* b, const double* x0,
                         const double* Minv, double tol, int64_t maxiter, int64_t D,
                         double* x_out, int* info_out, int64_t* iters_out);

/* ---- device-resident / multi-GPU entry points -----------------------------------------
 * Observations shard over ranks (one process, one context per GPU).  A build is
 *   lrvb_hessian_partial_dev  on every rank  -> stats buffer (this shard's sums)
 *   sum all-reduce of the stats buffer       (torch.distributed / RCCL, outside this lib)
 *   lrvb_hessian_finish_dev   on every rank  -> full free-coordinate Hessian
 * stats layout: [ value (1) | d f_data / d beta (n_cols) | tile-packed lower triangle of
 * X^T diag(w loss'') X (lrvb_stats_size - 1 - n_cols) ] -- sums over observations only; the
 * N-independent quadratic term is added by `finish` on every rank after the reduction.     */
int lrvb_stats_size(lrvb_ctx* ctx, int64_t* n_doubles);
int lrvb_hessian_partial_dev(lrvb_ctx* ctx, const double* free_dev, double* stats_dev);
int lrvb_hessian_finish_dev (lrvb_ctx* ctx, const double* free_dev, const double* stats_dev,
                             double* H_dev, int64_t ld);
/* Single-GPU convenience = partial + finish with everything resident.                      */
int lrvb_hessian_dev(lrvb_ctx* ctx, const double* free_dev, double* H_dev, int64_t ld);

/* Sum-over-ranks hook.  With a hook installed, every sum over observations that the declared-objective entry
 * points form -- [value | gradient] of lrvb_value / lrvb_grad (and their _vec forms), the product of lrvb_hvp /
 * lrvb_hvp_dev, the block products of lrvb_cg_solve_multi, the statistics buffer inside lrvb_hessian /
 * lrvb_hessian_dev, the tiles of lrvb_gram, every product inside lrvb_cg_solve, lrvb_minimize_trust_ncg and
 * lrvb_dk_grad_vec -- is handed to `fn(user, buf_dev, n, hip_stream)` BEFORE the N-independent terms (quadratic
 * term, packing second-order terms) are added.  `fn` must replace buf_dev[0 .. n) by its sum over all ranks, ordered
 * after the work already queued on `hip_stream` (the context's stream) and before whatever is queued on it next
 * -- e.g. an RCCL all-reduce launched on that stream -- and return 0.  Every rank then holds the global value,
 * gradient, product, Hessian and iterates, bit-identical, so the device CG / trust-region loops stay in lockstep
 * with one D-vector all-reduce per product; no counterpart in the reference, which is
 * single-process.  The statistics calls of the other model families are sums over observations too and go through
 * the hook the same way, EXACTLY ONCE PER CALL, on the device buffer, before anything is copied to the host:
 * lrvb_weighted_gram (S), lrvb_group_sums, lrvb_grouped_stats ([S | group sums]), lrvb_mixture_rows /
 * lrvb_mixture_stats ([S64 | val2 | count of indefinite rows | packed Schur operand]: every rank fails together when
 * any rank has an indefinite row), lrvb_quadform_gram ([K4 tiles | s | observation count]) and
 * lrvb_logitnormal_terms ([Hessian blocks | gradient | value], the part that was asked for), lrvb_glmm_terms and
 * lrvb_glmm_slopes_terms ([Hessian blocks | group sums | gradient | value]) and lrvb_glmm_group_influence / lrvb_glmm_slopes_group_influence (the G x Q result).  A call must therefore
 * be made by ALL ranks, with the same arguments apart from the rows they hold.  lrvb_hessian_partial_dev and the
 * per-observation row outputs (lrvb_obs_*, the gradient rows of lrvb_mixture_rows) stay rank-local by contract.
 * fn == NULL removes the hook.                                                                                */
typedef int (*lrvb_reduce_fn)(void* user, double* buf_dev, int64_t n, void* hip_stream);
int lrvb_set_reduce_hook(lrvb_ctx* ctx, lrvb_reduce_fn fn, void* user);

/* In-library collective (lrvb_comm_init / lrvb_allreduce_hessian), one process per GPU:
 * rank 0 obtains an id with lrvb_comm_unique_id and hands the 128 bytes to the other ranks by any channel; every rank
 * calls lrvb_comm_init(ctx, world_size, rank, &id) (collective: returns when all ranks have joined), which creates its
 * rank of ONE RCCL communicator on the context's device and installs it as the sum-over-ranks hook above (in-place
 * ncclAllReduce of doubles on the context's stream, RCCL over xGMI).  lrvb_allreduce_hessian sums a statistics buffer
 * of lrvb_hessian_partial_dev explicitly.  librccl is loaded at run time (dlopen), not linked.                     */
typedef struct lrvb_comm_id { char bytes[128]; } lrvb_comm_id;
int lrvb_comm_unique_id(lrvb_comm_id* id_out);
int lrvb_comm_init(lrvb_ctx* ctx, int world_size, int rank, const lrvb_comm_id* id);
int lrvb_comm_destroy(lrvb_ctx* ctx);
int lrvb_allreduce_hessian(lrvb_ctx* ctx, double* stats_dev, int64_t n_doubles);
int lrvb_hvp_dev    (lrvb_ctx* ctx, const double* free_dev, const double* v_dev, double* out_dev);
int lrvb_gram_dev   (lrvb_ctx* ctx, const double* free_dev, double* GtG_dev, int64_t ld);

/* ---- profiling (bench.py's roofline.achieved) ------------------------------------------ */
/* D^j g [u_1 .. u_j]: the j-th directional derivative of the vector-coordinate gradient g = d f / d eta along the
 * rows of U (j x V, row-major; j = `order` in 0..6, j = 0 returns g itself).  The reference's higher-order
 * sensitivity (`ParametricSensitivityTaylorExpansion`, LRVB/ModelSensitivity.py:382-515) builds this from j nested
 * autograd JVPs of the gradient closure (`append_jvp`, :38-62; `generate_two_term_derivative_array`, :221-234).
 * w_override (N, nullable): evaluate with these observation weights instead of the context's -- the derivative
 * of g along a direction in WEIGHT space, since the objective is linear in the weights; include_quad = 0
 * drops the N-independent quadratic term (it does not depend on the weights).  All host pointers.          */
int lrvb_dk_grad_vec(lrvb_ctx* ctx, const double* vec_in, int64_t V, int32_t order, const double* U,
                     const double* w_override, int32_t include_quad, double* out);

/* Trust-region Newton-CG minimisation of the objective in free coordinates, entirely on the device: the
 * optimiser `minimize_objective_trust_ncg` (LRVB/OptimizationUtils.py:44-75) hands to
 * scipy.optimize.minimize(method='trust-ncg') with fun_free / fun_free_grad / fun_free_hvp -- or, with a
 * preconditioner, the `_cond` family (LRVB/SparseObjectives.py:202-240: f(A y), A^T g, A^T H A v).  Same
 * algorithm and constants (Steihaug-Toint CG subproblem; eta, radius rules), so the iterates agree with the
 * scipy route to rounding, but no host callback per Hessian-vector product and ONE curvature pass per point.
 * y0, y_out: iterate in the optimiser's coordinates (x = A y; A = `precond`, D x D row-major, nullable = identity);
 * x_out (nullable): the minimiser in free coordinates.  maxiter <= 0 -> 200 D (scipy's default).
 * status: 0 = ||gradient|| < gtol, 1 = maxiter reached, 2 = the quadratic model predicted no decrease.       */
typedef struct lrvb_opt_result {
    double  fun;             /* objective at the returned point                      */
    double  jac_mag;         /* 2-norm of the (preconditioned) gradient there        */
    double  trust_radius;    /* final radius                                         */
    int32_t status, nit;     /* see above; outer iterations                          */
    int32_t nfev, njev, nhev;/* value / gradient / Hessian-vector evaluations        */
    int32_t nbuild;          /* Hessians built inside the CG runs (256 <= D <= 8192, models with a data term): after
                                max(8, D / 64) products at one point the point's Hessian is built (about D / 86 passes over
                                the observations) and the remaining products of the run are D x D matrix-vector products;
                                0 under tuning bit 3.  (Occupies what was tail padding: the struct size is unchanged.)   */
} lrvb_opt_result;
int lrvb_minimize_trust_ncg(lrvb_ctx* ctx, const double* y0, int64_t D, const double* precond,
                            double gtol, int64_t maxiter, double initial_trust_radius,
                            double max_trust_radius, double eta,
                            double* y_out, double* x_out, lrvb_opt_result* res);

typedef struct lrvb_prof {
    double  wsyrk_ms;       /* HIP-event time of the weighted-SYRK kernel, summed           */
    int64_t wsyrk_calls;
    double  wsyrk_flops;    /* algorithmic flops per launch: n_obs * n_cols * (n_cols + 1)   */
    double  wsyrk_bytes;    /* algorithmic bytes per launch: 8*(n_obs*(n_cols+1)) + tri      */
    double  pass_ms;        /* HIP-event time of the fused value/grad/curvature pass         */
    int64_t pass_calls;
    double  pass_bytes;     /* 8 * n_obs * (n_cols + 3)                                       */
    double  build_ms;       /* whole lrvb_hessian_dev calls                                  */
    int64_t build_calls;
    double  reduce_ms;      /* HIP-event time around the sum-over-ranks hook (the exchange step of SURVEY 8(e)): the
                               collective itself plus, on its first use in a step, the wait for the slowest rank   */
    int64_t reduce_calls;
} lrvb_prof;
int lrvb_profile_enable(lrvb_ctx* ctx, int on);   /* off by default (event overhead)        */
int lrvb_profile_get   (lrvb_ctx* ctx, lrvb_prof* out);
int lrvb_profile_reset (lrvb_ctx* ctx);
/* Tuning knobs: number of row splits of the weighted-SYRK grid (0 = automatic); `reserved` bit 0 =
 * always use the register-staged SYRK kernel, bit 1 = mixture rows always take the dense per-row
 * factorisation, bit 2 = the fused multi-vector pass (blocked CG, streamed influence) with four
 * waves per workgroup instead of eight, bit 3 = never use the resident Hessian (below): products are always passes over
 * the observations.  Every setting computes the same results by another code path
 * (they exist so that tests can compare the paths); any other bit of `reserved` is LRVB_ERR_INVALID.
 *
 * THE RESIDENT HESSIAN.  Every free-coordinate build (lrvb_hessian, lrvb_hessian_dev, lrvb_hessian_finish_dev) leaves a copy
 * of its result inside the context.  lrvb_hvp, lrvb_cg_solve and lrvb_cg_solve_multi asked for the SAME point afterwards form
 * their products H v from that matrix (a D x D product, identical on every rank, no pass over X and no reduction) -- the
 * reference's ConjugateGradientSolver is used exactly so: fun_free_hessian / fun_free_hvp at one optimum, many right-hand
 * sides (LRVB/ConjugateGradient.py:63-105).  The copy is dropped by lrvb_set_data(_dev), lrvb_set_weights(_dev),
 * lrvb_set_quad_scale (new value), lrvb_set_lik_info, lrvb_set_reduce_hook and lrvb_comm_init / _destroy;
 * buffers adopted with the `_dev` setters must be installed again after their contents change.
 * A long run of products at ONE point builds the matrix by itself: past max(8, D / 64) matrix-free products at the point
 * lrvb_hvp / lrvb_cg_solve last named (256 <= D <= 8192, models with a data term) the point's Hessian is built -- about
 * D / 86 passes over the observations -- and made resident; lrvb_minimize_trust_ncg does the same inside its CG runs
 * (lrvb_opt_result.nbuild).  Tuning bit 3 switches both off.                                                            */
int lrvb_set_tuning(lrvb_ctx* ctx, int n_splits, int reserved);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* LRVB_HIP_H */

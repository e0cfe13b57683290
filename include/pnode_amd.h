/*
 * pnode_amd -- C ABI of the MI355X-native explicit-RK time stepper + discrete-adjoint engine.
 *
 * This is the drop-in boundary for the hot path of caidao22/pnode
 * (reference: pnode/petsc_adjoint.py, "pa.py" below).  The reference has no FFI of its own on
 * this path: it binds PETSc's TS / TSAdjoint / TSTrajectory / Vec through petsc4py.  Every
 * entry point below therefore names the petsc4py call (pa.py file:line) or the PETSc routine
 * behind it that it replaces.  Plain pointers, sizes and scalars only -- no torch types.
 *
 * Groups (sections 1-5 below; 5 = the disk tier of the trajectory, added in round 2):
 *   1. device entry points (pn_rk_*, pn_adj_*, pn_param_accum, ...): enqueue ONE hand-written
 *      gfx950 kernel on the caller's HIP stream over raw device pointers.  They replace the
 *      PETSc Vec-op sequences (VecCopy + VecMAXPY + VecScale + VecAXPY + norms) that
 *      TSStep_RK / TSAdjointStep_RK / TSAdaptChoose issue per stage.
 *   2. host entry points (pn_ts_*, pn_traj_*, pn_tableau_*): the time-stepper state machine --
 *      tableau, step-size controller, exact-final-time / time-span matching, checkpoint
 *      scheduler.  No GPU needed; unit-testable on a CPU-only box.
 *
 * The callback into the user's dynamics f(t,u) stays on the host side above this ABI (it is a
 * Python nn.Module, pa.py:393-412), exactly where petsc4py's callback shells sit.
 *
 * All functions return 0 on success, non-zero on failure; pn_last_error() describes the last
 * failure on the calling thread.
 */
#ifndef PNODE_AMD_H
#define PNODE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN_MAX_STAGES 7      /* 5dp has 7 stages */
#define PN_MAX_TERMS 8       /* most vectors one kernel combines (lambda + 6 dlambda + forcing) */
#define PN_WGRAD_MAX_PAIRS 8  /* most (cotangent, input) pairs one pn_linear_wgrad_group launch takes */
#define PN_WGRAD_EXACT_FP32 1 /* pn_linear_wgrad_group flag: fp32 states on v_mfma_f32_32x32x2_f32 instead of the split-bf16 form */
#define PN_WGRAD_TILE_64 2    /* pn_linear_wgrad_group flag: always the 64 x 64 workgroup tile (the same bits as the 128 x 128 one a
                                 launch over whole rounds of the chip takes by itself: for comparisons) */
#define PN_ABI_VERSION 4      /* 2 (round 3): pn_rk_combine_wrms writes per-workgroup partials into a pinned BLOCK (pn_wrms_partials)
                                 and pn_stream_wait_wrms finishes the norm; work areas of the reductions are zero-filled once;
                                 pn_krylov_* added.  3 (round 4): the step loops pn_rk_attempt / pn_rk_adjoint_step (section 3a).
                                 4 (round 6): pn_kernel_id grew (PN_K_LINEAR_WGRAD, added in round 5 without a version change) and
                                 pn_prof_collect now takes the caller's array length; pn_colsum_*, pn_linear_wgrad* entered the
                                 ABI; pn_linear_wgrad_work_bytes takes the dtype; pn_linear_wgrad_group added; fp64 form of the
                                 fused kernel.  A client built against version 3 must not call this library: pn_abi_version()
                                 is how it finds out. */

typedef enum { PN_F32 = 0, PN_F64 = 1 } pn_dtype;

const char *pn_last_error(void);
int pn_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * 1. Tableaus.  Replaces ts.setRKType(...) (pa.py:641-650) / -ts_rk_type.
 *    Names: PETSc's "1fe" "2a" "2b" "3" "3bs" "4" "5f" "5dp", plus "midpoint" (extension).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int s;            /* stages */
  int order;        /* order of the propagated solution (exponent of the controller) */
  int fsal;         /* last stage == next step's first stage */
  int has_embed;    /* has an embedded lower-order solution (adaptive-capable) */
  double A[PN_MAX_STAGES][PN_MAX_STAGES];
  double b[PN_MAX_STAGES], bembed[PN_MAX_STAGES], c[PN_MAX_STAGES];
} pn_tableau;

int pn_tableau_get(const char *rk_type, pn_tableau *out);
/* pa.py:641-650: euler->1fe rk2->2b bosh3|fixed_bosh3->3bs rk4->4 dopri5|fixed_dopri5->5dp;
 * any other string -> PETSc's default "3bs".  Returns the rk type name (static storage). */
const char *pn_method_to_rk_type(const char *method);

/* Continuous extension (dense output) of a tableau, for -pn_output_times interpolate (extension: PETSc's TSInterpolate
 * for RK is not what the reference reaches; its time span forces a step onto every output time instead):
 *   y(t_n + theta*h) = y_n + h * sum_j beta_j(theta) K_j,   beta_j(theta) = sum_{p < npow} P[j][p] theta^(p+1).
 * Built for "3bs" (Bogacki-Shampine cubic, order 3), "4" (RK4's cubic, order 3) and "5dp" (Shampine's quartic, order 4);
 * any other type fails with a message naming those three.  *order: the order of the extension. */
#define PN_DENSE_MAX_POW 4
int pn_tableau_dense(const char *rk_type, int *order, int *npow, double P[PN_MAX_STAGES][PN_DENSE_MAX_POW]);

/* ------------------------------------------------------------------------------------------
 * 2. Device entry points.  `stream` is a hipStream_t.  `dtype` selects f32/f64 storage;
 *    coefficients are passed in double and rounded once to the storage type, as PETSc forms
 *    w[j] = h*A[i][j] in PetscReal before VecMAXPY.  All vectors have `n` elements.
 *    Zero coefficients must be dropped by the caller (nk counts the non-zeros).
 * ---------------------------------------------------------------------------------------- */

/* Y = u + sum_{j<nk} coef[j]*K[j]      (coef[j] = h*a_ij or h*b_j)
 * Replaces TSStep_RK's per-stage VecCopy(vec_sol,Y[i]) + VecMAXPY(Y[i],i,w,YdotRHS) and the
 * final VecMAXPY of TSEvaluateStep_RK, driven by ts.solve (pa.py:829). */
int pn_rk_stage(void *stream, int dtype, int64_t n, void *y, const void *u,
                int nk, const void *const *K, const double *coef);

/* Embedded error estimate, fused with the solution update:
 *   unew = u + sum coef_b[j]*K[j]      (written to `unew` unless unew == NULL; with
 *                                       unew == NULL `u` already IS the new solution -- FSAL)
 *   err  = sum coef_e[j]*K[j]          (coef_e[j] = h*(bembed_j - b_j))
 *   partial sums of (err / (atol + rtol*max(|unew|,|unew+err|)))^2 -> *result_dev =
 *   sqrt(sum/n)   [TSErrorWeightedNorm, NORM_2]   (also NaN/Inf if any element is).
 * Replaces TSEvaluateStep_RK(order-1) + TSErrorWeightedNorm inside TSAdaptChoose_Basic
 * (selected by ts.setFromOptions, pa.py:775).  ONE launch.  The norm is finished on the host, which has to wait for the
 * stream before it can judge the step anyway: every workgroup stores its partial sum into `result_dev` -- the device
 * pointer of a pn_pinned_block() of pn_wrms_partials(n) doubles -- and pn_stream_wait_wrms() adds them in index order
 * (bit-reproducible) and returns sqrt(sum/n).  `work`: pn_wrms_work_bytes(n) bytes of device memory, ZERO-FILLED once
 * before first use (arrival counters of the in-launch finish, PN_TUNE "wfin=1"; untouched otherwise); one work area and
 * one result block per stream. */
int pn_rk_combine_wrms(void *stream, int dtype, int64_t n, void *unew, const void *u,
                       int nk, const void *const *K, const double *coef_b, const double *coef_e,
                       double atol, double rtol, void *work, double *result_dev);
int64_t pn_wrms_work_bytes(int64_t n);
int64_t pn_wrms_partials(int64_t n);
/* Blocks until everything enqueued on `stream` is done, then finishes the norm from the host side of the pinned block
 * pn_rk_combine_wrms wrote.  The one host<->device synchronisation of an adaptive step. */
int pn_stream_wait_wrms(void *stream, const double *result_host, int64_t n, double *value);
/* pn_rk_combine_wrms under -ts_adapt_wnormtype infinity: the same update, the same err, the same launch geometry, and
 *   max_i |unew_i - uhat_i| / (atol + rtol*max(|unew_i|,|uhat_i|))   [TSErrorWeightedNorm, NORM_INFINITY]
 * (uhat = unew + err rounded to the storage type; fp32 states form the ratio in fp32, fp64 ones in double; no square is
 * taken).  A NaN term makes the norm NaN and an infinite one +inf: every level of the reduction carries NaN explicitly, since
 * the hardware's max returns the operand that is not NaN.  Replaces TSEvaluateStep_RK(order-1) + TSErrorWeightedNorm with
 * wnormtype NORM_INFINITY inside TSAdaptChoose_Basic (ts.setFromOptions, pa.py:775, reading -ts_adapt_wnormtype).  Same
 * signature as pn_rk_combine_wrms, so that it can stand in pn_vec_ops.rk_combine_wrms; `work` as there (untouched);
 * every workgroup stores the largest of its terms into the pinned block and pn_stream_wait_winf() takes the largest of
 * those.  Profiled as PN_K_COMBINE_WRMS. */
int pn_rk_combine_winf(void *stream, int dtype, int64_t n, void *unew, const void *u,
                       int nk, const void *const *K, const double *coef_b, const double *coef_e,
                       double atol, double rtol, void *work, double *result_dev);
/* pn_stream_wait_wrms for the block pn_rk_combine_winf wrote: waits for `stream`, then pn_winf_finish. */
int pn_stream_wait_winf(void *stream, const double *result_host, int64_t n, double *value);
/* The host half alone (no device): the largest of the per-workgroup partials of `block` (block[0] = their number), NaN if
 * any is NaN; 0.0 when every term was zero. */
int pn_winf_finish(const double *block, int64_t n, double *value);
/* pn_rk_combine_wrms / pn_rk_combine_winf with a tolerance per component (PETSc's TSSetTolerances(ts, atol, vatol, rtol, vrtol)
 * with vectors, petsc4py's ts.setTolerances(rtol=Vec, atol=Vec) on the ode.ts a user of the reference holds, pa.py:370): the
 * same arguments with `double atol, double rtol` replaced by two device vectors of `period` doubles and the period; element e
 * of the flattened state uses entry e % period, i.e.
 *   tol_e = vatol[e % period] + vrtol[e % period]*max(|unew_e|,|uhat_e|)
 * and everything else -- update, err, the storage-type rounding of uhat, the fp32 form of the ratio, launch geometry, pinned
 * partial block, finish (pn_stream_wait_wrms / pn_stream_wait_winf) and NaN/Inf propagation -- is the scalar entry point's:
 * vectors filled with one value give its norm and its unew bit for bit.  period must divide n (period == n: one entry per
 * element; period == n / B: one per component of a sample, repeated over the batch).  The vectors are only read.  They do
 * not fit pn_vec_ops.rk_combine_wrms (two scalars), so the native step loop does not reach them: a caller walks the tableau
 * itself (pn_rk_stage ... pn_rk_combine_wrms_v).  Profiled as PN_K_COMBINE_WRMS. */
int pn_rk_combine_wrms_v(void *stream, int dtype, int64_t n, void *unew, const void *u,
                         int nk, const void *const *K, const double *coef_b, const double *coef_e,
                         const double *vatol, const double *vrtol, int64_t period, void *work, double *result_dev);
int pn_rk_combine_winf_v(void *stream, int dtype, int64_t n, void *unew, const void *u,
                         int nk, const void *const *K, const double *coef_b, const double *coef_e,
                         const double *vatol, const double *vrtol, int64_t period, void *work, double *result_dev);
/* A stream of the caller's own on the current device: priority > 0 the device's LOWEST priority (background work: the
 * weight-sensitivity products that run beside the reverse sweep's critical chain), < 0 the highest, 0 the default.  Not a
 * replacement of anything in the reference (PETSc's Vec operations run on one stream). */
int pn_stream_create(int priority, void **stream);
int pn_stream_destroy(void *stream);
/* Blocks until everything enqueued on `stream` is done and returns *host_ptr (a pinned, device-visible double). */
int pn_pinned_scalar(double **host_ptr, double **dev_ptr);
int pn_pinned_free(double *host_ptr);
/* the same for a block of `nbytes` (e.g. all Hessenberg entries of one GMRES iteration) */
int pn_pinned_block(int64_t nbytes, double **host_ptr, double **dev_ptr);
int pn_stream_wait_scalar(void *stream, const double *host_ptr, double *value);

/* Adjoint stage cotangent:  w = c_lam*lambda + sum_{j<nk} coef[j]*dlam[j]
 *   with c_lam = H*b_i (lambda == NULL when b_i == 0) and coef[j] = H*a_ji.
 * Replaces TSAdjointStep_RK's VecCopy/VecSet + VecMAXPY into VecsSensiTemp and the VecScale of
 * the transposed-Jacobian product (the scale is folded into the cotangent), pa.py:875-878. */
int pn_adj_theta(void *stream, int dtype, int64_t n, void *w, const void *lambda, double c_lam,
                 int nk, const void *const *dlam, const double *coef);

/* lambda_out = lambda + sum_{j<nk} coef[j]*dlam[j] (+ forcing)     (coef == NULL: all ones)
 * and, optionally fused, a scaled copy  w_next = c_next*lambda_out  (skipped when w_next == NULL).
 * coef[j] carries a scalar that was not applied to a stage cotangent: a stage whose cotangent
 * is a pure multiple of lambda (H*b_i*lambda) is differentiated with lambda itself as the
 * cotangent and the factor H*b_i is folded into the consumers of its result.
 * Replaces the closing VecMAXPY of TSAdjointStep_RK and adj_u_tensor.add_(grad_output[i-1])
 * (pa.py:938). */
int pn_adj_accum(void *stream, int dtype, int64_t n, void *lambda_out, const void *lambda,
                 int nk, const void *const *dlam, const double *coef, const void *forcing,
                 void *w_next, double c_next);

/* mu[off_k : off_k+len_k] += alpha*g_k for every parameter tensor k (g_k == NULL: skipped).
 * Replaces RHSJacPShell.multTranspose's flatten+copy (pa.py:341-363, misc.py:9-14) and
 * TSAdjointStep_RK's VecScale + VecAXPY on the parameter sensitivities. */
int pn_param_accum(void *stream, int dtype, void *mu, double alpha, int nseg, const void *const *g,
                   const int64_t *offset, const int64_t *len);

/* The parameter sensitivities of all stages of one time step in ONE launch:
 *   mu[off_k + e] <- fma(alpha_{S-1}, g_{S-1,k}[e], ... fma(alpha_0, g_{0,k}[e], mu[off_k + e]))
 * for nsrc = S <= 32 gradient sets (the stages of one or of SEVERAL time steps), g[j*nseg + k] = set j's
 * gradient of parameter tensor k (NULL: skipped).  Rounding is that of S successive pn_param_accum calls
 * in the order j = 0..S-1 (results are bit-identical to them); mu is read and written once instead of S
 * times.  Replaces the per-stage VecAXPY on the parameter sensitivities inside TSAdjointStep_RK. */
int pn_param_accum_multi(void *stream, int dtype, void *mu, int nsrc, const double *alpha, int nseg,
                         const void *const *g, const int64_t *offset, const int64_t *len);

/* For up to 32 sources j:  mu[j][c] += alpha[j] * sum_r g[j][r*cols[j] + c]  for c < cols[j] -- the parameter sensitivities of
 * BIASES: the column sum of the cotangent at the output of a Linear layer, added to the bias's slice of mu; the sources are the
 * layers and stages of one or of several time steps (several sources may name the same mu: they are added in source order).
 * Every g is read once, in one pass (per-lane sums in double; partials added in a fixed association: bit-reproducible, no
 * atomics, independent of how sources are grouped into calls).  Replaces, for the bias parameters of func's nn.Linear layers,
 * the `sum` inside autograd's backward plus RHSJacPShell.multTranspose's flatten/copy (pa.py:341-363, misc.py:9-14) plus the
 * VecAXPY on mu inside TSAdjointStep_RK.  `work`: pn_colsum_work_bytes(nsrc, rows, cols) bytes, no initialisation needed.
 * pn_colsum_accum is the one-source form. */
int pn_colsum_accum_multi(void *stream, int dtype, int nsrc, const int64_t *rows, const int64_t *cols, const void *const *g,
                          void *const *mu, const double *alpha, void *work);
int64_t pn_colsum_work_bytes(int nsrc, const int64_t *rows, const int64_t *cols);
int pn_colsum_accum(void *stream, int dtype, int64_t rows, int64_t cols, const void *g, void *mu, double alpha, void *work);

/* The parameter sensitivities of a Linear layer `out = x W^T + b`, fused (csrc/pn_linear.hip; MFMA -- v_mfma_f32_32x32x2_f32, exact
 * fp32, or v_mfma_f64_16x16x4_f64 --, K split over the 8 XCDs, 64 x 64 output tiles):
 *   pw[s][m][n]    += sum_{k in K-range s} (alpha g[k][m]) x[k][n]                                              s = 0..7
 *   pb[s][j][m]    += sum_{k in the slabs of K-range s that tile column j adds up} alpha g[k][m]                j = 0..in_f/64-1
 * for g = the cotangent at the layer's output (rows x out_f) and x = the layer's input (rows x in_f), both row-major and 16-byte
 * aligned.  pw (elements of the state's dtype) / pb (always doubles; the workgroups of a tile row share the column sums of g between
 * them, hence the index j) are partial buffers of pn_linear_wgrad_work_bytes() bytes that the CALLER zero-fills once; they carry the
 * sum over the stages and time steps of a reverse sweep (each launch adds its tile to them: no separate accumulation pass), and
 * pn_linear_wgrad_finish adds them to the parameter's slices of mu (mu_w[m][n] += sum_s pw[s][m][n], s in order; mu_b[m] += sum_{s,j}
 * pb[s][j][m], in index order) and zero-fills them again.  pb / mu_b may be NULL (layer without bias).  Bit-reproducible, and the
 * same bits whether pairs go through pn_linear_wgrad one by one or through pn_linear_wgrad_group.  Replaces, for func's nn.Linear
 * layers, autograd's weight- and bias-gradient kernels, RHSJacPShell.multTranspose's flatten/copy (pa.py:341-363, misc.py:9-14)
 * and the VecAXPY on mu inside TSAdjointStep_RK.  pn_linear_wgrad_supported: fp32 or fp64, rows >= 256 (any number: eight K ranges of whole 32-row slabs, missing rows read as zeros),
 * out_f % 64 == 0, in_f % 64 == 0, out_f * in_f <= 2^22 (other shapes take the general path: a library GEMM accumulating into mu +
 * pn_colsum_accum_multi).
 * pn_linear_wgrad_group: the pairs of SEVERAL layers (1 <= npairs <= PN_WGRAD_MAX_PAIRS; shapes may differ, rows is common) in
 * ONE launch -- all Linear layers of one stage VJP: one launch boundary per stage, and the workgroups of the next pair start while
 * the previous pair drains.  No two pairs of a group may share pw or pb.
 * Arithmetic for fp32 states (flags = 0, also what pn_linear_wgrad uses): every operand is split EXACTLY into three bf16 terms
 * (hi + mid + lo = the fp32 value) and the six largest of the nine cross products -- each exact in fp32; what is dropped is below
 * 2^-23 |g x| -- are accumulated in fp32 on v_mfma_f32_32x32x16_bf16: the bf16 matrix pipe is 16 times as fast per product as the
 * fp32 one.  Error against float64 BELOW that of an fp32 fmaf chain (5.7e-8 against 1.0e-7 of sum |g x|, tools/mb_wgrad_bf16x3.hip);
 * an infinite operand gives NaN.  flags = PN_WGRAD_EXACT_FP32: v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fmaf chain per K range)
 * instead.  Either way bit-reproducible.  fp64 states: v_mfma_f64_16x16x4_f64.
 * Tiling of the split-bf16 form: 128 x 128 workgroup tiles (1024 threads, one workgroup per CU) when every layer's out_f and in_f
 * are multiples of 128 and the launch's tiles fill whole rounds of the chip, else 64 x 64 ones (512 threads); flags =
 * PN_WGRAD_TILE_64 keeps the latter.  The two give the same bits in pw and pb. */
typedef struct {
  const void *g, *x;         /* cotangent at the layer's output (rows x out_f), the layer's input (rows x in_f) */
  void *pw, *pb;             /* the layer's partial buffers (pb may be NULL) */
  double alpha;
  int64_t out_f, in_f;
} pn_wgrad_pair;
int pn_linear_wgrad_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f);
int64_t pn_linear_wgrad_work_bytes(int dtype, int64_t out_f, int64_t in_f, int64_t *bias_bytes);
int pn_linear_wgrad(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *x, double alpha,
                    void *pw, void *pb);
int pn_linear_wgrad_group(void *stream, int dtype, int64_t rows, int npairs, const pn_wgrad_pair *pairs, int flags);
int pn_linear_wgrad_finish(void *stream, int dtype, int64_t out_f, int64_t in_f, void *pw, void *pb, void *mu_w, void *mu_b);

/* The forward of a Linear layer with its activation in one launch (csrc/pn_linear.hip):  y = act(x w^T + b)  for x rows x in_f, w out_f x
 * in_f, b out_f values or NULL, y rows x out_f, all row-major fp32; act = PN_ACT_IDENTITY, PN_ACT_TANH (tanhf of the device library,
 * applied in fp32 to the biased sum: exactly +-1 once it saturates, NaN for NaN) or PN_ACT_RELU (of the biased sum z: z where z > 0, a
 * NaN stays that NaN, everything else -- -0 too -- is +0; so y under PN_ACT_RELU is relu of the y under PN_ACT_IDENTITY in the same
 * form, value for value) or PN_ACT_SIGMOID (y = 1 / (1 + expf(-z)) of the biased sum z in fp32: expf of the device library, one rounded
 * add, one correctly rounded division -- within 2.5 * 2^-24 of sigma of the y under PN_ACT_IDENTITY in the same form; never above 1,
 * exactly 1 from z >= 40 on, exactly +0 from z <= -110 on, in (0, 1] for |z| <= 80, NaN for NaN; not torch.sigmoid's bits) or
 * PN_ACT_GELU (exact GELU, approximate='none': y = 0.5f * z * (1.f + erff(z * 0.70710678f)) of the biased sum z in fp32, never contracted,
 * spelled once: the same bits of y in every form.  erff is the device library's, whose bound this file does not know: the error is
 * MEASURED, see pn_linear_fwd_pre below; y is exactly z from z >= 6 on and exactly -0 from z <= -6 on, NaN for NaN; not F.gelu's bits.
 * y alone is for evaluations nobody differentiates: GELU's derivative needs z, which pn_linear_fwd_pre writes beside y) or
 * PN_ACT_SOFTPLUS (nn.Softplus at beta 1, threshold 20, aten's formula: y = z > 20.f ? z : log1pf(expf(z)) of the biased sum z in fp32;
 * y == z above the threshold, an exact +0 once expf underflows (z <= -104), NaN for NaN) or PN_ACT_ELU (nn.ELU at alpha 1:
 * y = z > 0.f ? z : expm1f(z); z's bits where z > 0, -0 for -0, exactly -1 from z of about -17.4 down, NaN for NaN).  log1pf and expm1f
 * are the device library's, which states no bound: the error of both is MEASURED against float64 on the kernel's own z
 * (profiles/linear_softplus_elu.txt, tests/test_gpu_linear_softplus_elu.py) and held to the figure of F.softplus / F.elu on the same z
 * plus one unit of 2^-24, at most 4 * 2^-24 relative to y.  Both are spelled once: the same bits of y in every form; any other
 * act -- 3, 5, 6, 7, 9 ... 15, 17 ... too, which name nothing -- is refused, nothing launched.  The product is the split-bf16 one of pn_linear_wgrad
 * (three exact bf16 terms per operand, the six largest cross products, fp32 accumulation on v_mfma_f32_32x32x16_bf16; an infinite
 * operand gives NaN); one workgroup owns a 64 x 128 tile of y over all of in_f and writes it once: no atomics, no work buffers, the
 * same bits on every launch.  x, w, y non-NULL and 16-byte aligned, b 4-byte aligned; y shares no byte with x, w or b (other workgroups
 * still read them while a tile of y is stored): refused otherwise, nothing launched.  Replaces, inside the solver's own evaluations of
 * func (the body of evalRHSFunction, pa.py:393-412), the library GEMM and the elementwise kernel of an nn.Linear -> nn.Tanh pair.
 * pn_linear_fwd_supported: fp32, rows >= 256 (any number), out_f % 64 == 0, in_f % 32 == 0 and >= 64; everything else is the caller's to run
 * through the library. */
#define PN_ACT_IDENTITY 0
#define PN_ACT_TANH 1
#define PN_ACT_RELU 2
#define PN_ACT_SIGMOID 4 /* (3 names nothing and is refused) */
#define PN_ACT_GELU 8    /* (5 and 7 name nothing and are refused) */
#define PN_ACT_SOFTPLUS 16 /* beta 1, threshold 20 (6, 9 ... 15 name nothing and are refused) */
#define PN_ACT_ELU 32      /* alpha 1 (17 ... 31, 33 ... name nothing and are refused: the values are names, not bits to combine) */
int pn_linear_fwd_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f);
int pn_linear_fwd(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *x, const void *w, const void *b, int act,
                  void *y);
/* The K loop of pn_linear_fwd and pn_linear_bwd has two forms with the same bits in every output: the PIPELINED one (three LDS buffers,
 * two sets of fragment registers: the MFMAs of a slab run while the next slab's fragments are read and the one after it is split and
 * stored) that aligned shapes -- rows % 64 == 0, the output's columns % 128 == 0 and K % 64 == 0 -- take by themselves, and the PLAIN one,
 * which ragged shapes and an odd number of K slabs (K = 96, 160, ...) always take.  pn_linear_fwd_form / pn_linear_bwd_form are pn_linear_fwd / pn_linear_bwd with `flags`: 0, or
 * PN_LINEAR_FORM_PLAIN for the plain loop on an aligned shape too (for comparisons); any other bit is refused. */
#define PN_LINEAR_FORM_PLAIN 1
int pn_linear_fwd_form(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *x, const void *w, const void *b,
                       int act, void *y, int flags);
/* pn_linear_fwd_form with a SECOND output, the pre-activation:  z = x w^T + b  (rows x out_f, fp32) beside  y = act(z), for the pairs
 * whose derivative is a function of z and not of y (GELU: not monotonic, z cannot be had back from y).  The epilogue stores z at y's tile
 * positions under y's guards: one more 4-byte store per element, no scratch, no LDS beyond pn_linear_fwd's, no atomics.  z has the bits of
 * the y that PN_ACT_IDENTITY gives in the same form, and y the bits pn_linear_fwd_form gives for the same act, for every act (under
 * PN_ACT_IDENTITY z == y).  PN_ACT_GELU has no closed bound (the device library states none for erff); MEASURED on MI355X against float64
 * GELU of z, |z| < 6 (tools/mb_linear_gelu.py, tests/test_gpu_linear_gelu.py): |y - gelu(z)| at most 7.4 * 2^-24, at most 2.1 * 2^-24
 * max(1, |z|) -- the figures of fp32 F.gelu on the same z, digit for digit; absolute, because 1 + erff cancels for negative z: there
 * the error is small and the RELATIVE error is not bounded; y == z exactly for z >= 6, y == -0 for z <= -6 (erff is exactly +-1 from |z| of about 5.6 on), a NaN in a row
 * of x gives NaN in that row of y and of z and touches no other row.  z must be non-NULL (y alone: pn_linear_fwd_form), 16-byte aligned,
 * and share no byte with y, x, w or b; everything pn_linear_fwd_form refuses is refused here: nothing is launched, y and z are untouched.
 * Replaces, in the solver's evaluations of func that autograd will differentiate (the stage VJPs of the reverse sweep: the body of
 * RHSJacShell.multTranspose, petsc_adjoint.py:318-339), the library GEMM and the gelu kernel of an nn.Linear -> nn.GELU pair, whose
 * saved tensor is that z. */
int pn_linear_fwd_pre(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *x, const void *w, const void *b, int act,
                      void *y, void *z, int flags);

/* The backward of such a pair with respect to its input in one launch (csrc/pn_linear.hip): for g (the cotangent at the pair's output)
 * and a (the pair's output, tanh of the biased sum) rows x out_f, w out_f x in_f AS IT LIES (no transposed copy is read or kept: an
 * optimiser changes w in place between two replays of a captured sweep), all row-major fp32:
 *   gz[r][k] = g[r][k] (1 - a[r][k]^2)   rows x out_f, written once -- the cotangent pn_linear_wgrad consumes
 *   dx[r][n] = sum_k gz[r][k] w[k][n]     rows x in_f,  written once
 * gz is formed in fp32 (1 - a a may contract to an fma: not aten.tanh_backward bit for bit, within 3 * 2^-24 |g| of the exact value); the
 * product is the split-bf16 one of pn_linear_fwd on the same 64 x 128 tiles over all of out_f.  No atomics, no work buffers, the same bits
 * on every launch.  A NaN or Inf in g or a stays in its own rows of gz and dx; a == +-1 with finite g gives gz == 0; an infinite gz or w
 * gives NaN in the products it takes part in.  All five operands non-NULL and 16-byte aligned; gz and dx share no byte with each other
 * or with an input (other workgroups still read them): refused otherwise, nothing launched.  Replaces, in the reverse sweep's stage VJPs,
 * the tanh_backward kernel and the library GEMM of the pair.
 * pn_linear_bwd_supported: fp32, rows >= 256 (any number), out_f % 32 == 0 and >= 64, in_f % 64 == 0, the size limits of
 * pn_linear_fwd_supported. */
int pn_linear_bwd_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f);
int pn_linear_bwd(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *a, const void *w, void *gz,
                  void *dx);
int pn_linear_bwd_form(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *a, const void *w,
                       void *gz, void *dx, int flags);
/* pn_linear_bwd_form with the pair's activation as an argument: the shape rules (pn_linear_bwd_supported), the null, alignment and aliasing
 * refusals and the flags are pn_linear_bwd_form's.  act == PN_ACT_TANH launches exactly what pn_linear_bwd_form launches.
 * act == PN_ACT_RELU is the backward of an nn.Linear -> nn.ReLU pair, a its output:
 *   gz[r][k] = a[r][k] <= 0 ? +0 : g[r][k]      dx[r][n] = sum_k gz[r][k] w[k][n]
 * -- aten.threshold_backward(g, a, 0) bit for bit: a NaN in a lets g through, a == +0 or -0 gives +0, and no arithmetic touches g, so
 * every element of gz is g's bits or +0.  dx has the bits of pn_linear_dx fed that gz, in every form (the prologue sits in front of the
 * bare body's split, tile map and product order).  Replaces, in the reverse sweep's stage VJPs, the threshold_backward kernel and the
 * library GEMM of the pair (with -pn_linear_bare 1: threshold_backward and pn_linear_dx, which reads gz back).
 * act == PN_ACT_SIGMOID is the backward of an nn.Linear -> nn.Sigmoid pair, a its output:
 *   gz[r][k] = g[r][k] s,  s = fmaf(-a[r][k], a[r][k], a[r][k])      dx[r][n] = sum_k gz[r][k] w[k][n]
 * -- a (1 - a) in one fma, then ONE rounded product (never contracted into what follows), spelled the same in every form: two roundings,
 * within 2.5 * 2^-24 of |g a (1 - a)|, the same bits of gz in every form; not aten.sigmoid_backward bit for bit (three roundings there).
 * a == 0 or a == 1 with finite g gives gz == 0; a NaN in a or g stays in its own element of gz and its own row of dx; g = +-inf where s
 * is 0 gives NaN, as in aten.sigmoid_backward.  dx has the bits of pn_linear_dx fed that gz, in every form.  Replaces the
 * sigmoid_backward kernel and the library GEMM of the pair.
 * act == PN_ACT_GELU is the backward of an nn.Linear -> nn.GELU pair (approximate='none'); a is then the pair's PRE-activation z (what
 * pn_linear_fwd_pre wrote), not its output:
 *   gz[r][k] = g[r][k] d,  d = cdf + z pdf,  cdf = 0.5f * (1.f + erff(z * 0.70710678f)),  pdf = expf(-0.5f * z * z) * 0.3989423f
 * -- aten.gelu_backward's formula, never contracted, spelled once: the same bits of gz in every form.  Measured on MI355X against
 * float64 (tools/mb_linear_gelu.py): |gz - g d(z)| / |g| at most 3.2 * 2^-24 (aten.gelu_backward on the same operands: 3.1) -- absolute in
 * d, which crosses zero near z = -0.7518.  d is exactly 1
 * from z >= 6 on (gz == g); from z <= -6 down cdf is 0 and d = z pdf, below 4e-8 in size, an exact -0 once expf underflows; a NaN in a or g stays in its own element of gz and its own row of dx; g = +-inf
 * where d is 0 gives NaN, as in aten.gelu_backward.  dx has the bits of pn_linear_dx fed that gz, in every form.  Replaces the
 * gelu_backward kernel and the library GEMM of the pair.
 * act == PN_ACT_SOFTPLUS is the backward of an nn.Linear -> nn.Softplus pair (beta 1, threshold 20), a its output:
 *   gz[r][k] = g[r][k] * (-expm1f(-a[r][k]))      dx[r][n] = sum_k gz[r][k] w[k][n]
 * -- 1 - e^(-a) is sigma(z) written in the output: no cancellation for any a >= 0, exactly 1 from a of about 17.4 on (gz == g bit for bit
 * from a >= 18), +-0 at a == 0; ONE rounded product, never contracted, spelled once: the same bits of gz in every form.  The error of
 * expm1f is measured (profiles/linear_softplus_elu.txt): |gz - g (1 - e^(-a))| is held to the figure of g * (-torch.expm1(-a)) plus
 * one unit of 2^-24 |g|, at most 4 * 2^-24 |g|.
 * act == PN_ACT_ELU is the backward of an nn.Linear -> nn.ELU pair (alpha 1), a its output:
 *   gz[r][k] = a[r][k] > 0 ? g[r][k] : g[r][k] * (a[r][k] + 1.f)
 * -- aten.elu_backward on the result: g's bits where a > 0, else one rounded add and ONE rounded product (within 1.5 * 2^-24 |g| of
 * g (a + 1)), never contracted; the comparison is a > 0, so a NaN in a gives a NaN in gz.  For both: a NaN or +-inf in g stays in its
 * own element of gz and its own row of dx; dx has the bits of pn_linear_dx fed that gz, in every form.  They replace the elementwise
 * backward kernel and the library GEMM of the pair.
 * PN_ACT_IDENTITY is refused (no prologue, no gz: use pn_linear_dx); so is any other value, and an unknown flag; nothing is launched. */
int pn_linear_bwd_act(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *a, const void *w, int act,
                      void *gz, void *dx, int flags);

/* The backward of a BARE Linear layer -- no activation behind it -- with respect to its input (csrc/pn_linear.hip): for g rows x out_f (the
 * cotangent at the layer's output) and w out_f x in_f as it lies, row-major fp32,
 *   dx[r][n] = sum_k g[r][k] w[k][n]      rows x in_f, written once
 * by the kernel body of pn_linear_bwd without its prologue: no a is read, no gz is written (16 MiB less traffic at 4096 x 512), the A
 * operand is g's bits unchanged.  The bits are fixed by that: for finite g, dx equals the dx of pn_linear_bwd(g, a = 0, w) bit for bit
 * (g (1 - 0 0) is g exactly, with or without the fma), in every form -- plain, ragged, pipelined -- and on every launch.  A NaN or Inf
 * in g stays in its row of dx, an Inf in w in the columns it feeds.  g, w, dx non-NULL and 16-byte aligned; dx shares no byte with g or
 * w: refused otherwise, nothing launched.  Replaces, in the reverse sweep's stage VJPs, the library matmul of a bare nn.Linear of func
 * (the head of every `... -> Linear` net).  pn_linear_dx_supported is pn_linear_bwd_supported; pn_linear_dx_form takes the flags of
 * pn_linear_bwd_form (0 or PN_LINEAR_FORM_PLAIN; any other bit is refused, first). */
int pn_linear_dx_supported(int dtype, int64_t rows, int64_t out_f, int64_t in_f);
int pn_linear_dx(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *w, void *dx);
int pn_linear_dx_form(void *stream, int dtype, int64_t rows, int64_t out_f, int64_t in_f, const void *g, const void *w, void *dx, int flags);

/* result_dev[j] = <x, y_j> for j < nk <= PN_MAX_TERMS, accumulated in double, reduced in a fixed
 * order (bit-reproducible).  ||x||^2 is the case y_0 == x.  Replaces VecMDot / VecNorm inside
 * the KSP(GMRES) and SNES that PETSc's implicit steppers run (TS type BE/CN, pa.py:651-654;
 * the reference reaches them through ts.getSNES().getKSP(), pa.py:701-702).
 * `work` needs pn_dots_work_bytes(n) bytes, ZERO-FILLED once before its first use (arrival counter, as
 * pn_rk_combine_wrms; one launch); result_dev holds nk doubles (a pn_pinned_scalar() block has room for 8). */
int pn_dots(void *stream, int dtype, int64_t n, const void *x, int nk, const void *const *y,
            void *work, double *result_dev);
int64_t pn_dots_work_bytes(int64_t n);
/* out = sum_{j<nin} c[j]*x[j], 1 <= nin <= PN_MAX_TERMS (out may alias any x[j]).  The general
 * form of the streaming kernel; the Krylov / Newton updates of the implicit steppers use it where
 * PETSc calls VecAXPY / VecAXPBY / VecMAXPY / VecWAXPY / VecScale. */
int pn_lincomb(void *stream, int dtype, int64_t n, void *out, int nin, const void *const *x, const double *c);
/* Waits for the stream, then copies `count` doubles from a pn_pinned_scalar() block. */
int pn_stream_wait_scalars(void *stream, const double *host_ptr, int count, double *values);

/* y = x (device copy on the stream; u0 -> trajectory slot, span solutions -> output). */
int pn_copy(void *stream, int dtype, int64_t n, void *y, const void *x);
/* y = 0 */
int pn_zero(void *stream, int dtype, int64_t n, void *y);

/* Per-kernel timing for bench.py's roofline: when enabled, every device entry point above is
 * launched with a start/stop HIP event pair bound to the dispatch itself; pn_prof_collect()
 * synchronises and returns, per entry point, the number of launches, the summed kernel
 * duration in microseconds and the summed ALGORITHMIC bytes (each distinct input read once +
 * each output written once).  PN_K_LINEAR_WGRAD (pn_linear_wgrad / _group, an MFMA-bound product) is the
 * exception: what it reports as bytes are its FLOPs, 2 * rows * out * in per pair.
 * PN_K_COUNT is versioned with PN_ABI_VERSION (it grows when a kernel is added); pn_prof_collect takes the length `count` of the
 * caller's three arrays and fills min(count, PN_K_COUNT) entries, so a client built against a shorter enum is not overrun. */
typedef enum { PN_K_STAGE = 0, PN_K_COMBINE_WRMS, PN_K_ADJ_THETA, PN_K_ADJ_ACCUM,
               PN_K_PARAM_ACCUM, PN_K_COPY, PN_K_DOTS, PN_K_LINCOMB, PN_K_LINEAR_WGRAD, PN_K_COUNT } pn_kernel_id;
int pn_prof_enable(int on);
int pn_prof_is_enabled(void);
/* Diagnostic: override the launch geometry / cache policy of the streaming kernels at run time
 * ("vpt=2,ld=0,st=1", same grammar as the PN_TUNE environment variable; NULL = defaults).
 * Used by tools/ab_policy.py for interleaved A/B timing; results never depend on it. */
int pn_tune_set(const char *spec);
int pn_prof_collect(int count, int64_t *launches, double *usec, double *bytes);
const char *pn_kernel_name(int kernel_id);

/* ------------------------------------------------------------------------------------------
 * 3. Host time-stepper.  Replaces the PETSc.TS object held by ODEPetsc (pa.py:370) for the
 *    explicit-RK branch: TSSetType(RK)/TSRKSetType (638-650), TSSetExactFinalTime(MATCHSTEP)
 *    (640), TSSetTimeStep (770,813-817), TSSetTime/TSSetMaxTime (819-820), TSSetTimeSpan
 *    (822), TSSetFromOptions (775), the step loop of TSSolve (829) minus the stage
 *    arithmetic, TSAdaptChoose none|basic.
 * ---------------------------------------------------------------------------------------- */
typedef struct pn_ts pn_ts;

pn_ts *pn_ts_create(void);
void pn_ts_destroy(pn_ts *ts);
int pn_ts_set_rk_type(pn_ts *ts, const char *rk_type);
int pn_ts_get_tableau(const pn_ts *ts, pn_tableau *out);
/* pn_tableau_dense for the RK type `ts` currently has. */
int pn_ts_get_tableau_dense(const pn_ts *ts, int *order, int *npow, double P[PN_MAX_STAGES][PN_DENSE_MAX_POW]);
/* Options database subset, PETSc spellings without the leading dash: ts_adapt_type
 * (none|basic), ts_rk_type, ts_rtol, ts_atol, ts_max_steps, ts_max_reject,
 * ts_adapt_safety, ts_adapt_reject_safety, ts_adapt_clip (lo,hi), ts_adapt_dt_min,
 * ts_adapt_dt_max, ts_adapt_wnormtype (2|infinity).  Unknown keys return non-zero and are left to the caller. */
int pn_ts_set_option(pn_ts *ts, const char *key, const char *value);
/* ts_adapt_wnormtype (2|infinity; TSAdapt's -ts_adapt_wnormtype, read by ts.setFromOptions, pa.py:775): which
 * TSErrorWeightedNorm the callers hand to pn_ts_judge / pn_rows_control -- 2, the weighted RMS (default), or infinity, the
 * largest term (pn_rk_combine_winf, pn_rows_combine_winf).  The controller itself does not change.  Returns 1 for infinity. */
int pn_ts_wnorm_infinity(const pn_ts *ts);
int pn_ts_is_adaptive(const pn_ts *ts);
/* For steppers whose stage arithmetic lives above the ABI (TS types ARKIMEX / THETA, pa.py:651-656): tell the
 * controller the scheme's order (the exponent TSAdaptChoose_Basic uses) and whether it has an embedded
 * solution to estimate the error with.  order == 0 hands the controller back to the RK tableau. */
int pn_ts_set_scheme(pn_ts *ts, int order, int has_embed);
int pn_ts_get_tolerances(const pn_ts *ts, double *atol, double *rtol);

/* Begin a solve.  nspan == 1: integrate [t0, span[0]] (pa.py:818-820, t0 = 0);
 * nspan > 1: time span, t0 = span[0] (pa.py:822).  dt0 = step_size (pa.py:812-817). */
int pn_ts_begin(pn_ts *ts, double t0, double dt0, int nspan, const double *span);
/* Current attempt: time at step start and the step size to use. */
int pn_ts_attempt(const pn_ts *ts, double *t, double *h);
/* Judge the attempt.  enorm < 0: no error estimate (fixed step).  Outputs:
 *   accept      1 = step accepted (time advanced), 0 = rejected (retry with the new h)
 *   hit_span    index of the span point reached by this step, or -1
 *   done        1 = final time reached (or max_steps hit -> status != 0)
 * Restates TSAdaptChoose (+Basic), the MATCHSTEP rule and the span bookkeeping. */
int pn_ts_judge(pn_ts *ts, double enorm, int *accept, int *hit_span, int *done);
/* pa.py:523-525: a per-step list overrides the step size of step `stepno`. */
int pn_ts_override_next_dt(pn_ts *ts, double dt);
int64_t pn_ts_steps(const pn_ts *ts);
int64_t pn_ts_rejections(const pn_ts *ts);
double pn_ts_time(const pn_ts *ts);
/* The step size the controller remembers across an output time it cut a step for (0: none); TSSetTimeSpan's bookkeeping
 * (pa.py:822), read by the per-row controllers of section 3a''' at the start of a solve. */
double pn_ts_span_cached_dt(const pn_ts *ts);
/* accepted-step log of the last solve: start time and size of step k, 0 <= k < steps */
int pn_ts_step_log(const pn_ts *ts, int64_t k, double *t_start, double *h);

/* ------------------------------------------------------------------------------------------
 * 3a. The step loops (round 4).  In the reference `ts.solve` and `ts.adjointSolve` are PETSc's C loops
 *     (pa.py:829, 878): TSStep_RK forms every stage vector and calls back into Python only for func
 *     (evalRHSFunction, pa.py:393-412); TSAdjointStep_RK forms every stage cotangent and calls back only for
 *     the transposed-Jacobian products (RHSJacShell.multTranspose / RHSJacPShell.multTranspose, pa.py:52-82,
 *     341-363).  These two entry points are those loops for ONE step attempt / ONE reversed step: the tableau
 *     walk, the coefficients h*a_ij (formed in double, as TSStep_RK forms w[j] = h*A[i][j]) and the launches
 *     are here; the callbacks are the two the reference has.
 *
 *     pn_vec_ops: the vector operations the loops launch.  NULL (or NULL members) = this library's HIP entry
 *     points of section 2; a table of other functions with the same signatures lets the loops run on a
 *     different backend (the CPU-only test container's stand-in).
 * ---------------------------------------------------------------------------------------- */
typedef int (*pn_rk_stage_fn)(void *stream, int dtype, int64_t n, void *y, const void *u, int nk, const void *const *K,
                              const double *coef);
typedef int (*pn_rk_combine_wrms_fn)(void *stream, int dtype, int64_t n, void *unew, const void *u, int nk,
                                     const void *const *K, const double *coef_b, const double *coef_e, double atol,
                                     double rtol, void *work, double *result_dev);
typedef int (*pn_adj_theta_fn)(void *stream, int dtype, int64_t n, void *w, const void *lambda, double c_lam, int nk,
                               const void *const *dlam, const double *coef);
typedef int (*pn_adj_accum_fn)(void *stream, int dtype, int64_t n, void *lambda_out, const void *lambda, int nk,
                               const void *const *dlam, const double *coef, const void *forcing, void *w_next,
                               double c_next);
typedef struct pn_vec_ops {
  pn_rk_stage_fn rk_stage;
  pn_rk_combine_wrms_fn rk_combine_wrms;
  pn_adj_theta_fn adj_theta;
  pn_adj_accum_fn adj_accum;
} pn_vec_ops;

/* evalRHSFunction (pa.py:393-412): evaluate K_stage = f(t, Y_stage) -- the caller knows which buffer holds
 * Y_stage (u itself for stage 0, ystage[stage] otherwise) -- and return the device address of K_stage, which the
 * caller keeps alive until the step is over; 0 = failure. */
typedef int64_t (*pn_stage_cb)(void *user, int stage, double t);
/* One attempt of TSStep_RK with the tableau and tolerances of `ts`, of size h from the state `u` at time t:
 *   for i < s:  Y_i = u + h sum_j a_ij K_j  into ystage[i] (i >= 1; a first-same-as-last tableau writes its last
 *               stage value straight into `unew`);  K_i = cb(user, i, t + c_i h)
 *   k0 != NULL: K_0 is handed in (first-same-as-last, or the retry after a rejection); have_t_first: K_0 is
 *               evaluated at t_first instead of t (re-advancing from a checkpoint, see _first_stage_time);
 *   want_err:   unew and the error norm by pn_rk_combine_wrms (work / result_dev as there), else unew by pn_rk_stage
 *               (nothing to do for a first-same-as-last tableau).
 * kout[0..s) receives the addresses of the stage derivatives. */
int pn_rk_attempt(void *stream, int dtype, int64_t n, const pn_ts *ts, const pn_vec_ops *vec_ops, double t, double h,
                  const void *u, void *unew, void *const *ystage, const void *k0, int have_t_first, double t_first,
                  pn_stage_cb cb, void *user, int want_err, void *work, double *result_dev, const void **kout);

/* RHSJacShell.multTranspose + RHSJacPShell.multTranspose (pa.py:52-82, 341-363) for stage `stage` at time t: the
 * cotangent is lambda itself (cot_in_w == 0), in `wbuf` (1) or in `wbuf2` (2); the callback adds scale * (df/dp)^T cot to mu and
 * returns the device address of J^T cot (kept alive by the caller until the step is over), 0 when f does not depend on its
 * state argument, -1 on failure. */
typedef int64_t (*pn_vjp_cb)(void *user, int stage, double t, int cot_in_w, double scale);
/* TSAdjointStep_RK for the step [t, t + H] (recurrence in SURVEY 8a-6; a stage whose cotangent is a pure multiple of
 * lambda is differentiated with lambda itself, the factor H*b_i folded into the consumers of its result):
 * lambda <- lambda + sum_i dlambda_i (+ forcing, pa.py:938).
 * wbuf2 (may be NULL): a second cotangent buffer; the stages that need one then take wbuf and wbuf2 in turn, so that work the
 * callback left running on another stream (the weight-sensitivity products of the stage before) may still read the previous
 * stage's cotangent while this stage's is written. */
int pn_rk_adjoint_step(void *stream, int dtype, int64_t n, const pn_ts *ts, const pn_vec_ops *vec_ops, double t, double H,
                       void *lambda, void *wbuf, void *wbuf2, pn_vjp_cb cb, void *user, const void *forcing);
/* pn_rk_adjoint_step for a step that holds interpolated outputs (-pn_output_times interpolate): dense_w[i] (NULL: none) is
 * the cotangent D_i = sum_o h*beta_i(theta_o) g_o the step's outputs send to stage i (pn_rk_dense_adjoint), added to that
 * stage's cotangent as one more source after the lambda / dlambda terms:
 *   w_i = H b_i lambda + sum_j H a_ji dlambda_j + D_i.
 * A stage with a D_i is never folded into lambda and is not structurally zero even when b_i == 0.  dense_w == NULL is
 * pn_rk_adjoint_step.  The vector operations are those of vec_ops (adj_theta takes D_i as its last term). */
int pn_rk_adjoint_step_dense(void *stream, int dtype, int64_t n, const pn_ts *ts, const pn_vec_ops *vec_ops, double t,
                             double H, void *lambda, void *wbuf, void *wbuf2, pn_vjp_cb cb, void *user,
                             const void *const *dense_w, const void *forcing);

/* ------------------------------------------------------------------------------------------
 * 3a'. Dense output kernels (csrc/pn_dense.hip; extension, -pn_output_times interpolate).  Extend pn_lincomb: ONE launch
 *     for all the outputs of a step instead of one lincomb per output.  Coefficients travel as kernel arguments (no copy to
 *     the device, capturable), at most PN_DENSE_CHUNK outputs per launch; larger m is split into several launches.
 * ---------------------------------------------------------------------------------------- */
#define PN_DENSE_CHUNK 32
#define PN_DENSE_NONTEMPORAL 1      /* flags: the output rows are stored non-temporally */
/* out[o*ld + e] = u[e] + sum_{j<nk} coef[o*nk + j] * K[j][e]   for o < m, e < n   (nk <= PN_MAX_STAGES)
 * Replaces m pn_lincomb launches (bytes (nk+1)*m*n -> (nk+1+m)*n).  Summation order of pn_lincomb_kernel: u, then fma in j. */
int pn_rk_dense_eval(void *stream, int dtype, int64_t n, const void *u, int nk, const void *const *K, int m,
                     const double *coef, void *out, int64_t ld, int flags);
/* The transpose, for the reverse sweep:  D[j][e] (+)= sum_{o<m} coef[o*nd + j] * g[o*ld + e]   for j < nd (<= PN_MAX_STAGES),
 * G[e] (+)= sum_o g[o*ld + e] (G may be NULL).  accumulate: start from the D / G already there (else from the first row).
 * Fixed order (o ascending, fma), no atomics: bit-reproducible; a split into chunks gives the same bits. */
int pn_rk_dense_adjoint(void *stream, int dtype, int64_t n, int m, const void *g, int64_t ld, int nd, const double *coef,
                        void *const *D, void *G, int accumulate);

/* ------------------------------------------------------------------------------------------
 * 3a''. Time-gradient reductions (csrc/pn_tgrad.hip; extension: odeint_adjoint's dL/dt).  The
 *     reference returns no gradient for the output times (pa.py:947).  Both accumulate in double into slots of a device
 *     vector, reduce in a fixed order (per-workgroup partials, the last workgroup to arrive adds them in index order; no
 *     float atomics: bit-reproducible) and never wait for the host (capturable).  `work` needs pn_tgrad_work_bytes(n)
 *     bytes, ZERO-FILLED once before its first use (arrival counters, as pn_dots); one work area serves every launch of
 *     one stream.
 * ---------------------------------------------------------------------------------------- */
int64_t pn_tgrad_work_bytes(int64_t n);
/* acc[0] (+)= sum_{p<np} coef[p] * <x[p], y[p]>   (np <= PN_MAX_STAGES; accumulate 0: acc[0] is overwritten) */
int pn_tgrad_dots(void *stream, int dtype, int64_t n, int np, const void *const *x, const void *const *y, const double *coef,
                  void *work, double *acc, int accumulate);
/* acc[o] (+)= sum_{j<nk} coef[o*nk + j] * <g[o*ld ..], K[j]>   for o < m: the derivative of a step's interpolated outputs
 * with respect to their times (coef = beta'_j(theta_o)), each g row and each K_j read once per PN_DENSE_CHUNK rows. */
int pn_rk_dense_tgrad(void *stream, int dtype, int64_t n, int m, const void *g, int64_t ld, int nk, const void *const *K,
                      const double *coef, void *work, double *acc, int accumulate);

/* ------------------------------------------------------------------------------------------
 * 3a'''. Per-sample step control (csrc/pn_rows.hip; extension, -pn_adapt_scope sample).  The
 *     reference's TSAdapt treats the batch as one vector (one TSErrorWeightedNorm, one step size; ts.solve, pa.py:829).
 *     Here the state is B rows of d entries (row r at element r*d) and every row has its own time, step size and
 *     accept / reject decision: per row, these entry points stand for TSStep_RK's stage arithmetic (pn_rows_stage,
 *     pn_rows_combine_wrms), TSAdaptChoose_Basic + the MATCHSTEP / time-span bookkeeping of TSSolve (pn_rows_control,
 *     the text of pn_ts_judge compiled for the device) and TSAdjointStep_RK's cotangent arithmetic (pn_rows_adj_theta,
 *     pn_rows_adj_accum; ts.adjointSolve, pa.py:878).  `h`: B doubles on the device, the row's step size (0 makes the
 *     row's stage values equal its state and its cotangents zero: the identity).  Tableau coefficients are passed
 *     WITHOUT the step size; h[r]*coef[j] is formed in double on the device and rounded once.  A row's result never
 *     depends on B or on the other rows; with equal h a row is the bits of the pn_rk_* / pn_adj_* entry point.
 * ---------------------------------------------------------------------------------------- */
/* Y[r] = u[r] + sum_{j<nk} (h[r]*coef[j]) K[j][r]      (coef[j] = a_ij) */
int pn_rows_stage(void *stream, int dtype, int64_t B, int64_t d, void *y, const void *u, int nk, const void *const *K,
                  const double *coef, const double *h);
/* pn_rk_combine_wrms per row: unew[r] = u[r] + sum (h[r]*coef_b[j]) K[j][r] (unew == NULL: u already is the new state),
 * err = sum (h[r]*coef_e[j]) K[j][r], enorm[r] = sqrt(sum_e (err/(atol + rtol*max(|unew|,|unew+err|)))^2 / d) -- B doubles
 * on the device, finished in the launch (one row is summed by one group of threads in a fixed order). */
int pn_rows_combine_wrms(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk,
                         const void *const *K, const double *coef_b, const double *coef_e, const double *h, double atol,
                         double rtol, double *enorm);
/* pn_rows_combine_wrms under -ts_adapt_wnormtype infinity (pn_rk_combine_winf per row): the same unew, the same err, the same
 * group-per-row geometry, enorm[r] = max_e |unew - uhat| / (atol + rtol*max(|unew|,|uhat|)) over the row, NaN if any term of
 * the row is (of that row only).  Stands for the row's TSErrorWeightedNorm with NORM_INFINITY (ts.solve, pa.py:829). */
int pn_rows_combine_winf(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk,
                         const void *const *K, const double *coef_b, const double *coef_e, const double *h, double atol,
                         double rtol, double *enorm);
/* pn_rows_combine_wrms / pn_rows_combine_winf with a tolerance per column (pn_rk_combine_wrms_v per row): vatol, vrtol hold
 * `period` doubles on the device and period must be d -- every row uses entry c for its column c; the rows share the vectors,
 * which are only read.  Everything else is the scalar entry point's; vectors filled with one value give its bits. */
int pn_rows_combine_wrms_v(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk,
                           const void *const *K, const double *coef_b, const double *coef_e, const double *h,
                           const double *vatol, const double *vrtol, int64_t period, double *enorm);
int pn_rows_combine_winf_v(void *stream, int dtype, int64_t B, int64_t d, void *unew, const void *u, int nk,
                           const void *const *K, const double *coef_b, const double *coef_e, const double *h,
                           const double *vatol, const double *vrtol, int64_t period, double *enorm);
/* One judgement per unfinished row with the controller constants of `ts` (TSAdaptChoose_Basic, MATCHSTEP, time span:
 * pn_ts_judge's arithmetic), one thread per row.  State: sd = doubles [4][B] (t, h, time of the row's next first stage
 * evaluation, the step remembered across an output time), si = int32 [8][B] (span counter, accepted steps, rejections,
 * rejections of this step, previous attempt rejected, finished (1 final time, 2 ts_max_steps, 3 failed), failure code
 * (1 NaN/Inf norm, 2 ts_max_reject), unused).  nspan > 0: the output times span_dev[0..nspan) (on the device), else the row
 * integrates to max_time.  Written per round: log_d = doubles [3][B] (h_eff = the step size where accepted, else 0; t and
 * first-stage time at the round's START), log_hit = the index of the output time the row landed on or -1, accept = mask,
 * summary = int32 [4]: rows still unfinished, first failing row or -1, its failure code, 0.  `work`:
 * pn_rows_work_bytes(B) bytes, ZERO-FILLED once before first use (arrival counters).  pn_rows_control_host: the same on
 * host arrays (no device); pn_rows_failure: records the message of a failure code for pn_last_error() and returns 1. */
int64_t pn_rows_work_bytes(int64_t B);
int pn_rows_control(void *stream, const pn_ts *ts, int64_t B, int nspan, const double *span_dev, double max_time,
                    const double *enorm, double *sd, int32_t *si, double *log_d, int32_t *log_hit, int32_t *accept,
                    int32_t *summary, void *work);
int pn_rows_control_host(const pn_ts *ts, int64_t B, int nspan, const double *span, double max_time, const double *enorm,
                         double *sd, int32_t *si, double *log_d, int32_t *log_hit, int32_t *accept, int32_t *summary);
int pn_rows_failure(int code, int64_t row);
/* unext[r] = accept[r] ? unew[r] : u[r] (unext may be u: then only accepted rows are written), and where accept[r] and
 * 0 <= hit[r] < nout: sol[hit[r]*ld + r*d ..] = unew[r] (sol may be NULL).  Replaces getTimeSpanSolutions (pa.py:845). */
int pn_rows_commit(void *stream, int dtype, int64_t B, int64_t d, void *unext, const void *u, const void *unew,
                   const int32_t *accept, const int32_t *hit, void *sol, int64_t ld, int nout);
/* w[r] = (h[r]*c_lam) lambda[r] + sum_{j<nk} (h[r]*coef[j]) dlam[j][r]      (lambda == NULL: no such term; nk <= 6) */
int pn_rows_adj_theta(void *stream, int dtype, int64_t B, int64_t d, void *w, const void *lambda, double c_lam, int nk,
                      const void *const *dlam, const double *coef, const double *h);
/* lambda_out[r] = lambda[r] + sum_{j<nk} dlam[j][r] (+ g[hit[r]*ld + r*d ..] where 0 <= hit[r] < nout; g may be NULL):
 * the closing update of a reversed round with the masked forcing (pa.py:938 per row). */
int pn_rows_adj_accum(void *stream, int dtype, int64_t B, int64_t d, void *lambda_out, const void *lambda, int nk,
                      const void *const *dlam, const void *g, int64_t ld, const int32_t *hit, int nout);
/* -pn_adapt_scope sample with -pn_output_times interpolate: the controller sees [t[0], t[nout-1]] only and the rows serve
 * the output times themselves.  times_dev: the nout output times on the device; next: int32 [B], the row's first output
 * not yet served (1 at the start of a solve); P: the used rows of pn_tableau_dense's table, [nk][PN_DENSE_MAX_POW]
 * (kernel arguments); log_d / log_hit: the round's log as pn_rows_control has just written it; tnew: the times the
 * controller wrote (row PN_ROWS_T of sd).
 * pn_rows_dense_eval, after an accepted attempt of row r from t_r with h_r to tnew_r: the outputs next <= o <= nout-2 with
 * times[o] < tnew_r become sol[o*ld + r*d ..] = u[r] + sum_j c_j K[j][r], c_j = h_r beta_j((times[o] - t_r)/h_r) formed
 * in double as ODEPetsc._dense_coefs forms it (Horner from the highest power, then h * v) and rounded once; u first, then
 * fma in j order.  An output with times[o] == tnew_r, and output nout-1 when log_hit[r] >= 0 on entry (the controller
 * landed on the final time), is a copy of unew[r].  Written back: next, range = int32 [2][B] (the row's [lo, hi) of this
 * round) and log_hit[r] = the output copied or -1 (what pn_rows_adj_accum's masked forcing reads in the reverse sweep).
 * Rejected and finished rows (h_eff == 0) serve nothing; rows of sol outside a row's range are not touched.  A row's
 * bits do not depend on B or on the other rows.  pn_rows_dense_plan_host: the same plan on host arrays (no device);
 * next == NULL: range is given and only coefficients are formed; coef (may be NULL): [nout][B][nk], entries
 * (o, r, .) written for lo_r <= o < hi_r. */
int pn_rows_dense_eval(void *stream, int dtype, int64_t B, int64_t d, const void *u, int nk, const void *const *K,
                       const double *P, const void *unew, void *sol, int64_t ld, int nout, const double *times_dev,
                       const double *log_d, const double *tnew, int32_t *log_hit, int32_t *next, int32_t *range);
int pn_rows_dense_plan_host(int64_t B, int nout, const double *times, const double *log_d, const double *tnew,
                            int32_t *log_hit, int32_t *next, int32_t *range, int nk, const double *P, double *coef);
/* The transpose for a reversed round: D[j][r] = sum_{lo_r <= o < hi_r} c_{o,j,r} g[o*ld + r*d ..] (from zero, fma, o
 * ascending) for the nd used columns and G[r] = sum_o g[o*ld + r*d ..]; rows with an empty range get zeros. */
int pn_rows_dense_adjoint(void *stream, int dtype, int64_t B, int64_t d, const void *g, int64_t ld, int nout,
                          const double *times_dev, const double *log_d, const int32_t *range, int nd, const double *P,
                          void *const *D, void *G);
/* pn_rows_adj_theta with one more source, added last and NOT scaled by h[r] (pn_rk_adjoint_step_dense's D_i per row):
 * w[r] = (h[r]*c_lam) lambda[r] + sum_{j<nk} (h[r]*coef[j]) dlam[j][r] + dense_w[r]. */
int pn_rows_adj_theta_dense(void *stream, int dtype, int64_t B, int64_t d, void *w, const void *lambda, double c_lam,
                            int nk, const void *const *dlam, const double *coef, const double *h, const void *dense_w);
/* dL/dt of a per-sample solve (the reference returns no gradient for the output times, pa.py:947):
 * row r is a batch-of-one solve and its dL/dt is section 5.6's rule on its own logged steps; dtrow = doubles [nout][B]
 * holds what each row sends to each output time, and dL/dt is its sum over the rows.  Nothing waits for the host.
 * pn_rows_tgrad_dots: rowacc[r] (+)= sum_{p<np} coef[p] <x[p][r], y[p][r]> (np <= PN_MAX_STAGES; accumulate 0: overwritten),
 * products and sums in double, in the geometry and the tree of pn_rows_combine_wrms: a row's bits do not depend on B.
 * pn_rows_dense_tgrad: erow[o*B + r] = sum_{j<nk} beta'_j(theta) <g[o*ld + r*d ..], K[j][r]> for the outputs lo_r <= o < hi_r
 * of the round's logged range, theta = (times[o] - t_r)/h_r and beta'_j(theta) = sum_p (p+1) P[j][p] theta^p formed in double
 * (Horner, the shared text of csrc/pn_adapt.h); entries outside a row's range are not written.  pn_rows_dense_tgrad_host:
 * theta ([nout][B]) and beta' (dcoef, may be NULL: [nout][B][nk]) of the same ranges on host arrays (no device).
 * pn_rows_tgrad_scatter: one reversed round into every row's own column of dtrow (no atomics), from the round's log.  The
 * output interval [is, ie] of the round: with `range` (interpolated outputs) [0, nout-1], the step is its last when
 * log_hit[r] == nout-1; else ie = the output the row last landed on in the reversed order (kept in iv[r]; the step with
 * log_hit[r] >= 0 is the interval's last) and is = ie-1 (none when nout == 1).  With q = sum_j tbar[j][r] (+ held[r]) and
 * p = rowacc[r]/h_r + sum_j coef[j] tbar[j][r] (+ c_last held[r]): dtrow[is] += q, and for the last step dtrow[ie] += p,
 * dtrow[is] -= p.  fsal: stage 0 of the round was evaluated by the row's previous accepted step, so held[r] is replaced by
 * tbar0[r] (NULL: 0) for the round that reverses that step.  An output o of the range adds erow[o*B + r] to dtrow[o], takes
 * it from q and theta times it from p.  Rows with h_eff == 0 are not touched.  flush != 0 (after the last reversed round):
 * dtrow[0] += held[r] when nout > 1 (the row's first step evaluated stage 0 at t[0] itself), held[r] = 0.  held: B doubles,
 * iv: B int32, zero and nout-1 at the start of a reverse sweep.  pn_rows_tgrad_scatter_host: the same on host arrays.
 * pn_rows_tgrad_reduce: dt[i] = sum_r dtrow[i*B + r] in a fixed order (per-workgroup partials, the last workgroup adds them in
 * index order; the grid depends on B and nout alone).  `work`: pn_rows_tgrad_work_bytes(B, nout) bytes, ZERO-FILLED once. */
int pn_rows_tgrad_dots(void *stream, int dtype, int64_t B, int64_t d, int np, const void *const *x, const void *const *y,
                       const double *coef, double *rowacc, int accumulate);
int pn_rows_dense_tgrad(void *stream, int dtype, int64_t B, int64_t d, const void *g, int64_t ld, int nout,
                        const double *times_dev, const double *log_d, const int32_t *range, int nk, const double *P,
                        const void *const *K, double *erow);
int pn_rows_dense_tgrad_host(int64_t B, int nout, const double *times, const double *log_d, const int32_t *range, int nk,
                             const double *P, double *theta, double *dcoef);
int pn_rows_tgrad_scatter(void *stream, int64_t B, int nout, double *dtrow, const double *rowacc, int nt,
                          const double *const *tbar, const double *coef, const double *tbar0, double c_last, int fsal,
                          const double *log_d, const int32_t *log_hit, const int32_t *range, const double *erow,
                          const double *times_dev, double *held, int32_t *iv, int flush);
int pn_rows_tgrad_scatter_host(int64_t B, int nout, double *dtrow, const double *rowacc, int nt, const double *const *tbar,
                               const double *coef, const double *tbar0, double c_last, int fsal, const double *log_d,
                               const int32_t *log_hit, const int32_t *range, const double *erow, const double *times,
                               double *held, int32_t *iv, int flush);
int64_t pn_rows_tgrad_work_bytes(int64_t B, int nout);
int pn_rows_tgrad_reduce(void *stream, int64_t B, int nout, const double *dtrow, double *dt, void *work);
/* -pn_rows_compact 1: func is evaluated and differentiated on the rows of a round that have work to
 * do.  The reference has no counterpart: its TSStep_RK evaluates func on the whole vector (ts.solve, pa.py:829).  Nothing
 * here computes; values travel as bits (NaN payloads and -0.0 included).
 * pn_rows_list: the ordered list of such rows.  kind 0, the open rows: src = the int32 `finished` row of si, row r is listed
 * when src[r] == 0.  kind 1, the stepped rows: src = the fp64 h_eff row of a round's log_d, listed when src[r] > 0 (NaN is
 * not).  Written: idx[0..m) = the listed rows in ascending order, idx[m..B) = -1, pos[r] = the place of row r in idx or -1,
 * count[0] = m.  One workgroup; a row's place is the number of listed rows before it, so the list does not depend on
 * scheduling.  `work` is not used (no arrival counters; may be NULL).  B <= 0x7fffff00.  pn_rows_list_host: the same list
 * on host arrays (no device), the shared text of csrc/pn_adapt.h.
 * pn_rows_gather: out[k] = src[idx[k]] for k < m, rows of d entries; a row with idx[k] < 0 is written as zeros and nothing
 * is read for it.  m == 0 launches nothing.  d == 1 with PN_F64 gathers the rows' times.
 * pn_rows_scatter: out[r] = pos[r] >= 0 ? src[pos[r]] : +0 for every r < B: every row of out is written, none is read (no
 * atomics, no read-modify-write).  src == NULL: every row is +0.
 * Both copy 16 bytes per access when d * sizeof(T) is a multiple of 16 and out and src are 16-byte aligned, else element by
 * element; unprofiled, as the other row kernels are. */
int pn_rows_list(void *stream, int64_t B, int kind, const void *src, int32_t *idx, int32_t *pos, int32_t *count, void *work);
int pn_rows_list_host(int64_t B, int kind, const void *src, int32_t *idx, int32_t *pos, int32_t *count);
int pn_rows_gather(void *stream, int dtype, int64_t m, int64_t d, void *out, const void *src, const int32_t *idx);
int pn_rows_scatter(void *stream, int dtype, int64_t B, int64_t d, void *out, const void *src, const int32_t *pos);

/* ------------------------------------------------------------------------------------------
 * 3b. GMRES core for the implicit (theta-method) stage solves: the small dense part of
 *     KSPGMRES -- Hessenberg columns, Givens rotations, residual estimate, back substitution.
 *     The Krylov vectors live in HBM and are orthogonalised with pn_dots + pn_rk_stage-style
 *     linear combinations by the caller; the operator (shift*M - J, or its transpose) is the
 *     matrix-free shell above the ABI (pa.py:98-197 IJacShell.mult / multTranspose).
 * ---------------------------------------------------------------------------------------- */
typedef struct pn_gmres pn_gmres;
pn_gmres *pn_gmres_create(int restart);
void pn_gmres_destroy(pn_gmres *g);
/* start a cycle with initial residual norm beta */
int pn_gmres_begin(pn_gmres *g, double beta);
/* column k of the Hessenberg matrix: h[0..k] = <w, V_j>, h[k+1] = ||w - sum h_j V_j||;
 * applies the rotations and returns the residual-norm estimate after this iteration */
int pn_gmres_column(pn_gmres *g, int k, const double *h, double *resnorm);
/* coefficients y[0..k] of the update x += sum y_j V_j after k+1 iterations */
int pn_gmres_solve(pn_gmres *g, int k, double *y);

/* ------------------------------------------------------------------------------------------
 * 3c. Device-resident GMRES (round 3).  The same KSPGMRES as 3b -- classical Gram-Schmidt, Givens rotations,
 *     residual test after every column, restart -- with everything it decides kept in a state block in HBM, so that
 *     the host synchronises once per chunk of iterations instead of once per iteration (the reference's default
 *     linear_solver="petsc" for TS types BE / CN / ARKIMEX: pa.py:547, 581, 651-656, 701-702; operator = the
 *     matrix-free shell IJacShell.mult / multTranspose above this ABI, pa.py:98-197).
 *       state       pn_krylov_state_doubles(n, restart) doubles of device memory, ZERO-FILLED once before first use
 *       status_dev  device pointer of a pn_pinned_block() of >= 8 doubles; every decision refreshes it:
 *                   [0] stop (0 running, 1 converged, 2 happy breakdown, 3 iteration limit, 4 NaN, 5 singular
 *                   Hessenberg)  [1] iterations done in this cycle  [2] iterations of the solve  [3] residual-norm
 *                   estimate  [4] beta  [5] ||rhs||  [6] tol = max(rtol ||rhs||, atol)  [7] second Gram-Schmidt passes of the solve
 *       V           restart + 1 Krylov vectors of n elements, vector j at V + j*ldv;  vin: the operator's input
 *                   buffer (every new basis vector is also written there);  w: the operator's output A vin
 *     Once `stop` is set, every later pn_krylov_step of the cycle is a no-op on the device: the host may enqueue
 *     iterations ahead and read the status whenever it likes.
 *     `part` = 0: everything in one call (one rank).  Several ranks sum the Gram-Schmidt products over the ranks
 *     first: part 1 leaves them at state + pn_krylov_products_offset(restart) (k + 2 doubles, 1 at a cycle start),
 *     the caller all-reduces that block in stream order, then part 2 (and, for a step, part 3 after a second
 *     all-reduce of the same block) continues.
 * ---------------------------------------------------------------------------------------- */
int64_t pn_krylov_state_doubles(int64_t n, int restart);
int pn_krylov_products_offset(int restart);
/* Start a cycle from the residual r (first_cycle: r = rhs, x = 0): beta = ||r||, tolerances, V_0 = r/beta. */
int pn_krylov_begin(void *stream, int dtype, int64_t n, int restart, double *state, double *status_dev, const void *r,
                    void *V, int64_t ldv, void *vin, double rtol, double atol, int64_t maxit, int first_cycle, int part);
/* Iteration k of the cycle, w = A V_k given: Gram-Schmidt, V_{k+1}, Hessenberg column, residual estimate, stop flag.
 * k = -1: "the iteration the state block says is due" -- the launches then carry nothing that changes from one iteration to
 * the next, so operator application + step can be captured once as a hipGraph and replayed for every iteration. */
int pn_krylov_step(void *stream, int dtype, int64_t n, int restart, double *state, double *status_dev, int k, void *w,
                   void *V, int64_t ldv, void *vin, int part);
/* If the cycle has ended (stopped, or restart length reached) and x has not been updated for it yet:
 * x += sum_j y_j V_j with y from the back substitution; otherwise nothing. */
int pn_krylov_close(void *stream, int dtype, int64_t n, int restart, double *state, double *status_dev, void *x, void *V,
                    int64_t ldv);

/* ------------------------------------------------------------------------------------------
 * 4. Checkpoint scheduler.  Replaces TSTrajectory as enabled by ts.setSaveTrajectory()
 *    (pa.py:771-772) with -ts_trajectory_solution_only / -ts_trajectory_max_cps_ram
 *    (README.md:91-96).  It only plans: slots are indices into HBM slabs owned by the caller.
 *      mode PN_TRAJ_ALL       every step's state AND stage values kept  (solution_only 0)
 *      mode PN_TRAJ_SOLUTION  every step's state kept, stages recomputed (PETSc default)
 *      mode PN_TRAJ_BUDGET    at most max_slots states kept, the rest recomputed
 * ---------------------------------------------------------------------------------------- */
typedef enum { PN_TRAJ_ALL = 0, PN_TRAJ_SOLUTION = 1, PN_TRAJ_BUDGET = 2 } pn_traj_mode;
typedef struct pn_traj pn_traj;

pn_traj *pn_traj_create(void);
void pn_traj_destroy(pn_traj *tj);
int pn_traj_begin(pn_traj *tj, int mode, int64_t max_slots);
/* BUDGET mode, after pn_traj_begin: the checkpoints carry the stage values of their step (-ts_trajectory_solution_only 0:
 * PETSc's checkpoints hold them, README.md:91-96 "optimal checkpointing").  They are written whenever a sweep steps on
 * from a kept state, and reversing such a step then recomputes nothing.  Placement is then optimal for THAT cost
 * (re-advanced steps + stage computations of the reversed steps; the CAMS cost model of PETSc's TSTrajectory memory
 * type) instead of for the re-advanced steps alone. */
int pn_traj_set_carry(pn_traj *tj, int carries_stage_values);
/* Optional, BUDGET mode: the number of steps of the coming forward sweep when it is known in
 * advance (fixed step).  The sweep then keeps the states of the binomial-optimal (revolve-type)
 * schedule instead of thinning online; the reverse sweep places its intermediate checkpoints
 * optimally in either case (dynamic programme, up to 8192 steps x 64 slots). */
int pn_traj_set_total(pn_traj *tj, int64_t nsteps);
/* Number of accepted steps a fixed-step solve started with pn_ts_begin will take (dry run of the
 * state machine on a copy; -1 for an adaptive scheme). */
int64_t pn_ts_count_fixed_steps(const pn_ts *ts);
/* Forward sweep: where does the state at the START of step `step` go?  Returns a slot index,
 * or -1 = not kept (caller uses a work buffer).  May recycle slots (BUDGET mode). */
int64_t pn_traj_fwd_slot(pn_traj *tj, int64_t step);
/* Reverse sweep, to reverse step `step` (needs the state at its start):
 *   from_step, from_slot: nearest kept state at or before `step`;
 *   the caller re-advances from_step -> step, and on the way stores the states at
 *   store_step[k] into store_slot[k] (k < *nstore, at most cap entries). */
int pn_traj_rev_plan(pn_traj *tj, int64_t step, int64_t *from_step, int64_t *from_slot,
                     int *nstore, int64_t *store_step, int64_t *store_slot, int cap);
/* Step `step` has been reversed: the state at the start of step+1.. is no longer needed. */
int pn_traj_rev_done(pn_traj *tj, int64_t step);
int64_t pn_traj_slots_in_use(const pn_traj *tj);
/* Diagnostic: how many checkpoint-placement tables (dynamic programmes) this process has built so far.  The tables are
 * cached process-wide by (cost model, steps, slots): a training loop builds them once, not once per solve. */
int64_t pn_traj_dp_builds(void);
int64_t pn_traj_high_water(const pn_traj *tj);

/* ------------------------------------------------------------------------------------------
 * 5. Disk tier of the trajectory.  Replaces TSTrajectory type "basic" -- PETSc's DEFAULT type, the one the
 *    reference runs with unless `-ts_trajectory_type memory` is given (examples-pnode/ode_demo_petsc.py:26
 *    "By default, disk is used"; README.md:91-96): one file per checkpoint under -ts_trajectory_dirname
 *    (default "SA-data"), removed afterwards unless -ts_trajectory_keep_files.  Here HBM is the default
 *    tier and `-ts_trajectory_type basic` selects this one.  A checkpoint is `slot_bytes` raw bytes (the
 *    state at the start of a step, followed by the step's stage values in store-all mode).
 *    Copies are asynchronous on the caller's stream through `nbuf` pinned staging buffers; file I/O runs on
 *    a thread of the engine.  `device` = 0 makes every pointer a host pointer (plain memcpy): the mode the
 *    CPU-only tests of the host logic use.
 * ---------------------------------------------------------------------------------------- */
typedef struct pn_spill pn_spill;
pn_spill *pn_spill_create(const char *dir, int64_t slot_bytes, int nbuf, int device, int keep_files);
/* waits for outstanding I/O; deletes the files it wrote (and the directory, if it created it and it is
 * empty) unless keep_files was set */
void pn_spill_destroy(pn_spill *sp);
/* forward sweep (TSTrajectorySet): checkpoint `id` <- slot_bytes at `src`.  Returns once the copy is
 * enqueued on `stream`; the caller may recycle `src` with later work on the same stream. */
int pn_spill_put(pn_spill *sp, void *stream, int64_t id, const void *src);
/* reverse sweep: start reading checkpoint `id` in the background (no-op if every staging buffer is busy) */
int pn_spill_prefetch(pn_spill *sp, int64_t id);
/* reverse sweep (TSTrajectoryGet): checkpoint `id` -> `dst`, enqueued on `stream` after the file has been read */
int pn_spill_get(pn_spill *sp, void *stream, int64_t id, void *dst);
/* checkpoint `id` is no longer needed: its file is deleted (unless keep_files) */
int pn_spill_drop(pn_spill *sp, int64_t id);
int pn_spill_stats(pn_spill *sp, int64_t *files, int64_t *bytes_written, int64_t *bytes_read, int64_t *waits);

#ifdef __cplusplus
}
#endif
#endif /* PNODE_AMD_H */

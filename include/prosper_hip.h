/*
 * prosper_hip.h -- C ABI of libprosper_hip.so: the MI355X (gfx950) implementation of
 * prosper's truncated-EM hot path (select_Hprimes -> E_step -> M_step of the
 * component-analysis models in prosper/em/camodels/).
 *
 * The reference is pure Python/NumPy and has no FFI; each entry point below names the
 * reference code it replaces (file:line relative to the reference root).  A maintainer
 * binds these with ctypes from the model's select_Hprimes / E_step / M_step methods
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (e.g. torch.Tensor.data_ptr()) unless its name ends
 *     in _host; the caller owns the memory and keeps it alive until the stream has drained
 *   - matrices are dense row-major; "ld" arguments are row strides in elements
 *   - dims are int64_t; `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - calls only enqueue work: results are valid after the stream is synchronised
 *   - return value: 0 = ok, <0 = PM_E* bad argument, >0 = hipError_t of a failed launch
 *   - no hidden allocation, no global mutable state, no host<->device copies
 *   - float64 throughout: the reference computes in IEEE double
 */
#ifndef PROSPER_HIP_H
#define PROSPER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_OK 0
#define PM_EINVAL (-1)      /* null pointer / non-positive dimension            */
#define PM_ERANGE (-2)      /* dimension outside the supported range (see below) */

#define PM_MAX_H 1024       /* latents per datapoint row handled by one wavefront */
#define PM_MAX_HPRIME 16    /* candidates; state masks are 16-bit                 */

/* ABI version (major*1000 + minor); bumped when a signature changes. */
int pm_version(void);

/* ---------------------------------------------------------------------------------------
 * Deterministic reductions (libprosper_hip_det.so: the same sources built with -DPM_DETERMINISTIC)
 * ---------------------------------------------------------------------------------------
 * The M-step statistics are sums over datapoints formed with f64 atomics; the order the addends land in changes from run to
 * run and with it the last bits of the sums (the reference at a fixed number of ranks is deterministic).  In the deterministic
 * build every addend is rounded to a multiple of a quantum q_c = 2^-52 M_c before it is added, M_c a power of two no partial
 * sum of its category can exceed: all additions are then exact and the result is independent of their order -- the same
 * bits in every run.  pm_det_build(): 1 in that build, 0 in the default one (whose kernels contain none of this).
 * pm_det_set_quanta(unit, M8, stream): the eight magic constants 1.5 M_c of one kernel family (host OR device memory; copied before the
 * family's next launch on `stream`; PM_ERANGE-like -2 in the default build).  Categories per family:
 *   PM_DET_BSC_FUSED8 / PM_DET_DSC   0 Wq, mus, counts (sums of probabilities)   1 sum of q e   2 sum of log-evidences
 *   PM_DET_WP_SPARSE                 0 Wp (sums of E[s] y)
 *   PM_DET_GSC                       0 xpt_s / xpt_ss sums   1 xpt_sz sums   2 xpt_szsz sums
 *   PM_DET_GEMM                      0 the K-slices of pm_gemm_tn_acc_f64
 *   PM_DET_MCA                       0 Wq   1 Wp   2 pi   3 sum of q e   4 sums of log-evidences */
#define PM_DET_BSC_FUSED8 0
#define PM_DET_WP_SPARSE 1
#define PM_DET_GSC 2
#define PM_DET_GEMM 3
#define PM_DET_MCA 4
#define PM_DET_DSC 5
#define PM_DET_BSC_ROWS16 6   /* the other BSC kernel files: categories as PM_DET_BSC_FUSED8 */
#define PM_DET_BSC_FUSED 7
#define PM_DET_BSC_KERNELS 8
int pm_det_build(void);
int pm_det_set_quanta(int unit, const double *M8, void *stream);
/* GSC, deterministic build, inside an EM loop: the quanta of the next E-step (PM_DET_GSC) and of its M-step's contraction
 * (PM_DET_GEMM and PM_DET_WP_SPARSE), derived AND installed by one kernel from parameters that are on the device only -- gram
 * (H,H: its diagonal = |W_h|^2), psi_sq (H,H), tables as pm_gsc_mstep_finish_f64 leaves them (mu in row 6, 1/sigma_sq in
 * tables[8 H]); ymax = max |y_nd|, ynmax = max |y_n|, n = datapoints of the shard.  quanta16 (device): a copy of what was
 * installed, [8 of PM_DET_GSC | 8 of the contraction].  The bounds are those of GSC._det_quanta (gsc_et.py here; the
 * reference has no such mode).  -2 in the default build. */
int pm_gsc_det_quanta_f64(const double *gram, int64_t ldg, const double *psi_sq, const double *tables, int64_t H,
                          int64_t gamma, double ymax, double ynmax, double n, double *quanta16, void *stream);
/* A device-side row list that was built with an atomic counter (`rows[0 .. *count)`, distinct values in [0, N)) sorted
 * ascending, in place: what makes a gathered contraction over it (pm_gemm_tn_acc_rows_f64) independent of the order its
 * producers finished in.  `flags`: 8-byte aligned, 8 * ceil(N / 8) bytes that are ZERO on entry and zero again on return
 * (every listed row sets its byte; a workgroup per 8192 rows compacts them) + 4 * ceil(N / 8192) bytes of scratch behind them. */
int pm_sort_row_list_i32(int32_t *rows, const int32_t *count, int64_t N, unsigned char *flags, void *stream);
const char *pm_error_string(int code);

/* ---------------------------------------------------------------------------------------
 * Dense building blocks (hand-written f64 MFMA kernels, v_mfma_f64_16x16x4_f64)
 * ------------------------------------------------------------------------------------- */

/* C[M,N] = A[M,K] . B[N,K]^T   (both operands K-contiguous).
 * Scores a = W.y for every datapoint (replaces np.inner(W, y) per datapoint,
 * bsc_et.py:111, and the (W-y)**2 sums of bsc_et.py:177 via the Gram identity) with
 * A = Y, B = W^T-as-rows (H,D); also G = W.W^T (replaces np.inner(W,W), bsc_et.py:111). */
int pm_gemm_nt_f64(const double *A, int64_t lda, const double *B, int64_t ldb,
                   double *C, int64_t ldc, int64_t M, int64_t N, int64_t K, void *stream);

/* The same product for SMALL outputs (M, N <= 1024), deterministic: one workgroup per 16 x 16 tile, the K range split over
 * its eight wavefronts and summed in a fixed order -- no atomics, so every rank holding the same operands gets the same
 * bits (pm_gemm_nt_f64 splits such shapes over K with f64 atomics).  A == B: the Gram matrix W W^T of the models' energy
 * algebra (bsc_et.py:177-183 in Gram form), stored symmetric bit for bit. */
int pm_gemm_nt_small_f64(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc,
                         int64_t M, int64_t N, int64_t K, void *stream);
/* C = A . B (A: M x K, B: K x N, row-major; M <= 1024), same scheme: the W solve X = Wq^-1 . Wp behind the device inverse
 * (np.linalg.lstsq(Wq, Wp) at bsc_et.py:380, dsc_et.py:741) in one launch -- no zero fill, no K-slice atomics. */
int pm_gemm_nn_small_f64(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc,
                         int64_t M, int64_t N, int64_t K, void *stream);

/* C[M,N] += A[K,M]^T . B[K,N]   (reduction over the leading/row index, split over
 * workgroups, f64 atomics into C; C must be initialised by the caller).
 * Wp = E[s]^T . Y  -- replaces the per-datapoint np.outer accumulation of
 * bsc_et.py:339-363 (my_Wp). */
int pm_gemm_tn_acc_f64(const double *A, int64_t lda, const double *B, int64_t ldb,
                       double *C, int64_t ldc, int64_t M, int64_t N, int64_t K, void *stream);
/* The same product, decided on the device: the kernels return at once unless *gate (a device double) is non-zero.  The
 * dense half of the pair (pm_bsc_wp_sparse_f64, this) that is enqueued without the host knowing which one applies. */
int pm_gemm_tn_acc_gated_f64(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc,
                             int64_t M, int64_t N, int64_t K, const double *gate, void *stream);
/* C[M,N] += sum over the rows r = rows[0 .. *count) of A[r,:M]^T . B[r,:N]: the same product over a device-side list of
 * rows with a device-side length (count <= max_rows) -- the dense datapoints of GSC's moment contraction
 * (gsc_et.py:592-625; pm_gsc_estep_lists_f64 leaves the list).  `zero_row`: a row of zeros in A and in B (the ragged end of
 * the list reads it).  M % 128 == 0, N % 128 == 0, 16-byte aligned operands, else PM_ERANGE. */
int pm_gemm_tn_acc_rows_f64(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M,
                            int64_t N, const int32_t *rows, const int32_t *count, int64_t max_rows, int64_t zero_row,
                            void *stream);

/* Which kernels pm_gemm_nt_f64 would launch for an (M, N, K) product on the current device -- the function its launcher
 * takes every decision from; nothing is launched.  `aligned`: A and B 16-byte aligned with even lda and ldb (what the
 * launcher derives from its pointers).  Returns a mask of PM_NT_PLAN_* (> 0), or PM_EINVAL (null `out`, M, N or K < 1) /
 * PM_ERANGE (a dimension above INT32_MAX) as the launcher does; out[0] = resident workgroup slots (2 per CU; 512 without a
 * device), out[1] = 128-row panels that run as whole rounds of un-split tiles, out[2] = K-slices of the ragged remainder's
 * tiles (1: not split).  The deterministic build never splits K and reports its own choice. */
#define PM_NT_PLAN_DMA_MAIN 0x001       /* LDS-DMA kernel, whole rounds of un-split 128-row tiles                        */
#define PM_NT_PLAN_DMA_REST 0x002       /* ... the ragged remainder (or a product below one round) un-split, own launch  */
#define PM_NT_PLAN_DMA_REST_SPLIT 0x004 /* ... split over K (zero fill + f64 atomics), own launch                        */
#define PM_NT_PLAN_DMA_FUSED 0x008      /* whole rounds and the remainder's K-slices in ONE launch                       */
#define PM_NT_PLAN_DMA_REST64 0x010     /* the remainder in un-split 64-row tiles                                        */
#define PM_NT_PLAN_REG_MT1 0x020        /* register-staged kernel, 32-row tiles                                          */
#define PM_NT_PLAN_REG_MT2 0x040        /* ... 64-row tiles                                                              */
#define PM_NT_PLAN_REG_MT4 0x080        /* ... 128-row tiles                                                             */
#define PM_NT_PLAN_ALIGNED 0x100        /* the 16-byte-load flavour (every LDS-DMA path; register kernels: even K too)   */
#define PM_NT_PLAN_DMA_WHOLE 0x200      /* deterministic build: rounds and un-split remainder as ONE launch of 128-row tiles */
int pm_gemm_nt_plan(int64_t M, int64_t N, int64_t K, int aligned, int32_t *out);
/* The same for pm_gemm_tn_acc_f64 / pm_gemm_tn_acc_gated_f64 (`aligned` as above; PM_EINVAL for null `out`, M or N < 1,
 * K < 0; PM_ERANGE for M or N above INT32_MAX).  K == 0 launches nothing: mask 0.  out[0] = slots, out[1] = K-splits
 * (grid.y of the first launch), out[2] = rows of K per split (saturated at INT32_MAX). */
#define PM_TN_PLAN_DMA 0x01             /* LDS-DMA kernel (whole 128 x 128 tiles, K >= 64)                               */
#define PM_TN_PLAN_REG 0x02             /* register-staged kernel                                                        */
#define PM_TN_PLAN_ALIGNED 0x04         /* the 16-byte-load flavour                                                      */
#define PM_TN_PLAN_REMAP 0x08           /* K-splits a multiple of 8: all tiles of a split on one XCD                     */
#define PM_TN_PLAN_TAIL 0x10            /* a register-staged launch for the last K % 8 rows follows the LDS-DMA one      */
int pm_gemm_tn_plan(int64_t M, int64_t N, int64_t K, int aligned, int32_t *out);

/* out[n] = sum_d Y[n,d]^2 -- np.inner(y, y) of bsc_et.py:111 and (y**2).sum() of :172;
 * computed once per resident data shard. */
int pm_row_sqnorm_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, double *out, void *stream);

/* sums[d] += sum_n Y[n,d] (center == NULL) or sum_n (Y[n,d] - center[d])^2: the two collective means of
 * CAModel.standard_init (camodels/__init__.py:209-217, dsc_et.py:892-899) over a resident shard.
 * `sums` (D) is accumulated into (caller zeroes it). */
int pm_col_moments_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, const double *center,
                       double *sums, void *stream);

/* sums[d] += sum over the datapoints n with lse[n] >= cut of Y[n,d]: my_data_sum of BSC_ET.M_step when 'mu' is learned
 * (bsc_et.py:422-430) over the datapoints the truncation keeps (:247-258; cut = -inf keeps all).  `sums` is accumulated into. */
int pm_col_sum_kept_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, const double *lse, double cut, double *sums,
                        void *stream);

/* out[n] = sum_d w[d] Y[n,d]^2 -- y^T Sigma^-1 y of GSC with a diagonal noise covariance
 * (gsc_et.py:418-419, 476, 780-781). */
int pm_row_wsqnorm_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, const double *w, double *out,
                       void *stream);

/* inv = (U + U^T - diag(U) + diag(diag_add))^-1 for a symmetric positive definite n x n matrix given
 * by its upper triangle `upper` (n <= 256, one workgroup, Gauss-Jordan in registers, no pivoting).
 * `full` (optional) receives the assembled matrix, `pivots` (optional, 2 doubles) the smallest and
 * largest pivot: a non-positive or vanishing smallest pivot means "numerically singular".
 * Solves the H x H system of the M-step, np.linalg.lstsq(Wq, Wp) at bsc_et.py:380, as
 * W_new = inv . Wp (one pm_gemm_tn_acc_f64). */
int pm_spd_inverse_f64(const double *upper, int64_t ldu, const double *diag_add, int64_t n, double *full,
                       double *inv, int64_t ldo, double *pivots, void *stream);

/* The same inverse, warm-started: `prev_inv` (n x n, leading dimension n) is the inverse of a nearby matrix -- the
 * previous EM step's second moments.  Four Newton-Schulz steps X <- X + X (I - A X) on the matrix cores refine it into
 * `inv` (symmetrised); the Gauss-Jordan sweep is launched behind them and returns at once when the refinement converged:
 * the LAST residual the iteration formed, R_3 = (I - A prev_inv)^8, is below 1e-8 in the Frobenius norm, so the result's
 * is below 1e-16 up to rounding (round 6; until then the START residual had to be below 0.1 in the Frobenius norm, which
 * rejected the few-per-cent-in-every-direction residuals of an annealing ramp although they converge).  Then pivots =
 * {min_i 1 / inv_ii, max_i A_ii}: a lower bound of the smallest and an upper bound of the largest pivot of the sweep.  Else
 * the sweep overwrites `inv` with the exact inverse as pm_spd_inverse_f64 would.  The decision is taken on the device from
 * sums formed in a fixed order and left for the caller in pivots[2] (`pivots`: THREE doubles here): 1.0 = the refinement
 * stands and ||I - A prev_inv||_F < 1, 2.0 = it stands from a start further away, 0.0 = the sweep ran (`inv` is then exact
 * to cond(A) eps only: a caller that skipped the iterative refinement of its solve repeats it with one).  `work`:
 * pm_spd_inverse_warm_work_len(n) doubles; `full` (required, leading dimension ldo = n) receives the assembled matrix.
 * Same role as pm_spd_inverse_f64 (np.linalg.lstsq(Wq, Wp), bsc_et.py:380).
 * pm_spd_inverse_warm_long_f64: the same from a start that may be FAR -- a data-truncation step (bsc_et.py:247-258) whose
 * kept set jumped, a temperature step: the start is scaled by 1 / ||A prev_inv||_inf (both matrices are symmetric positive
 * definite, so the scaled residual's spectrum lies in [0, 1) and the iteration converges from any such start) and eight +
 * one steps run: accepted for ||A prev_inv||_inf / lambda_min(A prev_inv) up to ~14, ~60 us instead of the sweep's 0.3 ms. */
int64_t pm_spd_inverse_warm_work_len(int64_t n);
int pm_spd_inverse_warm_f64(const double *upper, int64_t ldu, const double *diag_add, int64_t n, const double *prev_inv,
                            int64_t ldp, double *work, double *full, double *inv, int64_t ldo, double *pivots,
                            void *stream);
int pm_spd_inverse_warm_long_f64(const double *upper, int64_t ldu, const double *diag_add, int64_t n,
                                 const double *prev_inv, int64_t ldp, double *work, double *full, double *inv, int64_t ldo,
                                 double *pivots, void *stream);

/* `batch` warm-started inverses at once (every kernel of pm_spd_inverse_warm_f64 gets a batch dimension): matrix b is
 * read at upper + b*stride_in (diag_add + b*n), its previous inverse at prev_inv + b*stride_prev (dense n x n), its
 * result written at inv + b*stride_out (dense n x n), pivots 2 doubles per matrix; `work`: batch *
 * pm_spd_inverse_warm_work_len(n) doubles (matrix b's accepted flag -- see above -- in the last word of its share).  GSC's M-step: (sum xpt_szsz)^-1 and (sum xpt_ss + eps I)^-1. */
int pm_spd_inverse_warm_batch_f64(const double *upper, int64_t ldu, int64_t stride_in, const double *diag_add, int64_t n,
                                  const double *prev_inv, int64_t stride_prev, double *work, double *inv,
                                  int64_t stride_out, double *pivots, int64_t batch, void *stream);

/* The same launches with GENERAL (non-symmetric) matrices among the batch: bit b of `general_mask` says matrix b is given in
 * full (row-major, both triangles; diag_add still added) and is refined by the left-sided Newton-Schulz iteration
 * X <- X + (I - X A^T) X from prev_inv + b*stride_prev -- its result is the inverse of the TRANSPOSE, (A^T)^-1 = (A^-1)^T,
 * not symmetrised.  GSC from its second EM step on: psi_sq leaves the M-step non-symmetric (gsc_et.py:660-675), with it
 * Lambda^-1 and sum xpt_szsz, which gsc_et.py:625 inverts as it is; W_new^T = (A^-1)^T Wp^T is then one pm_gemm_nt_f64.
 * `accepted` (batch doubles): 1.0 = the refinement of matrix b stands, 0.0 = its start was too far off and the guarded
 * sweep ran -- which for a general matrix inverts only its upper-mirrored stand-in: the caller then inverts on the host,
 * as the reference does.  A cold start is pm_spd_inverse_batch_f64 on the same buffer (upper-mirrored: a start within
 * ~1e-6) followed by this entry. */
int pm_inverse_warm_batch_f64(const double *mats, int64_t ldu, int64_t stride_in, const double *diag_add, int64_t n,
                              const double *prev_inv, int64_t stride_prev, double *work, double *inv, int64_t stride_out,
                              double *pivots, double *accepted, int64_t batch, uint32_t general_mask, void *stream);

/* `batch` independent inverses in one launch, one workgroup each (they run on different CUs at once): matrix b is
 * read at upper + b*stride_in, written at inv (and full, if given) + b*stride_out; diag_add (optional) holds n
 * doubles and pivots 2 doubles per matrix.  GSC's M-step needs (sum xpt_szsz)^-1 and (sum xpt_ss + eps I)^-1
 * (gsc_et.py:625, 673). */
int pm_spd_inverse_batch_f64(const double *upper, int64_t ldu, int64_t stride_in, const double *diag_add, int64_t n,
                             double *full, double *inv, int64_t ldo, int64_t stride_out, double *pivots,
                             int64_t batch, void *stream);

/* ---------------------------------------------------------------------------------------
 * Distributed k-th largest (the data-truncation cut): parallel.allsort(all_denoms)[-N_use], prosper/utils/parallel.py:87-110
 * with its consumers bsc_et.py:252, mca_et.py:252, dsc_et.py:832.  Radix select over an order-preserving 64-bit key
 * of the doubles, one digit per round: every rank histograms the digit at bit `shift` (`bits` wide, <= 12) of its
 * values that agree with the digits decided so far (state[0]); the caller sum-all-reduces the 4096 bins (RCCL) and
 * pm_kth_scan picks the bin that holds the k-th largest: state[0] |= digit << shift, state[1] = rank inside that bin;
 * `hist` is cleared.  Rounds (shift, bits) = (52,12) (40,12) (28,12) (16,12) (4,12) (0,4) decide all 64 bits;
 * pm_kth_value_f64 converts state[0] back: exactly the value a full sort returns.
 *   state (2 x uint64): [0] digits decided so far (0 before the first round), [1] k, 1-based from the largest.
 *   hist  (4096 x uint64), zeroed by the caller before the first round.
 * ------------------------------------------------------------------------------------- */
int pm_kth_hist_f64(const double *x, int64_t n, const uint64_t *state, int shift, int bits, uint64_t *hist, void *stream);
int pm_kth_scan(uint64_t *hist, uint64_t *state, int shift, int bits, void *stream);
int pm_kth_value_f64(const uint64_t *state, double *out, void *stream);
/* The same select in 1 + 6 + 1 launches instead of 13 (round 6: what a data-truncation step pays once nothing else in it
 * waits for the host): `hists` holds one histogram of 4096 bins PER ROUND (6 x 4096 uint64, zeroed by the caller -- one
 * fill), `states` seven (prefix, k) pairs, slot 0 = (0, k) from the caller.  pm_kth_round_f64(round r) first repeats, in
 * every workgroup, the scan of round r - 1 (its histogram -- sum-all-reduced by the caller between the two calls -- and
 * states[r - 1]; `shift_prev` / `bits_prev`: that round's digit; workgroup 0 stores the result as states[r]), then
 * histograms the digit [shift, shift + bits) of the values that agree with the prefix into hists[r].  pm_kth_final_f64
 * scans the last round and converts: out[0] = the k-th largest, exactly the value a full sort returns.  The value stays
 * on the device (pm_bsc_defer_apply_f64 reads it there).  n = 0 (an empty shard) is fine. */
int pm_kth_round_f64(const double *x, int64_t n, uint64_t *states, uint64_t *hists, int round, int shift_prev, int bits_prev,
                     int shift, int bits, void *stream);
int pm_kth_final_f64(uint64_t *states, const uint64_t *hists, int rounds, int shift_prev, int bits_prev, double *out,
                     void *stream);
/* ... without the fill in front: pm_kth_round_k_f64 (round 0 only) takes the rank k0 as an argument instead of from states[1],
 * pm_kth_final_z_f64 with rezero != 0 leaves the `rounds` histograms zeroed for the next select on the same buffer (which the
 * caller zeroes once, when it allocates it). */
int pm_kth_round_k_f64(const double *x, int64_t n, uint64_t *states, uint64_t *hists, int round, int shift_prev, int bits_prev,
                       int shift, int bits, int64_t k0, void *stream);
int pm_kth_final_z_f64(uint64_t *states, uint64_t *hists, int rounds, int shift_prev, int bits_prev, double *out, int rezero,
                       void *stream);

/* ---------------------------------------------------------------------------------------
 * Binary Sparse Coding (prosper/em/camodels/bsc_et.py)
 * ------------------------------------------------------------------------------------- */

/* select_Hprimes, bsc_et.py:98-115.
 *   scores  (N,H)  a[n,h] = <W_h, y_n>            (from pm_gemm_nt_f64)
 *   wnorm2  (H)    |W_h|^2  (diag of G; element stride `wnorm2_stride`, pass H+1 to read diag(G) in place)
 *   ynorm2  (N)    |y_n|^2
 *   cand    (N,Hprime) int32 out: indices of the Hprime largest a/|W_h|/|y|, ascending
 *           (last = best), i.e. np.argsort(sim)[-Hprime:]; ties broken towards the larger index. */
int pm_bsc_select_f64(const double *scores, int64_t lds, const double *wnorm2, int64_t wnorm2_stride,
                      const double *ynorm2, int64_t N, int64_t H, int64_t Hprime,
                      int32_t *cand, void *stream);

/* Scalars of one E-step (bsc_et.py:151-154,187-190). */
typedef struct pm_bsc_estep_params {
    double pil_bar;      /* log(pi / (1 - pi))                                   */
    double ecoef;        /* beta * pre1 = -(1/T) / (2 sigma^2): multiplies energies */
    double prior_scale;  /* 1 (anneal_prior false) or beta (anneal_prior true)    */
    double mu_sqnorm;    /* |mu|^2 (0 when mu == 0)                              */
} pm_bsc_estep_params;

/* E_step, bsc_et.py:119-192: log-pseudo-joints of the truncated state set
 *   [null ; singletons h = 0..H-1 ; multi-cause states in generate_state_matrix order].
 *   gram    (H,H)  G = W.W^T
 *   wmu     (H)    W.mu, or NULL when mu == 0
 *   ymu     (N)    Y.mu, or NULL when mu == 0
 *   cand    (N,Hprime) int32
 *   state_masks (S) uint16: bit j set <=> state uses candidate position j
 *                  (rows of camodels/__init__.py:21-47's state_matrix)
 *   logpj   (N, 1+H+S) out;  lse (N) out = log sum_k exp(logpj[n,k]) (stable), or NULL. */
int pm_bsc_estep_f64(const double *scores, int64_t lds, const double *gram, const double *ynorm2,
                     const double *wmu, const double *ymu, const int32_t *cand,
                     const uint16_t *state_masks, int64_t S,
                     const pm_bsc_estep_params *params_host,
                     int64_t N, int64_t H, int64_t Hprime,
                     double *logpj, int64_t ldl, double *lse, void *stream);

/* Layout of the packed M-step statistics buffer (float64, one RCCL all-reduce per EM step):
 *   [ Wp (H*D) | Wq (H*H) | qdiag (H) | mus (H) | scalars (PM_BSC_NSCALARS) ]
 * scalars: [0] sum_n sum_k q_nk e_nk (sigma statistic, bsc_et.py:395-415)
 *          [1] sum over kept n of log sum_k exp(logpj) (Fs, bsc_et.py:265)
 *          [2] number of kept datapoints (my_N after truncation, bsc_et.py:257)
 *          [3] number of datapoints whose E[s] row had more than PM_BSC_NZ_MAX non-zeros while the E-step pass wrote
 *              non-zero lists (pm_bsc_estep_fused8_nz_f64); gates pm_bsc_wp_sparse_f64 / pm_gemm_tn_acc_gated_f64 */
#define PM_BSC_NSCALARS 4
int64_t pm_bsc_stats_len(int64_t H, int64_t D);
int64_t pm_bsc_stats_offset_wq(int64_t H, int64_t D);
int64_t pm_bsc_stats_offset_qdiag(int64_t H, int64_t D);
int64_t pm_bsc_stats_offset_mus(int64_t H, int64_t D);
int64_t pm_bsc_stats_offset_scalars(int64_t H, int64_t D);

/* Per-datapoint part of M_step, bsc_et.py:271-272,334-366,395-415: posterior weights
 * q = exp(logpj - lse) of every kept datapoint (lse[n] >= lse_cut; pass -inf to keep all),
 * expectations E[s] (N,H) out (zero rows for cut datapoints), Wq block scatter, and the
 * scalar statistics.  `pair_ptr` (Hprime*Hprime+1) / `pair_states` are the CSR lists of
 * multi-cause states containing candidate positions (i,j) (derived from state_masks on
 * the host; pair_len = pair_ptr[Hprime*Hprime] entries).  Only the upper triangle of Wq is
 * accumulated (row <= col); the caller mirrors it and adds diag(qdiag).  Accumulates into `stats` (caller zeroes it once per EM step). */
int pm_bsc_mstep_rows_f64(const double *logpj, int64_t ldl, const double *lse, double lse_cut,
                          const int32_t *cand, const uint16_t *state_masks, int64_t S,
                          const int32_t *pair_ptr, const uint16_t *pair_states, int64_t pair_len,
                          const pm_bsc_estep_params *params_host,
                          int64_t N, int64_t H, int64_t D, int64_t Hprime,
                          double *expect, int64_t lde, double *stats, void *stream);

/* ---------------------------------------------------------------------------------------
 * BSC fast path: 16 lanes per datapoint (four datapoints per wavefront, DPP row reductions),
 * incremental multi-cause energies, negligible posterior terms skipped.  Same results as the
 * entry points above; available when pm_bsc_rows16_supported(H, Hprime, S) != 0 (H <= 512 and
 * the per-datapoint state areas fit LDS).
 * ------------------------------------------------------------------------------------- */
int pm_bsc_rows16_supported(int64_t H, int64_t Hprime, int64_t S);
/* ... and whether the list-writing form of the M-step row pass (pm_bsc_mstep_rows16_nz_f64: it keeps one more score row
 * per datapoint slot in LDS) fits as well; when it does not, callers run pm_bsc_mstep_rows16_f64 and the dense
 * pm_gemm_tn_acc_f64 (same statistics, bsc_et.py:334-366). */
int pm_bsc_rows16_nz_supported(int64_t H, int64_t Hprime, int64_t S);

/* select_Hprimes (bsc_et.py:98-115) and/or E_step (bsc_et.py:119-192) in one pass over the
 * scores: mode bit 0 = select (write `cand`; otherwise `cand` is an input), bit 1 = E-step
 * (write `logpj`, `lse`).  `state_parents[s]` = index of the state obtained from state s by
 * dropping its highest candidate position (0xFFFF when that leaves a singleton);
 * `size_offsets_host[g-2]` = index of the first state with g causes, g = 2..gamma, and
 * size_offsets_host[gamma-1] = S (states are ordered by size, camodels/__init__.py:32-35).
 * Selection ties: similarities equal in their leading 42 mantissa bits rank by latent index.
 * Further selection modes (other models reuse the selection pass): bit 2 = the Hprime SMALLEST
 * first (mca_et.py:107), bit 3 = rank `scores` as they are (no normalisation), bit 4 = rank the
 * squared distance |W_h|^2 - 2 scores[n,h] with |W_h|^2 from the Gram diagonal (mmca_et.py:119-120). */
int pm_bsc_select_estep_f64(const double *scores, int64_t lds, const double *gram, const double *ynorm2,
                            const double *wmu, const double *ymu, const uint16_t *state_masks,
                            const uint16_t *state_parents, const int32_t *size_offsets_host, int64_t S,
                            int64_t gamma, const pm_bsc_estep_params *params_host, int64_t N, int64_t H,
                            int64_t Hprime, int mode, int32_t *cand, double *logpj, int64_t ldl,
                            double *lse, void *stream);

/* Scores GEMM + select_Hprimes + E_step in ONE kernel (bsc_et.py:98-115 and :119-192): what pm_gemm_nt_f64 followed by
 * pm_bsc_select_estep_f64 computes, without the (N,H) scores buffer -- a workgroup owns 64 datapoints x all H latents
 * and runs the row pass out of its MFMA accumulators.  Y (N,D) data, Wt (H,D) = W^T; the other arguments, the
 * `mode` bits 0 and 1 and the outputs are those of pm_bsc_select_estep_f64 (BSC's own ranking only).  Needs
 * pm_bsc_fused_supported(H, D, Hprime, S): H <= 256, D a multiple of 8 (callers zero-pad the K dimension), 16-byte
 * aligned rows (ldy, ldw even).
 * M-step statistics in the same pass (stats != NULL; Hprime <= 8, mode & 2, lse given): for EVERY datapoint -- i.e. when
 * no data truncation follows (bsc_et.py:247-258 skipped) -- what pm_bsc_mstep_rows16_f64 computes from logpj:
 * E[s] rows into expect (N,H), and into the packed buffer `stats` of a model with D_stats observed dimensions (layout
 * above): the multi-cause part of Wq's upper triangle INCLUDING its diagonal, mus = sum_n E[s], the scalars.  The
 * qdiag block is not written: qdiag = mus - diag(Wq block) (s_h^2 = s_h).  `stats` is accumulated into. */
int pm_bsc_fused_supported(int64_t H, int64_t D, int64_t Hprime, int64_t S);
/* Workgroups of that kernel one CU holds at once for this shape (2 by design: one on the matrix pipe, one in its row
 * passes); diagnostic, <= 0 when unsupported. */
int pm_bsc_fused_occupancy(int64_t H, int64_t D, int64_t Hprime, int64_t S);
int pm_bsc_estep_fused_f64(const double *Y, int64_t ldy, const double *Wt, int64_t ldw, const double *gram,
                           const double *ynorm2, const double *wmu, const double *ymu,
                           const uint16_t *state_masks, const uint16_t *state_parents,
                           const int32_t *size_offsets_host, int64_t S, int64_t gamma,
                           const pm_bsc_estep_params *params_host, int64_t N, int64_t D, int64_t H,
                           int64_t Hprime, int mode, int32_t *cand, double *logpj, int64_t ldl, double *lse,
                           double *expect, int64_t lde, double *stats, int64_t D_stats, void *stream);

/* The same pass for config 2's shape class as a 16-wavefront kernel (csrc/bsc_fused8.hip): a workgroup of 1024 threads
 * owns 128 datapoints x all latents, one per CU; a wavefront accumulates 16 datapoints x 128 latents (<= 128 registers:
 * four wavefronts per SIMD), the row passes run one half-wavefront per datapoint.  Same arguments, outputs and reference
 * lines (bsc_et.py:98-115, :119-192) as pm_bsc_estep_fused_f64.  Needs pm_bsc_fused8_supported(H, D, Hprime, S) --
 * 128 < H <= 256, Hprime = 5 .. 8 (round 6; 8 until then), S that of gamma = 3 or 4 (84 / 154 at Hprime = 8), D a multiple of 8 -- and pm_bsc_fused8_whole_shard(H, Hprime, gamma, S): the
 * complete state set of sizes 2 .. gamma, gamma 3 or 4.  The call takes a WHOLE shard: whole rounds of resident
 * workgroups run 128-row tiles, a ragged remainder of up to two rounds of 16-row workgroups that split K four ways runs in
 * a second launch (no scores buffer, no separate row kernel), and `stats` / `expect` (the M-step statistics of
 * pm_bsc_estep_fused_f64) are accepted.  pm_bsc_fused8_main_rows(N, D): the leading rows the main launch takes.
 * `part`: 0 both launches, 1 only the main one, 2 only the remainder (callers that time or trace them separately). */
int pm_bsc_fused8_supported(int64_t H, int64_t D, int64_t Hprime, int64_t S);
int pm_bsc_fused8_whole_shard(int64_t H, int64_t Hprime, int64_t gamma, int64_t S);
int64_t pm_bsc_fused8_main_rows(int64_t N, int64_t D);
int pm_bsc_estep_fused8_f64(const double *Y, int64_t ldy, const double *Wt, int64_t ldw, const double *gram,
                            const double *ynorm2, const double *wmu, const double *ymu,
                            const uint16_t *state_masks, const uint16_t *state_parents,
                            const int32_t *size_offsets_host, int64_t S, int64_t gamma,
                            const pm_bsc_estep_params *params_host, int64_t N, int64_t D, int64_t H,
                            int64_t Hprime, int mode, int32_t *cand, double *logpj, int64_t ldl, double *lse,
                            double *expect, int64_t lde, double *stats, int64_t D_stats, int part, void *stream);

/* pm_bsc_estep_fused8_f64 that also leaves every E[s] row as a list of its non-zeros (statistics passes only: `stats`
 * given): nz_idx (N x PM_BSC_NZ_MAX uint16: latent indices, unused slots 0xFFFF) and nz_val (N x PM_BSC_NZ_MAX).  Past the
 * annealing phase a posterior of the truncated state set puts weight on a handful of latents (3.7 of 256 per datapoint
 * on config 2), and the M-step's Wp = E[s]^T Y (bsc_et.py:339-363) needs only those rows of the product.  A row with more
 * than PM_BSC_NZ_MAX non-zeros is counted in scalars[3], slot 0 of its list reads PM_BSC_NZ_OVERFLOW, and ITS dense row is
 * stored in `expect`; the dense row of a datapoint whose list is complete is NOT stored (round 5: the list is the row -- N x H
 * doubles of write traffic per step less; pm_bsc_expand_lists_gated_f64 rebuilds those rows when the dense product runs).
 * Statistics of the whole-shard passes (pm_bsc_fused8_whole_shard; both entries): the diagonal of the second moments is
 * left in `qdiag` in full (= mus: E[s_h^2] = E[s_h]) and the diagonal of the Wq block stays zero -- the assembled matrix
 * upper + upper^T - diag(upper) + diag(qdiag) is the same, no fix-up pass is needed. */
#define PM_BSC_NZ_MAX 16
#define PM_BSC_NZ_OVERFLOW 0xFFFEu      /* nz_idx[n][0] of a datapoint whose list overflowed (its dense row is in `expect`) */
int pm_bsc_estep_fused8_nz_f64(const double *Y, int64_t ldy, const double *Wt, int64_t ldw, const double *gram,
                               const double *ynorm2, const double *wmu, const double *ymu,
                               const uint16_t *state_masks, const uint16_t *state_parents,
                               const int32_t *size_offsets_host, int64_t S, int64_t gamma,
                               const pm_bsc_estep_params *params_host, int64_t N, int64_t D, int64_t H,
                               int64_t Hprime, int mode, int32_t *cand, double *logpj, int64_t ldl, double *lse,
                               double *expect, int64_t lde, double *stats, int64_t D_stats, uint16_t *nz_idx,
                               double *nz_val, int part, void *stream);
/* DEFERRED statistics for a data-truncation step (bsc_et.py:247-258 keeps the N_use datapoints with the largest evidence;
 * which ones is known only after the E-step of every rank).  pm_bsc_estep_fused8_defer_f64 is pm_bsc_estep_fused8_nz_f64
 * that, given `records` (N x PM_BSC_DEFER_LD doubles), accumulates NOTHING into `stats` but the overflow count scalars[3]:
 * per datapoint it leaves the non-zero list of E[s] (as above; the dense row when the list overflowed) and the record
 * [36 entries k (k + 1) / 2 + i (i <= k candidate positions) of the multi-cause states' second moments, diagonal entries 0 |
 * ecoef sum_k q_k e_k | pad].  `records` NULL: exactly pm_bsc_estep_fused8_nz_f64.
 * pm_bsc_defer_apply_f64 then adds the records of the datapoints with lse[n] >= *cut (a DEVICE double: the radix select's
 * result never visits the host; values below log(2^-1075) mean "keep all", bsc_et.py:253) into `stats` -- Wq pair block,
 * mus = qdiag, sum q e, sum lse, kept count, i.e. what the in-pass statistics of the kept datapoints would have been
 * (bsc_et.py:334-366, 395-415) -- and empties the lists (zeroes the dense rows) of the others, so that
 * pm_bsc_wp_sparse_expand_f64 / pm_gemm_tn_acc_gated_f64 behind it see kept datapoints only.  H <= 256, Hprime = 5 .. 8. */
#define PM_BSC_DEFER_LD 40
int pm_bsc_estep_fused8_defer_f64(const double *Y, int64_t ldy, const double *Wt, int64_t ldw, const double *gram,
                                  const double *ynorm2, const double *wmu, const double *ymu,
                                  const uint16_t *state_masks, const uint16_t *state_parents,
                                  const int32_t *size_offsets_host, int64_t S, int64_t gamma,
                                  const pm_bsc_estep_params *params_host, int64_t N, int64_t D, int64_t H,
                                  int64_t Hprime, int mode, int32_t *cand, double *logpj, int64_t ldl, double *lse,
                                  double *expect, int64_t lde, double *stats, int64_t D_stats, uint16_t *nz_idx,
                                  double *nz_val, double *records, int part, void *stream);
int pm_bsc_defer_apply_f64(const double *lse, const double *cut, const int32_t *cand, const double *records,
                           uint16_t *nz_idx, const double *nz_val, double *expect, int64_t lde, double *stats,
                           const pm_bsc_estep_params *params_host, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                           void *stream);
/* Wp (the leading H x D block of `stats`) += sum_n sum_t nz_val[n,t] . Y[n,:] into row nz_idx[n,t]  -- my_Wp of
 * bsc_et.py:339-363 from the non-zero lists; returns at once on the device when scalars[3] of `stats` is non-zero (some
 * list overflowed: pm_gemm_tn_acc_gated_f64 on `expect` does the work then).  H <= 256. */
int pm_bsc_wp_sparse_f64(const uint16_t *nz_idx, const double *nz_val, const double *Y, int64_t ldy, double *stats,
                         int64_t N, int64_t H, int64_t D, void *stream);
/* The dense rows pm_bsc_estep_fused8_nz_f64 did not store, for the dense product that runs when some list overflowed:
 * expect[n, :] = 0, then expect[n, nz_idx[n,t]] = nz_val[n,t], for every datapoint whose list is complete (slot 0 is not
 * PM_BSC_NZ_OVERFLOW).  Decided on the device like the products themselves: returns at once unless *gate (scalars[3]) is
 * non-zero.  Enqueue it between pm_bsc_wp_sparse_f64 and pm_gemm_tn_acc_gated_f64 (or use pm_bsc_wp_sparse_expand_f64). */
int pm_bsc_expand_lists_gated_f64(const uint16_t *nz_idx, const double *nz_val, double *expect, int64_t lde,
                                  int64_t N, int64_t H, const double *gate, void *stream);
/* pm_bsc_wp_sparse_f64 and pm_bsc_expand_lists_gated_f64 in ONE launch (what the M-step enqueues): the sparse product, or --
 * scalars[3] of `stats` non-zero -- the completion of `expect` for the dense product behind it. */
int pm_bsc_wp_sparse_expand_f64(const uint16_t *nz_idx, const double *nz_val, const double *Y, int64_t ldy, double *stats,
                                double *expect, int64_t lde, int64_t N, int64_t H, int64_t D, void *stream);
/* The same accumulation for any model whose statistics start with Wp = E[s]^T Y (DSC / TSC, dsc_et.py:703-735): Wp (H x D,
 * leading dimension ldw) and the device-side gate (a double: non-zero = skip) are given explicitly. */
int pm_wp_sparse_f64(const uint16_t *nz_idx, const double *nz_val, const double *Y, int64_t ldy, double *Wp, int64_t ldw,
                     const double *gate, int64_t N, int64_t H, int64_t D, void *stream);
/* The transposed output, no gate: C (D x H, leading dimension ldc) += Y^T . V with the rows of V (N x H) given as lists --
 * the listed rows of GSC's contraction [Y | xpt_s | xpt_sz]^T . xpt_sz (gsc_et.py:592-625); rows with an empty list
 * contribute nothing here (pm_gemm_tn_acc_rows_f64 takes them). */
int pm_wp_sparse_t_f64(const uint16_t *nz_idx, const double *nz_val, const double *Y, int64_t ldy, double *C, int64_t ldc,
                       int64_t N, int64_t H, int64_t D, void *stream);

/* Fast-path twin of pm_bsc_mstep_rows_f64 (same outputs, same `stats` layout). */
int pm_bsc_mstep_rows16_f64(const double *logpj, int64_t ldl, const double *lse, double lse_cut,
                            const int32_t *cand, const uint16_t *state_masks, int64_t S,
                            const pm_bsc_estep_params *params_host, int64_t N, int64_t H, int64_t D,
                            int64_t Hprime, double *expect, int64_t lde, double *stats, void *stream);
/* ... that also leaves the non-zeros of every E[s] row as a list (format of pm_bsc_estep_fused8_nz_f64; rows with more
 * than PM_BSC_NZ_MAX non-zeros count in scalars[3]).  The M-step after a data-truncation step.  Unlike that entry, this one
 * ALWAYS stores the dense row in `expect` and never writes PM_BSC_NZ_OVERFLOW into slot 0: the list of a row with more than
 * PM_BSC_NZ_MAX non-zeros holds its first PM_BSC_NZ_MAX.  Follow it with pm_bsc_wp_sparse_f64 (gated on scalars[3]) and the dense
 * product on `expect`, never with pm_bsc_wp_sparse_expand_f64 / pm_bsc_expand_lists_gated_f64, which would rebuild such a row
 * from its truncated list.  A cut datapoint gets a zero row and an empty list. */
int pm_bsc_mstep_rows16_nz_f64(const double *logpj, int64_t ldl, const double *lse, double lse_cut,
                               const int32_t *cand, const uint16_t *state_masks, int64_t S,
                               const pm_bsc_estep_params *params_host, int64_t N, int64_t H, int64_t D,
                               int64_t Hprime, double *expect, int64_t lde, double *stats, uint16_t *nz_idx,
                               double *nz_val, void *stream);

/* Host-only query (no device call, except for the compute units of the current device when `cus` <= 0 under
 * PM_BSC_PLAN_FUSED8): the launch that a Binary Sparse Coding entry point would make for N >= 1 datapoints of this shape; the
 * launchers, the *_supported predicates and pm_bsc_fused8_main_rows take every one of these decisions from the same functions.
 * `which`: PM_BSC_PLAN_SELECT (pm_bsc_select_f64), _ESTEP (pm_bsc_estep_f64), _MSTEP_ROWS (pm_bsc_mstep_rows_f64),
 * _SELECT_ESTEP (pm_bsc_select_estep_f64), _MSTEP_ROWS16 (pm_bsc_mstep_rows16_f64; with PM_BSC_PLAN_LISTS _nz_f64), _FUSED
 * (pm_bsc_estep_fused_f64), _FUSED8 (pm_bsc_estep_fused8_f64; with PM_BSC_PLAN_LISTS _nz_f64 and _defer_f64).
 * `flags`: the entry's `mode` argument in bits 0..4 (SELECT_ESTEP, FUSED, FUSED8: at least one of bits 0 and 1),
 * PM_BSC_PLAN_STATS (`stats` given: FUSED, FUSED8), PM_BSC_PLAN_LISTS (`nz_idx` given: MSTEP_ROWS16, FUSED8).
 * `S`: the length of the state table handed in.  `gamma` is read where the entry takes it (SELECT_ESTEP, FUSED, FUSED8), and
 * by MSTEP_ROWS for the length of the pair lists: sum_g C(Hprime, g) g^2 when S is the complete state set of sizes
 * 2 .. gamma, else the upper bound S gamma^2.  `D` is read by FUSED and FUSED8 (the K dimension).  `cus`: compute units for
 * the FUSED8 split, <= 0: those of the current device (256 when there is none).
 * out[0..PM_BSC_PLAN_LEN):
 *   0 family       PM_BSC_FAMILY_WAVE (one wavefront per datapoint: bsc_kernels.hip), _LANES16 (sixteen lanes per datapoint:
 *                  bsc_rows16.hip), _FUSED (bsc_fused.hip), _FUSED8 (bsc_fused8.hip)
 *   1 VPL          latents per lane: SELECT 1, 2, 4, 8, 16 (H <= 64, 128, 256, 512, 1024); LANES16 1, 2, 4, 8, 16, 32
 *                  (H <= 16, 32, 64, 128, 256, 512); else 0
 *   2 NJ           16-latent column blocks per wavefront: FUSED 8 (H <= 128) or 16, FUSED8 8; else 0
 *   3 HP, 4 GAMMA  FUSED8: the instantiation (5 .. 8; 3 or 4); else 0
 *   5 FULL         FUSED: H == 16 NJ; FUSED8: H == 256 (no shadow rows of W); else 0
 *   6 MSTATS       FUSED, FUSED8: statistics in the same pass; SELECT_ESTEP: the E-step instantiation (mode bit 1);
 *                  MSTEP_ROWS16: the list-writing instantiation
 *   7 LDS bytes    dynamic shared memory of the launch (FUSED8: of the main launch)
 *   8 grid         workgroups (FUSED8: of both launches together)
 *   9 main rows, 10 main grid, 11 TAIL rows, 12 TAIL grid, 13 TAIL LDS bytes      FUSED8 only (else 0): the leading rows the
 *                  128-row main launch takes -- whole rounds of `cus` workgroups; everything when the ragged round is at
 *                  least 70 % full or exceeds two rounds of 16-row TAIL workgroups (2 cus 16 rows) -- and the rest
 * Returns PM_OK, PM_EINVAL (null `out`, unknown `which` or flag, H, Hprime or N < 1, S < 0; D < 1 where D is read; no mode
 * bit 0 or 1, gamma outside 1 .. Hprime with mode bit 1, STATS without mode bit 1, LISTS without STATS) or PM_ERANGE exactly
 * where the launcher returns it for the shape: Hprime > H, H > PM_MAX_H, Hprime > PM_MAX_HPRIME, S > 65535 or the LDS layout
 * above 160 KB (WAVE); !pm_bsc_rows16_supported, lists with !pm_bsc_rows16_nz_supported (LANES16); !pm_bsc_fused_supported,
 * mode bits above 1, STATS with Hprime > 8 (FUSED); !pm_bsc_fused8_supported, !pm_bsc_fused8_whole_shard, mode bits above 1
 * (FUSED8); a value of out[] beyond INT32_MAX (a shard of more than 2^31 rows). */
#define PM_BSC_PLAN_SELECT 0
#define PM_BSC_PLAN_ESTEP 1
#define PM_BSC_PLAN_MSTEP_ROWS 2
#define PM_BSC_PLAN_SELECT_ESTEP 3
#define PM_BSC_PLAN_MSTEP_ROWS16 4
#define PM_BSC_PLAN_FUSED 5
#define PM_BSC_PLAN_FUSED8 6
#define PM_BSC_PLAN_MODE 31
#define PM_BSC_PLAN_STATS 32
#define PM_BSC_PLAN_LISTS 64
#define PM_BSC_FAMILY_WAVE 1
#define PM_BSC_FAMILY_LANES16 2
#define PM_BSC_FAMILY_FUSED 3
#define PM_BSC_FAMILY_FUSED8 4
#define PM_BSC_PLAN_LEN 14
int pm_bsc_plan(int which, int64_t H, int64_t D, int64_t Hprime, int64_t S, int64_t gamma, int flags, int64_t N, int cus,
                int32_t *out);

/* ---------------------------------------------------------------------------------------
 * Maximal Causes Analysis (prosper/em/camodels/mca_et.py)
 * ------------------------------------------------------------------------------------- */

/* R[n,h] = sum_d max(W[h,d] - Y[n,d], 0) = sum_d |max(W_hd, y_d) - y_d|: the candidate-selection
 * score of mca_et.py:104-106 (W (H,D) row-major).  Candidates = the Hprime SMALLEST per row,
 * ascending: pm_bsc_select_estep_f64 with mode = 1|4|8 (select, smallest-first, raw scores). */
int pm_mca_select_scores_f64(const double *Y, int64_t ldy, const double *W, int64_t ldw, double *R,
                             int64_t ldr, int64_t N, int64_t H, int64_t D, void *stream);

/* Scalars of one MCA step (mca_et.py:142-149, 213-221) or MMCA step (mmca_et.py:156-168, 251-262). */
typedef struct pm_mca_params {
    double pil_bar;   /* log(pi / (1 - pi))                                 */
    double pre1;      /* -1 / (2 sigma^2)                                   */
    double beta;      /* 1 / T (applied to the log-joints in the M-step)    */
    double inv_rho;   /* 1 / rho, rho = 1 / (1 - 1 / max(T, 1.05)) (MMCA: T bound 1.2, rho in [1, 35]) */
    double signed_w;  /* 0: MCA (W > 0).  1: MMCA, signed W (prosper/em/camodels/mmca_et.py): Wrho holds
                         sign(W)|W|^rho, Wrm1 holds |W|^(rho-1); Wbar_sd = sign(t)|t|^(1/rho), t = sum Wrho;
                         the M-step factor is min(1, (|W_jd| / |Wbar_sd|)^(rho-1)) (mmca_et.py:321-324) */
} pm_mca_params;

/* E_step, mca_et.py:114-179.  scores = Y.W^T (pm_gemm_nt_f64), wnorm2 = |W_h|^2 (contiguous),
 * Wrho = W^rho (H,D).  Multi-cause states use Wbar_sd = (sum_{j in s} Wrho[c_j,d])^(1/rho).
 * Outputs logpj (N,1+H+S), lse1 = log sum_k exp(logpj), lseb = log sum_k exp(beta*logpj). */
int pm_mca_estep_f64(const double *scores, int64_t lds, const double *wnorm2, const double *ynorm2,
                     const double *Y, int64_t ldy, const double *Wrho, const int32_t *cand,
                     const uint16_t *state_masks, int64_t S, const pm_mca_params *params_host, int64_t N,
                     int64_t H, int64_t D, int64_t Hprime, double *logpj, int64_t ldl, double *lse1,
                     double *lseb, void *stream);

/* Packed MCA statistics (float64): [ G1 = Q1^T.Y (H*D) | Wp_multi (H*D) | Wq_multi (H*D) |
 * q1sum (H) | scalars: sum E|s| (pi), sum_nk q e (sigma), sum lse1 (Q), kept count ].
 * Wp = G1 * W^2 + Wp_multi, Wq = q1sum (x) 1 * W^2 + Wq_multi (mca_et.py:293-321).
 * Those 3*H*D + H + 4 entries are the result (and what a multi-GPU job all-reduces); pm_mca_stats_len also
 * counts a scratch tail of 7 * 2*H*D entries: the kernels accumulate [Wp_multi | Wq_multi] once per XCD (one L2
 * each) and fold the copies into the documented slot, clearing the tail, before they return. */
#define PM_MCA_NSCALARS 4
int64_t pm_mca_stats_len(int64_t H, int64_t D);

/* Per-datapoint part of M_step, mca_et.py:236-327: q = exp(beta*logpj - lseb) for datapoints
 * with lseb[n] >= lse_cut; writes the singleton weights q1 (N,H) (zero rows for cut datapoints;
 * G1 = q1^T.Y is then one pm_gemm_tn_acc_f64 into stats[0..H*D)), scatters the multi-cause
 * terms Aid (mca_et.py:309) into Wp_multi / Wq_multi, accumulates the scalars.  W_new = Wp/Wq is
 * an element-wise ratio, so only weights that underflow to 0 (as in the reference) are dropped.
 * Wrm1 = W^(rho-1) (H,D).  `stats` is accumulated into (the caller zeroes it once per EM step).  Hprime <= PM_MAX_HPRIME
 * (16); any D up to 2^20: the observed dimensions are walked in slabs, one launch each, whose width follows the register
 * tile of Hprime -- 512 at Hprime <= 8, 256 at Hprime 9..12, 128 at Hprime 13..16 (pm_mca_plan: PM_MCA_PLAN_MSTEP_ROWS).
 * The slab that starts at dimension 0 writes q1 and adds q1sum and the scalars; every slab adds its columns of Wp_multi /
 * Wq_multi. */
int pm_mca_mstep_rows_f64(const double *logpj, int64_t ldl, const double *lse1, const double *lseb,
                          double lse_cut, const double *Y, int64_t ldy, const double *Wrho,
                          const double *Wrm1, const int32_t *cand, const uint16_t *state_masks, int64_t S,
                          const pm_mca_params *params_host, int64_t N, int64_t H, int64_t D,
                          int64_t Hprime, double *q1, int64_t ldq, double *stats, void *stream);

/* E_step and the per-datapoint part of M_step in one pass (no data truncation: every datapoint is
 * kept): outputs of pm_mca_estep_f64 plus q1 / stats of pm_mca_mstep_rows_f64, with every multi-cause
 * power evaluated once instead of twice (mca_et.py:114-179 + 236-327, mmca_et.py:126-199 + 274-347).
 * D <= 512, Hprime <= 12.  `stats` is accumulated into (caller zeroes it). */
int pm_mca_estep_mstats_f64(const double *scores, int64_t lds, const double *wnorm2, const double *ynorm2,
                            const double *Y, int64_t ldy, const double *Wrho, const double *Wrm1,
                            const int32_t *cand, const uint16_t *state_masks, int64_t S,
                            const pm_mca_params *params_host, int64_t N, int64_t H, int64_t D,
                            int64_t Hprime, double *logpj, int64_t ldl, double *lse1, double *lseb,
                            double *q1, int64_t ldq, double *stats, void *stream);
/* DEFERRED statistics for a data-truncation step (mca_et.py:248-262 keeps the N_use datapoints with the largest
 * log-denominator of the annealed weights; which ones is known only after every rank's E-step).
 * pm_mca_estep_mstats_defer_f64 is pm_mca_estep_mstats_f64 that, given `defer_rec` (N x Hprime x D doubles) and
 * `defer_sc` (N x 4), accumulates NOTHING into `stats`: per datapoint it leaves the Aid block of mca_et.py:309 (row j = its
 * j-th candidate: what it would have added to Wq, and times y to Wp) in defer_rec, [sum q |s|, sum q e, log sum exp(logpj), -]
 * in defer_sc, and the singleton posteriors in q1 as always.  Both NULL: exactly pm_mca_estep_mstats_f64.
 * pm_mca_defer_apply_f64 then adds the records of the datapoints with lseb[n] >= *cut (a DEVICE double: the radix
 * select's result never visits the host) into `stats` -- what the in-pass statistics of the kept datapoints would have been
 * (mca_et.py:274-327) -- and zeroes the q1 rows of the others, so that the G1 = q1^T Y product behind it
 * (pm_gemm_tn_acc_f64) sees kept datapoints only.  H, D <= 512, Hprime <= 12. */
int pm_mca_estep_mstats_defer_f64(const double *scores, int64_t lds, const double *wnorm2, const double *ynorm2,
                                  const double *Y, int64_t ldy, const double *Wrho, const double *Wrm1,
                                  const int32_t *cand, const uint16_t *state_masks, int64_t S,
                                  const pm_mca_params *params_host, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                                  double *logpj, int64_t ldl, double *lse1, double *lseb, double *q1, int64_t ldq,
                                  double *stats, double *defer_rec, double *defer_sc, void *stream);
int64_t pm_mca_defer_apply_work_len(int64_t H, int64_t D);      /* doubles of `work` (per-group partial sums, no atomics) */
int pm_mca_defer_apply_f64(const double *lseb, const double *cut, const double *Y, int64_t ldy, const int32_t *cand,
                           const double *records, const double *scalars, double *q1, int64_t ldq, double *stats,
                           double *work, int64_t N, int64_t H, int64_t D, int64_t Hprime, void *stream);
/* The per-step tables of the MCA / MMCA kernels from W^T (H x D, already clamped by check_params): tabs = [ W^T | sign(W) |W|^rho |
 * |W|^(rho-1) ] (three H x D planes; mca_et.py:218-227, mmca_et.py:250-260 compute them with NumPy on the host) and
 * wnorm2[h] = |W_h|^2.  The caller keeps the reference's assertions (finite logarithms, W^rho > 1e-86) on its host copy. */
int pm_mca_tables_f64(const double *wt, int64_t H, int64_t D, double rho, double *tabs, double *wnorm2, void *stream);
/* The element-wise W update of MCA_ET.M_step (mca_et.py:333-348) from the all-reduced `stats`
 * [G1 (H,D) | Wp_m (H,D) | Wq_m (H,D) | q1sum (H) | ...] and the current W^T (H,D): wt_new = (G1 W^2 + Wp_m) / (q1sum W^2 + Wq_m),
 * 0 / tiny where the denominator is below the smallest normal double; wt_clamped (or NULL) = max(wt_new, w_tol), what
 * check_params (mca_et.py:44-55) makes of it at the top of the next step. */
int pm_mca_w_update_f64(const double *stats, const double *wt, int64_t H, int64_t D, double w_tol, double *wt_new,
                        double *wt_clamped, void *stream);

/* Host-only query (no device call): the launch that pm_mca_estep_f64 (`which` = PM_MCA_PLAN_ESTEP), pm_mca_mstep_rows_f64
 * (PM_MCA_PLAN_MSTEP_ROWS), pm_mca_estep_mstats_f64 / pm_mca_estep_mstats_defer_f64 (PM_MCA_PLAN_FUSED; `defer`: records
 * given) or pm_mca_defer_apply_f64 (PM_MCA_PLAN_DEFER_APPLY; S, signed_w, inv_rho, defer not read) would make for N >= 1
 * datapoints; the launchers take every one of these decisions from the same function.  out[0..PM_MCA_PLAN_LEN):
 *   0 DPL      observed dimensions per lane of the instantiation (M-step: of the first slab)
 *   1 HP       height of the register tile V[HP][DPL] (4 / 8 / 12 / 16); E-step and deferred apply: Hprime
 *   2 ROOT     21 / 6: the log / exp-free power of that rho, 0: the table (fused pass: uniform-exponent) power
 *   3 paired   fused pass: 1 where the state loop takes two states per trip
 *   4 wavefronts per workgroup    5 dynamic LDS bytes of a workgroup    6 grid (deferred apply: of the scatter kernel)
 *   7 slab width, 8 slab count, 9 DPL of the last slab               (PM_MCA_PLAN_MSTEP_ROWS, else 0)
 *  10 `defer` as given                                               (PM_MCA_PLAN_FUSED, else 0)
 *  11 HR latent rows per scatter workgroup, 12 latent ranges, 13 datapoint groups, 14 grid of the q1 kernel
 *                                                                    (PM_MCA_PLAN_DEFER_APPLY, else 0)
 *  15 reserved (0)
 * PM_EINVAL: out NULL, unknown `which`, a non-positive dimension, S < 0, N < 1.  PM_ERANGE exactly where the launcher
 * returns it for the shape. */
#define PM_MCA_PLAN_ESTEP 0
#define PM_MCA_PLAN_MSTEP_ROWS 1
#define PM_MCA_PLAN_FUSED 2
#define PM_MCA_PLAN_DEFER_APPLY 3
#define PM_MCA_PLAN_LEN 16
int pm_mca_plan(int which, int64_t H, int64_t D, int64_t Hprime, int64_t S, int signed_w, double inv_rho, int64_t N,
                int defer, int32_t *out);

/* ---------------------------------------------------------------------------------------
 * Discrete Sparse Coding (prosper/em/camodels/dsc_et.py, DSC_ET): K-ary latents
 * ------------------------------------------------------------------------------------- */
#define PM_DSC_MAX_K 8      /* latent values incl. the zero value */

/* Scalars of one DSC step (dsc_et.py:376-388, 533-558). */
typedef struct pm_dsc_params {
    int32_t K;                       /* number of latent values                                   */
    int32_t K0;                      /* index of the value 0 (dsc_et.py:153)                      */
    double values[PM_DSC_MAX_K];     /* the latent values `states`                                */
    double logpi[PM_DSC_MAX_K];      /* log pi_k (selection only)                                 */
    double pre1;                     /* -1 / (2 sigma^2) (selection only)                         */
    double ecoef;                    /* beta * pre1: logpj = ecoef * e + pscale * prior           */
    double pscale;                   /* beta if anneal['anneal_prior'] else 1 (dsc_et.py:579-584)  */
    int32_t flags;                   /* PM_DSC_TABLE_ONLY | PM_DSC_LAST_POSITION (Ternary Sparse Coding) */
    int32_t reserved;
} pm_dsc_params;

/* select_Hprimes of DSC (dsc_et.py:347-410; `params_host` given) or TSC (tsc_et.py:142-213; `params_host` NULL) in ONE pass
 * over the scores: the ranking values of pm_dsc_select_scores_f64 / pm_tsc_select_scores_f64 are formed in registers and
 * ranked there (same values, same tie rules as the two-launch form); TSC candidates come out as latents (state % H).
 * Where pm_xsc_select_supported(H, Hprime, tsc) (TSC: H in {16, 32, 64, 128, 256}), else PM_ERANGE. */
int pm_xsc_select_supported(int64_t H, int64_t Hprime, int tsc);
int pm_xsc_select_f64(const double *scores, int64_t lds, const double *gram, const pm_dsc_params *params_host, int64_t N,
                      int64_t H, int64_t Hprime, int32_t *cand, void *stream);

/* Ternary Sparse Coding (prosper/em/camodels/tsc_et.py) runs on the DSC kernels with two flags:
 * PM_DSC_TABLE_ONLY     logpj has one column per row of the state table and nothing else (tsc_et.py:340-349:
 *                       the table holds the null and one-cause states too; no global singleton block);
 * PM_DSC_LAST_POSITION  a latent that occurs twice among a datapoint's candidates contributes to Wp / Wq
 *                       only through its LAST position, as NumPy's fancy-index `+=` does (tsc_et.py:471-475). */
#define PM_DSC_TABLE_ONLY 1
#define PM_DSC_LAST_POSITION 2

/* select_Hprimes of TSC, tsc_et.py:142-213: R (N, 2H) = minus the squared distance of every one-cause
 * state up to |y|^2 -- R[n,h] = -(G_hh + 2 scores[n,h]) (value -1), R[n,H+h] = -(G_hh - 2 scores[n,h])
 * (value +1).  The candidates are the latents (index mod H) of the Hprime largest entries, best last:
 * pm_bsc_select_estep_f64(mode = 1|8) on R with 2H columns. */
int pm_tsc_select_scores_f64(const double *scores, int64_t lds, const double *gram, int64_t N, int64_t H,
                             double *R, int64_t ldr, void *stream);

/* select_Hprimes, dsc_et.py:347-410: R[n,h] = -max_{k != K0} (pre1 (v_k^2 G_hh - 2 v_k scores[n,h]) + log pi_k),
 * the negated best singleton log-joint of latent h up to per-datapoint constants.  The candidates are
 * the Hprime smallest R, best first: pm_bsc_select_estep_f64(mode = 1|4|8) on R. */
int pm_dsc_select_scores_f64(const double *scores, int64_t lds, const double *gram,
                             const pm_dsc_params *params_host, int64_t N, int64_t H, double *R, int64_t ldr,
                             void *stream);

/* E_step, dsc_et.py:492-585.  state_idx (S,Hprime) uint8: index into `values` of every entry of the
 * multi-cause state matrix (itertools.product order, dsc_et.py:56-63); prior = pre_F (1 + (K-1)H + S)
 * (dsc_et.py:539-558).  Columns of logpj: [null | singletons by non-zero value then latent | states].
 * Also writes lse = log sum_k exp(logpj). */
int pm_dsc_estep_f64(const double *scores, int64_t lds, const double *gram, const double *ynorm2,
                     const int32_t *cand, const uint8_t *state_idx, int64_t S, const double *prior,
                     const pm_dsc_params *params_host, int64_t N, int64_t H, int64_t Hprime, double *logpj,
                     int64_t ldl, double *lse, void *stream);

/* Packed DSC statistics (float64): [ Wp = E[s]^T.Y (H*D, filled by pm_gemm_tn_acc_f64) |
 * Wq upper triangle, multi-cause part (H*H) | Wq diagonal, singleton part (H) |
 * expected counts of every non-zero value (PM_DSC_MAX_K, entry K0 unused) |
 * sum_nk q e, sum lse, kept datapoints, rows whose non-zero list overflowed (pm_dsc_mstep_rows_nz_f64) ]. */
int64_t pm_dsc_stats_len(int64_t H, int64_t D);

/* Per-datapoint part of M_step, dsc_et.py:660-735, for datapoints with lse[n] > lse_cut (strict,
 * dsc_et.py:832): writes E[s] rows into expect (N,H) (zero rows for cut datapoints) and accumulates
 * the statistics above into `stats` (caller zeroes it once per EM step). */
int pm_dsc_mstep_rows_f64(const double *logpj, int64_t ldl, const double *lse, double lse_cut,
                          const int32_t *cand, const uint8_t *state_idx, int64_t S, const double *prior,
                          const pm_dsc_params *params_host, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                          double *expect, int64_t lde, double *stats, void *stream);
/* The same pass that also leaves every E[s] row as a list of its non-zeros (format of pm_bsc_estep_fused8_nz_f64:
 * N x PM_BSC_NZ_MAX indices / values, unused index slots 0xFFFF; a longer row counts in the last scalar of `stats`), for
 * pm_wp_sparse_f64.  Only where pm_dsc_rows16_supported(...) holds (the sixteen-lanes-per-datapoint kernel). */
int pm_dsc_rows16_supported(int64_t H, int64_t Hprime, int64_t S, int64_t K, int flags);
int pm_dsc_mstep_rows_nz_f64(const double *logpj, int64_t ldl, const double *lse, double lse_cut,
                          const int32_t *cand, const uint8_t *state_idx, int64_t S, const double *prior,
                          const pm_dsc_params *params_host, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                          double *expect, int64_t lde, double *stats, uint16_t *nz_idx, double *nz_val,
                             void *stream);
/* The same pass with the data-truncation cut read on the DEVICE (round 6): `cut_dev` (one double, e.g. what pm_kth_final_f64
 * left, adjusted as dsc_et.py:832 / tsc_et.py:433-440 ask) replaces `lse_cut` when it is not NULL -- the M-step of a
 * truncation step then has no host round trip between the radix select and its row pass.  nz_idx / nz_val may be NULL
 * (then exactly pm_dsc_mstep_rows_f64). */
int pm_dsc_mstep_rows_cutp_f64(const double *logpj, int64_t ldl, const double *lse, double lse_cut, const double *cut_dev,
                               const int32_t *cand, const uint8_t *state_idx, int64_t S, const double *prior,
                               const pm_dsc_params *params_host, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                               double *expect, int64_t lde, double *stats, uint16_t *nz_idx, double *nz_val, void *stream);

/* pm_dsc_estep_f64 that ALSO produces the M-step's row statistics -- what pm_dsc_mstep_rows_nz_f64 computes from the stored
 * log-joints (dsc_et.py:587-774: E[s] rows, their non-zero lists, the candidates' second moments -> Wq, qdiag, the value
 * counts, the sigma / likelihood scalars) -- from the exponentials its log-sum-exp evaluates anyway: no second pass over the
 * log-joints.  For the E-step of an EM iteration with no data truncation ahead (every datapoint kept); `stats` is
 * accumulated into (caller zeroes it), `expect` / `nz_*` as in pm_dsc_mstep_rows_nz_f64.  Sixteen lanes per datapoint:
 * where pm_dsc_estep_mstats_supported(H, Hprime, S, K, flags) holds (else PM_ERANGE: run the two passes). */
int pm_dsc_estep_mstats_supported(int64_t H, int64_t Hprime, int64_t S, int64_t K, int flags);
int pm_dsc_estep_mstats_f64(const double *scores, int64_t lds, const double *gram, const double *ynorm2, const int32_t *cand,
                            const uint8_t *state_idx, int64_t S, const double *prior, const pm_dsc_params *params_host,
                            int64_t N, int64_t H, int64_t D, int64_t Hprime, double *logpj, int64_t ldl, double *lse,
                            double *expect, int64_t lde, double *stats, uint16_t *nz_idx, double *nz_val, void *stream);

/* Host-only query (no device call): the launch that pm_dsc_estep_f64 (`which` = PM_DSC_PLAN_ESTEP), pm_dsc_estep_mstats_f64
 * (PM_DSC_PLAN_ESTEP_MSTATS) or pm_dsc_mstep_rows_f64 / _nz_f64 / _cutp_f64 (PM_DSC_PLAN_MSTEP_ROWS) would make for N >= 1
 * datapoints of this shape; the launchers switch on the same function.  out[0..7]:
 *   0 kernel family   PM_DSC_PLAN_LANES16 (sixteen lanes per datapoint) or PM_DSC_PLAN_WAVE (one wavefront per datapoint)
 *   1 MAXHP           8 or PM_MAX_HPRIME: the instantiation's bound on Hprime
 *   2 VPL             8 or 16 latents per lane (sixteen-lane family; 0 for the wavefront family)
 *   3 KM              value counters per lane: 4 or PM_DSC_MAX_K (mstats), PM_DSC_MAX_K (mstep_rows), 0 (estep: none)
 *   4 stage           1: the log-prior table is held in LDS, 0: read from global memory
 *   5 NT              entries of the energy-term tables, 0: the generic walk over all positions (always 0 for mstep_rows).
 *                     A state table with more than three non-zero positions in some state turns the tables off inside
 *                     the kernel; that is not part of the plan.
 *   6 LDS bytes       dynamic shared memory of the launch
 *   7 grid            workgroups (sixteen-lane family: 16 datapoints each per sweep; wavefront family: 4)
 * Returns PM_OK, PM_EINVAL (null `out`, a size < 1, S < 0, K outside 2..PM_DSC_MAX_K, unknown `which`) or PM_ERANGE where
 * the launcher returns PM_ERANGE for the shape (Hprime > H, Hprime > PM_MAX_HPRIME, H > 65536, LDS; mstats where
 * pm_dsc_estep_mstats_supported is 0).  pm_dsc_mstep_rows_nz_f64 with lists needs family PM_DSC_PLAN_LANES16. */
#define PM_DSC_PLAN_ESTEP 0
#define PM_DSC_PLAN_ESTEP_MSTATS 1
#define PM_DSC_PLAN_MSTEP_ROWS 2
#define PM_DSC_PLAN_LANES16 1
#define PM_DSC_PLAN_WAVE 2
int pm_dsc_plan(int which, int64_t H, int64_t Hprime, int64_t S, int64_t K, int flags, int64_t N, int32_t *out);

/* ---------------------------------------------------------------------------------------
 * Gaussian (spike-and-slab) Sparse Coding, scalar noise (prosper/em/camodels/gsc_et.py, GSC)
 * ------------------------------------------------------------------------------------- */

/* Shapes the GSC kernel covers: H <= 512, gamma <= 8 (g x g systems solved in registers; instantiated for 2, 3, 4, 6, 8). */
int pm_gsc_supported(int64_t H, int64_t Hprime, int64_t gamma);

/* Host-only query (no device call): the launch that pm_gsc_estep_f64 and its siblings (`which` = PM_GSC_PLAN_ESTEP; `flags`:
 * PM_GSC_PLAN_LPJ for pm_gsc_estep_lpj_f64, PM_GSC_PLAN_LPJ | PM_GSC_PLAN_BLOCKS for pm_gsc_estep_lpj_blocks_f64,
 * PM_GSC_PLAN_LISTS for pm_gsc_estep_lists_f64), pm_gsc_list_pairs_f64 (PM_GSC_PLAN_LIST_PAIRS: H and N are read),
 * pm_gsc_pack_stats_f64 (PM_GSC_PLAN_PACK: H) or pm_gsc_component_scores_f64 (PM_GSC_PLAN_COMPONENT_SCORES: H, N) would make
 * for N >= 1 datapoints; the launchers take every one of these decisions from the same function.  `S`: the length of the
 * state table handed in (it may be a prefix of the full table of Hprime and gamma).  `cus`: compute units of the device,
 * <= 0 for the 256 the launcher assumes when it cannot ask.  `D` is read with PM_GSC_PLAN_LISTS only: > 0 adds what
 * pm_gsc_lists_supported asks of the M-step's contraction ((D + 2 H) % 128 == 0, H % 128 == 0), <= 0 plans the launch alone.
 * out[0..PM_GSC_PLAN_LEN):
 *   0 VPL          latents per lane of gsc_estep_kernel: 1, 2, 4, 8, 16, 32 (H <= 16, 32, 64, 128, 256, 512; LIST: 8 or 16)
 *   1 GMAX         size of the g x g systems in registers: 2, 3, 4, 6, 8 (gamma <= 2, 3, 4, 5..6, 7..8)
 *   2 form         PM_GSC_FORM_PLAIN (column sums by gsc_colsum_kernel, singleton diagonal in registers), _LACC (column sums
 *                  and the whole diagonal of sum xpt_szsz in LDS accumulators: where that layout is <= 53 KB), _LPJ
 *                  (log-joints written; statistics as PLAIN), _LIST (LACC + the row lists)
 *   3 LDS bytes    dynamic shared memory of the launch
 *   4 grid         workgroups (E-step: min(ceil(N / 16), 3 cus), LIST: at least ceil(N / 512))
 *   5 trips        E-step: groups of sixteen datapoints a workgroup walks at most, ceil(ceil(N / 16) / grid); list pairs:
 *                  trips of 512 datapoints per group; else 1
 *   6 colsum       1: gsc_colsum_kernel follows the E-step (PLAIN, LPJ)
 *   7 rows_c, 8 nchunks, 9 groups, 10 rows_per_group     (PM_GSC_PLAN_LIST_PAIRS, else 0): a workgroup owns rows_c rows of
 *                  one of the two products -- the largest divisor of H with rows_c * H <= 16384 -- and rows_per_group datapoints
 * Returns PM_OK, PM_EINVAL (null `out`, unknown `which` or flag, BLOCKS without LPJ, LISTS with LPJ, H < 1, N < 1, E-step:
 * Hprime < 1, S < 0) or PM_ERANGE exactly where the launcher returns it: !pm_gsc_supported, a state table whose LDS layout
 * exceeds 64 KB; LISTS: the LACC layout does not fit, gamma > 3, H <= 64, H > 256 (and the conditions on D above); list
 * pairs: H > 256 or H % 64 != 0; pack: H > 512; component scores: more than INT32_MAX workgroups. */
#define PM_GSC_PLAN_ESTEP 0
#define PM_GSC_PLAN_LIST_PAIRS 1
#define PM_GSC_PLAN_PACK 2
#define PM_GSC_PLAN_COMPONENT_SCORES 3
#define PM_GSC_PLAN_LPJ 1
#define PM_GSC_PLAN_BLOCKS 2
#define PM_GSC_PLAN_LISTS 4
#define PM_GSC_FORM_PLAIN 0
#define PM_GSC_FORM_LACC 1
#define PM_GSC_FORM_LPJ 2
#define PM_GSC_FORM_LIST 3
#define PM_GSC_PLAN_LEN 12
int pm_gsc_plan(int which, int64_t H, int64_t Hprime, int64_t S, int64_t gamma, int64_t D, int flags, int64_t N, int cus,
                int32_t *out);

/* stats (float64): [ sum_n xpt_ss, STRICT upper triangle, multi-cause part (H*H; its diagonal is sum_n xpt_s and is not formed here) |
 *                    sum_n xpt_szsz, both triangles as they are, multi-cause part (H*H) |
 *                    sum_n xpt_s (H) | sum_n xpt_sz (H) | diagonal of sum_n xpt_szsz that is not in the block above (H): the
 *                    singletons', and -- where the kernel keeps its column sums in LDS -- the multi-cause states' too |
 *                    scratch: seven more copies of the first 2*H*H entries ]
 * diag(sum xpt_ss) = sum_n xpt_s (s_h^2 = s_h).  The kernel accumulates the (H,H) blocks per XCD (one L2 each)
 * and folds the copies into the first 2*H*H entries (clearing the scratch) before it returns: the caller zeroes the
 * whole buffer once; the documented entries accumulate across calls as before. */
int64_t pm_gsc_stats_len(int64_t H);

/* The statistics pm_gsc_estep_f64 leaves in `stats` -> [sum xpt_ss (H,H) | sum xpt_szsz (H,H) | sum xpt_s (H) | sum xpt_sz (H)
 * | sum |y|^2] as the M-step all-reduces them (gsc_et.py:603-610, 662-671): xpt_ss mirrored from its upper triangle with
 * sum xpt_s on the diagonal, xpt_szsz as accumulated (it is not symmetric once psi_sq is not) plus the singletons' diagonal.
 * `sum_ynorm2`: device pointer to sum_n |y_n|^2 of the shard.  One launch. */
int pm_gsc_pack_stats_f64(const double *stats, int64_t H, const double *sum_ynorm2, double *out, void *stream);

/* The H- and H x H-sized tail of GSC's M-step for scalar sigma_sq (gsc_et.py:640-713) and the tables of the next
 * E-step, on the device (one workgroup): pi clip, mu, psi_sq (with (sum_ss + eps I)^-1 from pm_spd_inverse_batch_f64),
 * sigma_sq = (sum |y|^2 - trace(xsz_xsz . gram)) / N / D + eps, gram = W_new^T W_new.  `old` / `params`:
 * [pi (H) | mu (H) | psi_sq (H*H) | sigma_sq (1)]; `learn` bits 1 pi, 2 mu, 4 psi_sq, 8 sigma_sq (others copied from `old`).
 * `tables`: 9 x H doubles -- the eight rows pm_gsc_estep_f64 takes and a ninth holding 1 / sigma_sq, which that
 * function reads when it is called with sigma_sq == 0. */
int pm_gsc_mstep_finish_f64(const double *xs_xsz, const double *xsz_xsz, const double *sum_ss, const double *sum_zz,
                            const double *ss_inv, const double *sum_s, const double *sum_sz, const double *sum_yy,
                            const double *gram, const double *old, double N, int64_t D, int64_t H, int learn,
                            double *params, double *tables, void *stream);

/* select_Hprimes + E_step of GSC in one pass (gsc_et.py:721-809, 401-580, 260-398):
 *   scores (N,H) = Y.W;  gram = W^T.W (H,H);  psi_sq (H,H);
 *   tables (8*H): per-latent constants [c0 | c1 | gm | il | kl | ilam | mu | lpi] with
 *     lam = G_hh/s2 + 1/psi_hh, c0 = -(log psi_hh + log lam) - mu^2 G_hh/s2, c1 = 2 mu/s2,
 *     gm = G_hh mu, il = 1/(lam s2^2), kl = 1/(lam s2), ilam = 1/lam, lpi = log(pi/(1-pi))
 *   do_select != 0: candidates = the Hprime best component scores, sorted by latent index,
 *     written to `cand`; otherwise `cand` (sorted) is an input.
 *   sigma_sq == 0: `tables` has a ninth row whose first entry is 1/sigma_sq (left on the device by
 *     pm_gsc_mstep_finish_f64).
 * Outputs: xpt_s, xpt_sz (N,H) and the sums over datapoints accumulated into `stats`
 * (zeroed by the caller).  The (N,H,H) moments of the reference are never materialised.
 * The selection contract: the candidates are the Hprime largest component scores (pm_gsc_component_scores_f64, clamps
 * included), RANKED ON THE SCORE WITH ITS LOW 10 MANTISSA BITS DROPPED -- the kernel carries the latent index in those bits.
 * Equal ranking values resolve towards the larger latent index (the reference's argsort does the same on equal scores).
 * So the selected set equals the reference's whenever the Hprime-th and the (Hprime + 1)-th largest scores differ in the
 * upper 43 bits of the mantissa (or in sign or exponent); scores closer than that may be taken in index order instead. */
int pm_gsc_estep_f64(const double *scores, int64_t lds, const double *gram, const double *psi_sq,
                     const double *ynorm2, const double *tables, const uint16_t *state_masks, int64_t S,
                     int64_t gamma, double beta, double sigma_sq, int64_t N, int64_t H, int64_t Hprime,
                     int do_select, int32_t *cand, double *xpt_s, double *xpt_sz, int64_t ldx,
                     double *stats, void *stream);

/* The same pass, also splitting the rows of xpt_sz for the M-step's contraction over the datapoints
 * [Y | xpt_s | xpt_sz]^T . xpt_sz (gsc_et.py:592-625: my_Wp, the two H x H moment products): a row with at most
 * PM_BSC_NZ_MAX entries above the threshold tables[8 H + 1] leaves them as a list (nz_idx / nz_val, N x PM_BSC_NZ_MAX,
 * format of pm_bsc_estep_fused8_nz_f64; for pm_wp_sparse_t_f64), any other row an empty list and its index in
 * dense_rows[0 .. *dense_count) (for pm_gemm_tn_acc_rows_f64; *dense_count = 0 at launch; order as the workgroups finish).
 * nz_val holds TWO planes of N x PM_BSC_NZ_MAX doubles: xpt_sz at the listed entries, then xpt_s at them (pm_gsc_list_pairs_f64).
 * The threshold is written by pm_gsc_mstep_finish_f64 (2^-57 / N of the smallest |column sum| of xpt_sz over all ranks: what
 * the lists drop is below the rounding of the sums); 0 keeps every row dense.  Where pm_gsc_lists_supported(H, Hprime,
 * gamma, D), else PM_ERANGE. */
int pm_gsc_lists_supported(int64_t H, int64_t Hprime, int64_t gamma, int64_t D);
int pm_gsc_estep_lists_f64(const double *scores, int64_t lds, const double *gram, const double *psi_sq,
                           const double *ynorm2, const double *tables, const uint16_t *state_masks, int64_t S,
                           int64_t gamma, double beta, double sigma_sq, int64_t N, int64_t H, int64_t Hprime,
                           int do_select, int32_t *cand, double *xpt_s, double *xpt_sz, int64_t ldx, double *stats,
                           uint16_t *nz_idx, double *nz_val, int32_t *dense_rows, int32_t *dense_count, void *stream);

/* xs^T xsz and xsz^T xsz of GSC's M-step (gsc_et.py:603-610) over the LISTED datapoints from the lists alone (outer products of
 * a datapoint's listed entries): out[0 .. H*H) += sum_n xs_n xsz_n^T, out[H*H .. 2 H*H) += sum_n xsz_n xsz_n^T over the entries
 * nz_idx lists.  nz_val_s / nz_val: xpt_s / xpt_sz at those entries -- pm_gsc_estep_lists_f64 leaves them as the second and the
 * first plane of its `nz_val` (which therefore holds 2 x N x PM_BSC_NZ_MAX doubles).  The sparse product then streams the D
 * columns of Y only.  H in {64, 128, 192, 256}, else PM_ERANGE. */
int pm_gsc_list_pairs_f64(const uint16_t *nz_idx, const double *nz_val_s, const double *nz_val, int64_t N, int64_t H,
                          double *out, void *stream);

/* The same pass, also writing every state's log-joint -- what GSC.compute_lpj returns (gsc_et.py:811-944): no
 * annealing, prior odds included -- to logpj (N, ldl >= 1 + H + S): [null state ; singletons h = 0..H-1 ; multi-cause
 * states in state_masks order], rows in datapoint order (the reference sorts its cluster order back, :942-944). */
int pm_gsc_estep_lpj_f64(const double *scores, int64_t lds, const double *gram, const double *psi_sq,
                         const double *ynorm2, const double *tables, const uint16_t *state_masks, int64_t S,
                         int64_t gamma, double beta, double sigma_sq, int64_t N, int64_t H, int64_t Hprime,
                         int do_select, int32_t *cand, double *xpt_s, double *xpt_sz, int64_t ldx,
                         double *stats, double *logpj, int64_t ldl, void *stream);

/* ... and every datapoint's un-normalised sums over the multi-cause states -- what GSC.compute_posterior_hprime returns for a
 * data cluster (gsc_et.py:260-398) -- blocks (N, ldb >= 2 Hprime^2 + 2 Hprime + 1):
 * [sum_s p_s [i, k in s] | sum_s p_s (kappa kappa^T + Lambda^-1)_ik | sum_s p_s [i in s] | sum_s p_s kappa_i | sum_s p_s] over the
 * candidate positions i, k in the order of `cand`, p_s = exp(beta lp_s) with the reference's clamp to `tiny`. */
int pm_gsc_estep_lpj_blocks_f64(const double *scores, int64_t lds, const double *gram, const double *psi_sq,
                                const double *ynorm2, const double *tables, const uint16_t *state_masks, int64_t S,
                                int64_t gamma, double beta, double sigma_sq, int64_t N, int64_t H, int64_t Hprime,
                                int do_select, int32_t *cand, double *xpt_s, double *xpt_sz, int64_t ldx, double *stats,
                                double *logpj, int64_t ldl, double *blocks, int64_t ldb, void *stream);

/* GSC.component_scores (gsc_et.py:752-809): singleton log-posteriors without the prior, clamped as the reference
 * clamps them, in the reference's order (gsc_et.py:802-804): NaN and everything below -DBL_MAX -- so -inf too -- become
 * -DBL_MAX, then +inf becomes 0; the E-step kernel's selection applies the same two steps in the same order.
 * out (N, ldo >= H).  `scores`, `ynorm2`, `tables`
 * (rows c0, c1, gm, il are read), `sigma_sq` (> 0) as for pm_gsc_estep_f64. */
int pm_gsc_component_scores_f64(const double *scores, int64_t lds, const double *ynorm2, const double *tables,
                                double sigma_sq, int64_t N, int64_t H, double *out, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------
 * CAModel.inference (prosper/em/camodels/__init__.py:256-375), after compute_lpj
 * ------------------------------------------------------------------------------------- */

/* Per datapoint, from its K = 1 + H + S log-joints (logpj (N, ldl), columns [null ; singletons ; multi-cause states over
 * `cand` (N, Hprime) in state_masks order]): the topK columns of the normalised posterior, descending, ties larger column
 * first (argsort()[..., ::-1], :313) -> top_idx (N, topK) int32, their normalised log-probabilities top_lpc and their
 * log-joints relative to the row maximum top_rel (what the reference reports for logprob=False, :320-323), and the
 * log-marginals log p(s_h = 1 | y) -> marg (N, ldm >= H) (:333-339; the reference's final exp, :367, is the caller's). */
int pm_infer_topk_f64(const double *logpj, int64_t ldl, const int32_t *cand, const uint16_t *state_masks, int64_t N,
                      int64_t H, int64_t Hprime, int64_t S, int64_t topK, int32_t *top_idx, double *top_lpc,
                      double *top_rel, double *marg, int64_t ldm, void *stream);
/* The same for logpj rows with `single_cols` >= H one-cause columns in front of the multi-cause ones -- DSC's K-ary latents
 * (dsc_et.py:927-1059): [null ; (K - 1) H one-cause states, the first non-zero value's block first ; S multi-cause states].
 * `state_masks` then marks the positions at which a state's latent takes the value 1 (the reference's marginal,
 * dsc_et.py:1010-1016: the first value's one-cause state + those multi-cause states); top-K runs over all columns. */
int pm_infer_topk_cols_f64(const double *logpj, int64_t ldl, const int32_t *cand, const uint16_t *state_masks, int64_t N,
                           int64_t H, int64_t Hprime, int64_t S, int64_t single_cols, int64_t topK, int32_t *top_idx,
                           double *top_lpc, double *top_rel, double *marg, int64_t ldm, void *stream);

/* TSC_ET.inference after compute_lpj (tsc_et.py:546-680): logpj (N, ldl >= S) holds ONE log-joint per row of the ternary state
 * table, state_vals (S, Hprime) int8 the latent values -1 / 0 / +1 per candidate position, cand (N, Hprime) may repeat a latent.
 * rank != 0: top_idx (N, topK) = the best states descending by (value, column), and tie[n] = 1 when two of row n's topK + 1
 * best are exactly equal -- the order NumPy's argsort()[::-1] (:626) gives exact ties is not a function of (value, column),
 * so the caller ranks those rows with NumPy and calls again with rank == 0, top_idx given.  Either way: top_lpc / top_post
 * (N, topK) normalised log-probabilities / probabilities; m_out / am_out (N, H; am_out may be NULL) the signed / absolute
 * marginals sum_s p_s v and sum_s p_s |v| written at the candidates in position order (a repeated candidate's last position
 * wins, :640-655); s_out (N, topK, H) int8 the top states written likewise.  Entries of other latents are left as they are. */
int pm_infer_topk_signed_f64(const double *logpj, int64_t ldl, const int32_t *cand, const int8_t *state_vals, int64_t N,
                             int64_t H, int64_t Hprime, int64_t S, int64_t topK, int rank, int32_t *top_idx, double *top_lpc,
                             double *top_post, int32_t *tie, int8_t *s_out, double *m_out, double *am_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Mixture models (prosper/em/mixturemodels/MoG.py, MoP.py; mixture_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * Log-joints + posteriors, MoG.posterior / log_p_y (MoG.py:213-281) and MoP.posterior / log_p_y (MoP.py:176-232), which
 * loop over components in batches of 100 / 500 datapoints:
 *   logpj[n,h] = (S[n,h] + c[h]) * coef + lp[h]      (coef = -beta for MoG, +beta for MoP; lp = beta log pies)
 *   Bq != NULL (MoG, diagonal): S = sum_d y^2 Bq[h,d] + y Bl[h,d]  (Bq = 1/sigma^2, Bl = -2 W^T/sigma^2, Y squared on the fly)
 *   Bq == NULL (MoP):           S = sum_d (rowscale[n] y) Bl[h,d]   (Bl = log W^T; rowscale NULL = 1, else the scale of
 *                               MoP.normalize, MoP.py:236-245 -- its "+1" belongs in c)
 * and in the same kernel the posteriors (N, H): exp(logpj) with no max subtraction, NaN -> DBL_MIN, < DBL_MIN -> DBL_MIN,
 * inf -> DBL_MAX / H, divided by the row sum (MoG.py:222-229).  H <= PM_MAX_H; logpj / post dense (N, H). */
int pm_mix_scores_f64(const double *Y, int64_t ldy, const double *rowscale, const double *Bq, const double *Bl, int64_t ldb,
                      const double *c, double coef, const double *lp, int64_t N, int64_t D, int64_t H, double *logpj,
                      double *post, void *stream);
/* Batched Cholesky of the H covariances S (H, D, D) of a full-covariance MoG, one workgroup per component, through global
 * memory (any D): Linv (H, D, D) = L_h^-1 (lower triangular, zeros above), logdet[h] = log det S_h, status[h] = 0, or
 * status[h] = 1 and logdet[h] = NaN for a component that is not positive definite (Linv_h undefined: the caller inverts it
 * as the reference does, np.linalg.inv + slogdet(...)[1] at MoG.py:249-252).  L_work (H, D, D): scratch.  Replaces the per
 * component inverse and log-determinant of MoG.log_p_y for every positive definite component. */
int pm_mix_chol_f64(const double *S, int64_t D, int64_t H, double *L_work, double *Linv, double *logdet, int32_t *status,
                    void *stream);
/* The full-covariance term of MoG.log_p_y (MoG.py:262-268) for W (H, D) rows w_h, u = y_n - w_h, into S (N, lds >= H):
 * mode[h] == 0 (or mode NULL): B_h = L_h^-1 from pm_mix_chol_f64, S[n,h] = |B_h u|^2; mode[h] == 1: B_h = the transpose of
 * the host inverse Sinv_h, S[n,h] = u Sinv_h u^T.  B (H, D, D), mode (H) int32, both device. */
int pm_mix_maha_f64(const double *Y, int64_t ldy, const double *W, const double *B, const int32_t *mode, int64_t N,
                    int64_t D, int64_t H, double *S, int64_t lds, void *stream);
/* The epilogue of pm_mix_scores_f64 on its own, from a given S (N, lds): logpj and posteriors (N, H) (MoG.py:213-229). */
int pm_mix_posterior_f64(const double *S, int64_t lds, const double *c, double coef, const double *lp, int64_t N, int64_t H,
                         double *logpj, double *post, void *stream);
/* M-step statistics of MoG.M_step (MoG.py:142-202) and MoP.M_step (MoP.py:105-166), one shard, packed as
 *   [colsum P (H) | Y^T P (D, H) | kind 1: (Y*Y)^T P (D, H) | kind 2: Y^T diag(P[:,h]) Y (H, D, D)]
 * kind 0 (MoP): Y^T P with the rows of Y scaled by rowscale (NULL = 1; MoP's normalisation, whose "+1" adds colsum P);
 * kind 1 (MoG diagonal), kind 2 (MoG full): rowscale must be NULL.  The datapoints are cut into pm_mix_stats_chunks fixed
 * chunks whose partial statistics (the column sums of P formed by the workgroups that load P anyway) land in `work`
 * (pm_mix_mstats_work_len doubles) and are added in chunk order: no atomics, the same bits on every run.
 * pm_mix_stats_len: the packed length (-1 for a bad argument). */
int64_t pm_mix_stats_len(int64_t D, int64_t H, int kind);
int64_t pm_mix_stats_chunks(int64_t N, int64_t D, int64_t H, int kind);
int64_t pm_mix_mstats_work_len(int64_t N, int64_t D, int64_t H, int kind);
int pm_mix_mstats_f64(const double *Y, int64_t ldy, const double *P, int64_t ldp, const double *rowscale, int64_t N,
                      int64_t D, int64_t H, int kind, double *work, double *stats, void *stream);

/* ---------------------------------------------------------------------------------------
 * Held-out log-likelihood (loglik_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * Row log-sum-exp of log-joints X (N, ld >= S): v_n = m_n + log sum_s exp(a X[n,s] + o_s - m_n), m_n = max_s (a X[n,s] + o_s),
 * o = col_offset (S values; NULL = 0).  A row that is all -inf gives -inf, a NaN entry gives NaN.  rows_out (N; NULL = not
 * written) receives v, total[0] = sum_n v_n: workgroups add fixed row ranges in a fixed order into work
 * (pm_rows_lse_work_len(N) doubles) and one workgroup adds those in index order -- no atomics, the same bits on every run
 * and in both builds.  N == 0 writes total[0] = 0.  Any S.  The F(Theta; Y) of every component-analysis model's
 * log_likelihood is this total plus N c(Theta). */
int64_t pm_rows_lse_work_len(int64_t N);
/* The log-likelihood mode of pm_mix_scores_f64 (mixture_kernels.hip), same scores and arguments, for MoG diagonal and MoP:
 * rows[n] = log sum_h exp((S[n,h] + c[h]) coef + lp[h]) - (pmf ? sum_d lgamma(rowscale_n y_nd + yoff + 1) : 0), by a running
 * maximum and sum per row across the 64-wide H blocks; neither logpj nor the posteriors are formed, and H has no bound.
 * NaN in a row's terms gives NaN, all -inf gives -inf.  pmf (MoP's Poisson normaliser on the data the E-step sees: yoff = 1
 * when rowscale normalises, else 0) needs Bq == NULL. */
int pm_mix_loglik_f64(const double *Y, int64_t ldy, const double *rowscale, const double *Bq, const double *Bl, int64_t ldb,
                      const double *c, double coef, const double *lp, int64_t N, int64_t D, int64_t H, int pmf, double yoff,
                      double *rows, void *stream);
int pm_rows_lse_f64(const double *logpj, int64_t ld, int64_t N, int64_t S, double a, const double *col_offset,
                    double *rows_out, double *work, double *total, void *stream);

/* ---------------------------------------------------------------------------------------
 * Exact held-out log-likelihood (loglik_exact.hip)
 * ---------------------------------------------------------------------------------------
 * v_n = log sum_{all s} p(s, y_n | Theta) over the model's WHOLE state space, by enumeration on the device: states are
 * decoded from their index inside the kernels, nothing is stored per state.  rows_out (N; NULL = not written) receives v,
 * total[0] = sum_n v_n in a fixed order; the grid splits the state space into R ranges, R a function of N (through the tile
 * width and the number of tiles) and of the state count (never more ranges than chunks of the linear kernels, than states /
 * 1024 for MCA / MMCA, than supports / 32 for GSC, rounded up) and of nothing else: pm_loglik_exact_plan reports it; the
 * (max, sum exp) partials of every (range, datapoint) are combined in range order, no atomics: the same bits on every run
 * and in both builds.  N == 0 writes total[0] = 0.  A state of zero prior contributes nothing, a NaN in y_n gives v_n = NaN
 * (that row only).  `work`: pm_loglik_exact_work_len(N, H) doubles (a function of N and H only, linear in H).  Every entry
 * checks its arguments before it touches a device: PM_EINVAL for a null pointer, N < 0, D < 1, H < 1, ldy < D or a bad K,
 * PM_ERANGE past the bounds: K^H <= 2^32 and H <= 32 (linear models), H <= 32 (MCA / MMCA), H <= 16 (GSC). */
int64_t pm_loglik_exact_work_len(int64_t N, int64_t H);
/* What pm_loglik_exact_{lin,mca,gsc}_f64 launch for (N, D, K, H), from the host function the entries themselves take it from;
 * nothing is launched and no device is needed.  `kind`: PM_EXACT_LIN (K is read), PM_EXACT_MCA, PM_EXACT_GSC (K is ignored).
 * out[PM_EXACT_PLAN_LEN]:
 *   0 TN        datapoints per workgroup: lin 1 below N = 64 and 8 from there, MCA 1 below N = 16 and 4 from there, GSC 64
 *   1 L, 2 CH   lin: the L low digits of the state index are fixed per thread, CH = K^L <= 1024 lo states, at most four per
 *               thread; L is the largest such number of digits, and H where K^H <= 1024 (else 0, 1)
 *   3 space     what the ranges cut: lin the K^(H-L) chunks (values of the high digits), MCA / GSC the 2^H states; range r of R
 *               is [space r / R, space (r + 1) / R) in integer arithmetic
 *   4 units     the cap on R: lin the chunks, MCA ceil(2^H / 1024), GSC ceil(2^H / 32)
 *   5 R         min(units, min(4096, ceil(4096 / tiles))), tiles = ceil(N / TN); 1 for N = 0.  1 <= R <= units: no range is empty
 *   6 grid      tiles R workgroups of 256 threads
 *   7, 8        offset and length (doubles) of the (range, datapoint) partials inside `work`: N (H + 2) and 2 N R
 *   9           0
 * Returns PM_OK, PM_EINVAL (null `out`, unknown kind, N < 0, D < 1, H < 1, lin: K outside 2..8) or PM_ERANGE exactly where
 * the entry of the kind returns it. */
#define PM_EXACT_LIN 0
#define PM_EXACT_MCA 1
#define PM_EXACT_GSC 2
#define PM_EXACT_PLAN_LEN 10
int pm_loglik_exact_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, int64_t *out);
/* BSC, TSC, DSC: log p(s, y) = sum_h logp[h*K + k_h] - 1/2 s^T G s + x^T P s + cst + qcoef |x|^2, x = y - ymu (ymu: D values
 * or NULL for 0, BSC's mu), s_h = values[k_h] (K in 2..8 values, any reals), i.e. P = W / sigma^2 (D x H row-major),
 * G = W^T W / sigma^2 (H x H), logp the per-latent log-prior table (-inf for a value of zero prior), cst = -D/2 log(2 pi
 * sigma^2), qcoef = -1 / (2 sigma^2).  All pointers but the outputs and Y are small device arrays. */
int pm_loglik_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                            const double *logp, const double *values, int64_t K, double cst, double qcoef, int64_t N, int64_t D,
                            int64_t H, double *rows_out, double *work, double *total, void *stream);
/* MCA (signed_w = 0) and MMCA (signed_w = 1): log p(s, y) = |s| lp1 + (H - |s|) lp0 - inv_s2 / 2 |y - Wbar(s)|^2 + cst, with
 * Wbar_d(s) = (sum_{h in s} Wrho[h*D + d])^inv_rho (signed: sign(t) |t|^inv_rho), Wbar(0) = 0, Wrho = W^rho (signed:
 * sign(W) |W|^rho) as H x D rows; lp1 = log pi, lp0 = log(1 - pi), cst = -D/2 log(2 pi sigma^2). */
int pm_loglik_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w, double lp1,
                            double lp0, double inv_s2, double cst, int64_t N, int64_t D, int64_t H, double *rows_out,
                            double *work, double *total, void *stream);
/* GSC: log p(s, y) = sum_h logp[2h + s_h] + log N(y; W_s mu_s, Sigma + W_s Psi_s W_s^T), from the whitened products
 * P = Sigma^-1 W (D x H), M = W^T Sigma^-1 W (H x H), y^T Sigma^-1 y = sum_d wdiag_d y_d^2 (scalar / diagonal Sigma) or
 * |Lw y|^2 (full: Lw = chol(Sigma)^-1, D x D lower; at most one of wdiag and Lw), Psi (H x H), mu (H), logp[2h] =
 * log(1 - pi_h), logp[2h + 1] = log pi_h and cst = -D/2 log(2 pi) - 1/2 log det Sigma.  Per support, a wavefront factors
 * Psi_s = Lp Lp^T and I + Lp^T M_ss Lp in LDS (determinant lemma and Woodbury); a factor that is not positive definite
 * gives NaN. */
int pm_loglik_exact_gsc_f64(const double *Y, int64_t ldy, const double *P, const double *wdiag, const double *Lw,
                            const double *M, const double *Psi, const double *mu, const double *logp, double cst, int64_t N,
                            int64_t D, int64_t H, double *rows_out, double *work, double *total, void *stream);

/* ---------------------------------------------------------------------------------------
 * Exact posterior-mean reconstruction (recon_exact.hip)
 * ---------------------------------------------------------------------------------------
 * The posterior expectation sum_{all s} q_n(s) f(s), q_n(s) = p(s, y_n) / sum_{all s'} p(s', y_n), over the model's WHOLE
 * state space by enumeration on the device, with the models, arguments and log-joints of pm_loglik_exact_* (row constants
 * cancel in q and are not taken).  Two sweeps over the states: the first forms v_n = log sum_s exp l_n(s), the second the
 * sums weighted by exp(l_n(s) - v_n).  The state index space is cut into R ranges, R a function of the state count alone
 * (never of N); a workgroup owns one (row or row tile, range) and writes one partial, and the partials are merged in range
 * order.  No atomics: a row of the result is a function of that row of Y and of the parameters alone -- the same bits on
 * every run, in both builds, under a row permutation and in any shard.  A NaN in y_n makes that row NaN and no other; a
 * state of zero prior carries weight 0.
 *
 * `work`: pm_recon_exact_work_len(N, H, D) doubles, enough for any of the three entries.  The entries walk N in row blocks
 * of a fixed size (256 rows; MCA 64), so the length is bounded in N, does not depend on the state count and is at most
 * min(N, 256) (H + 1 + 256 max(H, 2)) or min(N, 64) (1 + 64 max(D, 2)), whichever is larger (-1 for N < 0, H < 1 or D < 1).
 * Every entry checks its arguments before it touches a device: PM_EINVAL for a null pointer, N < 0, D < 1, H < 1, ldy < D,
 * an output leading dimension below the row width or a bad K; PM_ERANGE past the bounds of pm_loglik_exact_* (K^H <= 2^32
 * and H <= 32; GSC H <= 16) and, for MCA / MMCA, D > 1024.  N == 0 launches nothing and returns PM_OK. */
int64_t pm_recon_exact_work_len(int64_t N, int64_t H, int64_t D);
/* What pm_recon_exact_{lin,mca,gsc}_f64 do for (N, D, K, H), from the host function the entries themselves take it from;
 * nothing is launched and no device is needed.  `kind` as for pm_loglik_exact_plan.  out[PM_EXACT_PLAN_LEN]:
 *   0 rows      rows per block of the host walk: 256, MCA 64            1 blocks   ceil(N / rows)
 *   2 L, 3 CH   as in pm_loglik_exact_plan (MCA, GSC: 0, 1)
 *   4 space     what the ranges cut: lin the chunks, MCA / GSC the states; range r is [space r / R, space (r + 1) / R)
 *   5 R         lin min(256, max(1, chunks / 2)), MCA min(64, max(1, states / 64)), GSC min(256, max(1, states / 32)): a
 *               function of the state count alone, 1 <= R <= space
 *   6 slabs     MCA: ceil(D / 64) 64-wide slabs of the dimensions a lane walks; else 0
 *   7           offset (doubles) of the partials inside `work` for the largest block, nb = min(N, rows) rows: nb (H + 1), MCA nb
 *   8, 9        length of the partials of sweep 1 (2 nb R) and of sweep 2 (nb R H, MCA nb R D)
 * Returns PM_OK, PM_EINVAL or PM_ERANGE as pm_loglik_exact_plan does, and PM_ERANGE where the entry of the kind returns it
 * (MCA: D > 1024). */
int pm_recon_exact_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, int64_t *out);
/* BSC, TSC, DSC: E (N x H, row stride lde >= H) receives E_n[s]_h = sum_s q_n(s) values[k_h]; Y, ymu, P, G, logp, values and
 * K as for pm_loglik_exact_lin_f64.  Columns of E past H are not written. */
int pm_recon_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                           const double *logp, const double *values, int64_t K, int64_t N, int64_t D, int64_t H, double *E,
                           int64_t lde, double *work, void *stream);
/* First and second posterior moments of the latents and the log-evidence term, per row, for exact EM; the
 * arguments of pm_recon_exact_lin_f64 and its contract (no atomics, nothing depends on PM_DETERMINISTIC, the state split and
 * every merge order are functions of the state count, H and K alone, a row's outputs are a function of that row and of the
 * parameters: the same bits on every run, in both builds, under a row permutation, in any shard and in any row block; a NaN
 * in y_n makes that row NaN and no other; a state of zero prior carries weight 0):
 *   E (N x H, row stride lde >= H)             E_n[s_h] -- the bits pm_recon_exact_lin_f64 writes for the same arguments
 *   C (N x H (H + 1) / 2, row stride ldc)      E_n[s_h s_h'] for h <= h', s_h = values[k_h], in the order (0,0), (0,1), ...,
 *                                              (0,H-1), (1,1), ...: the pair (h, h') sits at h H - h (h - 1) / 2 + h' - h
 *   v (N)                                      v_n = log sum_{all s} exp l_n(s), l the log-joint of pm_loglik_exact_lin_f64
 *                                              without its row constants
 * Per row block of 256 rows: sweeps 1 (v) and 2 (E) as pm_recon_exact_lin_f64 runs them; then the pair sweeps, over R3 =
 * min(256, max(1, chunks / 16)) ranges of their own (their epilogue is longer): one full weighted sweep that leaves the pairs
 * of the L low digits (from the per-thread masses of the lo states, after the loop), and one sweep per high digit i with every
 * weight multiplied by that digit's value, over the chunks where the value is not 0 (K = 2: half of them) -- row L + i of
 * E[s s^T], which gives the lo-hi and hi-hi pairs.  3 + (H - L) (K - 1) / K sweeps in all, against pm_recon_exact_lin_f64's 2.
 * Columns of E and C past their row widths are not written.
 * `work`: pm_moments_exact_work_len(N, H) doubles = min(N, 256) (H + 1 + 256 max(H, 55)) (-1 for N < 0 or H < 1): bounded in N.
 * PM_EINVAL / PM_ERANGE exactly where pm_recon_exact_lin_f64 returns them (K^H <= 2^32, H <= 32), PM_EINVAL also for
 * ldc < H (H + 1) / 2 or a null C or v with N > 0; checked before a device is touched; N == 0 launches nothing. */
int64_t pm_moments_exact_work_len(int64_t N, int64_t H);
/* What pm_moments_exact_lin_f64 does for (N, D, K, H); nothing is launched and no device is needed.
 * out[PM_MOMENTS_PLAN_LEN]:
 *   0 rows, 1 blocks, 2 L, 3 CH, 4 chunks, 5 R   as pm_recon_exact_plan(PM_EXACT_LIN, ...) reports them
 *   6 pinned sweeps   H - L, one per high digit          7 lo-lo pairs   L (L + 1) / 2, formed after the full sweep's loop
 *   8 R3              ranges of the pair sweeps: min(256, max(1, chunks / 16)), a function of the state count alone
 *   9                 offset (doubles) of the partials inside `work` for the largest block, nb = min(N, rows): nb (H + 1)
 *   10, 11            length of the largest partials of sweeps 1 and 2 (nb R max(2, H)) and of the pair sweeps
 *                     (nb R3 max(H, lo-lo pairs))
 * Returns PM_OK, PM_EINVAL or PM_ERANGE as pm_recon_exact_plan does. */
#define PM_MOMENTS_PLAN_LEN 12
int pm_moments_exact_plan(int64_t N, int64_t D, int64_t K, int64_t H, int64_t *out);
int pm_moments_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                             const double *logp, const double *values, int64_t K, int64_t N, int64_t D, int64_t H, double *E,
                             int64_t lde, double *C, int64_t ldc, double *v, double *work, void *stream);
/* MCA (signed_w = 0) and MMCA (signed_w = 1): Yhat (N x D, row stride ldo >= D) receives sum_s q_n(s) Wbar_d(s); Wrho,
 * inv_rho, lp1, lp0 and inv_s2 as for pm_loglik_exact_mca_f64.  One wavefront per state, lanes over the dimensions. */
int pm_recon_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w, double lp1,
                           double lp0, double inv_s2, int64_t N, int64_t D, int64_t H, double *Yhat, int64_t ldo,
                           double *work, void *stream);
/* GSC: E (N x H, row stride lde >= H) receives E_n[s o z]_h = sum_s q_n(s) kappa_s(y_n)_h (0 for h outside s), kappa_s =
 * mu_s + A_s^T (A_s beta_{n,s}) = E[z_s | s, y_n] in the notation of pm_loglik_exact_gsc_f64; P, M, Psi, mu and logp as
 * there (y^T Sigma^-1 y is a row constant and not needed). */
int pm_recon_exact_gsc_f64(const double *Y, int64_t ldy, const double *P, const double *M, const double *Psi,
                           const double *mu, const double *logp, int64_t N, int64_t D, int64_t H, double *E, int64_t lde,
                           double *work, void *stream);

/* ---------------------------------------------------------------------------------------
 * Exact top-K posterior states (infer_exact.hip)
 * ---------------------------------------------------------------------------------------
 * Per datapoint the topK states of largest log-joint l_n(s) over the model's WHOLE state space by enumeration on the device,
 * and v_n = log sum_{all s} exp l_n(s), with the models, operands and log-joints of pm_recon_exact_* (row constants are not
 * taken).  A state ranks before another if its log-joint is larger, or if the two are equal and its state index is smaller:
 * the order is a function of (value, index) alone.  The state index is sum_h k_h K^h (linear models) or the bit mask of s (MCA
 * / MMCA).  Outputs, per row n:
 *   top_idx (N x cols, int64, row stride ldi)   the state indices, best first
 *   top_l   (N x cols, row stride ldl)          their log-joints l_n(s), without the row constants
 *   v       (N)                                 v_n
 * with cols = min(topK, states); columns past cols are not written.  A state of zero prior has l = -inf and ranks after every
 * finite one, by index.  A row that holds a NaN log-joint gets index -1 and NaN in its cols columns and NaN in v; no other row
 * is affected.
 *
 * One sweep over the states: every thread keeps a running (max, sum exp) and its PM_INFER_EXACT_MAX_TOPK best (value, index)
 * pairs in registers, a workgroup -- one (row, state range) -- reduces both into one partial, and one wavefront per row merges
 * the row's R partials.  The contract is that of pm_recon_exact_*: no atomics and nothing depends on PM_DETERMINISTIC; the
 * split of the state space into R ranges, the assignment of states to threads and every merge are functions of the state count
 * (and H, K, D, topK) alone, never of N; l_n(s) comes from the single definitions of pm_exact.h.  A row of the result is a
 * function of that row of Y and of the parameters alone: the same bits on every run, in both builds, under a row permutation
 * and in any shard.
 *
 * topK: 1 .. PM_INFER_EXACT_MAX_TOPK (the length of a thread's list), else PM_EINVAL (< 1) / PM_ERANGE (above).  `work`:
 * pm_infer_exact_work_len(N, H, topK) doubles, enough for either entry: the entries walk N in row blocks (256 rows; MCA 64), so
 * the length is bounded in N: min(N, 256) (H + 256 (2 + 2 topK)) or min(N, 64) 64 (2 + 2 topK), whichever is larger (-1 for N <
 * 0, H < 1 or a topK outside its limits).  Every entry checks its arguments before it touches a device: PM_EINVAL for a null
 * pointer, N < 0, D < 1, H < 1, ldy < D, ldi or ldl < cols or a bad K; PM_ERANGE past the limits of pm_recon_exact_lin_f64
 * (K^H <= 2^32, H <= 32, K <= 8) and pm_recon_exact_mca_f64 (H <= 32, D <= 1024).  N == 0 launches nothing. */
#define PM_INFER_EXACT_MAX_TOPK 16
int64_t pm_infer_exact_work_len(int64_t N, int64_t H, int64_t topK);
/* What pm_infer_exact_{lin,mca}_f64 do for (N, D, K, H, topK), from the host function the entries themselves take it from;
 * nothing is launched and no device is needed.  `kind`: PM_EXACT_LIN (K is read) or PM_EXACT_MCA.  out[PM_INFER_PLAN_LEN]:
 *   0 rows      rows per block of the host walk: 256, MCA 64            1 blocks   ceil(N / rows)
 *   2 L, 3 CH   as in pm_loglik_exact_plan (MCA: 0, 1)
 *   4 space     what the ranges cut: lin the chunks, MCA the states; range r is [space r / R, space (r + 1) / R)
 *   5 R         lin min(256, max(1, chunks / 2)), MCA min(64, max(1, states / 64)): pm_recon_exact_plan's, 1 <= R <= space
 *   6 cols      min(topK, states): the columns written, and the length of a partial list
 *   7, 8        offset and length (doubles) of the (max, sum exp) partials inside `work` for the largest block, nb =
 *               min(N, rows) rows: nb H (MCA 0) and 2 nb R
 *   9, 10       offsets of the partial lists' values and of their indices (int64, one per double's place)
 *   11          length of either: nb R cols
 * Returns PM_OK, PM_EINVAL (null `out`, unknown kind -- PM_EXACT_GSC has no entry --, N < 0, D < 1, H < 1, topK < 1, lin: K
 * outside 2..8) or PM_ERANGE exactly where the entry of the kind returns it. */
#define PM_INFER_PLAN_LEN 12
int pm_infer_exact_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, int64_t topK, int64_t *out);
/* The linear models (K-ary: BSC, TSC, DSC); Y, ymu, P, G, logp, values and K as for pm_recon_exact_lin_f64. */
int pm_infer_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                           const double *logp, const double *values, int64_t K, int64_t N, int64_t D, int64_t H,
                           int64_t topK, int64_t *top_idx, int64_t ldi, double *top_l, int64_t ldl, double *v, double *work,
                           void *stream);
/* MCA (signed_w = 0) and MMCA (signed_w = 1); Wrho, inv_rho, lp1, lp0 and inv_s2 as for pm_recon_exact_mca_f64.  One wavefront
 * per state, lanes over the dimensions. */
int pm_infer_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w, double lp1,
                           double lp0, double inv_s2, int64_t N, int64_t D, int64_t H, int64_t topK, int64_t *top_idx,
                           int64_t ldi, double *top_l, int64_t ldl, double *v, double *work, void *stream);

/* ---------------------------------------------------------------------------------------
 * Posterior-mean reconstruction (reconstruct_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * yhat_n = sum_{s in K_n} q_n(s) ybar(s), q_n(s) = exp(a logpj[n,s] + o_s - lse_n), over exactly the states whose log-joints
 * an E-step pass left in logpj (N, ld >= K).  No atomics: every output element is written by one lane and the sums over a
 * row's states run in a fixed order, so both builds return the same bits and a row's value does not depend on the others.
 * Every entry checks its arguments before it touches a device (PM_EINVAL: null pointer, N < 0, short leading dimension,
 * inconsistent layout; PM_ERANGE: past a kernel's limit); N == 0 launches nothing.
 *
 * pm_gemm_nt_rows_f64: C = A . B^T as pm_gemm_nt_f64, but as ONE launch of one kernel with the whole K range per tile (no
 * K-slices, no second tile shape for a ragged last round): a row of C depends on its row of A and on B alone. */
int pm_gemm_nt_rows_f64(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M,
                        int64_t N, int64_t K, void *stream);
/* Posterior expectation of the latents from a log-joint row.  Columns of logpj: [single_off, single_off + nblocks H) the
 * one-cause blocks -- in block c latent h takes the value block_values_host[c] (HOST memory, nblocks <= 8 values; BSC: {1},
 * DSC: the non-zero values in order) --, [multi_off, multi_off + S) the table states -- in state s the latent at candidate
 * position j, cand[n, j], takes state_vals[s * Hprime + j] (S x Hprime doubles, device); a latent held by two positions (TSC)
 * receives both --; any other column below K (the null state) carries weight only.  lse: the rows' log-sum-exp where the
 * E-step left it (then a == 1 and col_offset == NULL), or NULL: a maximum pass and a sum pass over a logpj + col_offset (K
 * values or NULL), NaN for a row with a NaN entry.  out (N, ldo >= out_cols >= H): out[n, h] = E[s_h | y_n] for h < H, 1 in
 * column ones_col (-1: none; else H <= ones_col < out_cols: the column that carries mu through the product) and 0 in the
 * other columns up to out_cols.  With single_off = 0, nblocks = 1, the value 1 and S = 0 this is the row softmax of
 * a X + o: a mixture's responsibilities.  Hprime <= PM_MAX_HPRIME. */
int pm_recon_expect_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset,
                        const int32_t *cand, const double *state_vals, const double *block_values_host, int64_t N, int64_t H,
                        int64_t Hprime, int64_t K, int64_t single_off, int64_t nblocks, int64_t multi_off, int64_t S,
                        double *out, int64_t ldo, int64_t out_cols, int64_t ones_col, void *stream);
/* MCA (signed_w = 0) / MMCA (1): Yhat[n, d] += sum_s q_n(s) Wbar_d(s) over the S multi-cause states (columns 1 + H + s of
 * logpj, ld >= 1 + H + S; masks over the candidate positions as pm_mca_estep_f64), Wbar_d(s) = (sum_{j in s} Wrho[cand[n,j],
 * d])^inv_rho (signed: sign(t) |t|^inv_rho) with the E-step's power functions; lse as above (a = 1).  The null and one-cause
 * part of Yhat is pm_recon_expect_f64 + pm_gemm_nt_rows_f64 against W.  D <= 1024, Hprime <= PM_MAX_HPRIME. */
int pm_recon_mca_f64(const double *logpj, int64_t ld, const double *lse, const int32_t *cand, const uint16_t *state_masks,
                     const double *Wrho, double inv_rho, int signed_w, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                     int64_t S, double *Yhat, int64_t ldy, void *stream);

/* ---------------------------------------------------------------------------------------
 * Posterior variance of the reconstruction (recon_var.hip)
 * ---------------------------------------------------------------------------------------
 * V_nd = E_q[ybar_d(s)^2] - yhat_nd^2 over exactly the states and weights of the entries above.  For ybar = mu + W u the second
 * moment is E[((W u)_d)^2] = sum_h m2[n,h] W_dh^2 + 2 sum_{i<j} p[n,(i,j)] W_d,c_i W_d,c_j: two latents co-occur only among a
 * row's candidates c = cand[n, :].  No atomics and no branch on the build; every output element is written once by one lane,
 * and every sum runs in an order fixed by H, Hprime, S and D alone (a lane adds its states in ascending state number and its
 * pairs in ascending pair number): both builds return the same bits and a row's bits depend on that row alone.  Every entry
 * checks its arguments before it touches a device, at N == 0 too: PM_EINVAL for a null pointer, a negative size, a short
 * leading dimension or an inconsistent layout, PM_ERANGE past a limit; N == 0 launches nothing.
 *
 * pm_recon_moments2_f64: logpj, ld, lse, a, col_offset, cand, state_vals, block_values_host, N, H, Hprime, K, single_off,
 * nblocks, multi_off, S exactly as pm_recon_expect_f64.  m2 (N, ldm >= out_cols >= H): m2[n, h] = sum_c value_c^2 q(block c, h)
 * + sum over the table states of q(s) v_j^2 at every candidate position j that holds h (a latent held by two positions (TSC)
 * receives both), 0 in the columns [H, out_cols) (the K padding of the product that follows).  p (N, ldp >= Hprime (Hprime -
 * 1) / 2): p[n, (i,j)] = sum over the table states of q(s) v_i v_j, pairs of POSITIONS in the order (0,1), (0,2), ...,
 * (Hprime-2, Hprime-1), the order of pm_bsc_mtrain_rows_f64; p may be NULL when there are no pairs or no table states (Hprime
 * <= 1 or S == 0) and is written (zeros for S == 0) whenever it is given.  With S = 0 and one block of value 1, m2 is the row
 * softmax of a X + o.  Hprime <= PM_MAX_HPRIME, nblocks <= 8. */
int pm_recon_moments2_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset,
                          const int32_t *cand, const double *state_vals, const double *block_values_host, int64_t N,
                          int64_t H, int64_t Hprime, int64_t K, int64_t single_off, int64_t nblocks, int64_t multi_off,
                          int64_t S, double *m2, int64_t ldm, int64_t out_cols, double *p, int64_t ldp, void *stream);
/* GSC: m2 and p (layout and pair order as above) of u = s o z, E[u u^T] = sum_s q(s) (kappa_s kappa_s^T + Lambda_s^-1), from one
 * pass of pm_gsc_estep_lpj_blocks_f64 at the same beta: logpj (N, ldl >= 1 + H + S), blocks (N, ldb >= 2 Hprime^2 + 2 Hprime + 1;
 * NULL: no multi-cause states, S == 0), the scores (N, lds >= H) and tables (8 H) that pass was given, and cand (N, Hprime).
 * The weights are the E-step's own: exp(beta lp) floored at DBL_MIN for every state but the null state, normalised by 1 / (Z
 * + DBL_MIN).  m2[n,h] = q_h (kappa_h^2 + 1 / lambda_h) + the diagonal of the candidate block at the position that holds h;
 * p[n,(i,j)] = the mean of the block's (i,j) and (j,i) entries.  Hprime <= PM_MAX_HPRIME. */
int pm_recon_gsc_moments2_f64(const double *logpj, int64_t ldl, const double *blocks, int64_t ldb, const double *scores,
                              int64_t lds, const double *tables, const int32_t *cand, double beta, int64_t N, int64_t H,
                              int64_t Hprime, int64_t S, double *m2, int64_t ldm, int64_t out_cols, double *p, int64_t ldp,
                              void *stream);
/* V (N, ldv >= D) arrives holding sum_h m2[n,h] W_dh^2 (pm_gemm_nt_rows_f64 of m2 against W o W) and leaves as
 *   V[n,d] = max(V[n,d] + 2 sum_{i<j} p[n,(i,j)] Wt[c_i, d] Wt[c_j, d] - (Yhat[n,d] - mu[d])^2, 0)
 * (mu NULL: 0; a NaN stays NaN), Wt (H, ldw >= D) the transpose of W, Yhat (N, ldy >= D) the posterior mean.  A candidate
 * outside [0, H) is clamped into it.  p NULL or Hprime <= 1: no pair term, and cand and Wt are not read and may be NULL (the
 * mixtures, MCA / MMCA, Hprime = 1).  Any D; Hprime <= PM_MAX_HPRIME. */
int pm_recon_var_finish_f64(double *V, int64_t ldv, const double *Yhat, int64_t ldy, const double *mu, const double *p,
                            int64_t ldp, const int32_t *cand, const double *Wt, int64_t ldw, int64_t N, int64_t H, int64_t D,
                            int64_t Hprime, void *stream);
/* MCA (signed_w = 0) / MMCA (1): V[n, d] += sum_s q_n(s) Wbar_d(s)^2 over the S multi-cause states, arguments, Wbar, power
 * functions and limits of pm_recon_mca_f64.  The one-cause part of E[ybar^2] is pm_recon_moments2_f64 (one block of value 1, S =
 * 0) + pm_gemm_nt_rows_f64 against W o W; pm_recon_var_finish_f64 without pairs follows.  D <= 1024, Hprime <= PM_MAX_HPRIME. */
int pm_recon_mca_var_f64(const double *logpj, int64_t ld, const double *lse, const int32_t *cand, const uint16_t *state_masks,
                         const double *Wrho, double inv_rho, int signed_w, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                         int64_t S, double *V, int64_t ldv, void *stream);

/* ---------------------------------------------------------------------------------------
 * Latent codes (encode_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * mean[n, h] = sum_s q_n(s) s_h and prob[n, h] = sum_s q_n(s) [s_h != 0] under the weights of the reconstruction entries
 * above, over exactly the states of logpj (pm_encode_f64) or over the whole state space (pm_encode_exact_mca_f64).  No atomics
 * and no branch on the build: every output element is written once by one lane and every sum runs in an order fixed by the
 * shape alone, so both builds return the same bits and a row's bits depend on that row alone.  Every entry checks its
 * arguments before it touches a device (PM_EINVAL: null pointer, negative size, short leading dimension, inconsistent
 * layout; PM_ERANGE: past a limit); N == 0 launches nothing.
 *
 * pm_encode_f64: logpj, ld, lse, a, col_offset, cand, state_vals, block_values_host, N, H, Hprime, K, single_off, nblocks,
 * multi_off, S exactly as pm_recon_expect_f64; the row is read and every column's weight evaluated once for both outputs.
 * mean (N, ldm >= H): the bits pm_recon_expect_f64 writes into out[:, :H] for the same arguments (same order, same fma's; a
 * latent held by two candidate positions (TSC) receives both) -- except in a row whose log-sum-exp is NaN, which is NaN at
 * EVERY latent of both outputs, also where no column gives the latent a value and that entry writes 0.  prob (N, ldp >= H): sum_c q(block c, h) over the blocks of
 * non-zero value + the weights of the table states in which ANY position that holds h is non-zero -- a state counts once per
 * latent, so prob <= 1 --, returned as min(p, 1); a NaN stays NaN.  With one block of value 1 and a 0/1 table prob carries the
 * bits of mean (below the clamp).  With single_off = 0, nblocks = 1, the value 1 and S = 0 both are the row softmax of a X + o.
 * Hprime <= PM_MAX_HPRIME, nblocks <= 8. */
int pm_encode_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset, const int32_t *cand,
                  const double *state_vals, const double *block_values_host, int64_t N, int64_t H, int64_t Hprime, int64_t K,
                  int64_t single_off, int64_t nblocks, int64_t multi_off, int64_t S, double *mean, int64_t ldm, double *prob,
                  int64_t ldp, void *stream);
/* MCA (signed_w = 0) and MMCA (signed_w = 1): E (N x H, row stride lde >= H) receives E_n[s]_h = sum_{all s} q_n(s) s_h, the
 * posterior activation probabilities over all 2^H states; model, arguments, sweeps, row blocks and ranges of
 * pm_recon_exact_mca_f64 (R from pm_recon_exact_plan: a function of the state count alone; partials merged in range order).
 * `work`: pm_recon_exact_work_len(N, H, D) doubles.  PM_ERANGE for H > 32 or D > 1024.  Columns of E past H are not written. */
int pm_encode_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w, double lp1,
                            double lp0, double inv_s2, int64_t N, int64_t D, int64_t H, double *E, int64_t lde, double *work,
                            void *stream);

/* ---------------------------------------------------------------------------------------
 * Whole-image denoising by overlapping patches (patch_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * The patch grid.  Along an axis of length L, patches of length p at stride s >= 1 start at 0, s, 2s, ... while start + p <=
 * L, plus at L - p if the last of these is not L - p: every position is covered for every stride s <= p (and for s > p when
 * L <= 2p; any other stride leaves positions between the regular starts uncovered and is refused below).
 * pm_patches_count(L, p, s) is the number of starts (-1 for p > L, a non-positive argument or L > 2^30).  An image stack (B, Hi, Wi) -- row i of image
 * b at image + (b Hi + i) ld -- with patches of ph x pw values has N = B nr nc patches, nr = count(Hi, ph, s), nc =
 * count(Wi, pw, s), numbered row-major over (image, start row, start column); a patch is a row of D = ph pw values, element
 * (a, b) at a pw + b.  The entries below work on the rows [n0, n0 + n) of the (N, D) patch matrix, handed over as the
 * pointer to row n0, so that a caller walks an image in chunks and never holds the whole matrix.
 *
 * No entry holds an atomic or a branch on the build: both libraries return the same bits.  Every entry checks its arguments
 * before it touches a device: PM_EINVAL for a null pointer, B, Hi, Wi, ph, pw or stride < 1, ph > Hi, pw > Wi, a stride that
 * leaves pixels uncovered (stride > ph with Hi > 2 ph, or stride > pw with Wi > 2 pw), a leading
 * dimension shorter than its row, n0 < 0, n < 0 or n0 + n > N; PM_ERANGE for Hi or Wi > 2^30 or D > 4096.  n == 0 launches
 * nothing.
 *
 * pm_patches_extract_f64 / _f32 (the image's element type; f32 is converted exactly): out (n, ldo >= D) receives the patches.
 * center != 0: means (n) receives each patch's mean and out the patch minus its mean.  The mean's summation order is fixed
 * by D alone: with g the smallest power of two >= min(D, 64), partial sum l (l < g) adds the elements l, l + g, l + 2g, ...
 * in ascending order starting from the first (a partial sum without elements is +0), the g partial sums are combined by
 * butterflies v_l <- v_l + v_(l xor o) for o = g/2, g/4, ..., 1, and the result is divided by D once.  A patch's bits depend
 * on the patch alone, not on n0, n or its position among the rows. */
int64_t pm_patches_count(int64_t length, int64_t patch, int64_t stride);
int pm_patches_extract_f64(const double *image, int64_t ldi, int64_t B, int64_t Hi, int64_t Wi, int64_t ph, int64_t pw,
                           int64_t stride, int64_t n0, int64_t n, int center, double *out, int64_t ldo, double *means,
                           void *stream);
int pm_patches_extract_f32(const float *image, int64_t ldi, int64_t B, int64_t Hi, int64_t Wi, int64_t ph, int64_t pw,
                           int64_t stride, int64_t n0, int64_t n, int center, double *out, int64_t ldo, double *means,
                           void *stream);
/* acc (B, Hi, Wi; row stride lda >= Wi), a running sum the caller zeroes once: every pixel receives, ONE ADDITION AT A TIME IN
 * ASCENDING PATCH NUMBER, acc <- acc + est[k - n0, e] (means == NULL) or acc <- acc + (est[k - n0, e] + means[k - n0]) of the
 * patches k in [n0, n0 + n) that cover it (e: the pixel's element of patch k).  A pixel is owned by one lane (gather form); a
 * workgroup stages the estimate rows that reach its tile of pixels in LDS and reads them as rows.  Called with ascending,
 * disjoint ranges that together cover [0, N), the sequence of additions of a pixel -- and so the sum's bits -- is the same
 * for every split into ranges. */
int pm_patches_accumulate_f64(const double *est, int64_t lde, const double *means, int64_t n0, int64_t n, double *acc,
                              int64_t lda, int64_t B, int64_t Hi, int64_t Wi, int64_t ph, int64_t pw, int64_t stride,
                              void *stream);
/* out[b, i, j] = acc[b, i, j] / cover(i, j), one IEEE division; cover: the number of patches of the grid that contain the
 * pixel, computed from the grid rule.  out may be acc. */
int pm_patches_finish_f64(const double *acc, int64_t lda, double *out, int64_t ldo, int64_t B, int64_t Hi, int64_t Wi,
                          int64_t ph, int64_t pw, int64_t stride, void *stream);
/* The weighted overlap average.  Grid, patch numbering, ranges [n0, n0 + n) and the running-sum contract are
 * those of pm_patches_accumulate_f64; num and den (B, Hi, Wi; row stride lda >= Wi) are two running sums the caller zeroes
 * once.  The weight of element e of patch k is w = a b:
 *   a = 1 (wgt == NULL), wgt[k - n0, e] (wmode 0) or 1.0 / (v + floor), v = wgt[k - n0, e] < 0 ? 0 : wgt[k - n0, e] (wmode 1:
 *       wgt holds variances; a NaN stays NaN);
 *   b = 1 (window == NULL) or window[e], window holding D doubles;
 * with one factor present w is that factor and nothing is multiplied.  Every pixel receives, one patch at a time in
 * ascending patch number, with t = est[k - n0, e] (means == NULL) or est[k - n0, e] + means[k - n0]:
 *   num <- num + (w t)   (the product is rounded, then the sum: no fused multiply-add)
 *   den <- den + w       (den == NULL: skipped)
 * A pixel is owned by one lane; a workgroup stages the estimate rows and the weight rows that reach its tile together in
 * LDS and reads them as rows.  No atomics, no branch on the build: both libraries give the same bits, and the sequence of
 * additions of a pixel is the same for every split of [0, N) into ascending ranges.  est and wgt may be the same matrix.
 * With wgt == window == NULL num receives the bits pm_patches_accumulate_f64 writes and den the cover count.
 * PM_EINVAL, before anything touches a device: a null est or num; wmode other than 0 or 1; wmode 1 with wgt == NULL or a
 * floor that is negative or not finite; ldw < D with wgt given; everything pm_patches_accumulate_f64 refuses, with its codes
 * (PM_ERANGE for Hi or Wi > 2^30 or D > 4096).  n == 0 launches nothing. */
int pm_patches_accumulate_w_f64(const double *est, int64_t lde, const double *wgt, int64_t ldw, int wmode, double floor,
                                const double *window, const double *means, int64_t n0, int64_t n, double *num, double *den,
                                int64_t lda, int64_t B, int64_t Hi, int64_t Wi, int64_t ph, int64_t pw, int64_t stride,
                                void *stream);
/* out[b, i, j] = num[b, i, j] / den[b, i, j], one IEEE division (0 / 0 is NaN: a pixel all of whose weights are 0 has no
 * average).  out may be num.  PM_EINVAL for a null pointer, B, Hi or Wi < 1 or a leading dimension < Wi; PM_ERANGE for Hi or
 * Wi > 2^30. */
int pm_patches_finish_w_f64(const double *num, const double *den, int64_t lda, double *out, int64_t ldo, int64_t B,
                            int64_t Hi, int64_t Wi, void *stream);

/* ---------------------------------------------------------------------------------------
 * Pooled feature maps of an image's patch codes (pool_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * The codes of the N = B nr nc patches of an image stack (numbered as above: row-major over image, start row, start column)
 * are an (N, H) matrix, row stride ldc >= H: H channels on the patch grid (B, nr, nc).  Pooling reduces the grid to (B, gh,
 * gw) regions.  The region rule: region i of an axis of n patch positions cut into g regions is [floor(i n / g), floor((i +
 * 1) n / g)), 1 <= g <= n -- ascending, never empty, lengths differing by at most 1.  Output (b, i, j, h) covers the patches
 * of image b whose start-row index lies in region i of (nr, gh) and whose start-column index lies in region j of (nc, gw).
 *
 * pm_codes_pool_f64 works on the rows [n0, n0 + n) of the matrix, handed over as the pointer to row n0; n0 and n are
 * multiples of nc (whole patch rows R = b nr + r).  acc (B, gh, gw, H), contiguous, is a running result the caller fills once:
 * with +0 for mode 0 (sum), with -inf for mode 1 (max).
 *   mode 0: acc[b, i, j, h] <- acc + t_R for the patch rows R of image b in region row i that lie in the range, in ascending R,
 *           one addition at a time, with t_R = (((+0 + x[R, c0, h]) + x[R, c0 + 1, h]) + ...) over the columns [c0, c1) of
 *           region column j in ascending order: a sum over rows of sums over columns, both ascending.
 *   mode 1: the same walk with the larger of the two in place of the sum and -inf in place of +0, by explicit compares: a NaN
 *           input makes that output NaN, and of -0 and +0 the larger is +0, so the order changes no bit.
 * t_R depends on patch row R alone, so called with ascending, disjoint ranges that together cover [0, N) the sequence of
 * operations of an output -- and its bits -- is the same for every split into ranges.  Two launches: the partials t of the
 * range into `work` (pm_codes_pool_work_len(n, nc, gw, H) = (n / nc) gw H doubles; -1 for arguments the entry refuses), then
 * every output, owned by one lane, walks its partials.  h runs on the lanes; with H < 64 a wavefront holds several (patch
 * row, region column) pairs.  No atomics and no branch on the build: both libraries return the same bits.
 * pm_codes_pool_finish_f64: out[b, i, j, h] = acc[b, i, j, h] / (rows of region i x columns of region j), one IEEE division
 * (the mean; the count is exact in a double up to 2^53); out may be acc.
 * Every entry checks its arguments before it touches a device: PM_EINVAL for a null pointer, B, nr, nc, gh, gw or H < 1, gh >
 * nr, gw > nc, ldc < H, a mode other than 0 or 1, n0 < 0, n < 0, n0 + n > B nr nc, n0 or n not a multiple of nc; PM_ERANGE for
 * nr or nc > 2^30 or H > 2^20.  n == 0 launches nothing. */
int64_t pm_codes_pool_work_len(int64_t n, int64_t nc, int64_t gw, int64_t H);
int pm_codes_pool_f64(const double *codes, int64_t ldc, int64_t n0, int64_t n, int64_t B, int64_t nr, int64_t nc, int64_t gh,
                      int64_t gw, int64_t H, int mode, double *acc, double *work, void *stream);
int pm_codes_pool_finish_f64(const double *acc, double *out, int64_t B, int64_t nr, int64_t nc, int64_t gh, int64_t gw,
                             int64_t H, void *stream);

/* ---------------------------------------------------------------------------------------
 * Missing values: masked E-steps for inference (masked_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * mask (N, ldm >= D) bytes, non-zero = observed.  An unobserved value is selected away where it is read (m ? v : 0), never
 * multiplied: NaN or inf there changes no bit of any output.  No atomics, every output element is written once by one lane
 * and a row's sums over d run in an order fixed by D alone: both builds return the same bits and a row's bits depend on that
 * row (of the data and of the mask) and on the parameters alone.  Every entry checks its arguments before it touches a
 * device: PM_EINVAL for a null pointer, a negative size or a short leading dimension, PM_ERANGE past a limit; N == 0
 * launches nothing.
 *
 * pm_masked_prepare_f64: X0[n,d] = m ? Y[n,d] - mu[d] : 0 (mu NULL: 0), Mf[n,d] = m ? 1 : 0 (Mf may be NULL), xnorm2[n] =
 * sum_d X0^2, dn[n] = number of observed dimensions.  With these the terms that are dense over H are two products of
 * pm_gemm_nt_rows_f64: b = X0 . W (N, H) and diag G_n = Mf . (W o W) (N, H). */
int pm_masked_prepare_f64(const double *Y, int64_t ldy, const uint8_t *mask, int64_t ldm, const double *mu, int64_t N,
                          int64_t D, double *X0, int64_t ldx, double *Mf, int64_t ldf, double *xnorm2, int32_t *dn,
                          void *stream);
/* BSC: per row, the Hprime candidates with the largest b_h / sqrt(g_h) (a term with g_h = 0 counts as 0; ascending, ties
 * towards the larger index: the order of pm_bsc_select_f64; a row with nothing observed gets the Hprime largest indices)
 * into cand (N, Hprime), the Hprime (Hprime - 1) / 2 masked products sum_d m_d Wt[c_i, d] Wt[c_j, d] of the candidates' rows
 * of Wt (H, ldw >= D), and logpj (N, ldl >= 1 + H + S) in the layout of pm_bsc_estep_f64 with
 *   e_0 = xnorm2, e_h = g_h - 2 b_h + xnorm2, e_s = xnorm2 - 2 sum b_c + sum g_c + 2 sum_{i<j} pair_ij
 * (params.mu_sqnorm is not read: mu is part of X0).  H <= PM_MAX_H, Hprime <= PM_MAX_HPRIME, S <= 65535. */
int pm_bsc_masked_estep_f64(const double *b, int64_t ldb, const double *g, int64_t ldg, const double *xnorm2,
                            const uint8_t *mask, int64_t ldm, const double *Wt, int64_t ldw, const uint16_t *state_masks,
                            int64_t S, const pm_bsc_estep_params *params_host, int64_t N, int64_t H, int64_t D,
                            int64_t Hprime, int32_t *cand, double *logpj, int64_t ldl, void *stream);
/* MCA / MMCA selection scores R[n,h] = sum_d m_d max(W[h,d] - Y[n,d], 0): pm_mca_select_scores_f64 over the observed
 * dimensions. */
int pm_mca_masked_select_scores_f64(const double *Y, int64_t ldy, const uint8_t *mask, int64_t ldm, const double *W,
                                    int64_t ldw, double *R, int64_t ldr, int64_t N, int64_t H, int64_t D, void *stream);
/* MCA / MMCA E-step: pm_mca_estep_f64 with e_s = sum_d m_d (X0[n,d] - Wbar_d(s))^2 for the multi-cause states and, for the
 * one-cause states, the per-row wnorm2_obs (N, ldwn >= H) = Mf . (W o W), scores = X0 . W and xnorm2, all from
 * pm_masked_prepare_f64 with mu = NULL.  Same power functions, limits (D <= 1024) and outputs. */
int pm_mca_masked_estep_f64(const double *scores, int64_t lds, const double *wnorm2_obs, int64_t ldwn, const double *xnorm2,
                            const double *X0, int64_t ldx, const uint8_t *mask, int64_t ldm, const double *Wrho,
                            const int32_t *cand, const uint16_t *state_masks, int64_t S, const pm_mca_params *params_host,
                            int64_t N, int64_t H, int64_t D, int64_t Hprime, double *logpj, int64_t ldl, double *lse1,
                            double *lseb, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-entry noise weights: weighted E-steps for inference (weighted_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * weight (N, ldo >= D) doubles omega >= 0, finite (the caller checks; the kernels do not): entry (n, d) was observed with noise
 * variance sigma^2 / omega_nd, omega_nd = 0: not observed.  The masked entries above are the case omega in {0, 1}: on such
 * weights every entry here performs exactly their operations and returns their bits.  A value at weight 0 is selected away
 * where it is read (omega != 0 ? v : 0), never multiplied: NaN or inf there changes no bit of any output.  No atomics, every
 * output element is written once by one lane and a row's sums over d run in an order fixed by D alone: both builds return the
 * same bits and a row's bits depend on that row (of the data and of the weights) and on the parameters alone.  Every entry
 * checks its arguments before it touches a device: PM_EINVAL for a null pointer, a negative size or a short leading
 * dimension, PM_ERANGE past a limit; N == 0 launches nothing.
 *
 * pm_weighted_prepare_f64: with on = omega != 0 and x = on ? Y[n,d] - mu[d] : 0 (mu NULL: 0):  Xw[n,d] = on ? omega x : 0,
 * Om[n,d] = on ? omega : 0, X0[n,d] = x (X0 may be NULL), xnorm2[n] = sum_d fma(Xw, x, .) = sum_d omega x^2, dn[n] = number
 * of dimensions with omega != 0, logw[n] = sum_{on} log omega -- each per lane over d = lane, lane + 64, ... in ascending
 * order, then the xor butterfly (the order of pm_masked_prepare_f64).  With these the terms that are dense over H are two
 * products of pm_gemm_nt_rows_f64: b = Xw . W (N, H) and diag G_n = Om . (W o W) (N, H). */
int pm_weighted_prepare_f64(const double *Y, int64_t ldy, const double *weight, int64_t ldo, const double *mu, int64_t N,
                            int64_t D, double *Xw, int64_t ldxw, double *Om, int64_t ldom, double *X0, int64_t ldx0,
                            double *xnorm2, int32_t *dn, double *logw, void *stream);
/* BSC: pm_bsc_masked_estep_f64 with the pair products sum_d omega_d Wt[c_i, d] Wt[c_j, d]: the candidates' rows of Wt enter LDS
 * in slabs of 64 dimensions as omega != 0 ? w : 0 beside one staged row of omega, pair p is owned by lane p mod 64, which walks
 * d in ascending order with fma(wi * omega, wj, .).  Same selection (the Hprime largest b_h / sqrt(g_h), ascending, ties
 * towards the larger index; a row of zero weights gets the Hprime largest indices), log-joint layout and limits:
 * H <= PM_MAX_H, Hprime <= PM_MAX_HPRIME, S <= 65535. */
int pm_bsc_weighted_estep_f64(const double *b, int64_t ldb, const double *g, int64_t ldg, const double *xnorm2,
                              const double *weight, int64_t ldo, const double *Wt, int64_t ldw, const uint16_t *state_masks,
                              int64_t S, const pm_bsc_estep_params *params_host, int64_t N, int64_t H, int64_t D,
                              int64_t Hprime, int32_t *cand, double *logpj, int64_t ldl, void *stream);
/* MCA selection scores R[n,h] = sum_d omega_d max(W[h,d] - Y[n,d], 0): per output one thread walks d in ascending order with
 * acc = omega != 0 ? fma(omega, max(w - y, 0), acc) : acc. */
int pm_mca_weighted_select_scores_f64(const double *Y, int64_t ldy, const double *weight, int64_t ldo, const double *W,
                                      int64_t ldw, double *R, int64_t ldr, int64_t N, int64_t H, int64_t D, void *stream);
/* MCA / MMCA E-step: pm_mca_masked_estep_f64 with e_s = sum_d omega_d (X0[n,d] - Wbar_d(s))^2, per dimension
 * omega != 0 ? fma(omega df, df, e) : e; for the one-cause states wnorm2_obs (N, ldwn >= H) = Om . (W o W), scores = Xw . W and
 * xnorm2, all from pm_weighted_prepare_f64 with mu = NULL.  Same power functions, limits (D <= 1024, Hprime <= PM_MAX_HPRIME)
 * and outputs. */
int pm_mca_weighted_estep_f64(const double *scores, int64_t lds, const double *wnorm2_obs, int64_t ldwn, const double *xnorm2,
                              const double *X0, int64_t ldx, const double *weight, int64_t ldo, const double *Wrho,
                              const int32_t *cand, const uint16_t *state_masks, int64_t S, const pm_mca_params *params_host,
                              int64_t N, int64_t H, int64_t D, int64_t Hprime, double *logpj, int64_t ldl, double *lse1,
                              double *lseb, void *stream);

/* ---------------------------------------------------------------------------------------
 * Missing values: the M-step of BSC on incomplete rows (masked_train.hip)
 * ---------------------------------------------------------------------------------------
 * With a mask every data dimension d has its own normal equations A_d w_d = r_d, A_d = sum_n m_nd E_q[s s^T]_n (H x H).  No
 * atomics: every output element is written once and every sum over rows runs in ascending row order, so both builds return
 * the same bits on every run.  Every entry checks its arguments before it touches a device (PM_EINVAL: null pointer,
 * negative size, short leading dimension; PM_ERANGE: past a limit); N == 0 launches nothing.
 *
 * pm_bsc_mtrain_rows_f64: from a row's log-joints (layout of pm_bsc_masked_estep_f64), its log-sum-exp lse[n] (pm_rows_lse_f64),
 * its candidates and the state masks, with q(s) = exp(logpj_s - lse): es[n,h] = E[s_h] (lde >= H), q2[n,p] = sum of q over the
 * table states holding both candidates of pair p, pairs in the order (0,1), (0,2), ..., (Hprime-2, Hprime-1) (ldq >=
 * Hprime (Hprime - 1) / 2; q2 may be NULL at Hprime = 1), energy[n] = sum_s q(s) e_s with e_s = (logpj_s - prior_scale pil_bar
 * |s|) / ecoef, the energy the E-step scaled (params.ecoef < 0, else PM_EINVAL).  H <= PM_MAX_H, Hprime <= PM_MAX_HPRIME,
 * S <= 65535.  A row's outputs depend on that row alone. */
int pm_bsc_mtrain_rows_f64(const double *logpj, int64_t ldl, const double *lse, const int32_t *cand,
                           const uint16_t *state_masks, int64_t S, const pm_bsc_estep_params *params_host, int64_t N,
                           int64_t H, int64_t Hprime, double *es, int64_t lde, double *q2, int64_t ldq, double *energy,
                           void *stream);
/* out[c] = sum_n X[n,c] (X: N x C, ld >= C) in a fixed order: workgroups add fixed row ranges (a function of N alone) in
 * ascending order into work (pm_col_sum_ordered_work_len(N, C) doubles), the partials are added in index order.  N == 0
 * launches nothing and leaves out as it is. */
int64_t pm_col_sum_ordered_work_len(int64_t N, int64_t C);
int pm_col_sum_ordered_f64(const double *X, int64_t ld, int64_t N, int64_t C, double *work, double *out, void *stream);
/* A (D, H, H) dense: A[d, c_i, c_j] = A[d, c_j, c_i] = sum_n m_nd q2[n, (i,j)] over the rows' candidates cand (N, Hprime), each
 * cell added in ascending n; A[d, h, h] = diag[h, d] (H, ldd >= D: the dense product E[s]^T Mf); every other cell 0.  A
 * candidate outside [0, H) or a pair of equal candidates is skipped.  A workgroup owns 64 dimensions x
 * pm_bsc_mtrain_pairs_tile_rows(H) latent rows x H columns in LDS.  H <= 256, Hprime <= PM_MAX_HPRIME, D H^2 <= 2^28,
 * N <= INT32_MAX. */
int pm_bsc_mtrain_pairs_f64(const int32_t *cand, const double *q2, int64_t ldq, const uint8_t *mask, int64_t ldm,
                            const double *diag, int64_t ldd, int64_t N, int64_t D, int64_t H, int64_t Hprime, double *A,
                            void *stream);
int64_t pm_bsc_mtrain_pairs_tile_rows(int64_t H);
/* Behind pm_spd_inverse_batch_f64 (batch = D): Wt_new[h,d] = (Ainv_d r_d + Ainv_d (r_d - A_d Ainv_d r_d))[h] with r_d = r[:, d]
 * (H, ldr >= D), A and Ainv dense symmetric (D, H, H), where pivots (D, 2) = [smallest, largest] pass smallest > 0 and
 * smallest / largest > 1e-11; elsewhere Wt_new[:, d] = Wt_old[:, d] bit for bit.  status[d] = 1 solved, 0 kept.  H <= 256,
 * D H^2 <= 2^28. */
int pm_bsc_mtrain_solve_f64(const double *A, const double *Ainv, const double *pivots, const double *r, int64_t ldr,
                            const double *Wt_old, int64_t ldw, int64_t D, int64_t H, double *Wt_new, int64_t ldo,
                            int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------
 * Posterior draws of the noiseless data (posterior_sample.hip)
 * ---------------------------------------------------------------------------------------
 * ybar(s) for s ~ q_n(s) = exp(a logpj[n,s] + o_s - lse_n) over exactly the states and weights of the reconstruction entries
 * above.  No atomics and no branch on the build: every output element is written once by one lane, both builds
 * return the same bits and a row's values depend on that row's inputs alone.  Every entry checks its arguments before it
 * touches a device (PM_EINVAL: null pointer, negative size, short leading dimension, inconsistent layout; PM_ERANGE: past a
 * limit); N == 0 launches nothing.
 *
 * pm_sample_states_f64: the categorical draws.  logpj (N, ld >= K), a, col_offset as pm_recon_expect_f64; lse NULL: the rows'
 * log-sum-exp of a logpj + o by a maximum pass and a sum pass, else the caller's normaliser (N values, with any a and o; zeros
 * leave the weights un-normalised, as GSC's E-step forms them).  The weight of column k is w_k = exp(a logpj[n,k] + o_k -
 * lse_n), raised to weight_floor (>= 0; GSC: DBL_MIN) in every column but null_col (-1: in every column).  U (N, ldu >= M): the uniforms; idx (N, M) int32: for each, the column drawn.  With c the running sum of w in the
 * order below and C its last value, the draw for u is the smallest k with fl(u C) < c_k.  Order: lane l of the row's wavefront
 * owns the columns [l seg, (l + 1) seg), seg = ceil(K / 64) | 1; p_k = the lane's weights added in ascending k; base_l = the
 * lanes' totals added in ascending lane order; c_k = base_l + p_k (every + one rounded f64 addition).  c is non-decreasing and
 * stays put over a column of weight 0 by construction, so whatever U holds: 0 <= idx < K, a column of weight 0 is never
 * returned, u = 0 gives the first column of positive weight and the largest double below 1 the last one; a u that is NaN or
 * outside [0, 1) is clamped into [0, 1 - 2^-53].  A row with a NaN weight (a NaN log-joint), or whose weights do not sum to a
 * positive finite value, returns -1 for every sample and touches no other row.  K <= pm_sample_states_max_cols() (the CDF of a row
 * lives in the LDS of its wavefront). */
int64_t pm_sample_states_max_cols(void);
int pm_sample_states_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset,
                         double weight_floor, int64_t null_col, const double *U, int64_t ldu, int64_t N, int64_t K, int64_t M,
                         int32_t *idx, void *stream);
/* idx (N, M) -> the active list of each draw: act_idx (N, M, A) int32 the latents, act_val (N, M, A) their values, in ascending
 * candidate position; the column layout (single_off, nblocks, block_values_host, multi_off, S, state_vals, cand, Hprime) is
 * pm_recon_expect_f64's.  A one-cause column gives one entry, a table state one entry per position of non-zero value (a latent
 * held by two positions (TSC) appears twice; entries past A are dropped: A >= the table's largest support), any other column
 * (the null state) none.  Unused slots: index -1, value 0.  A draw of -1: index -1 and value NaN in every slot.  A candidate
 * outside [0, H) is clamped into it.  1 <= A <= PM_MAX_HPRIME, Hprime <= PM_MAX_HPRIME, nblocks <= 8. */
int pm_sample_active_f64(const int32_t *idx, const int32_t *cand, const double *state_vals, const double *block_values_host,
                         int64_t N, int64_t M, int64_t H, int64_t Hprime, int64_t K, int64_t single_off, int64_t nblocks,
                         int64_t multi_off, int64_t S, int64_t A, int32_t *act_idx, double *act_val, void *stream);
/* GSC: the same list format with the values z | s, y_n ~ N(kappa_s, Lambda_s^-1) of the DRAWN state alone.  idx (N, M) over the
 * columns [null ; H singletons ; S multi-cause states] (state_masks over the candidate positions as pm_gsc_estep_f64), cand
 * (N, Hprime), and what the E-step pass was given: scores (N, lds >= H) = Y Sigma^-1 W, G (H, H) = W^T Sigma^-1 W, psi_sq (H,
 * H), tables (8 H) and s2 (> 0).  E (N, M, lde >= gamma): the standard normals of each draw.  Singleton h: z = kappa_h + E[n,m,0]
 * / sqrt(lambda_h) from the tables.  Multi-cause state on the candidates a (ascending position, g <= gamma of them): Lambda =
 * G_aa / s2 + (psi_aa)^-1, kappa = mu_a + Lambda^-1 (scores_a - G_aa mu_a) / s2, z = kappa + L E[n,m,0..g), L the lower Cholesky
 * factor of Lambda^-1: at most 8 x 8 per (row, sample), one lane each, sums in ascending index.  A matrix that is not positive
 * definite gives NaN values; a draw of -1 the list of pm_sample_active_f64.  gamma <= 8, gamma <= A <= PM_MAX_HPRIME. */
int pm_sample_gsc_f64(const int32_t *idx, const int32_t *cand, const uint16_t *state_masks, const double *scores, int64_t lds,
                      const double *G, const double *psi_sq, const double *tables, double s2, const double *E, int64_t lde,
                      int64_t N, int64_t M, int64_t H, int64_t Hprime, int64_t S, int64_t gamma, int64_t A, int32_t *act_idx,
                      double *act_val, void *stream);
/* out[n ld_row + m ld_sample + d] = mu[d] + sum_j act_val[n,m,j] Wt[act_idx[n,m,j], d], d < D: one fma per entry in ascending
 * j, starting from mu[d] (NULL: 0); Wt (H, ldw >= D) the transpose of W.  A gather of at most A rows, not a dense product.  A
 * slot of index -1 adds nothing unless its value is NaN (a draw of -1), which makes the whole output row NaN.  Both output
 * strides are the caller's (>= D; (M, N, D): ld_row = D, ld_sample = N D).  Any D; A <= PM_MAX_HPRIME. */
int pm_sample_decode_lin_f64(const int32_t *act_idx, const double *act_val, int64_t A, const double *Wt, int64_t ldw,
                             const double *mu, int64_t N, int64_t M, int64_t H, int64_t D, double *out, int64_t ld_row,
                             int64_t ld_sample, void *stream);
/* MCA (signed_w = 0) / MMCA (1), columns [null ; H one-cause ; S multi-cause] as pm_recon_mca_f64: out[n, m, :] = 0 for the null
 * state, Wt[h, :] for a one-cause state (Wt (H, D), leading dimension D), Wbar(s) = (sum_{j in s} Wrho[cand[n,j], :])^inv_rho
 * (signed: sign(t) |t|^inv_rho) for a multi-cause state, the sum in ascending position and the power functions of
 * pm_recon_mca_f64; NaN for a draw of -1.  Output strides as above.  D <= 1024, Hprime <= PM_MAX_HPRIME. */
int pm_sample_decode_mca_f64(const int32_t *idx, const int32_t *cand, const uint16_t *state_masks, const double *Wt,
                             const double *Wrho, double inv_rho, int signed_w, int64_t N, int64_t M, int64_t H, int64_t D,
                             int64_t Hprime, int64_t S, double *out, int64_t ld_row, int64_t ld_sample, void *stream);

/* ---------------------------------------------------------------------------------------
 * k-means++ seeding of the mixture models (seed_kernels.hip)
 * ---------------------------------------------------------------------------------------
 * D^2 sampling over a shard Y (N, ldy >= D): H rounds of [update the distance of every row to its nearest chosen centre,
 * draw the next centre with probability proportional to it].  Every sum is a chain of plain IEEE additions of rounded terms
 * in a pinned order -- no fused multiply-add, no atomics, no branch on the build: both libraries return the same bits, and
 * tests/seeding_reference.py restates them in NumPy.
 *
 * Distance of row n to a centre c: with g the smallest power of two >= min(D, 64), partial sum l (l < g) adds t t, t =
 * Y[n,d] - c[d] (difference rounded, product rounded), for d = l, l + g, l + 2g, ... in ascending order starting from +0; the
 * g partial sums are combined by butterflies v_l <- v_l + v_(l xor o) for o = g/2, ..., 1.  A row's distance depends on that
 * row and the centre alone.
 *
 * Blocks: rpb = ceil(N / min(1024, ceil(N / 16))) rows per block, nb = ceil(N / rpb) blocks -- a function of N alone.  B_b
 * adds the distances of block b in ascending n starting from +0; Q_b = ((B_0 + B_1) + ...) + B_b; S = Q_(nb-1) is the
 * shard's potential.  `work` holds [B (nb) | Q (nb)]: pm_seed_work_len(N) = 2 max(nb, 1) doubles (-1 for N < 0 or N > 2^40).
 *
 * Every entry checks its arguments before it touches a device: PM_EINVAL for a null pointer (where not allowed below), a
 * non-positive D or nc, a negative N or H, a leading dimension shorter than D; PM_ERANGE for N > 2^40 and, in the entries
 * that keep the centre in LDS (update, plan), D > 6144.  N == 0 launches nothing.
 *
 * pm_seed_plan: host-only query, N >= 1.  out[0..PM_SEED_PLAN_LEN): 0 rpb, 1 nb, 2 g, 3 rows per wavefront (64 / max(g/2, 1):
 * a row belongs to max(g/2, 1) lanes, each holding two neighbouring partial sums, so that 16-byte loads keep the order),
 * 4 grid of the update kernel (one workgroup per block), 5 wavefronts per workgroup, 6 dynamic LDS bytes, 7 trips of a lane
 * over a row's pairs of elements.  Rows of Y that all start at a 16-byte boundary (Y aligned, ldy even) are read with 16-byte
 * loads, the last element of an odd row and every other shard with 8-byte loads; the bits are the same. */
#define PM_SEED_PLAN_LEN 8
int64_t pm_seed_work_len(int64_t N);
int pm_seed_plan(int64_t N, int64_t D, int32_t *out);
/* One round's pass over the shard.  The centre is row *idx_dev of centre_src (nc rows, ldc >= D; idx_dev NULL: row 0), read on
 * the device.  first != 0: dist[n] <- d(n, c); else dist[n] <- d(n, c) < dist[n] ? d(n, c) : dist[n], an explicit compare (a row
 * that is a centre keeps exactly 0; a NaN distance never replaces a number).  Then B, Q into `work` and S into
 * *potential_out (NULL: not written).  *idx_dev < 0 or >= nc (an exhausted shard: no row left to draw) leaves dist as it is and
 * writes B = Q = 0 and S = 0.  Two launches. */
int pm_seed_update_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, const double *centre_src, int64_t ldc, int64_t nc,
                       const int64_t *idx_dev, int first, double *dist, double *work, double *potential_out, void *stream);
/* The draw from dist (N) and the `work` the update left: t = u S' + t_offset (product rounded, sum rounded), S' = *S (device) or,
 * S NULL, the shard's own S; a one-rank caller passes S NULL and t_offset 0, so that t is formed on the device.  b* = the
 * smallest block with Q_b* > t; r = Q_(b*-1) (+0 for block 0), then r <- r + dist[n] over the block's rows in ascending n: the
 * drawn row is the first with r > t.  If the block ends before that (the two chains differ in rounding), the last row of the
 * block with dist > 0; if no block has Q_b > t (t rounded up to S), the last block with B_b > 0 is walked in the same way.  A
 * row of distance 0 is never drawn.  *idx_out receives the row, or -1 where the shard's S == 0 or no row has a positive
 * distance.  One workgroup. */
int pm_seed_pick_f64(const double *dist, int64_t N, const double *work, const double *S, double t_offset, double u,
                     int64_t *idx_out, void *stream);
/* centres[h, :] = Y[idx[h], :] for h < H (ldc >= D); a row with idx[h] outside [0, N) is left as it is. */
int pm_seed_gather_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, const int64_t *idx, int64_t H, double *centres,
                       int64_t ldc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PROSPER_HIP_H */

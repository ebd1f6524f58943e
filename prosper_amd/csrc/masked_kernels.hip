// Missing values: the E-steps of BSC and MCA / MMCA for data rows of which only the dimensions with a non-zero
// mask byte were observed.  The unobserved dimensions leave the likelihood: with m the row's mask,
//   BSC   e_s = sum_d m_d (x_d - sum_{h in s} W_dh)^2 = |x|^2_obs - 2 sum_{h in s} b_h + sum_{h,h' in s} G_n[h,h'],
//         b = W^T diag(m) x,  G_n = W^T diag(m) W  -- a Gram matrix PER DATAPOINT: the shared H x H table of the unmasked
//         kernels is gone.  b and diag G_n are dense over H and stay MFMA work (two pm_gemm_nt_rows_f64 calls on the
//         outputs of pm_masked_prepare_f64); the H'(H'-1)/2 off-diagonal entries over the row's candidates are formed here;
//   MCA   e_s = sum_d m_d (y_d - Wbar_d(s))^2, selection score sum_d m_d max(W_hd - y_d, 0).
// An unobserved value is never an operand: it is selected away (m ? v : 0) where it is read, so NaN or inf there changes
// no bit.  No atomics; every output element is written once by one lane; a row's reductions run in an order fixed by D
// alone -- both builds return the same bits and a row's bits do not depend on the rows around it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_common.h"
#include "mca_rows.h"
#include "obs_rows.h"      // the BSC and MCA / MMCA row kernels, shared with weighted_kernels.hip

namespace {

constexpr int WAVES = OBS_WAVES;

// ---------------------------------------------------------------------------------------------
// prepare: X0 = m ? y - mu : 0, Mf = m ? 1 : 0, |X0|^2, D_n.  One wavefront per row, lane l owns d = l, l + 64, ...
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void masked_prepare_kernel(const double *__restrict__ Y, int64_t ldy,
                                                              const uint8_t *__restrict__ mask, int64_t ldm,
                                                              const double *__restrict__ mu, int64_t N, int D,
                                                              double *__restrict__ X0, int64_t ldx, double *__restrict__ Mf,
                                                              int64_t ldf, double *__restrict__ xnorm2,
                                                              int32_t *__restrict__ dn) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * WAVES;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const uint8_t *mrow = mask + n * ldm;
        const double *yrow = Y + n * ldy;
        double acc = 0.0;
        int cnt = 0;
        for (int d = lane; d < D; d += 64) {
            const bool on = mrow[d] != 0;
            const double x = on ? yrow[d] - (mu ? mu[d] : 0.0) : 0.0;
            X0[n * ldx + d] = x;
            if (Mf) Mf[n * ldf + d] = on ? 1.0 : 0.0;
            acc = fma(x, x, acc);
            cnt += on ? 1 : 0;
        }
        acc = pm_wave_sum(acc);
        cnt = wave_sum_i32(cnt);
        if (lane == 0) {
            xnorm2[n] = acc;
            dn[n] = cnt;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// MCA: R[n,h] = sum_d m_d max(W[h,d] - Y[n,d], 0).  64 x 64 output tile per workgroup, 4 x 4 per thread, D in slabs of 16
// through LDS (the layout of mca_select_scores_kernel).  An unobserved y enters the slab as +inf: max(w - inf, 0) = 0, the
// value itself is never read into the arithmetic.  One thread owns an output and walks d in ascending order.
// ---------------------------------------------------------------------------------------------
constexpr int ST = 64, SK = 16, SLD = SK + 2;

__global__ __launch_bounds__(256) void mca_masked_select_scores_kernel(const double *__restrict__ Y, int64_t ldy,
                                                                        const uint8_t *__restrict__ mask, int64_t ldm,
                                                                        const double *__restrict__ W, int64_t ldw,
                                                                        double *__restrict__ R, int64_t ldr, int64_t N, int H,
                                                                        int D, int tiles_h) {
    __shared__ __attribute__((aligned(16))) double sy[ST * SLD], sw[ST * SLD];
    const int tid = threadIdx.x;
    const int64_t n0 = (int64_t)(blockIdx.x / tiles_h) * ST;
    const int h0 = (blockIdx.x % tiles_h) * ST;
    const int tr = tid >> 4, tc = tid & 15;  // thread tile: rows tr + 16 a, cols tc + 16 b
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.0;

    for (int k0 = 0; k0 < D; k0 += SK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + 256 * e, r = idx >> 4, c = idx & 15;
            const int64_t n = n0 + r;
            double yv = 0.0, wv = 0.0;      // padding: max(0 - 0, 0) = 0
            if (n < N && k0 + c < D) yv = mask[n * ldm + k0 + c] != 0 ? Y[n * ldy + k0 + c] : INFINITY;
            if (h0 + r < H && k0 + c < D) wv = W[(int64_t)(h0 + r) * ldw + k0 + c];
            sy[r * SLD + c] = yv;
            sw[r * SLD + c] = wv;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SK; ++k) {
            double yv[4], wv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) yv[a] = sy[(tr + 16 * a) * SLD + k];
#pragma unroll
            for (int c = 0; c < 4; ++c) wv[c] = sw[(tc + 16 * c) * SLD + k];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] += fmax(wv[c] - yv[a], 0.0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t n = n0 + tr + 16 * a;
        if (n >= N) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int h = h0 + tc + 16 * c;
            if (h < H) R[n * ldr + h] = acc[a][c];
        }
    }
}

}  // namespace

extern "C" int pm_masked_prepare_f64(const double *Y, int64_t ldy, const uint8_t *mask, int64_t ldm, const double *mu,
                                     int64_t N, int64_t D, double *X0, int64_t ldx, double *Mf, int64_t ldf, double *xnorm2,
                                     int32_t *dn, void *stream) {
    if (!Y || !mask || !X0 || !xnorm2 || !dn || N < 0 || D <= 0 || ldy < D || ldm < D || ldx < D || (Mf && ldf < D))
        return PM_EINVAL;
    if (D > INT32_MAX) return PM_ERANGE;
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(masked_prepare_kernel, dim3((unsigned)pm_row_grid(N, WAVES)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), Y, ldy, mask, ldm, mu, N, (int)D, X0, ldx, Mf, ldf, xnorm2, dn);
    return (int)hipGetLastError();
}

extern "C" int pm_bsc_masked_estep_f64(const double *b, int64_t ldb, const double *g, int64_t ldg, const double *xnorm2,
                                       const uint8_t *mask, int64_t ldm, const double *Wt, int64_t ldw,
                                       const uint16_t *state_masks, int64_t S, const pm_bsc_estep_params *params_host,
                                       int64_t N, int64_t H, int64_t D, int64_t Hprime, int32_t *cand, double *logpj,
                                       int64_t ldl, void *stream) {
    return bsc_obs_estep_launch<uint8_t>(b, ldb, g, ldg, xnorm2, mask, ldm, Wt, ldw, state_masks, S, params_host, N, H, D,
                                         Hprime, cand, logpj, ldl, stream);
}

extern "C" int pm_mca_masked_select_scores_f64(const double *Y, int64_t ldy, const uint8_t *mask, int64_t ldm,
                                               const double *W, int64_t ldw, double *R, int64_t ldr, int64_t N, int64_t H,
                                               int64_t D, void *stream) {
    if (!Y || !mask || !W || !R || N < 0 || H <= 0 || D <= 0 || ldy < D || ldm < D || ldw < D || ldr < H) return PM_EINVAL;
    if (H > INT32_MAX || D > INT32_MAX) return PM_ERANGE;
    const int tiles_h = (int)((H + ST - 1) / ST);
    const int64_t blocks = (N + ST - 1) / ST * tiles_h;
    if (blocks > INT32_MAX) return PM_ERANGE;
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(mca_masked_select_scores_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), Y, ldy, mask, ldm, W, ldw, R, ldr, N, (int)H, (int)D, tiles_h);
    return (int)hipGetLastError();
}

extern "C" int pm_mca_masked_estep_f64(const double *scores, int64_t lds, const double *wnorm2_obs, int64_t ldwn,
                                       const double *xnorm2, const double *X0, int64_t ldx, const uint8_t *mask, int64_t ldm,
                                       const double *Wrho, const int32_t *cand, const uint16_t *state_masks, int64_t S,
                                       const pm_mca_params *params_host, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                                       double *logpj, int64_t ldl, double *lse1, double *lseb, void *stream) {
    return mca_obs_estep_launch<uint8_t>(scores, lds, wnorm2_obs, ldwn, xnorm2, X0, ldx, mask, ldm, Wrho, cand, state_masks, S,
                                         params_host, N, H, D, Hprime, logpj, ldl, lse1, lseb, stream);
}
#undef MCA_ROW_TAIL
#undef MCA_STATS_EPILOGUE

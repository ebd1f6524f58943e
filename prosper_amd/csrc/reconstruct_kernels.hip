// reconstruct(): posterior-mean denoising  yhat_n = sum_{s in K_n} q_n(s) ybar(s),  q_n(s) = exp(a lpj[n,s] -
// rowLSE_n), from the log-joints an E-step pass left on the device (any leading dimension: the padded BSC buffers are read in
// place), the candidates and the state tables.
//
//   recon_expect_kernel   E[s] (N, H) of the linear models (BSC, DSC, TSC) -- and with one block of unit value and no table the
//                         normalised weights of the leading H states themselves: MCA / MMCA's one-cause weights, a mixture's
//                         responsibilities (softmax of a X + o).  Yhat = E[s] W^T (+ mu: a column of ones) is then one launch
//                         of pm_gemm_nt_rows_f64.
//   recon_mca_kernel      (recon_mca.h, shared with the variance) MCA / MMCA: Yhat_nd += sum_{multi-cause s} q_n(s) Wbar_d(s),
//                         Wbar with the E-step's own powers.
//
// One wavefront per datapoint in both; the sums over a row's states run in a fixed order (lane-strided partial sums, xor
// butterflies) and every output element is written by one lane: no atomics, the same bits in both library builds and whatever
// the other rows hold.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_common.h"
#include "recon_mca.h"

namespace {

constexpr int REC_THREADS = 256;
constexpr int REC_WAVES = REC_THREADS / 64;
static_assert(REC_WAVES == RMCA_WAVES, "rec_grid sizes recon_mca_kernel's grid: one row per wavefront");
constexpr int64_t REC_MAX_BLOCKS = 8192;

// Columns of a row: [soff, soff + nblk H) one-cause blocks (block c: latent h takes the value bv.v[c]), [moff, moff + S) the
// table states (state s: the latent at candidate position j takes tab[s, j]); every other column (the null state) carries
// weight but no value.  out[n, h] = E[s_h] for h < H, then 1 in column `ones_col` and 0 up to `out_cols` (the K padding of
// the product that follows).  A latent that sits at two candidate positions (TSC) receives both positions' sums.
__global__ __launch_bounds__(REC_THREADS) void recon_expect_kernel(
    const double *__restrict__ X, int64_t ld, const double *__restrict__ lse_in, double a, const double *__restrict__ off,
    const int32_t *__restrict__ cand, const double *__restrict__ tab, int64_t N, int H, int Hp, int K, int soff, int nblk,
    pm_blockvals bv, int moff, int S, double *__restrict__ out, int64_t ldo, int out_cols, int ones_col) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * REC_WAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * REC_WAVES;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *row = X + n * ld;
        const double lse = lse_in ? lse_in[n] : pm_row_lse(row, K, a, off, lane);
        // ---- table states: per candidate position, sum_s q_s tab[s, j]
        double t[PM_MAX_HPRIME];
        int cj[PM_MAX_HPRIME];
#pragma unroll
        for (int j = 0; j < PM_MAX_HPRIME; ++j) {
            t[j] = 0.0;
            cj[j] = -1;
        }
        if (S > 0) {
            for (int s = lane; s < S; s += 64) {
                const double q = exp(a * row[moff + s] + (off ? off[moff + s] : 0.0) - lse);
                const double *ts = tab + (int64_t)s * Hp;
#pragma unroll
                for (int j = 0; j < PM_MAX_HPRIME; ++j)
                    if (j < Hp) t[j] = fma(q, ts[j], t[j]);
            }
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j)
                if (j < Hp) {
                    t[j] = pm_wave_sum(t[j]);
                    cj[j] = cand[n * Hp + j];
                }
        }
        // ---- one-cause blocks, plus the table sums of the positions that hold this latent (position order)
        double *orow = out + n * ldo;
        for (int h = lane; h < H; h += 64) {
            double e = 0.0;
            for (int c = 0; c < nblk; ++c) {
                const int k = soff + c * H + h;
                e = fma(exp(a * row[k] + (off ? off[k] : 0.0) - lse), bv.v[c], e);
            }
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j)
                if (j < Hp && cj[j] == h) e += t[j];
            orow[h] = e;
        }
        for (int h = H + lane; h < out_cols; h += 64) orow[h] = (h == ones_col) ? 1.0 : 0.0;
    }
}

unsigned rec_grid(int64_t N) {
    int64_t nb = (N + REC_WAVES - 1) / REC_WAVES;
    if (nb > REC_MAX_BLOCKS) nb = REC_MAX_BLOCKS;
    return (unsigned)nb;
}

}  // namespace

extern "C" int pm_recon_expect_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset,
                                   const int32_t *cand, const double *state_vals, const double *block_values_host, int64_t N,
                                   int64_t H, int64_t Hprime, int64_t K, int64_t single_off, int64_t nblocks, int64_t multi_off,
                                   int64_t S, double *out, int64_t ldo, int64_t out_cols, int64_t ones_col, void *stream) {
    if (N < 0 || H <= 0 || K <= 0 || ld < K || out_cols < H || ldo < out_cols || single_off < 0 || nblocks < 0 ||
        multi_off < 0 || S < 0 || Hprime < 0 || (S > 0 && Hprime == 0) || !(ones_col == -1 || (ones_col >= H && ones_col < out_cols)))
        return PM_EINVAL;
    if (N == 0) return PM_OK;
    if (!logpj || !out || (nblocks > 0 && !block_values_host) || (S > 0 && (!cand || !state_vals)) ||
        (lse && (a != 1.0 || col_offset)))
        return PM_EINVAL;
    if (Hprime > PM_MAX_HPRIME || nblocks > PM_MAX_BLOCKVALS || K > INT32_MAX / 2 || H > INT32_MAX / 16 ||
        out_cols > INT32_MAX / 2)
        return PM_ERANGE;
    if (single_off + nblocks * H > K || multi_off + S > K) return PM_EINVAL;
    pm_blockvals bv;
    for (int c = 0; c < PM_MAX_BLOCKVALS; ++c) bv.v[c] = c < nblocks ? block_values_host[c] : 0.0;
    hipLaunchKernelGGL(recon_expect_kernel, dim3(rec_grid(N)), dim3(REC_THREADS), 0, static_cast<hipStream_t>(stream), logpj,
                       ld, lse, a, col_offset, cand, state_vals, N, (int)H, (int)Hprime, (int)K, (int)single_off,
                       (int)nblocks, bv, (int)multi_off, (int)S, out, ldo, (int)out_cols, (int)ones_col);
    return (int)hipGetLastError();
}

extern "C" int pm_recon_mca_f64(const double *logpj, int64_t ld, const double *lse, const int32_t *cand,
                                const uint16_t *state_masks, const double *Wrho, double inv_rho, int signed_w, int64_t N,
                                int64_t H, int64_t D, int64_t Hprime, int64_t S, double *Yhat, int64_t ldy, void *stream) {
    if (N < 0 || H <= 0 || D <= 0 || Hprime <= 0 || S < 0 || ld < 1 + H + S || ldy < D || !(inv_rho > 0.0)) return PM_EINVAL;
    if (D > 1024 || Hprime > PM_MAX_HPRIME || H > INT32_MAX / 2048 || S > INT32_MAX / 2) return PM_ERANGE;
    if (N == 0 || S == 0) return PM_OK;
    if (!logpj || !cand || !state_masks || !Wrho || !Yhat) return PM_EINVAL;
    return recon_mca_launch<false>(rec_grid(N), logpj, ld, lse, cand, state_masks, Wrho, inv_rho, signed_w, N, H, D, Hprime, S,
                                   Yhat, ldy, stream);
}

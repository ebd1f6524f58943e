// The MCA / MMCA read-out over the multi-cause states, shared by reconstruct() (pm_recon_mca_f64, reconstruct_kernels.hip)
// and its variance (pm_recon_mca_var_f64, recon_var.hip):
//   out[n, d] += sum_s q_n(s) f(Wbar_d(s)),   f(w) = w (the mean) or w^2 (SQUARE: the second moment),
// q = exp(lpj[n, 1 + H + s] - lse_n) over the S multi-cause states, Wbar_d(s) = (sum_{j in s} Wrho[c_j, d])^(1/rho) (MMCA:
// signed) with the sum in ascending position order and the power functions of mca_estep_kernel, so that Wbar is the E-step's.
// One wavefront per datapoint; lane l holds dimensions l, l + 64, ...: D <= 64 DPL.  Every output element is written by one
// lane and every sum runs in state order: no atomics, the same bits in both library builds.
#ifndef PM_RECON_MCA_H
#define PM_RECON_MCA_H

#include "pm_common.h"
#include "prosper_hip.h"

constexpr int RMCA_THREADS = 256;
constexpr int RMCA_WAVES = RMCA_THREADS / 64;

template <int DPL, bool SQUARE>
static __global__ __launch_bounds__(RMCA_THREADS) void recon_mca_kernel(const double *__restrict__ X, int64_t ld,
                                                                        const double *__restrict__ lse_in,
                                                                        const int32_t *__restrict__ cand,
                                                                        const uint16_t *__restrict__ masks,
                                                                        const double *__restrict__ Wrho, double inv_rho,
                                                                        int signed_w, int64_t N, int H, int D, int Hp, int S,
                                                                        double *__restrict__ out, int64_t ldo) {
    __shared__ __attribute__((aligned(16))) double s_tab[PM_POWTAB_LEN];
    const int tid = threadIdx.x, lane = tid & 63;
    bool r21, r6;
    pm_mca_pow_setup(s_tab, inv_rho, signed_w, tid, blockDim.x, r21, r6);
    __syncthreads();
    const int K = 1 + H + S;
    const int64_t wave0 = (int64_t)blockIdx.x * RMCA_WAVES + (tid >> 6), nwaves = (int64_t)gridDim.x * RMCA_WAVES;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *row = X + n * ld;
        const double lse = lse_in ? lse_in[n] : pm_row_lse(row, K, 1.0, nullptr, lane);
        int64_t coff[PM_MAX_HPRIME];
#pragma unroll
        for (int j = 0; j < PM_MAX_HPRIME; ++j) {
            int c = (j < Hp) ? cand[n * Hp + j] : 0;
            c = c < 0 ? 0 : (c >= H ? H - 1 : c);
            coff[j] = (int64_t)c * D;
        }
        double acc[DPL];
#pragma unroll
        for (int i = 0; i < DPL; ++i) acc[i] = 0.0;
        for (int s = 0; s < S; ++s) {
            const unsigned m = masks[s];
            const double q = exp(row[1 + H + s] - lse);
            double T[DPL];
#pragma unroll
            for (int i = 0; i < DPL; ++i) T[i] = 0.0;
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j) {
                if ((m >> j) & 1u) {          // uniform
                    const double *src = Wrho + coff[j];
#pragma unroll
                    for (int i = 0; i < DPL; ++i) {
                        const int d = lane + 64 * i;
                        T[i] += (d < D) ? src[d] : 0.0;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < DPL; ++i) {
                const double wbar = pm_mca_wbar(T[i], inv_rho, r21, r6, s_tab);
                acc[i] = fma(q, SQUARE ? wbar * wbar : wbar, acc[i]);
            }
        }
        double *orow = out + n * ldo;
#pragma unroll
        for (int i = 0; i < DPL; ++i) {
            const int d = lane + 64 * i;
            if (d < D) orow[d] += acc[i];
        }
    }
}

// The launch for D <= 1024 on `grid` workgroups (each entry's own cap).
template <bool SQUARE>
static int recon_mca_launch(unsigned grid, const double *logpj, int64_t ld, const double *lse, const int32_t *cand,
                            const uint16_t *state_masks, const double *Wrho, double inv_rho, int signed_w, int64_t N,
                            int64_t H, int64_t D, int64_t Hprime, int64_t S, double *out, int64_t ldo, void *stream) {
    auto *kernel = recon_mca_kernel<16, SQUARE>;
    if (D <= 64) kernel = recon_mca_kernel<1, SQUARE>;
    else if (D <= 128) kernel = recon_mca_kernel<2, SQUARE>;
    else if (D <= 256) kernel = recon_mca_kernel<4, SQUARE>;
    else if (D <= 512) kernel = recon_mca_kernel<8, SQUARE>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(RMCA_THREADS), 0, static_cast<hipStream_t>(stream), logpj, ld, lse, cand,
                       state_masks, Wrho, inv_rho, signed_w, N, (int)H, (int)D, (int)Hprime, (int)S, out, ldo);
    return (int)hipGetLastError();
}

#endif  // PM_RECON_MCA_H

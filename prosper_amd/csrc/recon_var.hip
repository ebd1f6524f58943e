// reconstruct(variance=True): the posterior variance of the noiseless value,
//   V_nd = E_q[ybar_d(s)^2] - yhat_nd^2,   q_n(s) = exp(a lpj[n,s] + o_s - rowLSE_n),
// over exactly the states of reconstruct(), from the log-joints an E-step pass left on the device.
//
//   recon_moments2_kernel   the second moments of the latents of the linear models: m2 (N, H) per latent and p (N, H'(H'-1)/2)
//                           per pair of candidate positions.  E[((W s)_d)^2] = sum_h m2_h W_dh^2 + 2 sum_{i<j} p_ij W_d,c_i
//                           W_d,c_j; the first sum is one launch of pm_gemm_nt_rows_f64 against W o W.
//   recon_gsc_moments2_kernel  GSC: the same m2 and p of u = s o z, assembled from the E-step pass's log-joints, its
//                           un-normalised multi-cause sums (pm_gsc_estep_lpj_blocks_f64) and the per-latent tables.
//   recon_var_finish_kernel V (holding the product) += 2 sum_p p W_d,c_i W_d,c_j, -= (yhat - mu)^2, clamped at 0.
//   recon_mca_kernel<DPL, true> (recon_mca.h)  MCA / MMCA: V += sum_{multi-cause s} q(s) Wbar_d(s)^2, reconstruct()'s kernel
//                           with the square.
//
// One wavefront per datapoint in all four.  No atomics and no branch on the build; every output element is written once by
// one lane, and every sum runs in an order fixed by the shapes (H, H', S, D) alone: a lane adds its states in ascending
// state number and its pairs in ascending pair number, with no reduction across lanes after the row's log-sum-exp.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_common.h"
#include "recon_mca.h"

namespace {

constexpr int RV_WAVES = 4;               // wavefronts per workgroup, one row each
constexpr int RV_THREADS = 64 * RV_WAVES;
static_assert(RV_WAVES == RMCA_WAVES, "rv_grid sizes recon_mca_kernel's grid: one row per wavefront");
constexpr int RV_CHUNK = 256;             // table states per LDS chunk of a wavefront
constexpr int64_t RV_MAX_BLOCKS = 2048;   // 8 workgroups per CU, grid-stride beyond: the second trip starts at row 8192
constexpr int RV_MAX_PAIRS = PM_MAX_HPRIME * (PM_MAX_HPRIME - 1) / 2;

unsigned rv_grid(int64_t N) {
    int64_t nb = (N + RV_WAVES - 1) / RV_WAVES;
    if (nb > RV_MAX_BLOCKS) nb = RV_MAX_BLOCKS;
    return (unsigned)nb;
}

// Columns of a row as in recon_expect_kernel.  Lane l owns the pairs l and l + 64 (order (0,1), (0,2), ..., (H'-2, H'-1)) and,
// for l < H', candidate position l: it adds q(s) v_i v_j (q(s) v_l^2) over the table states in ascending s.  m2[n, h] = sum_c
// bv[c]^2 q(block c, h) in block order, then the position sums of the positions that hold h in position order; 0 in the
// columns [H, out_cols).
__global__ __launch_bounds__(RV_THREADS) void recon_moments2_kernel(
    const double *__restrict__ X, int64_t ld, const double *__restrict__ lse_in, double a, const double *__restrict__ off,
    const int32_t *__restrict__ cand, const double *__restrict__ tab, int64_t N, int H, int Hp, int K, int soff, int nblk,
    pm_blockvals bv, int moff, int S, double *__restrict__ m2, int64_t ldm, int out_cols, double *__restrict__ p,
    int64_t ldp) {
    __shared__ double s_q[RV_WAVES][RV_CHUNK];
    __shared__ double s_m[RV_WAVES][PM_MAX_HPRIME];
    __shared__ int32_t s_c[RV_WAVES][PM_MAX_HPRIME];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npair = Hp * (Hp - 1) / 2;
    // what this lane owns; a lane without a pair (position) reads position 0 and writes nothing
    int i0 = 0, j0 = 0, i1 = 0, j1 = 0;
    {
        int k = 0;
        for (int i = 0; i < Hp; ++i)
            for (int j = i + 1; j < Hp; ++j, ++k) {
                if (k == lane) i0 = i, j0 = j;
                if (k == lane + 64) i1 = i, j1 = j;
            }
    }
    const int pos = lane < Hp ? lane : 0;
    double *wq = s_q[wave], *wm = s_m[wave];
    int32_t *wc = s_c[wave];
    const int64_t wave0 = (int64_t)blockIdx.x * RV_WAVES + wave, nwaves = (int64_t)gridDim.x * RV_WAVES;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *row = X + n * ld;
        const double lse = lse_in ? lse_in[n] : pm_row_lse(row, K, a, off, lane);
        double a0 = 0.0, a1 = 0.0, am = 0.0;
        for (int s0 = 0; s0 < S; s0 += RV_CHUNK) {
            const int cnt = min(RV_CHUNK, S - s0);
            for (int k = lane; k < cnt; k += 64)
                wq[k] = exp(a * row[moff + s0 + k] + (off ? off[moff + s0 + k] : 0.0) - lse);
            pm_wave_lds_sync();
            for (int k = 0; k < cnt; ++k) {
                const double q = wq[k];
                const double *ts = tab + (int64_t)(s0 + k) * Hp;
                a0 = fma(q, ts[i0] * ts[j0], a0);
                a1 = fma(q, ts[i1] * ts[j1], a1);
                am = fma(q, ts[pos] * ts[pos], am);
            }
            pm_wave_lds_sync();
        }
        if (p) {
            if (lane < npair) p[n * ldp + lane] = a0;
            if (lane + 64 < npair) p[n * ldp + lane + 64] = a1;
        }
        if (lane < Hp) {
            wm[lane] = am;
            wc[lane] = S > 0 ? cand[n * Hp + lane] : -1;
        }
        pm_wave_lds_sync();
        double *orow = m2 + n * ldm;
        for (int h = lane; h < H; h += 64) {
            double e = 0.0;
            for (int c = 0; c < nblk; ++c) {
                const int k = soff + c * H + h;
                e = fma(exp(a * row[k] + (off ? off[k] : 0.0) - lse), bv.v[c] * bv.v[c], e);
            }
            if (S > 0)
                for (int i = 0; i < Hp; ++i)
                    if (wc[i] == h) e += wm[i];
            orow[h] = e;
        }
        for (int h = H + lane; h < out_cols; h += 64) orow[h] = 0.0;
        pm_wave_lds_sync();      // wm / wc are rewritten for the next row
    }
}

// V[n, d] <- max(V[n, d] + 2 sum_{i<j} p[n, (i,j)] Wt[c_i, d] Wt[c_j, d] - (Yhat[n, d] - mu[d])^2, 0), the pairs added in
// ascending pair number; a NaN stays NaN.  Lane l holds dimensions l, l + 64, ...: any D.
__global__ __launch_bounds__(RV_THREADS) void recon_var_finish_kernel(double *__restrict__ V, int64_t ldv,
                                                                      const double *__restrict__ Yhat, int64_t ldy,
                                                                      const double *__restrict__ mu,
                                                                      const double *__restrict__ p, int64_t ldp,
                                                                      const int32_t *__restrict__ cand,
                                                                      const double *__restrict__ Wt, int64_t ldw, int64_t N,
                                                                      int H, int D, int Hp) {
    __shared__ double s_p[RV_WAVES][RV_MAX_PAIRS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npair = p ? Hp * (Hp - 1) / 2 : 0;
    double *wp = s_p[wave];
    const int64_t wave0 = (int64_t)blockIdx.x * RV_WAVES + wave, nwaves = (int64_t)gridDim.x * RV_WAVES;
    for (int64_t n = wave0; n < N; n += nwaves) {
        int64_t coff[PM_MAX_HPRIME];
#pragma unroll
        for (int j = 0; j < PM_MAX_HPRIME; ++j) coff[j] = 0;
        if (npair > 0) {
            for (int k = lane; k < npair; k += 64) wp[k] = p[n * ldp + k];
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j) {
                int c = (j < Hp) ? cand[n * Hp + j] : 0;
                c = c < 0 ? 0 : (c >= H ? H - 1 : c);
                coff[j] = (int64_t)c * ldw;
            }
            pm_wave_lds_sync();
        }
        double *vrow = V + n * ldv;
        const double *yrow = Yhat + n * ldy;
        for (int d = lane; d < D; d += 64) {
            double acc = 0.0;
            if (npair > 0) {
                double w[PM_MAX_HPRIME];
#pragma unroll
                for (int j = 0; j < PM_MAX_HPRIME; ++j) w[j] = (j < Hp) ? Wt[coff[j] + d] : 0.0;
                int k = 0;
#pragma unroll
                for (int i = 0; i < PM_MAX_HPRIME - 1; ++i)
#pragma unroll
                    for (int j = i + 1; j < PM_MAX_HPRIME; ++j)
                        if (j < Hp) {      // uniform; k runs over the pairs in the order of p
                            acc = fma(wp[k], w[i] * w[j], acc);
                            ++k;
                        }
            }
            const double c = yrow[d] - (mu ? mu[d] : 0.0);
            const double v = fma(2.0, acc, vrow[d]) - c * c;
            vrow[d] = v < 0.0 ? 0.0 : v;
        }
        if (npair > 0) pm_wave_lds_sync();      // wp is rewritten for the next row
    }
}

// GSC: m2 and p of u = s o z from what the E-step pass left per row -- the log-joints lp (columns [null ; H singletons ; S
// multi-cause states]), the un-normalised multi-cause sums `blk` of pm_gsc_estep_lpj_blocks_f64 and the scores a = y^T Sigma^-1
// W.  The weights are the E-step's: exp(beta lp) floored at DBL_MIN (NaN included) for every state but the null state,
// Z = p_0 + sum_h p_h + sum_multi p_s, normaliser 1 / (Z + DBL_MIN).  A singleton contributes p_h (kappa_h^2 + 1 / lambda_h)
// with kappa_h = (a_h - gm_h) kl_h + mu_h from the per-latent tables; the multi-cause states the candidate block of sum_s p_s
// (kappa kappa^T + Lambda^-1).  Z: lane-strided partial sums over h in ascending h, the null state in lane 0, a butterfly,
// then the multi-cause total.
__device__ __forceinline__ double rv_gsc_weight(double x) {
    const double tiny = 2.2250738585072014e-308;
    if (!(x >= -708.3964185322641)) return tiny;      // (NaN included)
    const double e = exp(x);
    return e < tiny ? tiny : e;
}

__global__ __launch_bounds__(RV_THREADS) void recon_gsc_moments2_kernel(
    const double *__restrict__ lp, int64_t ldl, const double *__restrict__ blk, int64_t ldb,
    const double *__restrict__ scores, int64_t lds, const double *__restrict__ tables, const int32_t *__restrict__ cand,
    double beta, int64_t N, int H, int Hp, double *__restrict__ m2, int64_t ldm, int out_cols, double *__restrict__ p,
    int64_t ldp) {
    const double tiny = 2.2250738585072014e-308;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HH = Hp * Hp, npair = Hp * (Hp - 1) / 2;
    const double *gm = tables + 2 * (int64_t)H, *kl = tables + 4 * (int64_t)H, *ilam = tables + 5 * (int64_t)H,
                 *mu = tables + 6 * (int64_t)H;
    const int64_t wave0 = (int64_t)blockIdx.x * RV_WAVES + wave, nwaves = (int64_t)gridDim.x * RV_WAVES;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *row = lp + n * ldl;
        const double *b = blk ? blk + n * ldb : nullptr;
        double z = lane == 0 ? exp(beta * row[0]) : 0.0;      // the null state is not floored
        for (int h = lane; h < H; h += 64) z += rv_gsc_weight(beta * row[1 + h]);
        z = pm_wave_sum(z);
        if (b) z += b[2 * HH + 2 * Hp];
        const double nf = 1.0 / (z + tiny);
        double *orow = m2 + n * ldm;
        const double *arow = scores + n * lds;
        for (int h = lane; h < H; h += 64) {
            const double kap = (arow[h] - gm[h]) * kl[h] + mu[h];
            double e = rv_gsc_weight(beta * row[1 + h]) * (kap * kap + ilam[h]) * nf;
            if (b)
                for (int i = 0; i < Hp; ++i)
                    if (cand[n * Hp + i] == h) e += b[HH + i * Hp + i] * nf;
            orow[h] = e;
        }
        for (int h = H + lane; h < out_cols; h += 64) orow[h] = 0.0;
        if (p) {
            for (int k = lane; k < npair; k += 64) {
                // pair k = (i, j), i < j, in the order (0,1), (0,2), ...
                int i = 0, r = k;
                while (r >= Hp - 1 - i) {
                    r -= Hp - 1 - i;
                    ++i;
                }
                const int j = i + 1 + r;
                // kappa kappa^T + Lambda^-1 is symmetric only while psi_sq is: the pair term takes both triangles
                p[n * ldp + k] = b ? 0.5 * (b[HH + i * Hp + j] + b[HH + j * Hp + i]) * nf : 0.0;
            }
        }
    }
}

}  // namespace

extern "C" int pm_recon_moments2_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset,
                                     const int32_t *cand, const double *state_vals, const double *block_values_host,
                                     int64_t N, int64_t H, int64_t Hprime, int64_t K, int64_t single_off, int64_t nblocks,
                                     int64_t multi_off, int64_t S, double *m2, int64_t ldm, int64_t out_cols, double *p,
                                     int64_t ldp, void *stream) {
    if (N < 0 || H <= 0 || K <= 0 || ld < K || out_cols < H || ldm < out_cols || single_off < 0 || nblocks < 0 ||
        multi_off < 0 || S < 0 || Hprime < 0 || (S > 0 && Hprime == 0))
        return PM_EINVAL;
    if (Hprime > PM_MAX_HPRIME || nblocks > PM_MAX_BLOCKVALS || K > INT32_MAX / 2 || H > INT32_MAX / 16 ||
        out_cols > INT32_MAX / 2)
        return PM_ERANGE;
    const int64_t npair = Hprime * (Hprime - 1) / 2;
    if (!logpj || !m2 || (nblocks > 0 && !block_values_host) || (S > 0 && (!cand || !state_vals)) ||
        (S > 0 && npair > 0 && !p) || (p && ldp < npair) || (lse && (a != 1.0 || col_offset)))
        return PM_EINVAL;
    if (single_off + nblocks * H > K || multi_off + S > K) return PM_EINVAL;
    if (N == 0) return PM_OK;
    pm_blockvals bv;
    for (int c = 0; c < PM_MAX_BLOCKVALS; ++c) bv.v[c] = c < nblocks ? block_values_host[c] : 0.0;
    hipLaunchKernelGGL(recon_moments2_kernel, dim3(rv_grid(N)), dim3(RV_THREADS), 0, static_cast<hipStream_t>(stream), logpj,
                       ld, lse, a, col_offset, cand, state_vals, N, (int)H, (int)Hprime, (int)K, (int)single_off,
                       (int)nblocks, bv, (int)multi_off, (int)S, m2, ldm, (int)out_cols, p, ldp);
    return (int)hipGetLastError();
}

extern "C" int pm_recon_gsc_moments2_f64(const double *logpj, int64_t ldl, const double *blocks, int64_t ldb,
                                         const double *scores, int64_t lds, const double *tables, const int32_t *cand,
                                         double beta, int64_t N, int64_t H, int64_t Hprime, int64_t S, double *m2, int64_t ldm,
                                         int64_t out_cols, double *p, int64_t ldp, void *stream) {
    if (N < 0 || H <= 0 || Hprime <= 0 || S < 0 || ldl < 1 + H + S || lds < H || out_cols < H || ldm < out_cols ||
        !(beta > 0.0))
        return PM_EINVAL;
    if (Hprime > PM_MAX_HPRIME || H > INT32_MAX / 16 || out_cols > INT32_MAX / 2) return PM_ERANGE;
    const int64_t npair = Hprime * (Hprime - 1) / 2;
    if (!logpj || !scores || !tables || !m2 || (blocks && (!cand || ldb < 2 * Hprime * Hprime + 2 * Hprime + 1)) ||
        (blocks && npair > 0 && !p) || (p && ldp < npair))
        return PM_EINVAL;
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(recon_gsc_moments2_kernel, dim3(rv_grid(N)), dim3(RV_THREADS), 0, static_cast<hipStream_t>(stream),
                       logpj, ldl, blocks, ldb, scores, lds, tables, cand, beta, N, (int)H, (int)Hprime, m2, ldm,
                       (int)out_cols, p, ldp);
    return (int)hipGetLastError();
}

extern "C" int pm_recon_var_finish_f64(double *V, int64_t ldv, const double *Yhat, int64_t ldy, const double *mu,
                                       const double *p, int64_t ldp, const int32_t *cand, const double *Wt, int64_t ldw,
                                       int64_t N, int64_t H, int64_t D, int64_t Hprime, void *stream) {
    if (N < 0 || H <= 0 || D <= 0 || Hprime < 0 || ldv < D || ldy < D) return PM_EINVAL;
    const bool pairs = p && Hprime >= 2;
    if (pairs && Hprime > PM_MAX_HPRIME) return PM_ERANGE;
    if (D > INT32_MAX / 2 || H > INT32_MAX / 2) return PM_ERANGE;
    if (!V || !Yhat) return PM_EINVAL;
    if (pairs && (!cand || !Wt || ldw < D || ldp < Hprime * (Hprime - 1) / 2)) return PM_EINVAL;
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(recon_var_finish_kernel, dim3(rv_grid(N)), dim3(RV_THREADS), 0, static_cast<hipStream_t>(stream), V,
                       ldv, Yhat, ldy, mu, pairs ? p : nullptr, ldp, cand, Wt, ldw, N, (int)H, (int)D, (int)Hprime);
    return (int)hipGetLastError();
}

extern "C" int pm_recon_mca_var_f64(const double *logpj, int64_t ld, const double *lse, const int32_t *cand,
                                    const uint16_t *state_masks, const double *Wrho, double inv_rho, int signed_w, int64_t N,
                                    int64_t H, int64_t D, int64_t Hprime, int64_t S, double *V, int64_t ldv, void *stream) {
    if (N < 0 || H <= 0 || D <= 0 || Hprime <= 0 || S < 0 || ld < 1 + H + S || ldv < D || !(inv_rho > 0.0)) return PM_EINVAL;
    if (D > 1024 || Hprime > PM_MAX_HPRIME || H > INT32_MAX / 2048 || S > INT32_MAX / 2) return PM_ERANGE;
    if (!logpj || !cand || !state_masks || !Wrho || !V) return PM_EINVAL;
    if (N == 0 || S == 0) return PM_OK;
    return recon_mca_launch<true>(rv_grid(N), logpj, ld, lse, cand, state_masks, Wrho, inv_rho, signed_w, N, H, D, Hprime, S, V,
                                  ldv, stream);
}

// The row kernels that masked_kernels.hip and weighted_kernels.hip share, written once: the BSC
// selection + pair products + log-joints of one row per wavefront, and the MCA / MMCA E-step.  OBS is the element type of the
// row's observation record:
//   uint8_t   a mask byte, non-zero = observed: the dimension enters with weight 1
//   double    a weight omega >= 0 (finite; checked by the host), 0 = not observed: the dimension enters omega times
// A dimension whose record is 0 is selected away where it is read, never multiplied.  The weighted forms are chosen so that
// omega in {0, 1} performs exactly the masked operations (1 * w is w): both give the same bits there.
// No atomics; every output element is written once by one lane; a row's reductions run in an order fixed by the shapes alone.
// The including unit defines MCA_ROW_TAIL (mca_rows.h) and #undef's it at its end.
#ifndef PM_OBS_ROWS_H
#define PM_OBS_ROWS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "prosper_hip.h"
#include "pm_common.h"
#include "mca_rows.h"

namespace {

constexpr int OBS_WAVES = 4;  // wavefronts per workgroup (BSC / prepare kernels)
constexpr int OBS_WLD = 65;   // LDS row of a 64-dimension slab of a candidate's W row: 65 doubles, lanes on different rows hit different banks

template <class OBS>
constexpr bool obs_weighted() {
    return std::is_same<OBS, double>::value;
}

// doubles of LDS per wavefront of bsc_obs_estep_kernel: [ ac (16) | gc (256) | w (16 * OBS_WLD) | c (16 x int32) | om (64, weights only) ]
template <class OBS>
constexpr int bsc_obs_per_wave() {
    return 16 + 256 + 16 * OBS_WLD + 8 + (obs_weighted<OBS>() ? 64 : 0);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, PM_WAVE);
    return v;
}

// ---------------------------------------------------------------------------------------------
// BSC: selection + log-joints of one row per wavefront.
//   select   the H' largest b_h / sqrt(g_h) (g_h = G_n[h,h]; 0 where g_h = 0), ascending, ties towards the larger index: the
//            order and tie rule of pm_bsc_select_f64
//   pairs    P_ij = sum_d o_d W[d,c_i] W[d,c_j], i < j (o the mask or the weight): the candidates' rows of W^T come from L2
//            in slabs of 64 dimensions (selected on the way into LDS, the weights beside them as one staged row); pair p is
//            owned by lane p % 64, which walks d in ascending order -- one fused multiply-add per dimension, no reduction
//            across lanes, so the order is fixed by D alone
//   logpj    columns [null ; H singletons ; S table states] as pm_bsc_estep_f64 writes them
// ---------------------------------------------------------------------------------------------
template <int VPL, class OBS>  // latents per lane: H <= 64 * VPL
__global__ __launch_bounds__(256) void bsc_obs_estep_kernel(const double *__restrict__ b, int64_t ldb,
                                                             const double *__restrict__ g, int64_t ldg,
                                                             const double *__restrict__ xnorm2,
                                                             const OBS *__restrict__ obs, int64_t ldo,
                                                             const double *__restrict__ Wt, int64_t ldw,
                                                             const uint16_t *__restrict__ masks, int S,
                                                             pm_bsc_estep_params P, int64_t N, int H, int D, int Hp,
                                                             int32_t *__restrict__ cand, double *__restrict__ logpj,
                                                             int64_t ldl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool WEIGHTED = obs_weighted<OBS>();
    constexpr int WAVES = OBS_WAVES, WLD = OBS_WLD;
    constexpr int PER_WAVE = bsc_obs_per_wave<OBS>();
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *s_base = reinterpret_cast<double *>(smem);
    double *s_ac = s_base + wave * PER_WAVE;
    double *s_gc = s_ac + 16;
    double *s_w = s_gc + 256;
    int32_t *s_c = reinterpret_cast<int32_t *>(s_w + 16 * WLD);
    double *s_om = s_w + 16 * WLD + 8;  // (weights only)
    uint16_t *s_masks = reinterpret_cast<uint16_t *>(s_base + WAVES * PER_WAVE);
    for (int s = tid; s < S; s += 256) s_masks[s] = masks[s];
    __syncthreads();

    // the (at most two) candidate pairs this lane owns: p = lane, lane + 64 in the order (0,1), (0,2), ..., (Hp-2,Hp-1)
    const int npair = Hp * (Hp - 1) / 2;
    int pi_[2] = {0, 0}, pj_[2] = {0, 0};
    {
        int p = 0;
        for (int i = 0; i < Hp; ++i)
            for (int j = i + 1; j < Hp; ++j, ++p) {
                if (p == lane) { pi_[0] = i; pj_[0] = j; }
                if (p == lane + 64) { pi_[1] = i; pj_[1] = j; }
            }
    }
    const bool own0 = lane < npair, own1 = lane + 64 < npair;

    unsigned invalid = 0;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i >= H) invalid |= 1u << i;

    const double ppil = P.prior_scale * P.pil_bar;
    const int64_t wave0 = (int64_t)blockIdx.x * WAVES + wave;
    const int64_t nwaves = (int64_t)gridDim.x * WAVES;

    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *brow = b + n * ldb;
        const double *grow = g + n * ldg;
        const OBS *orow = obs + n * ldo;

        // ---- selection
        double v[VPL];
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int h = lane + 64 * i;
            double x = -INFINITY;
            if (h < H) {
                const double gh = grow[h];
                x = gh > 0.0 ? brow[h] / sqrt(gh) : 0.0;
                if (x != x) x = -INFINITY;      // NaN (an observed NaN in the row) ranks lowest
            }
            v[i] = x;
        }
        unsigned taken = invalid;
        for (int r = 0; r < Hp; ++r) {
            double bv = -INFINITY;
            int bi = -1;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const int h = lane + 64 * i;
                const bool free_slot = !((taken >> i) & 1u);
                if (free_slot && (v[i] > bv || (v[i] == bv && h > bi))) {
                    bv = v[i];
                    bi = h;
                }
            }
            pm_wave_argmax(bv, bi);
            if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
            if (lane == 0) {
                cand[n * Hp + (Hp - 1 - r)] = bi;  // ascending: best candidate last
                s_c[Hp - 1 - r] = bi;
            }
        }
        pm_wave_lds_sync();

        // ---- pair products of the candidates' rows of W^T over the observed dimensions
        double a0 = 0.0, a1 = 0.0;
        for (int d0 = 0; d0 < D; d0 += 64) {
            const int d = d0 + lane;
            OBS ov = 0;
            if (d < D) ov = orow[d];
            const bool on = ov != 0;
            if constexpr (WEIGHTED) s_om[lane] = on ? (double)ov : 0.0;
            for (int j = 0; j < Hp; ++j) {
                double w = 0.0;
                if (on) w = Wt[(int64_t)s_c[j] * ldw + d];
                s_w[j * WLD + lane] = w;
            }
            pm_wave_lds_sync();
            if (own0) {
                const double *wi = s_w + pi_[0] * WLD, *wj = s_w + pj_[0] * WLD;
#pragma unroll 8
                for (int k = 0; k < 64; ++k) {
                    if constexpr (WEIGHTED) a0 = fma(wi[k] * s_om[k], wj[k], a0);
                    else a0 = fma(wi[k], wj[k], a0);
                }
            }
            if (own1) {
                const double *wi = s_w + pi_[1] * WLD, *wj = s_w + pj_[1] * WLD;
#pragma unroll 8
                for (int k = 0; k < 64; ++k) {
                    if constexpr (WEIGHTED) a1 = fma(wi[k] * s_om[k], wj[k], a1);
                    else a1 = fma(wi[k], wj[k], a1);
                }
            }
            pm_wave_lds_sync();
        }
        if (own0) {
            s_gc[pi_[0] * Hp + pj_[0]] = a0;
            s_gc[pj_[0] * Hp + pi_[0]] = a0;
        }
        if (own1) {
            s_gc[pi_[1] * Hp + pj_[1]] = a1;
            s_gc[pj_[1] * Hp + pi_[1]] = a1;
        }
        if (lane < Hp) {
            const int c = s_c[lane];
            s_ac[lane] = brow[c];
            s_gc[lane * Hp + lane] = grow[c];
        }
        pm_wave_lds_sync();

        // ---- log-joints
        const double yn = xnorm2[n];
        double *out = logpj + n * ldl;
        if (lane == 0) out[0] = P.ecoef * yn;
        for (int h = lane; h < H; h += 64) {
            const double e = grow[h] - 2.0 * brow[h] + yn;
            out[1 + h] = ppil + P.ecoef * e;
        }
        for (int s = lane; s < S; s += 64) {
            const unsigned mask_s = s_masks[s];
            double lin = 0.0, quad = 0.0;
            unsigned mi = mask_s;
            while (mi) {
                const int i = __builtin_ctz(mi);
                mi &= mi - 1;
                lin += s_ac[i];
                quad += s_gc[i * Hp + i];
                unsigned mj = mi;  // j > i: symmetric, counted twice
                double off = 0.0;
                while (mj) {
                    const int j = __builtin_ctz(mj);
                    mj &= mj - 1;
                    off += s_gc[i * Hp + j];
                }
                quad += 2.0 * off;
            }
            const double e = yn - 2.0 * lin + quad;
            out[1 + H + s] = ppil * (double)__builtin_popcount(mask_s) + P.ecoef * e;
        }
        pm_wave_lds_sync();  // s_c / s_ac / s_gc are rewritten for the next datapoint
    }
}

// ---------------------------------------------------------------------------------------------
// MCA / MMCA E-step: mca_estep_kernel with the observation record in the per-pixel energy of the multi-cause states, the
// per-row |W_h|^2_obs (N, H) in the one-cause energies and |y|^2_obs.  X0: the prepared data (0 where unobserved).  Same
// power functions (pm_pow_m20_21 / pm_pow_m5_6 / pm_pow_tab), same outputs.  Energy of a dimension with df = Wbar - y:
// fma(df, df, e) under a mask, fma(omega * df, df, e) under a weight.
// ---------------------------------------------------------------------------------------------
template <int DPL, class OBS>  // dimensions per lane: D <= 64 * DPL
__global__ __launch_bounds__(256) void mca_obs_estep_kernel(const double *__restrict__ scores, int64_t lds,
                                                             const double *__restrict__ wnorm2, int64_t ldwn,
                                                             const double *__restrict__ xnorm2,
                                                             const double *__restrict__ X0, int64_t ldx,
                                                             const OBS *__restrict__ obs, int64_t ldo,
                                                             const double *__restrict__ Wrho,
                                                             const int32_t *__restrict__ cand,
                                                             const uint16_t *__restrict__ masks, int S, pm_mca_params P,
                                                             int64_t N, int H, int D, int Hp,
                                                             double *__restrict__ logpj, int64_t ldl,
                                                             double *__restrict__ lse1, double *__restrict__ lseb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // [ power tables (PM_POWTAB_LEN) | per wave: wr (Hp * DS) | e (S) ] ; DS = 64 * DPL
    constexpr bool WEIGHTED = obs_weighted<OBS>();
    constexpr int DS = 64 * DPL;
    const int waves = blockDim.x >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *s_tab = reinterpret_cast<double *>(smem);
    double *s_wr = s_tab + PM_POWTAB_LEN + (size_t)wave * (Hp * DS + S);
    double *s_e = s_wr + Hp * DS;
    pm_load_powtab(s_tab, tid, blockDim.x);
    const bool r21 = P.signed_w == 0.0 && P.inv_rho > 0.0 && fabs(1.0 / P.inv_rho - 21.0) < 1e-9;
    const bool r6 = P.inv_rho > 0.0 && fabs(1.0 / P.inv_rho - 6.0) < 1e-9;
    __syncthreads();

    const int64_t wave0 = (int64_t)blockIdx.x * waves + wave;
    const int64_t nwaves = (int64_t)gridDim.x * waves;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const int32_t *cn = cand + n * Hp;
        double y[DPL];
        OBS ov[DPL];      // the record: `ov[i] != 0` is "observed", and under a weight it is omega itself
#pragma unroll
        for (int i = 0; i < DPL; ++i) {
            const int d = lane + 64 * i;
            ov[i] = 0;
            if (d < D) ov[i] = obs[n * ldo + d];
            y[i] = ov[i] != 0 ? X0[n * ldx + d] : 0.0;
        }
        for (int j = 0; j < Hp; ++j) {
            const double *src = Wrho + (int64_t)cn[j] * D;
#pragma unroll
            for (int i = 0; i < DPL; ++i) {
                const int d = lane + 64 * i;
                s_wr[j * DS + d] = (d < D) ? src[d] : 0.0;
            }
        }
        pm_wave_lds_sync();

        auto states = [&](auto root_tag) {
            constexpr int ROOT = decltype(root_tag)::value;
            for (int s = 0; s < S; ++s) {
                unsigned m = masks[s];
                double T[DPL];
#pragma unroll
                for (int i = 0; i < DPL; ++i) T[i] = 0.0;
                while (m) {      // ascending candidate position: the order of the unmasked kernel's row sums
                    const int j = __builtin_ctz(m);
                    m &= m - 1;
                    const double *wr = s_wr + j * DS + lane;
#pragma unroll
                    for (int i = 0; i < DPL; ++i) T[i] += wr[64 * i];
                }
                double part = 0.0;
#pragma unroll
                for (int i = 0; i < DPL; ++i) {
                    const double aT = fabs(T[i]);
                    const double wbar = (aT > 0.0) ? (ROOT == 21 ? aT * pm_pow_m20_21(aT)
                                                      : ROOT == 6 ? copysign(aT * pm_pow_m5_6(aT), T[i])
                                                                  : copysign(pm_pow_tab(aT, P.inv_rho, s_tab), T[i]))
                                                   : 0.0;
                    const double df = wbar - y[i];
                    if constexpr (WEIGHTED) part = ov[i] != 0 ? fma((double)ov[i] * df, df, part) : part;
                    else part = ov[i] != 0 ? fma(df, df, part) : part;
                }
                part = pm_wave_sum_dpp(part);
                if (lane == 0) s_e[s] = part;
            }
        };
        if (r21) states(std::integral_constant<int, 21>{});
        else if (r6) states(std::integral_constant<int, 6>{});
        else states(std::integral_constant<int, 0>{});
        pm_wave_lds_sync();

        const double yn = xnorm2[n];
        const double *arow = scores + n * lds;
        const double *wrow = wnorm2 + n * ldwn;
        double *out = logpj + n * ldl;
        MCA_ROW_TAIL(wrow, yn, arow, out, lse1[n], lseb[n]);
        pm_wave_lds_sync();
    }
}

// LDS of one bsc_obs_estep_kernel launch, and of one wavefront of mca_obs_estep_kernel (host)
template <class OBS>
inline size_t bsc_obs_shmem(int64_t S) {
    return sizeof(double) * OBS_WAVES * bsc_obs_per_wave<OBS>() + sizeof(uint16_t) * (size_t)S;
}

template <class OBS>
inline int bsc_obs_estep_launch(const double *b, int64_t ldb, const double *g, int64_t ldg, const double *xnorm2,
                                const OBS *obs, int64_t ldo, const double *Wt, int64_t ldw, const uint16_t *state_masks,
                                int64_t S, const pm_bsc_estep_params *params_host, int64_t N, int64_t H, int64_t D,
                                int64_t Hprime, int32_t *cand, double *logpj, int64_t ldl, void *stream) {
    if (!b || !g || !xnorm2 || !obs || !Wt || !params_host || !cand || !logpj || N < 0 || H <= 0 || D <= 0 || Hprime <= 0 ||
        S < 0 || ldb < H || ldg < H || ldo < D || ldw < D || ldl < 1 + H + S || (S > 0 && !state_masks))
        return PM_EINVAL;
    if (H > PM_MAX_H || Hprime > PM_MAX_HPRIME || Hprime > H || S > 65535 || D > INT32_MAX) return PM_ERANGE;
    if (N == 0) return PM_OK;
    const size_t shmem = bsc_obs_shmem<OBS>(S);
    if (shmem > 160 * 1024) return PM_ERANGE;
    dim3 grid((unsigned)pm_row_grid(N, OBS_WAVES)), block(256);
    hipStream_t s = static_cast<hipStream_t>(stream);
#define PM_LAUNCH(V)                                                                                                   \
    do {                                                                                                               \
        auto kern = bsc_obs_estep_kernel<V, OBS>;                                                                      \
        if (int e = pm_allow_lds(reinterpret_cast<const void *>(kern), shmem)) return e;                               \
        hipLaunchKernelGGL(kern, grid, block, shmem, s, b, ldb, g, ldg, xnorm2, obs, ldo, Wt, ldw, state_masks, (int)S, \
                           *params_host, N, (int)H, (int)D, (int)Hprime, cand, logpj, ldl);                            \
    } while (0)
    if (H <= 64) PM_LAUNCH(1);
    else if (H <= 128) PM_LAUNCH(2);
    else if (H <= 256) PM_LAUNCH(4);
    else if (H <= 512) PM_LAUNCH(8);
    else PM_LAUNCH(16);
#undef PM_LAUNCH
    return (int)hipGetLastError();
}

template <class OBS>
inline int mca_obs_estep_launch(const double *scores, int64_t lds, const double *wnorm2_obs, int64_t ldwn,
                                const double *xnorm2, const double *X0, int64_t ldx, const OBS *obs, int64_t ldo,
                                const double *Wrho, const int32_t *cand, const uint16_t *state_masks, int64_t S,
                                const pm_mca_params *params_host, int64_t N, int64_t H, int64_t D, int64_t Hprime,
                                double *logpj, int64_t ldl, double *lse1, double *lseb, void *stream) {
    if (!scores || !wnorm2_obs || !xnorm2 || !X0 || !obs || !Wrho || !cand || !params_host || !logpj || !lse1 || !lseb ||
        N < 0 || H <= 0 || D <= 0 || Hprime <= 0 || S < 0 || lds < H || ldwn < H || ldx < D || ldo < D || ldl < 1 + H + S ||
        (S > 0 && !state_masks))
        return PM_EINVAL;
    if (D > 1024 || Hprime > PM_MAX_HPRIME || Hprime > H || S > 65535) return PM_ERANGE;
    const int dpl = D <= 64 ? 1 : D <= 128 ? 2 : D <= 256 ? 4 : D <= 512 ? 8 : 16;
    const size_t per_wave = sizeof(double) * ((size_t)Hprime * 64 * dpl + S);
    if (per_wave > 150 * 1024) return PM_ERANGE;
    if (N == 0) return PM_OK;
    const size_t shared = sizeof(double) * PM_POWTAB_LEN;
    const int waves = mca_pick_waves(per_wave, shared);
    const size_t shmem = shared + per_wave * waves;
    dim3 grid((unsigned)pm_row_grid(N, waves)), block(64 * waves);
    hipStream_t s = static_cast<hipStream_t>(stream);
#define PM_LAUNCH(V)                                                                                                   \
    do {                                                                                                               \
        auto kern = mca_obs_estep_kernel<V, OBS>;                                                                      \
        if (int e = pm_allow_lds(reinterpret_cast<const void *>(kern), shmem)) return e;                               \
        hipLaunchKernelGGL(kern, grid, block, shmem, s, scores, lds, wnorm2_obs, ldwn, xnorm2, X0, ldx, obs, ldo, Wrho, \
                           cand, state_masks, (int)S, *params_host, N, (int)H, (int)D, (int)Hprime, logpj, ldl, lse1,  \
                           lseb);                                                                                      \
    } while (0)
    switch (dpl) {
        case 1: PM_LAUNCH(1); break;
        case 2: PM_LAUNCH(2); break;
        case 4: PM_LAUNCH(4); break;
        case 8: PM_LAUNCH(8); break;
        default: PM_LAUNCH(16); break;
    }
#undef PM_LAUNCH
    return (int)hipGetLastError();
}

}  // namespace

#endif

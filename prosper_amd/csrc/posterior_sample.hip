// sample_posterior(): draws ybar(s), s ~ q_n(s) = exp(a lpj[n,s] + o_s - rowLSE_n), from the log-joints an E-step
// pass left on the device, the candidates and the state tables -- the states, weights and layout of reconstruct().
//
//   sample_states_kernel       categorical draws: idx (N, M) int32, the column drawn for each of a row's M uniforms.  One
//                              wavefront per row builds the row's CDF once in LDS and serves all M uniforms from it.
//   sample_active_kernel       idx -> the draw's active list (latent, value) x A in ascending candidate position (BSC, DSC,
//                              TSC, the mixtures; MCA / MMCA's latents).  One lane per (row, sample).
//   sample_decode_lin_kernel   out[n, m, :] = mu + sum_j act_val_j Wt[act_idx_j, :]: a gather of at most A rows of W^T, one
//                              wavefront per (row, sample), lanes over d, one fma per term in ascending j.
//   sample_decode_mca_kernel   MCA / MMCA: W_h for a one-cause state, the rho-combination Wbar(s) with the power functions of
//                              recon_mca_kernel for a multi-cause state, 0 for the null state.
//
// No atomics, no branch on the build; every output element is written once by one lane, and a row's values depend on that row's
// inputs alone.
//
// The CDF and its order.  Lane l owns the seg consecutive columns [l seg, (l + 1) seg), seg = ceil(K / 64) made odd (the lanes'
// LDS reads at stride seg then fall on distinct banks); columns past K carry weight 0.
//   p_k    = the lane's running sum of its weights up to and including k, in ascending k, starting from 0
//   base_l = base_{l-1} (+) (lane l-1's last p), base_0 = 0: the segment totals added in ascending lane order
//   c_k    = base_l (+) p_k,   C = base_63 (+) (lane 63's last p)
// ((+): one rounded f64 addition).  The sequence c is non-decreasing BY CONSTRUCTION and c_k == c_{k-1} wherever w_k == 0: inside
// a segment p is non-decreasing and rounding is monotone, and a segment's last c is the next segment's base, the same rounded
// sum.  The draw for u is the smallest k with fl(u C) < c_k (binary search): it exists because fl(u C) < C for every u < 1, it
// has c_k > c_{k-1} and therefore w_k > 0, u = 0 gives the first column of positive weight and u = 1 - 2^-53 the last one that
// moved c (fl((1 - 2^-53) C) >= the largest double below C).
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_common.h"

namespace {

constexpr int SMP_THREADS = 256;
constexpr int64_t SMP_MAX_BLOCKS = 8192;       // decode kernels: a wavefront per (row, sample)
constexpr int64_t SMP_ROW_BLOCKS = 2048;       // the other kernels: 8192 wavefronts fill the device; more rows take another trip
constexpr int SMP_LDS_DOUBLES = 8192;          // 64 KB: one wavefront's CDF at the largest K, four at K <= 1984
constexpr int SMP_MAX_ACTIVE = PM_MAX_HPRIME;

__host__ __device__ inline int smp_seg(int64_t K) { return (int)((K + 63) / 64) | 1; }

// blockDim.x = 64 * waves; dynamic LDS: waves * 64 * seg doubles.
__global__ __launch_bounds__(SMP_THREADS) void sample_states_kernel(
    const double *__restrict__ X, int64_t ld, const double *__restrict__ lse_in, double a, const double *__restrict__ off,
    double wfloor, int null_col, const double *__restrict__ U, int64_t ldu, int64_t N, int K, int M, int seg,
    int32_t *__restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) double smp_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    double *cdf = smp_lds + (int64_t)wave * 64 * seg;
    const int Kpad = 64 * seg;
    const int64_t wave0 = (int64_t)blockIdx.x * waves + wave, nwaves = (int64_t)gridDim.x * waves;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *row = X + n * ld;
        const double lse = lse_in ? lse_in[n] : pm_row_lse(row, K, a, off, lane);
        // ---- weights, column k at cdf[k] (coalesced reads of the row); a NaN weight marks the row
        int bad = (lse != lse);
        for (int k = lane; k < Kpad; k += 64) {
            double w = 0.0;
            if (k < K) {
                w = exp(a * row[k] + (off ? off[k] : 0.0) - lse);
                bad |= (w != w);                                // (before the floor: fmax drops a NaN)
                if (k != null_col) w = fmax(w, wfloor);
            }
            cdf[k] = w;
        }
        bad = __any(bad);
        pm_wave_sync();
        // ---- the lane's running sums, then the bases in ascending lane order, then c in place
        double *mine = cdf + lane * seg;
        double p = 0.0;
        for (int i = 0; i < seg; ++i) {
            p += mine[i];
            mine[i] = p;
        }
        double run = 0.0, base = 0.0;
        for (int l = 0; l < 64; ++l) {
            base = (l == lane) ? run : base;
            run += __shfl(p, l, 64);
        }
        for (int i = 0; i < seg; ++i) mine[i] = base + mine[i];
        pm_wave_sync();
        const double C = run;
        bad |= !(C > 0.0) || !(C < INFINITY);
        // ---- the draws: the row's CDF serves every uniform (the wave's own LDS region: no barrier)
        int32_t *irow = idx + n * (int64_t)M;
        for (int m = lane; m < M; m += 64) {
            int k = -1;
            if (!bad) {
                double u = U[n * ldu + m];
                u = (u >= 0.0) ? u : 0.0;                                     // NaN and negatives -> 0
                u = (u < 1.0) ? u : 0x1.fffffffffffffp-1;         // >= 1 -> 1 - 2^-53
                const double t = u * C;
                int lo = 0, hi = Kpad - 1;                                     // c[hi] == C > t
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (t < cdf[mid]) hi = mid;
                    else lo = mid + 1;
                }
                k = lo < K ? lo : K - 1;       // (lo < K always: the padding never moves c; the clamp guards the store)
            }
            irow[m] = k;
        }
        pm_wave_sync();          // (the next row's weights overwrite the CDF)
    }
}

// One lane per (row, sample).  Slots beyond the state's entries: index -1, value 0; a draw of -1 (NaN row): index -1, value NaN
// in every slot.
__global__ __launch_bounds__(SMP_THREADS) void sample_active_kernel(const int32_t *__restrict__ idx, const int32_t *__restrict__ cand,
                                                                    const double *__restrict__ tab, int64_t N, int M, int H,
                                                                    int Hp, int K, int soff, int nblk, pm_blockvals bv, int moff,
                                                                    int S, int A, int32_t *__restrict__ act_idx,
                                                                    double *__restrict__ act_val) {
    const int64_t total = N * (int64_t)M;
    for (int64_t t = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * SMP_THREADS) {
        const int64_t n = t / M;
        const int k = idx[t];
        int32_t *ai = act_idx + t * A;
        double *av = act_val + t * A;
        int cnt = 0;
        if (k >= 0 && k < K) {
            if (k >= soff && k < soff + nblk * H) {
                const int c = (k - soff) / H;
                ai[0] = (k - soff) - c * H;
                av[0] = bv.v[c];
                cnt = 1;
            } else if (k >= moff && k < moff + S) {
                const double *ts = tab + (int64_t)(k - moff) * Hp;
                for (int j = 0; j < Hp; ++j) {
                    const double v = ts[j];
                    if (v != 0.0 && cnt < A) {
                        int c = cand[n * Hp + j];
                        c = c < 0 ? 0 : (c >= H ? H - 1 : c);
                        ai[cnt] = c;
                        av[cnt] = v;
                        ++cnt;
                    }
                }
            }
        }
        const double fill = (k >= 0 && k < K) ? 0.0 : NAN;
        for (int j = cnt; j < A; ++j) {
            ai[j] = -1;
            av[j] = fill;
        }
    }
}

// ---- GSC: z | s, y_n ~ N(kappa_s, Lambda_s^-1) of the drawn state alone ------------------------------------------------------
constexpr int SMP_GSC_MAX = 8;      // gamma <= 8, as the E-step

// In place: the lower Cholesky factor of the symmetric g x g matrix in the lower triangle of m.  False: not positive definite.
__device__ __forceinline__ bool smp_chol(double (*m)[SMP_GSC_MAX], int g) {
    for (int j = 0; j < g; ++j) {
        double d = m[j][j];
        for (int k = 0; k < j; ++k) d = fma(-m[j][k], m[j][k], d);
        if (!(d > 0.0)) return false;
        const double r = sqrt(d), ir = 1.0 / r;
        m[j][j] = r;
        for (int i = j + 1; i < g; ++i) {
            double v = m[i][j];
            for (int k = 0; k < j; ++k) v = fma(-m[i][k], m[j][k], v);
            m[i][j] = v * ir;
        }
    }
    return true;
}

// inv (lower triangle, symmetric) = (L L^T)^-1 = L^-T L^-1 for the lower factor L; t: scratch for L^-1.
__device__ __forceinline__ void smp_inv_from_chol(const double (*L)[SMP_GSC_MAX], double (*t)[SMP_GSC_MAX],
                                                  double (*inv)[SMP_GSC_MAX], int g) {
    for (int j = 0; j < g; ++j) {            // column j of L^-1 by forward substitution
        t[j][j] = 1.0 / L[j][j];
        for (int i = j + 1; i < g; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v = fma(L[i][k], t[k][j], v);
            t[i][j] = -v / L[i][i];
        }
    }
    for (int i = 0; i < g; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = i; k < g; ++k) v = fma(t[k][i], t[k][j], v);
            inv[i][j] = v;
        }
}

// One lane per (row, sample): the active list of the draw with the values z.  Null state: empty.  Singleton h: z = kappa_h +
// eps_0 sqrt(1 / lambda_h) from the per-latent tables (rows 2, 4, 5, 6 of `tables`: G_hh mu_h, 1 / (lambda_h s2), 1 / lambda_h,
// mu_h), as pm_recon_gsc_moments2_f64.  Multi-cause state with the candidates a_0 < ... < a_{g-1} (ascending position):
//   Lambda = G_aa / s2 + (Psi_aa)^-1,  kappa = mu_a + Lambda^-1 (scores_a - G_aa mu_a) / s2,  z = kappa + L eps_{0..g-1},
// L the lower Cholesky factor of Lambda^-1: three Cholesky factorisations of at most 8 x 8 in private memory, every sum in
// ascending index order.  A factorisation that meets a pivot <= 0 (or NaN) gives NaN values.
__global__ __launch_bounds__(SMP_THREADS) void sample_gsc_kernel(const int32_t *__restrict__ idx, const int32_t *__restrict__ cand,
                                                                 const uint16_t *__restrict__ masks,
                                                                 const double *__restrict__ scores, int64_t lds,
                                                                 const double *__restrict__ G, const double *__restrict__ psi,
                                                                 const double *__restrict__ tables, double s2,
                                                                 const double *__restrict__ E, int64_t lde, int64_t N, int M,
                                                                 int H, int Hp, int S, int gamma, int A,
                                                                 int32_t *__restrict__ act_idx, double *__restrict__ act_val) {
    const double *gm = tables + 2 * (int64_t)H, *kl = tables + 4 * (int64_t)H, *ilam = tables + 5 * (int64_t)H,
                 *mu = tables + 6 * (int64_t)H;
    const int64_t total = N * (int64_t)M;
    const double is2 = 1.0 / s2;
    for (int64_t t = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * SMP_THREADS) {
        const int64_t n = t / M;
        const int k = idx[t];
        int32_t *ai = act_idx + t * A;
        double *av = act_val + t * A;
        const double *eps = E + t * lde;
        const double *arow = scores + n * lds;
        int cnt = 0;
        bool ok = (k >= 0 && k <= H + S);
        if (ok && k >= 1 && k <= H) {
            const int h = k - 1;
            const double kap = (arow[h] - gm[h]) * kl[h] + mu[h];
            ai[0] = h;
            av[0] = fma(eps[0], sqrt(ilam[h]), kap);
            cnt = 1;
        } else if (ok && k > H) {
            const unsigned mk = masks[k - 1 - H];
            int a[SMP_GSC_MAX];
            int g = 0;
            for (int j = 0; j < Hp; ++j)
                if (((mk >> j) & 1u) && g < gamma && g < A) {
                    int c = cand[n * Hp + j];
                    a[g++] = c < 0 ? 0 : (c >= H ? H - 1 : c);
                }
            double P[SMP_GSC_MAX][SMP_GSC_MAX], Q[SMP_GSC_MAX][SMP_GSC_MAX], T[SMP_GSC_MAX][SMP_GSC_MAX];
            double rhs[SMP_GSC_MAX], kap[SMP_GSC_MAX];
            for (int i = 0; i < g; ++i)
                for (int j = 0; j <= i; ++j) P[i][j] = psi[(int64_t)a[i] * H + a[j]];
            bool pd = smp_chol(P, g);
            smp_inv_from_chol(P, T, Q, g);                                   // Q = Psi_aa^-1
            for (int i = 0; i < g; ++i) {
                double r = arow[a[i]];
                for (int j = 0; j < g; ++j) r = fma(-G[(int64_t)a[i] * H + a[j]], mu[a[j]], r);
                rhs[i] = r * is2;
                for (int j = 0; j <= i; ++j) Q[i][j] = fma(G[(int64_t)a[i] * H + a[j]], is2, Q[i][j]);      // Lambda
            }
            pd = smp_chol(Q, g) && pd;
            smp_inv_from_chol(Q, T, P, g);                                   // P = Lambda^-1 (lower triangle)
            for (int i = 0; i < g; ++i) {
                double v = mu[a[i]];
                for (int j = 0; j < g; ++j) v = fma(j <= i ? P[i][j] : P[j][i], rhs[j], v);
                kap[i] = v;
            }
            pd = smp_chol(P, g) && pd;                                       // P = L
            for (int i = 0; i < g; ++i) {
                double v = kap[i];
                for (int j = 0; j <= i; ++j) v = fma(P[i][j], eps[j], v);
                ai[i] = a[i];
                av[i] = pd ? v : NAN;
            }
            cnt = g;
        }
        const double fill = ok ? 0.0 : NAN;
        for (int j = cnt; j < A; ++j) {
            ai[j] = -1;
            av[j] = fill;
        }
    }
}

// One wavefront per (row, sample), lanes over d.
__global__ __launch_bounds__(SMP_THREADS) void sample_decode_lin_kernel(const int32_t *__restrict__ act_idx,
                                                                        const double *__restrict__ act_val, int A,
                                                                        const double *__restrict__ Wt, int64_t ldw,
                                                                        const double *__restrict__ mu, int64_t N, int M, int H,
                                                                        int D, double *__restrict__ out, int64_t ldn,
                                                                        int64_t ldm) {
    const int lane = threadIdx.x & 63;
    const int64_t total = N * (int64_t)M;
    const int64_t wave0 = (int64_t)blockIdx.x * (SMP_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (SMP_THREADS / 64);
    for (int64_t t = wave0; t < total; t += nwaves) {
        const int64_t n = t / M, m = t - n * M;
        int ai[SMP_MAX_ACTIVE];
        double av[SMP_MAX_ACTIVE];
#pragma unroll
        for (int j = 0; j < SMP_MAX_ACTIVE; ++j) {
            int i = (j < A) ? act_idx[t * A + j] : -1;
            ai[j] = i >= H ? H - 1 : i;
            av[j] = (j < A) ? act_val[t * A + j] : 0.0;
        }
        double *orow = out + n * ldn + m * ldm;
        for (int d = lane; d < D; d += 64) {
            double acc = mu ? mu[d] : 0.0;
#pragma unroll
            for (int j = 0; j < SMP_MAX_ACTIVE; ++j) {
                if (j < A) {                                   // uniform
                    if (ai[j] >= 0) acc = fma(av[j], Wt[(int64_t)ai[j] * ldw + d], acc);
                    else if (av[j] != av[j]) acc = av[j];
                }
            }
            orow[d] = acc;
        }
    }
}

// MCA / MMCA.  One wavefront per (row, sample), lanes over d (D <= 1024: the limit of recon_mca_kernel, whose powers these are).
__global__ __launch_bounds__(SMP_THREADS) void sample_decode_mca_kernel(const int32_t *__restrict__ idx,
                                                                        const int32_t *__restrict__ cand,
                                                                        const uint16_t *__restrict__ masks,
                                                                        const double *__restrict__ Wt,
                                                                        const double *__restrict__ Wrho, double inv_rho,
                                                                        int signed_w, int64_t N, int M, int H, int D, int Hp,
                                                                        int S, double *__restrict__ out, int64_t ldn,
                                                                        int64_t ldm) {
    __shared__ __attribute__((aligned(16))) double s_tab[PM_POWTAB_LEN];
    const int tid = threadIdx.x, lane = tid & 63;
    bool r21, r6;
    pm_mca_pow_setup(s_tab, inv_rho, signed_w, tid, blockDim.x, r21, r6);
    __syncthreads();
    const int64_t total = N * (int64_t)M;
    const int64_t wave0 = (int64_t)blockIdx.x * (SMP_THREADS / 64) + (tid >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (SMP_THREADS / 64);
    for (int64_t t = wave0; t < total; t += nwaves) {
        const int64_t n = t / M, m = t - n * M;
        const int k = idx[t];
        double *orow = out + n * ldn + m * ldm;
        if (k < 0 || k > H + S) {                                  // uniform: a NaN row
            for (int d = lane; d < D; d += 64) orow[d] = NAN;
        } else if (k == 0) {
            for (int d = lane; d < D; d += 64) orow[d] = 0.0;
        } else if (k <= H) {
            const double *src = Wt + (int64_t)(k - 1) * D;
            for (int d = lane; d < D; d += 64) orow[d] = src[d];
        } else {
            const unsigned mk = masks[k - 1 - H];
            int64_t coff[PM_MAX_HPRIME];
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j) {
                int c = (j < Hp) ? cand[n * Hp + j] : 0;
                c = c < 0 ? 0 : (c >= H ? H - 1 : c);
                coff[j] = (int64_t)c * D;
            }
            for (int d = lane; d < D; d += 64) {
                double T = 0.0;
#pragma unroll
                for (int j = 0; j < PM_MAX_HPRIME; ++j)
                    if ((mk >> j) & 1u) T += Wrho[coff[j] + d];   // uniform
                orow[d] = pm_mca_wbar(T, inv_rho, r21, r6, s_tab);
            }
        }
    }
}

unsigned smp_grid(int64_t items, int per_block, int64_t cap = SMP_MAX_BLOCKS) {
    int64_t nb = (items + per_block - 1) / per_block;
    if (nb > cap) nb = cap;
    return (unsigned)(nb < 1 ? 1 : nb);
}

}  // namespace

extern "C" int64_t pm_sample_states_max_cols(void) { return SMP_LDS_DOUBLES - 64; }

extern "C" int pm_sample_states_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset,
                                    double weight_floor, int64_t null_col, const double *U, int64_t ldu, int64_t N, int64_t K,
                                    int64_t M, int32_t *idx, void *stream) {
    if (N < 0 || K <= 0 || M <= 0 || ld < K || ldu < M || !(weight_floor >= 0.0) || null_col < -1 || null_col >= K)
        return PM_EINVAL;
    if (K > pm_sample_states_max_cols() || M > INT32_MAX / 2) return PM_ERANGE;
    if (!logpj || !U || !idx) return PM_EINVAL;
    if (N == 0) return PM_OK;
    const int seg = smp_seg(K);
    if ((int64_t)64 * seg > SMP_LDS_DOUBLES) return PM_ERANGE;
    int waves = SMP_LDS_DOUBLES / (64 * seg);
    if (waves > SMP_THREADS / 64) waves = SMP_THREADS / 64;
    const size_t lds = (size_t)waves * 64 * seg * sizeof(double);
    hipLaunchKernelGGL(sample_states_kernel, dim3(smp_grid(N, waves, SMP_ROW_BLOCKS)), dim3(64 * waves), lds, static_cast<hipStream_t>(stream),
                       logpj, ld, lse, a, col_offset, weight_floor, (int)null_col, U, ldu, N, (int)K, (int)M, seg, idx);
    return (int)hipGetLastError();
}

extern "C" int pm_sample_active_f64(const int32_t *idx, const int32_t *cand, const double *state_vals,
                                    const double *block_values_host, int64_t N, int64_t M, int64_t H, int64_t Hprime, int64_t K,
                                    int64_t single_off, int64_t nblocks, int64_t multi_off, int64_t S, int64_t A,
                                    int32_t *act_idx, double *act_val, void *stream) {
    if (N < 0 || M <= 0 || H <= 0 || K <= 0 || single_off < 0 || nblocks < 0 || multi_off < 0 || S < 0 || Hprime < 0 ||
        (S > 0 && Hprime == 0) || A < 1)
        return PM_EINVAL;
    if (Hprime > PM_MAX_HPRIME || A > SMP_MAX_ACTIVE || nblocks > PM_MAX_BLOCKVALS || K > INT32_MAX / 2 ||
        H > INT32_MAX / 16 || M > INT32_MAX / 2)
        return PM_ERANGE;
    if (single_off + nblocks * H > K || multi_off + S > K) return PM_EINVAL;
    if (!idx || !act_idx || !act_val || (nblocks > 0 && !block_values_host) || (S > 0 && (!cand || !state_vals)))
        return PM_EINVAL;
    if (N == 0) return PM_OK;
    pm_blockvals bv;
    for (int c = 0; c < PM_MAX_BLOCKVALS; ++c) bv.v[c] = c < nblocks ? block_values_host[c] : 0.0;
    hipLaunchKernelGGL(sample_active_kernel, dim3(smp_grid(N * M, SMP_THREADS, SMP_ROW_BLOCKS)), dim3(SMP_THREADS), 0,
                       static_cast<hipStream_t>(stream), idx, cand, state_vals, N, (int)M, (int)H, (int)Hprime, (int)K,
                       (int)single_off, (int)nblocks, bv, (int)multi_off, (int)S, (int)A, act_idx, act_val);
    return (int)hipGetLastError();
}

extern "C" int pm_sample_gsc_f64(const int32_t *idx, const int32_t *cand, const uint16_t *state_masks, const double *scores,
                                 int64_t lds, const double *G, const double *psi_sq, const double *tables, double s2,
                                 const double *E, int64_t lde, int64_t N, int64_t M, int64_t H, int64_t Hprime, int64_t S,
                                 int64_t gamma, int64_t A, int32_t *act_idx, double *act_val, void *stream) {
    if (N < 0 || M <= 0 || H <= 0 || Hprime <= 0 || S < 0 || gamma < 1 || A < 1 || A < gamma || lds < H || lde < gamma ||
        !(s2 > 0.0))
        return PM_EINVAL;
    if (gamma > SMP_GSC_MAX || A > SMP_MAX_ACTIVE || Hprime > PM_MAX_HPRIME || H > INT32_MAX / 16 || S > INT32_MAX / 2 ||
        M > INT32_MAX / 2)
        return PM_ERANGE;
    if (!idx || !scores || !tables || !E || !act_idx || !act_val || (S > 0 && (!cand || !state_masks || !G || !psi_sq)))
        return PM_EINVAL;
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(sample_gsc_kernel, dim3(smp_grid(N * M, SMP_THREADS, SMP_ROW_BLOCKS)), dim3(SMP_THREADS), 0,
                       static_cast<hipStream_t>(stream), idx, cand, state_masks, scores, lds, G, psi_sq, tables, s2, E, lde, N,
                       (int)M, (int)H, (int)Hprime, (int)S, (int)gamma, (int)A, act_idx, act_val);
    return (int)hipGetLastError();
}

extern "C" int pm_sample_decode_lin_f64(const int32_t *act_idx, const double *act_val, int64_t A, const double *Wt, int64_t ldw,
                                        const double *mu, int64_t N, int64_t M, int64_t H, int64_t D, double *out,
                                        int64_t ld_row, int64_t ld_sample, void *stream) {
    if (N < 0 || M <= 0 || H <= 0 || D <= 0 || A < 1 || ldw < D || ld_row < D || ld_sample < D) return PM_EINVAL;
    if (A > SMP_MAX_ACTIVE || H > INT32_MAX / 2 || D > INT32_MAX / 2 || M > INT32_MAX / 2) return PM_ERANGE;
    if (!act_idx || !act_val || !Wt || !out) return PM_EINVAL;
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(sample_decode_lin_kernel, dim3(smp_grid(N * M, SMP_THREADS / 64)), dim3(SMP_THREADS), 0,
                       static_cast<hipStream_t>(stream), act_idx, act_val, (int)A, Wt, ldw, mu, N, (int)M, (int)H, (int)D, out,
                       ld_row, ld_sample);
    return (int)hipGetLastError();
}

extern "C" int pm_sample_decode_mca_f64(const int32_t *idx, const int32_t *cand, const uint16_t *state_masks, const double *Wt,
                                        const double *Wrho, double inv_rho, int signed_w, int64_t N, int64_t M, int64_t H,
                                        int64_t D, int64_t Hprime, int64_t S, double *out, int64_t ld_row, int64_t ld_sample,
                                        void *stream) {
    if (N < 0 || M <= 0 || H <= 0 || D <= 0 || Hprime <= 0 || S < 0 || ld_row < D || ld_sample < D || !(inv_rho > 0.0))
        return PM_EINVAL;
    if (D > 1024 || Hprime > PM_MAX_HPRIME || H > INT32_MAX / 2048 || S > INT32_MAX / 2 || M > INT32_MAX / 2) return PM_ERANGE;
    if (!idx || !Wt || !out || (S > 0 && (!cand || !state_masks || !Wrho))) return PM_EINVAL;
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(sample_decode_mca_kernel, dim3(smp_grid(N * M, SMP_THREADS / 64)), dim3(SMP_THREADS), 0,
                       static_cast<hipStream_t>(stream), idx, cand, state_masks, Wt, Wrho, inv_rho, signed_w, N, (int)M, (int)H,
                       (int)D, (int)Hprime, (int)S, out, ld_row, ld_sample);
    return (int)hipGetLastError();
}

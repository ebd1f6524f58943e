// What the exact-enumeration units share: loglik_exact.hip sums exp l_n(s) over every latent state s,
// recon_exact.hip weights f(s) by exp(l_n(s) - v_n) over the same states, infer_exact.hip ranks them by l_n(s).  The log-joint
// l_n(s) and everything it is built
// from -- the online log-sum-exp, the bounds, the state space and its split into digits, the prep product, MCA's Wbar(s), GSC's staging and
// per-support factorisation -- are defined ONCE, here; so is the walk of one datapoint's states that recon_exact.hip and
// infer_exact.hip both make (the linear kernels' lo states, chunk terms and odometer; MCA's prior and wavefront energy; the
// ranges; the block's log-sum-exp tree).  The units keep their own tile shapes, partial layouts and merges.  Every device
// routine is inlined into its callers.
#ifndef PM_EXACT_H
#define PM_EXACT_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pm_common.h"

constexpr int PMX_THREADS = 256;              // every enumeration kernel
constexpr uint64_t PMX_MAX_STATES = 1ull << 32;
constexpr int PMX_LIN_MAX_K = 8;              // values per latent of the linear models (3 bits of a packed digit)
constexpr int PMX_LIN_MAX_J = 4;              // lo states per thread (CH <= 1024)
constexpr int PMX_MAX_H = 32;
constexpr int PMX_GSC_MAX_H = 16;
constexpr int PMX_GSC_TN = 64;                // GSC: one lane per datapoint of the tile
constexpr int PMX_GS = PMX_GSC_MAX_H;             // row stride of GSC's LDS matrices

// ---- log-sum-exp ------------------------------------------------------------------------------------------------------------
// The online step.  A -inf term (a state of zero prior) changes nothing and never meets another -inf in a difference; a NaN
// term makes the sum NaN.
__device__ __forceinline__ void pmx_lse_add(double &m, double &s, double z) {
    if (z == -INFINITY) return;
    const double d = z - m;                    // +inf while m is still -inf
    const double e = exp(-fabs(d));
    if (d > 0.0) {
        s = s * e + 1.0;
        m = z;
    } else {
        s += e;                                // NaN d: s becomes NaN
    }
}

// (m, s) += (m2, s2)
__device__ __forceinline__ void pmx_lse_merge(double &m, double &s, double m2, double s2) {
    if (s2 != s2) {
        s = s2;
        return;
    }
    if (m2 == -INFINITY) return;
    if (m2 > m) {
        s = s * exp(m - m2) + s2;
        m = m2;
    } else {
        s += s2 * exp(m2 - m);
    }
}

__device__ __forceinline__ double pmx_lse_value(double m, double s) {
    return (s != s) ? (double)NAN : (m == -INFINITY ? -INFINITY : m + log(s));
}

// ---- the state space --------------------------------------------------------------------------------------------------------
// K^H, or 0 past the bound
static uint64_t pmx_state_count(int64_t K, int64_t H) {
    uint64_t c = 1;
    for (int64_t h = 0; h < H; ++h) {
        c *= (uint64_t)K;
        if (c > PMX_MAX_STATES) return 0;
    }
    return c;
}

// The linear models' state index is sum_h k_h K^h.  Its L low digits (lo, CH = K^L states, up to PMX_LIN_MAX_J per thread) are
// fixed per thread; a workgroup walks chunks: values of the H - L high digits (hi).
static void pmx_lin_split(int64_t K, int64_t H, int &L, int &CH) {
    L = 0;
    CH = 1;
    while (L < H && CH * K <= PMX_LIN_MAX_J * PMX_THREADS) {
        CH *= (int)K;
        ++L;
    }
}

// ---- the prep product -------------------------------------------------------------------------------------------------------
// B[n, h] = sum_d (y_nd - ymu_d) P[d, h] (ymu NULL: 0), y the row of datapoint n, in ascending d
__device__ __forceinline__ double pmx_prep_dot(const double *y, const double *ymu, int64_t D, const double *P, int64_t H,
                                               int64_t h) {
    double acc = 0.0;
    for (int64_t d = 0; d < D; ++d) acc = fma(y[d] - (ymu ? ymu[d] : 0.0), P[d * H + h], acc);
    return acc;
}

// ... as a kernel, one thread per output of B (N x H): recon_exact.hip and infer_exact.hip launch it per row block
static __global__ void __launch_bounds__(PMX_THREADS) pmx_prep_kernel(const double *__restrict__ Y, int64_t ldy,
                                                                      const double *__restrict__ ymu, int64_t N, int64_t D,
                                                                      const double *__restrict__ P, int64_t H,
                                                                      double *__restrict__ B) {
    const int64_t i = (int64_t)blockIdx.x * PMX_THREADS + threadIdx.x;
    if (i >= N * H) return;
    const int64_t n = i / H, h = i % H;
    const double *y = Y + n * ldy;
    B[i] = pmx_prep_dot(y, ymu, D, P, H, h);
}

// The linear models' log-joint, for both units' kernels: log p(s, y_n) = sum_h logp[h, k_h] - 1/2 s^T G s + s^T B_n + (row
// constant), s_h = values[k_h], G = W^T W / sigma^2, B_n = W^T y_n / sigma^2.  With s = s_lo + s_hi:
//   l(s) = [prior_lo - 1/2 s_lo^T G_ll s_lo]          (per lo, once per workgroup, in registers: plo)
//        + [prior_hi - 1/2 s_hi^T G_hh s_hi]          (per chunk, shared: the sum of sHv)
//        - s_lo^T (G_lh s_hi)                          (per chunk a table sGv[h][k] = -values[k] (G_lh s_hi)_h, L lookups)
//   s^T B_n = s_lo^T B_n,lo (per lo and datapoint, registers: blo) + s_hi^T B_n,hi (per chunk and datapoint, shared: sBh)
// so a (state, datapoint) costs two adds and one exp.
//
// The walk of ONE datapoint's states by one workgroup -- what rx_lin_kernel<SWEEP> (recon_exact.hip) and ix_lin_kernel
// (infer_exact.hip) share: lo-state setup, per-chunk terms, digit odometer -- is the set of routines below over the kernel's
// own LDS arrays, named by a PmxLin.  ex_lin_kernel<TN> (loglik_exact.hip) walks TN datapoints at once and holds its own
// statement of the same terms, as ex_mca_kernel does of the one-line prior term.
struct PmxLin {
    double *G, *logp, *val, *B;   // H x H, H x K, K, H: the operands and the datapoint's row of B
    double *Gv;                   // PMX_MAX_H x PMX_LIN_MAX_K: -values[k] (G_lh s_hi)_h of the chunk
    double *Hv, *Sv;              // PMX_MAX_H each: prior_hi - 1/2 s_i (G_hh s_hi)_i and s_i per hi latent of the chunk
    double *Bh;                   // 1: s_hi^T B_n,hi of the chunk
    int *dig;                     // PMX_MAX_H: the chunk's hi digits
    int H, K, L, CH, NH;
};

// the operands into LDS; the caller syncs
__device__ __forceinline__ void pmx_lin_stage(const PmxLin &w, const double *G, const double *logp, const double *values,
                                              const double *Brow) {
    for (int i = threadIdx.x; i < w.H * w.H; i += PMX_THREADS) w.G[i] = G[i];
    for (int i = threadIdx.x; i < w.H * w.K; i += PMX_THREADS) w.logp[i] = logp[i];
    if ((int)threadIdx.x < w.K) w.val[threadIdx.x] = values[threadIdx.x];
    if ((int)threadIdx.x < w.H) w.B[threadIdx.x] = Brow[threadIdx.x];
}

// the hi digits of chunk c (thread 0); the caller syncs
__device__ __forceinline__ void pmx_lin_seek(const PmxLin &w, uint64_t c) {
    if (threadIdx.x == 0) {
        for (int i = 0; i < w.NH; ++i) {
            w.dig[i] = (int)(c % (uint64_t)w.K);
            c /= (uint64_t)w.K;
        }
    }
}

// odometer: the next chunk's hi digits (thread 0); the caller syncs
__device__ __forceinline__ void pmx_lin_next_chunk(const PmxLin &w) {
    if (threadIdx.x == 0) {
        for (int i = 0; i < w.NH; ++i) {
            if (++w.dig[i] < w.K) break;
            w.dig[i] = 0;
        }
    }
}

// the lo state `lo` of a thread: its packed digits (3 bits each), prior_lo - 1/2 s_lo^T G_ll s_lo and s_lo^T B_n,lo; a lo state
// past CH gets (0, -inf, 0)
__device__ __forceinline__ void pmx_lin_lo_state(const PmxLin &w, int lo, uint32_t &code, double &plo, double &blo) {
    const int H = w.H, K = w.K, L = w.L;
    code = 0;
    plo = -INFINITY;
    blo = 0.0;
    if (lo >= w.CH) return;
    int x = lo;
    double pr = 0.0, quad = 0.0, bl = 0.0;
    for (int h = 0; h < L; ++h) {
        const int k = x % K;
        x /= K;
        code |= (uint32_t)k << (3 * h);
        pr += w.logp[h * K + k];
    }
    for (int h = 0; h < L; ++h) {
        const double sh = w.val[(code >> (3 * h)) & 7];
        if (sh == 0.0) continue;
        double gs = 0.0;
        for (int l = 0; l < L; ++l) gs = fma(w.G[h * H + l], w.val[(code >> (3 * l)) & 7], gs);
        quad = fma(sh, gs, quad);
        bl = fma(sh, w.B[h], bl);
    }
    plo = pr - 0.5 * quad;
    blo = bl;
}

// the shared per-chunk terms from the hi digits, by the threads 0 .. PMX_MAX_H; the caller syncs
__device__ __forceinline__ void pmx_lin_chunk_terms(const PmxLin &w) {
    const int H = w.H, K = w.K, L = w.L, NH = w.NH;
    const int t = threadIdx.x;
    if (t < L) {                                        // g_t = (G_lh s_hi)_t, times every value
        double g = 0.0;
        for (int i = 0; i < NH; ++i) g = fma(w.G[t * H + L + i], w.val[w.dig[i]], g);
        for (int k = 0; k < K; ++k) w.Gv[t * K + k] = -w.val[k] * g;
    } else if (t < H) {                                 // hi latent i: prior - 1/2 s_i (G_hh s_hi)_i
        const int i = t - L;
        const double si = w.val[w.dig[i]];
        double g = 0.0;
        if (si != 0.0)
            for (int l = 0; l < NH; ++l) g = fma(w.G[t * H + L + l], w.val[w.dig[l]], g);
        w.Hv[i] = w.logp[t * K + w.dig[i]] - 0.5 * si * g;
        w.Sv[i] = si;
    } else if (t == PMX_MAX_H) {                         // s_hi^T B_n,hi
        double b = 0.0;
        for (int l = 0; l < NH; ++l) b = fma(w.val[w.dig[l]], w.B[L + l], b);
        w.Bh[0] = b;
    }
}

// prior_hi - 1/2 s_hi^T G_hh s_hi of the chunk, after pmx_lin_chunk_terms and the sync
__device__ __forceinline__ double pmx_lin_chunk_prior(const PmxLin &w) {
    double lhi = 0.0;
    for (int i = 0; i < w.NH; ++i) lhi += w.Hv[i];
    return lhi;
}

// l_n(s) of the state (lo state of `code`, plo, blo; the current chunk, lhi = pmx_lin_chunk_prior, bh = Bh[0])
__device__ __forceinline__ double pmx_lin_logjoint(const PmxLin &w, uint32_t code, double plo, double blo, double lhi,
                                                   double bh) {
    double cross = 0.0;
    for (int h = 0; h < w.L; ++h) cross += w.Gv[h * w.K + ((code >> (3 * h)) & 7)];
    return ((plo + lhi) + cross) + (blo + bh);
}

// ---- what recon_exact.hip and infer_exact.hip share beyond l_n(s) -----------------------------------------------------------
constexpr int PMX_WAVES = PMX_THREADS / 64;

// ranges of a space of `units`, at least `per` units each, at most `cap`: a function of the state count alone
static int64_t pmx_ranges(uint64_t units, uint64_t per, int64_t cap) {
    uint64_t r = units / per;
    if (r < 1) r = 1;
    return r > (uint64_t)cap ? cap : (int64_t)r;
}

// The 256 threads' (max, sum exp) pairs merged in a fixed order: lane l takes lane l + o for o = 32, 16, ..., 1, then the
// wavefronts 1, 2, 3 are merged into 0 in order.  Every thread calls it; thread 0 holds the result.  `red`: 2 PMX_WAVES doubles.
__device__ __forceinline__ void pmx_block_lse(double &m, double &s, double *red) {
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_down(m, o), s2 = __shfl_down(s, o);
        if ((int)(threadIdx.x & 63) < o) pmx_lse_merge(m, s, m2, s2);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[2 * (threadIdx.x >> 6)] = m;
        red[2 * (threadIdx.x >> 6) + 1] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < PMX_WAVES; ++w) pmx_lse_merge(m, s, red[2 * w], red[2 * w + 1]);
}

// ---- MCA / MMCA ---------------------------------------------------------------------------------------------------------------
// log p(s, y_n) = |s| lp1 + (H - |s|) lp0 + inv_s2 sum_d (y_nd Wbar_d(s) - 1/2 Wbar_d(s)^2) + (row constant), Wbar_d(s) =
// (sum_{h in s} Wrho[h,d])^(1/rho) (signed: sign(t) |t|^(1/rho)), Wbar(0) = 0; the state index is the bit mask of s.

// Wbar_d(s) of the state with the bit mask st != 0, the causes added in ascending h, libm's pow
__device__ __forceinline__ double pmx_mca_wbar(const double *Wrho, int64_t D, int64_t d, uint64_t st,
                                               double inv_rho, int signed_w) {
    double t = 0.0;
    for (uint64_t b = st; b; b &= b - 1) t += Wrho[(int64_t)__builtin_ctzll(b) * D + d];
    return signed_w ? copysign(pow(fabs(t), inv_rho), t) : pow(t, inv_rho);
}

// One wavefront per state with its lanes over the dimensions d = lane + 64 i (rx_mca_kernel, ix_mca_kernel): D <= 1024.
constexpr int PMX_MCA_MAX_D = 1024;
constexpr int PMX_MCA_SLABS = PMX_MCA_MAX_D / 64;

// log prior of a state with k of H causes active (a zero count never meets an infinite log-probability)
__device__ __forceinline__ double pmx_mca_prior(int k, int H, double lp1, double lp0) {
    return (k ? k * lp1 : 0.0) + (H - k ? (H - k) * lp0 : 0.0);
}

// sum_d (y_d Wbar_d(st) - 1/2 Wbar_d(st)^2) by one wavefront: lane `lane` forms Wbar of its dimensions of the first nsl slabs
// into wv (0 past D and for st = 0; y holds the lane's entries of the row, 0 past D), a butterfly adds the lanes: every lane
// returns the same bits
__device__ __forceinline__ double pmx_mca_wave_energy(const double *Wrho, int64_t D, int nsl, uint64_t st, double inv_rho,
                                                      int signed_w, int lane, const double (&y)[PMX_MCA_SLABS],
                                                      double (&wv)[PMX_MCA_SLABS]) {
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < PMX_MCA_SLABS; ++i) {
        wv[i] = 0.0;
        if (i < nsl) {
            const int64_t d = lane + 64 * i;
            if (d < D && st) {
                wv[i] = pmx_mca_wbar(Wrho, D, d, st, inv_rho, signed_w);
            }
            e = fma(wv[i], y[i] - 0.5 * wv[i], e);
        }
    }
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    return e;
}

// ---- GSC ----------------------------------------------------------------------------------------------------------------------
// Given the support s (k latents), y ~ N(W_s mu_s, C_s), C_s = Sigma + W_s Psi_s W_s^T.  With Psi_s = Lp Lp^T,
// M = W^T Sigma^-1 W, K_s = I + Lp^T M_ss Lp = Lk Lk^T and A_s = Lk^-1 Lp^T (determinant lemma and Woodbury):
//   log det C_s = log det Sigma + 2 sum log diag Lk,   r^T C_s^-1 r = r^T Sigma^-1 r - |A_s beta|^2,
//   beta = W_s^T Sigma^-1 r = u_n,s - M_ss mu_s  (u_n = W^T Sigma^-1 y_n, the rows of B),
//   r^T Sigma^-1 r = q_n - 2 mu_s^T u_n,s + mu_s^T M_ss mu_s.
// So log p(s, y_n) = kappa_s + mu_s^T u_n,s + 1/2 |A_s (u_n,s - m_s)|^2 + (row constant), m_s = M_ss mu_s and
// kappa_s = log prior(s) - sum log diag Lk - 1/2 mu_s^T m_s.  A wavefront factors one support at a time in its own LDS
// (k <= 16), then every lane -- one datapoint of the tile -- applies it.

// M, Psi (row stride PMX_GS), mu, logp and the tile's rows of B (sU, row stride PMX_GS; 0 past N) into LDS; the caller syncs
__device__ __forceinline__ void pmx_gsc_stage(double *sM, double *sPsi, double *sMu, double *sLp, double *sU,
                                              const double *M, const double *Psi,
                                              const double *mu, const double *logp,
                                              const double *B, int64_t n0, int64_t N, int H) {
    for (int i = threadIdx.x; i < H * H; i += PMX_THREADS) {
        sM[(i / H) * PMX_GS + i % H] = M[i];
        sPsi[(i / H) * PMX_GS + i % H] = Psi[i];
    }
    if ((int)threadIdx.x < H) {
        sMu[threadIdx.x] = mu[threadIdx.x];
        sLp[2 * threadIdx.x] = logp[2 * threadIdx.x];
        sLp[2 * threadIdx.x + 1] = logp[2 * threadIdx.x + 1];
    }
    for (int i = threadIdx.x; i < PMX_GSC_TN * H; i += PMX_THREADS) {
        const int64_t n = n0 + i / H;
        sU[(i / H) * PMX_GS + i % H] = n < N ? B[n * H + i % H] : 0.0;
    }
}

// log prior of the support with the bit mask st
__device__ __forceinline__ double pmx_gsc_prior(const double *sLp, uint64_t st, int H) {
    double lp = 0.0;
    for (int h = 0; h < H; ++h) lp += sLp[2 * h + (int)((st >> h) & 1)];
    return lp;
}

// In-place lower Cholesky factor of the k x k matrix X (row stride PMX_GS) by one wavefront; the upper triangle is left alone.
static __device__ void pmx_wave_cholesky(double *X, int k, int lane) {
    for (int j = 0; j < k; ++j) {
        const double d = sqrt(X[j * PMX_GS + j]);
        pm_wave_sync();
        for (int i = j + 1 + lane; i < k; i += 64) X[i * PMX_GS + j] /= d;
        if (lane == 0) X[j * PMX_GS + j] = d;
        pm_wave_sync();
        const int n = k - j - 1;
        for (int e = lane; e < n * n; e += 64) {
            const int i = j + 1 + e / n, l = j + 1 + e % n;
            if (l <= i) X[i * PMX_GS + l] -= X[i * PMX_GS + j] * X[l * PMX_GS + j];
        }
        pm_wave_sync();
    }
}

// The factorisation of the support idx[0 .. k), k >= 1, by one wavefront in its own LDS (Lp, T, X: PMX_GS x PMX_GS each; mv: PMX_GS).
// Leaves A_s in T, m_s in mv, Lk in X, and returns kappa_s for the support's log prior lp.  Ends with the wavefront's sync.
__device__ __forceinline__ double pmx_gsc_factor_support(const double *sM, const double *sPsi, const double *sMu, const int *idx,
                                                     int k, int lane, double lp, double *Lp, double *T, double *X,
                                                     double *mv) {
    // Lp = chol(Psi_ss)
    for (int e = lane; e < k * k; e += 64) Lp[(e / k) * PMX_GS + e % k] = sPsi[idx[e / k] * PMX_GS + idx[e % k]];
    pm_wave_sync();
    pmx_wave_cholesky(Lp, k, lane);
    // T = M_ss Lp (Lp lower: rows p >= l)
    for (int e = lane; e < k * k; e += 64) {
        const int i = e / k, l = e % k;
        double t = 0.0;
        for (int p = l; p < k; ++p) t = fma(sM[idx[i] * PMX_GS + idx[p]], Lp[p * PMX_GS + l], t);
        T[i * PMX_GS + l] = t;
    }
    // m_s = M_ss mu_s
    if (lane < k) {
        double t = 0.0;
        for (int p = 0; p < k; ++p) t = fma(sM[idx[lane] * PMX_GS + idx[p]], sMu[idx[p]], t);
        mv[lane] = t;
    }
    pm_wave_sync();
    // X = I + Lp^T T (lower triangle)
    for (int e = lane; e < k * k; e += 64) {
        const int i = e / k, l = e % k;
        if (l > i) continue;
        double t = (i == l) ? 1.0 : 0.0;
        for (int p = i; p < k; ++p) t = fma(Lp[p * PMX_GS + i], T[p * PMX_GS + l], t);
        X[i * PMX_GS + l] = t;
    }
    pm_wave_sync();
    pmx_wave_cholesky(X, k, lane);
    // A = Lk^-1 Lp^T, column l by lane l (into T)
    if (lane < k) {
        const int l = lane;
        for (int i = 0; i < k; ++i) {
            double t = (i <= l) ? Lp[l * PMX_GS + i] : 0.0;
            for (int p = 0; p < i; ++p) t = fma(-X[i * PMX_GS + p], T[p * PMX_GS + l], t);
            T[i * PMX_GS + l] = t / X[i * PMX_GS + i];
        }
    }
    pm_wave_sync();
    double ld = 0.0, mm = 0.0;
    for (int i = 0; i < k; ++i) {
        ld += log(X[i * PMX_GS + i]);
        mm = fma(sMu[idx[i]], mv[i], mm);
    }
    return lp - ld - 0.5 * mm;
}

#endif  // PM_EXACT_H

// Exact held-out log-likelihood by enumerating every latent state: v_n = log sum_{all s} p(s, y_n | Theta)
// for the six component-analysis models, on the device, with no state table and no (N, states) buffer.
//
// Every entry runs the same three stages:
//   ex_prep     B = Y P (N x H, P the model's whitened weights) and q_n = y_n^T Q y_n, one thread per output, fixed order;
//   the model's enumeration kernel: the grid is (datapoint tile) x (state range); a workgroup enumerates its range, every
//               thread keeps a running (max, sum exp) per datapoint of the tile over the states it owns, and a fixed tree
//               merges the 256 threads' pairs into ONE partial per (range, datapoint);
//   ex_combine  per datapoint, the R partials merged in a fixed order, plus the row constant cst + qcoef q_n; then one
//               workgroup adds the rows in a fixed order.
// R (ranges per tile) depends on N and the state count alone (ex_plan; pm_loglik_exact_plan exports it), the ranges are fixed slices of the state index space, and
// nothing is added by atomics: the result is a function of the input bits (every run, both library builds).  States are decoded from their
// index; every per-state quantity is recomputed directly from its digits (no incremental updates), so the accuracy does
// not depend on how far a range reaches.  What recon_exact.hip must form the same way -- the log-sum-exp, the bounds, the state
// count and its L / CH split, MCA's Wbar_d(s), GSC's staging and per-support factorisation -- lives in pm_exact.h.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_exact.h"

namespace {

constexpr int EX_THREADS = PMX_THREADS;
constexpr int64_t EX_BLOCKS = 4096;          // 16 workgroups per CU on 256 CUs, split between tiles and ranges
constexpr int64_t EX_MAX_RANGES = 4096;
constexpr int EX_MCA_TN = 4;

int ex_lin_tn(int64_t N) { return N >= 64 ? 8 : 1; }
int ex_mca_tn(int64_t N) { return N >= 16 ? EX_MCA_TN : 1; }

int64_t ex_tiles(int64_t N, int tn) { return (N + tn - 1) / tn; }

// ranges per tile: enough workgroups to fill the chip, a function of N (and the tile width)
int64_t ex_ranges(int64_t N, int tn) {
    const int64_t t = ex_tiles(N, tn);
    if (t <= 0) return 1;
    int64_t r = (EX_BLOCKS + t - 1) / t;
    if (r > EX_MAX_RANGES) r = EX_MAX_RANGES;
    return r < 1 ? 1 : r;
}

// ... and no more ranges than `units` (a function of the state count: chunks, or states over a minimum per range)
int64_t ex_ranges_for(int64_t N, int tn, uint64_t units) {
    const int64_t r = ex_ranges(N, tn);
    if (units < 1) units = 1;
    return (uint64_t)r > units ? (int64_t)units : r;
}

constexpr uint64_t EX_MCA_MIN_STATES = 1024;   // states per range at least: 4 per thread
constexpr uint64_t EX_GSC_MIN_STATES = 32;     // supports per range at least: 8 per wavefront

int64_t ex_part_len(int64_t N) {
    int64_t m = ex_ranges(N, ex_lin_tn(N));
    const int64_t a = ex_ranges(N, ex_mca_tn(N)), b = ex_ranges(N, PMX_GSC_TN);
    if (a > m) m = a;
    if (b > m) m = b;
    return 2 * N * m;
}

// What a launch is made of, for the three kinds (PM_EXACT_LIN / _MCA / _GSC): the ONE place the entries below and
// pm_loglik_exact_plan take it from.  `space` is what the ranges cut (lin: chunks of CH lo states; MCA, GSC: states), `units`
// what caps their number (lin: chunks; MCA, GSC: states over the minimum per range, rounded up).
struct ExPlan {
    int tn, L, CH;
    uint64_t space, units;
    int64_t R, grid, part_off, part_len;
};

// PM_EINVAL / PM_ERANGE exactly as the entries document them for (N, D, K, H); K is read by the linear kind alone
int ex_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, ExPlan &p) {
    if (N < 0 || D < 1 || H < 1) return PM_EINVAL;
    p.L = 0;
    p.CH = 1;
    if (kind == PM_EXACT_LIN) {
        if (K < 2 || K > PMX_LIN_MAX_K) return PM_EINVAL;
        const uint64_t S = pmx_state_count(K, H);
        if (H > PMX_MAX_H || S == 0) return PM_ERANGE;
        p.tn = ex_lin_tn(N);
        pmx_lin_split(K, H, p.L, p.CH);
        p.space = p.units = S / (uint64_t)p.CH;
    } else if (kind == PM_EXACT_MCA) {
        if (H > PMX_MAX_H) return PM_ERANGE;
        p.tn = ex_mca_tn(N);
        p.space = 1ull << H;
        p.units = (p.space + EX_MCA_MIN_STATES - 1) / EX_MCA_MIN_STATES;
    } else if (kind == PM_EXACT_GSC) {
        if (H > PMX_GSC_MAX_H) return PM_ERANGE;
        p.tn = PMX_GSC_TN;
        p.space = 1ull << H;
        p.units = (p.space + EX_GSC_MIN_STATES - 1) / EX_GSC_MIN_STATES;
    } else {
        return PM_EINVAL;
    }
    p.R = ex_ranges_for(N, p.tn, p.units);
    p.grid = ex_tiles(N, p.tn) * p.R;
    p.part_off = N * (H + 2);
    p.part_len = 2 * N * p.R;
    return PM_OK;
}

// work layout (doubles): B (N x H) | q (N) | rows (N) | partials (2 N R, from the plan's part_off)
struct ExWork {
    double *B, *q, *rows, *part;
};

ExWork ex_work(double *work, int64_t N, int64_t H, const ExPlan &p) {
    ExWork w;
    w.B = work;
    w.q = work + N * H;
    w.rows = w.q + N;
    w.part = work + p.part_off;
    return w;
}

// With x_n = y_n - ymu (ymu NULL: 0): B[n,h] = sum_d x_nd P[d,h] (h < H); q[n] = sum_d wdiag_d x_nd^2 (wdiag NULL: 1), or
// |Lw x_n|^2 with Lw lower (D x D)
__global__ void __launch_bounds__(EX_THREADS) ex_prep_kernel(const double *__restrict__ Y, int64_t ldy,
                                                             const double *__restrict__ ymu, int64_t N, int64_t D,
                                                             const double *__restrict__ P, int64_t H,
                                                             const double *__restrict__ wdiag, const double *__restrict__ Lw,
                                                             double *__restrict__ B, double *__restrict__ q) {
    const int64_t i = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;
    const int64_t cols = (P ? H : 0) + 1;
    if (i >= N * cols) return;
    const int64_t n = i / cols, h = i % cols;
    const double *y = Y + n * ldy;
    double acc = 0.0;
    if (P && h < H) {
        B[n * H + h] = pmx_prep_dot(y, ymu, D, P, H, h);
        return;
    }
    if (Lw) {
        for (int64_t d = 0; d < D; ++d) {
            double z = 0.0;
            for (int64_t e = 0; e <= d; ++e) z = fma(Lw[d * D + e], y[e] - (ymu ? ymu[e] : 0.0), z);
            acc = fma(z, z, acc);
        }
    } else {
        for (int64_t d = 0; d < D; ++d) {
            const double x = y[d] - (ymu ? ymu[d] : 0.0);
            acc = fma((wdiag ? wdiag[d] : 1.0) * x, x, acc);
        }
    }
    q[n] = acc;
}

// rows[n] = (the R partials of datapoint n merged in a fixed order) + cst + qcoef q_n: one wavefront per row, lane l merges
// the ranges l, l + 64, ... in order, then lane 0 takes lane l + o for o = 32, 16, ..., 1
__global__ void __launch_bounds__(EX_THREADS) ex_combine_kernel(const double *__restrict__ part, int64_t N, int64_t R,
                                                                double cst, double qcoef, const double *__restrict__ q,
                                                                double *__restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * (EX_THREADS / 64) + (threadIdx.x >> 6);
    if (n >= N) return;                        // (wave-uniform)
    double m = -INFINITY, s = 0.0;
    for (int64_t r = lane; r < R; r += 64) pmx_lse_merge(m, s, part[2 * (r * N + n)], part[2 * (r * N + n) + 1]);
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_down(m, o), s2 = __shfl_down(s, o);
        if (lane < o) pmx_lse_merge(m, s, m2, s2);
    }
    if (lane == 0) {
        rows[n] = pmx_lse_value(m, s) + cst + qcoef * q[n];
    }
}

// total[0] = sum_n rows[n]: thread t adds rows t, t + 256, ... in order, then a fixed tree (0.0 for N == 0)
__global__ void __launch_bounds__(EX_THREADS) ex_total_kernel(const double *__restrict__ rows, int64_t N,
                                                              double *__restrict__ total) {
    __shared__ double red[EX_THREADS];
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += EX_THREADS) t += rows[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int o = EX_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = red[0];
}

// The 256 threads' (m, s) of each of the tile's TN datapoints, merged by a fixed tree (thread t takes t + o for o = 128,
// 64, ..., 1), written as the (range, datapoint) partial.  `red` holds 2 * TN * EX_THREADS doubles.
template <int TN>
__device__ void block_partials(const double (&m)[TN], const double (&s)[TN], double *red, int64_t n0, int64_t N,
                               int64_t r, double *__restrict__ part) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        red[(2 * i) * EX_THREADS + t] = m[i];
        red[(2 * i + 1) * EX_THREADS + t] = s[i];
    }
    __syncthreads();
    for (int o = EX_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int i = 0; i < TN; ++i) {
                double mm = red[(2 * i) * EX_THREADS + t], ss = red[(2 * i + 1) * EX_THREADS + t];
                pmx_lse_merge(mm, ss, red[(2 * i) * EX_THREADS + t + o], red[(2 * i + 1) * EX_THREADS + t + o]);
                red[(2 * i) * EX_THREADS + t] = mm;
                red[(2 * i + 1) * EX_THREADS + t] = ss;
            }
        }
        __syncthreads();
    }
    if (t < TN && n0 + t < N) {
        const int64_t n = n0 + t;
        part[2 * (r * N + n)] = red[(2 * t) * EX_THREADS];
        part[2 * (r * N + n) + 1] = red[(2 * t + 1) * EX_THREADS];
    }
}

// ---- linear models: BSC, TSC, DSC ----------------------------------------------------------------------------------------
// l(s) in the decomposition pm_exact.h describes (lo digits per thread, chunks of hi digits); a workgroup walks the chunks
// of its range for the TN datapoints of its tile.
struct LinArgs {
    const double *G;        // H x H
    const double *logp;     // H x K
    const double *values;   // K
    const double *B;        // N x H
    double *part;
    int64_t N, R;
    uint64_t nchunks;
    int H, K, L, CH;
};

template <int TN>
__global__ void __launch_bounds__(EX_THREADS) ex_lin_kernel(LinArgs a) {
    extern __shared__ double lds[];
    const int H = a.H, K = a.K, L = a.L, CH = a.CH, NH = H - L;
    double *sG = lds;                          // H*H
    double *sLogp = sG + H * H;                // H*K
    double *sVal = sLogp + H * K;              // 8
    double *sB = sVal + PMX_LIN_MAX_K;          // TN*H
    double *sGv = sB + TN * H;                 // L*K   - values[k] (G_lh s_hi)_h
    double *sHv = sGv + PMX_MAX_H * PMX_LIN_MAX_K;  // NH: prior_hi + (-1/2 s_i (G_hh s_hi)_i) per hi latent
    double *sBh = sHv + PMX_MAX_H;              // TN
    int *sDig = (int *)(sBh + TN);             // H-L hi digits of the current chunk
    double *red = sBh + TN + PMX_MAX_H;         // 2*TN*256 (block_partials), overlaps nothing used after the loop

    const int64_t R = a.R, tile = blockIdx.x / R, r = blockIdx.x % R, n0 = tile * TN;
    for (int i = threadIdx.x; i < H * H; i += EX_THREADS) sG[i] = a.G[i];
    for (int i = threadIdx.x; i < H * K; i += EX_THREADS) sLogp[i] = a.logp[i];
    if ((int)threadIdx.x < K) sVal[threadIdx.x] = a.values[threadIdx.x];
    for (int i = threadIdx.x; i < TN * H; i += EX_THREADS) {
        const int64_t n = n0 + i / H;
        sB[i] = n < a.N ? a.B[n * H + i % H] : 0.0;
    }
    const uint64_t c0 = a.nchunks * (uint64_t)r / (uint64_t)R, c1 = a.nchunks * (uint64_t)(r + 1) / (uint64_t)R;
    if (threadIdx.x == 0) {                    // the hi digits of chunk c0
        uint64_t c = c0;
        for (int i = 0; i < NH; ++i) {
            sDig[i] = (int)(c % (uint64_t)K);
            c /= (uint64_t)K;
        }
    }
    __syncthreads();

    // per lo state of this thread: its packed digits (3 bits each), prior_lo - 1/2 s_lo^T G_ll s_lo and s_lo^T B_n,lo
    uint32_t code[PMX_LIN_MAX_J];
    double plo[PMX_LIN_MAX_J], blo[PMX_LIN_MAX_J][TN];
#pragma unroll
    for (int j = 0; j < PMX_LIN_MAX_J; ++j) {
        const int lo = threadIdx.x + j * EX_THREADS;
        code[j] = 0;
        plo[j] = -INFINITY;
#pragma unroll
        for (int i = 0; i < TN; ++i) blo[j][i] = 0.0;
        if (lo >= CH) continue;
        int x = lo;
        double pr = 0.0, quad = 0.0;
        for (int h = 0; h < L; ++h) {
            const int k = x % K;
            x /= K;
            code[j] |= (uint32_t)k << (3 * h);
            pr += sLogp[h * K + k];
        }
        for (int h = 0; h < L; ++h) {
            const double sh = sVal[(code[j] >> (3 * h)) & 7];
            if (sh == 0.0) continue;
            double gs = 0.0;
            for (int l = 0; l < L; ++l) gs = fma(sG[h * H + l], sVal[(code[j] >> (3 * l)) & 7], gs);
            quad = fma(sh, gs, quad);
#pragma unroll
            for (int i = 0; i < TN; ++i) blo[j][i] = fma(sh, sB[i * H + h], blo[j][i]);
        }
        plo[j] = pr - 0.5 * quad;
    }

    double m[TN], s[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        m[i] = -INFINITY;
        s[i] = 0.0;
    }
    for (uint64_t c = c0; c < c1; ++c) {
        // shared per-chunk terms from the hi digits
        const int t = threadIdx.x;
        if (t < L) {                                        // g_t = (G_lh s_hi)_t, times every value
            double g = 0.0;
            for (int i = 0; i < NH; ++i) g = fma(sG[t * H + L + i], sVal[sDig[i]], g);
            for (int k = 0; k < K; ++k) sGv[t * K + k] = -sVal[k] * g;
        } else if (t < H) {                                 // hi latent i: prior - 1/2 s_i (G_hh s_hi)_i
            const int i = t - L;
            const double si = sVal[sDig[i]];
            double g = 0.0;
            if (si != 0.0)
                for (int l = 0; l < NH; ++l) g = fma(sG[t * H + L + l], sVal[sDig[l]], g);
            sHv[i] = sLogp[t * K + sDig[i]] - 0.5 * si * g;
        } else if (t >= PMX_MAX_H && t < PMX_MAX_H + TN) {  // s_hi^T B_n,hi
            const int i = t - PMX_MAX_H;
            double b = 0.0;
            for (int l = 0; l < NH; ++l) b = fma(sVal[sDig[l]], sB[i * H + L + l], b);
            sBh[i] = b;
        }
        __syncthreads();
        double lhi = 0.0;
        for (int i = 0; i < NH; ++i) lhi += sHv[i];
        double bh[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) bh[i] = sBh[i];
#pragma unroll
        for (int j = 0; j < PMX_LIN_MAX_J; ++j) {
            if (threadIdx.x + j * EX_THREADS >= (unsigned)CH) break;
            double cross = 0.0;
            for (int h = 0; h < L; ++h) cross += sGv[h * K + ((code[j] >> (3 * h)) & 7)];
            const double l = (plo[j] + lhi) + cross;
#pragma unroll
            for (int i = 0; i < TN; ++i) pmx_lse_add(m[i], s[i], l + (blo[j][i] + bh[i]));
        }
        if (threadIdx.x == 0) {                             // odometer: the next chunk's hi digits
            for (int i = 0; i < NH; ++i) {
                if (++sDig[i] < K) break;
                sDig[i] = 0;
            }
        }
        __syncthreads();
    }
    block_partials<TN>(m, s, red, n0, a.N, r, a.part);
}

// ---- MCA / MMCA ----------------------------------------------------------------------------------------------------------
// log p(s, y_n) = |s| lp1 + (H - |s|) lp0 + inv_s2 (y_n^T Wbar(s) - 1/2 |Wbar(s)|^2) + (row constant), Wbar_d(s) from
// pmx_mca_wbar (pm_exact.h); the state index is the bit mask of s.
// Every thread owns the states r0 + t, r0 + t + 256, ... of the workgroup's range and forms Wbar(s) one dimension at a time.
struct McaArgs {
    const double *Y;
    int64_t ldy;
    const double *Wrho;     // H x D
    double *part;
    int64_t N, R, D;
    uint64_t nstates;
    double inv_rho, lp1, lp0, inv_s2;
    int H, signed_w;
};

template <int TN>
__global__ void __launch_bounds__(EX_THREADS) ex_mca_kernel(McaArgs a) {
    __shared__ double red[2 * TN * EX_THREADS];
    const int64_t R = a.R, tile = blockIdx.x / R, r = blockIdx.x % R, n0 = tile * TN;
    const uint64_t s0 = a.nstates * (uint64_t)r / (uint64_t)R, s1 = a.nstates * (uint64_t)(r + 1) / (uint64_t)R;
    const double *yrow[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) yrow[i] = a.Y + (n0 + i < a.N ? n0 + i : n0) * a.ldy;
    double m[TN], s[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        m[i] = -INFINITY;
        s[i] = 0.0;
    }
    for (uint64_t st = s0 + threadIdx.x; st < s1; st += EX_THREADS) {
        const int k = __popcll(st);
        double lp = (k ? k * a.lp1 : 0.0) + (a.H - k ? (a.H - k) * a.lp0 : 0.0);
        if (lp == -INFINITY) continue;
        double nrm = 0.0, dot[TN];
#pragma unroll
        for (int i = 0; i < TN; ++i) dot[i] = 0.0;
        if (st) {
            for (int64_t d = 0; d < a.D; ++d) {
                const double w = pmx_mca_wbar(a.Wrho, a.D, d, st, a.inv_rho, a.signed_w);
                nrm = fma(w, w, nrm);
#pragma unroll
                for (int i = 0; i < TN; ++i) dot[i] = fma(yrow[i][d], w, dot[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) pmx_lse_add(m[i], s[i], lp + a.inv_s2 * (dot[i] - 0.5 * nrm));
    }
    block_partials<TN>(m, s, red, n0, a.N, r, a.part);
}

// ---- GSC -----------------------------------------------------------------------------------------------------------------
// l(s) = kappa_s + mu_s^T u_n,s + 1/2 |A_s (u_n,s - m_s)|^2 (pm_exact.h).  A wavefront factors one support at a time in its
// own LDS (k <= 16), then every lane -- one datapoint of the tile -- applies it.
struct GscArgs {
    const double *M, *Psi, *mu, *logp;   // H x H, H x H, H, H x 2 (log(1 - pi_h), log pi_h)
    const double *B;                     // N x H
    double *part;
    int64_t N, R;
    uint64_t nstates;
    int H;
};

__global__ void __launch_bounds__(EX_THREADS) ex_gsc_kernel(GscArgs a) {
    constexpr int WAVES = EX_THREADS / 64;
    __shared__ double sM[PMX_GS * PMX_GS], sPsi[PMX_GS * PMX_GS], sMu[PMX_GS], sLp[2 * PMX_GS];
    __shared__ double sU[PMX_GSC_TN * PMX_GS];
    __shared__ double sX[WAVES][3][PMX_GS * PMX_GS];     // Lp | T, then A | Lk
    __shared__ double sV[WAVES][PMX_GS];             // m_s
    __shared__ int sIdx[WAVES][PMX_GS];              // the support's latents, ascending
    __shared__ double red[2][WAVES][64];
    const int H = a.H, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t R = a.R, tile = blockIdx.x / R, r = blockIdx.x % R, n0 = tile * PMX_GSC_TN;
    pmx_gsc_stage(sM, sPsi, sMu, sLp, sU, a.M, a.Psi, a.mu, a.logp, a.B, n0, a.N, H);
    __syncthreads();
    const uint64_t s0 = a.nstates * (uint64_t)r / (uint64_t)R, s1 = a.nstates * (uint64_t)(r + 1) / (uint64_t)R;
    double *Lp = sX[w][0], *T = sX[w][1], *X = sX[w][2];
    double *mv = sV[w];
    const int *idx = sIdx[w];
    const double *u = sU + lane * PMX_GS;
    double m = -INFINITY, s = 0.0;
    for (uint64_t st = s0 + w; st < s1; st += WAVES) {
        const int k = __popcll(st);
        const double lp = pmx_gsc_prior(sLp, st, H);
        if (lp == -INFINITY) continue;
        if (lane < H && ((st >> lane) & 1)) sIdx[w][__popcll(st & ((1ull << lane) - 1))] = lane;
        pm_wave_sync();
        double kappa = lp, lin = 0.0, quad = 0.0;
        if (k) {
            kappa = pmx_gsc_factor_support(sM, sPsi, sMu, idx, k, lane, lp, Lp, T, X, mv);
            // per datapoint: beta = u_s - m_s, z = A beta
            double beta[PMX_GS];
#pragma unroll
            for (int i = 0; i < PMX_GS; ++i) {
                if (i < k) {
                    const double ui = u[idx[i]];
                    lin = fma(sMu[idx[i]], ui, lin);
                    beta[i] = ui - mv[i];
                }
            }
#pragma unroll
            for (int i = 0; i < PMX_GS; ++i) {
                if (i < k) {
                    double z = 0.0;
#pragma unroll
                    for (int l = 0; l < PMX_GS; ++l)
                        if (l < k) z = fma(T[i * PMX_GS + l], beta[l], z);
                    quad = fma(z, z, quad);
                }
            }
            pm_wave_sync();                          // (the next support overwrites this wave's LDS)
        }
        pmx_lse_add(m, s, kappa + lin + 0.5 * quad);
    }
    red[0][w][lane] = m;
    red[1][w][lane] = s;
    __syncthreads();
    if (w == 0 && n0 + lane < a.N) {
        double mm = -INFINITY, ss = 0.0;
        for (int v = 0; v < WAVES; ++v) pmx_lse_merge(mm, ss, red[0][v][lane], red[1][v][lane]);
        const int64_t n = n0 + lane;
        a.part[2 * (r * a.N + n)] = mm;
        a.part[2 * (r * a.N + n) + 1] = ss;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
int ex_prep(const double *Y, int64_t ldy, const double *ymu, int64_t N, int64_t D, const double *P, int64_t H,
            const double *wdiag, const double *Lw, const ExWork &w, hipStream_t st) {
    const int64_t cols = (P ? H : 0) + 1, tot = N * cols;
    hipLaunchKernelGGL(ex_prep_kernel, dim3((unsigned)((tot + EX_THREADS - 1) / EX_THREADS)), dim3(EX_THREADS), 0, st, Y,
                       ldy, ymu, N, D, P, H, wdiag, Lw, w.B, w.q);
    return (int)hipGetLastError();
}

int ex_finish(int64_t N, int64_t R, double cst, double qcoef, const ExWork &w, double *rows_out, double *total,
              hipStream_t st) {
    double *rows = rows_out ? rows_out : w.rows;
    if (N > 0) {
        const int64_t rows_per_block = EX_THREADS / 64;
        hipLaunchKernelGGL(ex_combine_kernel, dim3((unsigned)((N + rows_per_block - 1) / rows_per_block)), dim3(EX_THREADS),
                           0, st, w.part, N, R, cst, qcoef, w.q, rows);
        const int err = (int)hipGetLastError();
        if (err) return err;
    }
    hipLaunchKernelGGL(ex_total_kernel, dim3(1), dim3(EX_THREADS), 0, st, rows, N, total);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int64_t pm_loglik_exact_work_len(int64_t N, int64_t H) {
    if (N < 0 || H < 1) return -1;
    const int64_t len = N * (H + 2) + ex_part_len(N);
    return len > 0 ? len : 1;
}

extern "C" int pm_loglik_exact_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, int64_t *out) {
    if (!out) return PM_EINVAL;
    ExPlan p;
    const int rc = ex_plan(kind, N, D, K, H, p);
    if (rc) return rc;
    out[0] = p.tn;
    out[1] = p.L;
    out[2] = p.CH;
    out[3] = (int64_t)p.space;
    out[4] = (int64_t)p.units;
    out[5] = p.R;
    out[6] = p.grid;
    out[7] = p.part_off;
    out[8] = p.part_len;
    out[9] = 0;
    return PM_OK;
}

extern "C" int pm_loglik_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                                       const double *logp, const double *values, int64_t K, double cst, double qcoef,
                                       int64_t N, int64_t D, int64_t H, double *rows_out, double *work, double *total,
                                       void *stream) {
    if (N < 0 || D < 1 || H < 1 || K < 2 || K > PMX_LIN_MAX_K || ldy < D || !P || !G || !logp || !values || !work || !total ||
        (N > 0 && !Y))
        return PM_EINVAL;
    ExPlan pl;
    const int rc = ex_plan(PM_EXACT_LIN, N, D, K, H, pl);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ExWork w = ex_work(work, N, H, pl);
    const int tn = pl.tn;
    const int64_t R = pl.R;
    if (N > 0) {
        int err = ex_prep(Y, ldy, ymu, N, D, P, H, nullptr, nullptr, w, st);
        if (err) return err;
        LinArgs a;
        a.G = G;
        a.logp = logp;
        a.values = values;
        a.B = w.B;
        a.part = w.part;
        a.N = N;
        a.R = R;
        a.H = (int)H;
        a.K = (int)K;
        a.L = pl.L;
        a.CH = pl.CH;
        a.nchunks = pl.space;
        const size_t lds = sizeof(double) * ((size_t)H * H + H * K + PMX_LIN_MAX_K + (size_t)tn * H + PMX_MAX_H * PMX_LIN_MAX_K +
                                             PMX_MAX_H + tn + PMX_MAX_H + 2 * (size_t)tn * EX_THREADS);
        const dim3 grid((unsigned)pl.grid);
        if (tn == 8)
            hipLaunchKernelGGL(ex_lin_kernel<8>, grid, dim3(EX_THREADS), lds, st, a);
        else
            hipLaunchKernelGGL(ex_lin_kernel<1>, grid, dim3(EX_THREADS), lds, st, a);
        err = (int)hipGetLastError();
        if (err) return err;
    }
    return ex_finish(N, R, cst, qcoef, w, rows_out, total, st);
}

extern "C" int pm_loglik_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w,
                                       double lp1, double lp0, double inv_s2, double cst, int64_t N, int64_t D, int64_t H,
                                       double *rows_out, double *work, double *total, void *stream) {
    if (N < 0 || D < 1 || H < 1 || ldy < D || !Wrho || !work || !total || (N > 0 && !Y)) return PM_EINVAL;
    ExPlan pl;
    const int rc = ex_plan(PM_EXACT_MCA, N, D, 0, H, pl);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ExWork w = ex_work(work, N, H, pl);
    const int tn = pl.tn;
    const int64_t R = pl.R;
    if (N > 0) {
        int err = ex_prep(Y, ldy, nullptr, N, D, nullptr, H, nullptr, nullptr, w, st);
        if (err) return err;
        McaArgs a;
        a.Y = Y;
        a.ldy = ldy;
        a.Wrho = Wrho;
        a.part = w.part;
        a.N = N;
        a.R = R;
        a.D = D;
        a.nstates = pl.space;
        a.inv_rho = inv_rho;
        a.lp1 = lp1;
        a.lp0 = lp0;
        a.inv_s2 = inv_s2;
        a.H = (int)H;
        a.signed_w = signed_w ? 1 : 0;
        const dim3 grid((unsigned)pl.grid);
        if (tn == EX_MCA_TN)
            hipLaunchKernelGGL(ex_mca_kernel<EX_MCA_TN>, grid, dim3(EX_THREADS), 0, st, a);
        else
            hipLaunchKernelGGL(ex_mca_kernel<1>, grid, dim3(EX_THREADS), 0, st, a);
        err = (int)hipGetLastError();
        if (err) return err;
    }
    return ex_finish(N, R, cst, -0.5 * inv_s2, w, rows_out, total, st);
}

extern "C" int pm_loglik_exact_gsc_f64(const double *Y, int64_t ldy, const double *P, const double *wdiag, const double *Lw,
                                       const double *M, const double *Psi, const double *mu, const double *logp, double cst,
                                       int64_t N, int64_t D, int64_t H, double *rows_out, double *work, double *total,
                                       void *stream) {
    if (N < 0 || D < 1 || H < 1 || ldy < D || !P || !M || !Psi || !mu || !logp || !work || !total || (N > 0 && !Y) ||
        (wdiag && Lw))
        return PM_EINVAL;
    ExPlan pl;
    const int rc = ex_plan(PM_EXACT_GSC, N, D, 0, H, pl);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ExWork w = ex_work(work, N, H, pl);
    const int64_t R = pl.R;
    if (N > 0) {
        int err = ex_prep(Y, ldy, nullptr, N, D, P, H, wdiag, Lw, w, st);
        if (err) return err;
        GscArgs a;
        a.M = M;
        a.Psi = Psi;
        a.mu = mu;
        a.logp = logp;
        a.B = w.B;
        a.part = w.part;
        a.N = N;
        a.R = R;
        a.nstates = pl.space;
        a.H = (int)H;
        hipLaunchKernelGGL(ex_gsc_kernel, dim3((unsigned)pl.grid), dim3(EX_THREADS), 0, st, a);
        err = (int)hipGetLastError();
        if (err) return err;
    }
    return ex_finish(N, R, cst, -0.5, w, rows_out, total, st);
}

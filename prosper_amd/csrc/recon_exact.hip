// Exact posterior-mean reconstruction by enumerating every latent state: sum_{all s} q_n(s) f(s) with
// q_n(s) = exp(l_n(s) - v_n), l the log-joint of loglik_exact.hip without its row constants and
// v_n = log sum_{all s} exp l_n(s), for the six component-analysis models, with no state table and no (N, states) buffer.
//
// Every entry walks N in row blocks of a fixed size and runs, per block:
//   pmx_prep         B = (Y - ymu) P (rows x H), one thread per output, fixed order (linear models and GSC);
//   sweep 1          the model's enumeration kernel: a workgroup owns one (row or 64-row tile, state range), every thread
//                    keeps a running (max, sum exp) over the states it owns, a fixed tree merges them into ONE partial;
//   rx_combine_lse   v_n from the R partials of the row, merged in range order;
//   sweep 2          the same kernel (second instantiation) with the weights exp(l - v_n): per thread masses or sums, the
//                    same fixed tree, one partial vector per (range, row);
//   rx_combine_sum   the R partial vectors added in range order into the output row.
// R, the ranges themselves, the assignment of states to threads and every merge order are functions of the state count (and
// H, K, D) alone, never of N, and a workgroup handles its rows independently of one another: a row of the result is a
// function of that row of Y and of the parameters.  Nothing is added by atomics and nothing depends on PM_DETERMINISTIC.
// States are decoded from their index; every per-state quantity is recomputed from its digits.  The pieces of l_n(s) shared
// with loglik_exact.hip are the single definitions of pm_exact.h.
// pm_moments_exact_lin_f64 adds the second moments E[s s^T] of the linear models for exact EM: sweeps 1 and 2
// as above, then rx_lin_kernel<3>'s pair sweeps over coarser ranges of their own.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_exact.h"

namespace {

constexpr int RX_THREADS = PMX_THREADS;
constexpr int RX_WAVES = RX_THREADS / 64;
constexpr int RX_MCA_MAX_D = PMX_MCA_MAX_D;
constexpr int RX_MCA_SLABS = PMX_MCA_SLABS;
constexpr int64_t RX_ROWS = 256;              // rows per block of the host walk: linear models, GSC
constexpr int64_t RX_MAX_RANGES = 256;
constexpr int64_t RX_MCA_ROWS = 64;           // ... MCA / MMCA (a partial is D wide)
constexpr int64_t RX_MCA_MAX_RANGES = 64;
constexpr uint64_t RX_LIN_MIN_CHUNKS = 2;     // chunks per range at least (where there are two)
constexpr uint64_t RX_PAIR_MIN_CHUNKS = 16;   // ... of the moments entry's pair sweeps, whose epilogue is longer
constexpr uint64_t RX_MCA_MIN_STATES = 64;    // states per range at least: 16 per wavefront
constexpr uint64_t RX_GSC_MIN_STATES = 32;    // supports per range at least: 8 per wavefront

// The 256 threads' values added in a fixed order: lane l takes lane l + o for o = 32, 16, ..., 1, then the four wavefronts'
// sums as (0 + 1) + (2 + 3).  Every thread calls it; thread 0 holds the result.  `red`: RX_WAVES doubles.
__device__ double block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ... and their (max, sum exp) pairs: pmx_block_lse (pm_exact.h), the same lane tree.

// v[n] = log sum exp of the row's R partials part[2 (r nb + n)], merged in range order: one thread per row
__global__ void __launch_bounds__(RX_THREADS) rx_combine_lse_kernel(const double *__restrict__ part, int64_t nb, int64_t R,
                                                                    double *__restrict__ v) {
    const int64_t n = (int64_t)blockIdx.x * RX_THREADS + threadIdx.x;
    if (n >= nb) return;
    double m = -INFINITY, s = 0.0;
    for (int64_t r = 0; r < R; ++r) pmx_lse_merge(m, s, part[2 * (r * nb + n)], part[2 * (r * nb + n) + 1]);
    v[n] = pmx_lse_value(m, s);
}

// out[n, j] = sum_r part[(r nb + n) width + j] in range order: one thread per output
__global__ void __launch_bounds__(RX_THREADS) rx_combine_sum_kernel(const double *__restrict__ part, int64_t nb, int64_t R,
                                                                    int64_t width, double *__restrict__ out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * RX_THREADS + threadIdx.x;
    if (i >= nb * width) return;
    const int64_t n = i / width, j = i % width;
    double acc = 0.0;
    for (int64_t r = 0; r < R; ++r) acc += part[(r * nb + n) * width + j];
    out[n * ldo + j] = acc;
}

// ---- linear models: BSC, TSC, DSC ----------------------------------------------------------------------------------------
// l(s) in the decomposition pm_exact.h describes (lo digits per thread, chunks of hi digits); a workgroup walks the chunks
// of its range for ONE datapoint.  Sweep 2 keeps no accumulator per latent and state visit: a thread adds the weight of a
// state to the mass of its lo state (one add), the chunk's mass (one add per state) to the NH high-digit sums weighted by
// the chunk's own digit values (NH fmas per chunk, i.e. per up to four states), and turns the lo masses into the low
// latents' sums once, after the loop.  E[s]_h = sum over threads of these sums, by block_sum's fixed tree.
constexpr int LIN_MAX_NH = 24;            // high digits at most (K = 2, H = 32: 22)
constexpr int LIN_MAX_LL = 55;            // pairs of low digits at most: L <= 10 (K = 2, CH = 1024)
constexpr int LIN_OUT3 = LIN_MAX_LL;      // outputs of sweep 3 at most (a pinned sweep: H <= 32)
static_assert(PMX_MAX_H <= LIN_OUT3, "a pinned sweep's outputs fit");

struct LinArgs {
    const double *G;        // H x H
    const double *logp;     // H x K
    const double *values;   // K
    const double *B;        // nb x H
    const double *v;        // nb (sweep 2)
    double *part;
    int64_t nb, R;
    uint64_t nchunks;
    int H, K, L, CH;
    // sweep 3 (the moments entry): sweep 2 with every weight multiplied by the value of hi digit `pin`, over the
    // chunks where that value is not 0 -- or, pin = -1, sweep 2's loop with the lo-lo pair sums as its only outputs
    int pin = -1;
    uint64_t pdiv = 1;          // K^pin: digit `pin` of chunk c is (c / pdiv) % K
    int64_t width = 0;      // doubles per partial of sweep 3: H, or L (L + 1) / 2 for pin = -1
};

template <int SWEEP>
__global__ void __launch_bounds__(RX_THREADS) rx_lin_kernel(LinArgs a) {
    __shared__ double sG[PMX_MAX_H * PMX_MAX_H], sLogp[PMX_MAX_H * PMX_LIN_MAX_K], sVal[PMX_LIN_MAX_K], sB[PMX_MAX_H];
    __shared__ double sGv[PMX_MAX_H * PMX_LIN_MAX_K];   // -values[k] (G_lh s_hi)_h
    __shared__ double sHv[PMX_MAX_H];                   // prior_hi - 1/2 s_i (G_hh s_hi)_i per hi latent
    __shared__ double sSv[PMX_MAX_H];                   // s_i of the chunk's hi digits
    __shared__ double sBh[1];
    __shared__ int sDig[PMX_MAX_H];
    __shared__ double red[2 * RX_WAVES];
    __shared__ double sOut[SWEEP == 3 ? RX_WAVES * LIN_OUT3 : 1];   // sweep 3: the wavefronts' sums of every output
    const int H = a.H, K = a.K, L = a.L, CH = a.CH, NH = H - L;
    const int64_t R = a.R, n = blockIdx.x / R, r = blockIdx.x % R;
    const PmxLin w = {sG, sLogp, sVal, sB, sGv, sHv, sSv, sBh, sDig, H, K, L, CH, NH};
    pmx_lin_stage(w, a.G, a.logp, a.values, a.B + n * H);
    const uint64_t c0 = a.nchunks * (uint64_t)r / (uint64_t)R, c1 = a.nchunks * (uint64_t)(r + 1) / (uint64_t)R;
    if (SWEEP == 3 && a.pin >= 0) {
        // a range none of whose chunks carries weight (the pinned digit moves every pdiv chunks and shows every value within
        // K of its moves): zeros, before any setup
        bool any = false;
        uint64_t c = c0;
        for (int i = 0; i <= K && c < c1 && !any; ++i) {
            any = a.values[(c / a.pdiv) % (uint64_t)K] != 0.0;
            c = (c / a.pdiv + 1) * a.pdiv;
        }
        if (!any) {
            if ((int)threadIdx.x < H) a.part[(r * a.nb + n) * a.width + threadIdx.x] = 0.0;
            return;
        }
    }
    pmx_lin_seek(w, c0);                       // the hi digits of chunk c0
    __syncthreads();

    // per lo state of this thread: its packed digits (3 bits each), prior_lo - 1/2 s_lo^T G_ll s_lo and s_lo^T B_n,lo
    uint32_t code[PMX_LIN_MAX_J];
    double plo[PMX_LIN_MAX_J], blo[PMX_LIN_MAX_J];
#pragma unroll
    for (int j = 0; j < PMX_LIN_MAX_J; ++j) pmx_lin_lo_state(w, threadIdx.x + j * RX_THREADS, code[j], plo[j], blo[j]);

    const double vn = SWEEP >= 2 ? a.v[n] : 0.0;
    double m = -INFINITY, s = 0.0;             // sweep 1
    double mlo[PMX_LIN_MAX_J], ehi[LIN_MAX_NH];    // sweep 2
#pragma unroll
    for (int j = 0; j < PMX_LIN_MAX_J; ++j) mlo[j] = 0.0;
#pragma unroll
    for (int i = 0; i < LIN_MAX_NH; ++i) ehi[i] = 0.0;
    for (uint64_t c = c0; c < c1; ++c) {
        double wpin = 1.0;                                  // sweep 3: the pinned digit's value in this chunk (uniform)
        if (SWEEP == 3 && a.pin >= 0) {
            wpin = sVal[(int)((c / a.pdiv) % (uint64_t)K)];
            if (wpin == 0.0) {                              // no state of the chunk carries weight: on to the next one
                pmx_lin_next_chunk(w);
                __syncthreads();
                continue;
            }
        }
        pmx_lin_chunk_terms(w);                             // shared per-chunk terms from the hi digits
        __syncthreads();
        const double lhi = pmx_lin_chunk_prior(w);
        const double bh = sBh[0];
        double cm = 0.0;
#pragma unroll
        for (int j = 0; j < PMX_LIN_MAX_J; ++j) {
            if (threadIdx.x + j * RX_THREADS >= (unsigned)CH) break;
            const double l = pmx_lin_logjoint(w, code[j], plo[j], blo[j], lhi, bh);
            if (SWEEP == 1) {
                pmx_lse_add(m, s, l);
            } else {
                double q = exp(l - vn);                    // (-inf - v: 0, a state of zero prior)
                if (SWEEP == 3 && a.pin >= 0) q *= wpin;
                mlo[j] += q;
                cm += q;
            }
        }
        if (SWEEP >= 2) {
#pragma unroll
            for (int i = 0; i < LIN_MAX_NH; ++i)
                if (i < NH) ehi[i] = fma(sSv[i], cm, ehi[i]);
        }
        pmx_lin_next_chunk(w);                            // odometer: the next chunk's hi digits
        __syncthreads();
    }
    if (SWEEP == 1) {
        pmx_block_lse(m, s, red);
        if (threadIdx.x == 0) {
            a.part[2 * (r * a.nb + n)] = m;
            a.part[2 * (r * a.nb + n) + 1] = s;
        }
        return;
    }
    if (SWEEP == 3) {
        // Sweep 2's outputs (a pinned sweep) or, pin = -1, sum_s q(s) s_h s_h' of the low latents (h <= h') from the lo masses,
        // with ONE barrier for all of them: per output block_sum's lane tree, the wavefront's sum into sOut, then (0 + 1) +
        // (2 + 3).
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        double *mine = sOut + wv * LIN_OUT3;
        for (int h = 0; h < L && a.pin >= 0; ++h) {
            double e = 0.0;
#pragma unroll
            for (int j = 0; j < PMX_LIN_MAX_J; ++j)
                if (threadIdx.x + j * RX_THREADS < (unsigned)CH) e = fma(sVal[(code[j] >> (3 * h)) & 7], mlo[j], e);
            for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o);
            if (lane == 0) mine[h] = e;
        }
#pragma unroll
        for (int i = 0; i < LIN_MAX_NH; ++i) {
            if (i < NH && a.pin >= 0) {
                double e = ehi[i];
                for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o);
                if (lane == 0) mine[L + i] = e;
            }
        }
        if (a.pin < 0) {
            int t = 0;
            for (int h = 0; h < L; ++h) {
                for (int h2 = h; h2 < L; ++h2) {
                    double e = 0.0;
#pragma unroll
                    for (int j = 0; j < PMX_LIN_MAX_J; ++j)
                        if (threadIdx.x + j * RX_THREADS < (unsigned)CH)
                            e = fma(sVal[(code[j] >> (3 * h)) & 7] * sVal[(code[j] >> (3 * h2)) & 7], mlo[j], e);
                    for (int o = 32; o > 0; o >>= 1) e += __shfl_down(e, o);
                    if (lane == 0) mine[t] = e;
                    ++t;
                }
            }
        }
        __syncthreads();
        double *out3 = a.part + (r * a.nb + n) * a.width;
        for (int t = threadIdx.x; t < (int)a.width; t += RX_THREADS)
            out3[t] = (sOut[t] + sOut[LIN_OUT3 + t]) + (sOut[2 * LIN_OUT3 + t] + sOut[3 * LIN_OUT3 + t]);
        return;
    }
    double *out = a.part + (r * a.nb + n) * (int64_t)H;
    for (int h = 0; h < L; ++h) {                           // the low latents from the lo masses
        double e = 0.0;
#pragma unroll
        for (int j = 0; j < PMX_LIN_MAX_J; ++j)
            if (threadIdx.x + j * RX_THREADS < (unsigned)CH) e = fma(sVal[(code[j] >> (3 * h)) & 7], mlo[j], e);
        e = block_sum(e, red);
        if (threadIdx.x == 0) out[h] = e;
    }
#pragma unroll
    for (int i = 0; i < LIN_MAX_NH; ++i) {
        if (i < NH) {                                       // (uniform)
            const double e = block_sum(ehi[i], red);
            if (threadIdx.x == 0) out[L + i] = e;
        }
    }
}

// The partials of one launch of sweep 3 added in range order into the moments' outputs, one thread per (row, column).  The
// place of the pair (h, h'), h <= h', in a row of C is h H - h (h - 1) / 2 + h' - h.  pin = -1: the columns are the lo-lo pairs
// in that order; pin >= 0 (latent p = L + pin): column j is the pair (j, p) for j < L and (p, j) for j >= p -- every pair of
// C is written by exactly one launch.
__global__ void __launch_bounds__(RX_THREADS) rx_combine_moments_kernel(const double *__restrict__ part, int64_t nb, int64_t R,
                                                                        int64_t width, int H, int L, int pin,
                                                                        double *__restrict__ C, int64_t ldc) {
    const int64_t i = (int64_t)blockIdx.x * RX_THREADS + threadIdx.x;
    if (i >= nb * width) return;
    const int64_t n = i / width;
    const int j = (int)(i % width);
    double *dst;
    {
        int h, h2;
        if (pin < 0) {
            int t = j;
            h = 0;
            while (t >= L - h) {
                t -= L - h;
                ++h;
            }
            h2 = h + t;
        } else {
            const int p = L + pin;
            if (j >= L && j < p) return;
            h = j < L ? j : p;
            h2 = j < L ? p : j;
        }
        dst = C + n * ldc + ((int64_t)h * H - (int64_t)h * (h - 1) / 2 + (h2 - h));
    }
    double acc = 0.0;
    for (int64_t r = 0; r < R; ++r) acc += part[(r * nb + n) * width + j];
    *dst = acc;
}

// ---- MCA / MMCA ----------------------------------------------------------------------------------------------------------
// l(s) = |s| lp1 + (H - |s|) lp0 + inv_s2 sum_d (y_d Wbar_d(s) - 1/2 Wbar_d(s)^2), Wbar_d(s) from pmx_mca_wbar; the state
// index is the bit mask of s.  A workgroup owns one (datapoint, range); wavefront w takes the states s0 + w, s0 + w + 4, ...
// with its lanes over the dimensions d = lane + 64 i (i < 16: D <= 1024), forms Wbar_d(s) once per state and sweep, sums
// the energy over the lanes by a butterfly (every lane holds the same bits) and, in sweep 2, adds q Wbar_d to its own
// dimensions' accumulators: no cross-lane traffic for the output.  The four wavefronts' results merge in wavefront order.
struct McaArgs {
    const double *Y;
    int64_t ldy;
    const double *Wrho;     // H x D
    const double *v;
    double *part;
    int64_t nb, R, D;
    uint64_t nstates;
    double inv_rho, lp1, lp0, inv_s2;
    int H, signed_w;
};

template <int SWEEP>
__global__ void __launch_bounds__(RX_THREADS) rx_mca_kernel(McaArgs a) {
    __shared__ double sAcc[SWEEP == 2 ? RX_WAVES * RX_MCA_MAX_D : 1];
    __shared__ double red[2 * RX_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t R = a.R, n = blockIdx.x / R, r = blockIdx.x % R, D = a.D;
    const uint64_t s0 = a.nstates * (uint64_t)r / (uint64_t)R, s1 = a.nstates * (uint64_t)(r + 1) / (uint64_t)R;
    const int nsl = (int)((D + 63) / 64);
    double y[RX_MCA_SLABS], acc[RX_MCA_SLABS];
#pragma unroll
    for (int i = 0; i < RX_MCA_SLABS; ++i) {
        const int64_t d = lane + 64 * i;
        y[i] = d < D ? a.Y[n * a.ldy + d] : 0.0;
        acc[i] = 0.0;
    }
    const double vn = SWEEP == 2 ? a.v[n] : 0.0;
    double m = -INFINITY, s = 0.0;
    for (uint64_t st = s0 + w; st < s1; st += RX_WAVES) {   // (st is uniform over the wavefront)
        const int k = __popcll(st);
        const double lp = pmx_mca_prior(k, a.H, a.lp1, a.lp0);
        if (lp == -INFINITY) continue;
        double wv[RX_MCA_SLABS];
        const double e = pmx_mca_wave_energy(a.Wrho, D, nsl, st, a.inv_rho, a.signed_w, lane, y, wv);
        const double l = lp + a.inv_s2 * e;
        if (SWEEP == 1) {
            pmx_lse_add(m, s, l);
        } else {
            const double q = exp(l - vn);
#pragma unroll
            for (int i = 0; i < RX_MCA_SLABS; ++i)
                if (i < nsl) acc[i] = fma(q, wv[i], acc[i]);
        }
    }
    if (SWEEP == 1) {
        if (lane == 0) {
            red[2 * w] = m;
            red[2 * w + 1] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int u = 1; u < RX_WAVES; ++u) pmx_lse_merge(m, s, red[2 * u], red[2 * u + 1]);
            a.part[2 * (r * a.nb + n)] = m;
            a.part[2 * (r * a.nb + n) + 1] = s;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < RX_MCA_SLABS; ++i)
        if (i < nsl) sAcc[w * RX_MCA_MAX_D + lane + 64 * i] = acc[i];
    __syncthreads();
    double *out = a.part + (r * a.nb + n) * D;
    for (int64_t d = threadIdx.x; d < D; d += RX_THREADS)
        out[d] = (sAcc[d] + sAcc[RX_MCA_MAX_D + d]) + (sAcc[2 * RX_MCA_MAX_D + d] + sAcc[3 * RX_MCA_MAX_D + d]);
}

// ---- GSC -----------------------------------------------------------------------------------------------------------------
// l(s) = kappa_s + mu_s^T u_n,s + 1/2 |A_s beta_n,s|^2 with pmx_gsc_factor_support's per-support factorisation (pm_exact.h):
// a wavefront factors one support at a time in its own LDS, then every lane -- one datapoint of the 64-row tile -- applies
// it.  Sweep 2 keeps z = A_s beta and adds q (mu_h + (A_s^T z)_pos) to the accumulator of every latent h of the support
// (pos its rank in the support): 16 accumulators per lane, indexed statically.  The wavefronts 1, 2, 3 hand theirs to
// wavefront 0 through LDS (the factorisation's, free after the loop), which adds them in that order.
struct GscArgs {
    const double *M, *Psi, *mu, *logp;   // H x H, H x H, H, H x 2 (log(1 - pi_h), log pi_h)
    const double *B;                     // nb x H
    const double *v;
    double *part;
    int64_t nb, R;
    uint64_t nstates;
    int H;
};

template <int SWEEP>
__global__ void __launch_bounds__(RX_THREADS) rx_gsc_kernel(GscArgs a) {
    __shared__ double sM[PMX_GS * PMX_GS], sPsi[PMX_GS * PMX_GS], sMu[PMX_GS], sLp[2 * PMX_GS];
    __shared__ double sU[PMX_GSC_TN * PMX_GS];
    __shared__ double sX[RX_WAVES][3][PMX_GS * PMX_GS];  // Lp | T, then A | Lk; after the loop (RX_WAVES - 1) x PMX_GS x 64 accumulators
    __shared__ double sV[RX_WAVES][PMX_GS];          // m_s
    __shared__ int sIdx[RX_WAVES][PMX_GS];           // the support's latents, ascending
    __shared__ double red[2][RX_WAVES][64];
    static_assert((RX_WAVES - 1) * PMX_GS * 64 <= RX_WAVES * 3 * PMX_GS * PMX_GS, "the accumulators fit the factorisation's LDS");
    const int H = a.H, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t R = a.R, tile = blockIdx.x / R, r = blockIdx.x % R, n0 = tile * PMX_GSC_TN;
    pmx_gsc_stage(sM, sPsi, sMu, sLp, sU, a.M, a.Psi, a.mu, a.logp, a.B, n0, a.nb, H);
    __syncthreads();
    const uint64_t s0 = a.nstates * (uint64_t)r / (uint64_t)R, s1 = a.nstates * (uint64_t)(r + 1) / (uint64_t)R;
    double *Lp = sX[w][0], *T = sX[w][1], *X = sX[w][2];
    double *mv = sV[w];
    const int *idx = sIdx[w];
    const double *u = sU + lane * PMX_GS;
    const double vn = (SWEEP == 2 && n0 + lane < a.nb) ? a.v[n0 + lane] : 0.0;
    double m = -INFINITY, s = 0.0;
    double acc[PMX_GS];
#pragma unroll
    for (int i = 0; i < PMX_GS; ++i) acc[i] = 0.0;
    for (uint64_t st = s0 + w; st < s1; st += RX_WAVES) {
        const int k = __popcll(st);
        const double lp = pmx_gsc_prior(sLp, st, H);
        if (lp == -INFINITY) continue;
        if (lane < H && ((st >> lane) & 1)) sIdx[w][__popcll(st & ((1ull << lane) - 1))] = lane;
        pm_wave_sync();
        double kappa = lp, lin = 0.0, quad = 0.0;
        double z[PMX_GS];
#pragma unroll
        for (int i = 0; i < PMX_GS; ++i) z[i] = 0.0;
        if (k) {
            kappa = pmx_gsc_factor_support(sM, sPsi, sMu, idx, k, lane, lp, Lp, T, X, mv);
            // per datapoint: beta = u_s - m_s, z = A beta
            double beta[PMX_GS];
#pragma unroll
            for (int i = 0; i < PMX_GS; ++i) {
                beta[i] = 0.0;
                if (i < k) {
                    const double ui = u[idx[i]];
                    lin = fma(sMu[idx[i]], ui, lin);
                    beta[i] = ui - mv[i];
                }
            }
#pragma unroll
            for (int i = 0; i < PMX_GS; ++i) {
                if (i < k) {
                    double zi = 0.0;
#pragma unroll
                    for (int l = 0; l < PMX_GS; ++l)
                        if (l < k) zi = fma(T[i * PMX_GS + l], beta[l], zi);
                    quad = fma(zi, zi, quad);
                    z[i] = zi;
                }
            }
        }
        const double l = kappa + lin + 0.5 * quad;
        if (SWEEP == 1) {
            pmx_lse_add(m, s, l);
        } else if (k) {
            const double q = exp(l - vn);
            int pos = 0;                          // (uniform: the rank of latent h in the support)
#pragma unroll
            for (int h = 0; h < PMX_GS; ++h) {
                if ((st >> h) & 1) {
                    double kap = sMu[h];
#pragma unroll
                    for (int i = 0; i < PMX_GS; ++i)
                        if (i < k) kap = fma(T[i * PMX_GS + pos], z[i], kap);
                    acc[h] = fma(q, kap, acc[h]);
                    ++pos;
                }
            }
        }
        pm_wave_sync();                              // (the next support overwrites this wave's LDS)
    }
    if (SWEEP == 1) {
        red[0][w][lane] = m;
        red[1][w][lane] = s;
        __syncthreads();
        if (w == 0 && n0 + lane < a.nb) {
            double mm = -INFINITY, ss = 0.0;
            for (int v = 0; v < RX_WAVES; ++v) pmx_lse_merge(mm, ss, red[0][v][lane], red[1][v][lane]);
            const int64_t n = n0 + lane;
            a.part[2 * (r * a.nb + n)] = mm;
            a.part[2 * (r * a.nb + n) + 1] = ss;
        }
        return;
    }
    __syncthreads();                              // every wavefront has left its factorisation
    double *sR = &sX[0][0][0];
    if (w > 0) {
#pragma unroll
        for (int h = 0; h < PMX_GS; ++h) sR[((w - 1) * PMX_GS + h) * 64 + lane] = acc[h];
    }
    __syncthreads();
    if (w == 0 && n0 + lane < a.nb) {
        double *out = a.part + (r * a.nb + n0 + lane) * H;
#pragma unroll
        for (int h = 0; h < PMX_GS; ++h) {
            if (h < H) {
                double e = acc[h];
                for (int u2 = 0; u2 < RX_WAVES - 1; ++u2) e += sR[(u2 * PMX_GS + h) * 64 + lane];
                out[h] = e;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
inline unsigned rx_blocks(int64_t items) { return (unsigned)((items + RX_THREADS - 1) / RX_THREADS); }

int rx_combine_lse(const double *part, int64_t nb, int64_t R, double *v, hipStream_t st) {
    hipLaunchKernelGGL(rx_combine_lse_kernel, dim3(rx_blocks(nb)), dim3(RX_THREADS), 0, st, part, nb, R, v);
    return (int)hipGetLastError();
}

int rx_combine_sum(const double *part, int64_t nb, int64_t R, int64_t width, double *out, int64_t ldo, hipStream_t st) {
    hipLaunchKernelGGL(rx_combine_sum_kernel, dim3(rx_blocks(nb * width)), dim3(RX_THREADS), 0, st, part, nb, R, width, out,
                       ldo);
    return (int)hipGetLastError();
}

int64_t rx_min(int64_t a, int64_t b) { return a < b ? a : b; }
int64_t rx_max(int64_t a, int64_t b) { return a > b ? a : b; }

// What a call is made of, for the three kinds (PM_EXACT_LIN / _MCA / _GSC): the ONE place the entries below and
// pm_recon_exact_plan take it from.  `space` is what the ranges cut (lin: chunks of CH lo states; MCA, GSC: states); a block
// of nb rows keeps [B (nb x H; not MCA) | v (nb) | partials] in `work`, the partials 2 nb R doubles in sweep 1 and
// width nb R in sweep 2 (width: H; MCA: D).
struct RxPlan {
    int64_t rows, blocks, R, width;
    uint64_t space;
    int L, CH, slabs, has_b;
};

// PM_EINVAL / PM_ERANGE exactly as the entries document them for (N, D, K, H); K is read by the linear kind alone
int rx_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, RxPlan &p) {
    if (N < 0 || D < 1 || H < 1) return PM_EINVAL;
    p.L = 0;
    p.CH = 1;
    p.slabs = 0;
    p.has_b = 1;
    p.rows = RX_ROWS;
    p.width = H;
    if (kind == PM_EXACT_LIN) {
        if (K < 2 || K > PMX_LIN_MAX_K) return PM_EINVAL;
        const uint64_t S = pmx_state_count(K, H);
        if (H > PMX_MAX_H || S == 0) return PM_ERANGE;
        pmx_lin_split(K, H, p.L, p.CH);
        if (H - p.L > LIN_MAX_NH) return PM_ERANGE;
        p.space = S / (uint64_t)p.CH;
        p.R = pmx_ranges(p.space, RX_LIN_MIN_CHUNKS, RX_MAX_RANGES);
    } else if (kind == PM_EXACT_MCA) {
        if (H > PMX_MAX_H || D > RX_MCA_MAX_D) return PM_ERANGE;
        p.rows = RX_MCA_ROWS;
        p.width = D;
        p.has_b = 0;
        p.slabs = (int)((D + 63) / 64);
        p.space = 1ull << H;
        p.R = pmx_ranges(p.space, RX_MCA_MIN_STATES, RX_MCA_MAX_RANGES);
    } else if (kind == PM_EXACT_GSC) {
        if (H > PMX_GSC_MAX_H) return PM_ERANGE;
        p.space = 1ull << H;
        p.R = pmx_ranges(p.space, RX_GSC_MIN_STATES, RX_MAX_RANGES);
    } else {
        return PM_EINVAL;
    }
    p.blocks = (N + p.rows - 1) / p.rows;
    return PM_OK;
}

// the three parts of `work` for a block of nb rows
struct RxWork {
    double *B, *v, *part;
};

int64_t rx_part_off(int64_t nb, int64_t H, const RxPlan &p) { return (p.has_b ? nb * H : 0) + nb; }

RxWork rx_work(double *work, int64_t nb, int64_t H, const RxPlan &p) {
    RxWork w;
    w.B = work;
    w.part = work + rx_part_off(nb, H, p);
    w.v = w.part - nb;
    return w;
}

}  // namespace

extern "C" int64_t pm_recon_exact_work_len(int64_t N, int64_t H, int64_t D) {
    if (N < 0 || H < 1 || D < 1) return -1;
    const int64_t a = rx_min(N, RX_ROWS) * (H + 1 + RX_MAX_RANGES * rx_max(H, 2));
    const int64_t b = rx_min(N, RX_MCA_ROWS) * (1 + RX_MCA_MAX_RANGES * rx_max(D, 2));
    return rx_max(rx_max(a, b), 1);
}

extern "C" int pm_recon_exact_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, int64_t *out) {
    if (!out) return PM_EINVAL;
    RxPlan p;
    const int rc = rx_plan(kind, N, D, K, H, p);
    if (rc) return rc;
    const int64_t nb = rx_min(N, p.rows);
    out[0] = p.rows;
    out[1] = p.blocks;
    out[2] = p.L;
    out[3] = p.CH;
    out[4] = (int64_t)p.space;
    out[5] = p.R;
    out[6] = p.slabs;
    out[7] = rx_part_off(nb, H, p);
    out[8] = 2 * nb * p.R;
    out[9] = p.width * nb * p.R;
    return PM_OK;
}

extern "C" int pm_recon_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                                      const double *logp, const double *values, int64_t K, int64_t N, int64_t D, int64_t H,
                                      double *E, int64_t lde, double *work, void *stream) {
    if (N < 0 || D < 1 || H < 1 || K < 2 || K > PMX_LIN_MAX_K || ldy < D || lde < H || !P || !G || !logp || !values || !work ||
        (N > 0 && (!Y || !E)))
        return PM_EINVAL;
    RxPlan pl;
    const int rc = rx_plan(PM_EXACT_LIN, N, D, K, H, pl);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LinArgs a;
    a.G = G;
    a.logp = logp;
    a.values = values;
    a.H = (int)H;
    a.K = (int)K;
    a.L = pl.L;
    a.CH = pl.CH;
    a.nchunks = pl.space;
    a.R = pl.R;
    for (int64_t n0 = 0; n0 < N; n0 += pl.rows) {
        const int64_t nb = rx_min(pl.rows, N - n0);
        const RxWork w = rx_work(work, nb, H, pl);
        double *B = w.B, *v = w.v, *part = w.part;
        hipLaunchKernelGGL(pmx_prep_kernel, dim3(rx_blocks(nb * H)), dim3(RX_THREADS), 0, st, Y + n0 * ldy, ldy, ymu, nb, D, P,
                           H, B);
        int err = (int)hipGetLastError();
        if (err) return err;
        a.B = B;
        a.v = v;
        a.part = part;
        a.nb = nb;
        const dim3 grid((unsigned)(nb * a.R));
        hipLaunchKernelGGL(rx_lin_kernel<1>, grid, dim3(RX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = rx_combine_lse(part, nb, a.R, v, st))) return err;
        hipLaunchKernelGGL(rx_lin_kernel<2>, grid, dim3(RX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = rx_combine_sum(part, nb, a.R, H, E + n0 * lde, lde, st))) return err;
    }
    return PM_OK;
}

// ---- the moments entry -------------------------------------------------------------------------------------
// E[s], E[s s^T] (packed upper triangle) and v per row: sweeps 1 and 2 as pm_recon_exact_lin_f64 runs them (E carries its
// bits), then the pair sweeps over R3 ranges of their own -- at least RX_PAIR_MIN_CHUNKS chunks each, so that their longer
// epilogue is paid per 64 states of a thread and not per 8: sweep 3 with pin = -1 for the lo-lo pairs, then one pinned sweep per
// hi digit over the chunks where that digit's value is not 0: sum_s q(s) s_p s_h for every h, which gives the lo-hi and hi-hi
// pairs.  3 + (H - L) (K - 1) / K sweeps.
int64_t rx_pair_ranges(const RxPlan &p) { return pmx_ranges(p.space, RX_PAIR_MIN_CHUNKS, RX_MAX_RANGES); }


extern "C" int64_t pm_moments_exact_work_len(int64_t N, int64_t H) {
    if (N < 0 || H < 1) return -1;
    return rx_max(rx_min(N, RX_ROWS) * (H + 1 + RX_MAX_RANGES * rx_max(H, LIN_MAX_LL)), 1);
}

extern "C" int pm_moments_exact_plan(int64_t N, int64_t D, int64_t K, int64_t H, int64_t *out) {
    if (!out) return PM_EINVAL;
    RxPlan p;
    const int rc = rx_plan(PM_EXACT_LIN, N, D, K, H, p);
    if (rc) return rc;
    const int64_t nb = rx_min(N, p.rows), ll = (int64_t)p.L * (p.L + 1) / 2;
    out[0] = p.rows;
    out[1] = p.blocks;
    out[2] = p.L;
    out[3] = p.CH;
    out[4] = (int64_t)p.space;
    out[5] = p.R;
    out[6] = H - p.L;
    out[7] = ll;
    out[8] = rx_pair_ranges(p);
    out[9] = rx_part_off(nb, H, p);
    out[10] = rx_max(2, H) * nb * p.R;
    out[11] = rx_max(H, ll) * nb * out[8];
    return PM_OK;
}

extern "C" int pm_moments_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                                        const double *logp, const double *values, int64_t K, int64_t N, int64_t D, int64_t H,
                                        double *E, int64_t lde, double *C, int64_t ldc, double *v, double *work, void *stream) {
    if (N < 0 || D < 1 || H < 1 || K < 2 || K > PMX_LIN_MAX_K || ldy < D || lde < H || ldc < H * (H + 1) / 2 || !P || !G ||
        !logp || !values || !work || (N > 0 && (!Y || !E || !C || !v)))
        return PM_EINVAL;
    RxPlan pl;
    const int rc = rx_plan(PM_EXACT_LIN, N, D, K, H, pl);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LinArgs a;
    a.G = G;
    a.logp = logp;
    a.values = values;
    a.H = (int)H;
    a.K = (int)K;
    a.L = pl.L;
    a.CH = pl.CH;
    a.nchunks = pl.space;
    a.R = pl.R;
    const int NH = (int)H - pl.L;
    const int64_t ll = (int64_t)pl.L * (pl.L + 1) / 2, R3 = rx_pair_ranges(pl);
    for (int64_t n0 = 0; n0 < N; n0 += pl.rows) {
        const int64_t nb = rx_min(pl.rows, N - n0);
        const RxWork w = rx_work(work, nb, H, pl);
        hipLaunchKernelGGL(pmx_prep_kernel, dim3(rx_blocks(nb * H)), dim3(RX_THREADS), 0, st, Y + n0 * ldy, ldy, ymu, nb, D, P,
                           H, w.B);
        int err = (int)hipGetLastError();
        if (err) return err;
        a.B = w.B;
        a.v = v + n0;
        a.part = w.part;
        a.nb = nb;
        a.pin = -1;
        a.pdiv = 1;
        a.R = pl.R;
        const dim3 grid((unsigned)(nb * a.R));
        hipLaunchKernelGGL(rx_lin_kernel<1>, grid, dim3(RX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = rx_combine_lse(w.part, nb, a.R, v + n0, st))) return err;
        hipLaunchKernelGGL(rx_lin_kernel<2>, grid, dim3(RX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = rx_combine_sum(w.part, nb, a.R, H, E + n0 * lde, lde, st))) return err;
        a.R = R3;
        const dim3 grid3((unsigned)(nb * R3));
        for (int pin = -1; pin < NH; ++pin) {
            a.pin = pin;
            a.width = pin < 0 ? ll : H;
            if (pin > 0) a.pdiv *= (uint64_t)K;
            hipLaunchKernelGGL(rx_lin_kernel<3>, grid3, dim3(RX_THREADS), 0, st, a);
            if ((err = (int)hipGetLastError())) return err;
            hipLaunchKernelGGL(rx_combine_moments_kernel, dim3(rx_blocks(nb * a.width)), dim3(RX_THREADS), 0, st, w.part, nb, R3,
                               a.width, (int)H, pl.L, pin, C + n0 * ldc, ldc);
            if ((err = (int)hipGetLastError())) return err;
        }
    }
    return PM_OK;
}

extern "C" int pm_recon_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w,
                                      double lp1, double lp0, double inv_s2, int64_t N, int64_t D, int64_t H, double *Yhat,
                                      int64_t ldo, double *work, void *stream) {
    if (N < 0 || D < 1 || H < 1 || ldy < D || ldo < D || !Wrho || !work || (N > 0 && (!Y || !Yhat))) return PM_EINVAL;
    RxPlan pl;
    const int rc = rx_plan(PM_EXACT_MCA, N, D, 0, H, pl);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    McaArgs a;
    a.ldy = ldy;
    a.Wrho = Wrho;
    a.D = D;
    a.nstates = pl.space;
    a.inv_rho = inv_rho;
    a.lp1 = lp1;
    a.lp0 = lp0;
    a.inv_s2 = inv_s2;
    a.H = (int)H;
    a.signed_w = signed_w ? 1 : 0;
    a.R = pl.R;
    for (int64_t n0 = 0; n0 < N; n0 += pl.rows) {
        const int64_t nb = rx_min(pl.rows, N - n0);
        const RxWork w = rx_work(work, nb, H, pl);
        double *v = w.v, *part = w.part;
        a.Y = Y + n0 * ldy;
        a.v = v;
        a.part = part;
        a.nb = nb;
        const dim3 grid((unsigned)(nb * a.R));
        hipLaunchKernelGGL(rx_mca_kernel<1>, grid, dim3(RX_THREADS), 0, st, a);
        int err = (int)hipGetLastError();
        if (err) return err;
        if ((err = rx_combine_lse(part, nb, a.R, v, st))) return err;
        hipLaunchKernelGGL(rx_mca_kernel<2>, grid, dim3(RX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = rx_combine_sum(part, nb, a.R, D, Yhat + n0 * ldo, ldo, st))) return err;
    }
    return PM_OK;
}

extern "C" int pm_recon_exact_gsc_f64(const double *Y, int64_t ldy, const double *P, const double *M, const double *Psi,
                                      const double *mu, const double *logp, int64_t N, int64_t D, int64_t H, double *E,
                                      int64_t lde, double *work, void *stream) {
    if (N < 0 || D < 1 || H < 1 || ldy < D || lde < H || !P || !M || !Psi || !mu || !logp || !work || (N > 0 && (!Y || !E)))
        return PM_EINVAL;
    RxPlan pl;
    const int rc = rx_plan(PM_EXACT_GSC, N, D, 0, H, pl);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GscArgs a;
    a.M = M;
    a.Psi = Psi;
    a.mu = mu;
    a.logp = logp;
    a.nstates = pl.space;
    a.H = (int)H;
    a.R = pl.R;
    for (int64_t n0 = 0; n0 < N; n0 += pl.rows) {
        const int64_t nb = rx_min(pl.rows, N - n0);
        const RxWork w = rx_work(work, nb, H, pl);
        double *B = w.B, *v = w.v, *part = w.part;
        hipLaunchKernelGGL(pmx_prep_kernel, dim3(rx_blocks(nb * H)), dim3(RX_THREADS), 0, st, Y + n0 * ldy, ldy,
                           (const double *)nullptr, nb, D, P, H, B);
        int err = (int)hipGetLastError();
        if (err) return err;
        a.B = B;
        a.v = v;
        a.part = part;
        a.nb = nb;
        const dim3 grid((unsigned)(((nb + PMX_GSC_TN - 1) / PMX_GSC_TN) * a.R));
        hipLaunchKernelGGL(rx_gsc_kernel<1>, grid, dim3(RX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = rx_combine_lse(part, nb, a.R, v, st))) return err;
        hipLaunchKernelGGL(rx_gsc_kernel<2>, grid, dim3(RX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = rx_combine_sum(part, nb, a.R, H, E + n0 * lde, lde, st))) return err;
    }
    return PM_OK;
}

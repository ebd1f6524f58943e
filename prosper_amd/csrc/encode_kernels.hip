// encode(): the code of a datapoint -- mean[n, h] = sum_{s in K_n} q_n(s) s_h and prob[n, h] = sum_{s in K_n}
// q_n(s) [s_h != 0] -- from the log-joints an E-step pass left on the device (any leading dimension), the candidates and the
// state tables, q_n(s) = exp(a lpj[n,s] + o_s - rowLSE_n) exactly as reconstruct() weights the same states; and
// the marginals sum_{all s} q_n(s) s_h of MCA / MMCA over the whole state space by enumeration.
//
//   encode_kernel       one wavefront per datapoint, grid-stride, in the shape of recon_expect_kernel
//                       (reconstruct_kernels.hip): the row's log-sum-exp, then ONE pass over the table states that evaluates
//                       every state's weight once and adds it to the value sums t[j] (mean) and to the indicator sums u[j]
//                       (prob) of the candidate positions, then the lane-strided loop over the latents, which adds the
//                       one-cause blocks.  `mean` repeats recon_expect_kernel's operations in its order (same fma's, same
//                       butterflies): the bits of pm_recon_expect_f64.
//   enc_mca_kernel      MCA / MMCA by enumeration: rx_mca_kernel's (datapoint, state range) workgroups, one wavefront per
//                       state with its lanes over the dimensions for the energy; in sweep 2 lane h keeps the sum of the
//                       weights of the states that hold latent h.
//
// The union rule of prob.  A TSC row may hold a latent at two candidate positions; a table state of such a row is a
// pseudo-state that gives the latent two values.  mean counts both positions, as reconstruct() and the E-step's energy do;
// prob counts the state ONCE for the latent if any of its positions is non-zero.  Every position j is mapped to first[j], the
// first position that holds the same latent; a state's set of active latents is the 16-bit mask of first[j] over its non-zero
// positions, u[j] collects the weights of the states whose mask holds bit j, and only positions with first[j] == j hand their
// sum to a latent.  With distinct candidates first[j] == j and u[j] = sum_s q_s [tab[s, j] != 0].
//
// No atomics, no PM_Q and no branch on the build: every output element is written by one lane, every sum runs in an order
// fixed by H, Hprime, S and the layout alone (lane-strided partial sums, xor butterflies, ranges merged in range order): both
// libraries return the same bits and a row's bits depend on that row alone.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_common.h"
#include "pm_exact.h"

namespace {

constexpr int ENC_THREADS = 256;
constexpr int ENC_WAVES = ENC_THREADS / 64;
constexpr int64_t ENC_MAX_BLOCKS = 8192;      // (recon_expect_kernel's grid: rows are handed out the same way)

// Columns of a row as in recon_expect_kernel: [soff, soff + nblk H) one-cause blocks (block c: latent h takes the value
// bv.v[c]), [moff, moff + S) the table states (state s: the latent at candidate position j takes tab[s, j]); every other
// column (the null state) carries weight only.
__global__ __launch_bounds__(ENC_THREADS) void encode_kernel(
    const double *__restrict__ X, int64_t ld, const double *__restrict__ lse_in, double a, const double *__restrict__ off,
    const int32_t *__restrict__ cand, const double *__restrict__ tab, int64_t N, int H, int Hp, int K, int soff, int nblk,
    pm_blockvals bv, int moff, int S, double *__restrict__ mean, int64_t ldm, double *__restrict__ prob, int64_t ldp) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * ENC_WAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * ENC_WAVES;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *row = X + n * ld;
        const double lse = lse_in ? lse_in[n] : pm_row_lse(row, K, a, off, lane);
        // ---- table states: per candidate position, sum_s q_s tab[s, j] and sum_s q_s [the state holds the position's latent]
        double t[PM_MAX_HPRIME], u[PM_MAX_HPRIME];
        int cj[PM_MAX_HPRIME];
        uint64_t first = 0xFEDCBA9876543210ull;                // first[j], four bits each (wave-uniform: two scalar registers)
        static_assert(PM_MAX_HPRIME == 16, "sixteen four-bit positions in one 64-bit word, a 16-bit mask per state");
#pragma unroll
        for (int j = 0; j < PM_MAX_HPRIME; ++j) {
            t[j] = 0.0;
            u[j] = 0.0;
            cj[j] = -1;
        }
        if (S > 0) {
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j)
                if (j < Hp) cj[j] = cand[n * Hp + j];
#pragma unroll
            for (int j = PM_MAX_HPRIME - 1; j > 0; --j)        // (descending i: the smallest matching position wins)
#pragma unroll
                for (int i = j - 1; i >= 0; --i)
                    if (j < Hp && cj[i] == cj[j]) first = (first & ~(15ull << (4 * j))) | ((uint64_t)i << (4 * j));
            for (int s = lane; s < S; s += 64) {
                const double q = exp(a * row[moff + s] + (off ? off[moff + s] : 0.0) - lse);
                const double *ts = tab + (int64_t)s * Hp;
                unsigned act = 0;
#pragma unroll
                for (int j = 0; j < PM_MAX_HPRIME; ++j)
                    if (j < Hp) {
                        const double v = ts[j];
                        t[j] = fma(q, v, t[j]);
                        act |= (v != 0.0 ? 1u : 0u) << (unsigned)((first >> (4 * j)) & 15u);
                    }
#pragma unroll
                for (int j = 0; j < PM_MAX_HPRIME; ++j)
                    if (j < Hp) u[j] = fma(q, ((act >> j) & 1u) ? 1.0 : 0.0, u[j]);
            }
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j)
                if (j < Hp) {
                    t[j] = pm_wave_sum(t[j]);
                    u[j] = pm_wave_sum(u[j]);
                }
        }
        // ---- one-cause blocks, plus the table sums of the positions that hold this latent (position order)
        double *mrow = mean + n * ldm, *prow = prob + n * ldp;
        for (int h = lane; h < H; h += 64) {
            double e = 0.0, p = 0.0;
            for (int c = 0; c < nblk; ++c) {
                const int k = soff + c * H + h;
                const double q = exp(a * row[k] + (off ? off[k] : 0.0) - lse);
                e = fma(q, bv.v[c], e);
                p = fma(q, bv.v[c] != 0.0 ? 1.0 : 0.0, p);
            }
#pragma unroll
            for (int j = 0; j < PM_MAX_HPRIME; ++j)
                if (j < Hp && cj[j] == h) {
                    e += t[j];
                    if ((int)((first >> (4 * j)) & 15u) == j) p += u[j];
                }
            if (lse != lse) e = p = lse;           // a NaN row is NaN at every latent, also where no column gives one a value (TSC)
            mrow[h] = e;
            prow[h] = p > 1.0 ? 1.0 : p;           // (a NaN stays NaN)
        }
    }
}

unsigned enc_grid(int64_t N) {
    int64_t nb = (N + ENC_WAVES - 1) / ENC_WAVES;
    if (nb > ENC_MAX_BLOCKS) nb = ENC_MAX_BLOCKS;
    return (unsigned)nb;
}

// ---- MCA / MMCA by enumeration ---------------------------------------------------------------------------------------------
// l(s), the ranges, the assignment of states to wavefronts and sweep 1 are rx_mca_kernel's (recon_exact.hip; its kernels live
// in that unit's anonymous namespace, so the sweep is restated here on the definitions of pm_exact.h): a workgroup owns one
// (datapoint, range); wavefront w takes the states s0 + w, s0 + w + 4, ... with its lanes over the dimensions d = lane + 64 i
// and sums the energy over the lanes by a butterfly, so the weight q of a state is wave-uniform.  Sweep 2: lane h < H adds q
// where bit h of the state is set -- no cross-lane traffic; the four wavefronts' sums merge as (0 + 1) + (2 + 3).
constexpr int ENC_MCA_MAX_D = 1024;
constexpr int ENC_MCA_SLABS = ENC_MCA_MAX_D / 64;
static_assert(ENC_THREADS == PMX_THREADS, "the enumeration kernels run PMX_THREADS threads");
static_assert(PMX_MAX_H <= 64, "one lane per latent");

struct EncMcaArgs {
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
__global__ void __launch_bounds__(ENC_THREADS) enc_mca_kernel(EncMcaArgs a) {
    __shared__ double sAcc[SWEEP == 2 ? ENC_WAVES * 64 : 1];
    __shared__ double red[2 * ENC_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t R = a.R, n = blockIdx.x / R, r = blockIdx.x % R, D = a.D;
    const uint64_t s0 = a.nstates * (uint64_t)r / (uint64_t)R, s1 = a.nstates * (uint64_t)(r + 1) / (uint64_t)R;
    const int nsl = (int)((D + 63) / 64);
    double y[ENC_MCA_SLABS];
#pragma unroll
    for (int i = 0; i < ENC_MCA_SLABS; ++i) {
        const int64_t d = lane + 64 * i;
        y[i] = d < D ? a.Y[n * a.ldy + d] : 0.0;
    }
    const double vn = SWEEP == 2 ? a.v[n] : 0.0;
    double m = -INFINITY, s = 0.0, acc = 0.0;
    for (uint64_t st = s0 + w; st < s1; st += ENC_WAVES) {   // (st is uniform over the wavefront)
        const int k = __popcll(st);
        const double lp = (k ? k * a.lp1 : 0.0) + (a.H - k ? (a.H - k) * a.lp0 : 0.0);
        if (lp == -INFINITY) continue;
        double e = 0.0;
#pragma unroll
        for (int i = 0; i < ENC_MCA_SLABS; ++i) {
            if (i < nsl) {
                const int64_t d = lane + 64 * i;
                double wv = 0.0;
                if (d < D && st) wv = pmx_mca_wbar(a.Wrho, D, d, st, a.inv_rho, a.signed_w);
                e = fma(wv, y[i] - 0.5 * wv, e);
            }
        }
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        const double l = lp + a.inv_s2 * e;
        if (SWEEP == 1) {
            pmx_lse_add(m, s, l);
        } else {
            const double q = exp(l - vn);
            if ((st >> lane) & 1ull) acc += q;
        }
    }
    if (SWEEP == 1) {
        if (lane == 0) {
            red[2 * w] = m;
            red[2 * w + 1] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int u = 1; u < ENC_WAVES; ++u) pmx_lse_merge(m, s, red[2 * u], red[2 * u + 1]);
            a.part[2 * (r * a.nb + n)] = m;
            a.part[2 * (r * a.nb + n) + 1] = s;
        }
        return;
    }
    sAcc[w * 64 + lane] = acc;
    __syncthreads();
    if ((int)threadIdx.x < a.H)
        a.part[(r * a.nb + n) * a.H + threadIdx.x] =
            (sAcc[threadIdx.x] + sAcc[64 + threadIdx.x]) + (sAcc[128 + threadIdx.x] + sAcc[192 + threadIdx.x]);
}

// v[n] = log sum exp of the row's R partials part[2 (r nb + n)], merged in range order: one thread per row
__global__ void __launch_bounds__(ENC_THREADS) enc_combine_lse_kernel(const double *__restrict__ part, int64_t nb, int64_t R,
                                                                      double *__restrict__ v) {
    const int64_t n = (int64_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (n >= nb) return;
    double m = -INFINITY, s = 0.0;
    for (int64_t r = 0; r < R; ++r) pmx_lse_merge(m, s, part[2 * (r * nb + n)], part[2 * (r * nb + n) + 1]);
    v[n] = pmx_lse_value(m, s);
}

// out[n, h] = sum_r part[(r nb + n) H + h] in range order: one thread per output
__global__ void __launch_bounds__(ENC_THREADS) enc_combine_sum_kernel(const double *__restrict__ part, int64_t nb, int64_t R,
                                                                      int64_t H, double *__restrict__ out, int64_t ldo) {
    const int64_t i = (int64_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (i >= nb * H) return;
    const int64_t n = i / H, h = i % H;
    double acc = 0.0;
    for (int64_t r = 0; r < R; ++r) acc += part[(r * nb + n) * H + h];
    out[n * ldo + h] = acc;
}

inline unsigned enc_blocks(int64_t items) { return (unsigned)((items + ENC_THREADS - 1) / ENC_THREADS); }

}  // namespace

extern "C" int pm_encode_f64(const double *logpj, int64_t ld, const double *lse, double a, const double *col_offset,
                             const int32_t *cand, const double *state_vals, const double *block_values_host, int64_t N,
                             int64_t H, int64_t Hprime, int64_t K, int64_t single_off, int64_t nblocks, int64_t multi_off,
                             int64_t S, double *mean, int64_t ldm, double *prob, int64_t ldp, void *stream) {
    if (N < 0 || H <= 0 || K <= 0 || ld < K || ldm < H || ldp < H || single_off < 0 || nblocks < 0 || multi_off < 0 || S < 0 ||
        Hprime < 0 || (S > 0 && Hprime == 0))
        return PM_EINVAL;
    if (N == 0) return PM_OK;
    if (!logpj || !mean || !prob || (nblocks > 0 && !block_values_host) || (S > 0 && (!cand || !state_vals)) ||
        (lse && (a != 1.0 || col_offset)))
        return PM_EINVAL;
    if (Hprime > PM_MAX_HPRIME || nblocks > PM_MAX_BLOCKVALS || K > INT32_MAX / 2 || H > INT32_MAX / 16) return PM_ERANGE;
    if (single_off + nblocks * H > K || multi_off + S > K) return PM_EINVAL;
    pm_blockvals bv;
    for (int c = 0; c < PM_MAX_BLOCKVALS; ++c) bv.v[c] = c < nblocks ? block_values_host[c] : 0.0;
    hipLaunchKernelGGL(encode_kernel, dim3(enc_grid(N)), dim3(ENC_THREADS), 0, static_cast<hipStream_t>(stream), logpj, ld,
                       lse, a, col_offset, cand, state_vals, N, (int)H, (int)Hprime, (int)K, (int)single_off, (int)nblocks, bv,
                       (int)multi_off, (int)S, mean, ldm, prob, ldp);
    return (int)hipGetLastError();
}

// `work`: pm_recon_exact_work_len(N, H, D) doubles suffice.  A block of nb <= 64 rows keeps [v (nb) | partials], the partials
// 2 nb R doubles in sweep 1 and nb R H in sweep 2 with R <= 64: at most nb (1 + 64 max(H, 2)).  The query returns at least
// min(N, 256) (H + 1 + 256 max(H, 2)), the linear kind's term, which is no smaller for any N, H.
extern "C" int pm_encode_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w,
                                       double lp1, double lp0, double inv_s2, int64_t N, int64_t D, int64_t H, double *E,
                                       int64_t lde, double *work, void *stream) {
    if (N < 0 || D < 1 || H < 1 || ldy < D || lde < H || !Wrho || !work || (N > 0 && (!Y || !E))) return PM_EINVAL;
    // rows per block, the state count and R from the reconstruction entry's own plan (and its PM_ERANGE: H > 32, D > 1024)
    int64_t plan[PM_EXACT_PLAN_LEN];
    const int rc = pm_recon_exact_plan(PM_EXACT_MCA, N, D, 0, H, plan);
    if (rc) return rc;
    const int64_t rows = plan[0], R = plan[5];
    hipStream_t st = static_cast<hipStream_t>(stream);
    EncMcaArgs a;
    a.ldy = ldy;
    a.Wrho = Wrho;
    a.D = D;
    a.nstates = (uint64_t)plan[4];
    a.inv_rho = inv_rho;
    a.lp1 = lp1;
    a.lp0 = lp0;
    a.inv_s2 = inv_s2;
    a.H = (int)H;
    a.signed_w = signed_w ? 1 : 0;
    a.R = R;
    for (int64_t n0 = 0; n0 < N; n0 += rows) {
        const int64_t nb = rows < N - n0 ? rows : N - n0;
        double *v = work, *part = work + nb;
        a.Y = Y + n0 * ldy;
        a.v = v;
        a.part = part;
        a.nb = nb;
        const dim3 grid((unsigned)(nb * R));
        hipLaunchKernelGGL(enc_mca_kernel<1>, grid, dim3(ENC_THREADS), 0, st, a);
        int err = (int)hipGetLastError();
        if (err) return err;
        hipLaunchKernelGGL(enc_combine_lse_kernel, dim3(enc_blocks(nb)), dim3(ENC_THREADS), 0, st, part, nb, R, v);
        if ((err = (int)hipGetLastError())) return err;
        hipLaunchKernelGGL(enc_mca_kernel<2>, grid, dim3(ENC_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        hipLaunchKernelGGL(enc_combine_sum_kernel, dim3(enc_blocks(nb * H)), dim3(ENC_THREADS), 0, st, part, nb, R, H,
                           E + n0 * lde, lde);
        if ((err = (int)hipGetLastError())) return err;
    }
    return PM_OK;
}

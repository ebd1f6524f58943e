// Exact top-K posterior states by enumerating every latent state: per datapoint the topK states of largest
// log-joint l_n(s) -- l the log-joint of loglik_exact.hip without its row constants --, best first under the
// order (larger l, then smaller state index), their log-joints, and v_n = log sum_{all s} exp l_n(s), for the linear
// models (K-ary) and MCA / MMCA, with no state table and no (N, states) buffer.
//
// Every entry walks N in row blocks of a fixed size and runs, per block:
//   pmx_prep         B = (Y - ymu) P (rows x H), one thread per output, fixed order (linear models);
//   the sweep        the model's enumeration kernel: a workgroup owns one (row, state range); every thread keeps a running
//                    (max, sum exp) AND its IX_TOPK best (l, index) pairs, sorted, in registers; pmx_block_lse's fixed tree
//                    merges the first, ix_block_top the second -- `cols` rounds of one (l, index) arg-max over the heads of the
//                    256 sorted lists, whose winner pops -- into ONE partial per (row, range): (m, s) and a sorted list;
//   ix_combine       per row, one wavefront: v_n from the R (m, s) pairs in range order, and the R sorted lists merged by
//                    `cols` rounds of the same arg-max over their heads.
// One sweep where reconstruct's unit makes two.  R, the ranges, the assignment of states to threads and every merge are
// functions of the state count (and H, K, D, topK) alone, never of N; the order is a total order on (l, index) and indices
// are unique, so no merge depends on the order its operands arrive in.  Nothing is added by atomics and nothing depends on
// PM_DETERMINISTIC.  l_n(s), the walk of the linear states, MCA's prior and energy, the ranges and the log-sum-exp tree are
// the single definitions of pm_exact.h, shared with recon_exact.hip.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_exact.h"

namespace {

constexpr int IX_THREADS = PMX_THREADS;
constexpr int IX_TOPK = PM_INFER_EXACT_MAX_TOPK;   // entries a thread keeps, whatever topK asks for
constexpr uint32_t IX_NONE = 0xFFFFFFFFu;          // index of an empty slot (with l = -inf): after every state but the last of 2^32
constexpr int64_t IX_ROWS = 256;                   // rows per block of the host walk: linear models
constexpr int64_t IX_MAX_RANGES = 256;
constexpr int64_t IX_MCA_ROWS = 64;                // ... MCA / MMCA
constexpr int64_t IX_MCA_MAX_RANGES = 64;
constexpr uint64_t IX_LIN_MIN_CHUNKS = 2;          // chunks per range at least (where there are two)
constexpr uint64_t IX_MCA_MIN_STATES = 64;         // states per range at least: 16 per wavefront
constexpr int IX_LANE_RANGES = (int)(IX_MAX_RANGES / 64);   // ranges a lane of ix_combine owns at most
static_assert(IX_MCA_MAX_RANGES <= IX_MAX_RANGES, "ix_combine's lanes cover every range");

// (l, i) ranks before (l2, i2): the larger log-joint, then the smaller index.  False for a NaN l.
__device__ __forceinline__ bool ix_before(double l, uint32_t i, double l2, uint32_t i2) {
    return l > l2 || (l == l2 && i < i2);
}

// A thread's IX_TOPK best pairs, best first; every subscript is a compile-time constant, so the lists stay in registers.
struct IxTop {
    double l[IX_TOPK];
    uint32_t i[IX_TOPK];
};

__device__ __forceinline__ void ix_top_clear(IxTop &t) {
#pragma unroll
    for (int k = 0; k < IX_TOPK; ++k) {
        t.l[k] = -INFINITY;
        t.i[k] = IX_NONE;
    }
}

// One comparison against the list's last entry for almost every state; else a compare-swap chain that carries the displaced
// entry down.
__device__ __forceinline__ void ix_top_push(IxTop &t, double l, uint32_t i) {
    if (!ix_before(l, i, t.l[IX_TOPK - 1], t.i[IX_TOPK - 1])) return;
#pragma unroll
    for (int k = 0; k < IX_TOPK; ++k) {
        if (ix_before(l, i, t.l[k], t.i[k])) {
            const double tl = t.l[k];
            const uint32_t ti = t.i[k];
            t.l[k] = l;
            t.i[k] = i;
            l = tl;
            i = ti;
        }
    }
}

__device__ __forceinline__ void ix_top_pop(IxTop &t) {
#pragma unroll
    for (int k = 0; k + 1 < IX_TOPK; ++k) {
        t.l[k] = t.l[k + 1];
        t.i[k] = t.i[k + 1];
    }
    t.l[IX_TOPK - 1] = -INFINITY;
    t.i[IX_TOPK - 1] = IX_NONE;
}

// The `cols` best pairs of the 256 threads' sorted lists, best first, into outl / outi (thread 0 writes).  Round k: every
// thread offers its head; lane l takes lane l + o for o = 32, 16, ..., 1 where that ranks before its own, the four wavefronts'
// winners meet in LDS and every thread picks the same one; the thread that offered it pops.  redl / redi: 2 PMX_WAVES each
// (two rounds alternate, one barrier per round).  Every thread calls it.
__device__ __forceinline__ void ix_block_top(IxTop &t, int cols, double *redl, uint32_t *redi, double *outl, int64_t *outi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < cols; ++k) {
        double bl = t.l[0];
        uint32_t bi = t.i[0];
        for (int o = 32; o > 0; o >>= 1) {
            const double l2 = __shfl_down(bl, o);
            const uint32_t i2 = __shfl_down(bi, o);
            if (ix_before(l2, i2, bl, bi)) {
                bl = l2;
                bi = i2;
            }
        }
        double *rl = redl + (k & 1) * PMX_WAVES;
        uint32_t *ri = redi + (k & 1) * PMX_WAVES;
        if (lane == 0) {
            rl[wv] = bl;
            ri[wv] = bi;
        }
        __syncthreads();
        bl = rl[0];
        bi = ri[0];
#pragma unroll
        for (int u = 1; u < PMX_WAVES; ++u) {
            if (ix_before(rl[u], ri[u], bl, bi)) {
                bl = rl[u];
                bi = ri[u];
            }
        }
        if (bi != IX_NONE && t.i[0] == bi) ix_top_pop(t);
        if (threadIdx.x == 0) {
            outl[k] = bl;
            outi[k] = (int64_t)bi;
        }
    }
}

// ---- linear models (K-ary) -----------------------------------------------------------------------------------------------
struct LinArgs {
    const double *G;        // H x H
    const double *logp;     // H x K
    const double *values;   // K
    const double *B;        // nb x H
    double *lse;            // 2 nb R
    double *pl;             // nb R cols
    int64_t *pi;            // nb R cols
    int64_t nb, R;
    uint64_t nchunks;
    int H, K, L, CH, cols;
};

__global__ void __launch_bounds__(IX_THREADS) ix_lin_kernel(LinArgs a) {
    __shared__ double sG[PMX_MAX_H * PMX_MAX_H], sLogp[PMX_MAX_H * PMX_LIN_MAX_K], sVal[PMX_LIN_MAX_K], sB[PMX_MAX_H];
    __shared__ double sGv[PMX_MAX_H * PMX_LIN_MAX_K], sHv[PMX_MAX_H], sSv[PMX_MAX_H], sBh[1];
    __shared__ int sDig[PMX_MAX_H];
    __shared__ double red[2 * PMX_WAVES], redl[2 * PMX_WAVES];
    __shared__ uint32_t redi[2 * PMX_WAVES];
    const int H = a.H, K = a.K, L = a.L, CH = a.CH, NH = H - L;
    const int64_t R = a.R, n = blockIdx.x / R, r = blockIdx.x % R;
    const PmxLin w = {sG, sLogp, sVal, sB, sGv, sHv, sSv, sBh, sDig, H, K, L, CH, NH};
    pmx_lin_stage(w, a.G, a.logp, a.values, a.B + n * H);
    const uint64_t c0 = a.nchunks * (uint64_t)r / (uint64_t)R, c1 = a.nchunks * (uint64_t)(r + 1) / (uint64_t)R;
    pmx_lin_seek(w, c0);
    __syncthreads();

    uint32_t code[PMX_LIN_MAX_J];
    double plo[PMX_LIN_MAX_J], blo[PMX_LIN_MAX_J];
#pragma unroll
    for (int j = 0; j < PMX_LIN_MAX_J; ++j) pmx_lin_lo_state(w, threadIdx.x + j * IX_THREADS, code[j], plo[j], blo[j]);

    double m = -INFINITY, s = 0.0;
    IxTop top;
    ix_top_clear(top);
    for (uint64_t c = c0; c < c1; ++c) {
        pmx_lin_chunk_terms(w);
        __syncthreads();
        const double lhi = pmx_lin_chunk_prior(w);
        const double bh = sBh[0];
#pragma unroll
        for (int j = 0; j < PMX_LIN_MAX_J; ++j) {
            if (threadIdx.x + j * IX_THREADS >= (unsigned)CH) break;
            const double l = pmx_lin_logjoint(w, code[j], plo[j], blo[j], lhi, bh);
            pmx_lse_add(m, s, l);
            // the state index: chunk c, lo state threadIdx.x + 256 j (below K^H <= 2^32)
            ix_top_push(top, l, (uint32_t)(c * (uint64_t)CH + (uint64_t)(threadIdx.x + j * IX_THREADS)));
        }
        pmx_lin_next_chunk(w);
        __syncthreads();
    }
    pmx_block_lse(m, s, red);
    const int64_t slot = r * a.nb + n;
    if (threadIdx.x == 0) {
        a.lse[2 * slot] = m;
        a.lse[2 * slot + 1] = s;
    }
    ix_block_top(top, a.cols, redl, redi, a.pl + slot * a.cols, a.pi + slot * a.cols);
}

// ---- MCA / MMCA ----------------------------------------------------------------------------------------------------------
// rx_mca_kernel's assignment: wavefront w takes the states s0 + w, s0 + w + 4, ... of the range with its lanes over the
// dimensions; every lane holds the same l and keeps the same list, of which lane 0's enters the merge.  A state of zero prior
// is ranked with l = -inf and, as in the other units, its energy is not formed.
struct McaArgs {
    const double *Y;
    int64_t ldy;
    const double *Wrho;     // H x D
    double *lse, *pl;
    int64_t *pi;
    int64_t nb, R, D;
    uint64_t nstates;
    double inv_rho, lp1, lp0, inv_s2;
    int H, signed_w, cols;
};

__global__ void __launch_bounds__(IX_THREADS) ix_mca_kernel(McaArgs a) {
    __shared__ double red[2 * PMX_WAVES], redl[2 * PMX_WAVES];
    __shared__ uint32_t redi[2 * PMX_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t R = a.R, n = blockIdx.x / R, r = blockIdx.x % R, D = a.D;
    const uint64_t s0 = a.nstates * (uint64_t)r / (uint64_t)R, s1 = a.nstates * (uint64_t)(r + 1) / (uint64_t)R;
    const int nsl = (int)((D + 63) / 64);
    double y[PMX_MCA_SLABS];
#pragma unroll
    for (int i = 0; i < PMX_MCA_SLABS; ++i) {
        const int64_t d = lane + 64 * i;
        y[i] = d < D ? a.Y[n * a.ldy + d] : 0.0;
    }
    double m = -INFINITY, s = 0.0;
    IxTop top;
    ix_top_clear(top);
    for (uint64_t st = s0 + w; st < s1; st += PMX_WAVES) {   // (st is uniform over the wavefront)
        const int k = __popcll(st);
        const double lp = pmx_mca_prior(k, a.H, a.lp1, a.lp0);
        double l = -INFINITY;
        if (lp != -INFINITY) {
            double wv[PMX_MCA_SLABS];
            const double e = pmx_mca_wave_energy(a.Wrho, D, nsl, st, a.inv_rho, a.signed_w, lane, y, wv);
            l = lp + a.inv_s2 * e;
            pmx_lse_add(m, s, l);
        }
        ix_top_push(top, l, (uint32_t)st);
    }
    if (lane == 0) {
        red[2 * w] = m;
        red[2 * w + 1] = s;
    } else {
        ix_top_clear(top);
    }
    __syncthreads();
    const int64_t slot = r * a.nb + n;
    if (threadIdx.x == 0) {
        for (int u = 1; u < PMX_WAVES; ++u) pmx_lse_merge(m, s, red[2 * u], red[2 * u + 1]);
        a.lse[2 * slot] = m;
        a.lse[2 * slot + 1] = s;
    }
    ix_block_top(top, a.cols, redl, redi, a.pl + slot * a.cols, a.pi + slot * a.cols);
}

// ---- the rows' results from their R partials -----------------------------------------------------------------------------
// One wavefront per row.  v_n: the R (m, s) pairs merged in range order (every lane forms the same bits).  The lists: lane l
// owns the ranges l, l + 64, ... and a cursor into each; `cols` rounds of an arg-max over the heads (a butterfly under the
// total order: every lane holds the winner), whose owner advances.  A row with a NaN log-joint -- v_n is NaN then -- gets index
// -1 and NaN in its `cols` columns.
__global__ void __launch_bounds__(IX_THREADS) ix_combine_kernel(const double *__restrict__ lse, const double *__restrict__ pl,
                                                                const int64_t *__restrict__ pi, int64_t nb, int64_t R, int cols,
                                                                int64_t *__restrict__ top_idx, int64_t ldi,
                                                                double *__restrict__ top_l, int64_t ldl,
                                                                double *__restrict__ v) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * PMX_WAVES + (threadIdx.x >> 6);
    if (n >= nb) return;                       // (wave-uniform)
    double m = -INFINITY, s = 0.0;
    for (int64_t r = 0; r < R; ++r) pmx_lse_merge(m, s, lse[2 * (r * nb + n)], lse[2 * (r * nb + n) + 1]);
    const double vn = pmx_lse_value(m, s);
    if (lane == 0) v[n] = vn;
    if (vn != vn) {
        for (int k = lane; k < cols; k += 64) {
            top_idx[n * ldi + k] = -1;
            top_l[n * ldl + k] = (double)NAN;
        }
        return;
    }
    int pos[IX_LANE_RANGES];
#pragma unroll
    for (int q = 0; q < IX_LANE_RANGES; ++q) pos[q] = 0;
    for (int k = 0; k < cols; ++k) {
        double bl = -INFINITY;
        uint32_t bi = IX_NONE;
#pragma unroll
        for (int q = 0; q < IX_LANE_RANGES; ++q) {
            const int64_t r = lane + 64 * q;
            if (r < R && pos[q] < cols) {
                const int64_t at = (r * nb + n) * cols + pos[q];
                const double l2 = pl[at];
                const uint32_t i2 = (uint32_t)pi[at];
                if (ix_before(l2, i2, bl, bi)) {
                    bl = l2;
                    bi = i2;
                }
            }
        }
        const uint32_t mine = bi;
        for (int o = 32; o > 0; o >>= 1) {
            const double l2 = __shfl_xor(bl, o);
            const uint32_t i2 = __shfl_xor(bi, o);
            if (ix_before(l2, i2, bl, bi)) {
                bl = l2;
                bi = i2;
            }
        }
        if (bi != IX_NONE && mine == bi) {     // the range whose head won moves on (indices are unique)
#pragma unroll
            for (int q = 0; q < IX_LANE_RANGES; ++q) {
                const int64_t r = lane + 64 * q;
                if (r < R && pos[q] < cols && (uint32_t)pi[(r * nb + n) * cols + pos[q]] == bi) ++pos[q];
            }
        }
        if (lane == 0) {
            top_idx[n * ldi + k] = (int64_t)bi;
            top_l[n * ldl + k] = bl;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
inline unsigned ix_blocks(int64_t items, int64_t per) { return (unsigned)((items + per - 1) / per); }
int64_t ix_min(int64_t a, int64_t b) { return a < b ? a : b; }
int64_t ix_max(int64_t a, int64_t b) { return a > b ? a : b; }

// What a call is made of, for the two kinds (PM_EXACT_LIN, PM_EXACT_MCA): the ONE place the entries below and
// pm_infer_exact_plan take it from.  A block of nb rows keeps [B (nb x H; lin) | (m, s) (2 nb R) | l (nb R cols) | index
// (nb R cols, int64)] in `work`.
struct IxPlan {
    int64_t rows, blocks, R, cols;
    uint64_t space;
    int L, CH, has_b;
};

// PM_EINVAL / PM_ERANGE exactly as the entries document them for (N, D, K, H, topK); K is read by the linear kind alone
int ix_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, int64_t topK, IxPlan &p) {
    if (N < 0 || D < 1 || H < 1 || topK < 1) return PM_EINVAL;
    p.L = 0;
    p.CH = 1;
    uint64_t states;
    if (kind == PM_EXACT_LIN) {
        if (K < 2 || K > PMX_LIN_MAX_K) return PM_EINVAL;
        states = pmx_state_count(K, H);
        if (H > PMX_MAX_H || states == 0) return PM_ERANGE;
        pmx_lin_split(K, H, p.L, p.CH);
        p.rows = IX_ROWS;
        p.has_b = 1;
        p.space = states / (uint64_t)p.CH;
        p.R = pmx_ranges(p.space, IX_LIN_MIN_CHUNKS, IX_MAX_RANGES);
    } else if (kind == PM_EXACT_MCA) {
        if (H > PMX_MAX_H || D > PMX_MCA_MAX_D) return PM_ERANGE;
        states = 1ull << H;
        p.rows = IX_MCA_ROWS;
        p.has_b = 0;
        p.space = states;
        p.R = pmx_ranges(p.space, IX_MCA_MIN_STATES, IX_MCA_MAX_RANGES);
    } else {
        return PM_EINVAL;
    }
    if (topK > IX_TOPK) return PM_ERANGE;
    p.cols = (uint64_t)topK < states ? topK : (int64_t)states;
    p.blocks = (N + p.rows - 1) / p.rows;
    return PM_OK;
}

struct IxWork {
    double *B, *lse, *pl;
    int64_t *pi;
};

int64_t ix_lse_off(int64_t nb, int64_t H, const IxPlan &p) { return p.has_b ? nb * H : 0; }

IxWork ix_work(double *work, int64_t nb, int64_t H, const IxPlan &p) {
    IxWork w;
    w.B = work;
    w.lse = work + ix_lse_off(nb, H, p);
    w.pl = w.lse + 2 * nb * p.R;
    w.pi = reinterpret_cast<int64_t *>(w.pl + nb * p.R * p.cols);
    return w;
}

int ix_combine(const IxWork &w, int64_t nb, const IxPlan &p, int64_t *top_idx, int64_t ldi, double *top_l, int64_t ldl,
               double *v, hipStream_t st) {
    hipLaunchKernelGGL(ix_combine_kernel, dim3(ix_blocks(nb, PMX_WAVES)), dim3(IX_THREADS), 0, st, w.lse, w.pl, w.pi, nb, p.R,
                       (int)p.cols, top_idx, ldi, top_l, ldl, v);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int64_t pm_infer_exact_work_len(int64_t N, int64_t H, int64_t topK) {
    if (N < 0 || H < 1 || topK < 1 || topK > IX_TOPK) return -1;
    const int64_t a = ix_min(N, IX_ROWS) * (H + IX_MAX_RANGES * (2 + 2 * topK));
    const int64_t b = ix_min(N, IX_MCA_ROWS) * IX_MCA_MAX_RANGES * (2 + 2 * topK);
    return ix_max(ix_max(a, b), 1);
}

extern "C" int pm_infer_exact_plan(int kind, int64_t N, int64_t D, int64_t K, int64_t H, int64_t topK, int64_t *out) {
    if (!out) return PM_EINVAL;
    IxPlan p;
    const int rc = ix_plan(kind, N, D, K, H, topK, p);
    if (rc) return rc;
    const int64_t nb = ix_min(N, p.rows);
    out[0] = p.rows;
    out[1] = p.blocks;
    out[2] = p.L;
    out[3] = p.CH;
    out[4] = (int64_t)p.space;
    out[5] = p.R;
    out[6] = p.cols;
    out[7] = ix_lse_off(nb, H, p);
    out[8] = 2 * nb * p.R;
    out[9] = out[7] + out[8];
    out[10] = out[9] + nb * p.R * p.cols;
    out[11] = nb * p.R * p.cols;
    return PM_OK;
}

extern "C" int pm_infer_exact_lin_f64(const double *Y, int64_t ldy, const double *ymu, const double *P, const double *G,
                                      const double *logp, const double *values, int64_t K, int64_t N, int64_t D, int64_t H,
                                      int64_t topK, int64_t *top_idx, int64_t ldi, double *top_l, int64_t ldl, double *v,
                                      double *work, void *stream) {
    if (N < 0 || D < 1 || H < 1 || K < 2 || K > PMX_LIN_MAX_K || topK < 1 || ldy < D || !P || !G || !logp || !values || !work ||
        (N > 0 && (!Y || !top_idx || !top_l || !v)))
        return PM_EINVAL;
    IxPlan pl;
    const int rc = ix_plan(PM_EXACT_LIN, N, D, K, H, topK, pl);
    if (rc) return rc;
    if (ldi < pl.cols || ldl < pl.cols) return PM_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LinArgs a;
    a.G = G;
    a.logp = logp;
    a.values = values;
    a.H = (int)H;
    a.K = (int)K;
    a.L = pl.L;
    a.CH = pl.CH;
    a.cols = (int)pl.cols;
    a.nchunks = pl.space;
    a.R = pl.R;
    for (int64_t n0 = 0; n0 < N; n0 += pl.rows) {
        const int64_t nb = ix_min(pl.rows, N - n0);
        const IxWork w = ix_work(work, nb, H, pl);
        hipLaunchKernelGGL(pmx_prep_kernel, dim3(ix_blocks(nb * H, IX_THREADS)), dim3(IX_THREADS), 0, st, Y + n0 * ldy, ldy, ymu,
                           nb, D, P, H, w.B);
        int err = (int)hipGetLastError();
        if (err) return err;
        a.B = w.B;
        a.lse = w.lse;
        a.pl = w.pl;
        a.pi = w.pi;
        a.nb = nb;
        hipLaunchKernelGGL(ix_lin_kernel, dim3((unsigned)(nb * a.R)), dim3(IX_THREADS), 0, st, a);
        if ((err = (int)hipGetLastError())) return err;
        if ((err = ix_combine(w, nb, pl, top_idx + n0 * ldi, ldi, top_l + n0 * ldl, ldl, v + n0, st))) return err;
    }
    return PM_OK;
}

extern "C" int pm_infer_exact_mca_f64(const double *Y, int64_t ldy, const double *Wrho, double inv_rho, int signed_w,
                                      double lp1, double lp0, double inv_s2, int64_t N, int64_t D, int64_t H, int64_t topK,
                                      int64_t *top_idx, int64_t ldi, double *top_l, int64_t ldl, double *v, double *work,
                                      void *stream) {
    if (N < 0 || D < 1 || H < 1 || topK < 1 || ldy < D || !Wrho || !work || (N > 0 && (!Y || !top_idx || !top_l || !v)))
        return PM_EINVAL;
    IxPlan pl;
    const int rc = ix_plan(PM_EXACT_MCA, N, D, 0, H, topK, pl);
    if (rc) return rc;
    if (ldi < pl.cols || ldl < pl.cols) return PM_EINVAL;
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
    a.cols = (int)pl.cols;
    a.R = pl.R;
    for (int64_t n0 = 0; n0 < N; n0 += pl.rows) {
        const int64_t nb = ix_min(pl.rows, N - n0);
        const IxWork w = ix_work(work, nb, H, pl);
        a.Y = Y + n0 * ldy;
        a.lse = w.lse;
        a.pl = w.pl;
        a.pi = w.pi;
        a.nb = nb;
        hipLaunchKernelGGL(ix_mca_kernel, dim3((unsigned)(nb * a.R)), dim3(IX_THREADS), 0, st, a);
        int err = (int)hipGetLastError();
        if (err) return err;
        if ((err = ix_combine(w, nb, pl, top_idx + n0 * ldi, ldi, top_l + n0 * ldl, ldl, v + n0, st))) return err;
    }
    return PM_OK;
}

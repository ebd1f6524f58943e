// k-means++ seeding (D^2 sampling) of the mixture models on the device: H dependent rounds over the resident
// shard, every sum in a pinned order so that a NumPy restatement (tests/seeding_reference.py) reproduces the bits.
//
//   seed_update_kernel   one streaming pass: dist[n] <- (min of dist[n] and) |Y[n] - c|^2, and the ordered sum B_b of
//                        the distances of every block of rpb rows
//   seed_prefix_kernel   Q_b = ((B_0 + B_1) + ...) + B_b, S = Q_last: one lane, at most 1024 additions
//   seed_pick_kernel     the weighted draw: t = u S (+ offset); the smallest block with Q_b > t, then a walk over that
//                        block's rows; one workgroup
//   seed_gather_kernel   centres[h] = Y[idx[h]]
//
// The distance of a row.  With g the smallest power of two >= min(D, 64), partial sum l adds (Y[n,d] - c[d])^2 (difference
// rounded, product rounded, sum rounded: no fused multiply-add anywhere in this file) for d = l, l + g, l + 2g, ... in
// ascending order from +0; butterflies v_l <- v_l + v_(l xor o), o = g/2 ... 1, combine them (pm_patches_extract_f64's rule).
// A 16-byte load holds the two neighbouring elements 2p and 2p + 1, i.e. the partial sums 2j and 2j + 1 of lane j: g / 2
// lanes cover one stride of g elements, so a row belongs to a group of max(g / 2, 1) lanes -- 32 at D > 32, which puts two
// rows on a wavefront (each load instruction reads two contiguous 512-byte pieces), down to one lane per row at D <= 2.
// (A whole wavefront on one row would put two lanes on every partial sum, and their terms alternate in the pinned order.)
// The butterflies at o >= 2 pair lane j with lane j xor o/2, the one at o = 1 adds the lane's own two sums.
//
// The centre is row *idx of centre_src, read through the index the pick kernel left in device memory: the rounds of a
// one-rank run are enqueued without a host synchronisation.  The workgroup keeps it in LDS.
//
// Blocks.  rpb = ceil(N / min(1024, ceil(N / 16))) rows per block, a function of N alone (pm_col_sum_ordered_f64's rule);
// workgroup b owns block b, walks it in tiles of (4 wavefronts x rows per wavefront) rows and, when its rows are written,
// adds their distances in ascending n.  That chain is serial by definition (rpb additions; 196 at N = 200 000) and runs
// once per workgroup behind the streaming part.
//
// No atomics and no PM_DETERMINISTIC branch: both library builds give the same bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pm_common.h"
#include "prosper_hip.h"

namespace {

constexpr int SEED_WAVES = 4;
constexpr int SEED_THREADS = 64 * SEED_WAVES;
constexpr int64_t SEED_MAX_BLOCKS = 1024;
constexpr int64_t SEED_MIN_ROWS = 16;
constexpr int64_t SEED_MAX_D = 6144;                   // the centre row in 48 KB of LDS
constexpr int64_t SEED_MAX_N = (int64_t)1 << 40;       // rpb < 2^31
constexpr int SEED_UNROLL = 8;                         // loads of a lane in flight before the first is used
constexpr int SEED_CHUNK = 1024;                       // distances staged in LDS per step of an ordered walk

typedef double seed_d2 __attribute__((ext_vector_type(2)));

struct seed_plan {
    int64_t rpb, nb;
    int g, lpr, rows_per_wave, trips;
};

seed_plan seed_make_plan(int64_t N, int64_t D) {
    seed_plan p;
    int64_t nb = (N + SEED_MIN_ROWS - 1) / SEED_MIN_ROWS;
    if (nb > SEED_MAX_BLOCKS) nb = SEED_MAX_BLOCKS;
    if (nb < 1) nb = 1;
    p.rpb = N > 0 ? (N + nb - 1) / nb : 0;
    p.nb = N > 0 ? (N + p.rpb - 1) / p.rpb : 0;
    int g = 1;
    while (g < 64 && g < D) g <<= 1;
    p.g = g;
    p.lpr = g >= 2 ? g / 2 : 1;
    p.rows_per_wave = 64 / p.lpr;
    const int64_t pairs = (D + 1) / 2;
    p.trips = (int)((pairs + p.lpr - 1) / p.lpr);
    return p;
}

// VEC: every row of Y starts at a 16-byte boundary (Y aligned, ldy even): the two elements of a pair come in one load.
template <bool VEC>
__global__ __launch_bounds__(SEED_THREADS) void seed_update_kernel(const double *__restrict__ Y, int64_t ldy, int64_t N, int D,
                                                                   const double *__restrict__ centre_src, int64_t ldc,
                                                                   int64_t nc, const int64_t *__restrict__ idx_dev,
                                                                   int first, double *__restrict__ dist,
                                                                   double *__restrict__ work, int64_t rpb, int g, int lpr) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double s_c[];      // the centre, D doubles (+ 1 of padding at odd D)
    __shared__ double s_d[SEED_CHUNK];
    const int64_t ci = idx_dev ? *idx_dev : 0;
    if (ci < 0 || ci >= nc) return;                                   // exhausted: seed_prefix_kernel writes the zeros
    const int tid = threadIdx.x;
    const double *c = centre_src + ci * ldc;
    for (int d = tid; d < D; d += SEED_THREADS) s_c[d] = c[d];
    if (tid == 0 && (D & 1)) s_c[D] = 0.0;
    __syncthreads();

    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = r0 + rpb < N ? r0 + rpb : N;
    const int j = tid & (lpr - 1);                                    // lane of the row's group
    const int groups = SEED_THREADS / lpr;
    const int P = (D + 1) >> 1;                                       // pairs of a row
    for (int64_t n = r0 + tid / lpr; n < r1; n += groups) {
        const double *row = Y + n * ldy;
        double a0 = 0.0, a1 = 0.0;
        for (int p = j; p < P; p += SEED_UNROLL * lpr) {
            seed_d2 v[SEED_UNROLL];
#pragma unroll
            for (int u = 0; u < SEED_UNROLL; ++u) {
                const int q = p + u * lpr;
                v[u].x = 0.0;
                v[u].y = 0.0;
                if (q < P) {
                    if (2 * q + 1 < D) {
                        if (VEC) {
                            v[u] = *reinterpret_cast<const seed_d2 *>(row + 2 * q);
                        } else {
                            v[u].x = row[2 * q];
                            v[u].y = row[2 * q + 1];
                        }
                    } else {
                        v[u].x = row[2 * q];                          // the last element of an odd row
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SEED_UNROLL; ++u) {
                const int q = p + u * lpr;
                if (q < P) {
                    const seed_d2 cc = *reinterpret_cast<const seed_d2 *>(s_c + 2 * q);
                    const double t0 = v[u].x - cc.x;
                    a0 = a0 + t0 * t0;
                    if (2 * q + 1 < D) {
                        const double t1 = v[u].y - cc.y;
                        a1 = a1 + t1 * t1;
                    }
                }
            }
        }
        for (int o = g >> 1; o >= 2; o >>= 1) {
            a0 = a0 + __shfl_xor(a0, o >> 1, 64);
            a1 = a1 + __shfl_xor(a1, o >> 1, 64);
        }
        const double dn = g >= 2 ? a0 + a1 : a0;
        if (j == 0) {
            double keep = dn;
            if (!first) {
                const double old = dist[n];
                keep = dn < old ? dn : old;
            }
            dist[n] = keep;
        }
    }
    // B_b: this block's distances in ascending n, one addition at a time
    __threadfence_block();
    __syncthreads();
    double acc = 0.0;
    for (int64_t m0 = r0; m0 < r1; m0 += SEED_CHUNK) {
        const int cnt = (int)(r1 - m0 < SEED_CHUNK ? r1 - m0 : SEED_CHUNK);
        for (int i = tid; i < cnt; i += SEED_THREADS) s_d[i] = dist[m0 + i];
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < cnt; ++i) acc = acc + s_d[i];
        __syncthreads();
    }
    if (tid == 0) work[blockIdx.x] = acc;
}

// work = [B (nb) | Q (nb)].  An exhausted round (index < 0 or past the centre rows) writes zeros.
__global__ __launch_bounds__(SEED_THREADS) void seed_prefix_kernel(double *__restrict__ work, int nb, int64_t nc,
                                                                   const int64_t *__restrict__ idx_dev,
                                                                   double *__restrict__ potential_out) {
#pragma clang fp contract(off)
    __shared__ double s_q[SEED_MAX_BLOCKS];
    const int tid = threadIdx.x;
    const int64_t ci = idx_dev ? *idx_dev : 0;
    const bool dead = ci < 0 || ci >= nc;
    for (int b = tid; b < nb; b += SEED_THREADS) s_q[b] = dead ? 0.0 : work[b];
    __syncthreads();
    if (tid == 0) {
        double q = s_q[0];
        for (int b = 1; b < nb; ++b) {
            q = q + s_q[b];
            s_q[b] = q;
        }
        if (potential_out) *potential_out = q;
    }
    __syncthreads();
    for (int b = tid; b < nb; b += SEED_THREADS) {
        work[nb + b] = s_q[b];
        if (dead) work[b] = 0.0;
    }
}

__global__ __launch_bounds__(SEED_THREADS) void seed_pick_kernel(const double *__restrict__ dist, int64_t N,
                                                                 const double *__restrict__ work, int nb, int64_t rpb,
                                                                 const double *__restrict__ S_dev, double t_offset, double u,
                                                                 int64_t *__restrict__ idx_out) {
#pragma clang fp contract(off)
    __shared__ double s_d[SEED_CHUNK];
    __shared__ int s_lo[SEED_THREADS], s_hi[SEED_THREADS];
    __shared__ int s_block;
    __shared__ int64_t s_found;
    const int tid = threadIdx.x;
    const double *B = work, *Q = work + nb;
    const double own = Q[nb - 1];
    if (own == 0.0) {                                                 // (uniform: every lane reads the same word)
        if (tid == 0) *idx_out = -1;
        return;
    }
    const double S = S_dev ? *S_dev : own;
    const double t = u * S + t_offset;
    // the smallest block with Q_b > t; where rounding leaves none (t == Q_last), the last block that holds a positive row
    int lo = nb, hi = -1;
    for (int b = tid; b < nb; b += SEED_THREADS) {
        if (Q[b] > t && b < lo) lo = b;
        if (B[b] > 0.0 && b > hi) hi = b;
    }
    s_lo[tid] = lo;
    s_hi[tid] = hi;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < SEED_THREADS; ++i) {
            lo = s_lo[i] < lo ? s_lo[i] : lo;
            hi = s_hi[i] > hi ? s_hi[i] : hi;
        }
        s_block = lo < nb ? lo : hi;
        s_found = -1;
    }
    __syncthreads();
    const int bs = s_block;
    if (bs < 0) {
        if (tid == 0) *idx_out = -1;
        return;
    }
    const int64_t r0 = (int64_t)bs * rpb;
    const int64_t r1 = r0 + rpb < N ? r0 + rpb : N;
    double r = bs > 0 ? Q[bs - 1] : 0.0;
    int64_t last_pos = -1;
    for (int64_t m0 = r0; m0 < r1; m0 += SEED_CHUNK) {
        const int cnt = (int)(r1 - m0 < SEED_CHUNK ? r1 - m0 : SEED_CHUNK);
        for (int i = tid; i < cnt; i += SEED_THREADS) s_d[i] = dist[m0 + i];
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < cnt; ++i) {
                const double d = s_d[i];
                r = r + d;
                if (d > 0.0) last_pos = m0 + i;
                if (r > t) {
                    s_found = m0 + i;
                    break;
                }
            }
        }
        __syncthreads();
        if (s_found >= 0) break;
    }
    if (tid == 0) *idx_out = s_found >= 0 ? s_found : last_pos;
}

__global__ __launch_bounds__(SEED_THREADS) void seed_gather_kernel(const double *__restrict__ Y, int64_t ldy, int64_t N, int D,
                                                                   const int64_t *__restrict__ idx,
                                                                   double *__restrict__ centres, int64_t ldc) {
    const int64_t i = idx[blockIdx.x];
    if (i < 0 || i >= N) return;
    for (int d = threadIdx.x; d < D; d += SEED_THREADS) centres[(int64_t)blockIdx.x * ldc + d] = Y[i * ldy + d];
}

}  // namespace

extern "C" int64_t pm_seed_work_len(int64_t N) {
    if (N < 0 || N > SEED_MAX_N) return -1;
    const seed_plan p = seed_make_plan(N, 1);
    return 2 * (p.nb > 0 ? p.nb : 1);
}

extern "C" int pm_seed_plan(int64_t N, int64_t D, int32_t *out) {
    if (!out || N < 1 || D < 1) return PM_EINVAL;
    if (N > SEED_MAX_N || D > SEED_MAX_D) return PM_ERANGE;
    const seed_plan p = seed_make_plan(N, D);
    out[0] = (int32_t)p.rpb;
    out[1] = (int32_t)p.nb;
    out[2] = p.g;
    out[3] = p.rows_per_wave;
    out[4] = (int32_t)p.nb;                                           // grid of the update kernel: one workgroup per block
    out[5] = SEED_WAVES;
    out[6] = (int32_t)(((D + 1) / 2 * 2) * sizeof(double));           // dynamic LDS bytes (the centre)
    out[7] = p.trips;
    return PM_OK;
}

extern "C" int pm_seed_update_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, const double *centre_src, int64_t ldc,
                                  int64_t nc, const int64_t *idx_dev, int first, double *dist, double *work,
                                  double *potential_out, void *stream) {
    if (!Y || !centre_src || !dist || !work || N < 0 || D < 1 || nc < 1 || ldy < D || ldc < D) return PM_EINVAL;
    if (N > SEED_MAX_N || D > SEED_MAX_D) return PM_ERANGE;
    if (N == 0) return PM_OK;
    const seed_plan p = seed_make_plan(N, D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)((D + 1) / 2 * 2) * sizeof(double);
    const bool vec = (reinterpret_cast<uintptr_t>(Y) % 16 == 0) && (ldy % 2 == 0);
    if (vec)
        hipLaunchKernelGGL(seed_update_kernel<true>, dim3((unsigned)p.nb), dim3(SEED_THREADS), lds, st, Y, ldy, N, (int)D,
                           centre_src, ldc, nc, idx_dev, first, dist, work, p.rpb, p.g, p.lpr);
    else
        hipLaunchKernelGGL(seed_update_kernel<false>, dim3((unsigned)p.nb), dim3(SEED_THREADS), lds, st, Y, ldy, N, (int)D,
                           centre_src, ldc, nc, idx_dev, first, dist, work, p.rpb, p.g, p.lpr);
    if (int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(seed_prefix_kernel, dim3(1), dim3(SEED_THREADS), 0, st, work, (int)p.nb, nc, idx_dev, potential_out);
    return (int)hipGetLastError();
}

extern "C" int pm_seed_pick_f64(const double *dist, int64_t N, const double *work, const double *S, double t_offset, double u,
                                int64_t *idx_out, void *stream) {
    if (!dist || !work || !idx_out || N < 0) return PM_EINVAL;
    if (N > SEED_MAX_N) return PM_ERANGE;
    if (N == 0) return PM_OK;
    const seed_plan p = seed_make_plan(N, 1);
    hipLaunchKernelGGL(seed_pick_kernel, dim3(1), dim3(SEED_THREADS), 0, static_cast<hipStream_t>(stream), dist, N, work,
                       (int)p.nb, p.rpb, S, t_offset, u, idx_out);
    return (int)hipGetLastError();
}

extern "C" int pm_seed_gather_f64(const double *Y, int64_t ldy, int64_t N, int64_t D, const int64_t *idx, int64_t H,
                                  double *centres, int64_t ldc, void *stream) {
    if (!Y || !idx || !centres || N < 0 || D < 1 || H < 0 || ldy < D || ldc < D) return PM_EINVAL;
    if (N > SEED_MAX_N || D > INT32_MAX || H > INT32_MAX) return PM_ERANGE;
    if (N == 0 || H == 0) return PM_OK;
    hipLaunchKernelGGL(seed_gather_kernel, dim3((unsigned)H), dim3(SEED_THREADS), 0, static_cast<hipStream_t>(stream), Y, ldy, N,
                       (int)D, idx, centres, ldc);
    return (int)hipGetLastError();
}

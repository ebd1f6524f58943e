// Held-out log-likelihood: the row log-sum-exp over a model's log-joints and its fixed-order total.
//
// pm_rows_lse_f64 reads the (N, S) log-joints an E-step wrote (any leading dimension, the padded rows of the BSC buffers
// included) and forms, per row, v_n = log sum_s exp(a x_ns + o_s) with the row maximum subtracted first; the sum over the
// rows is formed without atomics: every workgroup adds a fixed range of rows in a fixed order, and one workgroup adds the
// workgroup partials in index order.  The result is a function of the input bits alone (both library builds, every run).
#include <hip/hip_runtime.h>

#include <math.h>

#include "prosper_hip.h"

namespace {

constexpr int LSE_THREADS = 256;
constexpr int LSE_WAVES = LSE_THREADS / 64;
constexpr int64_t LSE_MAX_BLOCKS = 2048;     // 8 workgroups per CU on 256 CUs
constexpr int64_t LSE_MIN_ROWS = 16;         // rows per workgroup at least (4 per wavefront)

__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// (xor butterfly: the two lanes of every exchange add the same two operands, so all lanes end with the same bits)
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

int64_t lse_blocks(int64_t N, int64_t *rows_per_block) {
    if (N <= 0) {
        *rows_per_block = 0;
        return 0;
    }
    int64_t nb = (N + LSE_MIN_ROWS - 1) / LSE_MIN_ROWS;
    if (nb > LSE_MAX_BLOCKS) nb = LSE_MAX_BLOCKS;
    const int64_t rpb = (N + nb - 1) / nb;
    *rows_per_block = rpb;
    return (N + rpb - 1) / rpb;
}

// One wavefront per row: pass 1 the maximum of a x + o (and whether any entry is NaN), pass 2 the sum of exp(a x + o - max)
// over the same row (from L2: a row of the largest state set the E-steps produce is a few KB).
__global__ void __launch_bounds__(LSE_THREADS) rows_lse_kernel(const double *__restrict__ X, int64_t ld, int64_t N, int64_t S,
                                                              double a, const double *__restrict__ off,
                                                              double *__restrict__ rows_out, double *__restrict__ work,
                                                              int64_t rows_per_block) {
    __shared__ double part[LSE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    int64_t r1 = r0 + rows_per_block;
    if (r1 > N) r1 = N;
    double acc = 0.0;
    for (int64_t n = r0 + wave; n < r1; n += LSE_WAVES) {
        const double *x = X + n * ld;
        double m = -INFINITY;
        int bad = 0;
        for (int64_t j = lane; j < S; j += 64) {
            const double z = a * x[j] + (off ? off[j] : 0.0);
            bad |= (z != z);
            m = fmax(m, z);
        }
        m = wave_max(m);
        bad = __any(bad);
        double v;
        if (bad) {
            v = NAN;
        } else if (isinf(m)) {      // all -inf (or a +inf entry): the value is m itself
            v = m;
        } else {
            double s = 0.0;
            for (int64_t j = lane; j < S; j += 64) s += exp(a * x[j] + (off ? off[j] : 0.0) - m);
            v = m + log(wave_sum(s));
        }
        if (rows_out && lane == 0) rows_out[n] = v;
        acc += v;
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0];
        for (int w = 1; w < LSE_WAVES; ++w) t += part[w];
        work[blockIdx.x] = t;
    }
}

// total[0] = the workgroup partials added in a fixed tree order (0.0 for none).
__global__ void __launch_bounds__(LSE_THREADS) lse_total_kernel(const double *__restrict__ work, int64_t nb,
                                                                double *__restrict__ total) {
    __shared__ double red[LSE_THREADS];
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < nb; i += LSE_THREADS) t += work[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int o = LSE_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = red[0];
}

}  // namespace

extern "C" int64_t pm_rows_lse_work_len(int64_t N) {
    if (N < 0) return -1;
    int64_t rpb;
    const int64_t nb = lse_blocks(N, &rpb);
    return nb > 0 ? nb : 1;
}

extern "C" int pm_rows_lse_f64(const double *logpj, int64_t ld, int64_t N, int64_t S, double a, const double *col_offset,
                               double *rows_out, double *work, double *total, void *stream) {
    if (N < 0 || S <= 0 || ld < S || !work || !total || (N > 0 && !logpj)) return PM_EINVAL;
    int64_t rpb;
    const int64_t nb = lse_blocks(N, &rpb);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nb > 0) {
        hipLaunchKernelGGL(rows_lse_kernel, dim3((unsigned)nb), dim3(LSE_THREADS), 0, st, logpj, ld, N, S, a, col_offset,
                           rows_out, work, rpb);
        const int err = (int)hipGetLastError();
        if (err) return err;
    }
    hipLaunchKernelGGL(lse_total_kernel, dim3(1), dim3(LSE_THREADS), 0, st, work, nb, total);
    return (int)hipGetLastError();
}

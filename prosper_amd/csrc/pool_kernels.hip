// Pooled feature maps of an image's patch codes: the part after encode().
//
//   codes_pool_rows_kernel     rows [n0, n0 + n) of an (N, H) code matrix -> one partial per (patch row, region column, h):
//                              the region's columns of that patch row, added (or compared) one at a time in ascending order
//   codes_pool_merge_kernel    the partials of the patch rows of the range -> added (or compared) into the running result
//                              (B, gh, gw, H), one patch row at a time in ascending order; an output is owned by one lane
//   codes_pool_finish_kernel   running sum / (rows of the region x columns of the region) -> mean
//
// The patches of an image stack are numbered row-major over (image, start row, start column): patch row R = b nr + r holds
// the nc consecutive rows [R nc, (R + 1) nc) of the code matrix.  Region i of an axis of n patch positions cut into g is
// [floor(i n / g), floor((i + 1) n / g)): never empty for g <= n.  A range is whole patch rows, so a partial never depends
// on how the matrix was split into ranges, and the running result carries over ascending ranges: the sequence of additions
// of an output is the same for every split.
//
// h runs on the lanes (a code row is H contiguous doubles); the thread index is flat over (patch row, region column, h), so
// that with H < 64 a wavefront holds several (patch row, region column) pairs instead of H busy lanes.
//
// No atomics and no PM_DETERMINISTIC branch: both library builds give the same bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "pm_common.h"
#include "prosper_hip.h"

namespace {

constexpr int POOL_THREADS = 256;
constexpr int64_t POOL_MAX_AXIS = (int64_t)1 << 30;    // patch positions along an axis (region bounds in 64 bits: i n < 2^60)
constexpr int64_t POOL_MAX_H = (int64_t)1 << 20;       // values per code

// The larger of a and x by explicit compares: a NaN on either side is the result (fmax would drop it), and of -0 and +0 the
// result is +0 whichever comes first, so the order of the compares changes no bit.
__device__ __forceinline__ double pool_max(double a, double x) {
    const bool take = (x != x) | (x > a) | ((x == a) & (__double_as_longlong(x) >= 0));      // (selects, no branches)
    return a != a ? a : (take ? x : a);
}

template <int MODE>
__device__ __forceinline__ double pool_step(double a, double x) {
    return MODE == 0 ? a + x : pool_max(a, x);
}

// a <- step(a, p[0]), step(a, p[stride]), ... over `count` values, one at a time in that order.  The loads do not depend on
// the running value: eight are issued together, then folded in order.
template <int MODE>
__device__ __forceinline__ double pool_walk(double a, const double *p, int64_t stride, int64_t count) {
    int64_t k = 0;
    for (; k + 8 <= count; k += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[u * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) a = pool_step<MODE>(a, v[u]);
        p += 8 * stride;
    }
    for (; k < count; ++k) {
        a = pool_step<MODE>(a, *p);
        p += stride;
    }
    return a;
}

// thread idx = (Rl gw + j) H + h, Rl the patch row inside the range: t[idx] = (((e + x[c0]) + x[c0 + 1]) + ...) over the
// columns [c0, c1) of region column j, e = +0 (sum) or -inf (max).  The loads of a thread do not depend on its running
// value: unrolled, they are in flight together.
template <int MODE>
__global__ __launch_bounds__(POOL_THREADS) void codes_pool_rows_kernel(const double *__restrict__ codes, int64_t ldc,
                                                                       int64_t total, int nc, int gw, int H,
                                                                       double *__restrict__ t) {
    const int64_t idx = (int64_t)blockIdx.x * POOL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int64_t pair = idx / H;
    const int h = (int)(idx - pair * H);
    const int64_t Rl = pair / gw;
    const int j = (int)(pair - Rl * gw);
    const int c0 = (int)((int64_t)j * nc / gw), c1 = (int)((int64_t)(j + 1) * nc / gw);
    t[idx] = pool_walk<MODE>(MODE == 0 ? 0.0 : -INFINITY, codes + (Rl * nc + c0) * ldc + h, ldc, c1 - c0);
}

// thread idx = (bil gw + j) H + h, bil counting the (image, region row) pairs the range touches from bi_first = b gh + i:
// acc[b, i, j, h] <- acc + t_R for the patch rows R of the range in region row i of image b, ascending.
template <int MODE>
__global__ __launch_bounds__(POOL_THREADS) void codes_pool_merge_kernel(const double *__restrict__ t, int64_t Rfirst,
                                                                        int64_t Rlast, int64_t bi_first, int64_t total,
                                                                        int nr, int gh, int64_t gwH,
                                                                        double *__restrict__ acc) {
    const int64_t idx = (int64_t)blockIdx.x * POOL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int64_t bil = idx / gwH, jh = idx - bil * gwH;
    const int64_t bi = bi_first + bil, b = bi / gh;
    const int i = (int)(bi - b * gh);
    int64_t Ra = b * nr + (int64_t)i * nr / gh, Rb = b * nr + (int64_t)(i + 1) * nr / gh - 1;
    if (Ra < Rfirst) Ra = Rfirst;
    if (Rb > Rlast) Rb = Rlast;
    if (Ra > Rb) return;
    acc[bi * gwH + jh] = pool_walk<MODE>(acc[bi * gwH + jh], t + (Ra - Rfirst) * gwH + jh, gwH, Rb - Ra + 1);
}

__global__ __launch_bounds__(POOL_THREADS) void codes_pool_finish_kernel(const double *acc, double *out, int64_t total, int nr,
                                                                         int nc, int gh, int gw, int H) {
    const int64_t idx = (int64_t)blockIdx.x * POOL_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int64_t cell = idx / H, bi = cell / gw;
    const int j = (int)(cell - bi * gw), i = (int)(bi % gh);
    const int64_t rows = (int64_t)(i + 1) * nr / gh - (int64_t)i * nr / gh;
    const int64_t cols = (int64_t)(j + 1) * nc / gw - (int64_t)j * nc / gw;
    out[idx] = acc[idx] / (double)(rows * cols);
}

// the region of an axis of n positions cut into g that holds position r
int64_t pool_region_of(int64_t r, int64_t n, int64_t g) { return ((r + 1) * g - 1) / n; }

// common argument check of the entries: PM_OK, or the status to return
int pool_check(int64_t B, int64_t nr, int64_t nc, int64_t gh, int64_t gw, int64_t H) {
    if (B < 1 || nr < 1 || nc < 1 || gh < 1 || gw < 1 || H < 1 || gh > nr || gw > nc) return PM_EINVAL;
    if (nr > POOL_MAX_AXIS || nc > POOL_MAX_AXIS || H > POOL_MAX_H) return PM_ERANGE;
    return PM_OK;
}

template <int MODE>
int pool_launch(const double *codes, int64_t ldc, int64_t Rfirst, int64_t rows, int64_t nr, int64_t nc, int64_t gh,
                int64_t gw, int64_t H, double *acc, double *work, hipStream_t stream) {
    const int64_t Rlast = Rfirst + rows - 1, gwH = gw * H;
    const int64_t bf = Rfirst / nr, bl = Rlast / nr;
    const int64_t bi_first = bf * gh + pool_region_of(Rfirst - bf * nr, nr, gh);
    const int64_t bi_last = bl * gh + pool_region_of(Rlast - bl * nr, nr, gh);
    const __int128 total1 = (__int128)rows * gwH, total2 = (__int128)(bi_last - bi_first + 1) * gwH;
    if ((total1 + POOL_THREADS - 1) / POOL_THREADS > INT32_MAX || (total2 + POOL_THREADS - 1) / POOL_THREADS > INT32_MAX)
        return PM_ERANGE;
    hipLaunchKernelGGL(codes_pool_rows_kernel<MODE>, dim3((unsigned)(((int64_t)total1 + POOL_THREADS - 1) / POOL_THREADS)),
                       dim3(POOL_THREADS), 0, stream, codes, ldc, (int64_t)total1, (int)nc, (int)gw, (int)H, work);
    int e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(codes_pool_merge_kernel<MODE>, dim3((unsigned)(((int64_t)total2 + POOL_THREADS - 1) / POOL_THREADS)),
                       dim3(POOL_THREADS), 0, stream, work, Rfirst, Rlast, bi_first, (int64_t)total2, (int)nr, (int)gh, gwH,
                       acc);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int64_t pm_codes_pool_work_len(int64_t n, int64_t nc, int64_t gw, int64_t H) {
    if (n < 0 || nc < 1 || gw < 1 || gw > nc || H < 1 || nc > POOL_MAX_AXIS || H > POOL_MAX_H || n % nc != 0) return -1;
    const __int128 len = (__int128)(n / nc) * gw * H;
    return len > INT64_MAX ? -1 : (int64_t)len;
}

extern "C" int pm_codes_pool_f64(const double *codes, int64_t ldc, int64_t n0, int64_t n, int64_t B, int64_t nr, int64_t nc,
                                 int64_t gh, int64_t gw, int64_t H, int mode, double *acc, double *work, void *stream) {
    if (!codes || !acc || !work) return PM_EINVAL;
    if (mode != 0 && mode != 1) return PM_EINVAL;
    const int st = pool_check(B, nr, nc, gh, gw, H);
    if (st != PM_OK) return st;
    if (ldc < H || n0 < 0 || n < 0 || (__int128)n0 + n > (__int128)B * nr * nc || n0 % nc != 0 || n % nc != 0) return PM_EINVAL;
    if (n == 0) return PM_OK;
    if (mode == 0)
        return pool_launch<0>(codes, ldc, n0 / nc, n / nc, nr, nc, gh, gw, H, acc, work, static_cast<hipStream_t>(stream));
    return pool_launch<1>(codes, ldc, n0 / nc, n / nc, nr, nc, gh, gw, H, acc, work, static_cast<hipStream_t>(stream));
}

extern "C" int pm_codes_pool_finish_f64(const double *acc, double *out, int64_t B, int64_t nr, int64_t nc, int64_t gh,
                                        int64_t gw, int64_t H, void *stream) {
    if (!acc || !out) return PM_EINVAL;
    const int st = pool_check(B, nr, nc, gh, gw, H);
    if (st != PM_OK) return st;
    if (B > (int64_t)INT32_MAX * POOL_THREADS) return PM_ERANGE;
    const __int128 total = (__int128)B * gh * gw * H;
    if ((total + POOL_THREADS - 1) / POOL_THREADS > INT32_MAX) return PM_ERANGE;
    hipLaunchKernelGGL(codes_pool_finish_kernel, dim3((unsigned)(((int64_t)total + POOL_THREADS - 1) / POOL_THREADS)),
                       dim3(POOL_THREADS), 0, static_cast<hipStream_t>(stream), acc, out, (int64_t)total, (int)nr, (int)nc,
                       (int)gh, (int)gw, (int)H);
    return (int)hipGetLastError();
}

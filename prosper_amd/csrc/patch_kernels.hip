// Whole-image denoising by overlapping patches: the part around reconstruct().
//
//   patches_extract_kernel      image stack (B, Hi, Wi) -> rows [n0, n0 + n) of the (N, D) patch matrix, optionally centred
//   patches_accumulate_kernel   rows [n0, n0 + n) of an (N, D) estimate matrix (+ the patches' means) -> added into a running-sum
//                               image, gather form: a pixel is owned by one lane
//   patches_finish_kernel       running sum / cover count -> output image
//   patches_accumulate_w_kernel the weighted average: running sums of w est and of w, the same gather form
//   patches_finish_w_kernel     sum of w est / sum of w -> output image
//
// The patch grid of an axis of length L (patch length p, stride s): starts min(t s, L - p) for t = 0 .. n - 1, n = (L - p) / s
// + 1, one more when s does not divide L - p (the last start is then L - p).  The patches that cover position x are the
// contiguous index range [pat_lo(x), pat_hi(x)]; nothing is looked up in an index buffer.
//
// No atomics and no PM_DETERMINISTIC branch: every output element is written by one lane, and the additions a pixel sees
// run one at a time in ascending patch number, so both library builds and every chunking give the same bits.
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>

#include "pm_common.h"
#include "prosper_hip.h"

namespace {

constexpr int PAT_THREADS = 256;
constexpr int PAT_MAX_AXIS = 1 << 30;           // image height / width (index arithmetic inside a patch row in 32 bits)
constexpr int PAT_MAX_D = 4096;                 // values per patch
constexpr int PAT_SPAN = 256;                   // patches of one patch row per extract workgroup
constexpr int ACC_PPT = 8;                      // pixels per lane of the accumulate kernel (one column, ACC_PPT rows)
constexpr int ACC_LDS = 6144;                   // doubles of staged patches (48 KiB)
constexpr int ACC_MAXQ = 512;                   // staged patches at most (their means)
constexpr int ACCW_LDS = 3072;                  // doubles of each of the two staged arrays of the weighted kernel (48 KiB
                                                // together; one slot each, up to 2 x 4097, when a slot is longer)

struct pat_axis {
    int L, p, s, tmax, n;      // tmax: last start that is a multiple of s; n: number of starts
};

pat_axis pat_make_axis(int64_t L, int64_t p, int64_t s) {
    pat_axis a;
    a.L = (int)L;
    a.p = (int)p;
    a.s = (int)(s > L ? L : s);                 // (every s > L - p gives the grid {0, L - p})
    a.tmax = (a.L - a.p) / a.s;
    a.n = a.tmax + 1 + ((a.L - a.p) % a.s != 0);
    return a;
}

__device__ __forceinline__ int pat_start(const pat_axis &a, int t) {
    const int x = t * a.s, m = a.L - a.p;
    return x < m ? x : m;
}
// first and last patch index that covers position x (the range between them is contiguous, and never empty on the
// geometries pat_check admits)
__device__ __forceinline__ int pat_lo(const pat_axis &a, int x) { return x < a.p ? 0 : (x - a.p) / a.s + 1; }
__device__ __forceinline__ int pat_hi(const pat_axis &a, int x) {
    if (a.n > a.tmax + 1 && x >= a.L - a.p) return a.tmax + 1;
    const int h = x / a.s;
    return h < a.tmax ? h : a.tmax;
}

// One group of g lanes (g a power of two <= 64) per patch; a workgroup owns `PAT_SPAN` consecutive patches of one patch row
// (image b, start row r), so that no patch needs a division of its number.  Mean of a patch: lane l of the group adds the
// elements l, l + g, l + 2g, ... in ascending order (a lane without elements holds +0), the g partial sums are combined by
// xor butterflies with strides g/2, g/4, ... 1 (v = v + v[l ^ stride]), and the sum is divided by D once.
template <typename T>
__global__ __launch_bounds__(PAT_THREADS) void patches_extract_kernel(const T *__restrict__ img, int64_t ldi, int Hi,
                                                                      pat_axis ar, pat_axis ac, int64_t n0, int64_t n,
                                                                      int64_t R0, int nspans, int D, int g, int center,
                                                                      double *__restrict__ out, int64_t ldo,
                                                                      double *__restrict__ means) {
    const int64_t R = R0 + (int64_t)(blockIdx.x / (unsigned)nspans);
    const int c_first = (int)(blockIdx.x % (unsigned)nspans) * PAT_SPAN;
    const int c_end = c_first + PAT_SPAN < ac.n ? c_first + PAT_SPAN : ac.n;
    const int64_t b = R / ar.n;
    const int r = (int)(R - b * ar.n);
    const T *base = img + (b * Hi + pat_start(ar, r)) * ldi;
    const int l = threadIdx.x & (g - 1), grp = threadIdx.x / g, ngrp = PAT_THREADS / g;
    const int a0 = l / ac.p, b0 = l - a0 * ac.p;
    for (int cc = c_first; cc < c_end; cc += ngrp) {       // uniform trip count: the shuffles below see whole groups
        const int c = cc + grp;
        const int64_t k = R * ac.n + c;
        const bool valid = c < c_end && k >= n0 && k < n0 + n;
        const T *src = base + pat_start(ac, c < ac.n ? c : 0);
        double m = 0.0;
        if (center) {
            double s = 0.0;
            int a = a0, bb = b0;
            for (int e = l; e < D; e += g) {
                if (valid) s += (double)src[(int64_t)a * ldi + bb];
                bb += g;
                if (bb >= ac.p) {
                    a += bb / ac.p;
                    bb %= ac.p;
                }
            }
            for (int o = g >> 1; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
            m = s / (double)D;
            if (valid && l == 0) means[k - n0] = m;
        }
        if (valid) {
            double *dst = out + (k - n0) * ldo;
            int a = a0, bb = b0;
            for (int e = l; e < D; e += g) {
                const double x = (double)src[(int64_t)a * ldi + bb];
                dst[e] = center ? x - m : x;
                bb += g;
                if (bb >= ac.p) {
                    a += bb / ac.p;
                    bb %= ac.p;
                }
            }
        }
    }
}

// A workgroup owns a tile of TW x TH pixels of one image (TW a power of two, TH = ACC_PPT * PAT_THREADS / TW; lane -> one
// column and ACC_PPT rows, the running sums in registers).  It walks the patch rows that reach the tile in ascending order;
// of each it stages the patches that reach its columns -- consecutive rows of the estimate matrix, read as rows -- in LDS, at
// most Q at a time in ascending order, with an odd slot length DP (lanes of neighbouring pixels read neighbouring slots:
// distinct banks), and every pixel adds its elements from there in ascending patch number.  Patches outside [n0, n0 + n)
// are skipped; a tile no patch row of the range reaches neither loads nor stores.
__global__ __launch_bounds__(PAT_THREADS) void patches_accumulate_kernel(const double *__restrict__ est, int64_t lde,
                                                                         const double *__restrict__ means, int64_t n0,
                                                                         int64_t n, int64_t Rfirst, int64_t Rlast,
                                                                         double *__restrict__ acc, int64_t lda, int Hi,
                                                                         int Wi, pat_axis ar, pat_axis ac, int D, int DP,
                                                                         int Q, int TW, int tiles_j, int tiles_i) {
    __shared__ double s_e[ACC_LDS];
    __shared__ double s_m[ACC_MAXQ];
    const int tid = threadIdx.x;
    const int tj = (int)(blockIdx.x % (unsigned)tiles_j);
    const unsigned trow = blockIdx.x / (unsigned)tiles_j;
    const int ti = (int)(trow % (unsigned)tiles_i);
    const int64_t b = trow / (unsigned)tiles_i;
    const int nrg = PAT_THREADS / TW, TH = ACC_PPT * nrg;
    const int i0 = ti * TH, j0 = tj * TW;
    const int i1 = (i0 + TH < Hi ? i0 + TH : Hi) - 1, j1 = (j0 + TW < Wi ? j0 + TW : Wi) - 1;
    const int64_t Rbase = b * ar.n;
    int64_t rl = pat_lo(ar, i0), rh = pat_hi(ar, i1);
    if (rl < Rfirst - Rbase) rl = Rfirst - Rbase;
    if (rh > Rlast - Rbase) rh = Rlast - Rbase;
    if (rl > rh) return;                                   // (uniform over the workgroup)
    const int c_lo = pat_lo(ac, j0), c_hi = pat_hi(ac, j1);
    const int j = j0 + (tid & (TW - 1)), rg = tid / TW;
    const bool col = j < Wi;
    const int jl = col ? pat_lo(ac, j) : 1, jh = col ? pat_hi(ac, j) : 0;
    double v[ACC_PPT];
    double *pix = acc + (b * Hi + i0 + rg) * lda + j;
#pragma unroll
    for (int m = 0; m < ACC_PPT; ++m) v[m] = (col && i0 + rg + nrg * m < Hi) ? pix[(int64_t)nrg * m * lda] : 0.0;
    const int qs = PAT_THREADS / D, es = PAT_THREADS % D;
    for (int r = (int)rl; r <= (int)rh; ++r) {
        const int sr = pat_start(ar, r);
        const int64_t kr = (Rbase + r) * ac.n;             // number of the patch row's first patch
        int64_t cl = c_lo, ch = c_hi;
        if (cl < n0 - kr) cl = n0 - kr;
        if (ch > n0 + n - 1 - kr) ch = n0 + n - 1 - kr;
        if (cl > ch) continue;                             // (uniform)
        for (int cA = (int)cl; cA <= (int)ch; cA += Q) {
            const int cB = cA + Q - 1 < (int)ch ? cA + Q - 1 : (int)ch;
            const int nq = cB - cA + 1;
            const double *src = est + (kr + cA - n0) * lde;
            __syncthreads();                               // the previous staging has been read
            {
                int q = tid / D, e = tid - q * D;
                for (int idx = tid; idx < nq * D; idx += PAT_THREADS) {
                    s_e[q * DP + e] = src[(int64_t)q * lde + e];
                    q += qs;
                    e += es;
                    if (e >= D) {
                        e -= D;
                        ++q;
                    }
                }
                if (means)
                    for (int q2 = tid; q2 < nq; q2 += PAT_THREADS) s_m[q2] = means[kr + cA - n0 + q2];
            }
            __syncthreads();
            const int lo = jl > cA ? jl : cA, hi = jh < cB ? jh : cB;
            for (int c = lo; c <= hi; ++c) {
                const double *slot = s_e + (c - cA) * DP + (j - pat_start(ac, c));
                const double mu = means ? s_m[c - cA] : 0.0;
#pragma unroll
                for (int m = 0; m < ACC_PPT; ++m) {
                    const int i = i0 + rg + nrg * m, a = i - sr;
                    if (i < Hi && a >= 0 && a < ar.p) {
                        const double x = slot[a * ac.p];
                        v[m] = v[m] + (means ? x + mu : x);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < ACC_PPT; ++m)
        if (col && i0 + rg + nrg * m < Hi) pix[(int64_t)nrg * m * lda] = v[m];
}

__global__ __launch_bounds__(PAT_THREADS) void patches_finish_kernel(const double *acc, int64_t lda, double *out,
                                                                     int64_t ldo, int64_t rows, int Hi, int Wi, pat_axis ar,
                                                                     pat_axis ac) {
    const int64_t idx = (int64_t)blockIdx.x * PAT_THREADS + threadIdx.x;
    if (idx >= rows * Wi) return;
    const int64_t row = idx / Wi;                          // b * Hi + i
    const int j = (int)(idx - row * Wi), i = (int)(row % Hi);
    const int64_t cover = (int64_t)(pat_hi(ar, i) - pat_lo(ar, i) + 1) * (pat_hi(ac, j) - pat_lo(ac, j) + 1);
    out[row * ldo + j] = acc[row * lda + j] / (double)cover;
}

// The weighted overlap average: patches_accumulate_kernel with a weight per patch element.  Tiles, lanes, the
// walk over the patch rows and the staging order are the same; of every staged patch two rows go to LDS side by side, the
// weight w (s_w) and the product w t (s_p, t the estimate plus the patch's mean), each computed once where the element is
// staged, and a pixel adds num <- num + (w t), den <- den + w from there in ascending patch number.  w = a b: a = 1, wgt or
// 1 / (max(wgt, 0) + floor), b = 1 or window[e]; a factor that is not there is not multiplied.  Contraction is off: the
// product is rounded before it is added.  L doubles per staged array (dynamic LDS: two rows of 4097 doubles pass 48 KiB).
__global__ __launch_bounds__(PAT_THREADS) void patches_accumulate_w_kernel(
    const double *est, int64_t lde, const double *wgt, int64_t ldw, int wmode, double floor, const double *window,
    const double *means, int64_t n0, int64_t n, int64_t Rfirst, int64_t Rlast, double *num, double *den, int64_t lda, int Hi,
    int Wi, pat_axis ar, pat_axis ac, int D, int DP, int Q, int L, int TW, int tiles_j, int tiles_i) {
#pragma clang fp contract(off)
    extern __shared__ double s_w[];
    double *s_p = s_w + L;
    const int tid = threadIdx.x;
    const int tj = (int)(blockIdx.x % (unsigned)tiles_j);
    const unsigned trow = blockIdx.x / (unsigned)tiles_j;
    const int ti = (int)(trow % (unsigned)tiles_i);
    const int64_t b = trow / (unsigned)tiles_i;
    const int nrg = PAT_THREADS / TW, TH = ACC_PPT * nrg;
    const int i0 = ti * TH, j0 = tj * TW;
    const int i1 = (i0 + TH < Hi ? i0 + TH : Hi) - 1, j1 = (j0 + TW < Wi ? j0 + TW : Wi) - 1;
    const int64_t Rbase = b * ar.n;
    int64_t rl = pat_lo(ar, i0), rh = pat_hi(ar, i1);
    if (rl < Rfirst - Rbase) rl = Rfirst - Rbase;
    if (rh > Rlast - Rbase) rh = Rlast - Rbase;
    if (rl > rh) return;                                   // (uniform over the workgroup)
    const int c_lo = pat_lo(ac, j0), c_hi = pat_hi(ac, j1);
    const int j = j0 + (tid & (TW - 1)), rg = tid / TW;
    const bool col = j < Wi;
    const int jl = col ? pat_lo(ac, j) : 1, jh = col ? pat_hi(ac, j) : 0;
    double vn[ACC_PPT], vd[ACC_PPT];
    const int64_t pix = (b * Hi + i0 + rg) * lda + j;
#pragma unroll
    for (int m = 0; m < ACC_PPT; ++m) {
        const bool own = col && i0 + rg + nrg * m < Hi;
        vn[m] = own ? num[pix + (int64_t)nrg * m * lda] : 0.0;
        vd[m] = own && den ? den[pix + (int64_t)nrg * m * lda] : 0.0;
    }
    const int qs = PAT_THREADS / D, es = PAT_THREADS % D;
    for (int r = (int)rl; r <= (int)rh; ++r) {
        const int sr = pat_start(ar, r);
        const int64_t kr = (Rbase + r) * ac.n;             // number of the patch row's first patch
        int64_t cl = c_lo, ch = c_hi;
        if (cl < n0 - kr) cl = n0 - kr;
        if (ch > n0 + n - 1 - kr) ch = n0 + n - 1 - kr;
        if (cl > ch) continue;                             // (uniform)
        for (int cA = (int)cl; cA <= (int)ch; cA += Q) {
            const int cB = cA + Q - 1 < (int)ch ? cA + Q - 1 : (int)ch;
            const int nq = cB - cA + 1;
            const int64_t k0 = kr + cA - n0;               // row of the first staged patch in est / wgt / means
            __syncthreads();                               // the previous staging has been read
            {
                int q = tid / D, e = tid - q * D;
                for (int idx = tid; idx < nq * D; idx += PAT_THREADS) {
                    double t = est[(k0 + q) * lde + e];
                    if (means) t = t + means[k0 + q];
                    double w;
                    if (wgt) {
                        double a = wgt[(k0 + q) * ldw + e];
                        if (wmode == 1) {
                            a = a < 0.0 ? 0.0 : a;         // (a NaN stays)
                            a = 1.0 / (a + floor);
                        }
                        w = window ? a * window[e] : a;
                    } else {
                        w = window ? window[e] : 1.0;
                    }
                    s_w[q * DP + e] = w;
                    s_p[q * DP + e] = w * t;
                    q += qs;
                    e += es;
                    if (e >= D) {
                        e -= D;
                        ++q;
                    }
                }
            }
            __syncthreads();
            const int lo = jl > cA ? jl : cA, hi = jh < cB ? jh : cB;
            for (int c = lo; c <= hi; ++c) {
                const int slot = (c - cA) * DP + (j - pat_start(ac, c));
#pragma unroll
                for (int m = 0; m < ACC_PPT; ++m) {
                    const int i = i0 + rg + nrg * m, a = i - sr;
                    if (i < Hi && a >= 0 && a < ar.p) {
                        vn[m] = vn[m] + s_p[slot + a * ac.p];
                        if (den) vd[m] = vd[m] + s_w[slot + a * ac.p];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < ACC_PPT; ++m)
        if (col && i0 + rg + nrg * m < Hi) {
            num[pix + (int64_t)nrg * m * lda] = vn[m];
            if (den) den[pix + (int64_t)nrg * m * lda] = vd[m];
        }
}

__global__ __launch_bounds__(PAT_THREADS) void patches_finish_w_kernel(const double *num, const double *den, int64_t lda,
                                                                       double *out, int64_t ldo, int64_t rows, int Wi) {
    const int64_t idx = (int64_t)blockIdx.x * PAT_THREADS + threadIdx.x;
    if (idx >= rows * Wi) return;
    const int64_t row = idx / Wi;                          // b * Hi + i
    const int j = (int)(idx - row * Wi);
    out[row * ldo + j] = num[row * lda + j] / den[row * lda + j];
}

// common argument check of the three entries: PM_OK, or the status to return
int pat_check(int64_t B, int64_t Hi, int64_t Wi, int64_t ph, int64_t pw, int64_t stride) {
    if (B < 1 || Hi < 1 || Wi < 1 || ph < 1 || pw < 1 || ph > Hi || pw > Wi || stride < 1) return PM_EINVAL;
    // a stride past the patch length leaves gaps between the regular starts (unless 0 and L - p are all there is and meet)
    if ((stride > ph && Hi > 2 * ph) || (stride > pw && Wi > 2 * pw)) return PM_EINVAL;
    if (Hi > PAT_MAX_AXIS || Wi > PAT_MAX_AXIS || ph * pw > PAT_MAX_D) return PM_ERANGE;
    return PM_OK;
}

template <typename T>
int pat_extract(const T *img, int64_t ldi, int64_t B, int64_t Hi, int64_t Wi, int64_t ph, int64_t pw, int64_t stride,
                int64_t n0, int64_t n, int center, double *out, int64_t ldo, double *means, void *stream) {
    if (!img || !out || (center && !means)) return PM_EINVAL;
    const int st = pat_check(B, Hi, Wi, ph, pw, stride);
    if (st != PM_OK) return st;
    const pat_axis ar = pat_make_axis(Hi, ph, stride), ac = pat_make_axis(Wi, pw, stride);
    const int64_t D = ph * pw, rows = B * ar.n;
    if (ldi < Wi || ldo < D || n0 < 0 || n < 0 || n0 > rows * ac.n - n) return PM_EINVAL;
    if (n == 0) return PM_OK;
    const int64_t R0 = n0 / ac.n, R1 = (n0 + n - 1) / ac.n;
    const int64_t nspans = (ac.n + PAT_SPAN - 1) / PAT_SPAN;
    if ((R1 - R0 + 1) * nspans > INT32_MAX) return PM_ERANGE;
    int g = 1;
    while (g < D && g < 64) g <<= 1;
    hipLaunchKernelGGL(patches_extract_kernel<T>, dim3((unsigned)((R1 - R0 + 1) * nspans)), dim3(PAT_THREADS), 0,
                       static_cast<hipStream_t>(stream), img, ldi, (int)Hi, ar, ac, n0, n, R0, (int)nspans, (int)D, g,
                       center ? 1 : 0, out, ldo, means);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int64_t pm_patches_count(int64_t length, int64_t patch, int64_t stride) {
    if (length < 1 || patch < 1 || patch > length || stride < 1 || length > PAT_MAX_AXIS) return -1;
    return pat_make_axis(length, patch, stride).n;
}

extern "C" int pm_patches_extract_f64(const double *image, int64_t ldi, int64_t B, int64_t Hi, int64_t Wi, int64_t ph,
                                      int64_t pw, int64_t stride, int64_t n0, int64_t n, int center, double *out,
                                      int64_t ldo, double *means, void *stream) {
    return pat_extract(image, ldi, B, Hi, Wi, ph, pw, stride, n0, n, center, out, ldo, means, stream);
}

extern "C" int pm_patches_extract_f32(const float *image, int64_t ldi, int64_t B, int64_t Hi, int64_t Wi, int64_t ph,
                                      int64_t pw, int64_t stride, int64_t n0, int64_t n, int center, double *out,
                                      int64_t ldo, double *means, void *stream) {
    return pat_extract(image, ldi, B, Hi, Wi, ph, pw, stride, n0, n, center, out, ldo, means, stream);
}

extern "C" int pm_patches_accumulate_f64(const double *est, int64_t lde, const double *means, int64_t n0, int64_t n,
                                         double *acc, int64_t lda, int64_t B, int64_t Hi, int64_t Wi, int64_t ph, int64_t pw,
                                         int64_t stride, void *stream) {
    if (!est || !acc) return PM_EINVAL;
    const int st = pat_check(B, Hi, Wi, ph, pw, stride);
    if (st != PM_OK) return st;
    const pat_axis ar = pat_make_axis(Hi, ph, stride), ac = pat_make_axis(Wi, pw, stride);
    const int64_t D = ph * pw, rows = B * ar.n;
    if (lde < D || lda < Wi || n0 < 0 || n < 0 || n0 > rows * ac.n - n) return PM_EINVAL;
    if (n == 0) return PM_OK;
    const int DP = (int)D | 1;
    int Q = ACC_LDS / DP;
    if (Q > ACC_MAXQ) Q = ACC_MAXQ;
    // the widest tile whose patches of one patch row (halo included: at most (TW + pw - 2) / s + 2) are staged at once
    int TW = 64;
    while (TW > 16 && (TW + pw - 2) / ac.s + 2 > Q) TW >>= 1;
    const int TH = ACC_PPT * PAT_THREADS / TW;
    const int64_t tiles_j = (Wi + TW - 1) / TW, tiles_i = (Hi + TH - 1) / TH;
    if (tiles_j * tiles_i * B > INT32_MAX) return PM_ERANGE;
    hipLaunchKernelGGL(patches_accumulate_kernel, dim3((unsigned)(tiles_j * tiles_i * B)), dim3(PAT_THREADS), 0,
                       static_cast<hipStream_t>(stream), est, lde, means, n0, n, n0 / ac.n, (n0 + n - 1) / ac.n, acc, lda,
                       (int)Hi, (int)Wi, ar, ac, (int)D, DP, Q, TW, (int)tiles_j, (int)tiles_i);
    return (int)hipGetLastError();
}

extern "C" int pm_patches_finish_f64(const double *acc, int64_t lda, double *out, int64_t ldo, int64_t B, int64_t Hi,
                                     int64_t Wi, int64_t ph, int64_t pw, int64_t stride, void *stream) {
    if (!acc || !out) return PM_EINVAL;
    const int st = pat_check(B, Hi, Wi, ph, pw, stride);
    if (st != PM_OK) return st;
    if (lda < Wi || ldo < Wi) return PM_EINVAL;
    const pat_axis ar = pat_make_axis(Hi, ph, stride), ac = pat_make_axis(Wi, pw, stride);
    const int64_t blocks = (B * Hi * Wi + PAT_THREADS - 1) / PAT_THREADS;
    if (blocks > INT32_MAX) return PM_ERANGE;
    hipLaunchKernelGGL(patches_finish_kernel, dim3((unsigned)blocks), dim3(PAT_THREADS), 0, static_cast<hipStream_t>(stream),
                       acc, lda, out, ldo, B * Hi, (int)Hi, (int)Wi, ar, ac);
    return (int)hipGetLastError();
}

extern "C" int pm_patches_accumulate_w_f64(const double *est, int64_t lde, const double *wgt, int64_t ldw, int wmode,
                                           double floor, const double *window, const double *means, int64_t n0, int64_t n,
                                           double *num, double *den, int64_t lda, int64_t B, int64_t Hi, int64_t Wi,
                                           int64_t ph, int64_t pw, int64_t stride, void *stream) {
    if (!est || !num) return PM_EINVAL;
    if (wmode != 0 && wmode != 1) return PM_EINVAL;
    if (wmode == 1 && (!wgt || !(floor >= 0.0) || floor > DBL_MAX)) return PM_EINVAL;
    const int st = pat_check(B, Hi, Wi, ph, pw, stride);
    if (st != PM_OK) return st;
    const pat_axis ar = pat_make_axis(Hi, ph, stride), ac = pat_make_axis(Wi, pw, stride);
    const int64_t D = ph * pw, rows = B * ar.n;
    if (lde < D || (wgt && ldw < D) || lda < Wi || n0 < 0 || n < 0 || n0 > rows * ac.n - n) return PM_EINVAL;
    if (n == 0) return PM_OK;
    const int DP = (int)D | 1;
    const int L = DP > ACCW_LDS ? DP : ACCW_LDS;
    const int Q = L / DP;
    // (tile width: the rule of pm_patches_accumulate_f64 at this kernel's Q)
    int TW = 64;
    while (TW > 16 && (TW + pw - 2) / ac.s + 2 > Q) TW >>= 1;
    const int TH = ACC_PPT * PAT_THREADS / TW;
    const int64_t tiles_j = (Wi + TW - 1) / TW, tiles_i = (Hi + TH - 1) / TH;
    if (tiles_j * tiles_i * B > INT32_MAX) return PM_ERANGE;
    const size_t shmem = 2 * (size_t)L * sizeof(double);
    if (int e = pm_allow_lds(reinterpret_cast<const void *>(patches_accumulate_w_kernel), shmem)) return e;
    hipLaunchKernelGGL(patches_accumulate_w_kernel, dim3((unsigned)(tiles_j * tiles_i * B)), dim3(PAT_THREADS), shmem,
                       static_cast<hipStream_t>(stream), est, lde, wgt, ldw, wmode, floor, window, means, n0, n, n0 / ac.n,
                       (n0 + n - 1) / ac.n, num, den, lda, (int)Hi, (int)Wi, ar, ac, (int)D, DP, Q, L, TW, (int)tiles_j,
                       (int)tiles_i);
    return (int)hipGetLastError();
}

extern "C" int pm_patches_finish_w_f64(const double *num, const double *den, int64_t lda, double *out, int64_t ldo,
                                       int64_t B, int64_t Hi, int64_t Wi, void *stream) {
    if (!num || !den || !out) return PM_EINVAL;
    if (B < 1 || Hi < 1 || Wi < 1 || lda < Wi || ldo < Wi) return PM_EINVAL;
    if (Hi > PAT_MAX_AXIS || Wi > PAT_MAX_AXIS) return PM_ERANGE;
    const int64_t blocks = (B * Hi * Wi + PAT_THREADS - 1) / PAT_THREADS;
    if (blocks > INT32_MAX) return PM_ERANGE;
    hipLaunchKernelGGL(patches_finish_w_kernel, dim3((unsigned)blocks), dim3(PAT_THREADS), 0,
                       static_cast<hipStream_t>(stream), num, den, lda, out, ldo, B * Hi, (int)Wi);
    return (int)hipGetLastError();
}

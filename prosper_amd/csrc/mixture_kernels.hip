// Mixture models (prosper/em/mixturemodels/MoG.py, MoP.py): log-joints + posteriors, and the M-step statistics.
//
//   scores     logpj[n,h] = (S[n,h] + c[h]) * coef + lp[h],  S = A . B^T on f64 MFMA (v_mfma_f64_16x16x4_f64)
//                MoG diagonal:  S = [Y*Y, Y] . [1/sigma^2 ; -2 W/sigma^2]^T   (Y squared in registers, never stored)
//                MoP:           S = (s_n Y) . (log W)^T                     (s_n the row scale of MoP.normalize, or 1)
//              then, in the same kernel, the row epilogue of MoG.py:213-229 / MoP.py:176-190: exp (no max subtraction),
//              NaN -> tiny, < tiny -> tiny, inf -> max/H, divide by the row sum.
//   chol       batched Cholesky of the H covariances (one workgroup per component, through global memory, any D):
//              L^-1, log|det| and a per-component status; a component that is not positive definite is left to the host
//              (np.linalg.inv + slogdet, what MoG.py:249-252 does for every component)
//   maha       S[n,h] = |L_h^-1 (y_n - w_h)|^2, or (y_n - w_h) Sigma_h^-1 (y_n - w_h)^T for a host-inverted component
//              (MoG.py:262-268, the full-covariance term) + the epilogue kernel
//   mstats     packed per-shard statistics [colsum P | Y^T P | (Y*Y)^T P or the H Gram matrices Y^T diag(p_h) Y]
//              (MoG.py:142-202, MoP.py:105-166): the datapoint range is cut into G fixed chunks, each chunk's tiles are
//              written to a workspace, and one reduction adds the G partials in chunk order -- no atomics, so the same
//              inputs give the same bits on every run, in both library builds.
//
// Tiles: 256 threads = 4 wavefronts in a 2 x 2 grid over a 64 x 64 output tile, 32 x 32 (2 x 2 MFMA blocks) per wavefront;
// the K range advances 16 at a time through LDS with the next step's operands loaded into registers during the MFMAs.
// Out-of-range K entries are loaded as zeros (they enter the sums); out-of-range rows / columns are clamped or zeroed and
// never stored.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <float.h>
#include <math.h>

#include "prosper_hip.h"

typedef double pm_d4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int BT = 64;      // output tile edge
constexpr int BK = 16;      // K step
constexpr int LDA = BK + 1; // LDS row stride of [row][k] tiles (odd: the 16 rows of a fragment read spread over banks)
constexpr int LDT = BT + 1; // LDS row stride of [k][col] tiles
constexpr int EPI_PER_LANE = PM_MAX_H / 64;

__device__ __forceinline__ pm_d4 mfma(double a, double b, pm_d4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ double wave_sum(double v) {   // fixed butterfly: every lane ends with the same bits
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The posterior epilogue of one row held in `t[0 .. H)` (lane-strided, EPI_PER_LANE per lane): writes post[0 .. H).
__device__ __forceinline__ void posterior_row(const double *__restrict__ t, double *__restrict__ post, int H, int lane) {
    const double tiny = DBL_MIN, mx = DBL_MAX / (double)H;
    double p[EPI_PER_LANE];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < EPI_PER_LANE; ++i) {
        const int h = lane + 64 * i;
        double v = 0.0;
        if (h < H) {
            v = exp(t[h]);
            if (isnan(v)) v = tiny;
            if (v < tiny) v = tiny;
            if (isinf(v)) v = mx;
        }
        p[i] = v;
        s += v;
    }
    s = wave_sum(s);
#pragma unroll
    for (int i = 0; i < EPI_PER_LANE; ++i) {
        const int h = lane + 64 * i;
        if (h < H) post[h] = p[i] / s;
    }
}

// ---- scores + epilogue (MoG diagonal: Bq != null; MoP: Bq == null) --------------------------------------------------------
// LL (log-likelihood mode, pm_mix_loglik_f64): neither logpj nor the posteriors are written.  Each 64 x 64 tile of
// z = (S + c) coef + lp goes through LDS into a running maximum and sum per row (online log-sum-exp over the H blocks), and
// `post` receives one value per row, log sum_h exp(z_nh) - (pmf ? sum_d lgamma(rs_n y_nd + yoff + 1) : 0); the row term is
// formed from the operands the first H block loads anyway.  No H bound.
template <bool SQ, bool LL = false>
__global__ __launch_bounds__(256) void mix_scores_kernel(const double *__restrict__ Y, int64_t ldy,
                                                         const double *__restrict__ rs, const double *__restrict__ Bq,
                                                         const double *__restrict__ Bl, int64_t ldb,
                                                         const double *__restrict__ c, double coef,
                                                         const double *__restrict__ lp, int64_t N, int64_t D, int64_t H,
                                                         double *__restrict__ logpj, double *__restrict__ post,
                                                         int pmf = 0, double yoff = 0.0) {
    __shared__ double As[BT * LDA];
    __shared__ double Bs[BT * LDA];
    __shared__ double Qs[SQ ? BT * LDA : 1];
    __shared__ double Zs[LL ? BT * (BT + 1) : 1];
    __shared__ double Rt[LL ? BT : 1];
    // LL: running (max, sum, NaN seen, +inf seen) of the 16 rows r = wave + 4 i this wavefront finishes (all lanes alike)
    double run_m[LL ? 16 : 1], run_s[LL ? 16 : 1];
    int run_bad[LL ? 16 : 1], run_pinf[LL ? 16 : 1];
    if constexpr (LL) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            run_m[i] = -INFINITY;
            run_s[i] = 0.0;
            run_bad[i] = 0;
            run_pinf[i] = 0;
        }
    }
    double lg = 0.0;     // LL, pmf: this thread's part of its tile row's sum of lgamma
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t row0 = (int64_t)blockIdx.x * BT;
    // loader map: thread -> (tile row tid / 4, k quad tid % 4)
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    const int64_t arow = min(row0 + lr, N - 1);
    const double ascale = rs ? rs[arow] : 1.0;
    const double *__restrict__ ya = Y + arow * ldy;
    const int nk = (int)((D + BK - 1) / BK);

    for (int64_t h0 = 0; h0 < H; h0 += BT) {
        const int64_t brow = min(h0 + lr, H - 1);
        const double *__restrict__ bl = Bl + brow * ldb;
        const double *__restrict__ bq = SQ ? Bq + brow * ldb : nullptr;
        double ra[4], rb[4], rq[4];
        auto load = [&](int kt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t k = (int64_t)kt * BK + lk + j;
                const bool in = k < D;
                ra[j] = in ? ya[k] * ascale : 0.0;
                rb[j] = in ? bl[k] : 0.0;
                if (SQ) rq[j] = in ? bq[k] : 0.0;
                if (LL && pmf && in && h0 == 0) lg += lgamma(ra[j] + yoff + 1.0);
            }
        };
        pm_d4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = pm_d4{0.0, 0.0, 0.0, 0.0};
        load(0);
        for (int kt = 0; kt < nk; ++kt) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                As[lr * LDA + lk + j] = ra[j];
                Bs[lr * LDA + lk + j] = rb[j];
                if (SQ) Qs[lr * LDA + lk + j] = rq[j];
            }
            __syncthreads();
            if (kt + 1 < nk) load(kt + 1);
#pragma unroll
            for (int kk = 0; kk < BK; kk += 4) {
                const int k = kk + (lane >> 4);
                double a[2], b[2], q[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[i] = As[(wr * 32 + i * 16 + (lane & 15)) * LDA + k];
                    b[i] = Bs[(wc * 32 + i * 16 + (lane & 15)) * LDA + k];
                    if (SQ) q[i] = Qs[(wc * 32 + i * 16 + (lane & 15)) * LDA + k];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        if (SQ) acc[i][j] = mfma(a[i] * a[i], q[j], acc[i][j]);
                        acc[i][j] = mfma(a[i], b[j], acc[i][j]);
                    }
            }
        }
        if constexpr (LL) {
            // the tile into LDS (-inf past H), then each wavefront folds its 16 rows' 64 values into the running state
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int hl = wc * 32 + j * 16 + (lane & 15);
                    const int64_t h = h0 + hl;
                    const double ch = h < H ? c[h] : 0.0, lph = h < H ? lp[h] : 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rl = wr * 32 + i * 16 + (lane >> 4) + 4 * r;
                        Zs[rl * (BT + 1) + hl] = h < H ? (acc[i][j][r] + ch) * coef + lph : -INFINITY;
                    }
                }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const double z = Zs[(wave + 4 * i) * (BT + 1) + lane];
                const int bad = __any(z != z), pinf = __any(z == INFINITY);
                const double zz = (z != z || z == INFINITY) ? -INFINITY : z;
                double bm = zz;
                for (int o = 32; o >= 1; o >>= 1) bm = fmax(bm, __shfl_xor(bm, o, 64));
                run_bad[i] |= bad;
                run_pinf[i] |= pinf;
                if (bm == -INFINITY) continue;            // (wave-uniform)
                const double bs = wave_sum(exp(zz - bm));
                const double m = fmax(run_m[i], bm);
                run_s[i] = run_s[i] * exp(run_m[i] - m) + bs * exp(bm - m);
                run_m[i] = m;
            }
        } else {
        // (S + c) * coef + lp into logpj
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t h = h0 + wc * 32 + j * 16 + (lane & 15);
                if (h >= H) continue;
                const double ch = c[h], lph = lp[h];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t n = row0 + wr * 32 + i * 16 + (lane >> 4) + 4 * r;
                    if (n < N) logpj[n * H + h] = (acc[i][j][r] + ch) * coef + lph;
                }
            }
        }
    }
    if constexpr (LL) {
        // the lgamma row term: the 4 threads of a tile row (consecutive lanes) add their parts in a fixed order
        lg += __shfl_xor(lg, 1, 64);
        lg += __shfl_xor(lg, 2, 64);
        if ((tid & 3) == 0) Rt[lr] = lg;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int rl = wave + 4 * i;
            const int64_t n = row0 + rl;
            if (n >= N || lane != 0) continue;
            double v;
            if (run_bad[i]) v = NAN;
            else if (run_pinf[i]) v = INFINITY;
            else if (run_m[i] == -INFINITY) v = -INFINITY;
            else v = run_m[i] + log(run_s[i]);
            post[n] = pmf ? v - Rt[rl] : v;
        }
        return;
    } else {
    __threadfence_block();
    __syncthreads();
    // the row epilogue: one wavefront per row, 16 rows per wavefront (rows written by this workgroup only)
    for (int r = wave; r < BT; r += 4) {
        const int64_t n = row0 + r;
        if (n >= N) break;
        posterior_row(logpj + n * H, post + n * H, (int)H, lane);
    }
    }
}

// ---- the epilogue on its own (full covariance: after mix_maha_kernel) ------------------------------------------------------
__global__ __launch_bounds__(256) void mix_posterior_kernel(const double *__restrict__ S, int64_t lds,
                                                            const double *__restrict__ c, double coef,
                                                            const double *__restrict__ lp, int64_t N, int64_t H,
                                                            double *__restrict__ logpj, double *__restrict__ post) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    for (int64_t h = lane; h < H; h += 64) logpj[n * H + h] = (S[n * lds + h] + c[h]) * coef + lp[h];
    // (each lane reads back only what it wrote itself)
    posterior_row(logpj + n * H, post + n * H, (int)H, lane);
}

// ---- full covariance: u = y_n - w_h, B_h (D x D row-major) ----------------------------------------------------------------
// mode[h] == 0 (or mode NULL): B_h = L_h^-1, S[n,h] = |B_h u|^2;  mode[h] == 1: B_h = Sinv_h^T, S[n,h] = u . (u Sinv_h).
// grid (ceil(N / 64), H).  z = B_h u one 64-entry chunk at a time on MFMA, then the row sum of z^2 (or z u) of that chunk;
// the partial row sums are added in chunk order.
__global__ __launch_bounds__(256) void mix_maha_kernel(const double *__restrict__ Y, int64_t ldy,
                                                       const double *__restrict__ W, const double *__restrict__ SinvT,
                                                       const int32_t *__restrict__ mode, int64_t N, int64_t D, int64_t H,
                                                       double *__restrict__ S, int64_t lds) {
    __shared__ double As[BT * LDA];
    __shared__ double Bs[BT * LDA];
    __shared__ double red[2][BT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t row0 = (int64_t)blockIdx.x * BT, hh = blockIdx.y;
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    const int64_t arow = min(row0 + lr, N - 1);
    const double *__restrict__ ya = Y + arow * ldy;
    const double *__restrict__ w = W + hh * D;
    const double *__restrict__ Sm = SinvT + hh * D * D;
    const bool sq = !mode || mode[hh] == 0;
    const int nk = (int)((D + BK - 1) / BK);
    if (tid < 2 * BT) red[tid / BT][tid % BT] = 0.0;

    for (int64_t j0 = 0; j0 < D; j0 += BT) {
        const int64_t brow = min(j0 + lr, D - 1);
        const double *__restrict__ bl = Sm + brow * D;
        double ra[4], rb[4];
        auto load = [&](int kt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t k = (int64_t)kt * BK + lk + j;
                const bool in = k < D;
                ra[j] = in ? ya[k] - w[k] : 0.0;
                rb[j] = in ? bl[k] : 0.0;
            }
        };
        pm_d4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = pm_d4{0.0, 0.0, 0.0, 0.0};
        load(0);
        for (int kt = 0; kt < nk; ++kt) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                As[lr * LDA + lk + j] = ra[j];
                Bs[lr * LDA + lk + j] = rb[j];
            }
            __syncthreads();
            if (kt + 1 < nk) load(kt + 1);
#pragma unroll
            for (int kk = 0; kk < BK; kk += 4) {
                const int k = kk + (lane >> 4);
                double a[2], b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[i] = As[(wr * 32 + i * 16 + (lane & 15)) * LDA + k];
                    b[i] = Bs[(wc * 32 + i * 16 + (lane & 15)) * LDA + k];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma(a[i], b[j], acc[i][j]);
            }
        }
        // row dot of this chunk: lanes sharing lane >> 4 hold one row's 16 columns per MFMA block
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tr = wr * 32 + i * 16 + (lane >> 4) + 4 * r;
                const int64_t n = min(row0 + tr, N - 1);
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int64_t col = j0 + wc * 32 + j * 16 + (lane & 15);
                    if (col < D) {
                        const double z = acc[i][j][r];
                        s += sq ? z * z : z * (Y[n * ldy + col] - w[col]);
                    }
                }
                for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
                if ((lane & 15) == 0) red[wc][tr] += s;   // one writer per (wc, row); chunks in order
            }
    }
    __syncthreads();
    if (tid < BT) {
        const int64_t n = row0 + tid;
        if (n < N) S[n * lds + hh] = red[0][tid] + red[1][tid];
    }
}

// ---- M-step statistics ------------------------------------------------------------------------------------------------------
// One 64 x 64 tile of C1[m,j] = sum_{n in chunk} (A[n,m] sa_n) B[n,j]  (+ C2 = sum (A[n,m])^2 B[n,j] when SQ) over the rows of
// chunk blockIdx.z / Z; batch z = blockIdx.z % Z shifts the row scale by z (sa = P + z: column z of P) and the output by
// z * obatch.  Output of chunk g at part + g * gstride.
template <bool SQ>
__global__ __launch_bounds__(256) void mix_tn_kernel(const double *__restrict__ A, int64_t lda, const double *__restrict__ sa,
                                                     int64_t sa_ld, const double *__restrict__ B, int64_t ldb, int64_t N,
                                                     int64_t M, int64_t NB, int64_t chunk, int64_t Z,
                                                     double *__restrict__ part, int64_t gstride, int64_t off1,
                                                     int64_t off2, int64_t obatch, int64_t offcs) {
    __shared__ double As[BK * LDT];
    __shared__ double Bs[BK * LDT];
    __shared__ double csr[BK][BT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t z = blockIdx.z % Z, g = blockIdx.z / Z;
    const int64_t m0 = (int64_t)blockIdx.x * BT, j0 = (int64_t)blockIdx.y * BT;
    const int64_t nbeg = g * chunk, nend = min(N, nbeg + chunk);
    const double *__restrict__ s = sa ? sa + z : nullptr;
    // loader map: thread -> (k row tid / 16, column quad (tid % 16) * 4)
    const int lr = tid >> 4, lc = (tid & 15) * 4;
    double ra[4], rb[4];
    // offcs >= 0: the workgroups of the first row of tiles also sum the B columns they load (sum_n P[n,j], rows n = lr mod 16
    // per thread, the 16 phases added in order at the end) into part + g * gstride + offcs
    const bool cs = offcs >= 0 && blockIdx.x == 0 && z == 0;
    double csum[4] = {0.0, 0.0, 0.0, 0.0};
    auto load = [&](int64_t n0) {
        const int64_t n = n0 + lr;
        const bool in = n < nend;
        const double sc = (in && s) ? s[n * sa_ld] : 1.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = m0 + lc + j, jj = j0 + lc + j;
            ra[j] = (in && m < M) ? A[n * lda + m] * sc : 0.0;
            rb[j] = (in && jj < NB) ? B[n * ldb + jj] : 0.0;
        }
    };
    pm_d4 acc[2][2], acc2[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = acc2[i][j] = pm_d4{0.0, 0.0, 0.0, 0.0};
    if (nbeg < nend) load(nbeg);
    for (int64_t n0 = nbeg; n0 < nend; n0 += BK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[lr * LDT + lc + j] = ra[j];
            Bs[lr * LDT + lc + j] = rb[j];
            if (cs) csum[j] += rb[j];
        }
        __syncthreads();
        if (n0 + BK < nend) load(n0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const int k = kk + (lane >> 4);
            double a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = As[k * LDT + wr * 32 + i * 16 + (lane & 15)];
                b[i] = Bs[k * LDT + wc * 32 + i * 16 + (lane & 15)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = mfma(a[i], b[j], acc[i][j]);
                    if (SQ) acc2[i][j] = mfma(a[i] * a[i], b[j], acc2[i][j]);
                }
        }
    }
    if (cs) {
#pragma unroll
        for (int j = 0; j < 4; ++j) csr[lr][lc + j] = csum[j];
        __syncthreads();
        if (tid < BT && j0 + tid < NB) {
            double t = csr[0][tid];
            for (int k = 1; k < BK; ++k) t += csr[k][tid];
            part[g * gstride + offcs + j0 + tid] = t;
        }
    }
    double *__restrict__ o1 = part + g * gstride + off1 + z * obatch;
    double *__restrict__ o2 = part + g * gstride + off2 + z * obatch;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t jj = j0 + wc * 32 + j * 16 + (lane & 15);
            if (jj >= NB) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + wr * 32 + i * 16 + (lane >> 4) + 4 * r;
                if (m >= M) continue;
                o1[m * NB + jj] = acc[i][j][r];
                if (SQ) o2[m * NB + jj] = acc2[i][j][r];
            }
        }
}

// out[i] = sum over g = 0 .. G-1 in order of part[g * L + i]
__global__ __launch_bounds__(256) void mix_reduce_kernel(const double *__restrict__ part, int64_t L, int64_t G,
                                                         double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    double s = part[i];
    for (int64_t g = 1; g < G; ++g) s += part[g * L + i];
    out[i] = s;
}

// ---- batched Cholesky: one workgroup per component, L and L^-1 in global memory (any D) -------------------------------------
// Left-looking by columns: d_j = A_jj - sum_{k<j} L_jk^2 (a fixed-order workgroup reduction), then the rows below in parallel,
// L_ij = (A_ij - sum_{k<j} L_ik L_jk) / sqrt(d_j); the lower triangle of A is read.  A pivot that is not a positive finite
// number ends the component with status 1 (not positive definite) and logdet NaN.  Then X = L^-1, one column per thread by
// forward substitution.  logdet = sum_j log d_j = log det A.
__global__ __launch_bounds__(256) void mix_chol_kernel(const double *__restrict__ S, int64_t D, double *__restrict__ L,
                                                       double *__restrict__ X, double *__restrict__ logdet,
                                                       int32_t *__restrict__ status) {
    __shared__ double red[256];
    __shared__ double piv;
    const int tid = threadIdx.x;
    const int64_t h = blockIdx.x;
    const double *__restrict__ A = S + h * D * D;
    double *__restrict__ Lh = L + h * D * D;
    double *__restrict__ Xh = X + h * D * D;
    double ld = 0.0;
    for (int64_t j = 0; j < D; ++j) {
        double s = 0.0;
        for (int64_t k = tid; k < j; k += 256) s += Lh[j * D + k] * Lh[j * D + k];
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o >= 1; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) piv = A[j * D + j] - red[0];
        __syncthreads();
        const double d = piv;
        if (!(d > 0.0) || !isfinite(d)) {          // uniform over the workgroup
            if (tid == 0) {
                status[h] = 1;
                logdet[h] = NAN;
            }
            return;
        }
        ld += log(d);
        const double ljj = sqrt(d);
        for (int64_t i = j + 1 + tid; i < D; i += 256) {
            double t = A[i * D + j];
            for (int64_t k = 0; k < j; ++k) t -= Lh[i * D + k] * Lh[j * D + k];
            Lh[i * D + j] = t / ljj;
        }
        if (tid == 0) Lh[j * D + j] = ljj;
        __threadfence_block();
        __syncthreads();
    }
    for (int64_t c = tid; c < D; c += 256) {
        for (int64_t i = 0; i < c; ++i) Xh[i * D + c] = 0.0;
        Xh[c * D + c] = 1.0 / Lh[c * D + c];
        for (int64_t i = c + 1; i < D; ++i) {
            double t = 0.0;
            for (int64_t k = c; k < i; ++k) t += Lh[i * D + k] * Xh[k * D + c];
            Xh[i * D + c] = -t / Lh[i * D + i];
        }
    }
    if (tid == 0) {
        status[h] = 0;
        logdet[h] = ld;
    }
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int launched() { return (int)hipGetLastError(); }

int64_t stats_tiles(int64_t D, int64_t H) { return cdiv(D, BT) * cdiv(H, BT); }

}  // namespace

extern "C" int pm_mix_scores_f64(const double *Y, int64_t ldy, const double *rowscale, const double *Bq, const double *Bl,
                                 int64_t ldb, const double *c, double coef, const double *lp, int64_t N, int64_t D,
                                 int64_t H, double *logpj, double *post, void *stream) {
    if (!Y || !Bl || !c || !lp || !logpj || !post || N <= 0 || D <= 0 || H <= 0 || ldy < D || ldb < D) return PM_EINVAL;
    if (Bq && rowscale) return PM_EINVAL;
    if (H > PM_MAX_H) return PM_ERANGE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)cdiv(N, BT));
    if (Bq)
        mix_scores_kernel<true><<<grid, 256, 0, st>>>(Y, ldy, nullptr, Bq, Bl, ldb, c, coef, lp, N, D, H, logpj, post);
    else
        mix_scores_kernel<false><<<grid, 256, 0, st>>>(Y, ldy, rowscale, nullptr, Bl, ldb, c, coef, lp, N, D, H, logpj, post);
    return launched();
}

extern "C" int pm_mix_loglik_f64(const double *Y, int64_t ldy, const double *rowscale, const double *Bq, const double *Bl,
                                 int64_t ldb, const double *c, double coef, const double *lp, int64_t N, int64_t D,
                                 int64_t H, int pmf, double yoff, double *rows, void *stream) {
    if (!Y || !Bl || !c || !lp || !rows || N <= 0 || D <= 0 || H <= 0 || ldy < D || ldb < D) return PM_EINVAL;
    if (Bq && (rowscale || pmf)) return PM_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)cdiv(N, BT));
    if (Bq)
        mix_scores_kernel<true, true><<<grid, 256, 0, st>>>(Y, ldy, nullptr, Bq, Bl, ldb, c, coef, lp, N, D, H, nullptr, rows,
                                                             0, 0.0);
    else
        mix_scores_kernel<false, true><<<grid, 256, 0, st>>>(Y, ldy, rowscale, nullptr, Bl, ldb, c, coef, lp, N, D, H, nullptr,
                                                              rows, pmf, yoff);
    return launched();
}

extern "C" int pm_mix_chol_f64(const double *S, int64_t D, int64_t H, double *L_work, double *Linv, double *logdet,
                               int32_t *status, void *stream) {
    if (!S || !L_work || !Linv || !logdet || !status || D <= 0 || H <= 0) return PM_EINVAL;
    if (H > 2147483647) return PM_ERANGE;
    mix_chol_kernel<<<dim3((unsigned)H), 256, 0, static_cast<hipStream_t>(stream)>>>(S, D, L_work, Linv, logdet, status);
    return launched();
}

extern "C" int pm_mix_maha_f64(const double *Y, int64_t ldy, const double *W, const double *B, const int32_t *mode, int64_t N,
                               int64_t D, int64_t H, double *S, int64_t lds, void *stream) {
    if (!Y || !W || !B || !S || N <= 0 || D <= 0 || H <= 0 || ldy < D || lds < H) return PM_EINVAL;
    if (H > 65535) return PM_ERANGE;
    mix_maha_kernel<<<dim3((unsigned)cdiv(N, BT), (unsigned)H), 256, 0, static_cast<hipStream_t>(stream)>>>(
        Y, ldy, W, B, mode, N, D, H, S, lds);
    return launched();
}

extern "C" int pm_mix_posterior_f64(const double *S, int64_t lds, const double *c, double coef, const double *lp, int64_t N,
                                    int64_t H, double *logpj, double *post, void *stream) {
    if (!S || !c || !lp || !logpj || !post || N <= 0 || H <= 0 || lds < H) return PM_EINVAL;
    if (H > PM_MAX_H) return PM_ERANGE;
    mix_posterior_kernel<<<dim3((unsigned)cdiv(N, 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(S, lds, c, coef, lp, N, H,
                                                                                                 logpj, post);
    return launched();
}

extern "C" int64_t pm_mix_stats_len(int64_t D, int64_t H, int kind) {
    if (D <= 0 || H <= 0 || kind < 0 || kind > 2) return -1;
    return H + D * H + (kind == 1 ? D * H : kind == 2 ? H * D * D : 0);
}

extern "C" int64_t pm_mix_stats_chunks(int64_t N, int64_t D, int64_t H, int kind) {
    if (N <= 0 || D <= 0 || H <= 0 || kind < 0 || kind > 2) return -1;
    // about 1024 workgroups in the Y^T P launch, chunks of at least 256 datapoints, at most 64 partials, the workspace
    // (G packed statistics) at most 2^27 doubles, and G * H within grid z for the Gram launch
    int64_t G = cdiv(1024, stats_tiles(D, H));
    G = std::min<int64_t>(G, std::max<int64_t>(1, N / 256));
    G = std::min<int64_t>(G, std::max<int64_t>(1, ((int64_t)1 << 27) / pm_mix_stats_len(D, H, kind)));
    if (kind == 2) G = std::min<int64_t>(G, std::max<int64_t>(1, 65535 / H));
    return std::max<int64_t>(1, std::min<int64_t>(G, 64));
}

extern "C" int64_t pm_mix_mstats_work_len(int64_t N, int64_t D, int64_t H, int kind) {
    const int64_t G = pm_mix_stats_chunks(N, D, H, kind), L = pm_mix_stats_len(D, H, kind);
    return (G < 0 || L < 0) ? -1 : G * L;
}

extern "C" int pm_mix_mstats_f64(const double *Y, int64_t ldy, const double *P, int64_t ldp, const double *rowscale,
                                 int64_t N, int64_t D, int64_t H, int kind, double *work, double *stats, void *stream) {
    if (!Y || !P || !work || !stats || N <= 0 || D <= 0 || H <= 0 || ldy < D || ldp < H || kind < 0 || kind > 2)
        return PM_EINVAL;
    if (rowscale && kind != 0) return PM_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t G = pm_mix_stats_chunks(N, D, H, kind), L = pm_mix_stats_len(D, H, kind);
    if (G * (kind == 2 ? H : 1) > 65535) return PM_ERANGE;
    const int64_t chunk = cdiv(cdiv(N, G), BK) * BK;
    // Y^T P (row-scaled by s_n for MoP's normalisation), with (Y*Y)^T P for the diagonal MoG
    const dim3 g1((unsigned)cdiv(D, BT), (unsigned)cdiv(H, BT), (unsigned)G);
    if (kind == 1)
        mix_tn_kernel<true><<<g1, 256, 0, st>>>(Y, ldy, nullptr, 0, P, ldp, N, D, H, chunk, 1, work, L, H, H + D * H, 0, 0);
    else
        mix_tn_kernel<false><<<g1, 256, 0, st>>>(Y, ldy, rowscale, 1, P, ldp, N, D, H, chunk, 1, work, L, H, 0, 0, 0);
    if (int e = launched()) return e;
    if (kind == 2) {   // Gram_h = Y^T diag(p_h) Y: batch z = h scales the rows of A by column h of P
        const dim3 g2((unsigned)cdiv(D, BT), (unsigned)cdiv(D, BT), (unsigned)(G * H));
        mix_tn_kernel<false><<<g2, 256, 0, st>>>(Y, ldy, P, ldp, Y, ldy, N, D, D, chunk, H, work, L, H + D * H, 0, D * D, -1);
        if (int e = launched()) return e;
    }
    mix_reduce_kernel<<<dim3((unsigned)cdiv(L, 256)), 256, 0, st>>>(work, L, G, stats);
    return launched();
}

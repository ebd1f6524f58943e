// Training on incomplete data: the M-step of BSC for rows of which only the dimensions with a non-zero mask
// byte were observed.  With a mask every data dimension d has its own H x H normal matrix
//   A_d = sum_n m_nd E_q[s s^T]_n,   r_d = sum_n m_nd x_nd E_q[s]_n,   A_d w_d = r_d.
// E[s s^T]_n is diag(E[s]_n) plus the off-diagonal block over the row's H' candidates, so
//   rows    per row: E[s] (H), the candidates' pair moments q2 (H'(H'-1)/2) and the expected energy sum_s q(s) e(s), from the
//           masked E-step's log-joints and their log-sum-exp
//   colsum  sums over the rows in a fixed order (fixed row ranges per workgroup, the partials added in index order)
//   pairs   A[d, c_i, c_j] = sum_n m_nd q2_n[(i,j)], both triangles, and the diagonal from the dense product E[s]^T Mf
//   solve   w_d = A_d^-1 r_d with one step of iterative refinement behind pm_spd_inverse_batch_f64, the old row kept
//           where the pivots say the system is not usable
// No atomics anywhere: every output element is written once, every cell of A is added to in ascending row order by one
// wavefront.  Both library builds run the same code and return the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_common.h"

namespace {

constexpr int RW = 4;             // rows kernel: wavefronts per workgroup, one row each
constexpr int RCH = 256;          // rows kernel: table states per LDS chunk of a wavefront
constexpr int PWV = 16;           // pairs kernel: wavefronts per workgroup
constexpr int PDS = 64;           // pairs kernel: dimensions per slab, one per lane
constexpr int PCELLS = 256;       // pairs kernel: (latent row, column) cells of a tile: 64 x 256 doubles = 128 KB of LDS
constexpr int64_t MT_MAX_H = 256;
constexpr int64_t MT_MAX_CELLS = (int64_t)1 << 28;   // D H^2: A and its inverses are two tensors of at most 2 GiB
constexpr int64_t CS_MAX_BLOCKS = 1024;
constexpr int64_t CS_MIN_ROWS = 16;

// ---------------------------------------------------------------------------------------------
// rows: one wavefront per row.  q(s) = exp(logpj_s - lse); the energy of a state is recovered from its log-joint,
// e_s = (logpj_s - ppil |s|) / ecoef (logpj_s = ppil |s| + ecoef e_s is how pm_bsc_masked_estep_f64 formed it).
// Lane l owns the pairs l and l + 64 and, for l < H', candidate position l: it adds q(s) over the table states that
// contain them in ascending s -- no reduction across lanes, the order is fixed by the state table alone.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * RW) void mtrain_rows_kernel(const double *__restrict__ logpj, int64_t ldl,
                                                              const double *__restrict__ lse,
                                                              const int32_t *__restrict__ cand,
                                                              const uint16_t *__restrict__ masks, int S, double ppil,
                                                              double ecoef, int64_t N, int H, int Hp,
                                                              double *__restrict__ es, int64_t lde,
                                                              double *__restrict__ q2, int64_t ldq,
                                                              double *__restrict__ energy) {
    __shared__ double s_q[RW][RCH];
    __shared__ double s_m[RW][16];
    __shared__ int32_t s_c[RW][16];
    __shared__ uint16_t s_k[RW][RCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npair = Hp * (Hp - 1) / 2;
    // bit masks of what this lane owns; 0x10000 never matches a 16-bit state mask
    unsigned pm0 = 0x10000u, pm1 = 0x10000u;
    {
        int p = 0;
        for (int i = 0; i < Hp; ++i)
            for (int j = i + 1; j < Hp; ++j, ++p) {
                if (p == lane) pm0 = (1u << i) | (1u << j);
                if (p == lane + 64) pm1 = (1u << i) | (1u << j);
            }
    }
    const unsigned cm = lane < Hp ? (1u << lane) : 0x10000u;
    double *wq = s_q[wave], *wm = s_m[wave];
    int32_t *wc = s_c[wave];
    uint16_t *wk = s_k[wave];

    const int64_t wave0 = (int64_t)blockIdx.x * RW + wave;
    const int64_t nwaves = (int64_t)gridDim.x * RW;
    for (int64_t n = wave0; n < N; n += nwaves) {
        const double *lp = logpj + n * ldl;
        const double l = lse[n];
        double en = 0.0;
        if (lane == 0) {
            const double x = lp[0], q = exp(x - l);
            en = q == 0.0 ? en : q * (x / ecoef);      // (q = 0: no 0 * inf; a NaN row stays NaN)
        }
        double a0 = 0.0, a1 = 0.0, am = 0.0;
        for (int s0 = 0; s0 < S; s0 += RCH) {
            const int cnt = min(RCH, S - s0);
            for (int k = lane; k < cnt; k += 64) {
                const double x = lp[1 + H + s0 + k];
                const unsigned mk = masks[s0 + k];
                const double q = exp(x - l);
                wq[k] = q;
                wk[k] = (uint16_t)mk;
                const double e = (x - ppil * (double)__builtin_popcount(mk)) / ecoef;
                en = q == 0.0 ? en : fma(q, e, en);
            }
            pm_wave_lds_sync();
            for (int k = 0; k < cnt; ++k) {
                const unsigned mk = wk[k];
                const double q = wq[k];
                a0 += (mk & pm0) == pm0 ? q : 0.0;
                a1 += (mk & pm1) == pm1 ? q : 0.0;
                am += (mk & cm) == cm ? q : 0.0;
            }
            pm_wave_lds_sync();
        }
        if (lane < npair) q2[n * ldq + lane] = a0;
        if (lane + 64 < npair) q2[n * ldq + lane + 64] = a1;
        if (lane < Hp) {
            wm[lane] = am;
            wc[lane] = cand[n * Hp + lane];
        }
        pm_wave_lds_sync();
        for (int h = lane; h < H; h += 64) {
            const double x = lp[1 + h], q = exp(x - l);
            const double e = (x - ppil) / ecoef;
            en = q == 0.0 ? en : fma(q, e, en);
            double add = 0.0;
            for (int i = 0; i < Hp; ++i) add = wc[i] == h ? wm[i] : add;
            es[n * lde + h] = q + add;
        }
        en = pm_wave_sum(en);
        if (lane == 0) energy[n] = en;
        pm_wave_lds_sync();  // wm / wc are rewritten for the next row
    }
}

// ---------------------------------------------------------------------------------------------
// colsum: out[c] = sum_n X[n, c].  Workgroup b adds the rows [b rpb, (b + 1) rpb) in ascending order, one thread per column;
// the partials are added in ascending b.  rpb is a function of N alone.
// ---------------------------------------------------------------------------------------------
int64_t cs_blocks(int64_t N, int64_t *rows_per_block) {
    if (N <= 0) {
        *rows_per_block = 0;
        return 0;
    }
    int64_t nb = (N + CS_MIN_ROWS - 1) / CS_MIN_ROWS;
    if (nb > CS_MAX_BLOCKS) nb = CS_MAX_BLOCKS;
    const int64_t rpb = (N + nb - 1) / nb;
    *rows_per_block = rpb;
    return (N + rpb - 1) / rpb;
}

__global__ __launch_bounds__(256) void colsum_part_kernel(const double *__restrict__ X, int64_t ld, int64_t N, int C,
                                                          int64_t rpb, double *__restrict__ work) {
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = r0 + rpb < N ? r0 + rpb : N;
    for (int c = blockIdx.y * 256 + threadIdx.x; c < C; c += 256 * gridDim.y) {
        double acc = 0.0;
        for (int64_t n = r0; n < r1; ++n) acc += X[n * ld + c];
        work[(int64_t)blockIdx.x * C + c] = acc;
    }
}

__global__ __launch_bounds__(256) void colsum_total_kernel(const double *__restrict__ work, int64_t nb, int C,
                                                           double *__restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double acc = 0.0;
    for (int64_t b = 0; b < nb; ++b) acc += work[b * C + c];
    out[c] = acc;
}

// ---------------------------------------------------------------------------------------------
// pairs: a workgroup owns the LDS tile (64 dimensions) x (hb latent rows h0 ..) x (H columns) of A, laid out
// [row][column][dimension] so that the 64 lanes of an update -- one per dimension -- hit 64 consecutive doubles.  Every
// wavefront walks the flat (row n, pair p) list in ascending order, 64 entries per trip; an entry with candidates (lo, hi)
// touches cell [lo][hi] and, mirrored, cell [hi][lo] -- each where the cell's row is in the tile and the cell's column
// belongs to this wavefront (column % 16): a cell is always updated by the same wavefront, in ascending n, with a plain LDS
// read-modify-write in which lane dd adds q2 when m[n, d0 + dd] is set.  The upper cells of a trip go first, then the
// lower ones: the two sets are disjoint, so each cell still sees its rows in ascending order.  The tile is stored once,
// the diagonal taken from diag[h, d] = (E[s]^T Mf)[h, d].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * PWV) void mtrain_pairs_kernel(const int32_t *__restrict__ cand,
                                                                const double *__restrict__ q2, int64_t ldq,
                                                                const uint8_t *__restrict__ mask, int64_t ldm,
                                                                const double *__restrict__ diag, int64_t ldd, int N, int D,
                                                                int H, int Hp, int HB, int nblk, double *__restrict__ A) {
    extern __shared__ __attribute__((aligned(16))) double tile[];      // hb * H * PDS
    __shared__ uint8_t s_pi[128], s_pj[128];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slab = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const int d0 = slab * PDS, h0 = blk * HB;
    const int hb = min(HB, H - h0);
    const int cells = hb * H;
    for (int i = tid; i < cells * PDS; i += 64 * PWV) tile[i] = 0.0;
    const int npair = Hp * (Hp - 1) / 2;
    if (tid == 0) {
        int p = 0;
        for (int i = 0; i < Hp; ++i)
            for (int j = i + 1; j < Hp; ++j, ++p) {
                s_pi[p] = (uint8_t)i;
                s_pj[p] = (uint8_t)j;
            }
    }
    __syncthreads();

    const int d = d0 + lane;
    const bool dval = d < D;
    const int64_t total = (int64_t)N * npair;
    // this lane's entry of the current trip: flat index f = n npair + p, advanced by 64 per trip
    int n = npair ? lane / npair : 0, p = npair ? lane % npair : 0;
    const int dn = npair ? 64 / npair : 0, dp = npair ? 64 % npair : 0;
    for (int64_t f0 = 0; f0 < total; f0 += 64) {
        int cu = -1, cl = -1;      // upper / lower cell of this lane's entry that this wavefront updates here, or -1
        double q = 0.0;
        if (f0 + lane < total) {
            const int ci = cand[(int64_t)n * Hp + s_pi[p]], cj = cand[(int64_t)n * Hp + s_pj[p]];
            const int lo = min(ci, cj), hi = max(ci, cj);
            if (lo >= 0 && hi < H && lo != hi) {
                if (lo >= h0 && lo < h0 + hb && (hi % PWV) == wave) cu = (lo - h0) * H + hi;
                if (hi >= h0 && hi < h0 + hb && (lo % PWV) == wave) cl = (hi - h0) * H + lo;
                if (cu >= 0 || cl >= 0) q = q2[(int64_t)n * ldq + p];
            }
        }
        unsigned long long mu = __ballot(cu >= 0), ml = __ballot(cl >= 0);
        while (mu) {
            const int src = __builtin_ctzll(mu);
            mu &= mu - 1;
            const int nn = __shfl(n, src, 64), cell = __shfl(cu, src, 64);
            const double qq = __shfl(q, src, 64);
            if (dval && mask[(int64_t)nn * ldm + d] != 0) tile[cell * PDS + lane] += qq;
        }
        while (ml) {
            const int src = __builtin_ctzll(ml);
            ml &= ml - 1;
            const int nn = __shfl(n, src, 64), cell = __shfl(cl, src, 64);
            const double qq = __shfl(q, src, 64);
            if (dval && mask[(int64_t)nn * ldm + d] != 0) tile[cell * PDS + lane] += qq;
        }
        n += dn;
        p += dp;
        if (p >= npair) {
            p -= npair;
            ++n;
        }
    }
    __syncthreads();
    // store: columns fastest (coalesced rows of A_d)
    const int nd = min(PDS, D - d0);
    for (int i = tid; i < cells * nd; i += 64 * PWV) {
        const int c = i % H, r = (i / H) % hb, dd = i / cells;
        double v = tile[(r * H + c) * PDS + dd];
        if (c == h0 + r) v = diag[(int64_t)c * ldd + d0 + dd];
        A[((int64_t)(d0 + dd) * H + h0 + r) * H + c] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// solve: one workgroup per dimension.  x0 = Ainv r, x = x0 + Ainv (r - A x0); thread i forms element i of every product
// in ascending j (A and Ainv are symmetric: column reads, coalesced over i).  The pivot rule is _solve_ok's.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mtrain_solve_kernel(const double *__restrict__ A, const double *__restrict__ Ainv,
                                                           const double *__restrict__ pivots, const double *__restrict__ r,
                                                           int64_t ldr, const double *__restrict__ Wold, int64_t ldw, int H,
                                                           double *__restrict__ Wnew, int64_t ldo,
                                                           int32_t *__restrict__ status) {
    __shared__ double s_v[MT_MAX_H], s_x[MT_MAX_H];
    const int d = blockIdx.x, i = threadIdx.x;
    const double pmin = pivots[2 * (int64_t)d], pmax = pivots[2 * (int64_t)d + 1];
    const double ratio = pmax != 0.0 ? pmin / pmax : 0.0;
    const bool ok = pmin > 0.0 && isfinite(ratio) && ratio > 1e-11;
    if (!ok) {      // (uniform over the workgroup)
        if (i < H) Wnew[(int64_t)i * ldo + d] = Wold[(int64_t)i * ldw + d];
        if (i == 0) status[d] = 0;
        return;
    }
    const double *Ad = A + (int64_t)d * H * H, *Id = Ainv + (int64_t)d * H * H;
    const double rd = i < H ? r[(int64_t)i * ldr + d] : 0.0;
    s_v[i] = rd;
    __syncthreads();
    double x0 = 0.0;
    if (i < H)
        for (int j = 0; j < H; ++j) x0 = fma(Id[(int64_t)j * H + i], s_v[j], x0);
    s_x[i] = x0;
    __syncthreads();
    double t = 0.0;
    if (i < H)
        for (int j = 0; j < H; ++j) t = fma(Ad[(int64_t)j * H + i], s_x[j], t);
    s_v[i] = rd - t;
    __syncthreads();
    double y = 0.0;
    if (i < H)
        for (int j = 0; j < H; ++j) y = fma(Id[(int64_t)j * H + i], s_v[j], y);
    if (i < H) Wnew[(int64_t)i * ldo + d] = x0 + y;
    if (i == 0) status[d] = 1;
}

int pairs_tile_rows(int64_t H) {
    int64_t hb = PCELLS / H;
    if (hb < 1) hb = 1;
    if (hb > H) hb = H;
    return (int)hb;
}

}  // namespace

extern "C" int pm_bsc_mtrain_rows_f64(const double *logpj, int64_t ldl, const double *lse, const int32_t *cand,
                                      const uint16_t *state_masks, int64_t S, const pm_bsc_estep_params *params_host,
                                      int64_t N, int64_t H, int64_t Hprime, double *es, int64_t lde, double *q2,
                                      int64_t ldq, double *energy, void *stream) {
    if (!logpj || !lse || !cand || !params_host || !es || !energy || N < 0 || H <= 0 || Hprime <= 0 || S < 0 ||
        ldl < 1 + H + S || lde < H || (S > 0 && !state_masks))
        return PM_EINVAL;
    if (H > PM_MAX_H || Hprime > PM_MAX_HPRIME || Hprime > H || S > 65535) return PM_ERANGE;
    const int64_t npair = Hprime * (Hprime - 1) / 2;
    if (npair > 0 && (!q2 || ldq < npair)) return PM_EINVAL;
    if (!(params_host->ecoef < 0.0)) return PM_EINVAL;      // (the energies are recovered by dividing by it)
    if (N == 0) return PM_OK;
    hipLaunchKernelGGL(mtrain_rows_kernel, dim3((unsigned)pm_row_grid(N, RW)), dim3(64 * RW), 0,
                       static_cast<hipStream_t>(stream), logpj, ldl, lse, cand, state_masks, (int)S,
                       params_host->prior_scale * params_host->pil_bar, params_host->ecoef, N, (int)H, (int)Hprime, es, lde,
                       q2, ldq, energy);
    return (int)hipGetLastError();
}

extern "C" int64_t pm_col_sum_ordered_work_len(int64_t N, int64_t C) {
    if (N < 0 || C < 1) return -1;
    int64_t rpb;
    const int64_t nb = cs_blocks(N, &rpb);
    return (nb > 0 ? nb : 1) * C;
}

extern "C" int pm_col_sum_ordered_f64(const double *X, int64_t ld, int64_t N, int64_t C, double *work, double *out,
                                      void *stream) {
    if (!X || !work || !out || N < 0 || C < 1 || ld < C) return PM_EINVAL;
    if (C > INT32_MAX) return PM_ERANGE;
    if (N == 0) return PM_OK;
    int64_t rpb;
    const int64_t nb = cs_blocks(N, &rpb);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t gy = (C + 255) / 256;
    if (gy > 64) gy = 64;
    hipLaunchKernelGGL(colsum_part_kernel, dim3((unsigned)nb, (unsigned)gy), dim3(256), 0, st, X, ld, N, (int)C, rpb, work);
    if (int e = (int)hipGetLastError()) return e;
    hipLaunchKernelGGL(colsum_total_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, work, nb, (int)C, out);
    return (int)hipGetLastError();
}

extern "C" int pm_bsc_mtrain_pairs_f64(const int32_t *cand, const double *q2, int64_t ldq, const uint8_t *mask, int64_t ldm,
                                       const double *diag, int64_t ldd, int64_t N, int64_t D, int64_t H, int64_t Hprime,
                                       double *A, void *stream) {
    if (!cand || !mask || !diag || !A || N < 0 || D <= 0 || H <= 0 || Hprime <= 0 || ldm < D || ldd < D) return PM_EINVAL;
    if (H > MT_MAX_H || Hprime > PM_MAX_HPRIME || Hprime > H || D > MT_MAX_CELLS || D * H * H > MT_MAX_CELLS ||
        N > INT32_MAX)
        return PM_ERANGE;
    const int64_t npair = Hprime * (Hprime - 1) / 2;
    if (npair > 0 && (!q2 || ldq < npair)) return PM_EINVAL;
    if (N == 0) return PM_OK;
    const int HB = pairs_tile_rows(H);
    const int64_t nblk = (H + HB - 1) / HB, slabs = (D + PDS - 1) / PDS;
    const size_t shmem = sizeof(double) * (size_t)HB * H * PDS;
    if (shmem > 48 * 1024) {
        if (int e = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(mtrain_pairs_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem))
            return e;
    }
    hipLaunchKernelGGL(mtrain_pairs_kernel, dim3((unsigned)(slabs * nblk)), dim3(64 * PWV), shmem,
                       static_cast<hipStream_t>(stream), cand, q2, ldq, mask, ldm, diag, ldd, (int)N, (int)D, (int)H,
                       (int)Hprime, HB, (int)nblk, A);
    return (int)hipGetLastError();
}

extern "C" int64_t pm_bsc_mtrain_pairs_tile_rows(int64_t H) {
    if (H < 1 || H > MT_MAX_H) return -1;
    return pairs_tile_rows(H);
}

extern "C" int pm_bsc_mtrain_solve_f64(const double *A, const double *Ainv, const double *pivots, const double *r,
                                       int64_t ldr, const double *Wt_old, int64_t ldw, int64_t D, int64_t H, double *Wt_new,
                                       int64_t ldo, int32_t *status, void *stream) {
    if (!A || !Ainv || !pivots || !r || !Wt_old || !Wt_new || !status || D <= 0 || H <= 0 || ldr < D || ldw < D || ldo < D)
        return PM_EINVAL;
    if (H > MT_MAX_H || D > MT_MAX_CELLS || D * H * H > MT_MAX_CELLS) return PM_ERANGE;
    hipLaunchKernelGGL(mtrain_solve_kernel, dim3((unsigned)D), dim3(256), 0, static_cast<hipStream_t>(stream), A, Ainv,
                       pivots, r, ldr, Wt_old, ldw, (int)H, Wt_new, ldo, status);
    return (int)hipGetLastError();
}

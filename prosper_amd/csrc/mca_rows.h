// What the MCA / MMCA row kernels of mca_kernels.hip and masked_kernels.hip must agree on bit for bit, written once:
// the tail of an E-step row (column order of the log-joints, the row maximum, the two log-evidences with their -745
// guard), the end of a statistics kernel, and on the host the wavefronts per workgroup (the row grid is
// pm_row_grid of pm_common.h).
// mca_estep_kernel and mca_masked_estep_kernel differ in the energies (the mask) and in whose |W_h|^2 a row reads.
#ifndef PM_MCA_ROWS_H
#define PM_MCA_ROWS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "prosper_hip.h"
#include "pm_common.h"

// The two routines are function-like macros: as __forceinline__ functions they change the instruction streams of their
// kernels.  Each is one statement; the including unit #undef's them at its end.

// Tail of one E-step row, by the row's wavefront: log-pseudo-joints out in the column order [ null | H singletons | S
// states ] and the two log-evidences (beta = 1 for Q, beta = 1 / T for the weights).  s_e: the states' energies in, their
// log-joints out.  w2: |W_h|^2 of this row (the masked kernel's are per row).  Terms below e^-745 of the largest are
// exact zeros in f64 and are not evaluated.
// From the caller: lane, P (pm_mca_params), H, S, masks, s_e.
#define MCA_ROW_TAIL(w2, yn, arow, out, lse1_n, lseb_n)                                                                \
    do {                                                                                                               \
        double m1 = -INFINITY;                                                                                         \
        if (lane == 0) {                                                                                               \
            const double f0 = P.pre1 * yn;                                                                             \
            out[0] = f0;                                                                                               \
            m1 = f0;                                                                                                   \
        }                                                                                                              \
        for (int h = lane; h < H; h += 64) {                                                                           \
            const double f = P.pil_bar + P.pre1 * ((w2)[h] - 2.0 * arow[h] + yn);                                      \
            out[1 + h] = f;                                                                                            \
            m1 = fmax(m1, f);                                                                                          \
        }                                                                                                              \
        for (int s = lane; s < S; s += 64) {                                                                           \
            const double f = P.pil_bar * (double)__builtin_popcount((unsigned)masks[s]) + P.pre1 * s_e[s];             \
            out[1 + H + s] = f;                                                                                        \
            s_e[s] = f;                                                                                                \
            m1 = fmax(m1, f);                                                                                          \
        }                                                                                                              \
        m1 = pm_wave_max(m1);                                                                                          \
        double s1 = 0.0, sb = 0.0;                                                                                     \
        if (lane == 0) {                                                                                               \
            const double dlt = out[0] - m1; /* own store, same lane */                                                 \
            s1 += exp(dlt);                                                                                            \
            sb += exp(P.beta * dlt);                                                                                   \
        }                                                                                                              \
        for (int h = lane; h < H; h += 64) {                                                                           \
            const double dlt = (P.pil_bar + P.pre1 * ((w2)[h] - 2.0 * arow[h] + yn)) - m1;                             \
            if (dlt > -745.0) {                                                                                        \
                s1 += exp(dlt);                                                                                        \
                sb += exp(P.beta * dlt);                                                                               \
            }                                                                                                          \
        }                                                                                                              \
        for (int s = lane; s < S; s += 64) {                                                                           \
            const double dlt = s_e[s] - m1;                                                                            \
            if (dlt > -745.0) {                                                                                        \
                s1 += exp(dlt);                                                                                        \
                sb += exp(P.beta * dlt);                                                                               \
            }                                                                                                          \
        }                                                                                                              \
        s1 = pm_wave_sum(s1);                                                                                          \
        sb = pm_wave_sum(sb);                                                                                          \
        if (lane == 0) {                                                                                               \
            lse1_n = m1 + log(s1);                                                                                     \
            lseb_n = P.beta * m1 + log(sb);                                                                            \
        }                                                                                                              \
    } while (0)

// End of a statistics kernel (mca_mstep_rows_kernel, mca_estep_fused_body): the wavefronts' four scalars through s_red
// into stats' [ pi | sum q e | sum lse | count ] (quantised, PM_Q), then the workgroup's q1sum (H).  Every thread of the
// workgroup reaches it.
// From the caller: st_pi, st_sigma, st_ld, st_cnt, tid, lane, wave, waves, s_red, s_q1sum, stats, H, D.
#define MCA_STATS_EPILOGUE()                                                                                           \
    do {                                                                                                               \
        st_pi = pm_wave_sum(st_pi);                                                                                    \
        st_sigma = pm_wave_sum(st_sigma);                                                                              \
        st_ld = pm_wave_sum(st_ld);                                                                                    \
        st_cnt = pm_wave_sum(st_cnt);                                                                                  \
        if (lane == 0) {                                                                                               \
            s_red[wave * 4 + 0] = st_pi;                                                                               \
            s_red[wave * 4 + 1] = st_sigma;                                                                            \
            s_red[wave * 4 + 2] = st_ld;                                                                               \
            s_red[wave * 4 + 3] = st_cnt;                                                                              \
        }                                                                                                              \
        __syncthreads();                                                                                               \
        double *g_q1sum = stats + 3 * (int64_t)H * D;                                                                  \
        double *sc = g_q1sum + H;                                                                                      \
        if (tid < 4) {                                                                                                 \
            double v = 0.0;                                                                                            \
            for (int w = 0; w < waves; ++w) v += s_red[w * 4 + tid];                                                   \
            if (v != 0.0) pm_atomic_add(sc + tid, PM_Q(v, tid == 1 ? 3 : tid == 2 ? 4 : 2));                           \
        }                                                                                                              \
        for (int h = tid; h < H; h += blockDim.x) {                                                                    \
            const double v = s_q1sum[h];                                                                               \
            if (v != 0.0) pm_atomic_add(g_q1sum + h, v);                                                               \
        }                                                                                                              \
    } while (0)

// wavefronts per workgroup so that the per-wave LDS areas fit ~64 KB
inline int mca_pick_waves(size_t per_wave_bytes, size_t shared_bytes) {
    int w = 4;
    while (w > 1 && shared_bytes + w * per_wave_bytes > 64 * 1024) w >>= 1;
    return w;
}

#endif  // PM_MCA_ROWS_H

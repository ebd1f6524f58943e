// Launch decisions of the Binary Sparse Coding kernels as host-only functions, one per translation unit that owns a kernel
// family.  The launchers switch on these structs and pm_bsc_plan (bsc_kernels.hip) exports them, so the query cannot drift
// from the dispatch.  None of them makes a device call, except that pm_bsc::plan_fused8 asks the current device for its
// compute units when `cus` <= 0.
#ifndef PM_BSC_PLAN_H
#define PM_BSC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "prosper_hip.h"

namespace pm_bsc {

struct Plan {
    int family = 0;                    // PM_BSC_FAMILY_*
    int vpl = 0, nj = 0;               // latents per lane (SELECT, sixteen-lane kernels); 16-latent blocks per wavefront (fused)
    int hp = 0, gamma = 0;             // FUSED8: the <HP, GAMMA> instantiation
    int full = 0, mstats = 0;          // template flags (FUSED, FUSED8); SELECT_ESTEP: ESTEP; MSTEP_ROWS16: NZ
    size_t lds = 0, lds_tail = 0;      // dynamic shared memory (FUSED8: main launch, TAIL launch)
    int64_t grid = 0;                  // workgroups (FUSED8: of the main launch)
    int64_t main_rows = 0, tail_rows = 0, tail_grid = 0;   // FUSED8: the split of the shard
};

#define PM_BSC_HIDDEN __attribute__((visibility("hidden")))

// pm_bsc_select_f64, pm_bsc_estep_f64, pm_bsc_mstep_rows_f64 (bsc_kernels.hip).  pair_len: entries of the pair lists
// (MSTEP_ROWS only).
PM_BSC_HIDDEN int plan_wave(int which, int64_t H, int64_t Hprime, int64_t S, int64_t pair_len, int64_t N, Plan *p);
// pm_bsc_select_estep_f64, pm_bsc_mstep_rows16_f64 / _nz_f64 (bsc_rows16.hip)
PM_BSC_HIDDEN int plan_rows16(int which, int64_t H, int64_t Hprime, int64_t S, int flags, int64_t N, Plan *p);
// pm_bsc_estep_fused_f64 (bsc_fused.hip)
PM_BSC_HIDDEN int plan_fused(int64_t H, int64_t D, int64_t Hprime, int64_t S, int flags, int64_t N, Plan *p);
// pm_bsc_estep_fused8_f64 / _nz_f64 / _defer_f64 (bsc_fused8.hip)
PM_BSC_HIDDEN int plan_fused8(int64_t H, int64_t D, int64_t Hprime, int64_t S, int64_t gamma, int flags, int64_t N, int cus,
                              Plan *p);

}  // namespace pm_bsc

#endif

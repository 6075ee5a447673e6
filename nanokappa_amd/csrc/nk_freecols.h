// nk_freecols.h -- free-path sampling with K lifetime columns (nk_free_paths_columns): what the kernel k_free_columns<GEOM, KT>
// (nk_freecols.hip, a translation unit of its own like nk_freepath.hip) is handed, and its launch.  The C entry points are in
// nk_engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nk_freepath.h"

#define NK_FC_TILE 8             // columns one launch weighs per cast; a call with more is flown in tiles of this many
// a lane's sums between two of its rays, per column (only when n > 64: a lane then flies more than one ray): the ten doubles that
// are added once per ray (D[3], D^2[3], T, p_res, p_wall, w_left) and the three counts (casts, missed, capped) as 64-bit words
#define NK_FC_ACC 13
// workgroups of a launch with n > 64: its waves walk the list with this stride, so the scratch area of the lane sums stays bounded
#define NK_FC_MAX_WGS 1024

// Everything is a device pointer.  `f` is the single call's record with a leading column axis on what a column owns:
// f.tau [K][M], f.rows [K][nlist * NK_FP_ROW], f.counts [K][nlist * NK_FP_CNT], f.ray_D / ray_T / ray_seg / ray_end [K][rays ..];
// f.ray_x0 [rays * 3] and f.x0 are the ray's.  A launch weighs the columns c0 .. c0 + kc - 1.
struct NkFreeColsDev {
    NkFreeDev f;
    int32_t c0, kc;              // first column and columns of this launch, 1 <= kc <= the instantiation's KT
    int32_t M;                   // modes of the material: the stride of f.tau
    int64_t rays;                // nlist * n: the stride of the per-ray outputs
    double *acc;                 // [waves of the grid][kc][NK_FC_ACC][64] lane sums between rays, or null when n <= 64
    unsigned long long *shared;  // [nlist] casts this launch made for the mode's rays
};

// the smallest instantiation (1, 4 or NK_FC_TILE columns in registers) that holds kc columns
static inline int nk_free_columns_tile(int kc) { return kc <= 1 ? 1 : kc <= 4 ? 4 : NK_FC_TILE; }
// workgroups of a launch: one wave per mode of the list, or NK_FC_MAX_WGS workgroups that stride over it when n > 64
static inline unsigned nk_free_columns_grid(int64_t nlist, int n) {
    const int64_t g = (nlist + NK_FP_WAVES - 1) / NK_FP_WAVES;
    return (unsigned)((n > 64 && g > NK_FC_MAX_WGS) ? NK_FC_MAX_WGS : g);
}
// geom and lds as nk_free_paths_launch; grid = nk_free_columns_grid (q.acc is sized by it)
hipError_t nk_free_columns_launch(const NkDev &d, const NkFreeColsDev &q, int geom, size_t lds, unsigned grid, hipStream_t stream);

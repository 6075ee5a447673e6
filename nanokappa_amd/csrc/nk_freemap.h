// nk_freemap.h -- free-path maps (nk_free_paths_map): what the kernel k_free_map<GEOM> (nk_freemap.hip, a translation unit of
// its own like nk_freepath.hip) is handed besides the single call's record, and its launch.  The C entry points are in
// nk_engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nk_freepath.h"

// words of a cell's line (NK_FREE_MAP_LINE = 16 of them, 128 bytes): N, the nine w_a D_b at 1 + 3 a + b, p_res, p_wall, w_left, T, -, -
enum { NK_FM_N = 0, NK_FM_K = 1, NK_FM_PRES = 10, NK_FM_PWALL = 11, NK_FM_WLEFT = 12, NK_FM_T = 13 };
// words of the header line (line `ncells` of the grid): rays whose start cell was clamped, terms left out above B_K, B_P, B_T
enum { NK_FM_CLAMPED = 0, NK_FM_OVK = 1, NK_FM_OVP = 2, NK_FM_OVT = 3 };

// Everything is a device pointer; the per-ray outputs may be null (ray r = list index * n + sample).
struct NkFreeMapDev {
    double lo[3], inv_h[3];      // the field's grid convention: cell = floor((x - lo) * inv_h) per axis, clamped
    int32_t n[3], ncells;
    const double *weight;        // [nlist * 3] the weight vector of every list entry
    double sK, sP, sT;           // 2^k_K, 2^k_P, 2^k_T
    double BK, BP, BT;           // bounds of |w_a D_b|, of a ray's final weight and of its flight time
    unsigned long long *grid;    // [(ncells + 1) * 16] zeroed by the host: the cells' lines and the header line
    int32_t *ray_cell;           // [rays] the (clamped) start cell
    double *ray_w;               // [rays] the weight that went to word 10, 11 or 12; 0 otherwise
};

// as nk_free_paths_launch (one wave per list entry, NK_FP_WAVES waves per workgroup)
hipError_t nk_free_map_launch(const NkDev &d, const NkFreeDev &f, const NkFreeMapDev &g, int geom, size_t lds, hipStream_t stream);

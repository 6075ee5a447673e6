// nk_freepath.h -- free-path sampling and free-path maps (nk_free_paths, nk_free_paths_map): what the kernel
// k_free_paths<GEOM, MAP> (nk_freepath.hip, a translation unit of its own like nk_modes.hip) is handed, and its launch.  The C
// entry points are in nk_engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct NkDev;

// RNG stream tags of the pass (the bases of nk_device.h go up to NK_TAG_INIT = 0x40000): + 0..2 the three draws of a start
// point (k_init_particles' rule with step 0), + 3 the draw of a rough reflection (step = the ray's hit count)
#define NK_TAG_FREE 0x50000u

#define NK_FP_WAVES 4            // waves per workgroup = modes per workgroup (NK_WG / 64)
// a mode's row of sums (doubles): D[3], D^2[3] (squares of the per-ray displacement), T, hits, p_res, p_wall, w_left, p_int
#define NK_FP_ROW 12
// a mode's row of counts (64-bit): casts, missed, capped, -
#define NK_FP_CNT 4

// Everything is a device pointer; the per-ray outputs may be null (ray r = list index * n + sample).
struct NkFreeDev {
    const int32_t *modes;        // [nlist] or null: list index = mode
    int32_t nlist, n, max_segments;
    double w_min;
    const double *tau;           // [M] lifetimes at the call's temperature
    const double *vg;            // [M * 3] group velocities (the material's)
    const double *x0;            // [nlist * n * 3] start points, or null: drawn (Mesh.sample_volume)
    uint64_t seed;
    double *rows;                // [nlist * NK_FP_ROW]
    unsigned long long *counts;  // [nlist * NK_FP_CNT]
    double *ray_D, *ray_T, *ray_x0;   // [rays * 3], [rays], [rays * 3]
    int32_t *ray_seg, *ray_end;       // [rays] casts of the ray, its end code
};

// A map call's grid (nk_free_paths_map): every finished ray is binned by the cell of its start point.
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

// one wave per entry of the list, NK_FP_WAVES waves per workgroup; geom = 1 (planes in LDS) or 2 (tables in global memory, tree
// walk), lds = what nk_lds_setup of that geometry mode and kind 0 needs; map: a map call's grid, or null for the plain call
hipError_t nk_free_paths_launch(const NkDev &d, const NkFreeDev &f, const NkFreeMapDev *map, int geom, size_t lds, hipStream_t stream);

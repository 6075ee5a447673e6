// nk_freepath.h -- free-path sampling (nk_free_paths): what the kernel k_free_paths<GEOM> (nk_freepath.hip, a translation
// unit of its own like nk_modes.hip) is handed, and its launch.  The C entry points are in nk_engine.hip.
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

// one wave per mode of the list; geom = 1 (planes in LDS) or 2 (tables in global memory, tree walk), lds = what nk_lds_setup of
// that geometry mode and kind 0 needs
hipError_t nk_free_paths_launch(const NkDev &d, const NkFreeDev &f, int geom, size_t lds, hipStream_t stream);

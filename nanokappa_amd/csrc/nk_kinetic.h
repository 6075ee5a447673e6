// nk_kinetic.h -- kinetic flights (nk_kinetic_flights, nk_kinetic_flights_groups, nk_kinetic_flights_map): what the kernel
// k_kinetic<GEOM, BINS, GROUPED, MAP> (nk_kinetic.hip, a translation unit of its own like nk_freepath.hip) is handed, and its launch.  The C entry points are in
// nk_engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct NkDev;

// RNG stream tags of the pass (nk_freepath.h's NK_TAG_FREE is 0x50000).  Every draw is nk_uniform2_dev(seed, ray id, k, tag) with
// k = the ray's event count when the draw is made, and (a, b) the pair it returns:
//   + 0        k = 0: a picks the triangle of the source facet (nk_ss_right on its cumulative areas), sqrt(b) its first weight
//   + 1        k = 0: a the second barycentric draw (Mesh.sample_surface's rule, as nk_sample_res_face)
//   + 2        a segment, k = events so far: a the free time t_s = -tau ln(a) (a = 0 is taken as 2^-54), b the point on the segment
//   + 3        an intrinsic scattering, k = the event's number (counted from 1): a draws the new mode from cdf_scatter
//   + 64 + j   trial j < 64 of an emission (k = 0) or a diffuse re-emission (k = the event's number): a draws the mode from
//              cdf_flux, accepted iff b |v| < (v . n_in)+
// A rough facet's specular test is nk_fl_facet's, unchanged: nk_uniform2_dev(seed, ray id, k, NK_TAG_FREE + 3), k = the event's number.
#define NK_TAG_KIN 0x60000u
#define NK_KIN_TRIALS 64

#define NK_KIN_WAVES 4           // waves per workgroup (NK_WG / 64)
#define NK_KIN_MAX_SOURCES_DEV 8 // NK_KIN_MAX_SOURCES of the public header
// a source's row of 64-bit words: ends[8], lost, missed, capped, events, casts, D[3] 2^k_D, D^2[3] 2^k_D2, dwell 2^k_T, then the
// terms left out above their bounds: of D, of D^2, of the dwell (per ray), of a segment's time and of its displacement (per segment),
// then the segment points clamped into the map's edge cells (map calls only; 0 otherwise)
enum { NK_KR_ENDS = 0, NK_KR_LOST = 8, NK_KR_MISSED = 9, NK_KR_CAPPED = 10, NK_KR_EVENTS = 11, NK_KR_CASTS = 12, NK_KR_D = 13,
       NK_KR_D2 = 16, NK_KR_T = 19, NK_KR_OVD = 20, NK_KR_OVD2 = 21, NK_KR_OVT = 22, NK_KR_OVST = 23, NK_KR_OVSX = 24, NK_KR_CLAMPED = 25, NK_KIN_ROW = 32 };
// a ray's end code: >= 0 the source index of the reservoir that absorbed it
#define NK_KIN_LOST (-1)
#define NK_KIN_MISSED (-2)
#define NK_KIN_CAPPED (-3)

// Everything is a device pointer; the per-ray outputs may be null (ray r = source index * n + sample).
struct NkKinDev {
    int32_t nsrc, n, max_events, rays_per_wave, blocks;   // blocks = ceil(n / rays_per_wave): waves per source
    int32_t src_facet[NK_KIN_MAX_SOURCES_DEV];            // the 'T' facets in ascending order
    int32_t M, bins_off;                                  // bins_off: byte offset of the LDS bins in the dynamic area (BINS)
    const double *tau, *vg;                               // [M], [M * 3]
    const double *cdf_scatter, *cdf_flux;                 // [M]
    uint64_t seed;
    double sD, sD2, sT, BD, BD2, BT;                      // per ray: 2^k and the bounds of |D_a|, D_a^2 and the dwell
    double st, sx, Bt, Bx;                                // per segment: 2^k and the bounds of t and |t v_a|
    unsigned long long *rows;                             // [nsrc * NK_KIN_ROW] zeroed by the host
    unsigned long long *sub;                              // [nsrc * S * 4] {dwell, t v_x, t v_y, t v_z}, zeroed by the host
    double *ray_x0, *ray_D, *ray_T;                       // [rays * 3], [rays * 3], [rays]
    int32_t *ray_mode, *ray_end, *ray_events, *ray_casts; // [rays]
    unsigned long long *ray_hash;                         // [rays]
    // kinetic groups (GROUPED; GC = 0 and both pointers null otherwise): a segment's four words go to (source, subvolume, column
    // of the mode it was flown in) and `sub` is folded from the columns afterwards (k_kinetic_fold)
    const int32_t *group;                                 // [M] the column of every mode, 0 .. GC-1
    int32_t GC, pad_;                                     // columns: the call's groups and the rest column
    unsigned long long *grp;                              // [nsrc * S * GC * 4], zeroed by the host
    // kinetic maps (MAP; map null otherwise): a segment's four words also go to the line of (source, cell of x_p) on the field's
    // grid, cell = floor((x - lo) * inv_h) per axis, clamped; cell order (ix * ny + iy) * nz + iz
    int32_t gn[3], ncells;
    double lo[3], inv_h[3];
    unsigned long long *map;                              // [nsrc * ncells * 4], zeroed by the host
};

// one wave per (source, block of rays_per_wave rays); geom = 1 (planes in LDS) or 2 (tables in global memory, tree walk); lds = what
// nk_lds_setup of that geometry mode and kind 0 needs; bins: the per-subvolume words are gathered in LDS (f.bins_off, nsrc * S * 4
// words behind lds, times GC where f.GC > 0) before they go to memory.  f.GC > 0 picks the GROUPED instantiations and launches
// k_kinetic_fold behind them on the same stream; f.map != nullptr picks the MAP instantiations (never together with f.GC > 0)
hipError_t nk_kinetic_launch(const NkDev &d, const NkKinDev &f, int geom, size_t lds, bool bins, hipStream_t stream);

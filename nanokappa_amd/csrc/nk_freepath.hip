// nk_freepath.hip -- free-path sampling of the geometry-limited conductivity (nk_free_paths) and free-path maps (nk_free_paths_map):
// k_free_paths<GEOM, MAP> and its launch.  The C entry points (nk_free_paths, nk_free_paths_map and their _info) are in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds
// the four instantiations of k_free_paths and nothing else (the trick of nk_modes.hip).
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_freepath.h"
#include "nk_flight.h"

// =================================================================================== the rule
// For every mode m of the list n rays (DESIGN.md "Free-path sampling"); ray id = (m << 32) | sample, Philox key = the call's seed.
//   start   x = the caller's x0, or one draw of Mesh.sample_volume as k_init_particles makes it (three nk_uniform2_dev with step
//           0 and tags NK_TAG_FREE + 0..2);  W = 1, k = 0, v and tau of m.
//   repeat  cast from x along v (the general cast of the geometry mode: LDS planes or the tree);
//           a miss: g = 1, the segment is added, the ray ends (code 3, counted in `missed`);
//           a hit after tc: a = tc / tau, g = -expm1(-a), e = exp(-a);  D += W tau g v, T += W tau g, p_int += W g;  W *= e;
//           k += 1; hits += W;  then by the facet's boundary condition
//             'T' / 'F'  p_res += W, end (code 1)
//             'P'        x = hit point + the facet's translation (nk_event_pre), go on
//             'R'        (r0, r1) = nk_uniform2_dev(seed, ray id, k, NK_TAG_FREE + 3); specular iff true_spec && r0 <= specularity
//                        (nk_reflect's test; and the specular map names a mode): go on from the hit point in mode spec_map, its
//                        degenerate partner when degen_j2 names one and r1 >= 0.5; else diffuse: p_wall += W, end (code 2)
//           going on: W < w_min -> w_left += W, end (code 0);  k >= max_segments -> w_left += W, end (code 4, `capped`).
//   A mode that does not fly (v = 0) or does not live (tau <= 0) takes no cast: p_int += W, T += W max(tau, 0), end (code 0).
// Per mode: the sums over its rays of D, D^2 (per ray), T, hits, p_res, p_wall, w_left, p_int;  p_res + p_wall + w_left + p_int = n.
// One wave per mode of the list, lanes are samples: lane l takes samples l, l + 64, ... in ascending order and adds them up in
// that order; the 64 lane sums are combined by a butterfly (xor 32, 16, .., 1) and lane 0 stores the row.  No atomics: a row's
// bits depend on the mode, n and the seed (or x0) alone, not on the grid nor on the other modes of the list.  The statements of
// the flight and their roundings are nk_flight.h's; the facet step alone is written out in the kernel.
// The map (MAP; DESIGN.md "Free-path maps"): once per finished ray, by the lane that flew it, into the line of the ray's START cell
// -- the field's cell rule, i_a = floor((x_a - lo_a) * (1 / h_a)), an index outside [0, n_a) or a NaN clamped into the edge cell
// and counted.  A line is 16 unsigned 64-bit words {N, w_a D_b at 1 + 3 a + b, p_res, p_wall, w_left, T, 0, 0}; w is the weight
// vector of the ray's LIST ENTRY (also after reflections into other modes), D the ray's displacement; words 10 .. 12 take the
// ray's final weight W by its end (reservoir, diffuse wall, w_min cut or cap; a miss, a reflection into a dead mode and a no-cast
// ray add nothing).  Every real term is multiplied by a power of two (sK, sP, sT: the host's 2^k), rounded to nearest even
// (rint) and added as an integer in two's complement with atomicAdd(unsigned long long) on global memory; an exact zero is not
// added.  No floating-point atomics, no compare-and-swap loops: the integers are the same bits in any order of the rays.  A
// term above its bound (B_K, B_P, B_T) is left out and counted in the header line; the host reports it.  The rows and the per-ray
// outputs of a map call are the plain call's bit for bit: the same statements.

// one term into one word: rint(term s) as a two's-complement integer; above the bound (or a NaN) it is left out and counted
__device__ __forceinline__ void nk_fm_add(unsigned long long *w, double term, double s, double B, unsigned int &over) {
#pragma clang fp contract(off)
    if (!(fabs(term) <= B)) { over += 1u; return; }
    const long long q = (long long)rint(term * s);
    if (q != 0) atomicAdd(w, (unsigned long long)q);
}

// a finished ray into the line of its start cell; returns the weight routed to word 10, 11 or 12 (0 where none is)
__device__ __forceinline__ double nk_fm_bin(const NkFreeMapDev &g, int cell, const NkFlRay &c, double wx, double wy, double wz,
                                            unsigned int &ovK, unsigned int &ovP, unsigned int &ovT) {
#pragma clang fp contract(off)
    unsigned long long *w = g.grid + (size_t)cell * NK_FREE_MAP_LINE;          // cell < ncells <= 2^24
    atomicAdd(w + NK_FM_N, 1ull);
    const double wa[3] = {wx, wy, wz}, Db[3] = {c.Dx, c.Dy, c.Dz};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double term = wa[a] * Db[b];
            nk_fm_add(w + NK_FM_K + 3 * a + b, term, g.sK, g.BK, ovK);
        }
    double routed = 0.0;
    int word = -1;
    if (c.end == 1) word = NK_FM_PRES;
    else if (c.end == 2) word = NK_FM_PWALL;
    else if (c.end == 4 || c.end == NK_FL_END_WMIN) word = NK_FM_WLEFT;
    if (word >= 0) {
        routed = c.W;
        nk_fm_add(w + word, c.W, g.sP, g.BP, ovP);
    }
    nk_fm_add(w + NK_FM_T, c.T, g.sT, g.BT, ovT);
    return routed;
}

template <int GEOM, bool MAP>
__global__ __launch_bounds__(NK_WG) void k_free_paths(NkDev d, NkFreeDev f, NkFreeMapDev g) {
    extern __shared__ __align__(16) unsigned char smem[];
    NkLds L;
    nk_lds_setup<GEOM, 0>(d, smem, L);
    const int lane = (int)(threadIdx.x & 63u);
    const int li = __builtin_amdgcn_readfirstlane((int)blockIdx.x * NK_FP_WAVES + (int)(threadIdx.x >> 6));
    if (li >= f.nlist) return;                              // (after the only barrier)
    const int m0 = f.modes ? f.modes[li] : li;
    double wx = 0.0, wy = 0.0, wz = 0.0;
    if constexpr (MAP) { wx = g.weight[3 * (int64_t)li]; wy = g.weight[3 * (int64_t)li + 1]; wz = g.weight[3 * (int64_t)li + 2]; }
    double v[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) v[j] = 0.0;
    double sHits = 0.0, sInt = 0.0;
    unsigned long long casts = 0ull, missed = 0ull, capped = 0ull;
    unsigned int nClamped = 0u, ovK = 0u, ovP = 0u, ovT = 0u;
    for (int s0 = 0; s0 < f.n; s0 += 64) {
        const int s = s0 + lane;
        if (s >= f.n) continue;
        const int64_t r = (int64_t)li * f.n + s;
        const uint64_t rid = ((uint64_t)(uint32_t)m0 << 32) | (uint64_t)(uint32_t)s;
        double x, y, z;
        if (f.x0) { x = f.x0[3 * r]; y = f.x0[3 * r + 1]; z = f.x0[3 * r + 2]; }
        else nk_fl_sample(d, f.seed, rid, x, y, z);
        if (f.ray_x0) { f.ray_x0[3 * r] = x; f.ray_x0[3 * r + 1] = y; f.ray_x0[3 * r + 2] = z; }
        int cell = 0;
        if constexpr (MAP) {
            bool cl = false;
            const int ix = nk_field_axis(x, g.lo[0], g.inv_h[0], g.n[0], cl);
            const int iy = nk_field_axis(y, g.lo[1], g.inv_h[1], g.n[1], cl);
            const int iz = nk_field_axis(z, g.lo[2], g.inv_h[2], g.n[2], cl);
            nClamped += cl ? 1u : 0u;
            cell = (ix * g.n[1] + iy) * g.n[2] + iz;
        }
        int mode = m0;
        double vx = f.vg[3 * (int64_t)mode], vy = f.vg[3 * (int64_t)mode + 1], vz = f.vg[3 * (int64_t)mode + 2];
        double tau = f.tau[mode];
        NkFlRay c;
        nk_fl_start(c);
        int k = 0, ncast = 0;
        if (!(tau > 0.0) || (vx == 0.0 && vy == 0.0 && vz == 0.0)) {
            c.T = tau > 0.0 ? tau : 0.0;
            sInt = sInt + c.W;
        } else {
            for (;;) {
                double tc;
                int fc;
                NK_RAY(GEOM, d, L, NK_TREE_NO_SKIP, x, y, z, vx, vy, vz, tc, fc);
                ++ncast;
                if (fc < 0) {                               // a miss: the whole remaining flight, g = 1
                    nk_fl_miss(c, tau, vx, vy, vz, sInt);
                    ++missed;
                    c.end = 3;
                    break;
                }
                nk_fl_hit(c, tau, tc, vx, vy, vz, sInt, sHits);
                ++k;
                // The facet step, nk_fl_facet's statements written out: called as that function the step costs this kernel 2 % of
                // a call's time (profiles/free_flight_notes.txt); k_free_columns calls it.
                const NkFacet *fp = L.facets + fc;
                const int bc = fp->bc;
                if (bc == 'T' || bc == 'F') { c.end = 1; break; }
                const double hx = __builtin_fma(tc, vx, x), hy = __builtin_fma(tc, vy, y), hz = __builtin_fma(tc, vz, z);
                if (bc == 'P') {
                    x = hx + fp->tx; y = hy + fp->ty; z = hz + fp->tz;
                } else {
                    double r0, r1;
                    nk_uniform2_dev(f.seed, rid, (uint32_t)k, NK_TAG_FREE + 3u, r0, r1);
                    const int rough = fp->rough;
                    bool spec = false;
                    int out = -1;
                    if (rough >= 0 && rough < d.Fr) {       // (the host refuses 'R' facets without tables)
                        const int64_t idx = (int64_t)rough * d.M + mode;
                        out = d.spec_map[idx];
                        spec = d.true_spec[idx] && r0 <= d.specularity[idx] && out >= 0 && out < d.M;
                    }
                    if (!spec) { c.end = 2; break; }
                    if (d.degen_j2) {
                        const int j2 = d.degen_j2[out];
                        if (j2 > -1 && j2 < d.J && r1 >= 0.5) out = (out / d.J) * d.J + j2;
                    }
                    mode = out;
                    vx = f.vg[3 * (int64_t)mode]; vy = f.vg[3 * (int64_t)mode + 1]; vz = f.vg[3 * (int64_t)mode + 2];
                    tau = f.tau[mode];
                    x = hx; y = hy; z = hz;
                    if (!(tau > 0.0)) { sInt = sInt + c.W; c.end = 0; break; }     // reflected into a mode that does not live
                }
                if (c.W < f.w_min) { c.end = NK_FL_END_WMIN; break; }
                if (k >= f.max_segments) { ++capped; c.end = 4; break; }
            }
        }
        casts += (unsigned long long)ncast;
        nk_fl_ray_sums(c, v);
        double routed = 0.0;
        if constexpr (MAP) routed = nk_fm_bin(g, cell, c, wx, wy, wz, ovK, ovP, ovT);
        if (f.ray_D) { f.ray_D[3 * r] = c.Dx; f.ray_D[3 * r + 1] = c.Dy; f.ray_D[3 * r + 2] = c.Dz; }
        if (f.ray_T) f.ray_T[r] = c.T;
        if (f.ray_seg) f.ray_seg[r] = ncast;
        if (f.ray_end) f.ray_end[r] = nk_fl_end_code(c);
        if constexpr (MAP) {
            if (g.ray_cell) g.ray_cell[r] = cell;
            if (g.ray_w) g.ray_w[r] = routed;
        }
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) v[j] = nk_fl_wave_sum(v[j]);
    sHits = nk_fl_wave_sum(sHits); sInt = nk_fl_wave_sum(sInt);
    casts = nk_fl_wave_sum(casts); missed = nk_fl_wave_sum(missed); capped = nk_fl_wave_sum(capped);
    if (lane == 0) {
        nk_fl_store_row(f.rows + (int64_t)li * NK_FP_ROW, v, sHits, sInt);
        unsigned long long *cnt = f.counts + (int64_t)li * NK_FP_CNT;
        cnt[0] = casts; cnt[1] = missed; cnt[2] = capped; cnt[3] = 0ull;
    }
    if constexpr (MAP) {
        const unsigned long long nc = nk_fl_wave_sum((unsigned long long)nClamped), oK = nk_fl_wave_sum((unsigned long long)ovK);
        const unsigned long long oP = nk_fl_wave_sum((unsigned long long)ovP), oT = nk_fl_wave_sum((unsigned long long)ovT);
        if (lane == 0) {
            unsigned long long *hdr = g.grid + (size_t)g.ncells * NK_FREE_MAP_LINE;
            if (nc) atomicAdd(hdr + NK_FM_CLAMPED, nc);
            if (oK) atomicAdd(hdr + NK_FM_OVK, oK);
            if (oP) atomicAdd(hdr + NK_FM_OVP, oP);
            if (oT) atomicAdd(hdr + NK_FM_OVT, oT);
        }
    }
}

// the dispatch of NK_GEOM_LAUNCH (nk_engine.hip): the geometry mode and the map pick the instantiation
hipError_t nk_free_paths_launch(const NkDev &d, const NkFreeDev &f, const NkFreeMapDev *map, int geom, size_t lds, hipStream_t stream) {
    if (f.nlist <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((f.nlist + NK_FP_WAVES - 1) / NK_FP_WAVES);
    if (map) {
        if (geom == 1) k_free_paths<1, true><<<grid, NK_WG, lds, stream>>>(d, f, *map);
        else k_free_paths<2, true><<<grid, NK_WG, lds, stream>>>(d, f, *map);
    } else {
        if (geom == 1) k_free_paths<1, false><<<grid, NK_WG, lds, stream>>>(d, f, NkFreeMapDev{});
        else k_free_paths<2, false><<<grid, NK_WG, lds, stream>>>(d, f, NkFreeMapDev{});
    }
    return hipGetLastError();
}

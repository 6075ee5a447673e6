// nk_kinetic.hip -- kinetic flights: the deviational, time-step-free Monte Carlo of the steady linearised BTE in the relaxation-time
// picture (nk_kinetic_flights, nk_kinetic_flights_groups, nk_kinetic_flights_map): k_kinetic<GEOM, BINS, GROUPED, MAP>, k_kinetic_fold
// and their launch.  The C entry points are in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds
// the twelve instantiations of k_kinetic, k_kinetic_fold and nothing else (the trick of nk_modes.hip).
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_kinetic.h"
#include "nk_flight.h"

// =================================================================================== the rule
// DESIGN.md "Kinetic flights".  Sources are the 'T' facets in ascending order; from source f fly n energy packets, ray id =
// (f << 32) | sample, Philox key = the call's seed; the draws and their tags are listed in nk_kinetic.h.
//   emission  a point uniform on the facet (a triangle by cumulative area, a uniform point in it), a mode by rejection from
//             cdf_flux against the facet's inward normal (nk_kin_emit); after 64 refusals the ray is `lost`.
//   segment   t_s = -tau ln(u); a mode with v = 0 takes no cast and sits for t_s; else cast (the general cast of the geometry mode);
//             a miss ends the ray (`missed`, nothing is added).  t = min(t_s, t_c): D += t v, dwell += t (fused, nk_flight.h's manner);
//             one uniform point of the segment x_p = x + (u' t) v; t and t v go to the words of (source, nk_classify(x_p)).
//   event     k += 1.  t_s < t_c: scatter at x + t_s v into nk_ss_right(cdf_scatter, u).  Else the facet: 'T' absorbs (end = its
//             source index); 'P' and 'R' are nk_fl_facet's step; its diffuse outcome re-emits from the hit point by the emission's
//             rule with that facet's inward normal; a specular turn into a mode with tau <= 0 scatters at once (+ 3, this k).
//             k >= max_events ends the ray (`capped`).
// Lanes are rays and the lane loop is FLAT: a lane whose ray has ended starts its next ray (samples l, l + 64, .. of the wave's
// block) at the top of the same loop that casts, so no lane waits for the wave's slowest ray.  Every sum is a 64-bit integer at a
// power-of-two scale (a term above its bound is left out and counted): per source they are reduced over the wave by the butterfly
// and added once per wave; the per-subvolume words go to LDS bins first (BINS) or straight to memory.  Integer adds commute, so a
// result depends neither on the order of the rays nor on the launch grid.
// The map (MAP; DESIGN.md "Kinetic maps"): the same x_p also goes through the field's cell rule, and the segment's four integers --
// the same ones, no second rounding -- are added to the line of (source, cell(x_p)) in memory as well; points outside the grid
// land in its edge cells and are counted per source (row word NK_KR_CLAMPED).

// a mode for a packet that leaves a surface with inward normal n: flux-weighted, by rejection; false after NK_KIN_TRIALS refusals
__device__ __forceinline__ bool nk_kin_emit(const NkKinDev &f, uint64_t rid, uint32_t k, double nx, double ny, double nz, int &mode) {
#pragma clang fp contract(off)
    for (uint32_t j = 0; j < NK_KIN_TRIALS; ++j) {
        double u0, u1;
        nk_uniform2_dev(f.seed, rid, k, NK_TAG_KIN + 64u + j, u0, u1);
        int m = nk_ss_right(f.cdf_flux, f.M, u0);
        m = m > f.M - 1 ? f.M - 1 : m;
        const double vx = f.vg[3 * (int64_t)m], vy = f.vg[3 * (int64_t)m + 1], vz = f.vg[3 * (int64_t)m + 2];
        const double vn = (vx * nx + vy * ny) + vz * nz;
        const double sp = sqrt((vx * vx + vy * vy) + vz * vz);
        if (u1 * sp < vn) { mode = m; return true; }
    }
    return false;
}

// rint(term s) as a two's-complement integer, or 0 and a count where the term is above its bound (or a NaN)
__device__ __forceinline__ long long nk_kin_q(double term, double s, double B, unsigned int &over) {
#pragma clang fp contract(off)
    if (!(fabs(term) <= B)) { over += 1u; return 0ll; }
    return (long long)rint(term * s);
}

// the flat lane loop of one wave: the rays [blk * rays_per_wave, ..) of source src
// GROUPED (kinetic groups): the lane keeps the column of its mode beside tau -- loaded where tau is, when the mode changes -- and a
// segment's four words go to (source, subvolume, column) instead of (source, subvolume): the loop still does four adds per segment,
// and `sub` is folded from the columns afterwards (k_kinetic_fold)
// MAP (kinetic maps): the four words also go to the line of (source, cell of x_p) in memory -- four more adds per segment
template <int GEOM, bool BINS, bool GROUPED, bool MAP>
__device__ __forceinline__ void nk_kin_wave(const NkDev &d, const NkLds &L, const NkKinDev &f, int wi, int lane, unsigned long long *bins) {
#pragma clang fp contract(off)
    const int src = wi / f.blocks, blk = wi - src * f.blocks;
    int facet0 = 0;
#pragma unroll
    for (int j = 0; j < NK_KIN_MAX_SOURCES_DEV; ++j) facet0 = j == src ? f.src_facet[j] : facet0;
    const int s_end = (blk + 1) * f.rays_per_wave < f.n ? (blk + 1) * f.rays_per_wave : f.n;
    int next = blk * f.rays_per_wave + lane;
    NkFreeDev ff = {};                                       // what nk_fl_facet reads: the seed and the group velocities
    ff.seed = f.seed; ff.vg = f.vg;
    unsigned long long *sub;
    if constexpr (GROUPED) sub = (BINS ? bins : f.grp) + (size_t)src * d.S * f.GC * 4;
    else if constexpr (BINS) sub = bins + (size_t)src * d.S * 4;
    else sub = f.sub + (size_t)src * d.S * 4;
    [[maybe_unused]] unsigned int nClamped = 0u;             // MAP: segment points clamped into the grid's edge cells
    // the wave's sums
    unsigned int ends[NK_KIN_MAX_SOURCES_DEV];
#pragma unroll
    for (int j = 0; j < NK_KIN_MAX_SOURCES_DEV; ++j) ends[j] = 0u;
    unsigned int nLost = 0u, nMissed = 0u, nCapped = 0u, ovD = 0u, ovD2 = 0u, ovT = 0u, ovSt = 0u, ovSx = 0u;
    unsigned long long events = 0ull, casts = 0ull;
    long long aD[3] = {0ll, 0ll, 0ll}, aD2[3] = {0ll, 0ll, 0ll}, aT = 0ll;
    // the lane's ray
    int flying = 0, smp = 0, mode = 0, k = 0, ncast = 0, end = 0;
    [[maybe_unused]] int col = 0;                            // GROUPED: f.group[mode]
    uint64_t rid = 0ull, hash = 0ull;
    double x = 0.0, y = 0.0, z = 0.0, vx = 0.0, vy = 0.0, vz = 0.0, tau = 0.0, Dx = 0.0, Dy = 0.0, Dz = 0.0, T = 0.0;
    for (;;) {
        bool fin = false;
#ifdef NK_KIN_NESTED
        // developer build (make kinetic-nested): the per-ray loop the flat one is measured against -- the wave starts its next 64
        // rays only when the slowest of the last 64 has ended (the same rays, the same bits)
        const bool may_start = __ballot(flying) == 0ull;
#else
        const bool may_start = true;
#endif
        if (may_start && !flying && next < s_end) {         // the lane's next ray: the emission
            smp = next; next += 64;
            rid = ((uint64_t)(uint32_t)src << 32) | (uint64_t)(uint32_t)smp;
            double uf, us, ur, un;
            nk_uniform2_dev(f.seed, rid, 0u, NK_TAG_KIN + 0u, uf, us);
            nk_uniform2_dev(f.seed, rid, 0u, NK_TAG_KIN + 1u, ur, un);
            (void)un;
            const int f0 = d.facet_face_off[facet0], nf = d.facet_face_off[facet0 + 1] - f0;
            int a = nk_ss_right(d.facet_face_cdf + f0, nf, uf);
            a = a > nf - 1 ? nf - 1 : a;
            const double *fv = d.face_verts + 9 * (int64_t)d.facet_face_idx[f0 + a];
            const double sq = sqrt(us);
            const double a0 = 1.0 - sq, a1 = (1.0 - ur) * sq, a2 = ur * sq;
            x = (a0 * fv[0] + a1 * fv[3]) + a2 * fv[6];
            y = (a0 * fv[1] + a1 * fv[4]) + a2 * fv[7];
            z = (a0 * fv[2] + a1 * fv[5]) + a2 * fv[8];
            const NkFacet *fp = L.facets + facet0;
            k = 0; ncast = 0; hash = 0ull; Dx = Dy = Dz = T = 0.0; end = 0;
            mode = -1;
            if (!nk_kin_emit(f, rid, 0u, -fp->nx, -fp->ny, -fp->nz, mode)) { end = NK_KIN_LOST; fin = true; }
            else {
                vx = f.vg[3 * (int64_t)mode]; vy = f.vg[3 * (int64_t)mode + 1]; vz = f.vg[3 * (int64_t)mode + 2]; tau = f.tau[mode];
                if constexpr (GROUPED) col = f.group[mode];
            }
            const int64_t r = (int64_t)src * f.n + smp;
            if (f.ray_x0) { f.ray_x0[3 * r] = x; f.ray_x0[3 * r + 1] = y; f.ray_x0[3 * r + 2] = z; }
            if (f.ray_mode) f.ray_mode[r] = mode;
            flying = 1;
        }
        if (__ballot(flying) == 0ull) break;                // no ray in flight and none left to start
        if (flying && !fin) {                               // one segment and the event that ends it
            double u, up;
            nk_uniform2_dev(f.seed, rid, (uint32_t)k, NK_TAG_KIN + 2u, u, up);
            if (!(u > 0.0)) u = 0x1p-54;
            const double ts = -tau * log(u);
            const bool flies = vx != 0.0 || vy != 0.0 || vz != 0.0;
            double tc = __builtin_inf();
            int fc = -1;
            if (flies) {
                NK_RAY(GEOM, d, L, NK_TREE_NO_SKIP, x, y, z, vx, vy, vz, tc, fc);
                ++ncast;
            }
            if (flies && fc < 0) { end = NK_KIN_MISSED; fin = true; }
            else {
                const bool scat = !flies || ts < tc;
                const double t = scat ? ts : tc;
                Dx = __builtin_fma(t, vx, Dx); Dy = __builtin_fma(t, vy, Dy); Dz = __builtin_fma(t, vz, Dz);
                T = T + t;
                const double ap = up * t;
                const double px = __builtin_fma(ap, vx, x), py = __builtin_fma(ap, vy, y), pz = __builtin_fma(ap, vz, z);
                const int s = nk_classify(d, L.tb, px, py, pz);
                unsigned long long *w;                      // s < S (and col < GC: the host checks the table)
                if constexpr (GROUPED) w = sub + 4 * ((size_t)s * f.GC + col);
                else w = sub + 4 * s;
                const long long qt = nk_kin_q(t, f.st, f.Bt, ovSt);
                const long long qx = nk_kin_q(t * vx, f.sx, f.Bx, ovSx), qy = nk_kin_q(t * vy, f.sx, f.Bx, ovSx), qz = nk_kin_q(t * vz, f.sx, f.Bx, ovSx);
                if (qt) atomicAdd(w, (unsigned long long)qt);
                if (qx) atomicAdd(w + 1, (unsigned long long)qx);
                if (qy) atomicAdd(w + 2, (unsigned long long)qy);
                if (qz) atomicAdd(w + 3, (unsigned long long)qz);
                if constexpr (MAP) {                        // the same integers into the line of (source, cell of x_p)
                    bool cl = false;
                    const int ix = nk_field_axis(px, f.lo[0], f.inv_h[0], f.gn[0], cl);
                    const int iy = nk_field_axis(py, f.lo[1], f.inv_h[1], f.gn[1], cl);
                    const int iz = nk_field_axis(pz, f.lo[2], f.inv_h[2], f.gn[2], cl);
                    nClamped += cl ? 1u : 0u;
                    const int cell = (ix * f.gn[1] + iy) * f.gn[2] + iz;        // < ncells <= 2^24: every index is clamped
                    unsigned long long *c = f.map + 4 * ((size_t)src * f.ncells + cell);
                    if (qt) atomicAdd(c, (unsigned long long)qt);
                    if (qx) atomicAdd(c + 1, (unsigned long long)qx);
                    if (qy) atomicAdd(c + 2, (unsigned long long)qy);
                    if (qz) atomicAdd(c + 3, (unsigned long long)qz);
                }
                ++k;
                bool scatter_now = scat;
                if (scat) {
                    x = __builtin_fma(t, vx, x); y = __builtin_fma(t, vy, y); z = __builtin_fma(t, vz, z);
                    hash = hash * 1000003ull + 1ull;
                } else {
                    hash = hash * 1000003ull + (uint64_t)(fc + 2);
                    const NkFacet *fp = L.facets + fc;
                    if (fp->bc == 'T') {
                        int e = NK_KIN_MISSED;               // (every 'T' facet is a source)
#pragma unroll
                        for (int j = 0; j < NK_KIN_MAX_SOURCES_DEV; ++j) e = (j < f.nsrc && f.src_facet[j] == fc) ? j : e;
                        end = e; fin = true;
                    } else {
                        const double hx = __builtin_fma(tc, vx, x), hy = __builtin_fma(tc, vy, y), hz = __builtin_fma(tc, vz, z);
                        const double nx = -fp->nx, ny = -fp->ny, nz = -fp->nz;
                        bool turned;
                        const int what = nk_fl_facet(d, L, ff, fc, tc, rid, k, x, y, z, vx, vy, vz, mode, turned);
                        if (what != 0) {                    // diffuse: re-emitted from the hit point
                            x = hx; y = hy; z = hz;
                            if (!nk_kin_emit(f, rid, (uint32_t)k, nx, ny, nz, mode)) { end = NK_KIN_LOST; fin = true; }
                            else {
                                vx = f.vg[3 * (int64_t)mode]; vy = f.vg[3 * (int64_t)mode + 1]; vz = f.vg[3 * (int64_t)mode + 2]; tau = f.tau[mode];
                                if constexpr (GROUPED) col = f.group[mode];
                            }
                        } else if (turned) {
                            tau = f.tau[mode];
                            if constexpr (GROUPED) col = f.group[mode];
                            scatter_now = !(tau > 0.0);     // a specular turn into a mode that does not live
                        }
                    }
                }
                if (scatter_now) {
                    double us, un;
                    nk_uniform2_dev(f.seed, rid, (uint32_t)k, NK_TAG_KIN + 3u, us, un);
                    (void)un;
                    int m = nk_ss_right(f.cdf_scatter, f.M, us);
                    mode = m > f.M - 1 ? f.M - 1 : m;
                    vx = f.vg[3 * (int64_t)mode]; vy = f.vg[3 * (int64_t)mode + 1]; vz = f.vg[3 * (int64_t)mode + 2]; tau = f.tau[mode];
                    if constexpr (GROUPED) col = f.group[mode];
                }
                if (!fin && k >= f.max_events) { end = NK_KIN_CAPPED; fin = true; }
            }
        }
        if (fin) {                                          // the finished ray into the lane's sums
            events += (unsigned long long)k; casts += (unsigned long long)ncast;
#pragma unroll
            for (int j = 0; j < NK_KIN_MAX_SOURCES_DEV; ++j) ends[j] += end == j ? 1u : 0u;
            nLost += end == NK_KIN_LOST ? 1u : 0u; nMissed += end == NK_KIN_MISSED ? 1u : 0u; nCapped += end == NK_KIN_CAPPED ? 1u : 0u;
            aD[0] += nk_kin_q(Dx, f.sD, f.BD, ovD); aD[1] += nk_kin_q(Dy, f.sD, f.BD, ovD); aD[2] += nk_kin_q(Dz, f.sD, f.BD, ovD);
            aD2[0] += nk_kin_q(Dx * Dx, f.sD2, f.BD2, ovD2); aD2[1] += nk_kin_q(Dy * Dy, f.sD2, f.BD2, ovD2); aD2[2] += nk_kin_q(Dz * Dz, f.sD2, f.BD2, ovD2);
            aT += nk_kin_q(T, f.sT, f.BT, ovT);
            const int64_t r = (int64_t)src * f.n + smp;
            if (f.ray_D) { f.ray_D[3 * r] = Dx; f.ray_D[3 * r + 1] = Dy; f.ray_D[3 * r + 2] = Dz; }
            if (f.ray_T) f.ray_T[r] = T;
            if (f.ray_end) f.ray_end[r] = end;
            if (f.ray_events) f.ray_events[r] = k;
            if (f.ray_casts) f.ray_casts[r] = ncast;
            if (f.ray_hash) f.ray_hash[r] = hash;
            flying = 0;
        }
    }
    // once per wave: the butterfly, then lane 0 adds the row
    unsigned long long row[NK_KR_OVSX + 1];
#pragma unroll
    for (int j = 0; j < NK_KIN_MAX_SOURCES_DEV; ++j) row[NK_KR_ENDS + j] = (unsigned long long)ends[j];
    row[NK_KR_LOST] = nLost; row[NK_KR_MISSED] = nMissed; row[NK_KR_CAPPED] = nCapped; row[NK_KR_EVENTS] = events; row[NK_KR_CASTS] = casts;
#pragma unroll
    for (int a = 0; a < 3; ++a) { row[NK_KR_D + a] = (unsigned long long)aD[a]; row[NK_KR_D2 + a] = (unsigned long long)aD2[a]; }
    row[NK_KR_T] = (unsigned long long)aT;
    row[NK_KR_OVD] = ovD; row[NK_KR_OVD2] = ovD2; row[NK_KR_OVT] = ovT; row[NK_KR_OVST] = ovSt; row[NK_KR_OVSX] = ovSx;
    unsigned long long *out = f.rows + (size_t)src * NK_KIN_ROW;
#pragma unroll
    for (int j = 0; j <= NK_KR_OVSX; ++j) {
        const unsigned long long v = nk_fl_wave_sum(row[j]);
        if (lane == 0 && v) atomicAdd(out + j, v);
    }
    if constexpr (MAP) {
        const unsigned long long v = nk_fl_wave_sum((unsigned long long)nClamped);
        if (lane == 0 && v) atomicAdd(out + NK_KR_CLAMPED, v);
    }
}

// MAP asks for three waves per SIMD by name: left to itself the tree-walk instantiation with bins takes 170 VGPRs, two over what
// three waves allow (168); asked, all four fit (141 / 137 / 164 / 160, nothing spilled).  The other eight get the default (1) and
// compile to the instructions they had before the map existed.
template <int GEOM, bool BINS, bool GROUPED, bool MAP>
__global__ __launch_bounds__(NK_WG) __attribute__((amdgpu_waves_per_eu(MAP ? 3 : 1))) void k_kinetic(NkDev d, NkKinDev f) {
    extern __shared__ __align__(16) unsigned char smem[];
    NkLds L;
    nk_lds_setup<GEOM, 0>(d, smem, L);
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(smem + f.bins_off);
    const int nb = GROUPED ? f.nsrc * d.S * f.GC * 4 : f.nsrc * d.S * 4;
    if constexpr (BINS) {
        for (int i = (int)threadIdx.x; i < nb; i += NK_WG) bins[i] = 0ull;
        __syncthreads();
    }
    const int lane = (int)(threadIdx.x & 63u);
    const int wi = __builtin_amdgcn_readfirstlane((int)blockIdx.x * NK_KIN_WAVES + (int)(threadIdx.x >> 6));
    if (wi < f.nsrc * f.blocks) nk_kin_wave<GEOM, BINS, GROUPED, MAP>(d, L, f, wi, lane, bins);
    if constexpr (BINS) {
        __syncthreads();
        unsigned long long *out = GROUPED ? f.grp : f.sub;
        for (int i = (int)threadIdx.x; i < nb; i += NK_WG) {
            const unsigned long long v = bins[i];
            if (v) atomicAdd(out + i, v);
        }
    }
}

// kinetic groups: the plain words of (source, subvolume) are the integer sums of its columns' words -- one thread per word of
// `sub`, launched behind k_kinetic<.., true> on the same stream.  Integer adds commute, so `sub` holds the bits an ungrouped call gives.
__global__ __launch_bounds__(NK_WG) void k_kinetic_fold(NkKinDev f, int S) {
    const int i = (int)(blockIdx.x * NK_WG + threadIdx.x);            // (source * S + subvolume) * 4 + word
    if (i >= f.nsrc * S * 4) return;
    const unsigned long long *g = f.grp + (size_t)(i >> 2) * f.GC * 4 + (i & 3);
    unsigned long long v = 0ull;
    for (int c = 0; c < f.GC; ++c) v += g[(size_t)c * 4];
    f.sub[i] = v;
}

template <bool GROUPED, bool MAP>
static void nk_kinetic_pick(const NkDev &d, const NkKinDev &f, int geom, size_t lds, bool bins, unsigned grid, hipStream_t stream) {
    if (bins) {
        if (geom == 1) k_kinetic<1, true, GROUPED, MAP><<<grid, NK_WG, lds, stream>>>(d, f);
        else k_kinetic<2, true, GROUPED, MAP><<<grid, NK_WG, lds, stream>>>(d, f);
    } else {
        if (geom == 1) k_kinetic<1, false, GROUPED, MAP><<<grid, NK_WG, lds, stream>>>(d, f);
        else k_kinetic<2, false, GROUPED, MAP><<<grid, NK_WG, lds, stream>>>(d, f);
    }
}

// the dispatch of NK_GEOM_LAUNCH (nk_engine.hip): the geometry mode, the bins, the groups and the map pick the instantiation (the
// host refuses groups together with a map: only GROUPED = false is instantiated with MAP = true)
hipError_t nk_kinetic_launch(const NkDev &d, const NkKinDev &f, int geom, size_t lds, bool bins, hipStream_t stream) {
    const int waves = f.nsrc * f.blocks;
    if (waves <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((waves + NK_KIN_WAVES - 1) / NK_KIN_WAVES);
    if (f.GC > 0) {
        if (f.map) return hipErrorInvalidValue;
        nk_kinetic_pick<true, false>(d, f, geom, lds, bins, grid, stream);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const int words = f.nsrc * d.S * 4;
        k_kinetic_fold<<<(unsigned)((words + NK_WG - 1) / NK_WG), NK_WG, 0, stream>>>(f, d.S);
    } else if (f.map) {
        nk_kinetic_pick<false, true>(d, f, geom, lds, bins, grid, stream);
    } else {
        nk_kinetic_pick<false, false>(d, f, geom, lds, bins, grid, stream);
    }
    return hipGetLastError();
}

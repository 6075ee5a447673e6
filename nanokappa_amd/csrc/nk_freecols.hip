// nk_freecols.hip -- free-path sampling with K lifetime columns (nk_free_paths_columns): k_free_columns<GEOM, KT> and its launch.
// The C entry point (nk_free_paths_columns) is in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds the
// instantiations of k_free_columns and nothing else (the trick of nk_modes.hip and nk_freepath.hip).
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_freecols.h"
#include "nk_flight.h"

// =================================================================================== the rule
// The rule of k_free_paths (nk_freepath.hip; DESIGN.md "Free-path sampling") for K lifetime tables at once (DESIGN.md "Free-path
// sweeps").  The path of a ray -- start point, facets, periodic translations, specular / diffuse draws, the modes it is reflected
// into -- does not depend on the lifetimes, only its weights do.  So a ray is cast ONCE per segment and weighed once per column:
// column c keeps {W, D[3], T} and its end code, and takes part in a segment as long as it is alive.  The hit count k, the draw
// (seed, ray id, k, NK_TAG_FREE + 3) and the new mode are the ray's.  The ray flies while any column is alive.
// Column c of the result is k_free_paths with tau = column c, bit for bit: both kernels weigh a ray with the statements of
// nk_flight.h, whose roundings are spelled out, so neither the tile nor the neighbouring columns can change a column's bits.
// One wave per mode of the list, lanes are samples, lane l takes samples l, l + 64, ... ascending.  hits and p_int are added per
// segment and stay in registers; the sums that are added once per ray (D, D^2, T, p_res, p_wall, w_left, the counts) are formed
// from the finished ray's state when the lane starts its next ray or, for its last ray, before the butterfly -- between two rays
// of a lane (n > 64 only) they rest in `acc`, a scratch area in device memory, never inside the cast loop.  No atomics.

// A column's weights of one ray: the ray's record, the column's lifetime in the ray's mode and the casts made while it was alive
struct NkFcCol : NkFlRay {
    double tau;
    int nc;
};

// the sums a finished ray adds once to a column: nk_fl_ray_sums, and n[0..2] += its casts, missed, capped
__device__ __forceinline__ void nk_fc_ray_sums(const NkFcCol &c, double *v, unsigned long long *n) {
    nk_fl_ray_sums(c, v);
    n[0] += (unsigned long long)c.nc; n[1] += c.end == 3 ? 1ull : 0ull; n[2] += c.end == 4 ? 1ull : 0ull;
}

template <int GEOM, int KT>
__global__ __launch_bounds__(NK_WG) void k_free_columns(NkDev d, NkFreeColsDev q) {
    extern __shared__ __align__(16) unsigned char smem[];
    NkLds L;
    nk_lds_setup<GEOM, 0>(d, smem, L);
    const NkFreeDev &f = q.f;
    const int lane = (int)(threadIdx.x & 63u);
    const int slot = __builtin_amdgcn_readfirstlane((int)blockIdx.x * NK_FP_WAVES + (int)(threadIdx.x >> 6));
    const int nslots = (int)gridDim.x * NK_FP_WAVES;
    const int kc = q.kc;
    const double *taub = f.tau + (int64_t)q.c0 * q.M;
    const int mine = lane < f.n ? (f.n - lane + 63) / 64 : 0;      // rays of this lane
    for (int li = slot; li < f.nlist; li += nslots) {               // (after the only barrier; one turn unless n > 64)
        const int m0 = f.modes ? f.modes[li] : li;
        double sHits[KT], sInt[KT];
        NkFcCol col[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            sHits[c] = 0.0; sInt[c] = 0.0;
            col[c] = NkFcCol{};
        }
        unsigned long long shared = 0ull;
        for (int s0 = 0; s0 < f.n; s0 += 64) {
            const int s = s0 + lane;
            if (s >= f.n) continue;
            if (s0 > 0) {                                           // the ray this lane finished before: into the lane sums
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (c < kc) {
                        double *a = q.acc + (((int64_t)slot * kc + c) * NK_FC_ACC) * 64 + lane;
                        unsigned long long *an = (unsigned long long *)(a + 10 * 64);
                        double v[10];
                        unsigned long long n[3];
                        const bool ld = s0 > 64;
#pragma unroll
                        for (int j = 0; j < 10; ++j) v[j] = ld ? a[j * 64] : 0.0;
#pragma unroll
                        for (int j = 0; j < 3; ++j) n[j] = ld ? an[j * 64] : 0ull;
                        nk_fc_ray_sums(col[c], v, n);
#pragma unroll
                        for (int j = 0; j < 10; ++j) a[j * 64] = v[j];
#pragma unroll
                        for (int j = 0; j < 3; ++j) an[j * 64] = n[j];
                    }
            }
            const int64_t r = (int64_t)li * f.n + s;
            const uint64_t rid = ((uint64_t)(uint32_t)m0 << 32) | (uint64_t)(uint32_t)s;
            double x, y, z;
            if (f.x0) { x = f.x0[3 * r]; y = f.x0[3 * r + 1]; z = f.x0[3 * r + 2]; }
            else nk_fl_sample(d, f.seed, rid, x, y, z);
            if (f.ray_x0 && q.c0 == 0) { f.ray_x0[3 * r] = x; f.ray_x0[3 * r + 1] = y; f.ray_x0[3 * r + 2] = z; }
            int mode = m0;
            double vx = f.vg[3 * (int64_t)mode], vy = f.vg[3 * (int64_t)mode + 1], vz = f.vg[3 * (int64_t)mode + 2];
            const bool still = vx == 0.0 && vy == 0.0 && vz == 0.0;
            unsigned alive = 0u;
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < kc) {
                    NkFcCol &o = col[c];
                    o.tau = taub[(int64_t)c * q.M + mode];
                    nk_fl_start(o);
                    o.nc = 0;
                    if (!(o.tau > 0.0) || still) {
                        o.T = o.tau > 0.0 ? o.tau : 0.0;
                        sInt[c] = sInt[c] + o.W;
                    } else alive |= 1u << c;
                }
            int k = 0, ncast = 0;
            while (alive) {
                double tc;
                int fc;
                NK_RAY(GEOM, d, L, NK_TREE_NO_SKIP, x, y, z, vx, vy, vz, tc, fc);
                ++ncast;
                if (fc < 0) {
#pragma unroll
                    for (int c = 0; c < KT; ++c)
                        if (alive >> c & 1u) { nk_fl_miss(col[c], col[c].tau, vx, vy, vz, sInt[c]); col[c].end = 3; col[c].nc = ncast; }
                    break;
                }
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (alive >> c & 1u) nk_fl_hit(col[c], col[c].tau, tc, vx, vy, vz, sInt[c], sHits[c]);
                ++k;
                bool turned;
                const int outcome = nk_fl_facet(d, L, f, fc, tc, rid, k, x, y, z, vx, vy, vz, mode, turned);
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (alive >> c & 1u) {
                        NkFcCol &o = col[c];
                        int end = -1;
                        if (outcome) end = outcome;
                        else {
                            if (turned) o.tau = taub[(int64_t)c * q.M + mode];
                            if (!(o.tau > 0.0)) { sInt[c] = sInt[c] + o.W; end = 0; }     // reflected into a mode that does not live
                            else if (o.W < f.w_min) end = NK_FL_END_WMIN;
                            else if (k >= f.max_segments) end = 4;
                        }
                        if (end >= 0) { o.end = end; o.nc = ncast; alive &= ~(1u << c); }
                    }
            }
            shared += (unsigned long long)ncast;
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < kc) {
                    const NkFcCol &o = col[c];
                    const int64_t rc = (int64_t)(q.c0 + c) * q.rays + r;
                    if (f.ray_D) { f.ray_D[3 * rc] = o.Dx; f.ray_D[3 * rc + 1] = o.Dy; f.ray_D[3 * rc + 2] = o.Dz; }
                    if (f.ray_T) f.ray_T[rc] = o.T;
                    if (f.ray_seg) f.ray_seg[rc] = o.nc;
                    if (f.ray_end) f.ray_end[rc] = nk_fl_end_code(o);
                }
        }
        // the lane's last ray, the butterfly, the rows
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < kc) {
                double v[10];
                unsigned long long n[3];
                const bool ld = mine > 1;
                const double *a = q.acc + (((int64_t)slot * kc + c) * NK_FC_ACC) * 64 + lane;      // (read only when the lane flew two rays)
                const unsigned long long *an = (const unsigned long long *)(a + 10 * 64);
#pragma unroll
                for (int j = 0; j < 10; ++j) v[j] = ld ? a[j * 64] : 0.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) n[j] = ld ? an[j * 64] : 0ull;
                if (mine > 0) nk_fc_ray_sums(col[c], v, n);
#pragma unroll
                for (int j = 0; j < 10; ++j) v[j] = nk_fl_wave_sum(v[j]);
#pragma unroll
                for (int j = 0; j < 3; ++j) n[j] = nk_fl_wave_sum(n[j]);
                const double hits = nk_fl_wave_sum(sHits[c]), pint = nk_fl_wave_sum(sInt[c]);
                if (lane == 0) {
                    const int64_t rw = (int64_t)(q.c0 + c) * f.nlist + li;
                    nk_fl_store_row(f.rows + rw * NK_FP_ROW, v, hits, pint);
                    unsigned long long *cnt = f.counts + rw * NK_FP_CNT;
                    cnt[0] = n[0]; cnt[1] = n[1]; cnt[2] = n[2]; cnt[3] = 0ull;
                }
            }
        shared = nk_fl_wave_sum(shared);
        if (lane == 0) q.shared[li] = shared;
    }
}

// the dispatch of NK_GEOM_LAUNCH (nk_engine.hip), and of the column tile
template <int GEOM>
static hipError_t nk_fc_launch(const NkDev &d, const NkFreeColsDev &q, size_t lds, unsigned grid, hipStream_t stream) {
    switch (nk_free_columns_tile(q.kc)) {
        case 1: k_free_columns<GEOM, 1><<<grid, NK_WG, lds, stream>>>(d, q); break;
        case 4: k_free_columns<GEOM, 4><<<grid, NK_WG, lds, stream>>>(d, q); break;
        default: k_free_columns<GEOM, NK_FC_TILE><<<grid, NK_WG, lds, stream>>>(d, q); break;
    }
    return hipGetLastError();
}
hipError_t nk_free_columns_launch(const NkDev &d, const NkFreeColsDev &q, int geom, size_t lds, unsigned grid, hipStream_t stream) {
    if (q.f.nlist <= 0 || q.kc <= 0 || q.kc > NK_FC_TILE || grid == 0) return hipSuccess;
    return geom == 1 ? nk_fc_launch<1>(d, q, lds, grid, stream) : nk_fc_launch<2>(d, q, lds, grid, stream);
}

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

// =================================================================================== the rule
// The rule of k_free_paths (nk_freepath.hip; DESIGN.md "Free-path sampling") for K lifetime tables at once (DESIGN.md "Free-path
// sweeps").  The path of a ray -- start point, facets, periodic translations, specular / diffuse draws, the modes it is reflected
// into -- does not depend on the lifetimes, only its weights do.  So a ray is cast ONCE per segment and weighed once per column:
// column c keeps {W, D[3], T} and its end code, and takes part in a segment as long as it is alive.  The hit count k, the draw
// (seed, ray id, k, NK_TAG_FREE + 3) and the new mode are the ray's.  The ray flies while any column is alive.
// Column c of the result is k_free_paths with tau = column c, bit for bit: the statements below are that kernel's, written with
// the roundings its machine code has (make asm-freepath): the multiply-adds it fuses are __builtin_fma here, everything else is
// kept from fusing (#pragma clang fp contract(off)), so neither the tile nor the neighbouring columns can change a column's bits.
// One wave per mode of the list, lanes are samples, lane l takes samples l, l + 64, ... ascending.  hits and p_int are added per
// segment and stay in registers; the sums that are added once per ray (D, D^2, T, p_res, p_wall, w_left, the counts) are formed
// from the finished ray's state when the lane starts its next ray or, for its last ray, before the butterfly -- between two rays
// of a lane (n > 64 only) they rest in `acc`, a scratch area in device memory, never inside the cast loop.  No atomics.

// nk_freepath.hip's nk_fp_decay
__device__ __forceinline__ void nk_fc_decay(double a, double &g, double &e) {
#pragma clang fp contract(off)
    if (a <= 0.125) {
        double p = 1.0 / 39916800.0;
        p = __builtin_fma(p, a, -1.0 / 3628800.0);
        p = __builtin_fma(p, a, 1.0 / 362880.0);
        p = __builtin_fma(p, a, -1.0 / 40320.0);
        p = __builtin_fma(p, a, 1.0 / 5040.0);
        p = __builtin_fma(p, a, -1.0 / 720.0);
        p = __builtin_fma(p, a, 1.0 / 120.0);
        p = __builtin_fma(p, a, -1.0 / 24.0);
        p = __builtin_fma(p, a, 1.0 / 6.0);
        p = __builtin_fma(p, a, -0.5);
        p = __builtin_fma(p, a, 1.0);
        g = a * p;
        e = nk_exp_small(-a);
    } else {
        e = nk_exp(-a);
        g = 1.0 - e;
    }
}

// nk_freepath.hip's nk_fp_sample, statement for statement
__device__ __forceinline__ void nk_fc_sample(const NkDev &d, uint64_t seed, uint64_t rid, double &x, double &y, double &z) {
    double u0, u1, u2, u3, u4, u5;
    nk_uniform2_dev(seed, rid, 0u, NK_TAG_FREE + 0u, u0, u1);
    nk_uniform2_dev(seed, rid, 0u, NK_TAG_FREE + 1u, u2, u3);
    nk_uniform2_dev(seed, rid, 0u, NK_TAG_FREE + 2u, u4, u5);
    (void)u5;
    int sx = nk_ss_right(d.simplex_cdf, d.nS, u0);
    sx = sx > d.nS - 1 ? d.nS - 1 : sx;
    const double a0 = -log(u1), a1 = -log(u2), a2 = -log(u3), a3 = -log(u4);
    double asum = 0.0;
    asum += a0; asum += a1; asum += a2; asum += a3;
    const double *sp = d.simplex_pts + 12 * (int64_t)sx;
    const double w0 = a0 / asum, w1 = a1 / asum, w2 = a2 / asum, w3 = a3 / asum;
    x = y = z = 0.0;
    x += w0 * sp[0]; y += w0 * sp[1]; z += w0 * sp[2];
    x += w1 * sp[3]; y += w1 * sp[4]; z += w1 * sp[5];
    x += w2 * sp[6]; y += w2 * sp[7]; z += w2 * sp[8];
    x += w3 * sp[9]; y += w3 * sp[10]; z += w3 * sp[11];
}

__device__ __forceinline__ double nk_fc_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long nk_fc_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A column's weights of one ray.  end: 0 scattered intrinsically (no start, or reflected into a mode that does not live), 1
// reservoir, 2 diffuse wall, 3 miss, 4 cap, NK_FC_END_WMIN weight exhausted (code 0 of the public interface, but its W goes to w_left)
#define NK_FC_END_WMIN 5
struct NkFcCol {
    double W, Dx, Dy, Dz, T, tau;
    int nc, end;                 // casts made while the column was alive; its end code
};

// a hit after tc: k_free_paths' segment.  sInt += W g and hits += W e are single multiply-adds there (W e is not rounded first)
__device__ __forceinline__ void nk_fc_hit(NkFcCol &c, double tc, double vx, double vy, double vz, double &sInt, double &sHits) {
#pragma clang fp contract(off)
    double g, e;
    nk_fc_decay(tc / c.tau, g, e);
    const double wt = (c.W * c.tau) * g;
    c.Dx = __builtin_fma(wt, vx, c.Dx); c.Dy = __builtin_fma(wt, vy, c.Dy); c.Dz = __builtin_fma(wt, vz, c.Dz);
    c.T = c.T + wt;
    sInt = __builtin_fma(c.W, g, sInt);
    sHits = __builtin_fma(c.W, e, sHits);
    c.W = c.W * e;
}
// a miss: the whole remaining flight, g = 1
__device__ __forceinline__ void nk_fc_miss(NkFcCol &c, double vx, double vy, double vz, double &sInt) {
#pragma clang fp contract(off)
    const double wt = c.W * c.tau;
    c.Dx = __builtin_fma(wt, vx, c.Dx); c.Dy = __builtin_fma(wt, vy, c.Dy); c.Dz = __builtin_fma(wt, vz, c.Dz);
    c.T = c.T + wt;
    sInt = sInt + c.W;
}

// The sums a finished ray adds once, in k_free_paths' order and roundings (D^2 with one multiply-add): v[0..9] = v + the ray's,
// n[0..2] likewise.  Adding +0 where that kernel adds nothing changes no bit: these sums are +0 or positive.
__device__ __forceinline__ void nk_fc_ray_sums(const NkFcCol &c, double *v, unsigned long long *n) {
#pragma clang fp contract(off)
    v[0] = v[0] + c.Dx; v[1] = v[1] + c.Dy; v[2] = v[2] + c.Dz;
    v[3] = __builtin_fma(c.Dx, c.Dx, v[3]); v[4] = __builtin_fma(c.Dy, c.Dy, v[4]); v[5] = __builtin_fma(c.Dz, c.Dz, v[5]);
    v[6] = v[6] + c.T;
    v[7] = v[7] + (c.end == 1 ? c.W : 0.0);
    v[8] = v[8] + (c.end == 2 ? c.W : 0.0);
    v[9] = v[9] + ((c.end == 4 || c.end == NK_FC_END_WMIN) ? c.W : 0.0);
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
            col[c].W = 0.0; col[c].Dx = 0.0; col[c].Dy = 0.0; col[c].Dz = 0.0; col[c].T = 0.0; col[c].tau = 0.0; col[c].nc = 0; col[c].end = 0;
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
            else nk_fc_sample(d, f.seed, rid, x, y, z);
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
                    o.W = 1.0; o.Dx = 0.0; o.Dy = 0.0; o.Dz = 0.0; o.T = 0.0; o.nc = 0; o.end = 0;
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
                        if (alive >> c & 1u) { nk_fc_miss(col[c], vx, vy, vz, sInt[c]); col[c].end = 3; col[c].nc = ncast; }
                    break;
                }
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (alive >> c & 1u) nk_fc_hit(col[c], tc, vx, vy, vz, sInt[c], sHits[c]);
                ++k;
                // what the facet makes of the ray: 1 a reservoir ends it, 2 a diffuse reflection ends it, 0 it goes on (from a
                // new point, after a specular reflection in a new mode)
                const NkFacet *fp = L.facets + fc;
                const int bc = fp->bc;
                int outcome = 0;
                bool turned = false;
                if (bc == 'T' || bc == 'F') outcome = 1;
                else {
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
                        if (!spec) outcome = 2;
                        else {
                            if (d.degen_j2) {
                                const int j2 = d.degen_j2[out];
                                if (j2 > -1 && j2 < d.J && r1 >= 0.5) out = (out / d.J) * d.J + j2;
                            }
                            mode = out;
                            vx = f.vg[3 * (int64_t)mode]; vy = f.vg[3 * (int64_t)mode + 1]; vz = f.vg[3 * (int64_t)mode + 2];
                            x = hx; y = hy; z = hz;
                            turned = true;
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (alive >> c & 1u) {
                        NkFcCol &o = col[c];
                        int end = -1;
                        if (outcome) end = outcome;
                        else {
                            if (turned) o.tau = taub[(int64_t)c * q.M + mode];
                            if (!(o.tau > 0.0)) { sInt[c] = sInt[c] + o.W; end = 0; }     // reflected into a mode that does not live
                            else if (o.W < f.w_min) end = NK_FC_END_WMIN;
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
                    if (f.ray_end) f.ray_end[rc] = o.end == NK_FC_END_WMIN ? 0 : o.end;
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
                for (int j = 0; j < 10; ++j) v[j] = nk_fc_wave_sum(v[j]);
#pragma unroll
                for (int j = 0; j < 3; ++j) n[j] = nk_fc_wave_sum(n[j]);
                const double hits = nk_fc_wave_sum(sHits[c]), pint = nk_fc_wave_sum(sInt[c]);
                if (lane == 0) {
                    const int64_t rw = (int64_t)(q.c0 + c) * f.nlist + li;
                    double *row = f.rows + rw * NK_FP_ROW;
                    row[0] = v[0]; row[1] = v[1]; row[2] = v[2]; row[3] = v[3]; row[4] = v[4]; row[5] = v[5];
                    row[6] = v[6]; row[7] = hits; row[8] = v[7]; row[9] = v[8]; row[10] = v[9]; row[11] = pint;
                    unsigned long long *cnt = f.counts + rw * NK_FP_CNT;
                    cnt[0] = n[0]; cnt[1] = n[1]; cnt[2] = n[2]; cnt[3] = 0ull;
                }
            }
        shared = nk_fc_wave_sum(shared);
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

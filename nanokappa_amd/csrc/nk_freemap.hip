// nk_freemap.hip -- free-path maps (nk_free_paths_map): k_free_map<GEOM> and its launch: the flight of k_free_paths with every
// finished ray binned by the cell of its START point.  The C entry points (nk_free_paths_map, nk_free_paths_map_info) are in
// nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds
// k_free_map<1> and k_free_map<2> and nothing else (the trick of nk_modes.hip, nk_freepath.hip and nk_freecols.hip).
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_freemap.h"

// =================================================================================== the rule
// The flight is k_free_paths' (nk_freepath.hip; DESIGN.md "Free-path sampling"), statement for statement: one wave per list
// entry, lane l takes samples l, l + 64, ... ascending, the same start points, cast, decay, facet outcomes, draws, w_min,
// max_segments and end codes; the rows are summed in the same lane order and by the same xor butterfly.  The rows and the per-ray
// outputs equal nk_free_paths' bit for bit: the arithmetic is written with the roundings that kernel's machine code has (make
// asm-freepath; DESIGN.md "Free-path sweeps"): `p_int += W g`, `hits += W e`, `D += wt v` and `D2 += D D` are fused
// multiply-adds, `wt = (W tau) g`, `T += wt`, `W *= e` and the per-ray adds are not -- spelled out with __builtin_fma under
// #pragma clang fp contract(off), as nk_freecols.hip does.
// The map (DESIGN.md "Free-path maps"): once per finished ray, by the lane that flew it, into the line of the ray's START cell
// -- the field's cell rule, i_a = floor((x_a - lo_a) * (1 / h_a)), an index outside [0, n_a) or a NaN clamped into the edge cell
// and counted.  A line is 16 unsigned 64-bit words {N, w_a D_b at 1 + 3 a + b, p_res, p_wall, w_left, T, 0, 0}; w is the weight
// vector of the ray's LIST ENTRY (also after reflections into other modes), D the ray's displacement; words 10 .. 12 take the
// ray's final weight W by its end (reservoir, diffuse wall, w_min cut or cap; a miss, a reflection into a dead mode and a no-cast
// ray add nothing).  Every real term is multiplied by a power of two (sK, sP, sT: the host's 2^k), rounded to nearest even
// (rint) and added as an integer in two's complement with atomicAdd(unsigned long long) on global memory; an exact zero is not
// added.  No floating-point atomics, no compare-and-swap loops: the integers are the same bits in any order of the rays.  A
// term above its bound (B_K, B_P, B_T) is left out and counted in the header line; the host reports it.

// nk_freepath.hip's nk_fp_decay
__device__ __forceinline__ void nk_fm_decay(double a, double &g, double &e) {
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
__device__ __forceinline__ void nk_fm_sample(const NkDev &d, uint64_t seed, uint64_t rid, double &x, double &y, double &z) {
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

__device__ __forceinline__ double nk_fm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long nk_fm_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A ray's weights.  end: 0 scattered intrinsically (no start, or reflected into a mode that does not live), 1 reservoir, 2 diffuse
// wall, 3 miss, 4 cap, NK_FM_END_WMIN weight exhausted (code 0 of the public interface, but its W goes to w_left)
#define NK_FM_END_WMIN 5
struct NkFmRay {
    double W, Dx, Dy, Dz, T;
    int end;
};

// a hit after tc: k_free_paths' segment.  sInt += W g and hits += W e are single multiply-adds there (W e is not rounded first)
__device__ __forceinline__ void nk_fm_hit(NkFmRay &c, double tau, double tc, double vx, double vy, double vz, double &sInt, double &sHits) {
#pragma clang fp contract(off)
    double g, e;
    nk_fm_decay(tc / tau, g, e);
    const double wt = (c.W * tau) * g;
    c.Dx = __builtin_fma(wt, vx, c.Dx); c.Dy = __builtin_fma(wt, vy, c.Dy); c.Dz = __builtin_fma(wt, vz, c.Dz);
    c.T = c.T + wt;
    sInt = __builtin_fma(c.W, g, sInt);
    sHits = __builtin_fma(c.W, e, sHits);
    c.W = c.W * e;
}
// a miss: the whole remaining flight, g = 1
__device__ __forceinline__ void nk_fm_miss(NkFmRay &c, double tau, double vx, double vy, double vz, double &sInt) {
#pragma clang fp contract(off)
    const double wt = c.W * tau;
    c.Dx = __builtin_fma(wt, vx, c.Dx); c.Dy = __builtin_fma(wt, vy, c.Dy); c.Dz = __builtin_fma(wt, vz, c.Dz);
    c.T = c.T + wt;
    sInt = sInt + c.W;
}

// The sums a finished ray adds once, with k_free_paths' roundings (D^2 with one multiply-add): v[0..9] += the ray's D[3], D^2[3],
// T, p_res, p_wall, w_left.  Adding +0 where that kernel adds nothing changes no bit: these sums are +0 or positive.
__device__ __forceinline__ void nk_fm_ray_sums(const NkFmRay &c, double *v) {
#pragma clang fp contract(off)
    v[0] = v[0] + c.Dx; v[1] = v[1] + c.Dy; v[2] = v[2] + c.Dz;
    v[3] = __builtin_fma(c.Dx, c.Dx, v[3]); v[4] = __builtin_fma(c.Dy, c.Dy, v[4]); v[5] = __builtin_fma(c.Dz, c.Dz, v[5]);
    v[6] = v[6] + c.T;
    v[7] = v[7] + (c.end == 1 ? c.W : 0.0);
    v[8] = v[8] + (c.end == 2 ? c.W : 0.0);
    v[9] = v[9] + ((c.end == 4 || c.end == NK_FM_END_WMIN) ? c.W : 0.0);
}

// nk_field.hip's nk_field_axis: the field's cell rule along one axis
__device__ __forceinline__ int nk_fm_axis(double x, double lo, double inv_h, int n, bool &clamped) {
#pragma clang fp contract(off)
    const double f = floor((x - lo) * inv_h);
    if (!(f >= 0.0)) { clamped = true; return 0; }                  // (also a NaN coordinate)
    if (f >= (double)n) { clamped = true; return n - 1; }
    return (int)f;
}

// one term into one word: rint(term s) as a two's-complement integer; above the bound (or a NaN) it is left out and counted
__device__ __forceinline__ void nk_fm_add(unsigned long long *w, double term, double s, double B, unsigned int &over) {
#pragma clang fp contract(off)
    if (!(fabs(term) <= B)) { over += 1u; return; }
    const long long q = (long long)rint(term * s);
    if (q != 0) atomicAdd(w, (unsigned long long)q);
}

// a finished ray into the line of its start cell; returns the weight routed to word 10, 11 or 12 (0 where none is)
__device__ __forceinline__ double nk_fm_bin(const NkFreeMapDev &g, int cell, const NkFmRay &c, double wx, double wy, double wz,
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
    else if (c.end == 4 || c.end == NK_FM_END_WMIN) word = NK_FM_WLEFT;
    if (word >= 0) {
        routed = c.W;
        nk_fm_add(w + word, c.W, g.sP, g.BP, ovP);
    }
    nk_fm_add(w + NK_FM_T, c.T, g.sT, g.BT, ovT);
    return routed;
}

template <int GEOM>
__global__ __launch_bounds__(NK_WG) void k_free_map(NkDev d, NkFreeDev f, NkFreeMapDev g) {
    extern __shared__ __align__(16) unsigned char smem[];
    NkLds L;
    nk_lds_setup<GEOM, 0>(d, smem, L);
    const int lane = (int)(threadIdx.x & 63u);
    const int li = __builtin_amdgcn_readfirstlane((int)blockIdx.x * NK_FP_WAVES + (int)(threadIdx.x >> 6));
    if (li >= f.nlist) return;                              // (after the only barrier)
    const int m0 = f.modes ? f.modes[li] : li;
    const double wx = g.weight[3 * (int64_t)li], wy = g.weight[3 * (int64_t)li + 1], wz = g.weight[3 * (int64_t)li + 2];
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
        else nk_fm_sample(d, f.seed, rid, x, y, z);
        if (f.ray_x0) { f.ray_x0[3 * r] = x; f.ray_x0[3 * r + 1] = y; f.ray_x0[3 * r + 2] = z; }
        bool cl = false;
        const int ix = nk_fm_axis(x, g.lo[0], g.inv_h[0], g.n[0], cl);
        const int iy = nk_fm_axis(y, g.lo[1], g.inv_h[1], g.n[1], cl);
        const int iz = nk_fm_axis(z, g.lo[2], g.inv_h[2], g.n[2], cl);
        nClamped += cl ? 1u : 0u;
        const int cell = (ix * g.n[1] + iy) * g.n[2] + iz;
        int mode = m0;
        double vx = f.vg[3 * (int64_t)mode], vy = f.vg[3 * (int64_t)mode + 1], vz = f.vg[3 * (int64_t)mode + 2];
        double tau = f.tau[mode];
        NkFmRay c;
        c.W = 1.0; c.Dx = 0.0; c.Dy = 0.0; c.Dz = 0.0; c.T = 0.0; c.end = 0;
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
                    nk_fm_miss(c, tau, vx, vy, vz, sInt);
                    ++missed;
                    c.end = 3;
                    break;
                }
                nk_fm_hit(c, tau, tc, vx, vy, vz, sInt, sHits);
                ++k;
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
                if (c.W < f.w_min) { c.end = NK_FM_END_WMIN; break; }
                if (k >= f.max_segments) { ++capped; c.end = 4; break; }
            }
        }
        casts += (unsigned long long)ncast;
        nk_fm_ray_sums(c, v);
        const double routed = nk_fm_bin(g, cell, c, wx, wy, wz, ovK, ovP, ovT);
        if (f.ray_D) { f.ray_D[3 * r] = c.Dx; f.ray_D[3 * r + 1] = c.Dy; f.ray_D[3 * r + 2] = c.Dz; }
        if (f.ray_T) f.ray_T[r] = c.T;
        if (f.ray_seg) f.ray_seg[r] = ncast;
        if (f.ray_end) f.ray_end[r] = c.end == NK_FM_END_WMIN ? 0 : c.end;
        if (g.ray_cell) g.ray_cell[r] = cell;
        if (g.ray_w) g.ray_w[r] = routed;
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) v[j] = nk_fm_wave_sum(v[j]);
    sHits = nk_fm_wave_sum(sHits); sInt = nk_fm_wave_sum(sInt);
    casts = nk_fm_wave_sum(casts); missed = nk_fm_wave_sum(missed); capped = nk_fm_wave_sum(capped);
    const unsigned long long nc = nk_fm_wave_sum((unsigned long long)nClamped), oK = nk_fm_wave_sum((unsigned long long)ovK);
    const unsigned long long oP = nk_fm_wave_sum((unsigned long long)ovP), oT = nk_fm_wave_sum((unsigned long long)ovT);
    if (lane == 0) {
        double *row = f.rows + (int64_t)li * NK_FP_ROW;
        row[0] = v[0]; row[1] = v[1]; row[2] = v[2]; row[3] = v[3]; row[4] = v[4]; row[5] = v[5];
        row[6] = v[6]; row[7] = sHits; row[8] = v[7]; row[9] = v[8]; row[10] = v[9]; row[11] = sInt;
        unsigned long long *cnt = f.counts + (int64_t)li * NK_FP_CNT;
        cnt[0] = casts; cnt[1] = missed; cnt[2] = capped; cnt[3] = 0ull;
        unsigned long long *hdr = g.grid + (size_t)g.ncells * NK_FREE_MAP_LINE;
        if (nc) atomicAdd(hdr + NK_FM_CLAMPED, nc);
        if (oK) atomicAdd(hdr + NK_FM_OVK, oK);
        if (oP) atomicAdd(hdr + NK_FM_OVP, oP);
        if (oT) atomicAdd(hdr + NK_FM_OVT, oT);
    }
}

// the dispatch of NK_GEOM_LAUNCH (nk_engine.hip): the geometry mode picks the instantiation
hipError_t nk_free_map_launch(const NkDev &d, const NkFreeDev &f, const NkFreeMapDev &g, int geom, size_t lds, hipStream_t stream) {
    if (f.nlist <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((f.nlist + NK_FP_WAVES - 1) / NK_FP_WAVES);
    if (geom == 1) k_free_map<1><<<grid, NK_WG, lds, stream>>>(d, f, g);
    else k_free_map<2><<<grid, NK_WG, lds, stream>>>(d, f, g);
    return hipGetLastError();
}

// nk_freepath.hip -- free-path sampling of the geometry-limited conductivity (nk_free_paths): k_free_paths<GEOM> and its launch.
// The C entry points (nk_free_paths, nk_free_paths_info) are in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds
// k_free_paths<1> and k_free_paths<2> and nothing else (the trick of nk_modes.hip).
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_freepath.h"

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
// bits depend on the mode, n and the seed (or x0) alone, not on the grid nor on the other modes of the list.

// g = -expm1(-a) and e = exp(-a), a >= 0.  Up to 1/8 the series a (1 - a/2 + a^2/6 - ...) through a^10 / 11! (the next term is
// 2.4e-19 of the first); 1 - exp(-a) would lose the digits of a there (three of them at a = 2.5e-3, the common case: a flight
// across a 200 A box against a lifetime of 1e3 ps).
__device__ __forceinline__ void nk_fp_decay(double a, double &g, double &e) {
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

// One draw of Mesh.sample_volume (Mesh.py:890-904) as k_init_particles makes it ('random_domain'), keyed by the ray id.
__device__ __forceinline__ void nk_fp_sample(const NkDev &d, uint64_t seed, uint64_t rid, double &x, double &y, double &z) {
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

__device__ __forceinline__ double nk_fp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long nk_fp_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int GEOM>
__global__ __launch_bounds__(NK_WG) void k_free_paths(NkDev d, NkFreeDev f) {
    extern __shared__ __align__(16) unsigned char smem[];
    NkLds L;
    nk_lds_setup<GEOM, 0>(d, smem, L);
    const int lane = (int)(threadIdx.x & 63u);
    const int li = __builtin_amdgcn_readfirstlane((int)blockIdx.x * NK_FP_WAVES + (int)(threadIdx.x >> 6));
    if (li >= f.nlist) return;                              // (after the only barrier)
    const int m0 = f.modes ? f.modes[li] : li;
    double sDx = 0.0, sDy = 0.0, sDz = 0.0, qDx = 0.0, qDy = 0.0, qDz = 0.0, sT = 0.0;
    double sHits = 0.0, sRes = 0.0, sWall = 0.0, sLeft = 0.0, sInt = 0.0;
    unsigned long long casts = 0ull, missed = 0ull, capped = 0ull;
    for (int s0 = 0; s0 < f.n; s0 += 64) {
        const int s = s0 + lane;
        if (s >= f.n) continue;
        const int64_t r = (int64_t)li * f.n + s;
        const uint64_t rid = ((uint64_t)(uint32_t)m0 << 32) | (uint64_t)(uint32_t)s;
        double x, y, z;
        if (f.x0) { x = f.x0[3 * r]; y = f.x0[3 * r + 1]; z = f.x0[3 * r + 2]; }
        else nk_fp_sample(d, f.seed, rid, x, y, z);
        if (f.ray_x0) { f.ray_x0[3 * r] = x; f.ray_x0[3 * r + 1] = y; f.ray_x0[3 * r + 2] = z; }
        int mode = m0;
        double vx = f.vg[3 * (int64_t)mode], vy = f.vg[3 * (int64_t)mode + 1], vz = f.vg[3 * (int64_t)mode + 2];
        double tau = f.tau[mode];
        double W = 1.0, Dx = 0.0, Dy = 0.0, Dz = 0.0, T = 0.0;
        int k = 0, ncast = 0, end = 0;
        if (!(tau > 0.0) || (vx == 0.0 && vy == 0.0 && vz == 0.0)) {
            T = tau > 0.0 ? tau : 0.0;
            sInt += W;
        } else {
            for (;;) {
                double tc;
                int fc;
                NK_RAY(GEOM, d, L, NK_TREE_NO_SKIP, x, y, z, vx, vy, vz, tc, fc);
                ++ncast;
                if (fc < 0) {                               // a miss: the whole remaining flight, g = 1
                    const double wt = W * tau;
                    Dx += wt * vx; Dy += wt * vy; Dz += wt * vz; T += wt;
                    sInt += W;
                    ++missed;
                    end = 3;
                    break;
                }
                double g, e;
                nk_fp_decay(tc / tau, g, e);
                const double wt = W * tau * g;
                Dx += wt * vx; Dy += wt * vy; Dz += wt * vz; T += wt;
                sInt += W * g;
                W *= e;
                ++k;
                sHits += W;
                const NkFacet *fp = L.facets + fc;
                const int bc = fp->bc;
                if (bc == 'T' || bc == 'F') { sRes += W; end = 1; break; }
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
                    if (!spec) { sWall += W; end = 2; break; }
                    if (d.degen_j2) {
                        const int j2 = d.degen_j2[out];
                        if (j2 > -1 && j2 < d.J && r1 >= 0.5) out = (out / d.J) * d.J + j2;
                    }
                    mode = out;
                    vx = f.vg[3 * (int64_t)mode]; vy = f.vg[3 * (int64_t)mode + 1]; vz = f.vg[3 * (int64_t)mode + 2];
                    tau = f.tau[mode];
                    x = hx; y = hy; z = hz;
                    if (!(tau > 0.0)) { sInt += W; end = 0; break; }     // reflected into a mode that does not live
                }
                if (W < f.w_min) { sLeft += W; end = 0; break; }
                if (k >= f.max_segments) { sLeft += W; ++capped; end = 4; break; }
            }
        }
        casts += (unsigned long long)ncast;
        sDx += Dx; sDy += Dy; sDz += Dz;
        qDx += Dx * Dx; qDy += Dy * Dy; qDz += Dz * Dz;
        sT += T;
        if (f.ray_D) { f.ray_D[3 * r] = Dx; f.ray_D[3 * r + 1] = Dy; f.ray_D[3 * r + 2] = Dz; }
        if (f.ray_T) f.ray_T[r] = T;
        if (f.ray_seg) f.ray_seg[r] = ncast;
        if (f.ray_end) f.ray_end[r] = end;
    }
    sDx = nk_fp_wave_sum(sDx); sDy = nk_fp_wave_sum(sDy); sDz = nk_fp_wave_sum(sDz);
    qDx = nk_fp_wave_sum(qDx); qDy = nk_fp_wave_sum(qDy); qDz = nk_fp_wave_sum(qDz);
    sT = nk_fp_wave_sum(sT); sHits = nk_fp_wave_sum(sHits); sRes = nk_fp_wave_sum(sRes);
    sWall = nk_fp_wave_sum(sWall); sLeft = nk_fp_wave_sum(sLeft); sInt = nk_fp_wave_sum(sInt);
    casts = nk_fp_wave_sum(casts); missed = nk_fp_wave_sum(missed); capped = nk_fp_wave_sum(capped);
    if (lane == 0) {
        double *row = f.rows + (int64_t)li * NK_FP_ROW;
        row[0] = sDx; row[1] = sDy; row[2] = sDz; row[3] = qDx; row[4] = qDy; row[5] = qDz;
        row[6] = sT; row[7] = sHits; row[8] = sRes; row[9] = sWall; row[10] = sLeft; row[11] = sInt;
        unsigned long long *cnt = f.counts + (int64_t)li * NK_FP_CNT;
        cnt[0] = casts; cnt[1] = missed; cnt[2] = capped; cnt[3] = 0ull;
    }
}

// the dispatch of NK_GEOM_LAUNCH (nk_engine.hip): the geometry mode picks the instantiation
hipError_t nk_free_paths_launch(const NkDev &d, const NkFreeDev &f, int geom, size_t lds, hipStream_t stream) {
    if (f.nlist <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((f.nlist + NK_FP_WAVES - 1) / NK_FP_WAVES);
    if (geom == 1) k_free_paths<1><<<grid, NK_WG, lds, stream>>>(d, f);
    else k_free_paths<2><<<grid, NK_WG, lds, stream>>>(d, f);
    return hipGetLastError();
}

// nk_flight.h -- the flight of a free-path ray, stated once: what k_free_paths<GEOM, MAP> (nk_freepath.hip) and
// k_free_columns<GEOM, KT> (nk_freecols.hip) share.  Device code; included by those two translation units only, after nk_kernels.h.
//
// The arithmetic of a ray's weights is DEFINED here, rounding by rounding: the fused multiply-adds are written as __builtin_fma and
// everything else is kept from fusing (#pragma clang fp contract(off)).  `p_int += W g`, `hits += W e`, `D += wt v` and
// `D2 += D D` are fused; `wt = (W tau) g`, `T += wt`, `W *= e` and the sums a finished ray adds once are not.  Every kernel
// compiles this text, so the plain call, a map call and any column of a column call give the same bits whatever the compiler
// makes of the code around it (DESIGN.md "Free-path sweeps").
#pragma once
#include "nk_freepath.h"

// g = -expm1(-a) and e = exp(-a), a >= 0.  Up to 1/8 the series a (1 - a/2 + a^2/6 - ...) through a^10 / 11! (the next term is
// 2.4e-19 of the first); 1 - exp(-a) would lose the digits of a there (three of them at a = 2.5e-3, the common case: a flight
// across a 200 A box against a lifetime of 1e3 ps).  Above 1/8, 1 - nk_exp(-a) for every a up to +inf: nk_exp returns +0 below its
// underflow point however far (it clamps its argument), so a positive lifetime of 5e-324 gives e = +0, g = 1 like any other that
// the flight outlasts.  a is never NaN or negative here: tau > 0 and finite (nk_free_refuse), tc >= 0 from a cast that hit.
// The seam a = 1/8 belongs to the series; both sides are good to 3e-18 there (tests/free_path_edge_cases.py 'seam').
__device__ __forceinline__ void nk_fl_decay(double a, double &g, double &e) {
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

// One draw of Mesh.sample_volume (Mesh.py:890-904) as k_init_particles makes it ('random_domain'), keyed by the ray id.
__device__ __forceinline__ void nk_fl_sample(const NkDev &d, uint64_t seed, uint64_t rid, double &x, double &y, double &z) {
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

// the sum over the 64 lanes of a wave, in every lane: a butterfly (xor 32, 16, .., 1)
__device__ __forceinline__ double nk_fl_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long nk_fl_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A ray's weights (in a column call: one column's).  end: 0 scattered intrinsically (no start, or reflected into a mode that does
// not live), 1 reservoir, 2 diffuse wall, 3 miss, 4 cap, NK_FL_END_WMIN weight exhausted (code 0 of the public interface --
// nk_fl_end_code --, but its W goes to w_left)
#define NK_FL_END_WMIN 5
struct NkFlRay {
    double W, Dx, Dy, Dz, T;
    int end;
};
__device__ __forceinline__ void nk_fl_start(NkFlRay &c) { c.W = 1.0; c.Dx = 0.0; c.Dy = 0.0; c.Dz = 0.0; c.T = 0.0; c.end = 0; }
__device__ __forceinline__ int nk_fl_end_code(const NkFlRay &c) { return c.end == NK_FL_END_WMIN ? 0 : c.end; }

// a hit after tc: a = tc / tau, g = -expm1(-a), e = exp(-a);  D += W tau g v, T += W tau g, p_int += W g, hits += W e;  W *= e
// (W e is not rounded before it is added to hits)
__device__ __forceinline__ void nk_fl_hit(NkFlRay &c, double tau, double tc, double vx, double vy, double vz, double &sInt, double &sHits) {
#pragma clang fp contract(off)
    double g, e;
    nk_fl_decay(tc / tau, g, e);
    const double wt = (c.W * tau) * g;
    c.Dx = __builtin_fma(wt, vx, c.Dx); c.Dy = __builtin_fma(wt, vy, c.Dy); c.Dz = __builtin_fma(wt, vz, c.Dz);
    c.T = c.T + wt;
    sInt = __builtin_fma(c.W, g, sInt);
    sHits = __builtin_fma(c.W, e, sHits);
    c.W = c.W * e;
}
// a miss: the whole remaining flight, g = 1
__device__ __forceinline__ void nk_fl_miss(NkFlRay &c, double tau, double vx, double vy, double vz, double &sInt) {
#pragma clang fp contract(off)
    const double wt = c.W * tau;
    c.Dx = __builtin_fma(wt, vx, c.Dx); c.Dy = __builtin_fma(wt, vy, c.Dy); c.Dz = __builtin_fma(wt, vz, c.Dz);
    c.T = c.T + wt;
    sInt = sInt + c.W;
}

// The sums a finished ray adds once (D^2 with one multiply-add): v[0..9] += the ray's D[3], D^2[3], T, p_res, p_wall, w_left.
// Adding +0 where the ray adds nothing changes no bit: these sums are +0 or positive.
__device__ __forceinline__ void nk_fl_ray_sums(const NkFlRay &c, double *v) {
#pragma clang fp contract(off)
    v[0] = v[0] + c.Dx; v[1] = v[1] + c.Dy; v[2] = v[2] + c.Dz;
    v[3] = __builtin_fma(c.Dx, c.Dx, v[3]); v[4] = __builtin_fma(c.Dy, c.Dy, v[4]); v[5] = __builtin_fma(c.Dz, c.Dz, v[5]);
    v[6] = v[6] + c.T;
    v[7] = v[7] + (c.end == 1 ? c.W : 0.0);
    v[8] = v[8] + (c.end == 2 ? c.W : 0.0);
    v[9] = v[9] + ((c.end == 4 || c.end == NK_FL_END_WMIN) ? c.W : 0.0);
}
// a mode's row from the wave sums of v[0..9], hits and p_int
__device__ __forceinline__ void nk_fl_store_row(double *row, const double *v, double hits, double pint) {
    row[0] = v[0]; row[1] = v[1]; row[2] = v[2]; row[3] = v[3]; row[4] = v[4]; row[5] = v[5];
    row[6] = v[6]; row[7] = hits; row[8] = v[7]; row[9] = v[8]; row[10] = v[9]; row[11] = pint;
}

// What facet fc, met after tc as the ray's k-th hit, makes of the ray: 1 a reservoir ends it, 2 a diffuse reflection ends it, 0
// it goes on -- from the hit point moved by a periodic facet's translation, or from the hit point in the mode a specular
// reflection leads to (`turned`: mode and v are new, the caller reads the new lifetime).  A rough facet draws
// (r0, r1) = nk_uniform2_dev(seed, ray id, k, NK_TAG_FREE + 3): specular iff true_spec && r0 <= specularity (nk_reflect's test; and
// the specular map names a mode), into spec_map's mode or, when degen_j2 names one and r1 >= 0.5, its degenerate partner.
// k_free_columns calls this; k_free_paths carries the same statements inline, where the call measured 2 % slower
// (profiles/free_flight_notes.txt) -- a change of the step is made in both places.
__device__ __forceinline__ int nk_fl_facet(const NkDev &d, const NkLds &L, const NkFreeDev &f, int fc, double tc, uint64_t rid, int k,
                                           double &x, double &y, double &z, double &vx, double &vy, double &vz, int &mode, bool &turned) {
    turned = false;
    const NkFacet *fp = L.facets + fc;
    const int bc = fp->bc;
    if (bc == 'T' || bc == 'F') return 1;
    const double hx = __builtin_fma(tc, vx, x), hy = __builtin_fma(tc, vy, y), hz = __builtin_fma(tc, vz, z);
    if (bc == 'P') {
        x = hx + fp->tx; y = hy + fp->ty; z = hz + fp->tz;
        return 0;
    }
    double r0, r1;
    nk_uniform2_dev(f.seed, rid, (uint32_t)k, NK_TAG_FREE + 3u, r0, r1);
    const int rough = fp->rough;
    bool spec = false;
    int out = -1;
    if (rough >= 0 && rough < d.Fr) {                       // (the host refuses 'R' facets without tables)
        const int64_t idx = (int64_t)rough * d.M + mode;
        out = d.spec_map[idx];
        spec = d.true_spec[idx] && r0 <= d.specularity[idx] && out >= 0 && out < d.M;
    }
    if (!spec) return 2;
    if (d.degen_j2) {
        const int j2 = d.degen_j2[out];
        if (j2 > -1 && j2 < d.J && r1 >= 0.5) out = (out / d.J) * d.J + j2;
    }
    mode = out;
    vx = f.vg[3 * (int64_t)mode]; vy = f.vg[3 * (int64_t)mode + 1]; vz = f.vg[3 * (int64_t)mode + 2];
    x = hx; y = hy; z = hz;
    turned = true;
    return 0;
}

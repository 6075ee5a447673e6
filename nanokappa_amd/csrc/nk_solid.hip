// nk_solid.hip -- exact volume of solid in every cell of a field grid (nk_cell_solid_volume): k_solid_clip, k_solid_finish,
// their launches and the host side of the call.  No context: a set-up helper like nk_mesh_crossings.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/nanokappa_hip.h"
#include "nk_field.h"            // nk_field_k
#include "nk_solid.h"

// =================================================================================== the rule
// V[c] = volume of solid in cell c of the grid lo / h / n (cell (ix * ny + iy) * nz + iz), for a closed triangle mesh with
// outward normals, exact for the triangles: integrate the length of solid along x over the cell's (y, z) square.  A ray along
// x leaves the solid through faces with n_x > 0 and enters through faces with n_x < 0; the length inside the cell's x slab is
// the sum over the crossings of +-(x - x_lo) for a crossing in the slab, +-h_x for one beyond it, 0 for one before it.  Per
// (triangle, cell), with the triangle clipped to the cell (Sutherland-Hodgman against closed slabs, in the order y_lo, y_hi,
// z_lo, z_hi, x_lo, x_hi):
//   a = signed area of the clipped polygon's projection on the yz plane (positive where n_x > 0),
//   p = integral of (x - x_lo) dy dz over it: per fan triangle (vertex 0, i, i + 1) a_i ((x_0 + x_i + x_{i+1}) / 3 - x_lo),
//   A[c] += a, P[c] += p;  V[ix] = P[ix] + h_x sum_{ix' > ix} A[ix']   (an exclusive suffix sum per (iy, iz) column).
// All of it in GRID UNITS u = (x - lo) / h (the host divides, once): a cell is the unit cube [i, i + 1]^3, |a| <= 1, |p| <= 1,
// V is in cells until k_solid_finish multiplies by h_x h_y h_z.  A triangle is offered to the cells floor(u) of its bounding
// box, clamped into [0, n), and clipped against the integers i and i + 1 -- the numbers floor() compares with -- so a face
// lying in a grid plane perpendicular to x is counted in exactly one cell, and one in the grid's upper x boundary in the last.
// nanokappa_amd/field.py solid_volume is the same rule in NumPy, operation by operation (this file is compiled without
// multiply-add contraction so that the terms a and p are the same doubles there and here).
// The sums are 64-bit integers, the project's idiom (nk_field.hip): a 2^k_A and p 2^k_P rounded to nearest and added in two's
// complement, so V is the same bits from call to call whatever the order of the adds.  A cell receives at most one term per
// triangle, each at most 1, and so does a column's suffix sum (a triangle's pieces in one column do not overlap in the
// projection): k = nk_field_k(1, n_faces) keeps every sum below 2^62.

// A lane's polygon in LDS: coordinate c of vertex v at [(v * 3 + c) * NK_SOLID_WG] from the lane's own first word -- the
// lanes of the wave read and write consecutive words.  (Private arrays indexed by a loop variable would live in scratch.)
#define NK_SOLID_AT(b, v, c) (b)[((v) * 3 + (c)) * NK_SOLID_WG]

// One Sutherland-Hodgman step: the polygon src (ns vertices) against coordinate AXIS >= bound (LOWER) or <= bound, the plane
// itself inside; every vertex of the result goes to emit(x, y, z), at most CAP of them (a convex polygon gains one vertex per
// plane at most; CAP keeps a polygon that rounding has made non-convex from gaining more -- field.py truncates alike).
template <int AXIS, bool LOWER, int CAP, class Emit>
__host__ __device__ __forceinline__ void nk_solid_clip(const double *src, int ns, double bound, Emit &emit) {
    if (ns <= 0) return;
    double cx = NK_SOLID_AT(src, 0, 0), cy = NK_SOLID_AT(src, 0, 1), cz = NK_SOLID_AT(src, 0, 2);
    const double c0 = AXIS == 0 ? cx : AXIS == 1 ? cy : cz;
    double dc = LOWER ? c0 - bound : bound - c0;
    int out = 0;
    for (int i = 0; i < ns; ++i) {
        const int j = i + 1 < ns ? i + 1 : 0;                  // (the last edge closes the polygon)
        const double nx = NK_SOLID_AT(src, j, 0), ny = NK_SOLID_AT(src, j, 1), nz = NK_SOLID_AT(src, j, 2);
        const double n0 = AXIS == 0 ? nx : AXIS == 1 ? ny : nz;
        const double dn = LOWER ? n0 - bound : bound - n0;
        const bool in_c = dc >= 0.0, in_n = dn >= 0.0;
        if (in_c && out < CAP) { emit(cx, cy, cz); ++out; }
        if (in_c != in_n && out < CAP) {
            const double t = dc / (dc - dn);
            const double qx = AXIS == 0 ? bound : cx + t * (nx - cx);
            const double qy = AXIS == 1 ? bound : cy + t * (ny - cy);
            const double qz = AXIS == 2 ? bound : cz + t * (nz - cz);
            emit(qx, qy, qz);
            ++out;
        }
        cx = nx; cy = ny; cz = nz; dc = dn;
    }
}

// emit into a lane's polygon in LDS
struct NkSolidStore {
    double *dst;
    int n;
    __host__ __device__ __forceinline__ void operator()(double x, double y, double z) {
        NK_SOLID_AT(dst, n, 0) = x; NK_SOLID_AT(dst, n, 1) = y; NK_SOLID_AT(dst, n, 2) = z;
        ++n;
    }
};
// emit into the fan sums a and p (x_lo: the cell's lower x)
struct NkSolidFan {
    double x_lo;
    double x0, y0, z0, px, py, pz, a, p;
    int n;
    __host__ __device__ __forceinline__ void operator()(double x, double y, double z) {
        if (n == 0) { x0 = x; y0 = y; z0 = z; }
        else if (n >= 2) {
            const double ai = 0.5 * ((py - y0) * (z - z0) - (y - y0) * (pz - z0));
            const double pi = ai * ((x0 + px + x) / 3.0 - x_lo);
            a = a + ai;
            p = p + pi;
        }
        if (n >= 1) { px = x; py = y; pz = z; }
        ++n;
    }
};

// Work item w = (triangle, yz column of its cell range): clip to the column once, then walk the triangle's x cells.  pa, pb: the
// lane's two polygons.  (Also compiled for the host, where a stand-alone program can run it pair by pair.)
__host__ __device__ __forceinline__ void nk_solid_pair(const NkSolidDev &s, int64_t w, double *pa, double *pb) {
    int lo = 0, hi = s.nf;                                // the triangle of pair w: first[lo] <= w < first[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (s.first[mid] <= w) lo = mid; else hi = mid;
    }
    const int t = lo;
    const int32_t *r = s.rng + (size_t)t * 6;
    const int64_t local = w - s.first[t];
    const int dz = r[5] - r[2] + 1;
    const int iy = r[1] + (int)(local / dz), iz = r[2] + (int)(local % dz);
    if (local < 0 || iy > r[4]) return;                   // (cannot happen: first[] counts exactly the columns)
    const double *tv = s.tri + (size_t)t * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) NK_SOLID_AT(pa, k / 3, k % 3) = tv[k];
    NkSolidStore st;
    st.dst = pb; st.n = 0; nk_solid_clip<1, true, 4>(pa, 3, (double)iy, st);
    int ns = st.n;
    st.dst = pa; st.n = 0; nk_solid_clip<1, false, 5>(pb, ns, (double)iy + 1.0, st);
    ns = st.n;
    st.dst = pb; st.n = 0; nk_solid_clip<2, true, 6>(pa, ns, (double)iz, st);
    ns = st.n;
    st.dst = pa; st.n = 0; nk_solid_clip<2, false, 7>(pb, ns, (double)iz + 1.0, st);
    ns = st.n;
    if (ns < 3) return;
    for (int ix = r[0]; ix <= r[3]; ++ix) {
        st.dst = pb; st.n = 0; nk_solid_clip<0, true, 8>(pa, ns, (double)ix, st);
        if (st.n < 3) continue;
        NkSolidFan fan;
        fan.x_lo = (double)ix; fan.a = 0.0; fan.p = 0.0; fan.n = 0;
        fan.x0 = fan.y0 = fan.z0 = fan.px = fan.py = fan.pz = 0.0;
        nk_solid_clip<0, false, 9>(pb, st.n, (double)ix + 1.0, fan);
        const size_t c = ((size_t)ix * s.n[1] + iy) * s.n[2] + iz;        // ix, iy, iz lie in the clamped ranges: c < ncells
        const long long qa = (long long)rint(fan.a * s.sA), qp = (long long)rint(fan.p * s.sP);
#if defined(__HIP_DEVICE_COMPILE__)
        if (qa) atomicAdd(s.A + c, (unsigned long long)qa);
        if (qp) atomicAdd(s.P + c, (unsigned long long)qp);
#else
        s.A[c] += (unsigned long long)qa;
        s.P[c] += (unsigned long long)qp;
#endif
    }
}
__global__ __launch_bounds__(NK_SOLID_WG) void k_solid_clip(NkSolidDev s) {
    __shared__ double lds[2 * NK_SOLID_MAXV * 3 * NK_SOLID_WG];
    const int64_t w = (int64_t)blockIdx.x * NK_SOLID_WG + threadIdx.x;
    if (w >= s.pairs) return;                             // (no barrier below: a lane's polygons are its own)
    double *pa = lds + threadIdx.x;
    nk_solid_pair(s, w, pa, pa + NK_SOLID_MAXV * 3 * NK_SOLID_WG);
}

// One lane per (iy, iz) column, from the last x cell to the first: V = (P + sum of A beyond the cell) cell volume
__global__ __launch_bounds__(256) void k_solid_finish(const unsigned long long *A, const unsigned long long *P, int nx, int nyz,
                                                      double iA, double iP, double cellvol, double *V) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nyz) return;
    long long beyond = 0;
    for (int ix = nx - 1; ix >= 0; --ix) {
        const size_t c = (size_t)ix * nyz + j;
        V[c] = ((double)(long long)P[c] * iP + (double)beyond * iA) * cellvol;
        beyond += (long long)A[c];
    }
}

// =================================================================================== host side
static thread_local std::string g_solid_error;

// how far outside the grid, in cells, a vertex may lie through the rounding of (x - lo) / h (it is moved onto the boundary)
static const double NK_SOLID_SNAP = 1e-9;

static int nk_solid_fail(int rc, const std::string &msg) { g_solid_error = "nk_cell_solid_volume: " + msg; return rc; }

// The triangles in grid units, the cells offered to each and the first (triangle, column) pair of each (first[n_faces] = pairs);
// NK_ERR_ARG, with the text set, where the grid does not contain them.  (h > 0 and n > 0 have been checked.)
static int nk_solid_prepare(int64_t n_faces, const double *tri, const double lo[3], const double h[3], const int32_t n[3],
                            std::vector<double> &u, std::vector<int32_t> &rng, std::vector<int64_t> &first) {
    // grid units, the cells offered to every triangle, and the (triangle, column) pairs
    const size_t nf = (size_t)n_faces;
    u.resize(nf * 9); rng.resize(nf * 6); first.resize(nf + 1);
    int64_t pairs = 0;
    for (size_t t = 0; t < nf; ++t) {
        double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int v = 0; v < 3; ++v)
            for (int a = 0; a < 3; ++a) {
                double x = (tri[t * 9 + v * 3 + a] - lo[a]) / h[a];
                if (!(x >= -NK_SOLID_SNAP && x <= (double)n[a] + NK_SOLID_SNAP))               // (false for a NaN as well)
                    return nk_solid_fail(NK_ERR_ARG, "the grid does not contain the bounding box of the triangles (triangle " + std::to_string(t) +
                                         ", vertex " + std::to_string(v) + ", axis " + std::to_string(a) + " lies at " + std::to_string(x) + " cells of " + std::to_string(n[a]) + ")");
                x = std::min(std::max(x, 0.0), (double)n[a]);
                u[t * 9 + v * 3 + a] = x;
                mn[a] = std::min(mn[a], x); mx[a] = std::max(mx[a], x);
            }
        for (int a = 0; a < 3; ++a) {
            rng[t * 6 + a] = std::min((int32_t)floor(mn[a]), n[a] - 1);
            rng[t * 6 + 3 + a] = std::min((int32_t)floor(mx[a]), n[a] - 1);
        }
        first[t] = pairs;
        pairs += (int64_t)(rng[t * 6 + 4] - rng[t * 6 + 1] + 1) * (rng[t * 6 + 5] - rng[t * 6 + 2] + 1);
    }
    first[nf] = pairs;
    return NK_OK;
}

extern "C" {

const char *nk_solid_last_error(void) { return g_solid_error.c_str(); }

int nk_cell_solid_volume(int device, int64_t n_faces, const double *tri, const double lo[3], const double h[3], const int32_t n[3],
                         double *V, nk_solid_report *rep) {
    g_solid_error.clear();
    if (rep) memset(rep, 0, sizeof(*rep));
    if (n_faces <= 0) return nk_solid_fail(NK_ERR_ARG, "n_faces = " + std::to_string((long long)n_faces) + ": the mesh needs at least one triangle");
    if (n_faces > (1ll << 30)) return nk_solid_fail(NK_ERR_ARG, "n_faces = " + std::to_string((long long)n_faces) + " is more than 2^30");
    if (!tri || !lo || !h || !n || !V) return nk_solid_fail(NK_ERR_ARG, "NULL argument");
    for (int a = 0; a < 3; ++a)
        if (!(h[a] > 0.0) || !std::isfinite(h[a]) || !std::isfinite(lo[a])) return nk_solid_fail(NK_ERR_ARG, "the cell sizes h must be positive");
    const int64_t nc = (int64_t)n[0] * n[1] * n[2];
    if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0 || nc > (1ll << 24))
        return nk_solid_fail(NK_ERR_ARG, "the grid needs 1 .. 2^24 cells, not " + std::to_string(n[0]) + " x " + std::to_string(n[1]) + " x " + std::to_string(n[2]));
    std::vector<double> u;
    std::vector<int32_t> rng;
    std::vector<int64_t> first;
    if (nk_solid_prepare(n_faces, tri, lo, h, n, u, rng, first)) return NK_ERR_ARG;
    const size_t nf = (size_t)n_faces;
    const int64_t pairs = first[nf];
    const int64_t nwg = (pairs + NK_SOLID_WG - 1) / NK_SOLID_WG;
    if (nwg > 0x7fffffffll) return nk_solid_fail(NK_ERR_ARG, std::to_string((long long)pairs) + " (triangle, column) pairs are more than one launch takes");
    // the device
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return nk_solid_fail(NK_ERR_NODEVICE, std::string("no HIP device available (") + hipGetErrorString(e) + "); this library has no CPU fallback");
    if (device < 0 || device >= ndev) return nk_solid_fail(NK_ERR_ARG, "device out of range");
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return nk_solid_fail(NK_ERR_HIP, hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return nk_solid_fail(NK_ERR_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    const int kA = nk_field_k(1.0, n_faces), kP = kA;          // |a| <= 1 and |p| <= 1 in grid units, n_faces terms per sum at most
    const size_t ub = nf * 9 * sizeof(double), rb = nf * 6 * sizeof(int32_t), fb = (nf + 1) * sizeof(int64_t), gb = (size_t)nc * 8;
    char *buf = nullptr;                                         // {A, P, V, tri, first, rng}: every part a multiple of 8 bytes but the last
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    e = hipMalloc((void **)&buf, 3 * gb + ub + fb + rb);
    if (e != hipSuccess) return nk_solid_fail(NK_ERR_HIP, "allocating " + std::to_string((unsigned long long)(3 * gb + ub + fb + rb)) + " bytes: " + hipGetErrorString(e));
    NkSolidDev s;
    s.A = (unsigned long long *)buf;
    s.P = (unsigned long long *)(buf + gb);
    double *dV = (double *)(buf + 2 * gb);
    s.tri = (const double *)(buf + 3 * gb);
    s.first = (const int64_t *)(buf + 3 * gb + ub);
    s.rng = (const int32_t *)(buf + 3 * gb + ub + fb);
    s.pairs = pairs; s.nf = (int32_t)n_faces;
    for (int a = 0; a < 3; ++a) s.n[a] = n[a];
    s.sA = ldexp(1.0, kA); s.sP = ldexp(1.0, kP);
    float ms = 0.0f;
    e = hipMemset(buf, 0, 2 * gb);
    if (e == hipSuccess) e = hipMemcpy((void *)s.tri, u.data(), ub, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)s.first, first.data(), fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)s.rng, rng.data(), rb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, 0);
    if (e == hipSuccess) {
        k_solid_clip<<<(unsigned)nwg, NK_SOLID_WG, 0, 0>>>(s);
        const int nyz = n[1] * n[2];
        k_solid_finish<<<(nyz + 255) / 256, 256, 0, 0>>>(s.A, s.P, n[0], nyz, ldexp(1.0, -kA), ldexp(1.0, -kP), h[0] * h[1] * h[2], dV);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev1, 0);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    if (e == hipSuccess) e = hipMemcpy(V, dV, gb, hipMemcpyDeviceToHost);
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    hipFree(buf);
    if (e != hipSuccess) return nk_solid_fail(NK_ERR_HIP, hipGetErrorString(e));
    if (rep) { rep->ncells = nc; rep->pairs = pairs; rep->k_A = kA; rep->k_P = kP; rep->seconds = 1e-3 * (double)ms; }
    return NK_OK;
}

}  // extern "C"

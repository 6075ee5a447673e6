// nk_field.hip -- spatial field maps, plain and per group of modes: the kernel k_field<STATE, GROUPED>, its helpers, their
// launches and the derivation of the integer scales.  The C entry points (nk_set_field, nk_get_field, nk_tally_field_state,
// nk_field_info and their nk_*_field_groups* counterparts) are in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds the
// four instantiations of k_field, k_field_accum, k_field_finish and k_field_permute and nothing else.
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_field.h"
#include "nk_kind.h"

// LDS a launch may ask for on gfx950 (160 KB per CU; above 64 KB nk_allow_lds has to allow it per kernel)
static const size_t NK_FIELD_LDS_MAX = 160 * 1024;
// bins of one line in LDS: E, Fx, Fy, Fz (u64) + N (u32)
static const size_t NK_FIELD_LDS_LINE = 36;

// =================================================================================== the kernels
// The reference shows WHERE the heat goes with a scatter of every particle (Population.plot_figures, Population.py:1841-1979,
// called at :123 and every 100 steps at :1735).  The engine's counterpart is a field: a uniform grid lo / h / n over the
// geometry's bounding box, independent of the subvolumes, with five sums per cell -- N (particles), E = sum e, F = sum v e.
// k_field is a pass of its own over the store, which it only reads, with the two modes of k_spectral:
//   STATE = false (step mode): right after the sweep of a field step (and k_events_end / k_deliver); e = nk_tally_e against
//     the subvolume temperatures the sweep used, so the cells and the step's history row are sums of the same terms.
//   STATE = true: a snapshot, e against the occupation at the particle's interpolated temperature, as k_spectral<true>.
// Cell (ix, iy, iz), ix = floor((x - lo_x) * inv_h_x); an index outside [0, n) is CLAMPED into the edge cell (the store holds
// particles a hair outside the box: just behind a reservoir face, escapees waiting for contains_check -- the slice classifier
// puts those into the end slices too) and counted in the header's `clamped`.
// The sums are 64-BIT INTEGERS: every real term is scaled by a power of two (sE for e, sF for v e: the host's 2^k_E, 2^k_F,
// below), rounded to nearest (rint) and added as int64 in two's complement.  Integer adds commute, so a field is the same bits
// from run to run, for any grid of workgroups, on either path below, and on any split of the particles over ranks.
// A term above its bound (B_E, B_F) is NOT added: it raises the header's overflow counts and the host reports it.
// GROUPED = true: k_field says WHERE the heat goes, summed over all modes; k_spectral / k_modes say WHICH modes carry it, per
// subvolume.  The grouped pass does both at once: the five sums per (cell, group), group = group_of_mode[mode] from a table of
// the caller's (a frequency bin, a branch, a mean-free-path bin, a direction bin; -1 = in no group).  Same launch shape, modes,
// cell rule, integers and paths, so for a table that groups every mode the sums over the groups of a cell ARE the field's
// integers.  A particle of group -1 is added nowhere and counted in the header's `ungrouped`.
// The group of a particle must not cost a chain of dependent loads (k_spectral: packed word -> s2m -> band_of_mode): the
// table arrives permuted into the segments' order (gtab = group_of_slot, k_field_permute; entry of (segment s, stored index
// l) at s * nlmax + l, next to where the mode record is read from), so the group is ONE load whose address follows from the
// packed word alone, issued beside the record's.  Without the partition the stored index is the mode and gtab is the
// caller's table (gstride = 0).  GROUPED is a template parameter: the plain field holds no trace of the table.
// Grid memory: one 64-byte line of 8 words {N, E, Fx, Fy, Fz, -, -, -} per cell (ix * ny + iy) * nz + iz, or per (cell, group)
// at cell * G + g, so that a particle's five adds touch one line; line `lines` is the header {clamped, overflow E, overflow F,
// ran, skip, ungrouped, -, -} (NK_FIELD_*, nk_field.h).
//   lds_bins = 1: the whole grid fits the launch's LDS (behind the subvolume tables, at byte offset lds0): {E, Fx, Fy, Fz}
//     (u64) and N (u32) per line there, integer LDS adds, and one flush of integer global adds per workgroup (non-zero bins);
//   lds_bins = 0: the adds go to global memory directly.  Same integers either way.
// The only global atomics are 64-bit integer adds (global_atomic_add_x2, no compare-and-swap loop); the store is read once
// per launch whatever the grid size.
struct NkFieldDev {
    double lo[3], inv_h[3];
    int32_t n[3], lines;              // lines = cells, or cells * G
    double sE, sF;                    // 2^k_E, 2^k_F
    double BE, BF;                    // bounds of |e| and of |v e| (every component)
    unsigned long long *grid;         // [(lines + 1) * 8] the grid being filled
    int32_t lds_bins, lds0;
    // GROUPED only:
    const int32_t *gtab;              // group_of_slot [nseg * nlmax], or group_of_mode [M] without the partition
    int32_t gstride, glim;            // a segment's entries start at seg * gstride; stored indices >= glim have no entry
    int32_t G;
};
#define NK_FIELD_WG 1024
template <bool STATE, bool GROUPED>
__global__ __launch_bounds__(NK_FIELD_WG) void k_field(NkDev d, NkFieldDev f) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (!STATE && d.halt[0]) return;                 // a halted batch: the sweep did nothing at this step
    NkLds L;
    nk_lds_setup<0, 0>(d, smem, L);
    const int nl = f.lines;
    unsigned long long *bR = (unsigned long long *)(smem + f.lds0);     // [4 nl] E, Fx, Fy, Fz of line b at 4 b
    unsigned int *bN = (unsigned int *)(bR + 4 * (size_t)nl);            // [nl]
    if (f.lds_bins) {
        for (int i = threadIdx.x; i < 4 * nl; i += blockDim.x) bR[i] = 0ull;
        for (int i = threadIdx.x; i < nl; i += blockDim.x) bN[i] = 0u;
        __syncthreads();
    }
    unsigned long long *hdr = f.grid + (size_t)nl * 8;
    unsigned int n_clamped = 0, n_ovE = 0, n_ovF = 0, n_ung = 0, stuck = 0;
    const uint32_t lbmask = (1u << d.lb) - 1u;
    for (int seg = blockIdx.x; seg < d.nseg; seg += gridDim.x) {
        const int64_t base = (int64_t)seg * d.segcap + (d.seg_lo ? d.seg_lo[seg] : 0);
        const int count = d.seg_count[seg];
        // step mode: migrants that k_deliver could not place wait in the inbox -- the sweep tallied particles this pass
        // cannot see, so the sample is dropped (header `skip`)
        if (!STATE && d.mig_buf && threadIdx.x == 0 && d.mig_n[seg] > 0) stuck = 1;
        const NkSegModes sm = nk_seg_modes(d, seg);
        const int32_t *gs = GROUPED ? f.gtab + (int64_t)seg * f.gstride : nullptr;
        for (int k = threadIdx.x; k < count; k += blockDim.x) {
            const int64_t i = base + k;
            const int idx = (int)(d.w0[i] & lbmask);
            int g = 0;
            if (GROUPED) {
                g = idx < f.glim ? gs[idx] : -1;
                if ((unsigned)g >= (unsigned)f.G) { n_ung += 1u; continue; }
            }
            const NkMode *rec = sm.rec + idx;
            const double x = d.x[i], y = d.y[i], z = d.z[i];
            double e;
            if (STATE) {
                double invT;
                const double T = nk_interp_T(d, L.tb, x, y, z, invT);
                const double n0 = !d.T_ref_local ? nk_occupation(d, d.T_ref, rec->omega, rec->E0)
                                                 : (T > 0.0 ? nk_be(rec->omega * d.c_hk, rec->E0, invT, d.invT0) : 0.0);
                e = d.hbar * rec->omega * (d.occ[i] - n0);
            } else {
                const int s = nk_classify(d, L.tb, x, y, z);
                e = nk_tally_e(d, L.tb, s, d.occ[i], rec->omega, rec->E0);
            }
            bool cl = false;
            const int ix = nk_field_axis(x, f.lo[0], f.inv_h[0], f.n[0], cl);
            const int iy = nk_field_axis(y, f.lo[1], f.inv_h[1], f.n[1], cl);
            const int iz = nk_field_axis(z, f.lo[2], f.inv_h[2], f.n[2], cl);
            n_clamped += cl ? 1u : 0u;
            const int c = (ix * f.n[1] + iy) * f.n[2] + iz;
            const int b = GROUPED ? c * f.G + g : c;                             // < lines <= 2^24
            const double fx = rec->vx * e, fy = rec->vy * e, fz = rec->vz * e;
            const bool okE = fabs(e) <= f.BE;                                     // (false for a NaN as well)
            const bool okF = fabs(fx) <= f.BF && fabs(fy) <= f.BF && fabs(fz) <= f.BF;
            n_ovE += okE ? 0u : 1u;
            n_ovF += okF ? 0u : 1u;
            const unsigned long long qE = okE ? (unsigned long long)(long long)rint(e * f.sE) : 0ull;
            const unsigned long long qx = okF ? (unsigned long long)(long long)rint(fx * f.sF) : 0ull;
            const unsigned long long qy = okF ? (unsigned long long)(long long)rint(fy * f.sF) : 0ull;
            const unsigned long long qz = okF ? (unsigned long long)(long long)rint(fz * f.sF) : 0ull;
            if (f.lds_bins) {
                atomicAdd(bN + b, 1u);
                atomicAdd(bR + 4 * b + 0, qE);
                atomicAdd(bR + 4 * b + 1, qx);
                atomicAdd(bR + 4 * b + 2, qy);
                atomicAdd(bR + 4 * b + 3, qz);
            } else {
                unsigned long long *w = f.grid + (size_t)b * 8;
                atomicAdd(w + 0, 1ull);
                atomicAdd(w + 1, qE);
                atomicAdd(w + 2, qx);
                atomicAdd(w + 3, qy);
                atomicAdd(w + 4, qz);
            }
        }
    }
    if (n_clamped) atomicAdd(hdr + NK_FIELD_CLAMPED, (unsigned long long)n_clamped);
    if (n_ovE) atomicAdd(hdr + NK_FIELD_OVE, (unsigned long long)n_ovE);
    if (n_ovF) atomicAdd(hdr + NK_FIELD_OVF, (unsigned long long)n_ovF);
    if (n_ung) atomicAdd(hdr + NK_FIELD_UNGROUPED, (unsigned long long)n_ung);
    if (stuck) atomicAdd(hdr + NK_FIELD_SKIP, 1ull);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(hdr + NK_FIELD_RAN, 1ull);   // this rank's pass ran
    if (f.lds_bins) {
        __syncthreads();
        for (int b = threadIdx.x; b < nl; b += blockDim.x) {
            const unsigned int n = bN[b];
            if (n == 0u) continue;
            unsigned long long *w = f.grid + (size_t)b * 8;
            atomicAdd(w + 0, (unsigned long long)n);
#pragma unroll
            for (int k = 0; k < 4; ++k) { const unsigned long long v = bR[4 * b + k]; if (v) atomicAdd(w + 1 + k, v); }
        }
    }
}
// group_of_slot: the caller's table in the segments' order (s2m: mode of (segment, stored index), -1 where there is none)
__global__ __launch_bounds__(256) void k_field_permute(const int32_t *s2m, const int32_t *table, int32_t *slot, int64_t n, int M) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = s2m[i];
    slot[i] = (unsigned)m < (unsigned)M ? table[m] : -1;
}
// One sample's integer grid into the time average, in line order: acc[b][5] += grid[b][0..4] / {1, sE, sF, sF, sF} (doubles;
// the headroom of the integers is spent per sample, not per window), then the grid is cleared for the next sample.  With a
// communicator the grid has been all-reduced (integers, sum) first, so every rank adds the same numbers.  The sample counts
// only if the pass ran on every rank (header `ran` = nranks: not in a halted batch) and no rank saw undelivered migrants
// (`skip` = 0) -- read from this grid's own header; the same store gives the field's and the groups' grid the same `ran` and
// `skip`, so the two windows hold the same steps.
__global__ __launch_bounds__(256) void k_field_accum(unsigned long long *grid, int lines, double sE, double sF, double *acc, int nranks) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= lines) return;
    const unsigned long long *hdr = grid + (size_t)lines * 8;
    const bool take = hdr[NK_FIELD_RAN] == (unsigned long long)nranks && hdr[NK_FIELD_SKIP] == 0ull;
    unsigned long long *w = grid + (size_t)b * 8;
    if (take) {
        const double iE = 1.0 / sE, iF = 1.0 / sF;
        double *a = acc + (size_t)b * 5;
        a[0] += (double)(long long)w[0];
        a[1] += (double)(long long)w[1] * iE;
        a[2] += (double)(long long)w[2] * iF;
        a[3] += (double)(long long)w[3] * iF;
        a[4] += (double)(long long)w[4] * iF;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = 0ull;
}
// ... and the header into the running status {samples, clamped, overflow E, overflow F [, ungrouped: where the status has
// the word]}; the header is cleared.
__global__ void k_field_finish(unsigned long long *grid, int lines, long long *status, int nstatus, int nranks) {
    unsigned long long *hdr = grid + (size_t)lines * 8;
    const bool take = hdr[NK_FIELD_RAN] == (unsigned long long)nranks && hdr[NK_FIELD_SKIP] == 0ull;
    if (take) {
        status[NK_FIELD_ST_SAMPLES] += 1;
        status[NK_FIELD_ST_CLAMPED] += (long long)hdr[NK_FIELD_CLAMPED];
        if (nstatus > NK_FIELD_ST_UNGROUPED) status[NK_FIELD_ST_UNGROUPED] += (long long)hdr[NK_FIELD_UNGROUPED];
    }
    status[NK_FIELD_ST_OVE] += (long long)hdr[NK_FIELD_OVE];
    status[NK_FIELD_ST_OVF] += (long long)hdr[NK_FIELD_OVF];
    for (int k = 0; k < 8; ++k) hdr[k] = 0ull;
}

// =================================================================================== host side
static void nk_grid_free(NkFieldGrid &g) {
    if (g.grid) hipFree(g.grid);
    if (g.acc) hipFree(g.acc);
    if (g.status) hipFree(g.status);
    g = NkFieldGrid();
}
static size_t nk_grid_bytes(int64_t lines, int nstatus) {
    return ((size_t)lines + 1) * 64 + (size_t)lines * 5 * sizeof(double) + (size_t)nstatus * sizeof(long long);
}
// the three buffers of a grid, zeroed (on an error the caller frees)
static hipError_t nk_grid_alloc(NkFieldGrid &g, int64_t lines, int nstatus) {
    const size_t gb = ((size_t)lines + 1) * 64, ab = (size_t)lines * 5 * sizeof(double), sb = (size_t)nstatus * sizeof(long long);
    hipError_t e = hipMalloc((void **)&g.grid, gb);
    if (e == hipSuccess) e = hipMalloc((void **)&g.acc, ab);
    if (e == hipSuccess) e = hipMalloc((void **)&g.status, sb);
    if (e == hipSuccess) e = hipMemset(g.grid, 0, gb);
    if (e == hipSuccess) e = hipMemset(g.acc, 0, ab);
    if (e == hipSuccess) e = hipMemset(g.status, 0, sb);
    g.lines = lines; g.nstatus = nstatus;
    g.bytes = (int64_t)nk_grid_bytes(lines, nstatus);
    return e;
}

void nk_field_free(NkFieldHost &F) {
    nk_grid_free(F.g);
    F = NkFieldHost();
}
void nk_fgroups_free(NkFGroupsHost &Gh) {
    if (Gh.table) hipFree(Gh.table);
    if (Gh.slot) hipFree(Gh.slot);
    nk_grid_free(Gh.g);
    Gh = NkFGroupsHost();
}

// ---- Scales.  Every term of E is e_i = hbar omega (n_i - n0): n_i and n0 are Bose-Einstein occupations at temperatures the
// run can hold -- the ends of the tabulated range, the reservoirs' and the fixed reference temperature; T_hi is the highest of
// them -- so 0 <= n_i, n0 <= n_BE(omega, T_hi) and |e_i| <= hbar omega n_BE(omega, T_hi) = kB T_hi x / (exp(x) - 1) with
// x = hbar omega / (kB T_hi); x / (exp(x) - 1) <= 1 for every x >= 0, so
//     B_E = kB T_hi        (>= the largest hbar omega times the largest occupation difference, for every mode)
//     B_F = vmax B_E       (vmax = the largest |v| of the material: bounds every component of v_i e_i)
// A cell receives at most `capacity` terms (the slots of the store, all ranks), each at most B 2^k + 1/2 after rounding, so
// with the largest k for which capacity B 2^k <= 2^62 the int64 sum stays below 2^62 + capacity / 2 < 2^63: it cannot wrap.
// The kernel checks every term against B and reports a larger one (occupations uploaded from outside that range) instead of
// adding it.  Re-derived when the store grows (nk_step).
int nk_field_k(double B, int64_t capacity) {
    const double m = B * (double)std::max<int64_t>(capacity, 1);
    int ex = 0;
    (void)frexp(m, &ex);                        // m = f 2^ex, 0.5 <= f < 1: m 2^k <= 2^62 for k = 62 - ex
    int k = 62 - ex;
    return std::max(-1000, std::min(1000, k));
}
void nk_field_scale(NkFieldHost &F, int64_t capacity) {
    F.capacity = capacity;
    F.kE = nk_field_k(F.BE, capacity);
    F.kF = nk_field_k(F.BF, capacity);
    if (F.cfg.flags & NK_FIELD_TEST_SMALL_BOUND) F.kE = nk_field_k(F.BE * ldexp(1.0, 40), capacity);   // (the scale of the true bound)
}

int nk_field_configure(NkFieldHost &F, const nk_field *f, int flux_every, double kb, double T_hi, double vmax, std::string &err) {
    nk_field_free(F);
    const int64_t nc = (int64_t)f->n[0] * f->n[1] * f->n[2];
    if (f->n[0] <= 0 || f->n[1] <= 0 || f->n[2] <= 0 || nc > (1ll << 24)) { err = "nk_set_field: the grid needs 1 .. 2^24 cells"; return NK_ERR_ARG; }
    for (int a = 0; a < 3; ++a)
        if (!(f->h[a] > 0.0) || !std::isfinite(f->h[a]) || !std::isfinite(f->lo[a])) { err = "nk_set_field: the cell sizes h must be positive"; return NK_ERR_ARG; }
    if (f->every <= 0 || flux_every <= 0 || f->every % flux_every != 0) {
        err = "nk_set_field: every (" + std::to_string(f->every) + ") must be a positive multiple of flux_every (" + std::to_string(flux_every) + ")";
        return NK_ERR_ARG;
    }
    if (!(T_hi > 0.0) || !(vmax > 0.0)) { err = "nk_set_field: the material gives no bound for the field's terms"; return NK_ERR_ARG; }
    F.cfg = *f;
    F.ncells = (int32_t)nc;
    F.T_hi = T_hi; F.vmax = vmax;
    F.BE = kb * T_hi;
    F.BF = vmax * F.BE;
    if (f->flags & NK_FIELD_TEST_SMALL_BOUND) F.BE = ldexp(F.BE, -40);
    const char *env = getenv("NK_FIELD_PATH");
    F.force_global = (f->flags & NK_FIELD_GLOBAL) || (env && !strcmp(env, "global"));
    const hipError_t e = nk_grid_alloc(F.g, nc, 4);
    if (e != hipSuccess) { nk_field_free(F); err = std::string("nk_set_field: ") + hipGetErrorString(e); return NK_ERR_HIP; }
    F.on = true;
    nk_field_scale(F, 1);
    return NK_OK;
}

int nk_fgroups_configure(NkFGroupsHost &Gh, const NkFieldHost &F, int32_t ngroups, const int32_t *group_of_mode, int32_t M, std::string &err) {
    nk_fgroups_free(Gh);
    if (!F.on) { err = "nk_set_field_groups: no field was set (nk_set_field first: the groups use its grid, cadence and scales)"; return NK_ERR_ARG; }
    if (ngroups <= 0 || !group_of_mode || M <= 0) { err = "nk_set_field_groups: bad arguments"; return NK_ERR_ARG; }
    const int64_t lines = (int64_t)F.ncells * ngroups;
    if (lines > (1ll << 24)) {
        err = "nk_set_field_groups: " + std::to_string(F.ncells) + " cells x " + std::to_string(ngroups) + " groups = " +
              std::to_string((long long)lines) + " lines, more than 2^24";
        return NK_ERR_ARG;
    }
    for (int m = 0; m < M; ++m)
        if (group_of_mode[m] < -1 || group_of_mode[m] >= ngroups) {
            err = "nk_set_field_groups: group_of_mode[" + std::to_string(m) + "] = " + std::to_string(group_of_mode[m]) +
                  " is outside [-1, " + std::to_string(ngroups) + ")";
            return NK_ERR_ARG;
        }
    const size_t tb = (size_t)M * sizeof(int32_t);
    hipError_t e = hipMalloc((void **)&Gh.table, tb);
    if (e == hipSuccess) e = hipMemcpy(Gh.table, group_of_mode, tb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = nk_grid_alloc(Gh.g, lines, 8);
    if (e != hipSuccess) {
        nk_fgroups_free(Gh);
        (void)hipGetLastError();
        err = std::string("nk_set_field_groups: allocating ") + std::to_string((unsigned long long)(tb + nk_grid_bytes(lines, 8))) + " bytes: " + hipGetErrorString(e);
        return NK_ERR_HIP;
    }
    Gh.G = ngroups; Gh.M = M;
    Gh.g.bytes += (int64_t)tb;
    Gh.on = true;
    return NK_OK;
}

hipError_t nk_fgroups_permute(NkFGroupsHost &Gh, const NkDev &d, int64_t map_gen, hipStream_t stream) {
    if (!d.part || !d.s2m) return hipSuccess;         // the stored index is the mode: the pass reads the caller's table
    if (Gh.slot && Gh.key_gen == map_gen && Gh.key_nseg == d.nseg && Gh.key_nlmax == d.nlmax && Gh.key_cap == d.cap) return hipSuccess;
    const int64_t n = (int64_t)d.nseg * d.nlmax;
    if (n != Gh.slot_len) {
        if (Gh.slot) { hipFree(Gh.slot); Gh.g.bytes -= Gh.slot_len * 4; }
        Gh.slot = nullptr; Gh.slot_len = 0;
        hipError_t e = hipMalloc((void **)&Gh.slot, (size_t)n * 4);
        if (e != hipSuccess) return e;
        Gh.slot_len = n; Gh.g.bytes += n * 4;
    }
    k_field_permute<<<(int)((n + 255) / 256), 256, 0, stream>>>(d.s2m, Gh.table, Gh.slot, n, Gh.M);
    Gh.key_gen = map_gen; Gh.key_nseg = d.nseg; Gh.key_nlmax = d.nlmax; Gh.key_cap = d.cap;
    Gh.permutes += 1;
    return hipGetLastError();
}

bool nk_field_lds_bins(const NkFieldGrid &g, bool force_global, size_t lds0, size_t *lds_bytes) {
    const size_t l0 = (lds0 + 15) & ~(size_t)15;
    const size_t with_bins = l0 + NK_FIELD_LDS_LINE * (size_t)g.lines;
    const bool bins = !force_global && with_bins <= NK_FIELD_LDS_MAX;
    if (lds_bytes) *lds_bytes = bins ? with_bins : l0;
    return bins;
}

template <bool STATE, bool GROUPED>
static hipError_t nk_field_launch(int nwg, size_t lds, const NkDev &d, const NkFieldDev &f, hipStream_t stream) {
    hipError_t e = nk_allow_lds((const void *)k_field<STATE, GROUPED>, lds);
    if (e != hipSuccess) return e;
    k_field<STATE, GROUPED><<<nwg, NK_FIELD_WG, lds, stream>>>(d, f);
    return hipGetLastError();
}

hipError_t nk_field_pass(NkFieldHost &F, NkFGroupsHost *Gh, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream) {
    NkFieldGrid &g = Gh ? Gh->g : F.g;
    NkFieldDev f;
    for (int a = 0; a < 3; ++a) { f.lo[a] = F.cfg.lo[a]; f.inv_h[a] = 1.0 / F.cfg.h[a]; f.n[a] = F.cfg.n[a]; }
    f.lines = (int32_t)g.lines;
    f.sE = ldexp(1.0, F.kE); f.sF = ldexp(1.0, F.kF);
    f.BE = F.BE; f.BF = F.BF;
    f.grid = g.grid;
    size_t lds = 0;
    f.lds_bins = nk_field_lds_bins(g, F.force_global, lds0, &lds) ? 1 : 0;
    f.lds0 = (int32_t)((lds0 + 15) & ~(size_t)15);
    f.gtab = nullptr; f.gstride = 0; f.glim = 0; f.G = 1;
    if (Gh) {
        const bool part = d.part && d.s2m;
        if (part && (!Gh->slot || Gh->slot_len != (int64_t)d.nseg * d.nlmax)) return hipErrorInvalidValue;    // (nk_fgroups_permute comes first)
        f.gtab = part ? Gh->slot : Gh->table;
        f.gstride = part ? d.nlmax : 0;
        f.glim = part ? d.nlmax : Gh->M;
        f.G = Gh->G;
    }
    // two 1024-thread workgroups per CU where their LDS allows it, else one
    const int per_cu = 2 * lds <= NK_FIELD_LDS_MAX ? 2 : 1;
    const int nwg = std::max(1, std::min(per_cu * num_cu, (int)d.nseg));
    if (Gh) return state ? nk_field_launch<true, true>(nwg, lds, d, f, stream) : nk_field_launch<false, true>(nwg, lds, d, f, stream);
    return state ? nk_field_launch<true, false>(nwg, lds, d, f, stream) : nk_field_launch<false, false>(nwg, lds, d, f, stream);
}

hipError_t nk_field_accumulate(NkFieldGrid &g, const NkFieldHost &F, int nranks, hipStream_t stream) {
    const int lines = (int)g.lines;
    k_field_accum<<<(lines + 255) / 256, 256, 0, stream>>>(g.grid, lines, ldexp(1.0, F.kE), ldexp(1.0, F.kF), g.acc, nranks);
    k_field_finish<<<1, 1, 0, stream>>>(g.grid, lines, g.status, g.nstatus, nranks);
    return hipGetLastError();
}

hipError_t nk_field_clear_grid(NkFieldGrid &g, hipStream_t stream) {
    return hipMemsetAsync(g.grid, 0, ((size_t)g.lines + 1) * 64, stream);
}

// nk_fgroups.hip -- grouped field maps: count, energy and heat flux per (cell of the field's grid, group of modes).  The
// kernels and their launches; the C entry points (nk_set_field_groups, nk_get_field_groups, nk_tally_field_groups_state,
// nk_field_groups_info) are in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds
// k_field_groups<false>, k_field_groups<true>, k_fgroups_permute, k_fgroups_accum, k_fgroups_finish, k_fgroups_clear and
// nothing else.
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_fgroups.h"

// LDS a launch may ask for on gfx950 (160 KB per CU; above 64 KB hipFuncSetAttribute has to allow it per kernel)
static const size_t NK_FG_LDS_MAX = 160 * 1024;
// bins of one line in LDS: E, Fx, Fy, Fz (u64) + N (u32)
static const size_t NK_FG_LDS_LINE = 36;

// =================================================================================== grouped field maps
// k_field (nk_kernels.h) says WHERE the heat goes, summed over all modes; k_spectral / k_modes say WHICH modes carry it, per
// subvolume.  k_field_groups does both at once: the field's five sums per (cell, group), group = group_of_mode[mode] from a
// table of the caller's (a frequency bin, a branch, a mean-free-path bin, a direction bin; -1 = in no group).  A pass of its
// own over the store, which it only reads, with k_field's launch shape, its two modes, its cell rule (nk_field_axis, clamped),
// its integers (rint(e 2^k_E), rint(v e 2^k_F) as int64 in two's complement; a term above B_E / B_F is not added but counted)
// and its two paths.  For a table that groups every mode the sums over the groups of a cell ARE the field's integers.
// Grid memory: one 64-byte line per (cell, group), line = cell * G + g, {N, E, Fx, Fy, Fz, -, -, -}; line `lines` is the
// header {clamped, overflow E, overflow F, ran, skip, ungrouped, -, -}.
// The group of a particle must not cost a chain of dependent loads (k_spectral: packed word -> s2m -> band_of_mode): the
// table arrives permuted into the segments' order (gtab = group_of_slot, k_fgroups_permute; entry of (segment s, stored index
// l) at s * nlmax + l, next to where the mode record is read from), so the group is ONE load whose address follows from the
// packed word alone, issued beside the record's.  Without the partition the stored index is the mode and gtab is the
// caller's table (gstride = 0).  A particle of group -1 is added nowhere and counted in the header's `ungrouped`.
struct NkFGroupsDev {
    const int32_t *gtab;              // group_of_slot [nseg * nlmax], or group_of_mode [M] without the partition
    int32_t gstride, glim;            // a segment's entries start at seg * gstride; stored indices >= glim have no entry
    int32_t G, lines;
    unsigned long long *grid;         // [(lines + 1) * 8]
};
template <bool STATE>
__global__ __launch_bounds__(NK_FIELD_WG) void k_field_groups(NkDev d, NkFieldDev f, NkFGroupsDev q) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (!STATE && d.halt[0]) return;                 // a halted batch: the sweep did nothing at this step
    NkLds L;
    nk_lds_setup<0, 0>(d, smem, L);
    const int nl = q.lines;
    unsigned long long *bR = (unsigned long long *)(smem + f.lds0);     // [4 nl] E, Fx, Fy, Fz of line b at 4 b
    unsigned int *bN = (unsigned int *)(bR + 4 * (size_t)nl);            // [nl]
    if (f.lds_bins) {
        for (int i = threadIdx.x; i < 4 * nl; i += blockDim.x) bR[i] = 0ull;
        for (int i = threadIdx.x; i < nl; i += blockDim.x) bN[i] = 0u;
        __syncthreads();
    }
    unsigned long long *hdr = q.grid + (size_t)nl * 8;
    unsigned int n_clamped = 0, n_ovE = 0, n_ovF = 0, n_ung = 0, stuck = 0;
    const uint32_t lbmask = (1u << d.lb) - 1u;
    for (int seg = blockIdx.x; seg < d.nseg; seg += gridDim.x) {
        const int64_t base = (int64_t)seg * d.segcap + (d.seg_lo ? d.seg_lo[seg] : 0);
        const int count = d.seg_count[seg];
        // step mode: migrants that k_deliver could not place wait in the inbox -- the sweep tallied particles this pass
        // cannot see, so the sample is dropped (header `skip`), as the field's is
        if (!STATE && d.mig_buf && threadIdx.x == 0 && d.mig_n[seg] > 0) stuck = 1;
        const NkSegModes sm = nk_seg_modes(d, seg);
        const int32_t *gs = q.gtab + (int64_t)seg * q.gstride;
        for (int k = threadIdx.x; k < count; k += blockDim.x) {
            const int64_t i = base + k;
            const int idx = (int)(d.w0[i] & lbmask);
            const int g = idx < q.glim ? gs[idx] : -1;
            if ((unsigned)g >= (unsigned)q.G) { n_ung += 1u; continue; }
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
            const int b = ((ix * f.n[1] + iy) * f.n[2] + iz) * q.G + g;      // < lines <= 2^24
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
                unsigned long long *w = q.grid + (size_t)b * 8;
                atomicAdd(w + 0, 1ull);
                atomicAdd(w + 1, qE);
                atomicAdd(w + 2, qx);
                atomicAdd(w + 3, qy);
                atomicAdd(w + 4, qz);
            }
        }
    }
    if (n_clamped) atomicAdd(hdr + NK_FG_CLAMPED, (unsigned long long)n_clamped);
    if (n_ovE) atomicAdd(hdr + NK_FG_OVE, (unsigned long long)n_ovE);
    if (n_ovF) atomicAdd(hdr + NK_FG_OVF, (unsigned long long)n_ovF);
    if (n_ung) atomicAdd(hdr + NK_FG_UNGROUPED, (unsigned long long)n_ung);
    if (stuck) atomicAdd(hdr + NK_FG_SKIP, 1ull);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(hdr + NK_FG_RAN, 1ull);   // this rank's pass ran
    if (f.lds_bins) {
        __syncthreads();
        for (int b = threadIdx.x; b < nl; b += blockDim.x) {
            const unsigned int n = bN[b];
            if (n == 0u) continue;
            unsigned long long *w = q.grid + (size_t)b * 8;
            atomicAdd(w + 0, (unsigned long long)n);
#pragma unroll
            for (int k = 0; k < 4; ++k) { const unsigned long long v = bR[4 * b + k]; if (v) atomicAdd(w + 1 + k, v); }
        }
    }
}
// group_of_slot: the caller's table in the segments' order (s2m: mode of (segment, stored index), -1 where there is none)
__global__ __launch_bounds__(256) void k_fgroups_permute(const int32_t *s2m, const int32_t *table, int32_t *slot, int64_t n, int M) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = s2m[i];
    slot[i] = (unsigned)m < (unsigned)M ? table[m] : -1;
}
// One sample's integer grid into the window's sums, in line order: acc[b][5] += grid[b][0..4] / {1, sE, sF, sF, sF}, then the
// grid is cleared for the next sample.  With a communicator the grid has been all-reduced (integers, sum) first.  The sample
// counts under the field's own rule -- the pass ran on every rank and no rank saw undelivered migrants -- read from this
// grid's header, which the same store gave the same `ran` and `skip` as the field's: the two windows hold the same steps.
__global__ __launch_bounds__(256) void k_fgroups_accum(unsigned long long *grid, int lines, double sE, double sF, double *acc, int nranks) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= lines) return;
    const unsigned long long *hdr = grid + (size_t)lines * 8;
    const bool take = hdr[NK_FG_RAN] == (unsigned long long)nranks && hdr[NK_FG_SKIP] == 0ull;
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
// ... and the header into the running status {samples, clamped, overflow E, overflow F, ungrouped}; the header is cleared.
__global__ void k_fgroups_finish(unsigned long long *grid, int lines, long long *status, int nranks) {
    unsigned long long *hdr = grid + (size_t)lines * 8;
    const bool take = hdr[NK_FG_RAN] == (unsigned long long)nranks && hdr[NK_FG_SKIP] == 0ull;
    if (take) {
        status[NK_FG_ST_SAMPLES] += 1;
        status[NK_FG_ST_CLAMPED] += (long long)hdr[NK_FG_CLAMPED];
        status[NK_FG_ST_UNGROUPED] += (long long)hdr[NK_FG_UNGROUPED];
    }
    status[NK_FG_ST_OVE] += (long long)hdr[NK_FG_OVE];
    status[NK_FG_ST_OVF] += (long long)hdr[NK_FG_OVF];
    for (int k = 0; k < 8; ++k) hdr[k] = 0ull;
}
// the grid and its header back to zero (after a state-mode call has copied them out)
__global__ __launch_bounds__(256) void k_fgroups_clear(unsigned long long *grid, int64_t words) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) grid[i] = 0ull;
}

// =================================================================================== host side
void nk_fgroups_free(NkFGroupsHost &Gh) {
    if (Gh.table) hipFree(Gh.table);
    if (Gh.slot) hipFree(Gh.slot);
    if (Gh.grid) hipFree(Gh.grid);
    if (Gh.acc) hipFree(Gh.acc);
    if (Gh.status) hipFree(Gh.status);
    Gh = NkFGroupsHost();
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
    const size_t tb = (size_t)M * sizeof(int32_t), gb = ((size_t)lines + 1) * 64, ab = (size_t)lines * 5 * sizeof(double), sb = 8 * sizeof(long long);
    hipError_t e = hipMalloc((void **)&Gh.table, tb);
    if (e == hipSuccess) e = hipMalloc((void **)&Gh.grid, gb);
    if (e == hipSuccess) e = hipMalloc((void **)&Gh.acc, ab);
    if (e == hipSuccess) e = hipMalloc((void **)&Gh.status, sb);
    if (e == hipSuccess) e = hipMemcpy(Gh.table, group_of_mode, tb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(Gh.grid, 0, gb);
    if (e == hipSuccess) e = hipMemset(Gh.acc, 0, ab);
    if (e == hipSuccess) e = hipMemset(Gh.status, 0, sb);
    if (e != hipSuccess) {
        nk_fgroups_free(Gh);
        (void)hipGetLastError();
        err = std::string("nk_set_field_groups: allocating ") + std::to_string((unsigned long long)(tb + gb + ab + sb)) + " bytes: " + hipGetErrorString(e);
        return NK_ERR_HIP;
    }
    Gh.G = ngroups; Gh.lines = lines; Gh.M = M;
    Gh.bytes = (int64_t)(tb + gb + ab + sb);
    Gh.on = true;
    return NK_OK;
}

hipError_t nk_fgroups_permute(NkFGroupsHost &Gh, const NkDev &d, int64_t map_gen, hipStream_t stream) {
    if (!d.part || !d.s2m) return hipSuccess;         // the stored index is the mode: the pass reads the caller's table
    if (Gh.slot && Gh.key_gen == map_gen && Gh.key_nseg == d.nseg && Gh.key_nlmax == d.nlmax && Gh.key_cap == d.cap) return hipSuccess;
    const int64_t n = (int64_t)d.nseg * d.nlmax;
    if (n != Gh.slot_len) {
        if (Gh.slot) { hipFree(Gh.slot); Gh.bytes -= Gh.slot_len * 4; }
        Gh.slot = nullptr; Gh.slot_len = 0;
        hipError_t e = hipMalloc((void **)&Gh.slot, (size_t)n * 4);
        if (e != hipSuccess) return e;
        Gh.slot_len = n; Gh.bytes += n * 4;
    }
    k_fgroups_permute<<<(int)((n + 255) / 256), 256, 0, stream>>>(d.s2m, Gh.table, Gh.slot, n, Gh.M);
    Gh.key_gen = map_gen; Gh.key_nseg = d.nseg; Gh.key_nlmax = d.nlmax; Gh.key_cap = d.cap;
    Gh.permutes += 1;
    return hipGetLastError();
}

static NkFieldDev nk_fgroups_field_dev(const NkFieldHost &F) {
    NkFieldDev f;
    for (int a = 0; a < 3; ++a) { f.lo[a] = F.cfg.lo[a]; f.inv_h[a] = 1.0 / F.cfg.h[a]; f.n[a] = F.cfg.n[a]; }
    f.ncells = F.ncells;
    f.sE = ldexp(1.0, F.kE); f.sF = ldexp(1.0, F.kF);
    f.BE = F.BE; f.BF = F.BF;
    f.grid = nullptr;                                  // (the field's own grid is not this pass's business)
    f.lds_bins = 0; f.lds0 = 0;
    return f;
}

bool nk_fgroups_lds_bins(const NkFGroupsHost &Gh, const NkFieldHost &F, size_t lds0, size_t *lds_bytes) {
    const size_t l0 = (lds0 + 15) & ~(size_t)15;
    const size_t with_bins = l0 + NK_FG_LDS_LINE * (size_t)Gh.lines;
    const bool bins = !F.force_global && with_bins <= NK_FG_LDS_MAX;
    if (lds_bytes) *lds_bytes = bins ? with_bins : l0;
    return bins;
}

hipError_t nk_fgroups_pass(NkFGroupsHost &Gh, const NkFieldHost &F, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream) {
    NkFieldDev f = nk_fgroups_field_dev(F);
    size_t lds = 0;
    f.lds_bins = nk_fgroups_lds_bins(Gh, F, lds0, &lds) ? 1 : 0;
    f.lds0 = (int32_t)((lds0 + 15) & ~(size_t)15);
    NkFGroupsDev q;
    const bool part = d.part && d.s2m;
    if (part && (!Gh.slot || Gh.slot_len != (int64_t)d.nseg * d.nlmax)) return hipErrorInvalidValue;    // (nk_fgroups_permute comes first)
    q.gtab = part ? Gh.slot : Gh.table;
    q.gstride = part ? d.nlmax : 0;
    q.glim = part ? d.nlmax : Gh.M;
    q.G = Gh.G; q.lines = (int32_t)Gh.lines;
    q.grid = Gh.grid;
    // two 1024-thread workgroups per CU where their LDS allows it, else one
    const int per_cu = 2 * lds <= NK_FG_LDS_MAX ? 2 : 1;
    const int nwg = std::max(1, std::min(per_cu * num_cu, (int)d.nseg));
    const void *fn = state ? (const void *)k_field_groups<true> : (const void *)k_field_groups<false>;
    if (lds > 65536 && Gh.lds_attr[state ? 1 : 0] < (int)lds) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        Gh.lds_attr[state ? 1 : 0] = (int)lds;
    }
    if (state) k_field_groups<true><<<nwg, NK_FIELD_WG, lds, stream>>>(d, f, q);
    else k_field_groups<false><<<nwg, NK_FIELD_WG, lds, stream>>>(d, f, q);
    return hipGetLastError();
}

hipError_t nk_fgroups_accumulate(NkFGroupsHost &Gh, const NkFieldHost &F, int nranks, hipStream_t stream) {
    const int lines = (int)Gh.lines;
    k_fgroups_accum<<<(lines + 255) / 256, 256, 0, stream>>>(Gh.grid, lines, ldexp(1.0, F.kE), ldexp(1.0, F.kF), Gh.acc, nranks);
    k_fgroups_finish<<<1, 1, 0, stream>>>(Gh.grid, lines, Gh.status, nranks);
    return hipGetLastError();
}

hipError_t nk_fgroups_clear_grid(NkFGroupsHost &Gh, hipStream_t stream) {
    const int64_t words = (Gh.lines + 1) * 8;
    const int nb = (int)std::min<int64_t>((words + 255) / 256, 4096);
    k_fgroups_clear<<<nb, 256, 0, stream>>>(Gh.grid, words);
    return hipGetLastError();
}

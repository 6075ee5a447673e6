// nk_modes.hip -- mode-resolved tally: the launches of k_modes / k_modes_accum (nk_kernels.h) and the integer scale.  The C
// entry points (nk_set_modes, nk_get_modes, nk_tally_modes_state, nk_modes_info) are in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds
// k_modes<false>, k_modes<true>, k_modes_accum and k_modes_finish and nothing else.
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_field.h"
#include "nk_modes.h"
#include "nk_kind.h"

// LDS a launch may ask for on gfx950 (160 KB per CU; above 64 KB nk_allow_lds has to allow it per kernel)
static const size_t NK_MODES_LDS_MAX = 160 * 1024;
// bins of one (mode, subvolume) in LDS: E (u64) + N (u32)
static const size_t NK_MODES_LDS_BIN = 12;

void nk_modes_free(NkModesHost &Mo) {
    if (Mo.tE) hipFree(Mo.tE);
    if (Mo.tN) hipFree(Mo.tN);
    if (Mo.hdr) hipFree(Mo.hdr);
    if (Mo.accE) hipFree(Mo.accE);
    if (Mo.accN) hipFree(Mo.accN);
    if (Mo.status) hipFree(Mo.status);
    Mo = NkModesHost();
}

// The field's bound and scale rule (nk_field.hip): |e_i| <= B_E = kB T_hi, and the largest k with capacity B_E 2^k <= 2^62 -- a
// bin receives at most `capacity` terms, so its int64 sum cannot wrap.
void nk_modes_bound(NkModesHost &Mo, double kb, double T_hi) {
    Mo.T_hi = T_hi;
    Mo.BE = kb * T_hi;
    if (Mo.cfg.flags & NK_MODES_TEST_SMALL_BOUND) Mo.BE = ldexp(Mo.BE, -40);
    Mo.capacity = 0;
}
void nk_modes_scale(NkModesHost &Mo, int64_t capacity) {
    Mo.capacity = capacity;
    Mo.kE = nk_field_k((Mo.cfg.flags & NK_MODES_TEST_SMALL_BOUND) ? Mo.BE * ldexp(1.0, 40) : Mo.BE, capacity);   // (the scale of the true bound)
}

int nk_modes_configure(NkModesHost &Mo, const nk_modes *m, int flux_every, int64_t nbins, double kb, double T_hi, std::string &err) {
    nk_modes_free(Mo);
    if (m->every <= 0 || flux_every <= 0 || m->every % flux_every != 0) {
        err = "nk_set_modes: every (" + std::to_string(m->every) + ") must be a positive multiple of flux_every (" + std::to_string(flux_every) + ")";
        return NK_ERR_ARG;
    }
    if (m->capacity < 0) { err = "nk_set_modes: capacity must not be negative"; return NK_ERR_ARG; }
    if (!(T_hi > 0.0) || nbins <= 0) { err = "nk_set_modes: the material gives no bound for the terms"; return NK_ERR_ARG; }
    Mo.cfg = *m;
    Mo.nbins = nbins;
    nk_modes_bound(Mo, kb, T_hi);
    const char *env = getenv("NK_MODES_PATH");
    Mo.force_global = (m->flags & NK_MODES_GLOBAL) || (env && !strcmp(env, "global"));
    const size_t nb = (size_t)nbins, total = nb * (8 + 4 + 8 + 8) + 8 * 8 + 4 * 8;
    hipError_t e = hipMalloc((void **)&Mo.tE, nb * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&Mo.tN, nb * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&Mo.accE, nb * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&Mo.accN, nb * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&Mo.hdr, 8 * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&Mo.status, 4 * 8);
    if (e == hipSuccess) e = hipMemset(Mo.tE, 0, nb * 8);
    if (e == hipSuccess) e = hipMemset(Mo.tN, 0, nb * 4);
    if (e == hipSuccess) e = hipMemset(Mo.accE, 0, nb * 8);
    if (e == hipSuccess) e = hipMemset(Mo.accN, 0, nb * 8);
    if (e == hipSuccess) e = hipMemset(Mo.hdr, 0, 8 * 8);
    if (e == hipSuccess) e = hipMemset(Mo.status, 0, 4 * 8);
    if (e != hipSuccess) {
        nk_modes_free(Mo);
        (void)hipGetLastError();
        err = std::string("nk_set_modes: ") + std::to_string(total) + " bytes of tables: " + hipGetErrorString(e);
        return NK_ERR_HIP;
    }
    Mo.bytes = (int64_t)total;
    Mo.on = true;
    nk_modes_scale(Mo, 1);
    return NK_OK;
}

static NkModesDev nk_modes_dev(const NkModesHost &Mo) {
    NkModesDev m;
    m.sE = ldexp(1.0, Mo.kE);
    m.BE = Mo.BE;
    m.tE = Mo.tE; m.tN = Mo.tN; m.hdr = Mo.hdr;
    m.owner = 0; m.lds0 = 0; m.slice = 0; m.nteam = NK_MODES_WG / 64;
    return m;
}

static size_t nk_modes_slice(const NkDev &d) { return (NK_MODES_LDS_BIN * (size_t)d.nlmax * (size_t)d.S + 15) & ~(size_t)15; }

// Segments a workgroup walks at a time (teams of 16 / nteam waves): the largest of 16, 8, 4, 2, 1 whose bins, behind the l0 bytes
// of subvolume tables, leave room for two workgroups per CU; 0 when not even one team's do (then: the global path).
static int nk_modes_nteam(const NkDev &d, size_t l0) {
    const size_t slice = nk_modes_slice(d);
    for (int nt = NK_MODES_WG / 64; nt >= 1; nt >>= 1)
        if (2 * (l0 + (size_t)nt * slice) <= NK_MODES_LDS_MAX) return nt;
    return 0;
}

bool nk_modes_owner(const NkModesHost &Mo, const NkDev &d, size_t lds0, size_t *lds_bytes, int *nteam) {
    const size_t l0 = (lds0 + 15) & ~(size_t)15;
    // the owner path needs the partition (a team owns its segment's modes) and bins that fit twice into a CU's LDS
    const int nt = (!Mo.force_global && d.part && d.nlmax > 0) ? nk_modes_nteam(d, l0) : 0;
    const bool owner = nt > 0;
    if (lds_bytes) *lds_bytes = owner ? l0 + (size_t)nt * nk_modes_slice(d) : l0;
    if (nteam) *nteam = owner ? nt : NK_MODES_WG / 64;               // (global path: one wave per segment)
    return owner;
}

hipError_t nk_modes_pass(NkModesHost &Mo, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream) {
    NkModesDev m = nk_modes_dev(Mo);
    size_t lds = 0;
    int nteam = 1;
    m.owner = nk_modes_owner(Mo, d, lds0, &lds, &nteam) ? 1 : 0;
    m.lds0 = (int32_t)((lds0 + 15) & ~(size_t)15);
    m.slice = (int32_t)nk_modes_slice(d);
    m.nteam = nteam;
    if (!m.owner) {                                   // nobody owns a row: every sample starts from zero
        hipError_t e = hipMemsetAsync(Mo.tE, 0, (size_t)Mo.nbins * 8, stream);
        if (e == hipSuccess) e = hipMemsetAsync(Mo.tN, 0, (size_t)Mo.nbins * 4, stream);
        if (e != hipSuccess) return e;
    }
    // two 1024-thread workgroups per CU (the threads a CU holds), fewer where there are fewer groups of segments
    const int G = std::max(1, std::min(2 * num_cu, ((int)d.nseg + nteam - 1) / nteam));
    const void *fn = state ? (const void *)k_modes<true> : (const void *)k_modes<false>;
    hipError_t e = nk_allow_lds(fn, lds);
    if (e != hipSuccess) return e;
    if (state) k_modes<true><<<G, NK_MODES_WG, lds, stream>>>(d, m);
    else k_modes<false><<<G, NK_MODES_WG, lds, stream>>>(d, m);
    return hipGetLastError();
}

hipError_t nk_modes_accumulate(NkModesHost &Mo, int nranks, int num_cu, hipStream_t stream) {
    const NkModesDev m = nk_modes_dev(Mo);
    const int G = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)num_cu * 8, (Mo.nbins + 255) / 256));
    k_modes_accum<0><<<G, 256, 0, stream>>>(m, Mo.accE, Mo.accN, Mo.nbins, nranks);
    k_modes_finish<0><<<1, 1, 0, stream>>>(m, Mo.status, nranks);
    return hipGetLastError();
}

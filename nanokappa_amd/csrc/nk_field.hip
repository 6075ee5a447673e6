// nk_field.hip -- spatial field maps: the launches of k_field / k_field_accum (nk_kernels.h) and the derivation of the
// integer scales.  The C entry points (nk_set_field, nk_get_field, nk_tally_field_state, nk_field_info) are in nk_engine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's object holds
// k_field<false>, k_field<true>, k_field_accum and k_field_finish and nothing else.
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_field.h"

// LDS a launch may ask for on gfx950 (160 KB per CU; above 64 KB hipFuncSetAttribute has to allow it per kernel)
static const size_t NK_FIELD_LDS_MAX = 160 * 1024;
// bins of one cell in LDS: E, Fx, Fy, Fz (u64) + N (u32)
static const size_t NK_FIELD_LDS_CELL = 36;

void nk_field_free(NkFieldHost &F) {
    if (F.grid) hipFree(F.grid);
    if (F.acc) hipFree(F.acc);
    if (F.status) hipFree(F.status);
    F = NkFieldHost();
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
    const size_t gb = ((size_t)nc + 1) * 64, ab = (size_t)nc * 5 * sizeof(double), sb = 4 * sizeof(long long);
    hipError_t e = hipMalloc((void **)&F.grid, gb);
    if (e == hipSuccess) e = hipMalloc((void **)&F.acc, ab);
    if (e == hipSuccess) e = hipMalloc((void **)&F.status, sb);
    if (e == hipSuccess) e = hipMemset(F.grid, 0, gb);
    if (e == hipSuccess) e = hipMemset(F.acc, 0, ab);
    if (e == hipSuccess) e = hipMemset(F.status, 0, sb);
    if (e != hipSuccess) { nk_field_free(F); err = std::string("nk_set_field: ") + hipGetErrorString(e); return NK_ERR_HIP; }
    F.bytes = (int64_t)(gb + ab + sb);
    F.on = true;
    nk_field_scale(F, 1);
    return NK_OK;
}

static NkFieldDev nk_field_dev(const NkFieldHost &F) {
    NkFieldDev f;
    for (int a = 0; a < 3; ++a) { f.lo[a] = F.cfg.lo[a]; f.inv_h[a] = 1.0 / F.cfg.h[a]; f.n[a] = F.cfg.n[a]; }
    f.ncells = F.ncells;
    f.sE = ldexp(1.0, F.kE); f.sF = ldexp(1.0, F.kF);
    f.BE = F.BE; f.BF = F.BF;
    f.grid = F.grid;
    f.lds_bins = 0; f.lds0 = 0;
    return f;
}

bool nk_field_lds_bins(const NkFieldHost &F, size_t lds0, size_t *lds_bytes) {
    const size_t l0 = (lds0 + 15) & ~(size_t)15;
    const size_t with_bins = l0 + NK_FIELD_LDS_CELL * (size_t)F.ncells;
    const bool bins = !F.force_global && with_bins <= NK_FIELD_LDS_MAX;
    if (lds_bytes) *lds_bytes = bins ? with_bins : l0;
    return bins;
}

hipError_t nk_field_pass(NkFieldHost &F, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream) {
    NkFieldDev f = nk_field_dev(F);
    size_t lds = 0;
    f.lds_bins = nk_field_lds_bins(F, lds0, &lds) ? 1 : 0;
    f.lds0 = (int32_t)((lds0 + 15) & ~(size_t)15);
    // two 1024-thread workgroups per CU where their LDS allows it, else one
    const int per_cu = 2 * lds <= NK_FIELD_LDS_MAX ? 2 : 1;
    const int G = std::max(1, std::min(per_cu * num_cu, (int)d.nseg));
    const void *fn = state ? (const void *)k_field<true> : (const void *)k_field<false>;
    if (lds > 65536 && F.lds_attr[state ? 1 : 0] < (int)lds) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        F.lds_attr[state ? 1 : 0] = (int)lds;
    }
    if (state) k_field<true><<<G, NK_FIELD_WG, lds, stream>>>(d, f);
    else k_field<false><<<G, NK_FIELD_WG, lds, stream>>>(d, f);
    return hipGetLastError();
}

hipError_t nk_field_accumulate(NkFieldHost &F, int nranks, hipStream_t stream) {
    const NkFieldDev f = nk_field_dev(F);
    k_field_accum<0><<<(F.ncells + 255) / 256, 256, 0, stream>>>(f, F.acc, nranks);
    k_field_finish<0><<<1, 1, 0, stream>>>(f, F.status, nranks);
    return hipGetLastError();
}

hipError_t nk_field_clear_grid(NkFieldHost &F, hipStream_t stream) {
    return hipMemsetAsync(F.grid, 0, ((size_t)F.ncells + 1) * 64, stream);
}

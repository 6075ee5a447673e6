// nk_field.h -- host state of the spatial field maps (nk_set_field; kernels k_field / k_field_accum in nk_kernels.h, launched
// from nk_field.hip, a translation unit of its own so that the rest of the library's machine code does not depend on it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/nanokappa_hip.h"

struct NkDev;

struct NkFieldHost {
    bool on = false;
    nk_field cfg = {};
    int32_t ncells = 0;
    // scales (nk_field_scale): the integers hold e 2^kE and v e 2^kF
    int32_t kE = 0, kF = 0;
    double BE = 0.0, BF = 0.0;            // bounds of |e_i| and |v_i e_i|
    double T_hi = 0.0, vmax = 0.0;        // what the bounds were derived from
    int64_t capacity = 0;                 // particle slots (all ranks) the scales allow for
    bool force_global = false;
    unsigned long long *grid = nullptr;   // [(ncells + 1) * 8] one sample's integers + header line
    double *acc = nullptr;                // [ncells * 5] sums over the samples since the last reset: N, E, Fx, Fy, Fz
    long long *status = nullptr;          // [4] samples, clamped, overflow E, overflow F
    int64_t bytes = 0;
    int lds_attr[2] = {0, 0};             // dynamic LDS the two instantiations of k_field were last allowed
};

void nk_field_free(NkFieldHost &F);
// validate f against the engine's state and allocate; kb in eV/K, T_hi the highest temperature an occupation can stand for,
// vmax the largest group speed; NK_ERR_* with `err` set
int nk_field_configure(NkFieldHost &F, const nk_field *f, int flux_every, double kb, double T_hi, double vmax, std::string &err);
// the largest k with capacity B 2^k <= 2^62 (shared with the mode tally, nk_modes.hip)
int nk_field_k(double B, int64_t capacity);
// k_E, k_F for `capacity` particle slots
void nk_field_scale(NkFieldHost &F, int64_t capacity);
// one pass over the store into F.grid; lds0: bytes of LDS the subvolume tables take (nk_lds(ctx, false))
// where the bins of a pass live: true = in LDS behind the `lds0` bytes of subvolume tables (then *lds_bytes, if given, receives
// what the launch asks for), false = global integer adds directly.  nk_field_pass and nk_field_info both ask here.
bool nk_field_lds_bins(const NkFieldHost &F, size_t lds0, size_t *lds_bytes = nullptr);
hipError_t nk_field_pass(NkFieldHost &F, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream);
// F.grid (already summed over the ranks) into the accumulator and the status words; clears the grid
hipError_t nk_field_accumulate(NkFieldHost &F, int nranks, hipStream_t stream);
hipError_t nk_field_clear_grid(NkFieldHost &F, hipStream_t stream);

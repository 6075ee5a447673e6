// nk_modes.h -- host state of the mode-resolved tally (nk_set_modes; kernels k_modes / k_modes_accum in nk_kernels.h, launched
// from nk_modes.hip, a translation unit of its own so that the rest of the library's machine code does not depend on it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/nanokappa_hip.h"

struct NkDev;

struct NkModesHost {
    bool on = false;
    nk_modes cfg = {};
    int64_t nbins = 0;                    // M * S
    int32_t kE = 0;                       // the integers hold e 2^kE (nk_field_k: the field's rule)
    double BE = 0.0, T_hi = 0.0;          // bound of |e_i| and the temperature it was derived from
    int64_t capacity = 0;                 // particle slots (all ranks) the scale allows for
    bool force_global = false;
    unsigned long long *tE = nullptr;     // [nbins] one sample's integers, bin m * S + s
    unsigned int *tN = nullptr;           // [nbins]
    unsigned long long *hdr = nullptr;    // [8] overflow E, ran, skip
    double *accE = nullptr, *accN = nullptr;   // [nbins] sums over the samples since the last reset (this rank's particles)
    long long *status = nullptr;          // [4] samples, skipped, overflow E, -
    int64_t bytes = 0;
};

void nk_modes_free(NkModesHost &Mo);
// validate m and allocate (zeroed); kb in eV/K, T_hi the highest temperature an occupation can stand for; NK_ERR_* with `err` set
int nk_modes_configure(NkModesHost &Mo, const nk_modes *m, int flux_every, int64_t nbins, double kb, double T_hi, std::string &err);
void nk_modes_bound(NkModesHost &Mo, double kb, double T_hi);
void nk_modes_scale(NkModesHost &Mo, int64_t capacity);
// where the bins of a pass live: true = the nlmax x S bins of every team of waves in its own slice of LDS behind the `lds0`
// bytes of subvolume tables (owner path; *lds_bytes receives what the launch asks for, *nteam the segments a workgroup walks at
// a time), false = global integer adds
bool nk_modes_owner(const NkModesHost &Mo, const NkDev &d, size_t lds0, size_t *lds_bytes = nullptr, int *nteam = nullptr);
// one pass over the store into the sample table (cleared first on the global path)
hipError_t nk_modes_pass(NkModesHost &Mo, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream);
// the sample (its header already summed over the ranks) into the accumulators and the status words; clears the header
hipError_t nk_modes_accumulate(NkModesHost &Mo, int nranks, int num_cu, hipStream_t stream);

// nk_fgroups.h -- host state of the grouped field maps (nk_set_field_groups; kernels k_field_groups / k_fgroups_permute /
// k_fgroups_accum / k_fgroups_finish / k_fgroups_clear in nk_fgroups.hip, a translation unit of its own so that the rest of the
// library's machine code does not depend on it).  The grid, the cadence, the scales and the bounds are the field's (nk_field.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/nanokappa_hip.h"
#include "nk_field.h"

struct NkDev;

// header line of the grid / status words
enum { NK_FG_CLAMPED = 0, NK_FG_OVE = 1, NK_FG_OVF = 2, NK_FG_RAN = 3, NK_FG_SKIP = 4, NK_FG_UNGROUPED = 5 };
enum { NK_FG_ST_SAMPLES = 0, NK_FG_ST_CLAMPED = 1, NK_FG_ST_OVE = 2, NK_FG_ST_OVF = 3, NK_FG_ST_UNGROUPED = 4 };

struct NkFGroupsHost {
    bool on = false;
    int32_t G = 0;
    int64_t lines = 0;                    // ncells * G
    int32_t M = 0;
    int32_t *table = nullptr;             // [M] the caller's group_of_mode
    int32_t *slot = nullptr;              // [slot_len] group_of_slot: the table in the segments' order (k_fgroups_permute)
    int64_t slot_len = 0;
    // what `slot` was built for: the mode map's generation, the segmentation and the store's slots
    int64_t key_gen = -1, key_cap = -1;
    int32_t key_nseg = -1, key_nlmax = -1;
    int64_t permutes = 0;                 // times the permuted table was built
    unsigned long long *grid = nullptr;   // [(lines + 1) * 8] one sample's integers + header line
    double *acc = nullptr;                // [lines * 5] sums over the samples since the last reset: N, E, Fx, Fy, Fz
    long long *status = nullptr;          // [8] samples, clamped, overflow E, overflow F, ungrouped
    int64_t bytes = 0;
    int lds_attr[2] = {0, 0};             // dynamic LDS the two instantiations of k_field_groups were last allowed
};

void nk_fgroups_free(NkFGroupsHost &Gh);
// validate the table against the field and allocate; NK_ERR_* with `err` set
int nk_fgroups_configure(NkFGroupsHost &Gh, const NkFieldHost &F, int32_t ngroups, const int32_t *group_of_mode, int32_t M, std::string &err);
// group_of_slot for the mode map `map_gen` of d (no-op where it is current, or without the partition)
hipError_t nk_fgroups_permute(NkFGroupsHost &Gh, const NkDev &d, int64_t map_gen, hipStream_t stream);
// where the bins of a pass live: true = in LDS behind the `lds0` bytes of subvolume tables, false = global integer adds
bool nk_fgroups_lds_bins(const NkFGroupsHost &Gh, const NkFieldHost &F, size_t lds0, size_t *lds_bytes = nullptr);
// one pass over the store into Gh.grid
hipError_t nk_fgroups_pass(NkFGroupsHost &Gh, const NkFieldHost &F, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream);
// Gh.grid (already summed over the ranks) into the accumulator and the status words; clears the grid
hipError_t nk_fgroups_accumulate(NkFGroupsHost &Gh, const NkFieldHost &F, int nranks, hipStream_t stream);
hipError_t nk_fgroups_clear_grid(NkFGroupsHost &Gh, hipStream_t stream);

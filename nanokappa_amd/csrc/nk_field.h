// nk_field.h -- host state of the spatial field maps (nk_set_field) and of the grouped field maps on the same grid
// (nk_set_field_groups).  One kernel, k_field<STATE, GROUPED>, fills either grid; it and its helpers (k_field_accum,
// k_field_finish, k_field_permute) are defined and launched in nk_field.hip, a translation unit of its own so that the rest of
// the library's machine code does not depend on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/nanokappa_hip.h"

struct NkDev;

// words of a grid's header line, and of its status (NK_FIELD_UNGROUPED / NK_FIELD_ST_UNGROUPED: the groups' grid only)
enum { NK_FIELD_CLAMPED = 0, NK_FIELD_OVE = 1, NK_FIELD_OVF = 2, NK_FIELD_RAN = 3, NK_FIELD_SKIP = 4, NK_FIELD_UNGROUPED = 5 };
enum { NK_FIELD_ST_SAMPLES = 0, NK_FIELD_ST_CLAMPED = 1, NK_FIELD_ST_OVE = 2, NK_FIELD_ST_OVF = 3, NK_FIELD_ST_UNGROUPED = 4 };

// the buffers of one grid: a line per cell (the field) or per (cell, group)
struct NkFieldGrid {
    int64_t lines = 0;
    unsigned long long *grid = nullptr;   // [(lines + 1) * 8] one sample's integers + header line
    double *acc = nullptr;                // [lines * 5] sums over the samples since the last reset: N, E, Fx, Fy, Fz
    long long *status = nullptr;          // [nstatus] samples, clamped, overflow E, overflow F (field: 4) [, ungrouped, -, -, - (groups: 8)]
    int32_t nstatus = 0;
    int64_t bytes = 0;                    // device memory of this grid (the groups': with their tables)
};

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
    NkFieldGrid g;                        // ncells lines
};

// The groups live on the field's grid, with its cadence, scales and bounds.
struct NkFGroupsHost {
    bool on = false;
    int32_t G = 0;
    int32_t M = 0;
    int32_t *table = nullptr;             // [M] the caller's group_of_mode
    int32_t *slot = nullptr;              // [slot_len] group_of_slot: the table in the segments' order (k_field_permute)
    int64_t slot_len = 0;
    // what `slot` was built for: the mode map's generation, the segmentation and the store's slots
    int64_t key_gen = -1, key_cap = -1;
    int32_t key_nseg = -1, key_nlmax = -1;
    int64_t permutes = 0;                 // times the permuted table was built
    NkFieldGrid g;                        // ncells * G lines
};

void nk_field_free(NkFieldHost &F);
void nk_fgroups_free(NkFGroupsHost &Gh);
// validate f against the engine's state and allocate; kb in eV/K, T_hi the highest temperature an occupation can stand for,
// vmax the largest group speed; NK_ERR_* with `err` set
int nk_field_configure(NkFieldHost &F, const nk_field *f, int flux_every, double kb, double T_hi, double vmax, std::string &err);
// validate the table against the field and allocate; NK_ERR_* with `err` set
int nk_fgroups_configure(NkFGroupsHost &Gh, const NkFieldHost &F, int32_t ngroups, const int32_t *group_of_mode, int32_t M, std::string &err);
// the largest k with capacity B 2^k <= 2^62 (shared with the mode tally, nk_modes.hip)
int nk_field_k(double B, int64_t capacity);
// k_E, k_F for `capacity` particle slots
void nk_field_scale(NkFieldHost &F, int64_t capacity);
// group_of_slot for the mode map `map_gen` of d (no-op where it is current, or without the partition)
hipError_t nk_fgroups_permute(NkFGroupsHost &Gh, const NkDev &d, int64_t map_gen, hipStream_t stream);

// What follows serves both grids: Gh = nullptr is the field's own (F.g), else the groups' (Gh->g).
// Where the bins of a pass live: true = in LDS behind the `lds0` bytes of subvolume tables (nk_lds(ctx, false); then *lds_bytes,
// if given, receives what the launch asks for), false = global integer adds directly.  nk_field_pass and the two *_info ask here.
bool nk_field_lds_bins(const NkFieldGrid &g, bool force_global, size_t lds0, size_t *lds_bytes = nullptr);
// one pass over the store into the grid
hipError_t nk_field_pass(NkFieldHost &F, NkFGroupsHost *Gh, const NkDev &d, bool state, size_t lds0, int num_cu, hipStream_t stream);
// the grid (already summed over the ranks) into the accumulator and the status words; clears the grid
hipError_t nk_field_accumulate(NkFieldGrid &g, const NkFieldHost &F, int nranks, hipStream_t stream);
// the grid and its header back to zero (after a state-mode call has copied them out)
hipError_t nk_field_clear_grid(NkFieldGrid &g, hipStream_t stream);

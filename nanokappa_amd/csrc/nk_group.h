// nk_group.h -- replica groups (nk_group_create; kernels k_sweep_group / k_tail_group in nk_group.hip, a translation unit of its
// own so that the rest of the library's machine code does not depend on it): R contexts with the same configuration are stepped
// by ONE k_sweep_group and ONE k_tail_group launch per step.  The host side (members, halts, hand-over) is in nk_engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nk_kind.h"

struct NkDev;

#define NK_GROUP_MAX 32          // members of a group at most

// Where the members' workgroups begin in the two grids (exclusive prefix sums; entry R = the grid, entries above R = INT32_MAX, so
// a workgroup finds its member by counting the entries it is not below), and what else differs between members but not between
// steps.  Lives in device memory next to the members' NkDevs; the kernels read both through the constant address space.
struct NkGroupHead {
    int32_t pre_sweep[NK_GROUP_MAX + 1];
    int32_t pre_tail[NK_GROUP_MAX + 1];
    int32_t rows[NK_GROUP_MAX];          // tally rows of a member = workgroups of its sweep
    int32_t NB;                          // reduce workgroups of every member (the members agree on S and R)
    int32_t pad_;
};
// What differs between members AND steps: one record per (step of the call, member), uploaded once per call.
struct NkGroupRec {
    uint32_t step;
    int32_t do_relax, do_flux;
    int32_t down;                        // direction of the alternating walk at this step (NkDev::down)
    double *hist_row, *acc;
};

// k: the kind of the k_sweep that the group's sweep mirrors (nk_kind.h; a group's scope leaves pid, lrec, fast and box open)
hipError_t nk_group_launch_sweep(const NkSweepKind &k, int grid, size_t lds, hipStream_t stream, const NkGroupHead *head, const NkDev *devs,
                                 const NkGroupRec *recs);
// the FAST instantiations live in an object of their own, built with the flags of nk_sweep_plain.hip (Makefile)
hipError_t nk_group_launch_sweep_fast(const NkSweepKind &k, int grid, size_t lds, hipStream_t stream, const NkGroupHead *head, const NkDev *devs,
                                      const NkGroupRec *recs);
hipError_t nk_group_launch_tail(bool box, int grid, size_t lds, hipStream_t stream, const NkGroupHead *head, const NkDev *devs, const NkGroupRec *recs);

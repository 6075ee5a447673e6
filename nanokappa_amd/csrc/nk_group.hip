// nk_group.hip -- replica groups: k_sweep_group / k_tail_group and their launches.  One launch serves R contexts: a workgroup
// finds its member r and its index among that member's workgroups in a prefix table, takes the member's NkDev, and runs the SAME
// device functions as k_sweep / k_tail (nk_kernels.h) with its relative index -- nothing in either kernel waits on another
// workgroup (the reduce's last-arriver ticket is per member and does not block).  The C entry points (nk_group_create, nk_group_step,
// ...) are in nk_engine.hip.
//
// This file is compiled twice (Makefile): nk_group.o with the library's flags (machine LICM off) holds the launches, k_tail_group
// and the sweeps that mirror the k_sweep instantiations of nk_engine.hip; nk_group_plain.o (-DNK_GROUP_PLAIN, the flags of
// nk_sweep_plain.hip) holds the sweeps that mirror the FAST instantiations built there -- the same expressions compiled the same way.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nanokappa_hip.h"
// Every non-template kernel of nk_kernels.h becomes a template here that nothing instantiates, so this file's objects hold
// the group kernels and nothing else.
#define NK_KERNEL_LINKAGE template <int NK_NOT_IN_THIS_TU = 0>
#include "nk_kernels.h"
#include "nk_group.h"

// The members' NkDevs (1.2 KB each), the prefix table and the per-step records are read through the CONSTANT address space: the
// loads are scalar and invariant like those of kernel arguments, whatever the kernel stores in between.
#define NK_CONSTANT_AS __attribute__((address_space(4)))

// member of workgroup b: the number of entries 1 .. NK_GROUP_MAX - 1 of the prefix table that b is not below (entries above R are
// INT32_MAX).  b is wave-uniform, the table two scalar loads: a count, no dependent chain of loads.
__device__ __forceinline__ int nk_group_member(const NK_CONSTANT_AS int32_t *pre, int b) {
    int r = 0;
#pragma unroll
    for (int k = 1; k < NK_GROUP_MAX; ++k) r += (b >= pre[k]) ? 1 : 0;
    return r;
}
__device__ __forceinline__ void nk_group_dev(NkDev &d, const NkDev *devs, int r) {
    const NK_CONSTANT_AS NkDev *c = (const NK_CONSTANT_AS NkDev *)devs + r;
    __builtin_memcpy(&d, c, sizeof(NkDev));
}

// k_sweep<1, false, false, PID, false, LREC, FAST, BOX> for the members of a group; the launch bounds of that instantiation.
template <bool PID, bool LREC, int FAST, bool BOX>
__global__ __launch_bounds__(NK_WG, NK_SWEEP_BOUND(1, false, false, false)) void k_sweep_group(const NkGroupHead *head_, const NkDev *devs,
                                                                                               const NkGroupRec *recs_) {
    extern __shared__ __align__(16) unsigned char smem[];
    const NK_CONSTANT_AS NkGroupHead *head = (const NK_CONSTANT_AS NkGroupHead *)head_;
    const int b = (int)blockIdx.x;
    const int r = nk_group_member(head->pre_sweep, b);
    const int wg = b - head->pre_sweep[r], nwg = head->pre_sweep[r + 1] - head->pre_sweep[r];
    const NK_CONSTANT_AS NkGroupRec *rec = (const NK_CONSTANT_AS NkGroupRec *)recs_ + r;
    NkDev d;
    nk_group_dev(d, devs, r);
    if (d.halt[0]) return;                          // this member asked for a larger store: it stops alone, the others run on
    d.down = rec->down;
    if (FAST) { d.sv_kind = 0; d.sv_interp = FAST - 1; d.T_ref_local = 1; }
    NkLds L;
    nk_lds_setup<1, PID ? 3 : 2>(d, smem, L);
    nk_sweep_body<1, false, false, PID, false, LREC, FAST, BOX>(d, L, rec->step, rec->do_relax, rec->do_flux, wg, nwg);
    nk_lds_flush(d, L, wg);
}

typedef void (*NkGroupSweepFn)(const NkGroupHead *, const NkDev *, const NkGroupRec *);

#ifdef NK_GROUP_PLAIN

hipError_t nk_group_launch_sweep_fast(const NkSweepKind &k, int grid, size_t lds, hipStream_t stream, const NkGroupHead *head, const NkDev *devs,
                                      const NkGroupRec *recs) {
    if (k.pid || (k.fast != 1 && k.fast != 2)) return hipErrorInvalidValue;
    const NkGroupSweepFn fn = nk_lift([](auto L, auto F1, auto X) -> NkGroupSweepFn { return k_sweep_group<false, L.value, F1.value ? 1 : 2, X.value>; },
                                      k.lrec, k.fast == 1, k.box);
    fn<<<grid, NK_WG, lds, stream>>>(head, devs, recs);
    return hipGetLastError();
}

#else

// k_tail<1, BOX> with fuse = 1 for the members of a group: per member NB reduce workgroups (the last to arrive runs the update),
// then the workgroups of the NEXT step's emission.
template <bool BOX>
__global__ __launch_bounds__(NK_WG) void k_tail_group(const NkGroupHead *head_, const NkDev *devs, const NkGroupRec *recs_) {
    extern __shared__ __align__(16) unsigned char smem[];
    const NK_CONSTANT_AS NkGroupHead *head = (const NK_CONSTANT_AS NkGroupHead *)head_;
    const int b = (int)blockIdx.x;
    const int r = nk_group_member(head->pre_tail, b);
    const int wg = b - head->pre_tail[r], nwg = head->pre_tail[r + 1] - head->pre_tail[r];
    const int n_reduce = head->NB;
    const NK_CONSTANT_AS NkGroupRec *rec = (const NK_CONSTANT_AS NkGroupRec *)recs_ + r;
    NkDev d;
    nk_group_dev(d, devs, r);
    if (wg < n_reduce) {
        double *sh = reinterpret_cast<double *>(smem);
        int &last = *reinterpret_cast<int *>(smem + NK_WG * sizeof(double));
        nk_reduce_body(d, head->rows[r], rec->acc, rec->hist_row, rec->do_flux, 1, wg, n_reduce, sh, last);
    } else {
        nk_emit_body<1, BOX>(d, rec->step + 1u, smem, wg - n_reduce, nwg - n_reduce, true);
    }
}

hipError_t nk_group_launch_sweep(const NkSweepKind &k, int grid, size_t lds, hipStream_t stream, const NkGroupHead *head, const NkDev *devs,
                                 const NkGroupRec *recs) {
    if (k.fast) return nk_group_launch_sweep_fast(k, grid, lds, stream, head, devs, recs);
    const NkGroupSweepFn fn = nk_lift([](auto P, auto L, auto X) -> NkGroupSweepFn { return k_sweep_group<P.value, L.value, 0, X.value>; },
                                      k.pid, k.lrec, k.box);
    fn<<<grid, NK_WG, lds, stream>>>(head, devs, recs);
    return hipGetLastError();
}

hipError_t nk_group_launch_tail(bool box, int grid, size_t lds, hipStream_t stream, const NkGroupHead *head, const NkDev *devs, const NkGroupRec *recs) {
    if (box) k_tail_group<true><<<grid, NK_WG, lds, stream>>>(head, devs, recs);
    else k_tail_group<false><<<grid, NK_WG, lds, stream>>>(head, devs, recs);
    return hipGetLastError();
}

#endif

// nk_engine.hip -- host side (C ABI, include/nanokappa_hip.h) of libnanokappa_hip.so; kernels in nk_kernels.h.
// gfx950 / MI355X only.  HIP runtime + (lazily, multi-GPU only) RCCL; no PyTorch, no CPU fallback.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <type_traits>
#include <chrono>
#include <time.h>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/nanokappa_hip.h"
#include "nk_kernels.h"
#include "nk_field.h"
#include "nk_modes.h"
#include "nk_group.h"
#include "nk_freepath.h"
#include "nk_freecols.h"
#include "nk_kinetic.h"
// instantiated in nk_sweep_plain.hip (compiled with the machine LICM on; see there)
extern template __global__ void k_sweep<1, false, false, false, false, true, 1>(NkDev, uint32_t, int, int);
extern template __global__ void k_sweep<1, false, false, false, false, true, 2>(NkDev, uint32_t, int, int);
extern template __global__ void k_sweep<1, false, false, false, false, false, 1>(NkDev, uint32_t, int, int);
extern template __global__ void k_sweep<1, false, false, false, false, false, 2>(NkDev, uint32_t, int, int);
extern template __global__ void k_sweep<1, false, false, false, false, true, 1, true>(NkDev, uint32_t, int, int);
extern template __global__ void k_sweep<1, false, false, false, false, true, 2, true>(NkDev, uint32_t, int, int);
extern template __global__ void k_sweep<1, false, false, false, false, false, 1, true>(NkDev, uint32_t, int, int);
extern template __global__ void k_sweep<1, false, false, false, false, false, 2, true>(NkDev, uint32_t, int, int);

struct NkRccl {      // symbols resolved lazily with dlopen: a single-GPU run never loads librccl
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;      // optional: ends a communicator whose peers never arrived
};

static thread_local std::string g_create_error;

struct nk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    NkDev d;                       // device view (pointers into `allocs` / `pallocs`)
    std::vector<void *> allocs;    // everything hipMalloc'ed except the particle arrays
    std::vector<void *> pallocs;   // particle arrays (re-allocated by nk_reserve)
    void *store_buf = nullptr;     // the one among them that holds the particle fields (nk_alloc_fields)
    size_t store_pad = 0;
    bool store_pid = false;
    bool store_nts = true;         // false: box store (no cached next hit, NkDev::box)
    bool mesh_box = false;         // nk_set_mesh: the mesh is an axis-aligned box whose six sides are its six facets
    bool box_forbidden = false;    // this context met particles a box store cannot express (nk_init_boundaries): cached layout from then on
    int32_t *anomalies = nullptr;  // device word of k_init_boundaries
    bool have_material = false, have_mesh = false, have_sv = false, have_params = false;
    int64_t step = 0;
    bool pending_relax = false;
    int g_sweep = 0;               // persistent grid of k_sweep = rows of `partials`
    std::vector<hipEvent_t> evpool;
    NkSweepKind g_sweep_kind = {};     // which k_sweep instantiation g_sweep was sized for (g_sweep == 0: none yet)
    size_t g_sweep_lds = 0;            //   and with how much LDS per workgroup
    int layout_key = -1;               // how the particle store was laid out: 1 modes partitioned | 2 ids tracked
    std::vector<double> h_enter_prob;  // host copy of enter_prob (sizes the segments' head room)
    // set-up table builder state (nk_specular_*)
    int64_t spec_M = 0;
    double *spec_v = nullptr, *spec_om = nullptr, *spec_dl = nullptr, *spec_svx = nullptr;
    int32_t *spec_rank = nullptr;
    double spec_vmax = 0.0;
    NkSpecMode *spec_modes = nullptr;
    int32_t *spec_in = nullptr, *spec_out = nullptr;
    unsigned long long *spec_count = nullptr;
    double *ks_kv = nullptr, *ks_mat = nullptr;   // 'k' model pair search: wavevectors [Q*3]; k_to_q, q_to_k, tol (21 doubles)
    double ks_tol[3] = {0, 0, 0};
    int64_t ks_Q = 0;
    int64_t spec_cap = 0;
    int64_t spec_last = 0;            // pairs of the last nk_specular_pairs call (still on the device)
    // rough tables under construction on the device (nk_rough_begin .. nk_rough_finish)
    int rb_Fr = 0;
    double *rb_k2 = nullptr, *rb_nin = nullptr, *rb_eta = nullptr, *rb_sub = nullptr, *rb_spec = nullptr, *rb_roul = nullptr;
    uint8_t *rb_ts = nullptr;
    unsigned int *rb_map = nullptr;
    std::vector<int32_t> rb_facet;
    int64_t o2o_first = 0;            // 'one_to_one': particles entering at the first step (sizes the spawn inboxes)
    bool stepped = false;             // a timestep has run (the emission ownership of a rank is fixed from then on)
    int64_t emitted_for = -1;         // step whose emission already ran in the tail launch of the step before it (k_tail), also across
                                      // nk_step calls: a driver that steps one by one (Population.run_timestep) then never launches k_emit;
                                      // -1 after anything that changes the store or the tables (the emission is simply run again: its
                                      // counters are double-buffered)
    std::vector<double> h_vg;         // host copy of the group velocities (the mode map deals the modes by their event rate)
    std::vector<int32_t> h_m2s, h_s2m;  // host copies of the mode map (NkDev::m2s / s2m), built with the segmentation
    int32_t *m2s_dev = nullptr, *s2m_dev = nullptr, *nl_dev = nullptr;
    unsigned int *rbar = nullptr;     // k_resident: step word, halt word, one flag per workgroup
    bool walked = false;              // box store: sweeps have alternated since the segments were last moved down (NkDev::seg_lo may be > 0)
    int map_nseg = 0;                 // segmentation the map was dealt for
    NkMode *modetab_p = nullptr;      // permuted mode table (own allocation: its size follows nseg)
    int64_t modetab_p_len = 0;
    void *inbox = nullptr, *inbox_n = nullptr;   // 'one_to_one' spawn inboxes (sized with nseg)
    void *mig_buf = nullptr, *mig_n = nullptr;   // migration inboxes (rough facets; sized with nseg and segcap)
    double *ep_p = nullptr, *rc_p = nullptr;     // (reservoir, mode) tables in the segments' order (sized with nseg)
    int rm_nseg = 0, rm_nlmax = 0;               // segmentation rc_p was built for (0: the counters live in res_counter)
    int32_t halt_words[4] = {0, 0, 0, 0};
    double *acc = nullptr;         // [NB + 2]: tally columns, then the two halt requests that travel with them
    double *hist = nullptr;        // [hist_cap] history rows (NkRow) in pinned host memory
    int hist_cap = 0;
    nk_params params;
    nk_timing timing;
    NkRccl rccl;
    ncclComm_t comm = nullptr;
    int comm_rank = -1, comm_nranks = 0;   // as RCCL reports them (nk_comm_info)
    double comm_selftest = 0.0;
    int num_cu = 256;
    std::vector<int32_t> h_ffo, h_ffi;   // host copies of the mesh's facet -> faces CSR, its area cdf and the vertices
    std::vector<double> h_fcdf, h_verts;
    std::vector<double> h_rbf_inv;       // host copy of the RBF system inverse (sv_interp 3)
    std::vector<NkFacet> host_facets;   // host mirror of d.facets (patched by nk_set_reservoirs / nk_set_rough)
    const double *d_omega = nullptr, *d_vg = nullptr;   // kept to rebuild the packed mode records
    std::vector<double> h_Tgrid;
    double T_lo = 0.0, T_hi = 0.0;      // range of the subvolume temperatures last seen by the host
    // band-resolved heat flux (nk_set_bands, k_spectral): off while band_B == 0 -- then nothing is launched or allocated
    int32_t band_B = 0;                  // bands
    int32_t *band_map = nullptr;         // [M] band of every mode, -1 = none
    double *band_slabs = nullptr;        // per-workgroup partial slabs of k_spectral
    size_t band_slabs_n = 0;
    double *band_rows_d = nullptr;       // reduced rows of a batch's heat-flux steps, [rows][4 S B]
    size_t band_rows_n = 0;
    std::vector<double> band_rows;       // the rows of the last nk_step call: F [S][B][3], then N [S][B]
    std::vector<int64_t> band_steps;     //   and the absolute step of each
    // spatial field maps (nk_set_field, k_field; nk_field.hip): off by default -- then nothing is launched or allocated
    NkFieldHost field;
    // grouped field maps (nk_set_field_groups, k_field<., true>; nk_field.hip): off by default, need a field
    NkFGroupsHost fgroups;
    int64_t map_gen = 0;                 // counts nk_build_mode_map: the groups' permuted table follows the mode map
    // mode-resolved tally (nk_set_modes, k_modes; nk_modes.hip): off by default -- then nothing is launched or allocated
    NkModesHost modes;
    double res_T_max = 0.0;              // highest reservoir temperature (nk_set_reservoirs): bounds the field's terms
    // free-path sampling (nk_free_paths, k_free_paths<*, false>; nk_freepath.hip): the last call's report -- nothing is kept on the device
    nk_free_path_report fp_last = {};
    int32_t fc_calls = 0;        // nk_free_paths_columns calls so far (k_free_columns; nk_freecols.hip)
    int32_t kin_calls = 0;       // nk_kinetic_flights calls so far (k_kinetic; nk_kinetic.hip)
    nk_free_path_map_report fm_last = {};   // the last nk_free_paths_map call's report (k_free_paths<*, true>; nk_freepath.hip)
};

#define NK_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
            return NK_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)
#define NK_ARG(cond, msg)                                                                              \
    do {                                                                                               \
        if (!(cond)) { ctx->err = msg; return NK_ERR_ARG; }                                            \
    } while (0)
#define NK_TRY(call)                                                                                   \
    do { int rc_ = (call); if (rc_) return rc_; } while (0)

template <class T>
static int nk_upload(nk_ctx *ctx, const T *src, size_t n, const T **dst, bool particle = false) {
    void *p = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    NK_HIP(hipMalloc(&p, bytes));
    (particle ? ctx->pallocs : ctx->allocs).push_back(p);
    if (src && n) NK_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    else NK_HIP(hipMemset(p, 0, bytes));
    *dst = (const T *)p;
    return NK_OK;
}
#define NK_UP(src, n, dst) NK_TRY(nk_upload(ctx, src, n, dst))
// One zeroed array of the particle store, registered in ctx->pallocs.
template <class T>
static int nk_palloc(nk_ctx *ctx, T *&field, size_t count) {
    const T *p = nullptr;
    NK_TRY(nk_upload<T>(ctx, nullptr, count, &p, true));
    field = (T *)p;
    return NK_OK;
}

// The particle fields of a store of `cap` slots (a multiple of 64): ONE allocation cut into blocks of 64 slots, every block
// x | y | z | occ | [nts] | [pid] | w0 (NkField, nk_device.h; the sweep addresses a block's fields from ONE base pointer at
// compile-time distances, NkBlock).  The allocation is registered in ctx->pallocs.
// bytes of one particle in the store: x y z occ (+ nts unless it is a box store) (+ pid) + the packed word
static inline int nk_particle_bytes(bool with_pid, bool with_nts) { return 36 + (with_nts ? 8 : 0) + (with_pid ? 8 : 0); }
static inline size_t nk_store_bytes(int64_t cap, bool with_pid, bool with_nts) {
    const int64_t nblk = (cap + 63) / 64;
    const int nf = 4 + (with_nts ? 1 : 0) + (with_pid ? 1 : 0);   // 8-byte fields per particle
    const int bd = nf * 64 + 32;                                  // doubles per block (the 64 packed words take 32)
    const size_t bytes = (size_t)nblk * bd * 8;
    return bytes ? bytes : 64;
}
// the fields of a store of `cap` slots that starts at b
static void nk_point_fields(NkDev &d, double *b, int64_t cap, bool with_pid, bool with_nts) {
    const int nf = 4 + (with_nts ? 1 : 0) + (with_pid ? 1 : 0);
    const int bd = nf * 64 + 32;
    int k = 4;
    d.x = {b, bd}; d.y = {b + 64, bd}; d.z = {b + 128, bd}; d.occ = {b + 192, bd};
    d.nts = {with_nts ? b + 64 * (k++) : nullptr, bd};
    d.pid = {with_pid ? (uint64_t *)(b + 64 * (k++)) : nullptr, bd};
    d.w0 = {(uint32_t *)(b + 64 * k), 2 * bd};
}
static int nk_alloc_fields(nk_ctx *ctx, NkDev &d, int64_t cap, bool with_pid, bool with_nts) {
    const size_t bytes = nk_store_bytes(cap, with_pid, with_nts);
    void *buf = nullptr;
    // developer probe (scripts/placement_probe.py): NK_STORE_PAD_KB shifts the store inside a larger allocation
    const size_t pad = getenv("NK_STORE_PAD_KB") ? (size_t)atol(getenv("NK_STORE_PAD_KB")) * 1024 : 0;
    NK_HIP(hipMalloc(&buf, bytes + pad));
    ctx->pallocs.push_back(buf);
    NK_HIP(hipMemsetAsync(buf, 0, bytes + pad, ctx->stream));
    ctx->store_buf = buf; ctx->store_pad = pad; ctx->store_pid = with_pid; ctx->store_nts = with_nts;
    nk_point_fields(d, (double *)((char *)buf + pad), cap, with_pid, with_nts);
    return NK_OK;
}
// Host copy of a whole field (slot order) and back.
template <class T>
static int nk_field_download(nk_ctx *ctx, const NkDev &d, const NkField<T> &f, std::vector<T> &out) {
    // the field's elements are strided by blocks: copy block-wise with hipMemcpy2D (rows of 64 elements)
    out.resize((size_t)d.cap);
    const int64_t nblk = d.cap / 64;
    if (nblk == 0) return NK_OK;
    NK_HIP(hipMemcpy2D(out.data(), 64 * sizeof(T), f.p, (size_t)f.blk * sizeof(T), 64 * sizeof(T), (size_t)nblk, hipMemcpyDeviceToHost));
    return NK_OK;
}
template <class T>
static int nk_field_upload(nk_ctx *ctx, const NkDev &d, const NkField<T> &f, const T *src) {
    const int64_t nblk = d.cap / 64;
    if (nblk == 0) return NK_OK;
    NK_HIP(hipMemcpy2D(f.p, (size_t)f.blk * sizeof(T), src, 64 * sizeof(T), 64 * sizeof(T), (size_t)nblk, hipMemcpyHostToDevice));
    return NK_OK;
}

// 1 = ray-casting tables fit LDS, 2 = they stay in global memory
static inline int nk_geom_mode(const nk_ctx *ctx) { return (ctx->d.F <= NK_LDS_FACES && ctx->d.Fc <= NK_LDS_FACES) ? 1 : 2; }
// kind: 0 plain, 1 k_emit (emission scratch), 2 / 3 k_sweep (mode records, carry without / with ids)
static inline bool nk_want_split(const nk_ctx *ctx);
static inline size_t nk_lds(const nk_ctx *ctx, bool geom, int kind = 0) {
    const NkDev &d = ctx->d;
    const int gm = geom ? nk_geom_mode(ctx) : 0;
    return nk_lds_bytes(d.S, d.R, d.F, d.NP, d.Fc, gm, kind, (gm == 1 && d.res_lds) ? d.res_nf : 0, d.rbf_P, d.nlrec, nk_want_split(ctx) ? 0 : 1);
}
// k_tail: the emission's tables or the reduce's scratch, whichever is larger
static inline size_t nk_tail_lds(const nk_ctx *ctx) { return std::max(nk_lds(ctx, true, 1), (size_t)(NK_WG * 8 + 16)); }
#define NK_GEOM_LAUNCH(kernel, grid, lds, ...)                                                        \
    do {                                                                                               \
        if (nk_geom_mode(ctx) == 1) kernel<1><<<grid, NK_WG, lds, ctx->stream>>>(__VA_ARGS__);         \
        else kernel<2><<<grid, NK_WG, lds, ctx->stream>>>(__VA_ARGS__);                                \
    } while (0)
// k_emit / k_tail: the same, plus the box store's variant (no first ray cast)
#define NK_EMIT_LAUNCH(kernel, grid, lds, ...)                                                        \
    do {                                                                                               \
        if (ctx->d.box) kernel<1, true><<<grid, NK_WG, lds, ctx->stream>>>(__VA_ARGS__);               \
        else if (nk_geom_mode(ctx) == 1) kernel<1, false><<<grid, NK_WG, lds, ctx->stream>>>(__VA_ARGS__);   \
        else kernel<2, false><<<grid, NK_WG, lds, ctx->stream>>>(__VA_ARGS__);                         \
    } while (0)
static inline int nk_sweep_grid(const nk_ctx *ctx) { return ctx->num_cu * 8; }
// 1 / 2: slice subvolumes, 'nearest' / 'linear' particle temperatures and the local reference temperature (k_sweep's FAST)
static inline int nk_sweep_fast(const nk_ctx *ctx) {
    const NkDev &d = ctx->d;
    if (getenv("NK_NO_FAST")) return 0;              // developer probe
    return (d.sv_kind == 0 && d.T_ref_local && (d.sv_interp == 0 || d.sv_interp == 1)) ? 1 + d.sv_interp : 0;
}
// the sweep keeps its segments' mode records in LDS when the modes are partitioned over the segments and a segment's share fits
static inline bool nk_want_lrec(const nk_ctx *ctx) { return ctx->d.nlrec > 0; }      // decided with the segmentation (nk_alloc_particles)

// nk_kind.h: the dynamic LDS every kernel function has been allowed so far, per device, for the whole process
hipError_t nk_allow_lds(const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> allowed;
    int device = 0;
    if (bytes <= 64 * 1024) return hipSuccess;
    hipError_t e = hipGetDevice(&device);
    std::lock_guard<std::mutex> lock(mu);
    size_t &mark = allowed[{device, fn}];
    if (e != hipSuccess || bytes <= mark) return e;
    if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) == hipSuccess) mark = bytes;
    return e;
}

// The mode records hold three lifetime rows (two grid intervals) around the live temperature range [T_lo, T_hi] and
// E0 = exp(hbar omega / (kB T0)) at its middle T0 (nk_device.h "lean FP64 arithmetic"); rebuilt when the range leaves the
// window or drifts away from T0, and whenever the segmentation (hence the permuted copy) changes.
static int nk_update_tau_window(nk_ctx *ctx, bool force) {
    NkDev &d = ctx->d;
    if (!ctx->have_material) return NK_OK;
    const std::vector<double> &g = ctx->h_Tgrid;
    const double Tm = 0.5 * (ctx->T_lo + ctx->T_hi);
    int i = (int)(std::lower_bound(g.begin(), g.end(), Tm) - g.begin()) - 1;          // interval (g[i], g[i+1]] holds T_mid
    if (i < 0) i = 0;
    // the second interval on the side where the range reaches further
    int row0 = (i + 1 < d.NT && ctx->T_hi - g[std::min(i + 1, d.NT - 1)] > g[i] - ctx->T_lo) ? i : i - 1;
    if (row0 > d.NT - NK_TAU_ROWS) row0 = d.NT - NK_TAU_ROWS;
    if (row0 < 0) row0 = 0;
    const bool window_ok = d.tau_row0 >= 0 && ctx->T_lo > g[d.tau_row0] &&
                           ctx->T_hi <= g[std::min(d.tau_row0 + NK_TAU_ROWS - 1, d.NT - 1)];
    const bool window_best = d.tau_row0 == row0;                   // a range wider than two intervals: keep the best window
    const bool t0_ok = d.T0 > 0.0 && fabs(ctx->T_lo - d.T0) <= 0.02 * d.T0 && fabs(ctx->T_hi - d.T0) <= 0.02 * d.T0;
    const bool t0_best = d.T0 > 0.0 && fabs(Tm - d.T0) <= 0.002 * d.T0;
    if (!force && (window_ok || window_best) && (t0_ok || t0_best)) return NK_OK;
    d.T0 = Tm > 0.0 ? Tm : 300.0;
    d.invT0 = 1.0 / d.T0;
    d.c_hk = d.hbar / d.kb;
    NkMode *tp = nullptr;
    if (d.part && d.nseg > 0 && d.m2s) {
        const int64_t need = (int64_t)d.nseg * d.nlmax;
        if (need > ctx->modetab_p_len) {
            if (ctx->modetab_p) hipFree(ctx->modetab_p);
            ctx->modetab_p = nullptr; ctx->modetab_p_len = 0;
            NK_HIP(hipMalloc((void **)&ctx->modetab_p, (size_t)need * sizeof(NkMode)));
            NK_HIP(hipMemset(ctx->modetab_p, 0, (size_t)need * sizeof(NkMode)));
            ctx->modetab_p_len = need;
        }
        tp = ctx->modetab_p;
    }
    d.modetab_p = tp;
    k_build_modetab<<<(d.M + 255) / 256, 256, 0, ctx->stream>>>(ctx->d_omega, ctx->d_vg, d.tau, d.M, d.NT, row0, d.c_hk, d.invT0,
                                                                  d.nseg > 0 ? d.nseg : 1, d.nlmax, d.m2s, (NkMode *)d.modetab, tp);
    NK_HIP(hipGetLastError());
    d.tau_row0 = row0;
    ctx->timing.tau_rebuilds += 1;
    for (int k = 0; k < NK_TAU_ROWS; ++k) d.tau_g[k] = (row0 + k < d.NT) ? g[row0 + k] : INFINITY;
    for (int k = 0; k + 1 < NK_TAU_ROWS; ++k) d.tau_ig[k] = 1.0 / (d.tau_g[k + 1] - d.tau_g[k]);
    if (d.NT < NK_TAU_ROWS) d.tau_g[0] = INFINITY;     // no packed window: every lookup takes the full-table path
    return NK_OK;
}

static void nk_track_T(nk_ctx *ctx, const double *T, int S) {
    double lo = T[0], hi = T[0];
    for (int i = 1; i < S; ++i) { lo = std::min(lo, T[i]); hi = std::max(hi, T[i]); }
    ctx->T_lo = lo; ctx->T_hi = hi;
}

extern "C" {

const char *nk_last_error(const nk_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int nk_device_count(void) {
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess ? ndev : 0;
}

int nk_create(nk_ctx **out, int device_id, uint64_t seed) {
    if (!out) { g_create_error = "nk_create: out is NULL"; return NK_ERR_ARG; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("nk_create: no HIP device available (") + hipGetErrorString(e) +
                         "); this library has no CPU fallback";
        return NK_ERR_NODEVICE;
    }
    if (device_id < 0 || device_id >= ndev) { g_create_error = "nk_create: device_id out of range"; return NK_ERR_ARG; }
    nk_ctx *ctx = new nk_ctx();
    memset(&ctx->d, 0, sizeof(NkDev));
    memset(&ctx->params, 0, sizeof(nk_params));
    memset(&ctx->timing, 0, sizeof(nk_timing));
    ctx->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreate(&ctx->stream)) != hipSuccess) {
        g_create_error = std::string("nk_create: ") + hipGetErrorString(e);
        delete ctx;
        return NK_ERR_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        ctx->num_cu = prop.multiProcessorCount;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            g_create_error = std::string("nk_create: device is ") + prop.gcnArchName + ", this build targets gfx950 only";
            hipStreamDestroy(ctx->stream);
            delete ctx;
            return NK_ERR_NODEVICE;
        }
    }
    ctx->d.seed = seed;
    ctx->d.rank = 0;
    ctx->d.nranks = 1;
    ctx->d.tau_row0 = -1;
    ctx->d.stamps = nullptr;
    ctx->params.dt = 1.0; ctx->params.T_ref_local = 1; ctx->params.flux_every = 10; ctx->params.contains_every = 100;
    ctx->d.dt = 1.0; ctx->d.inv_dt = 1.0; ctx->d.T_ref_local = 1;
    // bookkeeping words in device memory: halt[4], overflow, ticket, ev_ticket
    const int32_t *p32 = nullptr;
    int rc;
    if ((rc = nk_upload<int32_t>(ctx, nullptr, 16, &p32))) {
        g_create_error = ctx->err;
        delete ctx;
        return rc;
    }
    ctx->d.halt = (int32_t *)p32;
    ctx->d.overflow = (int32_t *)p32 + 4;
    ctx->d.ticket = (int32_t *)p32 + 5;
    ctx->d.ev_ticket = (int32_t *)p32 + 6;
    ctx->anomalies = (int32_t *)p32 + 7;
    *out = ctx;
    return NK_OK;
}

static void nk_specular_free(nk_ctx *ctx);

void nk_destroy(nk_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (ctx->comm && ctx->rccl.CommDestroy) ctx->rccl.CommDestroy(ctx->comm);
    for (auto &e : ctx->evpool) hipEventDestroy(e);
    nk_specular_free(ctx);
    for (void *p : ctx->allocs) hipFree(p);
    for (void *p : ctx->pallocs) hipFree(p);
    if (ctx->acc) hipFree(ctx->acc);
    if (ctx->rbar) hipFree(ctx->rbar);
    if (ctx->hist) hipHostFree(ctx->hist);
    if (ctx->modetab_p) hipFree(ctx->modetab_p);
    if (ctx->m2s_dev) hipFree(ctx->m2s_dev);
    if (ctx->s2m_dev) hipFree(ctx->s2m_dev);
    if (ctx->nl_dev) hipFree(ctx->nl_dev);
    if (ctx->inbox) hipFree(ctx->inbox);
    if (ctx->inbox_n) hipFree(ctx->inbox_n);
    if (ctx->mig_buf) hipFree(ctx->mig_buf);
    if (ctx->mig_n) hipFree(ctx->mig_n);
    if (ctx->ep_p) hipFree(ctx->ep_p);
    if (ctx->rc_p) hipFree(ctx->rc_p);
    if (ctx->band_map) hipFree(ctx->band_map);
    if (ctx->band_slabs) hipFree(ctx->band_slabs);
    if (ctx->band_rows_d) hipFree(ctx->band_rows_d);
    nk_field_free(ctx->field);
    nk_fgroups_free(ctx->fgroups);
    nk_modes_free(ctx->modes);
    hipStreamDestroy(ctx->stream);
    delete ctx;
}

int nk_set_material(nk_ctx *ctx, const nk_material *m) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && m, "nk_set_material: NULL argument");
    NK_ARG(m->Q > 0 && m->J > 0 && m->NT >= 2 && m->nE >= 2, "nk_set_material: bad sizes");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    d.Q = m->Q; d.J = m->J; d.NT = m->NT; d.M = m->Q * m->J;
    for (int i = 1; i < m->NT; ++i) NK_ARG(m->T_grid[i] > m->T_grid[i - 1], "nk_set_material: T_grid must ascend");
    NK_UP(m->omega, (size_t)d.M, &ctx->d_omega);
    NK_UP(m->group_vel, (size_t)d.M * 3, &ctx->d_vg);
    ctx->h_vg.assign(m->group_vel, m->group_vel + (size_t)d.M * 3);
    NK_UP((const NkMode *)nullptr, (size_t)d.M, &d.modetab);
    NK_UP(m->lifetime, (size_t)d.NT * d.M, &d.tau);
    NK_UP(m->T_grid, (size_t)d.NT, &d.Tgrid);
    ctx->h_Tgrid.assign(m->T_grid, m->T_grid + m->NT);
    d.nE = m->nE;
    NK_UP(m->T_array, (size_t)d.nE, &d.Tarr);
    NK_UP(m->energy_array, (size_t)d.nE, &d.Earr);
    d.Tfill_lo = m->T_fill_lo; d.Tfill_hi = m->T_fill_hi;
    d.hbar = m->hbar; d.kb = m->kb; d.QV = m->QV; d.active_modes = (double)m->active_modes;
    ctx->have_material = true;
    ctx->T_lo = ctx->T_hi = m->T_grid[0];
    int rc = nk_update_tau_window(ctx, true);
    if (rc) return rc;
    NK_HIP(hipStreamSynchronize(ctx->stream));
    return NK_OK;
}

// One reference of the face tree: a face and the box of the piece of it this reference stands for.
struct NkFaceRef { int face; double lo[3], hi[3]; };
// Cuts the (convex, planar) polygon P at the plane x_axis = c; keeps the side `upper`.
static int nk_clip_polygon(const double (*P)[3], int n, int axis, double c, bool upper, double (*out)[3]) {
    int no = 0;
    for (int i = 0; i < n; ++i) {
        const double *A = P[i], *B = P[(i + 1) % n];
        const bool ina = upper ? A[axis] >= c : A[axis] <= c, inb = upper ? B[axis] >= c : B[axis] <= c;
        if (ina) { for (int k = 0; k < 3; ++k) out[no][k] = A[k]; ++no; }
        if (ina != inb) {
            const double t = (c - A[axis]) / (B[axis] - A[axis]);
            for (int k = 0; k < 3; ++k) out[no][k] = A[k] + t * (B[k] - A[k]);
            out[no][axis] = c;
            ++no;
        }
    }
    return no;
}
static void nk_split_polygon(const double (*P)[3], int n, int face, int depth, std::vector<NkFaceRef> &refs) {
    NkFaceRef r;
    r.face = face;
    for (int k = 0; k < 3; ++k) { r.lo[k] = 1e300; r.hi[k] = -1e300; }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { r.lo[k] = std::min(r.lo[k], P[i][k]); r.hi[k] = std::max(r.hi[k], P[i][k]); }
    double area2[3] = {0, 0, 0};                        // twice the polygon's vector area
    for (int i = 1; i + 1 < n; ++i) {
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) { a[k] = P[i][k] - P[0][k]; b[k] = P[i + 1][k] - P[0][k]; }
        area2[0] += a[1] * b[2] - a[2] * b[1]; area2[1] += a[2] * b[0] - a[0] * b[2]; area2[2] += a[0] * b[1] - a[1] * b[0];
    }
    const double area = 0.5 * sqrt(area2[0] * area2[0] + area2[1] * area2[1] + area2[2] * area2[2]);
    const double e[3] = {r.hi[0] - r.lo[0], r.hi[1] - r.lo[1], r.hi[2] - r.lo[2]};
    const double box_area = e[0] * e[1] + e[1] * e[2] + e[0] * e[2];      // half the box's surface
    int axis = 0;
    for (int k = 1; k < 3; ++k) if (e[k] > e[axis]) axis = k;
    if (depth <= 0 || n < 3 || n > 12 || !(box_area > 3.0 * area) || !(e[axis] > 0.0)) { refs.push_back(r); return; }
    const double c = 0.5 * (r.lo[axis] + r.hi[axis]);
    double lo[16][3], hi[16][3];
    const int nl = nk_clip_polygon(P, n, axis, c, false, lo), nh = nk_clip_polygon(P, n, axis, c, true, hi);
    if (nl < 3 || nh < 3) { refs.push_back(r); return; }
    nk_split_polygon(lo, nl, face, depth - 1, refs);
    nk_split_polygon(hi, nh, face, depth - 1, refs);
}
static void nk_split_face(const double *V, int face, int max_depth, std::vector<NkFaceRef> &refs) {
    double P[16][3];
    for (int a = 0; a < 3; ++a) for (int k = 0; k < 3; ++k) P[a][k] = V[3 * a + k];
    nk_split_polygon(P, 3, face, max_depth, refs);
}

int nk_set_mesh(nk_ctx *ctx, const nk_mesh *m) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && m, "nk_set_mesh: NULL argument");
    NK_ARG(m->F > 0 && m->Fc > 0, "nk_set_mesh: empty mesh");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    d.F = m->F; d.Fc = m->Fc; d.tol = m->tol;
    for (int i = 0; i < 6; ++i) d.bbox[i] = m->bbox[i];
    // distinct planes (bitwise-equal normal and k), in order of their first face; faces grouped by plane
    std::vector<std::vector<int>> members;
    for (int f = 0; f < m->F; ++f) {
        int found = -1;
        for (size_t pl = 0; pl < members.size() && found < 0; ++pl) {
            int g = members[pl][0];
            if (m->normals[3 * g] == m->normals[3 * f] && m->normals[3 * g + 1] == m->normals[3 * f + 1] &&
                m->normals[3 * g + 2] == m->normals[3 * f + 2] && m->k[g] == m->k[f])
                found = (int)pl;
        }
        if (found < 0) { members.push_back(std::vector<int>()); found = (int)members.size() - 1; }
        members[found].push_back(f);
    }
    d.NP = (int)members.size();
    std::vector<double> planes((size_t)d.NP * NK_PLANE_DOUBLES, 0.0), faces((size_t)m->F * NK_FACE_DOUBLES, 0.0);
    std::vector<int> face_pos((size_t)m->F, 0);     // where face f went
    int pos = 0;
    for (int pl = 0; pl < d.NP; ++pl) {
        double *p = &planes[(size_t)pl * NK_PLANE_DOUBLES];
        int g = members[pl][0];
        p[0] = m->normals[3 * g]; p[1] = m->normals[3 * g + 1]; p[2] = m->normals[3 * g + 2]; p[3] = m->k[g];
        int32_t rng[2] = {pos, pos + (int)members[pl].size()};
        memcpy(p + 4, rng, 8);
        for (int f : members[pl]) {
            double *q = &faces[(size_t)pos * NK_FACE_DOUBLES];
            for (int k = 0; k < 3; ++k) {
                q[k] = m->bounds_lo[3 * f + k]; q[3 + k] = m->bounds_hi[3 * f + k]; q[6 + k] = m->origins[3 * f + k];
            }
            const double *A = m->basis + 9 * f;      // A[d][b]: columns are (e1, e2, n)
            double a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[3], a11 = A[4], a12 = A[5], a20 = A[6], a21 = A[7], a22 = A[8];
            double det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
            NK_ARG(det != 0.0 && isfinite(det), "nk_set_mesh: degenerate face");
            q[9] = (a11 * a22 - a12 * a21) / det; q[10] = (a02 * a21 - a01 * a22) / det; q[11] = (a01 * a12 - a02 * a11) / det;
            q[12] = (a12 * a20 - a10 * a22) / det; q[13] = (a00 * a22 - a02 * a20) / det; q[14] = (a02 * a10 - a00 * a12) / det;
            int32_t id[2] = {f, m->face_facet[f]};
            memcpy(q + 15, id, 8);
            face_pos[f] = pos;
            ++pos;
        }
    }
    // Large meshes (tables in global memory): the face tree of nk_find_boundary_tree.  Faces in Morton order of their box
    // centres, leaves of 4, every level the unions of 4 consecutive nodes of the level below.
    d.NG = 0;
    d.tree_top = 0; d.tree_leaves = 0;
    d.tree_nfam = 0; d.tree_lds_fam0 = 0; d.tree_lds_off = 0;
    for (int k = 0; k < NK_TREE_LEVELS; ++k) d.tree_base[k] = 0;
    bool use_tree = !(m->F <= NK_LDS_FACES && m->Fc <= NK_LDS_FACES) && !getenv("NK_NO_TREE");   // env: developer probe
    std::vector<NkFaceRef> refs;
    if (use_tree) {
        // A sliver lying diagonally has a box far larger than itself (the 1250 fan triangles of a wire's cap each cover an
        // eighth of the cap), so such faces enter the tree as several references, each with the box of one piece of the
        // triangle.  The face test itself is unchanged: a face met twice gives the same answer twice.
        const int max_depth = getenv("NK_TREE_SPLIT") ? atoi(getenv("NK_TREE_SPLIT")) : 4;
        for (int f = 0; f < m->F; ++f) nk_split_face(m->vertices + 9 * (size_t)f, f, max_depth, refs);
        if (refs.size() > (size_t)4 * (1 << (2 * NK_TREE_LEVELS))) {      // too many for the implicit tree: whole faces
            refs.clear();
            for (int f = 0; f < m->F; ++f) nk_split_face(m->vertices + 9 * (size_t)f, f, 0, refs);
        }
        use_tree = refs.size() <= (size_t)4 * (1 << (2 * NK_TREE_LEVELS));
    }
    if (use_tree) {
        const int F = (int)refs.size();
        // Shape: `top` levels of 4 below a top family of c = 2..4 nodes, every node present, so that the walk's index
        // arithmetic needs no child pointers; leaves hold 2 to 4 references.  Contents: top-down, every node's references
        // dealt evenly to its children after ordering them along the longest axis of their centres (median cuts) --
        // consecutive Morton codes cut at fixed counts gave boxes that a ray entered 35-45 times per cast.
        int top = 0;
        while ((int64_t)4 << (2 * top) < (int64_t)(F + 3) / 4) ++top;
        const int per_top = 1 << (2 * top);                                    // leaves below one node of the top family
        const int c_top = std::max(1, (int)(((int64_t)(F + 3) / 4 + per_top - 1) / per_top));
        const int NL = c_top * per_top;
        std::vector<int> order((size_t)F), slot((size_t)NL * 4, -1);
        for (int i = 0; i < F; ++i) order[i] = i;
        std::vector<double> cen((size_t)F * 3);
        for (int i = 0; i < F; ++i) for (int k = 0; k < 3; ++k) cen[3 * (size_t)i + k] = 0.5 * (refs[i].lo[k] + refs[i].hi[k]);
        // cut [a, b) into parts of the given sizes along the longest axis of the centres, two groups at a time
        std::function<void(int, int, const int *, int)> cut = [&](int a, int b, const int *sizes, int n) {
            if (n <= 1 || b - a <= 1) return;
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            for (int i = a; i < b; ++i)
                for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], cen[3 * (size_t)order[i] + k]); hi[k] = std::max(hi[k], cen[3 * (size_t)order[i] + k]); }
            int axis = 0;
            for (int k = 1; k < 3; ++k) if (hi[k] - lo[k] > hi[axis] - lo[axis]) axis = k;
            const int nl = n / 2;
            int left = 0;
            for (int i = 0; i < nl; ++i) left += sizes[i];
            if (left > 0 && left < b - a)
                std::nth_element(order.begin() + a, order.begin() + a + left, order.begin() + b, [&](int p, int q) {
                    const double cp = cen[3 * (size_t)p + axis], cq = cen[3 * (size_t)q + axis];
                    return cp < cq || (cp == cq && p < q);
                });
            cut(a, a + left, sizes, nl);
            cut(a + left, b, sizes + nl, n - nl);
        };
        std::function<void(int, int, int, int)> deal = [&](int a, int b, int level, int node) {   // node of `level` gets [a, b)
            if (level == 0) {
                for (int i = a; i < b; ++i) slot[(size_t)4 * node + (i - a)] = order[i];
                return;
            }
            int sizes[4];
            for (int k = 0; k < 4; ++k) sizes[k] = (b - a) / 4 + (k < (b - a) % 4 ? 1 : 0);
            cut(a, b, sizes, 4);
            int pos = a;
            for (int k = 0; k < 4; ++k) { deal(pos, pos + sizes[k], level - 1, 4 * node + k); pos += sizes[k]; }
        };
        {
            int sizes[4] = {0, 0, 0, 0};
            for (int k = 0; k < c_top; ++k) sizes[k] = F / c_top + (k < F % c_top ? 1 : 0);
            cut(0, F, sizes, c_top);
            int pos = 0;
            for (int k = 0; k < c_top; ++k) { deal(pos, pos + sizes[k], top, k); pos += sizes[k]; }
        }
        // leaf records (NK_TREE_LEAF_DOUBLES, nk_device.h): the four faces' boxes in single precision (filled in below, once the
        // slack is known), then per face plane, box, barycentric rows; the padding faces keep n = k = 0 and can never be hit
        std::vector<double> tf((size_t)NL * NK_TREE_LEAF_DOUBLES, 0.0);
        for (size_t i = 0; i < slot.size(); ++i) {
            if (slot[i] < 0) continue;
            const int f = refs[slot[i]].face;
            double *q = &tf[(i / 4) * NK_TREE_LEAF_DOUBLES + 16 + 20 * (i % 4)];
            const double *src = &faces[(size_t)face_pos[f] * NK_FACE_DOUBLES];
            q[0] = m->normals[3 * f]; q[1] = m->normals[3 * f + 1]; q[2] = m->normals[3 * f + 2]; q[3] = m->k[f];
            memcpy(q + 4, src, NK_FACE_DOUBLES * sizeof(double));
        }
        // boxes: union of the member faces' boxes, inflated by far more than any rounding in the slab test
        double big = 0.0;
        for (int k = 0; k < 6; ++k) big = std::max(big, fabs(m->bbox[k]));
        // ... and, for a piece of a face, by the slack of the barycentric test (a point accepted with u = -tol lies
        // tol * |edge| outside the triangle)
        const double margin = m->tol + 1e-6 * (1.0 + big);
        std::vector<double> slack((size_t)m->F);
        for (int f = 0; f < m->F; ++f) {
            const double *V = m->vertices + 9 * (size_t)f;
            double e = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int k = 0; k < 3; ++k) e = std::max(e, fabs(V[3 * a + k] - V[3 * ((a + 1) % 3) + k]));
            slack[f] = margin + 8.0 * m->tol * e;
        }
        for (size_t i = 0; i < slot.size(); ++i) {           // the faces' own boxes, rounded outwards (padding: a box no ray enters)
            float *fb = reinterpret_cast<float *>(&tf[(i / 4) * NK_TREE_LEAF_DOUBLES]) + 6 * (i % 4);
            for (int k = 0; k < 3; ++k) {
                if (slot[i] < 0) { fb[k] = 3.0e38f; fb[3 + k] = -3.0e38f; continue; }
                const NkFaceRef &r = refs[slot[i]];
                fb[k] = nextafterf((float)(r.lo[k] - slack[r.face]), -INFINITY);
                fb[3 + k] = nextafterf((float)(r.hi[k] + slack[r.face]), INFINITY);
            }
        }
        std::vector<double> boxes;
        int count = NL, level = 0, prev_base = 0;
        for (;;) {
            const int padded = (count + 3) / 4 * 4, base = (int)(boxes.size() / 6);
            d.tree_base[level] = base;
            boxes.resize(boxes.size() + (size_t)padded * 6, 0.0);
            for (int i = 0; i < count; ++i) {
                double *B = &boxes[(size_t)(base + i) * 6];
                for (int k = 0; k < 3; ++k) { B[k] = 1e300; B[3 + k] = -1e300; }
                if (level == 0) {
                    for (int c = 4 * i; c < 4 * i + 4; ++c) {
                        if (slot[c] < 0) continue;
                        const NkFaceRef &r = refs[slot[c]];
                        for (int k = 0; k < 3; ++k) {
                            B[k] = std::min(B[k], r.lo[k] - slack[r.face]);
                            B[3 + k] = std::max(B[3 + k], r.hi[k] + slack[r.face]);
                        }
                    }
                } else {
                    const int below = (int)((size_t)(base - prev_base));   // nodes stored for the level below (padded)
                    for (int c = 4 * i; c < 4 * i + 4 && c < below; ++c) {
                        const double *C = &boxes[(size_t)(prev_base + c) * 6];
                        if (C[0] > C[3]) continue;                          // padding node
                        for (int k = 0; k < 3; ++k) { B[k] = std::min(B[k], C[k]); B[3 + k] = std::max(B[3 + k], C[3 + k]); }
                    }
                }
            }
            for (int i = count; i < padded; ++i) {                          // padding nodes: never entered (index >= count)
                double *B = &boxes[(size_t)(base + i) * 6];
                for (int k = 0; k < 3; ++k) { B[k] = 1e300; B[3 + k] = -1e300; }
            }
            if (count <= 4) break;
            prev_base = base;
            count = (count + 3) / 4;
            ++level;
        }
        d.tree_top = level;
        d.tree_nfam = (int32_t)(boxes.size() / 24);
        d.tree_lds_fam0 = d.tree_nfam; d.tree_lds_off = 0;
        auto tree_base_of = [&](int lv) { return (int)d.tree_base[lv]; };
        d.tree_leaves = NL;
        d.NG = 1;
        // facet tags: the facet of a node whose faces all belong to one facet, else -1 (nk_tree_skip)
        std::vector<int32_t> tags(boxes.size() / 6, -1);
        {
            const int nlev = level + 1;
            int cnt = NL;
            for (int lv = 0; lv < nlev; ++lv) {
                const int b0 = tree_base_of(lv);
                for (int i = 0; i < cnt; ++i) {
                    int tag = -3;                               // -3: nothing seen yet
                    for (int c = 4 * i; c < 4 * i + 4; ++c) {
                        int t;
                        if (lv == 0) { if (slot[c] < 0) continue; t = m->face_facet[refs[slot[c]].face]; }
                        else { const int below = tree_base_of(lv) - tree_base_of(lv - 1); if (c >= below) continue; t = tags[(size_t)tree_base_of(lv - 1) + c]; if (t == -3) continue; }
                        tag = (tag == -3) ? t : (tag == t ? tag : -1);
                    }
                    tags[(size_t)b0 + i] = tag == -3 ? -1 : tag;
                }
                cnt = (cnt + 3) / 4;
            }
        }
        // families of four: single-precision boxes rounded outwards (one ulp further than the nearest float: cheap and safe)
        const size_t nfam = boxes.size() / 24;
        std::vector<float> fboxes(nfam * NK_TREE_FAMILY_FLOATS);
        double bound = 0.0;
        for (size_t f = 0; f < nfam; ++f) {
            for (int j = 0; j < 24; ++j) {
                const bool is_lo = (j % 6) < 3;
                double v = boxes[f * 24 + j];
                if (v > 3.0e38) v = 3.0e38;                     // padding nodes (never entered)
                if (v < -3.0e38) v = -3.0e38;
                fboxes[f * NK_TREE_FAMILY_FLOATS + j] = nextafterf((float)v, is_lo ? -INFINITY : INFINITY);
                if (fabs(v) < 1e37) bound = std::max(bound, fabs(v));
            }
        }
        d.tree_bound = bound;
        NK_UP(fboxes.data(), fboxes.size(), &d.tree_boxes);
        NK_UP(tags.data(), tags.size(), &d.tree_tags);
        NK_UP(tf.data(), tf.size(), &d.tree_faces);
    }
    NK_UP(planes.data(), planes.size(), &d.planes);
    NK_UP(faces.data(), faces.size(), &d.faces);
    NK_UP(m->vertices, (size_t)m->F * 9, &d.face_verts);
    NK_UP(m->facet_face_off, (size_t)m->Fc + 1, &d.facet_face_off);
    const int nidx = m->facet_face_off[m->Fc];
    NK_UP(m->facet_face_idx, (size_t)nidx, &d.facet_face_idx);
    std::vector<double> cdf((size_t)nidx, 1.0);
    for (int fc = 0; fc < m->Fc; ++fc) {          // np.random.choice(p=areas/sum): cdf = cumsum(p); cdf /= cdf[-1]
        int f0 = m->facet_face_off[fc], f1 = m->facet_face_off[fc + 1];
        double tot = 0.0, acc = 0.0;
        for (int a = f0; a < f1; ++a) tot += m->face_area[m->facet_face_idx[a]];
        for (int a = f0; a < f1; ++a) { acc += m->face_area[m->facet_face_idx[a]] / tot; cdf[a] = acc; }
        for (int a = f0; a < f1; ++a) cdf[a] /= cdf[f1 - 1];
    }
    NK_UP(cdf.data(), cdf.size(), &d.facet_face_cdf);
    ctx->h_ffo.assign(m->facet_face_off, m->facet_face_off + m->Fc + 1);
    ctx->h_ffi.assign(m->facet_face_idx, m->facet_face_idx + nidx);
    ctx->h_fcdf = cdf;
    ctx->h_verts.assign(m->vertices, m->vertices + (size_t)m->F * 9);
    std::vector<NkFacet> fct((size_t)m->Fc);
    for (int fc = 0; fc < m->Fc; ++fc) {
        NkFacet &q = fct[fc];
        memset(&q, 0, sizeof(q));
        q.cx = m->facet_centroid[3 * fc]; q.cy = m->facet_centroid[3 * fc + 1]; q.cz = m->facet_centroid[3 * fc + 2];
        q.nx = m->facet_normal[3 * fc]; q.ny = m->facet_normal[3 * fc + 1]; q.nz = m->facet_normal[3 * fc + 2];
        q.bc = m->facet_bc[fc]; q.partner = m->facet_partner[fc]; q.res = -1; q.rough = -1;
        NK_ARG(q.bc == 'T' || q.bc == 'F' || q.bc == 'P' || q.bc == 'R', "nk_set_mesh: unknown boundary condition");
        NK_ARG(q.bc != 'P' || (q.partner >= 0 && q.partner < m->Fc), "nk_set_mesh: periodic facet without partner");
        if (q.bc == 'P') {                          // translation of a periodic crossing, Population.py:1467
            const int pf = q.partner;
            q.tx = m->facet_centroid[3 * pf] - q.cx; q.ty = m->facet_centroid[3 * pf + 1] - q.cy; q.tz = m->facet_centroid[3 * pf + 2] - q.cz;
        }
    }
    ctx->host_facets = fct;
    NK_UP(fct.data(), fct.size(), &d.facets);
    {   // how far a facet's faces are from its own plane (nk_tree_skip): largest component of n_face - n_facet, and the
        // largest |n_face . centroid + k_face|
        std::vector<double> fs((size_t)m->Fc * 2, 0.0);
        for (int f = 0; f < m->F; ++f) {
            const int fc = m->face_facet[f];
            if (fc < 0 || fc >= m->Fc) continue;
            const NkFacet &q = fct[fc];
            const double nx = m->normals[3 * f], ny = m->normals[3 * f + 1], nz = m->normals[3 * f + 2];
            const double dn = std::max(fabs(nx - q.nx), std::max(fabs(ny - q.ny), fabs(nz - q.nz)));
            const double dk = fabs(nx * q.cx + ny * q.cy + nz * q.cz + m->k[f]);
            fs[2 * (size_t)fc] = std::max(fs[2 * (size_t)fc], dn);
            fs[2 * (size_t)fc + 1] = std::max(fs[2 * (size_t)fc + 1], dk);
        }
        // only facets of many faces are worth it (a cap, a flat side of an imported mesh): the others say "never"
        std::vector<int> nfaces((size_t)m->Fc, 0);
        for (int f = 0; f < m->F; ++f) if (m->face_facet[f] >= 0 && m->face_facet[f] < m->Fc) ++nfaces[m->face_facet[f]];
        for (int fc = 0; fc < m->Fc; ++fc) if (nfaces[fc] < 16) fs[2 * (size_t)fc] = 1e300;
        NK_UP(fs.data(), fs.size(), &d.facet_skip);
    }
    d.nS = m->nS;
    if (m->nS > 0) {
        NK_UP(m->simplex_pts, (size_t)m->nS * 12, &d.simplex_pts);
        std::vector<double> sc((size_t)m->nS);
        double tot = 0.0, acc = 0.0;
        for (int s = 0; s < m->nS; ++s) tot += m->simplex_vol[s];
        for (int s = 0; s < m->nS; ++s) { acc += m->simplex_vol[s] / tot; sc[s] = acc; }
        for (int s = 0; s < m->nS; ++s) sc[s] /= sc[m->nS - 1];
        NK_UP(sc.data(), sc.size(), &d.simplex_cdf);
    }
    // Box store (nk_device.h, NkDev::box): six planes with exact unit axis normals, one facet each, whose faces are the whole
    // side of the bounding box (two triangles over its four corners).  Then "which wall does a particle meet next, and when"
    // follows from its position alone, with the reference's own expression (nk_box_first_hit), and need not be stored.
    ctx->mesh_box = false;
    if (d.cap == 0) d.box = 0;                       // (an existing store keeps its layout until nk_check_ready re-deals it)
    if (m->F == 12 && m->Fc == 6 && d.NP == 6) {
        bool ok = true;
        int seen = 0;
        int box_facet[6] = {0, 0, 0, 0, 0, 0};
        d.box_ids = 0;
        for (int pl = 0; pl < 6 && ok; ++pl) {
            const double *pn = &planes[(size_t)pl * NK_PLANE_DOUBLES];
            int a = -1, sgn = 0;
            for (int k = 0; k < 3; ++k) {
                if (pn[k] == 1.0 || pn[k] == -1.0) { if (a >= 0) ok = false; a = k; sgn = pn[k] > 0 ? 1 : 0; }
                else if (pn[k] != 0.0) ok = false;
            }
            if (!ok || a < 0) { ok = false; break; }
            const int w = 2 * a + sgn;
            if (seen & (1 << w)) { ok = false; break; }
            seen |= 1 << w;
            const double wall = sgn ? -pn[3] : pn[3];              // n.x + k = 0  ->  x_a = -k (normal +e_a) or k (-e_a)
            if (!(fabs(wall - m->bbox[(sgn ? 3 : 0) + a]) <= 1e-9 * (1.0 + fabs(wall)))) { ok = false; break; }
            if (members[pl].size() != 2) { ok = false; break; }
            int fct0 = -1, face0 = 0x7fffffff;
            double area = 0.0;
            for (int f : members[pl]) {
                if (fct0 < 0) fct0 = m->face_facet[f]; else if (m->face_facet[f] != fct0) ok = false;
                face0 = std::min(face0, f);
                area += m->face_area[f];
                const double *V = m->vertices + 9 * (size_t)f;
                for (int c = 0; c < 3 && ok; ++c)
                    for (int k = 0; k < 3; ++k) {
                        const double v = V[3 * c + k], lo = m->bbox[k], hi = m->bbox[3 + k];
                        const double e = 1e-9 * (1.0 + fabs(lo) + fabs(hi));
                        if (k == a) { if (fabs(v - wall) > e) ok = false; }
                        else if (fabs(v - lo) > e && fabs(v - hi) > e) ok = false;      // a corner of the side
                    }
            }
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            const double side = (m->bbox[3 + b] - m->bbox[b]) * (m->bbox[3 + c] - m->bbox[c]);
            if (!(fabs(area - side) <= 1e-9 * side) || fct0 < 0 || fct0 >= m->Fc) ok = false;
            if (!ok) break;
            d.box_k[w] = pn[3];
            box_facet[w] = fct0;
            d.box_ids = (d.box_ids & ~(0xFFull << (8 * w))) | ((uint64_t)(fct0 & 15) << (8 * w)) | ((uint64_t)(face0 & 15) << (8 * w + 4));
        }
        if (ok && seen == 63) {
            // one facet per wall
            int fm = 0;
            for (int w = 0; w < 6; ++w) fm |= 1 << box_facet[w];
            ctx->mesh_box = fm == 63;
        }
    }
    ctx->have_mesh = true;
    return NK_OK;
}

// The box store is used when the mesh allows it, the tables sit in LDS, and nothing in this context spoke against it
// (NK_NO_BOX=1: developer switch / tests of the cached layout on boxes).
static inline bool nk_want_box(const nk_ctx *ctx) {
    return ctx->have_mesh && ctx->mesh_box && !ctx->box_forbidden && !getenv("NK_NO_BOX") && !getenv("NK_SPLIT") &&
           ctx->d.F <= NK_LDS_FACES && ctx->d.Fc <= NK_LDS_FACES;
}

static int nk_patch_facets(nk_ctx *ctx) {
    NK_HIP(hipMemcpy((void *)ctx->d.facets, ctx->host_facets.data(), (size_t)ctx->d.Fc * sizeof(NkFacet), hipMemcpyHostToDevice));
    return NK_OK;
}

// The reservoir counters live in the segments' order (rc_p) while a store exists; before the segmentation changes (or
// the reservoirs are replaced) they go back to the caller's order.
static int nk_entry_tables_drop(nk_ctx *ctx, bool keep_counters) {
    NkDev &d = ctx->d;
    if (ctx->rm_nseg > 0 && keep_counters && d.R > 0 && d.res_counter) {
        const int64_t n = (int64_t)d.R * d.M;
        k_perm_rm<<<(int)((n + 255) / 256), 256, 0, ctx->stream>>>(0, d.R, d.M, ctx->rm_nseg, ctx->rm_nlmax,
                                                                   d.m2s, d.res_counter, ctx->rc_p + (ctx->step & 1) * d.rc_len);      // (the map the tables were built with; the copy the next step reads)
        NK_HIP(hipGetLastError());
        NK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (ctx->ep_p) { hipFree(ctx->ep_p); ctx->ep_p = nullptr; }
    if (ctx->rc_p) { hipFree(ctx->rc_p); ctx->rc_p = nullptr; }
    d.ep_p = nullptr; d.rc_p = nullptr;
    ctx->rm_nseg = 0;
    return NK_OK;
}
static int nk_entry_tables_build(nk_ctx *ctx) {
    NkDev &d = ctx->d;
    if (!(d.R > 0 && d.nseg > 0 && d.m2s && d.enter_prob && d.res_counter) || ctx->rm_nseg == d.nseg) return NK_OK;
    int rc = nk_entry_tables_drop(ctx, true);
    if (rc) return rc;
    const size_t len = (size_t)d.nseg * d.R * d.nlmax;
    NK_HIP(hipMalloc((void **)&ctx->ep_p, len * 8));
    NK_HIP(hipMalloc((void **)&ctx->rc_p, 2 * len * 8));
    NK_HIP(hipMemsetAsync(ctx->ep_p, 0, len * 8, ctx->stream));
    NK_HIP(hipMemsetAsync(ctx->rc_p, 0, 2 * len * 8, ctx->stream));
    d.rc_len = (int64_t)len;
    const int64_t n = (int64_t)d.R * d.M;
    k_perm_rm<<<(int)((n + 255) / 256), 256, 0, ctx->stream>>>(1, d.R, d.M, d.nseg, d.nlmax, d.m2s, (double *)d.enter_prob, ctx->ep_p);
    k_perm_rm<<<(int)((n + 255) / 256), 256, 0, ctx->stream>>>(1, d.R, d.M, d.nseg, d.nlmax, d.m2s, d.res_counter, ctx->rc_p + (ctx->step & 1) * d.rc_len);
    NK_HIP(hipGetLastError());
    d.ep_p = ctx->ep_p; d.rc_p = ctx->rc_p;
    ctx->rm_nseg = d.nseg;
    ctx->rm_nlmax = d.nlmax;
    return NK_OK;
}

static int nk_alloc_tally(nk_ctx *ctx) {
    NkDev &d = ctx->d;
    d.NB = 5 * d.S + 5 * d.R + 1;
    if (ctx->acc) { hipFree(ctx->acc); ctx->acc = nullptr; }
    if (ctx->hist) { hipHostFree(ctx->hist); ctx->hist = nullptr; }      // the history rows follow NB
    ctx->hist_cap = 0;
    NK_HIP(hipMalloc((void **)&ctx->acc, (size_t)(d.NB + 2) * sizeof(double)));
    NK_HIP(hipMemset(ctx->acc, 0, (size_t)(d.NB + 2) * sizeof(double)));
    const double *p;
    NK_UP((const double *)nullptr, (size_t)(ctx->num_cu * 16) * d.NB, &p);     // >= the sweep's and k_events' persistent grids
    d.partials = (double *)p;
    return NK_OK;
}

// Append [w; p] = inv[:, :S] @ T_sv to a host copy of the temperatures (what k_update does on the device).
static void nk_rbf_coefficients(nk_ctx *ctx, std::vector<double> &T) {
    const int S = ctx->d.S, P = ctx->d.rbf_P;
    T.resize((size_t)S + P);
    for (int j = 0; j < P; ++j) {
        double a = 0.0;
        for (int i = 0; i < S; ++i) a += ctx->h_rbf_inv[(size_t)j * P + i] * T[i];
        T[(size_t)S + j] = a;
    }
}

int nk_set_subvolumes(nk_ctx *ctx, const nk_subvols *s, const double *T_sv_init) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && s && T_sv_init, "nk_set_subvolumes: NULL argument");
    NK_ARG(s->S > 0 && s->S <= 512, "nk_set_subvolumes: S must be in [1, 512]");
    NK_ARG(ctx->have_material, "nk_set_subvolumes: call nk_set_material first");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    d.S = s->S; d.sv_kind = s->kind; d.sv_axis = s->axis; d.sv_interp = s->interp;
    NK_ARG(s->axis >= 0 && s->axis < 3, "nk_set_subvolumes: axis");
    NK_ARG(!(s->kind != 0 && s->interp != 2 && s->interp != 3), "nk_set_subvolumes: slice interpolation needs slice subvolumes");
    NK_ARG(s->interp >= 0 && s->interp <= 3, "nk_set_subvolumes: interp must be 0..3");
    NK_UP(s->centers, (size_t)s->S * 3, &d.centers);
    NK_UP(s->volumes, (size_t)s->S, &d.sv_volume);
    d.rbf_P = 0;
    std::vector<double> t0(T_sv_init, T_sv_init + s->S);
    if (s->interp == 3) {
        NK_ARG(s->rbf_inv && s->rbf_shift && s->rbf_scale, "nk_set_subvolumes: interp 3 needs the RBF tables");
        const int nd = (s->rbf_used[0] != 0) + (s->rbf_used[1] != 0) + (s->rbf_used[2] != 0);
        NK_ARG(nd >= 1, "nk_set_subvolumes: RBF interpolation over no coordinate");
        d.rbf_P = s->S + nd + 1;
        for (int k = 0; k < 3; ++k) {
            d.rbf_used[k] = s->rbf_used[k] != 0; d.rbf_shift[k] = s->rbf_shift[k]; d.rbf_scale[k] = s->rbf_scale[k];
            NK_ARG(!d.rbf_used[k] || d.rbf_scale[k] != 0.0, "nk_set_subvolumes: zero RBF scale");
        }
        NK_UP(s->rbf_inv, (size_t)d.rbf_P * d.rbf_P, &d.rbf_inv);
        ctx->h_rbf_inv.assign(s->rbf_inv, s->rbf_inv + (size_t)d.rbf_P * d.rbf_P);
        nk_rbf_coefficients(ctx, t0);
    }
    const double *t;
    NK_UP(t0.data(), t0.size(), &t);
    d.T_sv = (double *)t;
    if (s->kind == 0 && s->S > 1) {
        double c0 = s->centers[s->axis], c1 = s->centers[3 + s->axis];
        NK_ARG(c1 > c0, "nk_set_subvolumes: slice centres must ascend along the axis");
        double Lx = c1 - c0;
        d.sv_lo = c0 - 0.5 * Lx; d.sv_invL = 1.0 / Lx;
    } else { d.sv_lo = 0.0; d.sv_invL = 0.0; }
    ctx->have_sv = true;
    nk_track_T(ctx, T_sv_init, s->S);
    int rc = nk_update_tau_window(ctx, false);
    if (rc) return rc;
    return nk_alloc_tally(ctx);
}

int nk_set_reservoirs(nk_ctx *ctx, const nk_reservoirs *r) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && r, "nk_set_reservoirs: NULL argument");
    NK_ARG(ctx->have_material && ctx->have_mesh && ctx->have_sv, "nk_set_reservoirs: set material, mesh, subvolumes first");
    NK_ARG(r->R >= 0 && r->R <= 64, "nk_set_reservoirs: R must be in [0, 64]");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    NK_TRY(nk_entry_tables_drop(ctx, false));
    d.R = r->R; d.res_gen = r->gen;
    d.res_nf = 0; d.res_lds = 0;
    NK_ARG((int64_t)d.R * d.M < (1ll << 28), "nk_set_reservoirs: R*Q*J too large for the particle id layout");
    if (r->R > 0) {
        NK_UP(r->facet, (size_t)r->R, &d.res_facet);
        NK_UP(r->T, (size_t)r->R, &d.res_T);
        ctx->res_T_max = *std::max_element(r->T, r->T + r->R);
        NK_UP(r->enter_prob, (size_t)r->R * d.M, &d.enter_prob);
        const double *c;
        NK_UP(r->counter, (size_t)r->R * d.M, &c);
        d.res_counter = (double *)c;
        double pmax = 0.0;
        for (size_t i = 0; i < (size_t)r->R * d.M; ++i) pmax = std::max(pmax, r->enter_prob[i]);
        ctx->h_enter_prob.assign(r->enter_prob, r->enter_prob + (size_t)r->R * d.M);
        ctx->o2o_first = 0;
        NK_ARG(r->gen >= 0 && r->gen <= 2, "nk_set_reservoirs: gen must be 0 (constant), 1 (fixed_rate) or 2 (one_to_one)");
        if (r->gen == 2) {
            // one_to_one: cumulative enter_prob per reservoir (np.cumsum, then / max: Population.py:467-468) and the
            // first step's emission; the list must hold whatever leaves in one step
            NK_ARG(r->n_leaving, "nk_set_reservoirs: one_to_one needs n_leaving");
            std::vector<double> roul((size_t)r->R * d.M);
            std::vector<int32_t> nl((size_t)r->R);
            int64_t first = 0;
            for (int i = 0; i < r->R; ++i) {
                double run = 0.0, mx = 0.0;
                for (int m = 0; m < d.M; ++m) { run += r->enter_prob[(size_t)i * d.M + m]; roul[(size_t)i * d.M + m] = run; mx = std::max(mx, run); }
                NK_ARG(mx > 0.0, "nk_set_reservoirs: one_to_one reservoir with zero entry probability");
                for (int m = 0; m < d.M; ++m) roul[(size_t)i * d.M + m] /= mx;
                NK_ARG(r->n_leaving[i] >= 0 && r->n_leaving[i] < (1ll << 24), "nk_set_reservoirs: n_leaving out of range");
                nl[(size_t)i] = (int32_t)r->n_leaving[i];
                first += r->n_leaving[i];
            }
            NK_UP(roul.data(), roul.size(), &d.res_roulette);
            const int32_t *pn;
            NK_UP(nl.data(), nl.size(), &pn);
            d.nleave_prev = (int32_t *)pn;
            ctx->o2o_first = first;
        }
        NK_ARG(pmax < 4094.0, "nk_set_reservoirs: more than 4094 particles of one mode per step (id layout)");
        for (int i = 0; i < r->R; ++i) {
            NK_ARG(r->facet[i] >= 0 && r->facet[i] < d.Fc, "nk_set_reservoirs: facet index");
            ctx->host_facets[r->facet[i]].res = i;
        }
        // sampling tables of the reservoir facets, gathered per reservoir (faces in Mesh.sample_surface order)
        std::vector<int32_t> off((size_t)r->R + 1, 0);
        std::vector<double> rcdf, rverts;
        for (int i = 0; i < r->R; ++i) {
            const int f0 = ctx->h_ffo[r->facet[i]], f1 = ctx->h_ffo[r->facet[i] + 1];
            NK_ARG(f1 > f0, "nk_set_reservoirs: reservoir facet without faces");
            for (int a = f0; a < f1; ++a) {
                rcdf.push_back(ctx->h_fcdf[a]);
                const double *v = &ctx->h_verts[(size_t)ctx->h_ffi[a] * 9];
                rverts.insert(rverts.end(), v, v + 9);
            }
            off[(size_t)i + 1] = (int32_t)rcdf.size();
        }
        NK_UP(off.data(), off.size(), &d.res_face_off);
        NK_UP(rcdf.data(), rcdf.size(), &d.res_face_cdf);
        NK_UP(rverts.data(), rverts.size(), &d.res_face_verts);
        d.res_nf = (int32_t)rcdf.size();
        d.res_lds = d.res_nf <= NK_LDS_RESFACES ? 1 : 0;
        int rc = nk_patch_facets(ctx);
        if (rc) return rc;
        if ((rc = nk_entry_tables_build(ctx))) return rc;
    }
    return nk_alloc_tally(ctx);
}

int nk_set_rough(nk_ctx *ctx, const nk_rough *r) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && r, "nk_set_rough: NULL argument");
    NK_ARG(ctx->have_material && ctx->have_mesh, "nk_set_rough: set material and mesh first");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    d.Fr = r->Fr;
    ctx->g_sweep = 0;
    if (r->Fr > 0) {
        size_t n = (size_t)r->Fr * d.M;
        NK_UP(r->specularity, n, &d.specularity);
        NK_UP(r->true_spec, n, &d.true_spec);
        NK_UP(r->spec_map, n, &d.spec_map);
        NK_UP(r->roulette, n, &d.roulette);
        {   // bucket index of the roulette search (nk_reflect): first position with roulette >= k / nlut * last
            int nlut = 1024;
            while (nlut < 65536 && (int64_t)nlut * 4 < d.M) nlut *= 2;
            d.roul_nlut = nlut;
            std::vector<int32_t> lut((size_t)r->Fr * (nlut + 1));
            for (int f = 0; f < r->Fr; ++f) {
                const double *ro = r->roulette + (size_t)f * d.M;
                const double last = ro[d.M - 1];
                int pos = 0;                                     // thresholds ascend: one merge pass per facet
                for (int k = 0; k < nlut; ++k) {
                    const double thr = ((double)k / (double)nlut) * last;
                    while (pos < d.M && ro[pos] < thr) ++pos;
                    lut[(size_t)f * (nlut + 1) + k] = pos;
                }
                lut[(size_t)f * (nlut + 1) + nlut] = d.M;        // everything is below the end of the last bucket
            }
            NK_UP(lut.data(), lut.size(), &d.roul_lut);
        }
        if (r->degen_j2) NK_UP(r->degen_j2, (size_t)d.M, &d.degen_j2); else d.degen_j2 = nullptr;
        for (int i = 0; i < r->Fr; ++i) {
            NK_ARG(r->facet[i] >= 0 && r->facet[i] < d.Fc, "nk_set_rough: facet index");
            ctx->host_facets[r->facet[i]].rough = i;
        }
        return nk_patch_facets(ctx);
    }
    return NK_OK;
}

int nk_set_params(nk_ctx *ctx, const nk_params *p) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && p, "nk_set_params: NULL argument");
    NK_ARG(p->dt > 0, "nk_set_params: dt must be positive");
    ctx->params = *p;
    NkDev &d = ctx->d;
    d.dt = p->dt; d.inv_dt = 1.0 / p->dt; d.norm_fixed = p->norm_fixed; d.particle_density = p->particle_density;
    d.T_ref_local = p->T_ref_local; d.T_ref = p->T_ref;
    ctx->have_params = true;
    return NK_OK;
}

// Host copy of the live particles, segment by segment (used by download and by re-layouts).
struct NkHostParticles {
    std::vector<double> x, y, z, occ, nts;
    std::vector<int32_t> mode, facet;
    std::vector<uint64_t> pid;
};
// Every kernel but the sweep and the emission expects a segment's particles from slot 0 of its range (NkDev::seg_lo): move them
// down after alternating sweeps, before anything else reads the store.  Needed once per download, regrow, contains_check step
// (every 100th) or flush of the deferred relaxation; the kernel moves only what is not there already.
static int nk_normalize(nk_ctx *ctx, int honor_halt = 0) {
    NkDev &d = ctx->d;
    d.down = 0;
    if (!ctx->walked || !d.seg_lo) return NK_OK;
    k_anchor<<<ctx->num_cu * 8, NK_WG, 0, ctx->stream>>>(d, honor_halt);
    NK_HIP(hipGetLastError());
    if (!honor_halt) ctx->walked = false;             // (inside a batch the launch may have been skipped by a halt: stay cautious)
    return NK_OK;
}
static int nk_gather_live(nk_ctx *ctx, NkHostParticles &h, bool want_all) {
    NkDev &d = ctx->d;
    if (d.cap == 0) return NK_OK;
    NK_TRY(nk_normalize(ctx));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> cnt((size_t)d.nseg);
    NK_HIP(hipMemcpy(cnt.data(), d.seg_count, (size_t)d.nseg * 4, hipMemcpyDeviceToHost));
    int64_t live = 0;
    for (int c : cnt) live += c;
    if (!want_all) { h.x.resize((size_t)live); return NK_OK; }
    std::vector<double> bd;
    std::vector<uint32_t> bw;
    std::vector<uint64_t> bu;
    // a field comes back whole (slot order), then the live head of every segment is kept
    auto keep = [&](const auto &all, auto *dst) {
        for (int sgm = 0; sgm < d.nseg; ++sgm) {
            memcpy(dst, all.data() + (size_t)sgm * d.segcap, (size_t)cnt[sgm] * sizeof(*dst));
            dst += cnt[sgm];
        }
    };
    h.x.resize(live); h.y.resize(live); h.z.resize(live); h.occ.resize(live); h.nts.resize(live);
    h.mode.resize(live); h.facet.resize(live); h.pid.assign(live, 0);
    std::vector<uint32_t> w0((size_t)live);
    int rc;
    if ((rc = nk_field_download(ctx, d, d.x, bd))) return rc; keep(bd, h.x.data());
    if ((rc = nk_field_download(ctx, d, d.y, bd))) return rc; keep(bd, h.y.data());
    if ((rc = nk_field_download(ctx, d, d.z, bd))) return rc; keep(bd, h.z.data());
    if ((rc = nk_field_download(ctx, d, d.occ, bd))) return rc; keep(bd, h.occ.data());
    std::vector<int32_t> bfc;
    if (d.nts) { if ((rc = nk_field_download(ctx, d, d.nts, bd))) return rc; keep(bd, h.nts.data()); }
    else {
        // box store: the next hit is not kept -- cast it where the particles stand (k_next_hit; needs the tables)
        if (ctx->have_material && ctx->have_mesh && ctx->have_sv && d.modetab) {
            double *dn = nullptr; int32_t *df = nullptr;
            NK_HIP(hipMalloc((void **)&dn, (size_t)d.cap * 8));
            if (hipMalloc((void **)&df, (size_t)d.cap * 4) != hipSuccess) { hipFree(dn); ctx->err = "nk_gather_live: out of memory"; return NK_ERR_HIP; }
            hipMemsetAsync(dn, 0, (size_t)d.cap * 8, ctx->stream); hipMemsetAsync(df, 0xff, (size_t)d.cap * 4, ctx->stream);
            k_next_hit<1><<<nk_sweep_grid(ctx), NK_WG, nk_lds(ctx, true), ctx->stream>>>(d, dn, df);
            bd.resize((size_t)d.cap); bfc.resize((size_t)d.cap);
            hipError_t e1 = hipGetLastError();
            if (e1 == hipSuccess) e1 = hipMemcpy(bd.data(), dn, (size_t)d.cap * 8, hipMemcpyDeviceToHost);
            if (e1 == hipSuccess) e1 = hipMemcpy(bfc.data(), df, (size_t)d.cap * 4, hipMemcpyDeviceToHost);
            hipFree(dn); hipFree(df);
            if (e1 != hipSuccess) { ctx->err = std::string("nk_gather_live: ") + hipGetErrorString(e1); return NK_ERR_HIP; }
            keep(bd, h.nts.data());
        } else { std::fill(h.nts.begin(), h.nts.end(), 0.0); }
    }
    if ((rc = nk_field_download(ctx, d, d.w0, bw))) return rc; keep(bw, w0.data());
    if (d.pid) { if ((rc = nk_field_download(ctx, d, d.pid, bu))) return rc; keep(bu, h.pid.data()); }
    // packed word -> (mode, facet): mode = idx * nseg + segment when the modes are partitioned
    const uint32_t lbmask = (1u << d.lb) - 1u;
    int64_t k = 0;
    for (int sgm = 0; sgm < d.nseg; ++sgm)
        for (int j = 0; j < cnt[sgm]; ++j, ++k) {
            const uint32_t idx = w0[(size_t)k] & lbmask;
            h.mode[(size_t)k] = d.part ? ctx->h_s2m[(size_t)sgm * d.nlmax + idx] : (int32_t)idx;
            if (d.nts) h.facet[(size_t)k] = (int32_t)(w0[(size_t)k] >> d.lb) - 1;
            else h.facet[(size_t)k] = (w0[(size_t)k] & NK_LOST) ? -1 : (bfc.empty() ? 0 : bfc[(size_t)sgm * d.segcap + j]);
        }
    return NK_OK;
}

// Lay N particles out over the segments.  Partitioned modes: every particle goes to the segment that owns its mode.
// Global mode indices (rough facets): equal shares, sorted by mode (stable), so that a tile shares a few mode records.
static int nk_scatter(nk_ctx *ctx, int64_t N, const double *x, const double *y, const double *z, const int32_t *mode,
                      const double *occ, const double *n_ts, const int32_t *facet, const uint64_t *pid, uint64_t pid_offset) {
    if (ctx) ctx->emitted_for = -1;
    NkDev &d = ctx->d;
    const int M = d.M;
    for (int64_t i = 0; i < N; ++i) NK_ARG(mode[i] >= 0 && mode[i] < M, "nk_upload_particles: mode index out of range");
    std::vector<int64_t> order((size_t)N);
    std::vector<int64_t> start((size_t)d.nseg + 1, 0);
    if (d.part) {
        const std::vector<int32_t> &m2s = ctx->h_m2s;
        for (int64_t i = 0; i < N; ++i) start[(size_t)(m2s[(size_t)mode[i]] % d.nseg) + 1] += 1;
        for (int sgm = 0; sgm < d.nseg; ++sgm) start[(size_t)sgm + 1] += start[(size_t)sgm];
        // inside a segment: by local mode index (stable), so that a tile shares a few records
        std::vector<int64_t> key((size_t)N);
        for (int64_t i = 0; i < N; ++i) { order[(size_t)i] = i; key[(size_t)i] = (int64_t)(m2s[(size_t)mode[i]] % d.nseg) * ((int64_t)d.nlmax + 1) + m2s[(size_t)mode[i]] / d.nseg; }
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return key[(size_t)a] < key[(size_t)b]; });
    } else {
        std::vector<int64_t> mstart((size_t)M + 1, 0);               // counting sort by mode
        for (int64_t i = 0; i < N; ++i) mstart[(size_t)mode[i] + 1] += 1;
        for (int m = 0; m < M; ++m) mstart[(size_t)m + 1] += mstart[(size_t)m];
        std::vector<int64_t> cur(mstart.begin(), mstart.end() - 1);
        for (int64_t i = 0; i < N; ++i) order[(size_t)cur[(size_t)mode[i]]++] = i;
        for (int sgm = 0; sgm <= d.nseg; ++sgm) start[(size_t)sgm] = (N * sgm) / d.nseg;
    }
    std::vector<int32_t> cnt((size_t)d.nseg);
    for (int sgm = 0; sgm < d.nseg; ++sgm) {
        cnt[(size_t)sgm] = (int32_t)(start[(size_t)sgm + 1] - start[(size_t)sgm]);
        NK_ARG(cnt[(size_t)sgm] <= d.segcap, "nk_upload_particles: segment capacity too small");
    }
    // a field is laid out whole on the host (slot order: every segment's particles from its start), then uploaded
    auto put = [&](const auto *src, const auto &field) -> int {
        typedef typename std::remove_const<typename std::remove_pointer<decltype(src)>::type>::type T;
        std::vector<T> all((size_t)d.cap, T(0));
        for (int sgm = 0; sgm < d.nseg; ++sgm) {
            const int64_t lo = start[(size_t)sgm], n = cnt[(size_t)sgm];
            T *o = all.data() + (size_t)sgm * d.segcap;
            for (int64_t k = 0; k < n; ++k) o[k] = src[order[(size_t)(lo + k)]];
        }
        return nk_field_upload(ctx, d, field, all.data());
    };
    int rc;
    if ((rc = put(x, d.x)) || (rc = put(y, d.y)) || (rc = put(z, d.z)) || (rc = put(occ, d.occ))) return rc;
    if (n_ts && d.nts && (rc = put(n_ts, d.nts))) return rc;
    {
        std::vector<uint32_t> w0((size_t)N);
        for (int64_t i = 0; i < N; ++i) {
            const int32_t fc = facet ? facet[i] : -1;
            NK_ARG(fc >= -1 && fc < d.Fc, "nk_upload_particles: facet index out of range");
            const uint32_t idx = d.part ? (uint32_t)(ctx->h_m2s[(size_t)mode[i]] / d.nseg) : (uint32_t)mode[i];
            // (box store: the facet is not kept, only whether the last cast missed)
            w0[(size_t)i] = d.nts ? (((uint32_t)(fc + 1) << d.lb) | idx) : (((facet && fc < 0) ? NK_LOST : 0u) | idx);
        }
        if ((rc = put((const uint32_t *)w0.data(), d.w0))) return rc;
    }
    if (d.pid) {
        if (pid) { if ((rc = put(pid, d.pid))) return rc; }
        else {
            std::vector<uint64_t> ids((size_t)N);
            for (int64_t i = 0; i < N; ++i) ids[(size_t)i] = pid_offset + (uint64_t)i;
            if ((rc = put((const uint64_t *)ids.data(), d.pid))) return rc;
        }
    }
    NK_HIP(hipMemcpy(d.seg_count, cnt.data(), (size_t)d.nseg * 4, hipMemcpyHostToDevice));
    if (d.seg_lo) NK_HIP(hipMemset(d.seg_lo, 0, (size_t)d.nseg * 4));      // (the particles were dealt from slot 0 of their segments)
    ctx->walked = false;
    return NK_OK;
}

// Does this configuration draw random numbers per particle (then ids are tracked)?  Are the modes partitioned over the
// segments (always, but for a developer probe; with rough facets a particle whose mode changed migrates, k_deliver)?
static inline bool nk_want_pid(const nk_ctx *ctx) { return ctx->d.Fr > 0 || ctx->params.track_ids != 0; }
// Split sweep (events through per-segment queues and k_events): large meshes, whose events are tree walks.  NK_SPLIT=0/1 forces.
static inline bool nk_want_split(const nk_ctx *ctx) {
    if (const char *e = getenv("NK_SPLIT")) return atoi(e) != 0;
    return ctx->have_mesh && !(ctx->d.F <= NK_LDS_FACES && ctx->d.Fc <= NK_LDS_FACES);
}
static inline bool nk_want_part(const nk_ctx *ctx) { return !getenv("NK_NO_PARTITION"); }   // env: developer probe

// The instantiation this context runs (nk_kind.h), derived here and nowhere else.  Ids and the split sweep are read from the store
// as it is laid out (stored: d.pid, d.qx) or from what the configuration asks for (nk_want_pid, nk_want_split): nk_sweep_blocks
// runs inside nk_alloc_particles, before the store exists, and asks for the wanted ones; the steps launch on the store they have.
// nk_check_ready re-deals a store whose layout_key (written by nk_alloc_particles from d.pid and d.qx) differs from the wanted
// one, so after it the two readings agree.  The box store has one source: nk_alloc_particles sets d.box = nk_want_box before it
// sizes the grid, and layout_key covers it too.
static NkSweepKind nk_sweep_kind(const nk_ctx *ctx, bool stored) {
    const NkDev &d = ctx->d;
    return nk_kind_normalise({nk_geom_mode(ctx), d.Fr > 0, d.sv_interp == 3, stored ? (bool)d.pid : nk_want_pid(ctx),
                              stored ? d.qx != nullptr : nk_want_split(ctx), nk_want_lrec(ctx), nk_sweep_fast(ctx), d.box != 0});
}
// One picker per kernel family: the instantiation of a (normalised) kind as a pointer, nullptr for a combination that does not
// exist (`if constexpr`: it is never named, so never instantiated).  The FAST sweeps are instantiated in nk_sweep_plain.hip.
typedef void (*NkSweepFn)(NkDev, uint32_t, int, int);
typedef void (*NkResidentFn)(NkDev, uint32_t, int, int, int, double *, int, unsigned int *);
static NkSweepFn nk_sweep_kernel(const NkSweepKind &k) {
    auto fast = [](auto L, auto F1, auto X) -> NkSweepFn { return k_sweep<1, false, false, false, false, L.value, F1.value ? 1 : 2, X.value>; };
    if (k.fast) return nk_lift(fast, k.lrec, k.fast == 1, k.box);
    return nk_lift([](auto G1, auto R, auto B, auto P, auto S, auto L, auto X) -> NkSweepFn {
        if constexpr ((R.value && !P.value) || (X.value && (!G1.value || S.value))) return nullptr;
        else return k_sweep<G1.value ? 1 : 2, R.value, B.value, P.value, S.value, L.value, 0, X.value>;
    }, k.geom == 1, k.rough, k.rbf, k.pid, k.split, k.lrec, k.box);
}
static NkSweepFn nk_events_kernel(const NkSweepKind &k) {
    return nk_lift([](auto G1, auto R, auto B, auto P) -> NkSweepFn {
        if constexpr (R.value && !P.value) return nullptr;
        else return k_events<G1.value ? 1 : 2, R.value, B.value, P.value>;
    }, k.geom == 1, k.rough, k.rbf, k.pid);
}
static NkResidentFn nk_resident_kernel(const NkSweepKind &k) {
    return nk_lift([](auto X, auto P, auto L) -> NkResidentFn { return k_resident<X.value, P.value, L.value>; }, k.box, k.pid, k.lrec);
}

// Persistent grid of the sweep = what the device keeps resident of the instantiation this configuration uses (before the
// tables are known: four workgroups per CU, the common case).
static int nk_sweep_blocks(nk_ctx *ctx) {
    if (!(ctx->have_material && ctx->have_mesh && ctx->have_sv)) return ctx->num_cu * NK_SWEEP_OCC;
    const NkSweepKind kind = nk_sweep_kind(ctx, false);
    const size_t lds_w = nk_lds(ctx, true, kind.pid ? 3 : 2);
    if (ctx->g_sweep == 0 || !(ctx->g_sweep_kind == kind) || ctx->g_sweep_lds != lds_w) {
        int per_cu = 0;
        const NkSweepFn sweep = nk_sweep_kernel(kind);          // (nullptr: one workgroup per CU here, the step reports it)
        hipError_t e_ = sweep ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sweep, NK_WG, lds_w) : hipErrorInvalidDeviceFunction;
        if (e_ != hipSuccess || per_cu < 1) per_cu = 1;
        if (per_cu > 8) per_cu = 8;
        { const int bound = NK_SWEEP_BOUND(kind.geom, kind.rough, kind.rbf, kind.split); if (per_cu > bound) per_cu = bound; }   // what it was compiled for
        if (const char *e = getenv("NK_SWEEP_PER_CU")) { int v = atoi(e); if (v >= 1 && v < per_cu) per_cu = v; }   // developer probe
        ctx->g_sweep = ctx->num_cu * per_cu;
        ctx->g_sweep_kind = kind;
        ctx->g_sweep_lds = lds_w;
        if (getenv("NK_VERBOSE")) fprintf(stderr, "[nanokappa_hip] sweep: %d workgroups per CU (occupancy query rc %d), %zu B LDS each\n", per_cu, (int)e_, lds_w);
    }
    return ctx->g_sweep;
}

// The segment that owns mode m (host copy of the mode map; before a map exists for this segmentation: the plain deal).
static inline int nk_mode_seg(const nk_ctx *ctx, int m, int nseg) {
    return (ctx->map_nseg == nseg && !ctx->h_m2s.empty()) ? ctx->h_m2s[(size_t)m] % nseg : m % nseg;
}

// Deal the modes over the segments (NkDev::m2s / s2m / seg_nl, nk_device.h).  A mode's work per step = its particles (every
// active mode holds the same number) + its boundary events, sum_a |v_a| dt / extent_a of the mesh's bounding box per particle,
// an event weighing NK_EVENT_WEIGHT (0.45: from the stamps' cycles per tile) of a mean particle-step.  In the order of their
// event rate every mode goes to the segment that is furthest behind its SHARE of the work (longest-processing-time greedy).
// The shares follow the dispatch order: the SIMD issues the oldest wave first, so the k-th workgroup a CU received runs ahead
// of the (k+1)-th; share = 1 + NK_AGE_SKEW (0.14; 0.20 until the box sweep lost its general ray cast, profiles/r04_notes.txt (21)) x (1 - 2 k / (per_cu - 1)) -- speed only: if workgroups were dispatched in
// another order the sweep would merely be as uneven as with equal shares.  Modes that cannot move (never populated) fill up
// the shortest segments.  d.nlmax is the capacity of a segment's slot range (set by the caller).
static int nk_build_mode_map(nk_ctx *ctx) {
    NkDev &d = ctx->d;
    if (ctx->m2s_dev) { hipFree(ctx->m2s_dev); ctx->m2s_dev = nullptr; }
    if (ctx->s2m_dev) { hipFree(ctx->s2m_dev); ctx->s2m_dev = nullptr; }
    if (ctx->nl_dev) { hipFree(ctx->nl_dev); ctx->nl_dev = nullptr; }
    d.m2s = nullptr; d.s2m = nullptr; d.seg_nl = nullptr;
    ctx->h_m2s.clear(); ctx->h_s2m.clear(); ctx->map_nseg = 0;
    ctx->map_gen += 1;
    if (d.M <= 0 || d.nseg <= 0) return NK_OK;
    const int M = d.M, nseg = d.nseg, nlmax = d.nlmax;
    const bool plain = !d.part;          // developer probe without the partition: the modes' emission is dealt m % nseg, forwards
    std::vector<int32_t> nl((size_t)nseg, 0);
    ctx->h_m2s.assign((size_t)M, 0);
    ctx->h_s2m.assign((size_t)nseg * nlmax, -1);
    auto place = [&](int m, int seg) {
        const int l = nl[(size_t)seg]++;
        ctx->h_m2s[(size_t)m] = l * nseg + seg;
        ctx->h_s2m[(size_t)seg * nlmax + l] = m;
    };
    if (plain) {
        for (int m = 0; m < M; ++m) place(m, m % nseg);
    } else {
        std::vector<double> rate((size_t)M, 0.0);
        std::vector<char> active((size_t)M, 1);
        const bool have_v = ctx->h_vg.size() == (size_t)M * 3;
        if (have_v) {
            double inv[3] = {0, 0, 0};
            if (ctx->have_mesh) for (int a = 0; a < 3; ++a) { const double e = d.bbox[3 + a] - d.bbox[a]; inv[a] = e > 0.0 ? 1.0 / e : 0.0; }
            for (int m = 0; m < M; ++m) {
                const double *v = &ctx->h_vg[3 * (size_t)m];
                active[(size_t)m] = (v[0] != 0.0 || v[1] != 0.0 || v[2] != 0.0) ? 1 : 0;
                rate[(size_t)m] = fabs(v[0]) * inv[0] + fabs(v[1]) * inv[1] + fabs(v[2]) * inv[2];
            }
        }
        double rsum = 0.0; int64_t nact = 0;
        for (int m = 0; m < M; ++m) if (active[(size_t)m]) { rsum += rate[(size_t)m]; ++nact; }
        const double rmean = nact > 0 && rsum > 0.0 ? rsum / (double)nact : 1.0;
        const double beta = getenv("NK_EVENT_WEIGHT") ? atof(getenv("NK_EVENT_WEIGHT")) : 0.45;
        // shares by dispatch age: only when every resident wave of the sweep has exactly one segment
        std::vector<double> share((size_t)nseg, 1.0);
        const int g = ctx->g_sweep, per_cu = ctx->num_cu > 0 ? g / ctx->num_cu : 0;
        const double skew = getenv("NK_AGE_SKEW") ? atof(getenv("NK_AGE_SKEW")) : 0.14;
        if (per_cu > 1 && g == per_cu * ctx->num_cu && nseg == g * (NK_WG / 64) && skew != 0.0)
            for (int sg = 0; sg < nseg; ++sg) {
                const int k = (sg / (NK_WG / 64)) / ctx->num_cu;
                share[(size_t)sg] = 1.0 + skew * (1.0 - 2.0 * (double)k / (double)(per_cu - 1));
            }
        std::vector<int32_t> order((size_t)M);
        for (int m = 0; m < M; ++m) order[(size_t)m] = m;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
            if (active[(size_t)a] != active[(size_t)b]) return active[(size_t)a] > active[(size_t)b];
            return rate[(size_t)a] > rate[(size_t)b];
        });
        // least relative load first; ties to the lower segment index (deterministic)
        typedef std::pair<double, int> Key;
        std::priority_queue<Key, std::vector<Key>, std::greater<Key>> heap;
        std::vector<double> load((size_t)nseg, 0.0);
        for (int sg = 0; sg < nseg; ++sg) heap.push(Key(0.0, sg));
        int k = 0;
        for (; k < M && active[(size_t)order[(size_t)k]]; ++k) {
            const int m = order[(size_t)k];
            int sg = -1;
            while (!heap.empty()) { const Key top = heap.top(); heap.pop(); if (nl[(size_t)top.second] < nlmax) { sg = top.second; break; } }
            if (sg < 0) { ctx->err = "nk_build_mode_map: the segments' slot ranges are full (internal sizing error)"; return NK_ERR_ARG; }
            place(m, sg);
            load[(size_t)sg] += 1.0 + beta * rate[(size_t)m] / rmean;
            heap.push(Key(load[(size_t)sg] / share[(size_t)sg], sg));
        }
        // the modes that never hold a particle: wherever there is most room
        std::priority_queue<std::pair<int, int>, std::vector<std::pair<int, int>>, std::greater<std::pair<int, int>>> room;
        for (int sg = 0; sg < nseg; ++sg) room.push(std::make_pair((int)nl[(size_t)sg], sg));
        for (; k < M; ++k) {
            const std::pair<int, int> top = room.top(); room.pop();
            if (top.first >= nlmax) { ctx->err = "nk_build_mode_map: no room for the inactive modes (internal sizing error)"; return NK_ERR_ARG; }
            place(order[(size_t)k], top.second);
            room.push(std::make_pair(top.first + 1, top.second));
        }
    }
    NK_HIP(hipMalloc((void **)&ctx->m2s_dev, (size_t)M * 4));
    NK_HIP(hipMalloc((void **)&ctx->s2m_dev, (size_t)nseg * nlmax * 4));
    NK_HIP(hipMalloc((void **)&ctx->nl_dev, (size_t)nseg * 4));
    NK_HIP(hipMemcpy(ctx->m2s_dev, ctx->h_m2s.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->s2m_dev, ctx->h_s2m.data(), (size_t)nseg * nlmax * 4, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->nl_dev, nl.data(), (size_t)nseg * 4, hipMemcpyHostToDevice));
    d.m2s = ctx->m2s_dev; d.s2m = ctx->s2m_dev; d.seg_nl = ctx->nl_dev;
    ctx->map_nseg = nseg;
    return NK_OK;
}

// Particles that can enter one segment in one step, as the host sizes the store: the fullest segment's sum of floor(p) + 1 over its
// (reservoir, mode) entries, divided by the rank count ONCE (rounded up), plus R.  The sweep's halt criterion does not use this
// figure but the sum nk_emit_one leaves in seg_bound, which rounds up entry by entry -- a rank can own ceil(c / nranks) of an entry's
// c levels -- and so exceeds this one by less than one per entry, R (nl - 1) in all, from two ranks on.  That lowers the live count
// at which a segment asks for room by as much; a freshly uploaded store has a third of a segment and 107 slots more than that to
// spare (DESIGN.md (e) has the arithmetic, tests/test_shards_host.py the two sums, tests/test_gpu_shards.py the measurement).
static int64_t nk_spawn_bound(const nk_ctx *ctx, int nseg) {
    const NkDev &d = ctx->d;
    if (d.R <= 0) return 0;
    if (d.res_gen == 2) return 4 * (ctx->o2o_first / std::max(nseg, 1) + 64);
    std::vector<int64_t> per((size_t)nseg, 0);
    for (int r = 0; r < d.R; ++r)
        for (int m = 0; m < d.M; ++m) per[(size_t)(nk_mode_seg(ctx, m, nseg))] += (int64_t)floor(ctx->h_enter_prob[(size_t)r * d.M + m]) + 1;
    int64_t mx = 0;
    for (int64_t v : per) mx = std::max(mx, v);
    return (mx + d.nranks - 1) / d.nranks + d.R;
}

// Where the store's allocation lies in memory changes how fast everything that streams it runs -- the sweep and a plain copy
// alike: three levels, 4.97 / 5.2 / 5.65 TB/s for the in-place copy of a 44-byte store; of 200 successive 833 MB allocations on
// one box 119 were slow, 70 in between and 11 fast, scattered (profiles/r03_notes.txt (9), (17), (26)).  Round 3 searched: the
// store that is about to be used was timed with k_probe_place, then up to 95 further allocations of the same size, all held at
// once, and the fastest kept.  Round 4: the search is OPT-IN (NK_PLACE_TRIES=n > 1; default 1 = the store is timed once, for the
// record, and never moved).  Reasons: with the box store the sweep is bound by its instructions, not its memory -- 0.175-0.178 ms
// on the slowest level against 0.170-0.172 on the fastest (profiles/r04_notes.txt (6)) -- and a search that holds up to a third
// of the free memory, runs on every regrow and on eight ranks at once is no way to buy 3 %.  What the levels are NOT (r04
// notes (7), counters over the same copy on the slowest and the fastest of 40 allocations): not the TLB (UTCL1 misses: 0 on both),
// not the request count or size (identical), not DRAM credit stalls (equal); and with the launches serialised by the profiler
// the two buffers run equally fast -- the difference only exists between back-to-back launches.
// With a search: ends as soon as one candidate is 12 % faster than the slowest (relative: no absolute rate of a particular
// device), never more than a third of the free memory or a second; a probe that fails leaves the store where it is.
static int nk_place_store(nk_ctx *ctx) {
    NkDev &d = ctx->d;
    ctx->timing.place_tries = 0; ctx->timing.place_gbps = 0.0; ctx->timing.place_worst_gbps = 0.0;
    const int tries = getenv("NK_PLACE_TRIES") ? atoi(getenv("NK_PLACE_TRIES")) : 1;
    const size_t bytes = nk_store_bytes(d.cap, ctx->store_pid, ctx->store_nts);
    const int pbytes = nk_particle_bytes(ctx->store_pid, ctx->store_nts);
    // test hooks: NK_PLACE_MIN_MB (stores below it are not timed; default 64), NK_PLACE_FORCE=1 (always move into the last candidate)
    const size_t min_mb = getenv("NK_PLACE_MIN_MB") ? (size_t)atol(getenv("NK_PLACE_MIN_MB")) : 64;
    const bool force = getenv("NK_PLACE_FORCE") != nullptr;
    if (tries < 1 || !ctx->store_buf || ctx->store_pad != 0 || bytes < (min_mb << 20) || d.nseg <= 0 || d.segcap < 64) return NK_OK;
    size_t free_b = 0, total_b = 0;
    NK_HIP(hipMemGetInfo(&free_b, &total_b));
    const auto wall0 = std::chrono::steady_clock::now();
    const int g = std::max(1, std::min(nk_sweep_blocks(ctx), (d.nseg + NK_WG / 64 - 1) / (NK_WG / 64)));
    const int tiles = d.segcap / 64;
    hipEvent_t e0, e1;
    NK_HIP(hipEventCreate(&e0)); NK_HIP(hipEventCreate(&e1));
    auto probe = [&](void *buf, double &ms) -> int {
        NkDev t = d;
        nk_point_fields(t, (double *)buf, d.cap, ctx->store_pid, ctx->store_nts);
        k_probe_place<<<g, NK_WG, 0, ctx->stream>>>(t, tiles);           // untimed: page tables, caches
        NK_HIP(hipEventRecord(e0, ctx->stream));
        for (int k = 0; k < 3; ++k) k_probe_place<<<g, NK_WG, 0, ctx->stream>>>(t, tiles);
        NK_HIP(hipEventRecord(e1, ctx->stream));
        NK_HIP(hipGetLastError());
        NK_HIP(hipStreamSynchronize(ctx->stream));
        float f = 0.f;
        NK_HIP(hipEventElapsedTime(&f, e0, e1));
        ms = (double)f / 3.0;
        return NK_OK;
    };
    std::vector<void *> cand(1, ctx->store_buf);
    std::vector<double> ms(1, 0.0);
    int rc = probe(cand[0], ms[0]);
    while (!rc && (int)cand.size() < tries) {
        double lo = ms[0], hi = ms[0];
        for (double v : ms) { lo = std::min(lo, v); hi = std::max(hi, v); }
        if (hi > 1.12 * lo && !force) break;             // a candidate 12 % faster than the slowest has been seen
        if (bytes * cand.size() > free_b / 3) break;                     // the extra ones: never more than a third of what is free
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count() > 1000.0) break;   // ... nor more than a second (large stores: 0.1 s per allocation)
        void *buf = nullptr;
        if (hipMalloc(&buf, bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        cand.push_back(buf); ms.push_back(0.0);
        if (hipMemsetAsync(buf, 0, bytes, ctx->stream) != hipSuccess) { rc = NK_ERR_HIP; ctx->err = "nk_place_store: hipMemsetAsync failed"; break; }
        rc = probe(buf, ms.back());
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    size_t best = 0, worst = 0;
    for (size_t k = 1; k < cand.size(); ++k) { if (ms[k] < ms[best]) best = k; if (ms[k] > ms[worst]) worst = k; }
    if (force) best = cand.size() - 1;
    if (!rc && best != 0 && (ms[best] < 0.97 * ms[0] || force)) {        // move in
        if (hipMemcpyAsync(cand[best], cand[0], bytes, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = NK_ERR_HIP; ctx->err = "nk_place_store: copy into the chosen store failed"; }
        else {
            for (void *&p : ctx->pallocs) if (p == cand[0]) p = cand[best];
            ctx->store_buf = cand[best];
            nk_point_fields(d, (double *)cand[best], d.cap, ctx->store_pid, ctx->store_nts);
            std::swap(cand[0], cand[best]);                              // cand[0] stays, the rest goes
        }
    } else best = 0;
    for (size_t k = 1; k < cand.size(); ++k) hipFree(cand[k]);
    const double gb = 2.0 * (double)d.nseg * tiles * 64 * (pbytes - (ctx->store_pid ? 8 : 0)) / 1e9;      // read + written by one probe launch (it leaves the ids alone)
    ctx->timing.place_tries = (int64_t)cand.size();
    ctx->timing.place_gbps = ms[best] > 0.0 ? gb / (ms[best] * 1e-3) : 0.0;
    ctx->timing.place_worst_gbps = ms[worst] > 0.0 ? gb / (ms[worst] * 1e-3) : 0.0;
    if (rc) {                                            // a failed probe is no reason to fail an allocation or a regrow
        if (getenv("NK_VERBOSE")) fprintf(stderr, "[nanokappa_hip] store placement: probe failed (%s); the store stays where it is\n", ctx->err.c_str());
        (void)hipGetLastError();
        rc = NK_OK;
    }
    if (getenv("NK_VERBOSE")) {
        fprintf(stderr, "[nanokappa_hip] store placement: %zu allocation(s) of %.0f MB probed:", cand.size(), (double)bytes / 1048576.0);
        for (size_t k = 0; k < ms.size(); ++k) fprintf(stderr, " %.1f", ms[k] * 1e3);
        fprintf(stderr, " us per pass; kept number %zu (%.2f TB/s); %.1f ms\n", best, ctx->timing.place_gbps / 1e3,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count());
    }
    return rc;
}

// (Re)allocate the particle store for `capacity` particles, `max_seg` of them at most in one segment when the modes are
// partitioned (0 = unknown: even spread assumed).
// particles of the tiled rule (particle p has mode umodes[p % nu]) per unique mode, for p in [pid_lo, pid_lo + N)
static inline int64_t nk_tiled_count(int64_t u, int64_t nu, int64_t pid_lo, int64_t N) {
    const int64_t first = pid_lo % nu;
    return N / nu + (((u - first + nu) % nu) < N % nu ? 1 : 0);
}
// The arrays of a store of d.nseg segments and d.cap slots, for nk_alloc_particles and nk_regrow alike: the particle fields, the
// segments' counters, the split sweep's event queues and (developer build) the stamp words.  Whatever it allocated before an
// error is in ctx->pallocs, where the caller finds it.
static int nk_alloc_store(nk_ctx *ctx, bool pid, bool nts, bool seg_lo, bool split) {
    NkDev &d = ctx->d;
    const size_t nseg = (size_t)d.nseg, cap = (size_t)d.cap;
    NK_TRY(nk_alloc_fields(ctx, d, d.cap, pid, nts));
    NK_TRY(nk_palloc(ctx, d.seg_count, nseg));
    NK_TRY(nk_palloc(ctx, d.seg_new, nseg));
    NK_TRY(nk_palloc(ctx, d.seg_bound, nseg));
    if (seg_lo) NK_TRY(nk_palloc(ctx, d.seg_lo, nseg));
    if (split) {
        NK_TRY(nk_palloc(ctx, d.qx, cap)); NK_TRY(nk_palloc(ctx, d.qy, cap)); NK_TRY(nk_palloc(ctx, d.qz, cap));
        NK_TRY(nk_palloc(ctx, d.qocc, cap)); NK_TRY(nk_palloc(ctx, d.qnts, cap));
        NK_TRY(nk_palloc(ctx, d.qw0, cap));
        if (pid) NK_TRY(nk_palloc(ctx, d.qpid, cap));
        NK_TRY(nk_palloc(ctx, d.seg_evq, 2 * nseg + 1));
    }
#ifdef NK_STAMPS
    NK_TRY(nk_palloc(ctx, d.stamps, nseg * 16));
#endif
    return NK_OK;
}
static int nk_alloc_particles(nk_ctx *ctx, int64_t capacity, const int32_t *mode = nullptr, int64_t N = 0,
                              const int32_t *umodes = nullptr, int64_t nu = 0, int64_t pid_lo = 0) {
    if (ctx) ctx->emitted_for = -1;
    NkDev &d = ctx->d;
    NK_TRY(nk_entry_tables_drop(ctx, true));
    for (void *p : ctx->pallocs) hipFree(p);
    ctx->pallocs.clear();
    // Segments = load-balance granularity of the persistent sweep.  For large ensembles exactly ONE segment per resident wave
    // (long segments amortise the per-segment costs: first-tile latency, the partial last event batch and spawn tile, and
    // a whole number per wave keeps the waves level).  Small ensembles: more, shorter segments, down to 128 slots, until
    // every resident wave has one -- a wave's serial chain (tiles, event passes, entering particles) is what a small
    // sweep waits for.
    d.part = nk_want_part(ctx) ? 1 : 0;
    d.box = nk_want_box(ctx) ? 1 : 0;
    d.nlrec = 0;
    int64_t nseg = 0;
    // the sweep's LDS (hence its residency, hence the segment count) depends on the record area, which depends on the segment
    // count: settle in a few rounds
    for (int round = 0; round < 4; ++round) {
        const int64_t waves = (int64_t)nk_sweep_blocks(ctx) * (NK_WG / 64);
        int64_t ns = capacity / 128;
        if (const char *e = getenv("NK_SEGMENTS")) ns = atoi(e) > 0 ? atoi(e) : ns;          // developer probe
        else if (ns >= waves) ns = waves;
        ns = ns < 64 ? 64 : (ns > NK_MAX_SEGMENTS ? NK_MAX_SEGMENTS : ns);
        const bool same = ns == nseg;
        nseg = ns;
        d.nseg = (int32_t)nseg;
        // slots per segment: the mean share of the modes plus head room for the uneven shares of nk_build_mode_map
        d.nlmax = d.M > 0 ? (int32_t)((d.M + nseg - 1) / nseg) : 1;
        if (d.part && d.M > nseg) d.nlmax += d.nlmax / 6 + 2;
        // the segments' mode records in LDS where a segment's share fits and the LDS they take costs no resident workgroup
        d.nlrec = 0;
        if (d.part && d.nlmax <= NK_LREC && !getenv("NK_NO_LREC")) {
            const int without = nk_sweep_blocks(ctx);
            d.nlrec = d.nlmax;
            if (nk_sweep_blocks(ctx) < without) d.nlrec = 0;
        }
        if (same) break;
    }
    NK_ARG(d.nlmax < (1 << 14), "too many modes per segment for k_emit's packed entry word: use more particles (segments) or fewer modes");
    NK_TRY(nk_build_mode_map(ctx));
    {   // bits of the stored mode index; the rest of the 32-bit word holds facet + 1
        const int64_t maxidx = d.part ? d.nlmax - 1 : (d.M > 0 ? d.M - 1 : 0);
        int lb = 1;
        while ((1ll << lb) <= maxidx) ++lb;
        NK_ARG(lb < 30 && (int64_t)d.Fc + 1 < (1ll << (31 - lb)), "mesh has too many facets for the packed particle word (facets x modes)");
        d.lb = lb;
    }
    int64_t segcap = (capacity + nseg - 1) / nseg;
    if (d.part && (mode || umodes) && N > 0) {           // room for the fullest segment of this population + a step's arrivals
        std::vector<int64_t> per((size_t)nseg, 0);
        if (mode) { for (int64_t i = 0; i < N; ++i) if (mode[i] >= 0 && mode[i] < d.M) per[(size_t)nk_mode_seg(ctx, mode[i], (int)nseg)] += 1; }
        else for (int64_t u = 0; u < nu; ++u) per[(size_t)nk_mode_seg(ctx, umodes[u], (int)nseg)] += nk_tiled_count(u, nu, pid_lo, N);
        int64_t mx = 0;
        for (int64_t v : per) mx = std::max(mx, v);
        segcap = std::max(segcap, mx + mx / 4 + 64);
    }
    const bool tight = getenv("NK_TIGHT_STORE") != nullptr;      // test hook: barely enough room, so that a growing ensemble halts soon
    if (ctx->have_material && d.R > 0 && !ctx->h_enter_prob.empty())
        segcap = (tight ? segcap : std::max(segcap, segcap / 8 * 9)) + (tight ? 1 : 2) * nk_spawn_bound(ctx, (int)nseg) + 2 * NK_TILE;
    segcap = ((segcap + 63) / 64) * 64;
    NK_ARG(nseg * segcap < (1ll << 31), "particle store too large for 32-bit slot arithmetic");
    d.segcap = (int32_t)segcap;
    d.cap = nseg * segcap;
    ctx->timing.slots = d.cap;
    d.seg_lo = nullptr; d.down = 0; ctx->walked = false;
    d.qx = d.qy = d.qz = d.qocc = d.qnts = nullptr; d.qw0 = nullptr; d.qpid = nullptr; d.seg_evq = nullptr;
    NK_TRY(nk_alloc_store(ctx, nk_want_pid(ctx), !d.box, true, nk_want_split(ctx)));   // (seg_lo zeroed: the particles start at slot 0 of their segments)
    ctx->layout_key = (d.part ? 1 : 0) | (d.pid ? 2 : 0) | (d.qx ? 4 : 0) | (d.box ? 8 : 0);
    // tables that follow the segmentation: permuted mode records, 'one_to_one' inboxes
    if (ctx->have_material) NK_TRY(nk_update_tau_window(ctx, true));
    if (ctx->inbox) { hipFree(ctx->inbox); ctx->inbox = nullptr; }
    if (ctx->inbox_n) { hipFree(ctx->inbox_n); ctx->inbox_n = nullptr; }
    d.sp_inbox = nullptr; d.sp_inbox_n = nullptr; d.sp_icap = 0;
    if (ctx->mig_buf) { hipFree(ctx->mig_buf); ctx->mig_buf = nullptr; }
    if (ctx->mig_n) { hipFree(ctx->mig_n); ctx->mig_n = nullptr; }
    d.mig_buf = nullptr; d.mig_n = nullptr; d.mig_cap = 0;
    NK_TRY(nk_place_store(ctx));
    return nk_entry_tables_build(ctx);
}

// Rough facets with partitioned modes: per-segment inboxes of 64-byte records for the particles that change segment
// (`cap` records each; 0 = half a segment).  The inboxes are empty between steps, so resizing them loses nothing.
static int nk_ensure_migration(nk_ctx *ctx, int64_t cap) {
    NkDev &d = ctx->d;
    if (!(d.Fr > 0 && d.part)) return NK_OK;
    if (cap <= 0) cap = std::max<int64_t>(256, d.segcap / 2);
    if (d.mig_buf && d.mig_cap >= cap) return NK_OK;
    if (ctx->mig_buf) { hipFree(ctx->mig_buf); ctx->mig_buf = nullptr; }
    if (ctx->mig_n) { hipFree(ctx->mig_n); ctx->mig_n = nullptr; }
    d.mig_buf = nullptr; d.mig_n = nullptr; d.mig_cap = 0;
    NK_HIP(hipMalloc(&ctx->mig_buf, (size_t)d.nseg * cap * 64));
    NK_HIP(hipMalloc(&ctx->mig_n, (size_t)d.nseg * 4));
    NK_HIP(hipMemset(ctx->mig_n, 0, (size_t)d.nseg * 4));
    d.mig_buf = (double2 *)ctx->mig_buf; d.mig_n = (int32_t *)ctx->mig_n; d.mig_cap = (int32_t)cap;
    return NK_OK;
}

// 'one_to_one': per-segment inboxes for the records of k_emit_one_to_one
static int nk_ensure_inbox(nk_ctx *ctx) {
    NkDev &d = ctx->d;
    if (!(d.R > 0 && d.res_gen == 2) || d.sp_inbox) return NK_OK;
    const int64_t icap = 4 * (ctx->o2o_first / d.nseg + 64);
    NK_HIP(hipMalloc(&ctx->inbox, (size_t)d.nseg * icap * 8));
    NK_HIP(hipMalloc(&ctx->inbox_n, (size_t)d.nseg * 4));
    NK_HIP(hipMemset(ctx->inbox_n, 0, (size_t)d.nseg * 4));
    d.sp_inbox = (uint64_t *)ctx->inbox; d.sp_inbox_n = (int32_t *)ctx->inbox_n; d.sp_icap = (int32_t)icap;
    return NK_OK;
}

// Grow every segment to `segcap_new` slots on the device (same segmentation: the particles keep their segments).
static int nk_regrow(nk_ctx *ctx, int64_t segcap_new) {
    if (ctx) ctx->emitted_for = -1;
    NK_TRY(nk_normalize(ctx));
    NkDev &d = ctx->d;
    NK_HIP(hipStreamSynchronize(ctx->stream));
    const NkDev old = d;
    std::vector<void *> old_allocs;
    old_allocs.swap(ctx->pallocs);
    void *const old_store = ctx->store_buf; const size_t old_pad = ctx->store_pad;
    segcap_new = ((segcap_new + 63) / 64) * 64;
    NK_ARG((int64_t)old.nseg * segcap_new < (1ll << 31), "particle store too large for 32-bit slot arithmetic");
    d.segcap = (int32_t)segcap_new;
    d.cap = (int64_t)d.nseg * d.segcap;
    // (the old store was moved down above: k_regrow copies from slot 0; the event queues are empty between steps: new ones, nothing to copy)
    const int rc = nk_alloc_store(ctx, (bool)old.pid, (bool)old.nts, old.seg_lo != nullptr, old.qx != nullptr);
    if (rc) {                                            // out of memory: keep the old store
        for (void *p : ctx->pallocs) hipFree(p);
        ctx->pallocs.swap(old_allocs);
        ctx->store_buf = old_store; ctx->store_pad = old_pad;
        d = old;
        return rc;
    }
    ctx->timing.regrows += 1;
    k_regrow<<<ctx->num_cu * 8, NK_WG, 0, ctx->stream>>>(old, d);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    for (void *p : old_allocs) hipFree(p);
    ctx->timing.slots = d.cap;
    return nk_place_store(ctx);       // (the old store's memory is free again: often the better place)
}

int nk_reserve(nk_ctx *ctx, int64_t capacity) {
    NK_ARG(ctx, "nk_reserve: NULL context");
    NK_ARG(capacity > 0 && capacity < (1ll << 31) - (1 << 20), "nk_reserve: capacity out of range");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    if (capacity <= d.cap) return NK_OK;
    if (d.cap == 0) return nk_alloc_particles(ctx, capacity);
    // Same number of segments before and after (every large ensemble: one segment per resident wave): the segments grow in
    // place on the device.  Otherwise the particles are re-dealt through the host.
    int64_t nseg_new = capacity / 128;
    const int64_t waves = (int64_t)nk_sweep_blocks(ctx) * (NK_WG / 64);
    if (nseg_new >= waves) nseg_new = waves;
    nseg_new = nseg_new < 64 ? 64 : (nseg_new > NK_MAX_SEGMENTS ? NK_MAX_SEGMENTS : nseg_new);
    if (nseg_new == d.nseg || getenv("NK_SEGMENTS")) return nk_regrow(ctx, (capacity + d.nseg - 1) / d.nseg);
    NkHostParticles h;
    int rc = nk_gather_live(ctx, h, true);
    if (rc) return rc;
    rc = nk_alloc_particles(ctx, capacity, h.mode.data(), (int64_t)h.mode.size());
    if (rc) return rc;
    if (!h.x.empty())
        return nk_scatter(ctx, (int64_t)h.x.size(), h.x.data(), h.y.data(), h.z.data(), h.mode.data(), h.occ.data(),
                          h.nts.data(), h.facet.data(), h.pid.data(), 0);
    return NK_OK;
}

int nk_upload_particles(nk_ctx *ctx, int64_t N, const double *x, const double *y, const double *z, const int32_t *mode,
                        const double *occ, const double *n_ts, const int32_t *facet, const uint64_t *pid,
                        uint64_t pid_offset) {
    NK_ARG(ctx && N >= 0, "nk_upload_particles: bad arguments");
    NK_ARG(N == 0 || (x && y && z && mode && occ), "nk_upload_particles: x, y, z, mode, occ are required");
    NK_ARG(ctx->have_material, "nk_upload_particles: call nk_set_material first");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    NK_HIP(hipStreamSynchronize(ctx->stream));
    if (n_ts && facet && ctx->mesh_box && !ctx->box_forbidden) {
        // a state handed over WITH its cached hits: a box store re-derives them from the positions, which is the same thing
        // only for particles inside the box (nk_init_boundaries has the other half of this rule)
        const double *k = d.box_k;
        for (int64_t i = 0; i < N && !ctx->box_forbidden; ++i)
            if (facet[i] >= 0 && !(x[i] >= k[0] && x[i] <= -k[1] && y[i] >= k[2] && y[i] <= -k[3] && z[i] >= k[4] && z[i] <= -k[5])) ctx->box_forbidden = true;
    }
    bool fits = d.cap > 0 && ctx->layout_key == ((nk_want_part(ctx) ? 1 : 0) | (nk_want_pid(ctx) ? 2 : 0) | (nk_want_split(ctx) ? 4 : 0) | (nk_want_box(ctx) ? 8 : 0)) && N + N / 5 + 1024 <= d.cap;
    if (fits && d.part) {                              // every segment must hold its modes' particles with head room
        std::vector<int64_t> per((size_t)d.nseg, 0);
        for (int64_t i = 0; i < N; ++i) if (mode[i] >= 0 && mode[i] < d.M) per[(size_t)nk_mode_seg(ctx, mode[i], d.nseg)] += 1;
        const int64_t room = (int64_t)d.segcap - nk_spawn_bound(ctx, d.nseg) - 2 * NK_TILE;
        for (int64_t v : per) fits = fits && v + v / 16 <= room;
    }
    if (!fits) {                                       // forget old contents and size for 1.5 N
        const int64_t want = getenv("NK_TIGHT_STORE") ? N + N / 8 + 1024 : N + N / 2 + 65536;
        int rc = nk_alloc_particles(ctx, std::max(want, d.cap), mode, N);
        if (rc) return rc;
    }
    int rc = nk_scatter(ctx, N, x, y, z, mode, occ, n_ts, facet, pid, pid_offset);
    if (rc) return rc;
    int32_t zero6[6] = {0, 0, 0, 0, 0, 0};
    NK_HIP(hipMemcpy(d.halt, zero6, 24, hipMemcpyHostToDevice));     // halt[4], overflow, ticket
    ctx->pending_relax = false;
    return NK_OK;
}

static int nk_check_ready(nk_ctx *ctx) {
    NK_ARG(ctx->have_material && ctx->have_mesh && ctx->have_sv && ctx->have_params,
           "engine not configured: need material, mesh, subvolumes and params");
    NkDev &d = ctx->d;
    // every rough / reservoir facet must be backed by its table, otherwise a kernel would index garbage
    for (int f = 0; f < d.Fc; ++f) {
        const NkFacet &hf = ctx->host_facets[f];
        NK_ARG(hf.bc != 'R' || hf.rough >= 0, "a facet has BC 'R' but nk_set_rough did not cover it");
        NK_ARG(!(hf.bc == 'T' || hf.bc == 'F') || hf.res >= 0, "a facet has BC 'T' but nk_set_reservoirs did not cover it");
    }
    NK_ARG(d.cap > 0, "no particle storage: call nk_reserve / nk_upload_particles");
    NK_ARG(nk_lds(ctx, true, 3) <= 160 * 1024 && nk_lds(ctx, true, 1) <= 160 * 1024, "tables do not fit the 160 KiB LDS");
    // the store's layout follows the configuration (ids, partitioned modes): tables set after the upload re-deal it
    const int want = (nk_want_part(ctx) ? 1 : 0) | (nk_want_pid(ctx) ? 2 : 0) | (nk_want_split(ctx) ? 4 : 0) | (nk_want_box(ctx) ? 8 : 0);
    if (ctx->layout_key != want) {
        NkHostParticles h;
        int rc = nk_gather_live(ctx, h, true);
        if (rc) return rc;
        const bool had_pid = (bool)d.pid;
        const int64_t cap_old = d.cap;
        if ((rc = nk_alloc_particles(ctx, cap_old, h.mode.data(), (int64_t)h.mode.size()))) return rc;
        if (!h.x.empty() && (rc = nk_scatter(ctx, (int64_t)h.x.size(), h.x.data(), h.y.data(), h.z.data(), h.mode.data(), h.occ.data(),
                                             h.nts.data(), h.facet.data(), had_pid ? h.pid.data() : nullptr, 0)))
            return rc;
    }
    return NK_OK;
}

// Mesh._count_crossings of the host geometry on a device (no context needed): see k_mesh_crossings.
int nk_mesh_crossings(int device, int64_t n_rays, const double *origins, const double *dirs, int64_t n_faces, const double *v0,
                      const double *e1, const double *e2, int skip_self, int32_t *counts) {
    if (n_rays <= 0 || n_faces <= 0 || !origins || !dirs || !v0 || !e1 || !e2 || !counts) return NK_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return NK_ERR_HIP;
    double *buf = nullptr;
    int32_t *dc = nullptr;
    const size_t nr = (size_t)n_rays * 3, nf = (size_t)n_faces * 3;
    if (hipMalloc((void **)&buf, (2 * nr + 3 * nf) * sizeof(double)) != hipSuccess) return NK_ERR_HIP;
    if (hipMalloc((void **)&dc, (size_t)n_rays * sizeof(int32_t)) != hipSuccess) { hipFree(buf); return NK_ERR_HIP; }
    double *po = buf, *pd = po + nr, *p0 = pd + nr, *p1 = p0 + nf, *p2 = p1 + nf;
    hipError_t e = hipMemcpy(po, origins, nr * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pd, dirs, nr * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p0, v0, nf * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p1, e1, nf * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p2, e2, nf * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        k_mesh_crossings<<<(int)((n_rays + NK_WG - 1) / NK_WG), NK_WG>>>(n_rays, po, pd, n_faces, p0, p1, p2, skip_self, dc);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(counts, dc, (size_t)n_rays * sizeof(int32_t), hipMemcpyDeviceToHost);
    hipFree(buf); hipFree(dc);
    return e == hipSuccess ? NK_OK : NK_ERR_HIP;
}

int nk_init_boundaries(nk_ctx *ctx) {
    NK_ARG(ctx, "nk_init_boundaries: NULL context");
    int rc = nk_check_ready(ctx);
    if (rc) return rc;
    NK_HIP(hipSetDevice(ctx->device));
    if ((rc = nk_normalize(ctx))) return rc;
    for (int pass = 0; pass < 2; ++pass) {
        NK_HIP(hipMemsetAsync(ctx->anomalies, 0, 4, ctx->stream));
        NK_GEOM_LAUNCH(k_init_boundaries, nk_sweep_grid(ctx), nk_lds(ctx, true), ctx->d, ctx->anomalies);
        NK_HIP(hipGetLastError());
        int32_t bad = 0;
        NK_HIP(hipMemcpyAsync(&bad, ctx->anomalies, 4, hipMemcpyDeviceToHost, ctx->stream));
        NK_HIP(hipStreamSynchronize(ctx->stream));
        if (!(ctx->d.box && bad > 0)) break;
        // Particles that start OUTSIDE the box and would meet a wall from behind (a resumed state with particles behind their
        // reservoir face, test ensembles planted outside): the reference runs their event when they reach that wall, a store
        // without cached hits would let them fly in.  This context keeps the cached layout from here on.
        ctx->box_forbidden = true;
        if ((rc = nk_check_ready(ctx))) return rc;       // re-deals the store (layout key changed)
    }
    return NK_OK;
}

static int nk_flush_relax(nk_ctx *ctx, int honor_halt) {
    if (!ctx->pending_relax) return NK_OK;
    NK_TRY(nk_normalize(ctx));
    k_relax<<<nk_sweep_grid(ctx), NK_WG, nk_lds(ctx, false), ctx->stream>>>(ctx->d, honor_halt);
    NK_HIP(hipGetLastError());
    ctx->pending_relax = false;
    return NK_OK;
}

// ---- band-resolved heat flux (k_spectral, nk_kernels.h).  A workgroup keeps S x Bt bins of 28 B in LDS behind the subvolume
// tables, within the 64 KB a launch gets without asking; a table of more bands is done in tiles of Bt bands, one pass each.
static inline size_t nk_band_lds0(const nk_ctx *ctx) { return (nk_lds(ctx, false) + 15) & ~(size_t)15; }
static inline int nk_band_tile(const nk_ctx *ctx) {
    const size_t l0 = nk_band_lds0(ctx), per = (size_t)ctx->d.S * 28;
    if (l0 >= 65536 || per == 0) return 0;
    return (int)std::min<size_t>((65536 - l0) / per, (size_t)ctx->band_B);
}
static inline int nk_band_grid(const nk_ctx *ctx) { return std::max(1, std::min(2 * ctx->num_cu, (int)ctx->d.nseg)); }
// slabs for one pass and `rows` reduced rows on the device
static int nk_band_ensure(nk_ctx *ctx, int rows) {
    const int S = ctx->d.S, B = ctx->band_B, Bt = nk_band_tile(ctx);
    NK_ARG(Bt > 0, "band-resolved flux: the subvolume tables leave no room for one band's bins in 64 KB of LDS");
    const size_t ns = (size_t)nk_band_grid(ctx) * 4 * S * Bt, nr = (size_t)rows * 4 * S * B;
    if (ns > ctx->band_slabs_n) {
        if (ctx->band_slabs) hipFree(ctx->band_slabs);
        ctx->band_slabs = nullptr; ctx->band_slabs_n = 0;
        NK_HIP(hipMalloc((void **)&ctx->band_slabs, ns * sizeof(double)));
        ctx->band_slabs_n = ns;
    }
    if (nr > ctx->band_rows_n) {
        if (ctx->band_rows_d) hipFree(ctx->band_rows_d);
        ctx->band_rows_d = nullptr; ctx->band_rows_n = 0;
        NK_HIP(hipMalloc((void **)&ctx->band_rows_d, nr * sizeof(double)));
        ctx->band_rows_n = nr;
    }
    return NK_OK;
}
// One band row [4 S B] into row_dev: k_spectral + k_spectral_reduce per tile of bands (step mode honours the halt word).
static int nk_band_pass(nk_ctx *ctx, bool state, double *row_dev) {
    const NkDev &d = ctx->d;
    const int S = d.S, B = ctx->band_B, Bt = nk_band_tile(ctx), G = nk_band_grid(ctx);
    const size_t l0 = nk_band_lds0(ctx);
    for (int b0 = 0; b0 < B; b0 += Bt) {
        const int bt = std::min(Bt, B - b0);
        const size_t lds = l0 + (size_t)S * bt * 28;
        if (state) k_spectral<true><<<G, NK_SPEC_WG, lds, ctx->stream>>>(d, ctx->band_map, b0, bt, (int)l0, ctx->band_slabs);
        else k_spectral<false><<<G, NK_SPEC_WG, lds, ctx->stream>>>(d, ctx->band_map, b0, bt, (int)l0, ctx->band_slabs);
        const int nc = 4 * S * bt;
        k_spectral_reduce<<<(nc + 3) / 4, 256, 0, ctx->stream>>>(state ? nullptr : d.halt, ctx->band_slabs, G, S, B, b0, bt, row_dev);
    }
    NK_HIP(hipGetLastError());
    return NK_OK;
}

// ---- spatial field maps (k_field; nk_field.hip).  The bounds of the terms follow the temperatures the run can hold and the
// scales the slots of the store (all ranks): both are looked at again at the start of every nk_step / nk_tally_field_state
// call and after the store has grown -- places every rank of a communicator reaches together.
static int nk_field_refresh(nk_ctx *ctx) {
    NkFieldHost &F = ctx->field;
    const NkDev &d = ctx->d;
    const int fe = ctx->params.flux_every;
    NK_ARG(fe > 0 && F.cfg.every % fe == 0, "field: every must be a positive multiple of flux_every");
    // (host values only: nothing is copied or synchronised here; one rank pays two comparisons per nk_step call)
    double T_hi = std::max(ctx->h_Tgrid.empty() ? 0.0 : ctx->h_Tgrid.back(), d.Tfill_hi);
    if (!d.T_ref_local) T_hi = std::max(T_hi, d.T_ref);
    if (d.R > 0) T_hi = std::max(T_hi, ctx->res_T_max);
    if (T_hi != F.T_hi) {
        F.T_hi = T_hi;
        F.BE = d.kb * T_hi; F.BF = F.vmax * F.BE;
        if (F.cfg.flags & NK_FIELD_TEST_SMALL_BOUND) F.BE = ldexp(F.BE, -40);
        F.capacity = 0;
    }
    // One rank: the store's slots.  With a communicator the scales must be the same on every rank, so the slots are summed
    // over the ranks -- a rank may have reserved on its own since the last call, which the others cannot know without asking:
    // one small all-reduce per nk_step call, the price of integers that can be all-reduced.
    double cap = (double)d.cap;
    if (ctx->comm) NK_TRY(nk_comm_allreduce(ctx, &cap, 1));
    const int64_t slots = std::max<int64_t>((int64_t)cap, F.cfg.capacity);      // (nk_field.capacity: a floor the caller chose)
    if (slots != F.capacity) nk_field_scale(F, slots);
    return NK_OK;
}
// ---- grouped field maps (k_field<., true>; nk_field.hip).  Grid, cadence, bounds and scales are the field's, so the field's
// refresh serves both; what is the groups' own is the table in the segments' order, rebuilt wherever the field looks at its
// scales again (a new mode map, a store that has grown).
static int nk_fgroups_refresh(nk_ctx *ctx) {
    const hipError_t e = nk_fgroups_permute(ctx->fgroups, ctx->d, ctx->map_gen, ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->err = "nk_set_field_groups: the table in the segments' order (" + std::to_string((long long)ctx->d.nseg * ctx->d.nlmax * 4) +
                   " bytes): " + hipGetErrorString(e);
        return NK_ERR_HIP;
    }
    return NK_OK;
}
// ---- what the field's grid and the groups' share (grouped: which of the two)
static NkFieldGrid &nk_field_grid(nk_ctx *ctx, bool grouped) { return grouped ? ctx->fgroups.g : ctx->field.g; }
// One pass into the integer grid; summed over the ranks (integers: the result does not depend on who held which particle).
static int nk_field_sample(nk_ctx *ctx, bool grouped, bool state) {
    NkFieldGrid &g = nk_field_grid(ctx, grouped);
    NK_HIP(nk_field_pass(ctx->field, grouped ? &ctx->fgroups : nullptr, ctx->d, state, nk_lds(ctx, false), ctx->num_cu, ctx->stream));
    if (ctx->comm) {
        ncclResult_t nrc = ctx->rccl.AllReduce(g.grid, g.grid, ((size_t)g.lines + 1) * 8, ncclInt64, ncclSum, ctx->comm, ctx->stream);
        if (nrc != ncclSuccess) { ctx->err = std::string("ncclAllReduce of the ") + (grouped ? "field groups'" : "field") + " grid failed"; return NK_ERR_COMM; }
    }
    return NK_OK;
}
static const char NK_FIELD_LEFT_OUT[] = " (occupations outside the material's temperature range?); they were left out of the sums";
static std::string nk_field_overflow(const nk_ctx *ctx, bool grouped, const char *who, long long ovE, long long ovF) {
    return std::string(who) + (grouped ? ": field groups overflow: " : ": field overflow: ") + std::to_string(ovE) + " term(s) of E above B_E = " +
           std::to_string(ctx->field.BE) + " eV, " + std::to_string(ovF) + " term(s) of F above B_F = " + std::to_string(ctx->field.BF);
}
// The status words {samples, clamped, overflow E, overflow F [, ungrouped]} (the field's 4, the groups' 8); a term above its
// bound is an error that names the sum.
static int nk_field_status(nk_ctx *ctx, bool grouped, long long st[8], const char *who) {
    NkFieldGrid &g = nk_field_grid(ctx, grouped);
    NK_HIP(hipMemcpy(st, g.status, (size_t)g.nstatus * sizeof(long long), hipMemcpyDeviceToHost));
    if (st[NK_FIELD_ST_OVE] || st[NK_FIELD_ST_OVF]) {
        long long z[2] = {0, 0};
        NK_HIP(hipMemcpy(g.status + NK_FIELD_ST_OVE, z, sizeof(z), hipMemcpyHostToDevice));
        ctx->err = nk_field_overflow(ctx, grouped, who, st[NK_FIELD_ST_OVE], st[NK_FIELD_ST_OVF]) + NK_FIELD_LEFT_OUT;
        return NK_ERR_CAPACITY;
    }
    return NK_OK;
}
// The accumulator of a grid as N [lines], E [lines], F [lines][3] and two of its status words; reset = start a new window.
static int nk_field_get(nk_ctx *ctx, bool grouped, const char *who, double *N, double *E, double *F, int64_t *samples, int64_t *count, int count_word, int32_t reset) {
    NkFieldGrid &g = nk_field_grid(ctx, grouped);
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    const size_t nl = (size_t)g.lines;
    std::vector<double> a(nl * 5);
    NK_HIP(hipMemcpy(a.data(), g.acc, a.size() * sizeof(double), hipMemcpyDeviceToHost));
    long long st[8];
    int rc = nk_field_status(ctx, grouped, st, who);
    if (rc) return rc;
    for (size_t b = 0; b < nl; ++b) {
        if (N) N[b] = a[5 * b];
        if (E) E[b] = a[5 * b + 1];
        if (F) { F[3 * b] = a[5 * b + 2]; F[3 * b + 1] = a[5 * b + 3]; F[3 * b + 2] = a[5 * b + 4]; }
    }
    if (samples) *samples = st[NK_FIELD_ST_SAMPLES];
    if (count) *count = st[count_word];
    if (reset) {
        NK_HIP(hipMemset(g.acc, 0, a.size() * sizeof(double)));
        NK_HIP(hipMemset(g.status, 0, (size_t)g.nstatus * sizeof(long long)));
    }
    return NK_OK;
}

// ---- mode-resolved tally (k_modes; nk_modes.hip).  Bound and scale as the field's, looked at again at the same places.
static double nk_modes_T_hi(const nk_ctx *ctx) {
    const NkDev &d = ctx->d;
    double T_hi = std::max(ctx->h_Tgrid.empty() ? 0.0 : ctx->h_Tgrid.back(), d.Tfill_hi);
    if (!d.T_ref_local) T_hi = std::max(T_hi, d.T_ref);
    if (d.R > 0) T_hi = std::max(T_hi, ctx->res_T_max);
    return T_hi;
}
static int nk_modes_refresh(nk_ctx *ctx) {
    NkModesHost &Mo = ctx->modes;
    const NkDev &d = ctx->d;
    const int fe = ctx->params.flux_every;
    NK_ARG(fe > 0 && Mo.cfg.every % fe == 0, "modes: every must be a positive multiple of flux_every");
    const double T_hi = nk_modes_T_hi(ctx);
    if (T_hi != Mo.T_hi) nk_modes_bound(Mo, d.kb, T_hi);
    // (with a communicator the scale must be the same on every rank: the slots are summed over the ranks, as for the field)
    double cap = (double)d.cap;
    if (ctx->comm) NK_TRY(nk_comm_allreduce(ctx, &cap, 1));
    const int64_t slots = std::max<int64_t>((int64_t)cap, Mo.cfg.capacity);
    if (slots != Mo.capacity) nk_modes_scale(Mo, slots);
    return NK_OK;
}
// One pass into the sample table.  With a communicator only the header (overflow E, ran, skip) is summed over the ranks, so that
// every rank takes or drops the same samples; the table stays this rank's own (it is tens of megabytes).
static int nk_modes_sample(nk_ctx *ctx, bool state) {
    NkModesHost &Mo = ctx->modes;
    NK_HIP(nk_modes_pass(Mo, ctx->d, state, nk_lds(ctx, false), ctx->num_cu, ctx->stream));
    if (ctx->comm) {
        ncclResult_t nrc = ctx->rccl.AllReduce(Mo.hdr, Mo.hdr, 8, ncclInt64, ncclSum, ctx->comm, ctx->stream);
        if (nrc != ncclSuccess) { ctx->err = "ncclAllReduce of the mode tally's header failed"; return NK_ERR_COMM; }
    }
    return NK_OK;
}
// The status words {samples, skipped, overflow E, -}; a term above its bound is an error that names the sum.
static int nk_modes_status(nk_ctx *ctx, long long st[4], const char *who) {
    NkModesHost &Mo = ctx->modes;
    NK_HIP(hipMemcpy(st, Mo.status, 4 * sizeof(long long), hipMemcpyDeviceToHost));
    if (st[2]) {
        long long z = 0;
        NK_HIP(hipMemcpy(Mo.status + 2, &z, sizeof(z), hipMemcpyHostToDevice));
        ctx->err = std::string(who) + ": mode tally overflow: " + std::to_string(st[2]) + " term(s) of E above B_E = " + std::to_string(Mo.BE) +
                   " eV (occupations outside the material's temperature range?); they were left out of the sums";
        return NK_ERR_CAPACITY;
    }
    return NK_OK;
}

// [M][S] (the device's order: a segment's wave writes whole rows) -> [S][M] (the interface's)
extern "C++" {
template <typename TI, typename TO>
static void nk_modes_transpose(const TI *in, TO *out, int M, int S) {
    for (int m = 0; m < M; ++m)
        for (int s = 0; s < S; ++s) out[(size_t)s * M + m] = (TO)in[(size_t)m * S + s];
}
}

// ================================================================================ a batch of steps
// Up to `nsteps` timesteps are enqueued without host synchronisation, the stream is drained once, and the history rows are read.
// A sweep that sees a segment which COULD overflow at the following step raises the halt word; the remaining steps of the batch
// then do nothing, *done < nsteps comes back, and nk_step grows the store (state intact, nothing dropped) and carries on.
// Three paths step a batch: nk_step_batch (launches per step), nk_step_resident (many steps per launch) and nk_group_batch (shared
// launches of a replica group).  What a context keeps across them -- the frame NkBatch, the per-step record, the prelude of a
// contains-check step, the read-back and the hand-over to the next call -- exists once, below; a path supplies only its launches.
static inline NkRow nk_row(const nk_ctx *ctx) { return NkRow{ctx->d.NB, ctx->d.S}; }
// the step tallies every `every`-th step (steps count from 1 there) / runs the contains check ahead of it (every contains_every-th)
static inline bool nk_nth_step(int every, int64_t stepno) { return every > 0 && ((stepno + 1) % every) == 0; }
static inline bool nk_flux_step(const nk_ctx *ctx, int64_t stepno) { return nk_nth_step(ctx->params.flux_every, stepno); }
static inline bool nk_contains_step(const nk_ctx *ctx, int64_t stepno) {
    return ctx->params.contains_every > 0 && (stepno % ctx->params.contains_every) == 0 && ctx->d.nS > 0;
}

// The history rows live in pinned HOST memory that the device writes directly (1.1 KB per step over PCIe by the one
// workgroup of the update): no copy back, no fill kernel -- a driver that steps one by one pays for every operation of a
// call (round 3: fill + two copies = a tenth of such a call).
static int nk_batch_hist(nk_ctx *ctx, int32_t nsteps) {
    const size_t row_bytes = (size_t)nk_row(ctx).width() * sizeof(double);
    if (nsteps > ctx->hist_cap) {
        if (ctx->hist) hipHostFree(ctx->hist);
        ctx->hist = nullptr;
        ctx->hist_cap = 0;
        const int rows_alloc = nsteps < 1024 ? 1024 : nsteps;   // generous: a later, longer call must not pay a realloc
        NK_HIP(hipHostMalloc((void **)&ctx->hist, (size_t)rows_alloc * row_bytes, hipHostMallocMapped));
        ctx->hist_cap = rows_alloc;
    }
    ctx->timing.batches += 1;
    memset(ctx->hist, 0, (size_t)nsteps * row_bytes);   // row_valid = 0 (host memory; the stream is idle between calls)
    return NK_OK;
}

// The frame of a batch: what is decided once when it begins and what it hands over when it ends.
struct NkBatch {
    int g_sweep = 0, g_emit = 0;   // grids of the sweep and of the emission (k_emit, k_deliver, the emission's share of k_tail)
    bool tail_emit = false;        // the next step's emission rides in this step's tail launch
    bool alt = false;              // the sweeps alternate between walking their segments upwards and downwards
    bool relax0 = false;           // the step before the batch left its relaxation deferred ...
    bool flushed0 = false;         // ... and a k_relax ahead of the batch's first step has flushed it
    bool emitted_ahead = false;    // the coming step's emission has run already (in the tail of the step before it)
};
// Is a relaxation deferred when step s of the batch begins?  Every step leaves its own deferred, so only the first step asks.
// (This is the `pending` flag the three paths used to carry along: it has no state of its own.)
static inline bool nk_batch_pending(const NkBatch &b, int s) { return s > 0 || b.relax0; }

// Begin a batch.  resident: no tail launch, no alternating walk (k_resident emits inside and walks upwards only).
// *launches counts the kernels enqueued.
static int nk_batch_enter(nk_ctx *ctx, int32_t nsteps, NkBatch &b, bool resident = false, int64_t *launches = nullptr) {
    NkDev &d = ctx->d;
    NK_TRY(nk_batch_hist(ctx, nsteps));
    (void)nk_sweep_blocks(ctx);
    b.g_sweep = std::min(ctx->g_sweep, (d.nseg + 3) / 4);
    b.g_emit = std::min(ctx->num_cu * 8, (d.nseg + 3) / 4);
    d.tree_lds_fam0 = d.tree_nfam; d.tree_lds_off = 0;         // (the split sweep may move the top of the face tree: nk_events_lds)
    b.relax0 = ctx->pending_relax;
    b.flushed0 = false;
    // The next step's emission rides in the same launch as this step's reduce / update (k_tail) wherever it depends on neither
    // (no rough facets, not 'one_to_one').  (On a second stream instead, the two cross-stream event waits per step cost more
    // than the 12 us they hid: 0.289 against 0.270 ms per step on config 2, profiles/r03_notes.txt (11).)
    b.tail_emit = !resident && d.R > 0 && d.res_gen != 2 && !getenv("NK_NO_TAIL_EMIT");
    b.emitted_ahead = b.tail_emit && ctx->emitted_for == ctx->step;   // in the previous step's k_tail (maybe of the call before)
    ctx->emitted_for = -1;
    ctx->timing.emit_fused = resident ? 2 : b.tail_emit ? 1 : 0;      // (2: emission inside the resident kernel)
    // the fused sweeps of small meshes (box store or cached store) alternate between walking their segments upwards and downwards
    // (NkDev::down; nk_device.h), on every rank alike (the direction follows the step's parity).  Not the split sweep of large meshes:
    // measured no gain there (config 4's store is ten times the memory-side cache).  NK_NO_ALTERNATE=1: never.
    b.alt = !resident && d.seg_lo && nk_geom_mode(ctx) == 1 && !d.qx && !getenv("NK_NO_ALTERNATE");
    if (!b.alt) {
        if (launches && ctx->walked && d.seg_lo) *launches += 1;
        NK_TRY(nk_normalize(ctx));
    }
    d.down = 0;
    return NK_OK;
}
// What runs ahead of step s when it is a contains-check step (nothing on the others): the segments moved down, the deferred
// relaxation flushed, k_contains.  *launches counts the kernels enqueued.
static int nk_batch_prelude(nk_ctx *ctx, NkBatch &b, int s, int64_t *launches = nullptr) {
    NkDev &d = ctx->d;
    const int64_t stepno = ctx->step + s;
    if (!nk_contains_step(ctx, stepno)) return NK_OK;
    int64_t n = (ctx->walked && d.seg_lo) ? 1 : 0;
    NK_TRY(nk_normalize(ctx, 1));       // (k_relax, k_contains: particles from slot 0)
    if (nk_batch_pending(b, s)) {
        k_relax<<<nk_sweep_grid(ctx), NK_WG, nk_lds(ctx, false), ctx->stream>>>(d, 1);
        if (s == 0) b.flushed0 = true;
        n += 1;
    }
    NK_GEOM_LAUNCH(k_contains, nk_sweep_grid(ctx), nk_lds(ctx, true), d, (uint32_t)stepno);
    if (launches) *launches += n + 1;
    return NK_OK;
}
// What the launches of step s are passed (NkGroupRec, nk_group.h: a group uploads these, the other paths pass the values).
static NkGroupRec nk_batch_rec(const nk_ctx *ctx, const NkBatch &b, int s) {
    const int64_t stepno = ctx->step + s;
    NkGroupRec rec;
    rec.step = (uint32_t)stepno;
    rec.do_relax = (nk_batch_pending(b, s) && !nk_contains_step(ctx, stepno)) ? 1 : 0;   // (there k_relax has run ahead: nk_batch_prelude)
    rec.do_flux = nk_flux_step(ctx, stepno) ? 1 : 0;
    rec.down = b.alt ? (int32_t)(stepno & 1) : 0;
    rec.hist_row = ctx->hist + (size_t)s * nk_row(ctx).width();
    rec.acc = ctx->acc;
    return rec;
}
// After the wait: the rows into h, the steps that ran, and the halt words as the last step that ran left them (its update wrote
// them behind the row); no row: ask the device.
static int nk_batch_collect(nk_ctx *ctx, int32_t nsteps, std::vector<double> &h, int32_t *done) {
    const NkRow row = nk_row(ctx);
    const size_t W = (size_t)row.width();
    h.resize((size_t)nsteps * W);
    memcpy(h.data(), ctx->hist, (size_t)nsteps * W * sizeof(double));
    int32_t nd = 0;
    while (nd < nsteps && h[(size_t)nd * W + row.valid()] != 0.0) ++nd;
    if (nd > 0) for (int k_ = 0; k_ < 4; ++k_) ctx->halt_words[k_] = (int32_t)h[(size_t)(nd - 1) * W + row.halt(k_)];
    else NK_HIP(hipMemcpy(ctx->halt_words, ctx->d.halt, 16, hipMemcpyDeviceToHost));
    *done = nd;
    return NK_OK;
}
// How a batch of which nd steps ran leaves the emission that ran ahead and the deferred relaxation.
static void nk_batch_leave(nk_ctx *ctx, const NkBatch &b, int32_t nsteps, int32_t nd) {
    // the emission that ran ahead in the last tail is good for the next call unless the batch halted (the store grows first)
    const int32_t *hw_ = ctx->halt_words;
    ctx->emitted_for = (b.tail_emit && nd == nsteps && !hw_[0] && !hw_[2] && !hw_[3]) ? ctx->step + nsteps : -1;
    // the deferred relaxation as the device left it: pending after any completed step; if none ran, whatever it was before,
    // unless a k_relax ahead of the first step flushed it (that kernel honours the halt word, which was clear then)
    if (nd > 0) ctx->pending_relax = true;
    else ctx->pending_relax = b.relax0 && !b.flushed0;
}
// the two timing events of a call (evpool[64], [65]) and four per timed step; created once and reused
static int nk_batch_events(nk_ctx *ctx) {
    if (!ctx->evpool.empty()) return NK_OK;
    ctx->evpool.resize(16 * 4 + 2);
    for (auto &e : ctx->evpool) NK_HIP(hipEventCreate(&e));
    return NK_OK;
}

// k_events keeps the top of the face tree in LDS: as many whole levels as fit beside its tables at NK_EVENTS_OCC workgroups per CU
// (160 KB per CU; NK_EVENTS_TREE_LDS = bytes to use at most, 0 = none: developer probe).  Returns the kernel's dynamic LDS and
// sets NkDev::tree_lds_fam0 / tree_lds_off.
static size_t nk_events_lds(nk_ctx *ctx, size_t lds_g) {
    NkDev &d = ctx->d;
    size_t lds_ev = lds_g;
    if (!(d.qx && nk_geom_mode(ctx) == 2 && d.NG > 0 && d.tree_nfam > 0)) return lds_ev;
    const size_t off = (lds_g + 15) & ~(size_t)15, fixed = off + (size_t)NK_EVENTS_PEND * NK_EV_WG * 4 + 1024;
    size_t budget = (size_t)160 * 1024 / NK_EV_PER_CU > fixed ? (size_t)160 * 1024 / NK_EV_PER_CU - fixed : 0;
    if (const char *e = getenv("NK_EVENTS_TREE_LDS")) { const size_t v = (size_t)atol(e); if (v < budget) budget = v; }
    for (int l = 0; l <= d.tree_top; ++l) {
        const int fam0 = d.tree_base[l] >> 2;
        const size_t bytes = (size_t)(d.tree_nfam - fam0) * NK_TREE_FAMILY_FLOATS * 4;
        if (bytes <= budget) { d.tree_lds_fam0 = fam0; d.tree_lds_off = (int32_t)off; lds_ev = off + bytes; break; }
    }
    if (getenv("NK_VERBOSE") && ctx->timing.batches <= 1)
        fprintf(stderr, "[nanokappa_hip] k_events: families %d .. %d of the face tree in LDS (%zu B of %zu B per workgroup)\n", d.tree_lds_fam0, d.tree_nfam, lds_ev - off, lds_ev);
    return lds_ev;
}
// The side tallies of the particles the sweep of batch step s has just tallied (before the tail: T_sv still the tally's; timed
// with the tail, nk_timing.events_kernel_ms).  band_s: the batch step of each band row so far.
static int nk_side_tallies(nk_ctx *ctx, int s, std::vector<int> &band_s) {
    const int64_t stepno = ctx->step + s;
    if (!nk_flux_step(ctx, stepno)) return NK_OK;
    const int nranks = ctx->comm ? ctx->comm_nranks : 1;
    // the band-resolved flux: one row per heat-flux step (k_spectral)
    if (ctx->band_B > 0) {
        NK_TRY(nk_band_pass(ctx, false, ctx->band_rows_d + band_s.size() * 4 * (size_t)ctx->d.S * ctx->band_B));
        band_s.push_back(s);
    }
    // the field of the same particles on field steps (k_field; one launch per field step whatever the grid size)
    if (ctx->field.on && nk_nth_step(ctx->field.cfg.every, stepno)) {
        NK_TRY(nk_field_sample(ctx, false, false));
        NK_HIP(nk_field_accumulate(ctx->field.g, ctx->field, nranks, ctx->stream));
        // ... and the same sums per (cell, group of modes): taken or dropped with the field's sample
        if (ctx->fgroups.on) {
            NK_TRY(nk_field_sample(ctx, true, false));
            NK_HIP(nk_field_accumulate(ctx->fgroups.g, ctx->field, nranks, ctx->stream));
        }
    }
    // the mode-resolved tally of the same particles on mode steps (k_modes: one wave per segment)
    if (ctx->modes.on && nk_nth_step(ctx->modes.cfg.every, stepno)) {
        NK_TRY(nk_modes_sample(ctx, false));
        NK_HIP(nk_modes_accumulate(ctx->modes, nranks, ctx->num_cu, ctx->stream));
    }
    return NK_OK;
}
// The band rows of the nd steps that ran, from the device to ctx->band_rows / band_steps.
static int nk_band_collect(nk_ctx *ctx, const std::vector<int> &band_s, int32_t nd) {
    if (band_s.empty()) return NK_OK;
    const size_t rl = 4 * (size_t)ctx->d.S * ctx->band_B;
    std::vector<double> br(band_s.size() * rl);
    NK_HIP(hipMemcpyAsync(br.data(), ctx->band_rows_d, br.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    // a step whose migrants did not all fit their segments (k_deliver: halt word 2, the store grows before they are
    // delivered) has tallied particles the pass could not see: no row for it
    const int unseen = ctx->halt_words[2] ? nd - 1 : -1;
    for (size_t r = 0; r < band_s.size(); ++r) {
        if (band_s[r] >= nd || band_s[r] == unseen) continue;
        ctx->band_rows.insert(ctx->band_rows.end(), br.begin() + r * rl, br.begin() + (r + 1) * rl);
        ctx->band_steps.push_back(ctx->step + band_s[r]);
    }
    return NK_OK;
}
// nk_timing of a batch of nsteps of which nd ran: the kernels of its first nev steps (events ev[4 s .. 4 s + 3]) and the whole call
static int nk_batch_timing(nk_ctx *ctx, int nev, int32_t nsteps, int32_t nd) {
    const hipEvent_t *ev = ctx->evpool.data();
    float ms = 0.f;
    double sk = 0.0, ek = 0.0, vk = 0.0;
    const int nt = nd < nev ? nd : nev;
    for (int s = 0; s < nt; ++s) {
        NK_HIP(hipEventElapsedTime(&ms, ev[4 * s], ev[4 * s + 1])); ek += ms;
        NK_HIP(hipEventElapsedTime(&ms, ev[4 * s + 1], ev[4 * s + 2])); sk += ms;
        NK_HIP(hipEventElapsedTime(&ms, ev[4 * s + 2], ev[4 * s + 3])); vk += ms;
    }
    NK_HIP(hipEventElapsedTime(&ms, ev[64], ev[65]));
    if (nt > 0 && nd == nsteps) {
        ctx->timing.step_kernel_ms = sk / nt;
        ctx->timing.emit_kernel_ms = ek / nt;
        ctx->timing.events_kernel_ms = vk / nt;
        ctx->timing.total_ms = ms;
    }
    return NK_OK;
}
#ifdef NK_STAMPS
#include "nk_stamps.h"
#endif
// The one wait of a stepping call (nk_step_batch, nk_group_batch).  A call of a few steps (a driver that steps one by one) is over
// in a fraction of a millisecond: poll instead of sleeping on the stream -- the wake-up of a blocked wait is a tenth of such a call.
static int nk_wait_call(hipStream_t stream, int32_t nsteps, std::string &err) {
    hipError_t e = hipSuccess;
    const char *what = "hipStreamQuery";
    if (nsteps <= 4) while ((e = hipStreamQuery(stream)) == hipErrorNotReady) { }
    if (e == hipSuccess) { what = "hipStreamSynchronize(stream)"; e = hipStreamSynchronize(stream); }
    if (e != hipSuccess) { err = std::string(what) + ": " + hipGetErrorString(e); return NK_ERR_HIP; }
    return NK_OK;
}

// The launch-per-step path: the sequence of a step, written once.
static int nk_step_batch(nk_ctx *ctx, int32_t nsteps, std::vector<double> &h, int32_t *done) {
    NkDev &d = ctx->d;
    const int R = d.R, NB = d.NB;
    NkBatch b;
    NK_TRY(nk_batch_enter(ctx, nsteps, b));
    const size_t lds_g = nk_lds(ctx, true), lds_w = nk_lds(ctx, true, d.pid ? 3 : 2), lds_e = nk_lds(ctx, true, 1), lds_t = nk_tail_lds(ctx);
    const size_t lds_ev = nk_events_lds(ctx, lds_g);
    const NkSweepKind kind = nk_sweep_kind(ctx, true);
    const NkSweepFn sweep = nk_sweep_kernel(kind), events = kind.split ? nk_events_kernel(kind) : nullptr;
    NK_ARG(sweep && (events || !kind.split), "nk_step: no k_sweep / k_events is built for this configuration");
    if (kind.split) NK_HIP(nk_allow_lds((const void *)events, lds_ev));      // (the tree's top levels can take k_events past 64 KB)
    const int g_sweep = b.g_sweep, g_emit = b.g_emit;
    const int g_ev = kind.split ? ctx->num_cu * NK_EV_PER_CU : 0;    // k_events: resident waves drawing from all queues
    const int rows = g_sweep + g_ev;
    // per-kernel timing on the first 4 steps of a batch; none for the short calls of a driver that steps one by one (six event
    // records are a tenth of such a call).  Every record is a marker packet between two dependent kernels: measured ~2 us each
    // on the stream -- with records on 16 of a region's 20 steps (round 3) a step took 0.213 ms, in 100-step batches 0.206.
    const int nev = nsteps < 4 ? 0 : 4;
    NK_TRY(nk_batch_events(ctx));
    hipEvent_t *ev = ctx->evpool.data();
    NK_HIP(hipEventRecord(ev[64], ctx->stream));
    std::vector<int> band_s;                                  // batch step of each band row (one per heat-flux step; none when off)
    if (ctx->band_B > 0) {
        int nflux = 0;
        for (int s = 0; s < nsteps; ++s) nflux += nk_flux_step(ctx, ctx->step + s) ? 1 : 0;
        if (nflux > 0) NK_TRY(nk_band_ensure(ctx, nflux));
    }
    for (int s = 0; s < nsteps; ++s) {
        NK_TRY(nk_batch_prelude(ctx, b, s));
        const NkGroupRec rec = nk_batch_rec(ctx, b, s);
        const uint32_t step = rec.step;
        const int do_flux = rec.do_flux;
        if (s < nev) NK_HIP(hipEventRecord(ev[4 * s], ctx->stream));
        if (R > 0 && d.res_gen == 2) k_emit_one_to_one<<<ctx->num_cu * 4, NK_WG, 0, ctx->stream>>>(d, step);
        if (R > 0 && !b.emitted_ahead) NK_EMIT_LAUNCH(k_emit, g_emit, lds_e, d, step);
        if (s < nev) NK_HIP(hipEventRecord(ev[4 * s + 1], ctx->stream));
        if (b.alt) ctx->walked = true;
        d.down = rec.down;
        sweep<<<g_sweep, NK_WG, lds_w, ctx->stream>>>(d, step, rec.do_relax, do_flux);
        d.down = 0;
        if (kind.split) {
            k_events_begin<<<1, 1024, 0, ctx->stream>>>(d);
            events<<<g_ev, NK_EV_WG, lds_ev, ctx->stream>>>(d, step, do_flux, g_sweep);
            k_events_end<<<(d.nseg + 255) / 256, 256, 0, ctx->stream>>>(d);
        }
        // rough facets: the migrants of this step go to their segments before the tallies are reduced (and before the next step's
        // emission, in the tail launch, appends behind them)
        if (d.mig_buf) k_deliver<<<g_emit, NK_WG, 0, ctx->stream>>>(d, 1);
        if (s < nev) NK_HIP(hipEventRecord(ev[4 * s + 2], ctx->stream));
        NK_TRY(nk_side_tallies(ctx, s, band_s));
        double *hrow = rec.hist_row;
        const bool ahead = b.tail_emit;                        // the next step's emission beside this step's tail (the last step's too: for the next call)
        if (ctx->comm) {
            if (ahead) NK_EMIT_LAUNCH(k_tail, NB + g_emit, lds_t, d, step + 1u, rows, ctx->acc, hrow, do_flux, 0, NB);
            else k_reduce<<<NB, NK_WG, 0, ctx->stream>>>(d, rows, ctx->acc, hrow, do_flux, 0);
            ncclResult_t nrc = ctx->rccl.AllReduce(ctx->acc, ctx->acc, (size_t)NB + 2, ncclDouble, ncclSum, ctx->comm, ctx->stream);
            if (nrc != ncclSuccess) { ctx->err = "ncclAllReduce failed"; return NK_ERR_COMM; }
            k_update<<<1, NK_WG, 0, ctx->stream>>>(d, ctx->acc, hrow, do_flux);
        } else if (ahead) {
            NK_EMIT_LAUNCH(k_tail, NB + g_emit, lds_t, d, step + 1u, rows, ctx->acc, hrow, do_flux, 1, NB);
        } else {
            k_reduce<<<NB, NK_WG, 0, ctx->stream>>>(d, rows, ctx->acc, hrow, do_flux, 1);
        }
        b.emitted_ahead = ahead;
        if (s < nev) NK_HIP(hipEventRecord(ev[4 * s + 3], ctx->stream));
        if ((s & 63) == 0) NK_HIP(hipGetLastError());   // a bad launch configuration shows at the first step of a batch (every step launches the same)
    }
    NK_HIP(hipEventRecord(ev[65], ctx->stream));
    NK_HIP(hipGetLastError());
    // the history rows and the halt words come back through pinned memory, enqueued behind the steps: ONE wait per call (a
    // Population.run_timestep is one such call per step -- the reference driver's granularity, nanokappa.py:91-98)
    NK_TRY(nk_wait_call(ctx->stream, nsteps, ctx->err));
    NK_TRY(nk_batch_collect(ctx, nsteps, h, done));
#ifdef NK_STAMPS
    NK_TRY(nk_stamps_report(ctx));
#endif
    NK_TRY(nk_band_collect(ctx, band_s, *done));
    nk_batch_leave(ctx, b, nsteps, *done);
    return nk_batch_timing(ctx, nev, nsteps, *done);
}

// Small ensembles: many steps per launch (k_resident, nk_kernels.h).  OPT-IN (NK_RESIDENT=1): at 1e5 particles (31^3 x 6 modes)
// it measured faster than the launches it replaces -- 0.027 ms per step against 0.034-0.037 -- but at 1e6 slower, 0.057 against
// 0.048 (profiles/r04_notes.txt (17), (26); its first version, with FP64 atomics on shared addresses and device-scope fences,
// was slower at every size, (9)).  One rank, no rough facets, tables in LDS, not 'one_to_one', no RBF temperatures, at most
// NK_RESIDENT_MAX slots (default 1.2e6).
static inline bool nk_want_resident(const nk_ctx *ctx) {
    const NkDev &d = ctx->d;
    if (!getenv("NK_RESIDENT") || getenv("NK_NO_RESIDENT") || ctx->comm || d.nranks != 1 || d.Fr > 0 || d.mig_buf || d.qx || nk_geom_mode(ctx) != 1) return false;
    if (ctx->band_B > 0) return false;                 // the band-resolved flux pass runs between the launches of nk_step_batch
    if (ctx->field.on) return false;                   // ... and so does the field pass
    if (ctx->modes.on) return false;                   // ... and the mode tally's
    if (d.res_gen == 2 || d.sv_interp == 3 || d.NB > 254 || d.S > 128 || d.nseg <= 0) return false;
    const int64_t lim = getenv("NK_RESIDENT_MAX") ? atoll(getenv("NK_RESIDENT_MAX")) : 1200000;
    return d.cap <= lim && nk_lds(ctx, true, 5) <= 160 * 1024;
}
// The resident path: one launch for every run of steps up to the next contains-check step.
static int nk_step_resident(nk_ctx *ctx, int32_t nsteps, std::vector<double> &h, int32_t *done) {
    NkDev &d = ctx->d;
    const int NB = d.NB;
    NkBatch b;
    NK_TRY(nk_batch_enter(ctx, nsteps, b, true));     // (moves the segments down: the preludes then launch no k_anchor)
    const NkSweepKind kind = nk_sweep_kind(ctx, true);            // (nk_want_resident: tables in LDS, no split -- kind.box is d.box)
    const NkResidentFn resident = nk_resident_kernel(kind);
    NK_ARG(resident, "nk_step: no k_resident is built for this configuration");
    const size_t lds = nk_lds(ctx, true, kind.pid ? 5 : 4);
    // more dynamic LDS than the default limit of a launch has to be allowed (if that fails, the launch itself will say it does not fit)
    if (nk_allow_lds((const void *)resident, lds) != hipSuccess) (void)hipGetLastError();
    // every workgroup must be resident for the grid barrier: no more than the device holds at once (occupancy query), and no
    // more than there are segments
    int per_cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, resident, NK_WG, lds) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
    if (per_cu > 2) per_cu = 2;
    int G = std::min(ctx->num_cu * per_cu, (d.nseg + NK_WG / 64 - 1) / (NK_WG / 64));
    if (const char *e = getenv("NK_RESIDENT_GRID")) { const int v = atoi(e); if (v >= 1 && v < G) G = v; }   // developer probe
    G = std::max(1, G);
    // the tally rows, double-buffered by step parity (k_resident), live in `partials`: num_cu * 16 * NB doubles >= 2 G NBP, G <= 2 num_cu
    NK_ARG((size_t)2 * G * (size_t)((NB + 1) & ~1) <= (size_t)ctx->num_cu * 16 * NB, "nk_step_resident: tally rows exceed the partials buffer");
    NK_TRY(nk_batch_events(ctx));
    hipEvent_t t0 = ctx->evpool[64], t1 = ctx->evpool[65];
    if (!ctx->rbar) NK_HIP(hipMalloc((void **)&ctx->rbar, (32 + 4096) * sizeof(unsigned int)));
    NK_HIP(hipEventRecord(t0, ctx->stream));
    for (int k = 0; k < nsteps;) {
        NK_TRY(nk_batch_prelude(ctx, b, k));
        const NkGroupRec rec = nk_batch_rec(ctx, b, k);
        int n = 1;                                                // the steps of this launch: up to the next contains-check step
        while (k + n < nsteps && !nk_contains_step(ctx, ctx->step + k + n)) ++n;
        NK_HIP(hipMemsetAsync(ctx->rbar, 0, (32 + 1024 + 128) * sizeof(unsigned int), ctx->stream));     // the flags count from 1 in every launch
        resident<<<G, NK_WG, lds, ctx->stream>>>(d, rec.step, n, rec.do_relax, ctx->params.flux_every, rec.hist_row, nk_row(ctx).width(), ctx->rbar);
        NK_HIP(hipGetLastError());
        k += n;
    }
    NK_HIP(hipEventRecord(t1, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_TRY(nk_batch_collect(ctx, nsteps, h, done));
    const int32_t nd = *done;
    if (getenv("NK_VERBOSE") && ctx->timing.batches % 8 == 2) {   // developer probe: the clock marks of the launch's last step (10 ns ticks)
        unsigned long long m[12];
        NK_HIP(hipMemcpy(m, ctx->rbar + 8, sizeof(m), hipMemcpyDeviceToHost));
        if (m[0] && m[6] >= m[0])
            fprintf(stderr, "[nanokappa_hip] resident step, workgroup 0 [us]: sweep %.2f  row + flag %.2f  emission %.2f  all flags seen %.2f  rows summed %.2f  update published %.2f | workgroup G/2: sweep %.2f  row + emission %.2f  update seen %.2f\n",
                    (m[1] - m[0]) * 0.01, (m[2] - m[1]) * 0.01, (m[3] - m[2]) * 0.01, (m[4] - m[3]) * 0.01, (m[5] - m[4]) * 0.01, (m[6] - m[5]) * 0.01,
                    (m[9] - m[8]) * 0.01, (m[10] - m[9]) * 0.01, (m[11] - m[10]) * 0.01);
    }
    nk_batch_leave(ctx, b, nsteps, nd);
    float ms = 0.f;
    NK_HIP(hipEventElapsedTime(&ms, t0, t1));
    if (nd == nsteps && nd > 0) {
        ctx->timing.step_kernel_ms = (double)ms / nd;              // the resident kernel IS the step
        ctx->timing.emit_kernel_ms = 0.0;
        ctx->timing.events_kernel_ms = 0.0;
        ctx->timing.total_ms = ms;
    }
    return NK_OK;
}

// What the side tallies that are on derive from the store, again after anything that changed it: the field's scales, the groups'
// table in the segments' order, the mode tally's.
static int nk_tallies_refresh(nk_ctx *ctx) {
    if (ctx->field.on) NK_TRY(nk_field_refresh(ctx));
    if (ctx->fgroups.on) NK_TRY(nk_fgroups_refresh(ctx));
    if (ctx->modes.on) NK_TRY(nk_modes_refresh(ctx));
    return NK_OK;
}
// nk_step in three parts, shared with nk_group_step: what runs before the first batch of a call ...
static int nk_step_begin(nk_ctx *ctx) {
    int rc = nk_check_ready(ctx);
    if (rc) return rc;
    NK_HIP(hipSetDevice(ctx->device));
    if ((rc = nk_update_tau_window(ctx, false))) return rc;
    if ((rc = nk_ensure_inbox(ctx))) return rc;
    if ((rc = nk_ensure_migration(ctx, 0))) return rc;
    ctx->stepped = true;
    ctx->band_rows.clear();
    ctx->band_steps.clear();
    return nk_tallies_refresh(ctx);
}
struct NkStepRun {
    int32_t s_out = 0;     // rows delivered so far
    int overflow = 0;      // reason mask: 2 / 4 a segment filled up (tile commit / event survivors), 8 one_to_one inbox full,
                           // 16 one_to_one index overflow
    int grown = 0;
};
// ... what follows every batch: the nd rows of `h` go to the caller's arrays, the context moves on by nd steps, and a batch that
// halted is served (the store grows on the device, waiting migrants are delivered) ...
static int nk_step_consume(nk_ctx *ctx, int32_t nsteps, nk_tally *out, NkStepRun &run, const std::vector<double> &h, int32_t nd) {
    NkDev &d = ctx->d;
    const int S = d.S, R = d.R, NB = d.NB;
    const NkRow at = nk_row(ctx);
    int rc = NK_OK;
    for (int s = 0; s < nd; ++s) {
        const double *row = &h[(size_t)s * at.width()];
        if (row[at.overflow()] != 0.0) run.overflow |= (int)row[at.overflow()];
        if (!out) continue;
        const size_t q = (size_t)(run.s_out + s);
        if (out->E_raw) memcpy(out->E_raw + q * S, row, S * 8);
        if (out->N_sv) memcpy(out->N_sv + q * S, row + S, S * 8);
        if (out->flux_raw) {
            if (row[at.flux()] != 0.0) memcpy(out->flux_raw + q * 3 * S, row + 2 * S, 3 * S * 8);
            else for (int k = 0; k < 3 * S; ++k) out->flux_raw[q * 3 * S + k] = NAN;
        }
        if (out->N_leaving && R) memcpy(out->N_leaving + q * R, row + 5 * S, R * 8);
        if (out->res_energy && R) memcpy(out->res_energy + q * R, row + 5 * S + R, R * 8);
        if (out->res_flux && R) memcpy(out->res_flux + q * 3 * R, row + 5 * S + 2 * R, 3 * R * 8);
        if (out->N_emitted) out->N_emitted[q] = row[NB - 1];
        if (out->T_sv) memcpy(out->T_sv + q * S, row + at.T(), S * 8);
        if (out->E_sv) memcpy(out->E_sv + q * S, row + at.E(), S * 8);
    }
    if (nd > 0) {
        const double *last = &h[(size_t)(nd - 1) * at.width()];
        nk_track_T(ctx, last + at.T(), S);
        double live = 0.0;
        for (int k = 0; k < S; ++k) live += last[S + k];
        ctx->timing.live = (int64_t)live;
    }
    ctx->step += nd;
    run.s_out += nd;
    int32_t hw[4];
    memcpy(hw, ctx->halt_words, 16);                 // as the batch left them (copied with the history rows)
    if (run.s_out < nsteps || hw[0] || hw[2] || hw[3]) {
        // halted: a segment could overflow at the next step (or could not take its migrants, which then wait in its
        // inbox).  Grow every segment by half (on the device, state intact), deliver, and carry on.
        ctx->timing.halts += 1;
        if (++run.grown > 40) { ctx->err = "nk_step: the particle store keeps filling up"; return NK_ERR_CAPACITY; }
        const bool only_inbox = hw[3] && !hw[0] && !hw[2] && run.s_out == nsteps;
        if (!only_inbox) {
            const int64_t need = (int64_t)d.segcap + d.segcap / 2 + 2 * nk_spawn_bound(ctx, d.nseg) + 2 * NK_TILE;
            if ((rc = nk_regrow(ctx, need))) {
                ctx->err = "particle store nearly full after step " + std::to_string((long long)ctx->step) +
                           " and it could not be grown (" + ctx->err + "); the state is intact";
                return NK_ERR_CAPACITY;
            }
        }
        int32_t zero4[4] = {0, 0, 0, 0};
        NK_HIP(hipMemcpy(d.halt, zero4, 16, hipMemcpyHostToDevice));
        // (hw[2] comes out of the all-reduced vector: with several ranks every one of them is here at the same step, has
        // grown its segments by the same amount, and delivers whatever waits in its own inboxes)
        if (hw[2]) {                                 // migrants that did not fit: they do now
            k_deliver<<<ctx->num_cu * 8, NK_WG, 0, ctx->stream>>>(d, 0);
            NK_HIP(hipGetLastError());
            NK_HIP(hipStreamSynchronize(ctx->stream));
            int32_t again[4];
            NK_HIP(hipMemcpy(again, d.halt, 16, hipMemcpyDeviceToHost));
            if (again[2]) { ctx->err = "nk_step: migrating particles do not fit their segment after growing it"; return NK_ERR_CAPACITY; }
            NK_HIP(hipMemcpy(d.halt, zero4, 16, hipMemcpyHostToDevice));
        }
        if (d.mig_buf && (hw[3] || !only_inbox)) {   // inboxes follow the segments (or double when they ran half full)
            const int64_t want = std::max<int64_t>(hw[3] ? 2 * (int64_t)d.mig_cap : 0, d.segcap / 2);
            if ((rc = nk_ensure_migration(ctx, want))) return rc;
        }
        if ((rc = nk_update_tau_window(ctx, false))) return rc;
        if ((rc = nk_tallies_refresh(ctx))) return rc;                   // the store has grown
    }
    return NK_OK;
}
// ... and what ends the call
static int nk_step_end(nk_ctx *ctx, int overflow) {
    int rc = NK_OK;
    ctx->timing.slots = ctx->d.cap;
    if (overflow & 256) {                                // k_resident: its grid barrier was not met (a workgroup was not resident?)
        uint32_t z2[2] = {0u, 0u};
        NK_HIP(hipMemcpy(ctx->anomalies + 1, z2, 8, hipMemcpyHostToDevice));
        int32_t z = 0;
        NK_HIP(hipMemcpy(ctx->d.overflow, &z, 4, hipMemcpyHostToDevice));
        ctx->err = "nk_step: the resident kernel's grid barrier timed out; set NK_NO_RESIDENT=1";
        return NK_ERR_HIP;
    }
    if (overflow) {
        ctx->err = "particle capacity exceeded during nk_step (reason mask " + std::to_string(overflow) +
                   "): particles were dropped; call nk_reserve with a larger capacity";
        return NK_ERR_CAPACITY;
    }
    if (ctx->comm && !ctx->band_rows.empty()) {          // the band rows of the call: summed over the ranks in one all-reduce
        if ((rc = nk_comm_allreduce(ctx, ctx->band_rows.data(), (int64_t)ctx->band_rows.size()))) return rc;
    }
    if (ctx->field.on) {
        long long st[8];
        rc = nk_field_status(ctx, false, st, "nk_step");
        if (ctx->fgroups.on) {                           // (both are read, so that neither keeps a stale overflow for the next call)
            const std::string ef = ctx->err;
            long long sg[8];
            const int rcg = nk_field_status(ctx, true, sg, "nk_step");
            if (rc && rcg == NK_ERR_CAPACITY) ctx->err = ef + "; " + ctx->err;
            else if (rc) ctx->err = ef;
            if (!rc) rc = rcg;
        }
        if (rc) return rc;
    }
    if (ctx->modes.on) {
        long long st[4];
        if ((rc = nk_modes_status(ctx, st, "nk_step"))) return rc;
    }
    return NK_OK;
}

int nk_step(nk_ctx *ctx, int32_t nsteps, nk_tally *out) {
    NK_ARG(ctx && nsteps > 0, "nk_step: bad arguments");
    int rc = nk_step_begin(ctx);
    if (rc) return rc;
    NkStepRun run;
    std::vector<double> h;
    while (run.s_out < nsteps) {
        int32_t nd = 0;
        if ((rc = nk_want_resident(ctx) ? nk_step_resident(ctx, nsteps - run.s_out, h, &nd) : nk_step_batch(ctx, nsteps - run.s_out, h, &nd))) return rc;
        if ((rc = nk_step_consume(ctx, nsteps, out, run, h, nd))) return rc;
    }
    return nk_step_end(ctx, run.overflow);
}

// =============================================================================== replica groups
// R contexts with the same configuration stepped by shared launches (k_sweep_group / k_tail_group, nk_group.hip).  The group owns
// a device copy of the members' NkDevs (refreshed once per call: the lifetime window or a grown store change them), the prefix
// tables of the two grids, and one record per (step, member) of a call; everything else -- particles, tables, tallies, history
// rows, halt words, the alternating walk, the emission that ran ahead, the deferred relaxation -- stays the member's own and is
// kept by the code that keeps it for nk_step_batch (NkBatch, nk_batch_*), so that a member can be stepped alone between group calls.
struct nk_group {
    int R = 0;
    std::vector<nk_ctx *> m;
    int device = 0;
    std::string err;
    unsigned char *dev = nullptr;          // NkGroupHead, then NkDev[R]
    unsigned char *stage = nullptr;        // pinned host copy of the same
    NkGroupRec *recs_d = nullptr, *recs_h = nullptr;   // [recs_cap steps][R]; recs_h pinned
    int recs_cap = 0;
    std::vector<hipEvent_t> ev;            // 3 per timed step (4 steps), then the call's first and last
    std::vector<char> halted, alone;       // per member: it has halted / finished a call alone since the group was created
    nk_group_report rep = {};
};
static thread_local std::string g_group_error;

#define NK_GHIP(call)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            g->err = std::string(#call) + ": " + hipGetErrorString(e_);                                \
            return NK_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

// what the shared launches bake in: the members of a group agree on all of it
struct NkGroupKey {
    NkSweepKind kind;
    int S, R, NB, flux_every, contains_every, res_gen;
    double dt;
    int64_t step;
};
static NkGroupKey nk_group_key(nk_ctx *ctx) {
    const NkDev &d = ctx->d;
    NkGroupKey k;
    k.kind = nk_sweep_kind(ctx, true);                  // (the store's: nk_group_check has run nk_check_ready on every member)
    k.S = d.S; k.R = d.R; k.NB = d.NB;
    k.flux_every = ctx->params.flux_every; k.contains_every = ctx->params.contains_every; k.res_gen = d.res_gen;
    k.dt = d.dt;
    k.step = ctx->step;
    return k;
}
// What a group call is launched with: the members' common key and the largest LDS need among them (the LDS a member needs follows
// its segmentation -- the mode records of a segment -- hence its store size, in which members may differ: a launch asks for the
// largest need, every workgroup carves its own member's layout out of it).  Worked out once per call by nk_group_check.
struct NkGroupPlan { NkGroupKey key; size_t lds_w = 0, lds_t = 0; int device = 0; };
// "" when the member is inside the fast path's scope, else the reason
static std::string nk_group_scope(nk_ctx *ctx) {
    const NkDev &d = ctx->d;
    if (!(ctx->have_material && ctx->have_mesh && ctx->have_sv && ctx->have_params)) return "it is not ready (engine not configured: need material, mesh, subvolumes and params)";
    if (ctx->comm || d.nranks != 1) return "it belongs to a communicator (several ranks)";
    if (d.Fr > 0 || d.mig_buf) return "it has rough facets (their migrants are delivered between the sweep and the tail)";
    if (nk_geom_mode(ctx) != 1) return "its mesh is too large for tables in LDS";
    if (nk_want_split(ctx) || d.qx) return "it uses the split sweep";
    if (d.sv_interp == 3) return "it uses RBF temperatures";
    if (d.res_gen == 2) return "its generator is 'one_to_one'";
    if (ctx->band_B > 0) return "its band-resolved flux is on (nk_set_bands)";
    if (ctx->field.on) return "its field maps are on (nk_set_field)";
    if (ctx->modes.on) return "its mode tally is on (nk_set_modes)";
    if (d.R > 0 && getenv("NK_NO_TAIL_EMIT")) return "NK_NO_TAIL_EMIT is set (the emission would need a launch of its own)";
    return "";
}
// Everything nk_group_create refuses, also asked again by every nk_group_step (members may have been stepped alone or re-configured).
static int nk_group_check(nk_ctx *const *m, int R, NkGroupPlan *plan, std::string &err) {
    if (R < 1 || R > NK_GROUP_MAX_MEMBERS) { err = "nk_group: R = " + std::to_string(R) + " is outside 1 .. " + std::to_string(NK_GROUP_MAX_MEMBERS); return NK_ERR_ARG; }
    if (!m) { err = "nk_group: NULL members"; return NK_ERR_ARG; }
    for (int r = 0; r < R; ++r) {
        if (!m[r]) { err = "nk_group: member " + std::to_string(r) + " is NULL"; return NK_ERR_ARG; }
        for (int q = 0; q < r; ++q)
            if (m[q] == m[r]) { err = "nk_group: member " + std::to_string(r) + " is the same context as member " + std::to_string(q) + " (given twice)"; return NK_ERR_ARG; }
    }
    for (int r = 1; r < R; ++r)
        if (m[r]->device != m[0]->device) {
            err = "nk_group: member " + std::to_string(r) + " is on device " + std::to_string(m[r]->device) + ", member 0 on device " + std::to_string(m[0]->device);
            return NK_ERR_ARG;
        }
    for (int r = 0; r < R; ++r) {
        const std::string why = nk_group_scope(m[r]);
        if (!why.empty()) { err = "nk_group: member " + std::to_string(r) + " is outside the grouped path: " + why; return NK_ERR_ARG; }
    }
    for (int r = 0; r < R; ++r) {                        // (may re-deal a store whose layout no longer fits the configuration, as nk_step would)
        if (nk_check_ready(m[r])) { err = "nk_group: member " + std::to_string(r) + " is not ready: " + m[r]->err; return NK_ERR_ARG; }
        const std::string why = nk_group_scope(m[r]);
        if (!why.empty()) { err = "nk_group: member " + std::to_string(r) + " is outside the grouped path: " + why; return NK_ERR_ARG; }
    }
    size_t lds_w = 0, lds_t = 0;
    for (int r = 0; r < R; ++r) {
        const size_t w = nk_lds(m[r], true, m[r]->d.pid ? 3 : 2), tl = nk_tail_lds(m[r]);
        if (w > 64 * 1024 || tl > 64 * 1024) { err = "nk_group: member " + std::to_string(r) + " is outside the grouped path: its tables need more than 64 KB of LDS"; return NK_ERR_ARG; }
        lds_w = std::max(lds_w, w); lds_t = std::max(lds_t, tl);
    }
    const NkGroupKey k0 = nk_group_key(m[0]);
    for (int r = 1; r < R; ++r) {
        const NkGroupKey k = nk_group_key(m[r]);
        const char *what = nullptr;
        std::string a, b;
#define NK_GROUP_SAME(field, name) if (!what && !(k.field == k0.field)) { what = name; a = std::to_string(k.field); b = std::to_string(k0.field); }
        NK_GROUP_SAME(step, "current step")
        NK_GROUP_SAME(S, "subvolumes")
        NK_GROUP_SAME(R, "reservoirs")
        NK_GROUP_SAME(NB, "tally bins")
        NK_GROUP_SAME(flux_every, "flux_every")
        NK_GROUP_SAME(contains_every, "contains_every")
        NK_GROUP_SAME(dt, "dt")
        NK_GROUP_SAME(res_gen, "generator")
        NK_GROUP_SAME(kind.pid, "kernel instantiation (particle ids)")
        NK_GROUP_SAME(kind.lrec, "kernel instantiation (mode records in LDS)")
        NK_GROUP_SAME(kind.fast, "kernel instantiation (subvolume fast path)")
        NK_GROUP_SAME(kind.box, "kernel instantiation (box store)")
        // (nk_group_scope admits one value of each of these: a disagreement would be a fault of the scope's)
        NK_GROUP_SAME(kind.geom, "kernel instantiation (table placement)")
        NK_GROUP_SAME(kind.rough, "kernel instantiation (rough facets)")
        NK_GROUP_SAME(kind.rbf, "kernel instantiation (RBF temperatures)")
        NK_GROUP_SAME(kind.split, "kernel instantiation (split sweep)")
#undef NK_GROUP_SAME
        if (what) {
            err = "nk_group: member " + std::to_string(r) + " disagrees with member 0 on the " + what + " (" + a + " against " + b + ")";
            return NK_ERR_ARG;
        }
    }
    if (plan) { plan->key = k0; plan->lds_w = lds_w; plan->lds_t = lds_t; plan->device = m[0]->device; }
    return NK_OK;
}

int nk_group_create(nk_group **out, nk_ctx *const *members, int32_t R) {
    if (!out) { g_group_error = "nk_group_create: NULL out"; return NK_ERR_ARG; }
    *out = nullptr;
    NkGroupPlan plan;
    int rc = nk_group_check(members, R, &plan, g_group_error);
    if (rc) return rc;
    const int device = plan.device;
    nk_group *g = new nk_group();
    g->R = R;
    g->m.assign(members, members + R);
    g->halted.assign((size_t)R, 0);
    g->alone.assign((size_t)R, 0);
    g->device = device;
    g->rep.R = R;
    const size_t bytes = sizeof(NkGroupHead) + (size_t)NK_GROUP_MAX * sizeof(NkDev);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&g->dev, bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&g->stage, bytes, hipHostMallocDefault);
    if (e == hipSuccess) {
        g->ev.resize(3 * 4 + 2);
        for (auto &v : g->ev) { v = nullptr; if (e == hipSuccess) e = hipEventCreate(&v); }
    }
    if (e != hipSuccess) {
        g_group_error = std::string("nk_group_create: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        nk_group_destroy(g);
        return NK_ERR_HIP;
    }
    *out = g;
    return NK_OK;
}

void nk_group_destroy(nk_group *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    for (auto &v : g->ev) if (v) hipEventDestroy(v);
    if (g->dev) hipFree(g->dev);
    if (g->stage) hipHostFree(g->stage);
    if (g->recs_d) hipFree(g->recs_d);
    if (g->recs_h) hipHostFree(g->recs_h);
    delete g;
}

const char *nk_group_last_error(const nk_group *g) { return g ? g->err.c_str() : g_group_error.c_str(); }

int nk_group_info(nk_group *g, nk_group_report *out) {
    if (!g || !out) { if (g) g->err = "nk_group_info: NULL argument"; return NK_ERR_ARG; }
    *out = g->rep;
    return NK_OK;
}

// a member's error becomes the group's: "member r: ..."
static int nk_member_failed(nk_group *g, int r, int rc) {
    g->err = "member " + std::to_string(r) + ": " + g->m[(size_t)r]->err;
    return rc;
}
// nk_step_batch for all members at once, within the grouped path's scope (nk_group_scope): per step one k_sweep_group and one
// k_tail_group on `stream` (every member's ctx->stream is that stream during the call), one wait for the whole call.  hs[r] / nds[r]:
// member r's history rows and how many of its steps ran (a member that halted stops alone).
static int nk_group_batch(nk_group *g, const NkGroupPlan &plan, hipStream_t stream, int32_t nsteps, std::vector<std::vector<double>> &hs,
                          std::vector<int32_t> &nds) {
    const int R = g->R;
    int rc = NK_OK;
    const NkGroupKey &key = plan.key;
    const size_t lds_w = plan.lds_w, lds_t = plan.lds_t;
    const int NB = key.NB;
    NkGroupHead *head = reinterpret_cast<NkGroupHead *>(g->stage);
    NkDev *devs = reinterpret_cast<NkDev *>(g->stage + sizeof(NkGroupHead));
    for (int k = 0; k <= NK_GROUP_MAX; ++k) head->pre_sweep[k] = head->pre_tail[k] = INT32_MAX;
    for (int k = 0; k < NK_GROUP_MAX; ++k) head->rows[k] = 0;
    head->NB = NB; head->pad_ = 0;
    if (nsteps > g->recs_cap) {
        if (g->recs_d) hipFree(g->recs_d);
        if (g->recs_h) hipHostFree(g->recs_h);
        g->recs_d = g->recs_h = nullptr; g->recs_cap = 0;
        const int cap = nsteps < 1024 ? 1024 : nsteps;
        NK_GHIP(hipMalloc((void **)&g->recs_d, (size_t)cap * R * sizeof(NkGroupRec)));
        NK_GHIP(hipHostMalloc((void **)&g->recs_h, (size_t)cap * R * sizeof(NkGroupRec), hipHostMallocDefault));
        g->recs_cap = cap;
    }
    std::vector<NkBatch> mem((size_t)R);
    int grid_sweep = 0, grid_tail = 0;
    for (int r = 0; r < R; ++r) {
        nk_ctx *ctx = g->m[r];
        NkBatch &me = mem[(size_t)r];
        if ((rc = nk_batch_enter(ctx, nsteps, me, false, &g->rep.member_launches))) return nk_member_failed(g, r, rc);
        head->pre_sweep[r] = grid_sweep; head->pre_tail[r] = grid_tail; head->rows[r] = me.g_sweep;
        grid_sweep += me.g_sweep;
        grid_tail += NB + (me.tail_emit ? me.g_emit : 0);
        devs[r] = ctx->d;
        // the records of the whole call: what nk_step_batch passes to each step's launches
        for (int s = 0; s < nsteps; ++s) g->recs_h[(size_t)s * R + r] = nk_batch_rec(ctx, me, s);
    }
    head->pre_sweep[R] = grid_sweep; head->pre_tail[R] = grid_tail;
    NkGroupHead *head_d = reinterpret_cast<NkGroupHead *>(g->dev);
    NkDev *devs_d = reinterpret_cast<NkDev *>(g->dev + sizeof(NkGroupHead));
    NK_GHIP(hipMemcpyAsync(g->dev, g->stage, sizeof(NkGroupHead) + (size_t)R * sizeof(NkDev), hipMemcpyHostToDevice, stream));
    NK_GHIP(hipMemcpyAsync(g->recs_d, g->recs_h, (size_t)nsteps * R * sizeof(NkGroupRec), hipMemcpyHostToDevice, stream));
    const int nev = nsteps < 4 ? 0 : 4;                  // (nk_timing's convention: none for the short calls of a driver that steps one by one)
    hipEvent_t *ev = g->ev.data();
    hipEvent_t t0 = g->ev[12], t1 = g->ev[13];
    NK_GHIP(hipEventRecord(t0, stream));
    for (int s = 0; s < nsteps; ++s) {
        for (int r = 0; r < R; ++r) {                    // what a step may need per member: the prelude of a contains_check step ...
            nk_ctx *ctx = g->m[r];
            NkDev &d = ctx->d;
            NkBatch &me = mem[(size_t)r];
            if ((rc = nk_batch_prelude(ctx, me, s, &g->rep.member_launches))) return nk_member_failed(g, r, rc);
            // ... and an emission that no tail has run ahead (the first step after anything that changed the store or the tables)
            if (d.R > 0 && !me.emitted_ahead) {
                NK_EMIT_LAUNCH(k_emit, me.g_emit, nk_lds(ctx, true, 1), d, (uint32_t)(ctx->step + s));
                g->rep.member_launches += 1;
            }
            if (me.alt) ctx->walked = true;
            me.emitted_ahead = me.tail_emit;
        }
        if (s < nev) NK_GHIP(hipEventRecord(ev[3 * s], stream));
        NK_GHIP(nk_group_launch_sweep(key.kind, grid_sweep, lds_w, stream, head_d, devs_d, g->recs_d + (size_t)s * R));
        if (s < nev) NK_GHIP(hipEventRecord(ev[3 * s + 1], stream));
        NK_GHIP(nk_group_launch_tail(key.kind.box, grid_tail, lds_t, stream, head_d, devs_d, g->recs_d + (size_t)s * R));
        if (s < nev) NK_GHIP(hipEventRecord(ev[3 * s + 2], stream));
        g->rep.sweep_launches += 1;
        g->rep.tail_launches += 1;
    }
    NK_GHIP(hipEventRecord(t1, stream));
    NK_GHIP(hipGetLastError());
    g->rep.grid_sweep = grid_sweep;
    g->rep.grid_tail = grid_tail;
    if ((rc = nk_wait_call(stream, nsteps, g->err))) return rc;      // ONE wait per call
    bool all_ran = true;
    for (int r = 0; r < R; ++r) {
        nk_ctx *ctx = g->m[r];
        int32_t nd = 0;
        if ((rc = nk_batch_collect(ctx, nsteps, hs[(size_t)r], &nd))) return nk_member_failed(g, r, rc);
        nds[(size_t)r] = nd;
        nk_batch_leave(ctx, mem[(size_t)r], nsteps, nd);
        if (nd < nsteps) all_ran = false;
    }
    float ms = 0.f;
    if (nev > 0 && all_ran) {
        double sk = 0.0, tk = 0.0;
        for (int s = 0; s < nev; ++s) {
            NK_GHIP(hipEventElapsedTime(&ms, ev[3 * s], ev[3 * s + 1])); sk += ms;
            NK_GHIP(hipEventElapsedTime(&ms, ev[3 * s + 1], ev[3 * s + 2])); tk += ms;
        }
        g->rep.sweep_kernel_ms = sk / nev;
        g->rep.tail_kernel_ms = tk / nev;
    }
    NK_GHIP(hipEventElapsedTime(&ms, t0, t1));
    g->rep.total_ms = ms;
    return NK_OK;
}

int nk_group_step(nk_group *g, int32_t nsteps, nk_tally *outs) {
    if (!g) return NK_ERR_ARG;
    if (nsteps <= 0) { g->err = "nk_group_step: bad arguments"; return NK_ERR_ARG; }
    const int R = g->R;
    NkGroupPlan plan;
    int rc = nk_group_check(g->m.data(), R, &plan, g->err);
    if (rc) return rc;
    NK_GHIP(hipSetDevice(g->device));
    // one stream for the whole call: member 0's.  The members' own streams are idle between calls (every call ends with a wait).
    const hipStream_t stream = g->m[0]->stream;
    std::vector<hipStream_t> own((size_t)R);
    for (int r = 0; r < R; ++r) { own[(size_t)r] = g->m[r]->stream; g->m[r]->stream = stream; }
    auto leave = [&](int code) { for (int r = 0; r < R; ++r) g->m[r]->stream = own[(size_t)r]; return code; };
    for (int r = 0; r < R; ++r)
        if ((rc = nk_step_begin(g->m[r]))) return leave(nk_member_failed(g, r, rc));
    std::vector<std::vector<double>> hs((size_t)R);
    std::vector<int32_t> nds((size_t)R, 0);
    if ((rc = nk_group_batch(g, plan, stream, nsteps, hs, nds))) return leave(rc);
    g->rep.steps += nsteps;
    for (int r = 0; r < R; ++r) {
        nk_ctx *ctx = g->m[r];
        NkStepRun run;
        nk_tally *out = outs ? &outs[r] : nullptr;
        const int64_t halts0 = ctx->timing.halts;
        if ((rc = nk_step_consume(ctx, nsteps, out, run, hs[(size_t)r], nds[(size_t)r]))) return leave(nk_member_failed(g, r, rc));
        if (ctx->timing.halts != halts0 && !g->halted[(size_t)r]) { g->halted[(size_t)r] = 1; g->rep.halted += 1; }
        if (run.s_out < nsteps) {                        // a straggler: its store has grown, it takes its remaining steps alone
            if (!g->alone[(size_t)r]) { g->alone[(size_t)r] = 1; g->rep.finished_alone += 1; }
            std::vector<double> h;
            while (run.s_out < nsteps) {
                int32_t nd = 0;
                if ((rc = nk_step_batch(ctx, nsteps - run.s_out, h, &nd)) || (rc = nk_step_consume(ctx, nsteps, out, run, h, nd))) return leave(nk_member_failed(g, r, rc));
                g->rep.member_launches += 2 * (int64_t)nd;
            }
        }
        if ((rc = nk_step_end(ctx, run.overflow))) return leave(nk_member_failed(g, r, rc));
    }
    return leave(NK_OK);
}

int nk_download_particles(nk_ctx *ctx, int64_t capacity, double *x, double *y, double *z, int32_t *mode, double *occ,
                          double *n_ts, int32_t *facet, uint64_t *pid, int64_t *N_out) {
    NK_ARG(ctx && N_out, "nk_download_particles: NULL argument");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    *N_out = 0;
    if (d.cap == 0) return NK_OK;
    if (ctx->have_material && ctx->have_sv && ctx->have_mesh) NK_TRY(nk_flush_relax(ctx, 0));
    NkHostParticles h;
    int rc = nk_gather_live(ctx, h, capacity != 0);
    if (rc) return rc;
    const int64_t live = (int64_t)h.x.size();
    *N_out = live;
    if (capacity == 0) return NK_OK;
    NK_ARG(capacity >= live, "nk_download_particles: capacity smaller than the live particle count");
    if (x) memcpy(x, h.x.data(), live * 8);
    if (y) memcpy(y, h.y.data(), live * 8);
    if (z) memcpy(z, h.z.data(), live * 8);
    if (occ) memcpy(occ, h.occ.data(), live * 8);
    if (n_ts) memcpy(n_ts, h.nts.data(), live * 8);
    if (mode) memcpy(mode, h.mode.data(), live * 4);
    if (facet) memcpy(facet, h.facet.data(), live * 4);
    if (pid) memcpy(pid, h.pid.data(), live * 8);
    return NK_OK;
}

int nk_get_subvol_temperature(nk_ctx *ctx, double *T_sv) {
    NK_ARG(ctx && T_sv && ctx->have_sv, "nk_get_subvol_temperature: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_HIP(hipMemcpy(T_sv, ctx->d.T_sv, (size_t)ctx->d.S * 8, hipMemcpyDeviceToHost));
    return NK_OK;
}
int nk_set_subvol_temperature(nk_ctx *ctx, const double *T_sv) {
    NK_ARG(ctx && T_sv && ctx->have_sv, "nk_set_subvol_temperature: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<double> t(T_sv, T_sv + ctx->d.S);
    if (ctx->d.sv_interp == 3) nk_rbf_coefficients(ctx, t);
    NK_HIP(hipMemcpy(ctx->d.T_sv, t.data(), t.size() * 8, hipMemcpyHostToDevice));
    nk_track_T(ctx, T_sv, ctx->d.S);
    return NK_OK;
}
int nk_get_step(nk_ctx *ctx, int64_t *step) {
    NK_ARG(ctx && step, "nk_get_step: NULL argument");
    *step = ctx->step;
    return NK_OK;
}
int nk_get_timing(nk_ctx *ctx, nk_timing *t) {
    NK_ARG(ctx && t, "nk_get_timing: NULL argument");
    *t = ctx->timing;
    t->box_store = (ctx->d.cap > 0 && ctx->d.box) ? 1 : 0;
    return NK_OK;
}

// ------------------------------------------------------------------------------------------ RCCL
static int nk_load_rccl(NkRccl &r, std::string &err) {
    if (r.lib) return NK_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char *n : names) { r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (r.lib) break; }
    if (!r.lib) { err = std::string("cannot load librccl: ") + dlerror(); return NK_ERR_COMM; }
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
    r.AllReduce = (decltype(r.AllReduce))dlsym(r.lib, "ncclAllReduce");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
    r.CommCount = (decltype(r.CommCount))dlsym(r.lib, "ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank))dlsym(r.lib, "ncclCommUserRank");
    r.CommAbort = (decltype(r.CommAbort))dlsym(r.lib, "ncclCommAbort");         // (optional)
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.CommDestroy || !r.CommCount || !r.CommUserRank) { err = "librccl lacks expected symbols"; return NK_ERR_COMM; }
    return NK_OK;
}
int nk_comm_unique_id(void *id128) {
    static NkRccl r;
    std::string err;
    if (!id128) return NK_ERR_ARG;
    if (nk_load_rccl(r, err)) { g_create_error = err; return NK_ERR_COMM; }
    ncclUniqueId id;
    memset(&id, 0, sizeof(id));
    if (r.GetUniqueId(&id) != ncclSuccess) { g_create_error = "ncclGetUniqueId failed"; return NK_ERR_COMM; }
    memcpy(id128, &id, 128);
    return NK_OK;
}
int nk_comm_init(nk_ctx *ctx, const void *id128, int rank, int nranks) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && id128 && nranks >= 1 && rank >= 0 && rank < nranks, "nk_comm_init: bad arguments");
    NK_ARG(!ctx->stepped, "nk_comm_init: must be called before the first nk_step (emission ownership is per rank)");
    NK_HIP(hipSetDevice(ctx->device));
    ctx->d.rank = rank;
    ctx->d.nranks = nranks;
    if (nranks == 1 && !getenv("NK_FORCE_COMM")) return NK_OK;   // NK_FORCE_COMM: exercise RCCL with a 1-rank communicator
    if (getenv("NK_COMM_DRYRUN")) return NK_OK;   // test hook: this rank's share of the emission, no communicator (tallies stay local)
    if (nk_load_rccl(ctx->rccl, ctx->err)) return NK_ERR_COMM;
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    memcpy(&id, id128, 128);
    // every way out of here that is not NK_OK leaves the context as a single rank without communicator (a failed
    // self-test used to leave ctx->comm set and d.nranks = nranks behind)
    auto fail = [&](const std::string &why, bool hung) -> int {
        ctx->err = why;
        if (ctx->comm) {
            if (hung && ctx->rccl.CommAbort) ctx->rccl.CommAbort(ctx->comm);       // peers missing: a destroy would wait for them
            else if (!hung && ctx->rccl.CommDestroy) ctx->rccl.CommDestroy(ctx->comm);
        }
        ctx->comm = nullptr; ctx->comm_rank = -1; ctx->comm_nranks = 0; ctx->comm_selftest = 0.0;
        ctx->d.rank = 0; ctx->d.nranks = 1;
        return NK_ERR_COMM;
    };
    if (ctx->rccl.CommInitRank(&ctx->comm, nranks, id, rank) != ncclSuccess) { ctx->comm = nullptr; return fail("ncclCommInitRank failed", false); }
    // The communicator proves itself before anything relies on it: RCCL's own view of the rank count, then an all-reduce of
    // {1, rank + 1} on the engine's stream -- every expected rank took part exactly once iff the sums are nranks and
    // nranks (nranks + 1) / 2.
    int cn = 0, cr = -1;
    if (ctx->rccl.CommCount(ctx->comm, &cn) != ncclSuccess || ctx->rccl.CommUserRank(ctx->comm, &cr) != ncclSuccess) {
        return fail("ncclCommCount / ncclCommUserRank failed", false);
    }
    ctx->comm_nranks = cn; ctx->comm_rank = cr;
    if (cn != nranks || cr != rank) {
        return fail("RCCL reports rank " + std::to_string(cr) + " of " + std::to_string(cn) + ", expected rank " + std::to_string(rank) + " of " + std::to_string(nranks), false);
    }
    double *probe = nullptr, hp[2] = {1.0, (double)(rank + 1)};
    double *hpin = nullptr;                              // pinned: the copy back must really be asynchronous for the deadline below
    if (hipMalloc((void **)&probe, 16) != hipSuccess || hipHostMalloc((void **)&hpin, 16, hipHostMallocDefault) != hipSuccess) {
        if (probe) hipFree(probe);
        return fail("self-test of the new communicator: out of memory", false);
    }
    hpin[0] = hp[0]; hpin[1] = hp[1];
    hipError_t he = hipMemcpyAsync(probe, hpin, 16, hipMemcpyHostToDevice, ctx->stream);
    ncclResult_t nrc = he == hipSuccess ? ctx->rccl.AllReduce(probe, probe, 2, ncclDouble, ncclSum, ctx->comm, ctx->stream) : ncclSystemError;
    if (he == hipSuccess && nrc == ncclSuccess) he = hipMemcpyAsync(hpin, probe, 16, hipMemcpyDeviceToHost, ctx->stream);
    bool hung = false;
    if (he == hipSuccess && nrc == ncclSuccess) {
        // a rank that never joins would leave this all-reduce waiting for ever: poll with a deadline (NK_COMM_TIMEOUT_S, 180 s)
        const double limit = getenv("NK_COMM_TIMEOUT_S") ? atof(getenv("NK_COMM_TIMEOUT_S")) : 180.0;
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            he = hipStreamQuery(ctx->stream);
            if (he != hipErrorNotReady) break;
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) { hung = true; break; }
            struct timespec ts = {0, 200000};
            nanosleep(&ts, nullptr);
        }
    }
    if (hung) return fail("self-test all-reduce of the new communicator did not finish in time: a rank is missing", true);   // (probe stays allocated: the stream may still touch it)
    hp[0] = hpin[0]; hp[1] = hpin[1];
    hipFree(probe); hipHostFree(hpin);
    if (he != hipSuccess || nrc != ncclSuccess) return fail("self-test all-reduce of the new communicator failed", false);
    ctx->comm_selftest = hp[0];
    if (hp[0] != (double)nranks || hp[1] != 0.5 * (double)nranks * (double)(nranks + 1)) {
        return fail("self-test all-reduce returned " + std::to_string(hp[0]) + " / " + std::to_string(hp[1]) + " instead of " +
                    std::to_string(nranks) + " / " + std::to_string(nranks * (nranks + 1) / 2) + ": not every rank took part", false);
    }
    return NK_OK;
}
int nk_comm_allreduce(nk_ctx *ctx, double *inout, int64_t n) {
    NK_ARG(ctx && inout && n >= 0, "nk_comm_allreduce: bad arguments");
    if (!ctx->comm || n == 0) return NK_OK;
    NK_HIP(hipSetDevice(ctx->device));
    double *buf = nullptr;
    NK_HIP(hipMalloc((void **)&buf, (size_t)n * 8));
    hipError_t he = hipMemcpyAsync(buf, inout, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream);
    ncclResult_t nrc = he == hipSuccess ? ctx->rccl.AllReduce(buf, buf, (size_t)n, ncclDouble, ncclSum, ctx->comm, ctx->stream) : ncclSystemError;
    if (he == hipSuccess && nrc == ncclSuccess) he = hipMemcpyAsync(inout, buf, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (he == hipSuccess && nrc == ncclSuccess) he = hipStreamSynchronize(ctx->stream);
    hipFree(buf);
    if (he != hipSuccess || nrc != ncclSuccess) { ctx->err = "nk_comm_allreduce failed"; return NK_ERR_COMM; }
    return NK_OK;
}
int nk_comm_info(nk_ctx *ctx, nk_comm_report *out) {
    NK_ARG(ctx && out, "nk_comm_info: NULL argument");
    memset(out, 0, sizeof(*out));
    out->rank = ctx->d.rank; out->nranks = ctx->d.nranks;
    out->comm_rank = ctx->comm ? ctx->comm_rank : -1;
    out->comm_nranks = ctx->comm ? ctx->comm_nranks : 0;
    out->device = ctx->device;
    out->selftest_sum = ctx->comm ? ctx->comm_selftest : 0.0;
    out->selftest_ok = (ctx->comm && ctx->comm_selftest == (double)ctx->d.nranks) ? 1 : 0;
    if (hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof(out->pci_bus_id), ctx->device) != hipSuccess) out->pci_bus_id[0] = 0;
    return NK_OK;
}

// ------------------------------------------------------------------------------------- parity taps
}  // extern "C"
// Scratch device buffer of a tap: freed on every return path.
template <class T>
struct NkDevBuf {
    T *p = nullptr;
    hipError_t err = hipSuccess;
    NkDevBuf(const T *src, int64_t count) {
        err = hipMalloc((void **)&p, (size_t)(count > 0 ? count : 1) * sizeof(T));
        if (err == hipSuccess && src) err = hipMemcpy(p, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice);
    }
    ~NkDevBuf() { if (p) hipFree(p); }
    hipError_t get(T *dst, int64_t count) const { return dst ? hipMemcpy(dst, p, (size_t)count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
    NkDevBuf(const NkDevBuf &) = delete;
    NkDevBuf &operator=(const NkDevBuf &) = delete;
};
#define NK_BUF(T, name, src, count) NkDevBuf<T> name(src, count); NK_HIP(name.err)
extern "C" {

// Population.initialise_all_particles on the device (k_init_particles): N particles with ids pid_lo .. pid_lo + N - 1, modes
// tiled over the ids, positions uniform in the solid ('random_domain': sv_first NULL) or in the subvolume the index
// belongs to ('random_subvol': sv_first[S + 1], ascending, sv_first[0] = 0).  Replaces nk_reserve + nk_upload_particles.
int nk_init_particles(nk_ctx *ctx, int64_t N, int64_t capacity, uint64_t pid_lo, const int32_t *unique_modes, int64_t n_unique,
                      const int64_t *sv_first) {
    if (ctx) ctx->emitted_for = -1;
    NK_ARG(ctx && N >= 0 && unique_modes && n_unique > 0, "nk_init_particles: bad arguments");
    NK_ARG(ctx->have_material && ctx->have_mesh && ctx->have_sv, "nk_init_particles: set the material, the mesh and the subvolumes first");
    NkDev &d = ctx->d;
    NK_ARG(d.nS > 0, "nk_init_particles: the mesh was set without its volume tables (simplices)");
    NK_ARG(nk_want_part(ctx), "nk_init_particles: needs the mode-partitioned store");
    for (int64_t u = 0; u < n_unique; ++u) NK_ARG(unique_modes[u] >= 0 && unique_modes[u] < d.M, "nk_init_particles: mode index out of range");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    int rc = nk_alloc_particles(ctx, std::max<int64_t>(capacity, N + N / 2 + 65536), nullptr, N, unique_modes, n_unique, (int64_t)(pid_lo % (uint64_t)n_unique));
    if (rc) return rc;
    NK_BUF(int32_t, um, unique_modes, n_unique);
    NK_BUF(int64_t, sf, sv_first, sv_first ? d.S + 1 : 0);
    NK_HIP(hipMemsetAsync(d.seg_count, 0, (size_t)d.nseg * sizeof(int32_t), ctx->stream));
    int32_t zero6[6] = {0, 0, 0, 0, 0, 0};
    NK_HIP(hipMemcpyAsync(d.halt, zero6, 24, hipMemcpyHostToDevice, ctx->stream));     // halt[4], overflow, ticket
    if (N > 0) k_init_particles<<<ctx->num_cu * 8, NK_WG, nk_lds(ctx, false), ctx->stream>>>(d, N, pid_lo, um.p, (int32_t)n_unique, sv_first ? sf.p : nullptr);
    NK_HIP(hipGetLastError());
    int32_t ovf = 0;
    NK_HIP(hipMemcpyAsync(&ovf, d.overflow, 4, hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_ARG(!(ovf & 64), "nk_init_particles: a particle did not find its subvolume in 4096 draws ('random_subvol' with very small "
                         "subvolumes): create the particles on the host (NK_HOST_INIT=1)");
    NK_ARG(ovf == 0, "nk_init_particles: a segment overflowed (internal sizing error)");
    ctx->pending_relax = false;
    return NK_OK;
}

// The tallies of the particles where they stand (the t = 0 row of the reference: calculate_energy and the flux sums before
// normalisation, Population.py:704-717, :734-736): E_raw[S], N[S], flux_raw[3 S] (subvolume-major).  This rank's particles only.
int nk_tally_state(nk_ctx *ctx, double *E_raw, double *N_sv, double *flux_raw) {
    NK_ARG(ctx && E_raw && N_sv && flux_raw, "nk_tally_state: bad arguments");
    int rc = nk_check_ready(ctx);
    if (rc) return rc;
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    if ((rc = nk_normalize(ctx))) return rc;
    if (ctx->pending_relax) {                          // the state the caller means includes the deferred relaxation
        k_relax<<<nk_sweep_grid(ctx), NK_WG, nk_lds(ctx, false), ctx->stream>>>(d, 0);
        ctx->pending_relax = false;
    }
    const int g = nk_sweep_grid(ctx);
    NK_BUF(double, acc, nullptr, d.NB + 2);
    k_tally_state<<<g, NK_WG, nk_lds(ctx, false), ctx->stream>>>(d);
    k_reduce<<<d.NB, NK_WG, 0, ctx->stream>>>(d, g, acc.p, nullptr, 1, 0);
    NK_HIP(hipGetLastError());
    std::vector<double> h((size_t)d.NB + 1);
    NK_HIP(hipMemcpyAsync(h.data(), acc.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    const int S = d.S;
    for (int s_ = 0; s_ < S; ++s_) { E_raw[s_] = h[(size_t)s_]; N_sv[s_] = h[(size_t)S + s_]; }
    for (int k = 0; k < 3 * S; ++k) flux_raw[k] = h[(size_t)2 * S + k];
    return NK_OK;
}

int nk_set_bands(nk_ctx *ctx, int32_t nbands, const int32_t *band_of_mode) {
    NK_ARG(ctx && nbands >= 0, "nk_set_bands: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->band_map) hipFree(ctx->band_map);
    if (ctx->band_slabs) hipFree(ctx->band_slabs);
    if (ctx->band_rows_d) hipFree(ctx->band_rows_d);
    ctx->band_map = nullptr; ctx->band_slabs = nullptr; ctx->band_rows_d = nullptr;
    ctx->band_slabs_n = ctx->band_rows_n = 0;
    ctx->band_B = 0;
    ctx->band_rows.clear();
    ctx->band_steps.clear();
    if (nbands == 0) return NK_OK;
    NK_ARG(band_of_mode, "nk_set_bands: band_of_mode is NULL");
    NK_ARG(ctx->have_material && ctx->have_sv, "nk_set_bands: set the material and the subvolumes first");
    const int M = ctx->d.M;
    for (int m = 0; m < M; ++m) NK_ARG(band_of_mode[m] >= -1 && band_of_mode[m] < nbands, "nk_set_bands: a band index is out of range");
    ctx->band_B = nbands;
    if (nk_band_tile(ctx) <= 0) {
        ctx->band_B = 0;
        ctx->err = "nk_set_bands: " + std::to_string(ctx->d.S) + " subvolumes leave no room for one band's bins in 64 KB of LDS";
        return NK_ERR_ARG;
    }
    hipError_t e = hipMalloc((void **)&ctx->band_map, (size_t)M * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(ctx->band_map, band_of_mode, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx->band_B = 0;
        ctx->err = std::string("nk_set_bands: ") + hipGetErrorString(e);
        return NK_ERR_HIP;
    }
    return NK_OK;
}

int nk_get_band_rows(nk_ctx *ctx, double *F, double *N, int64_t *steps, int32_t cap, int32_t *nrows) {
    NK_ARG(ctx && nrows && cap >= 0, "nk_get_band_rows: bad arguments");
    const int32_t n = (int32_t)ctx->band_steps.size();
    *nrows = n;
    if (n == 0 || cap == 0) return NK_OK;
    NK_ARG(cap >= n, "nk_get_band_rows: cap is smaller than the number of rows");
    const size_t sb = (size_t)ctx->d.S * ctx->band_B, rl = 4 * sb;
    for (int32_t r = 0; r < n; ++r) {
        const double *row = ctx->band_rows.data() + r * rl;
        if (F) memcpy(F + r * 3 * sb, row, 3 * sb * sizeof(double));
        if (N) memcpy(N + r * sb, row + 3 * sb, sb * sizeof(double));
        if (steps) steps[r] = ctx->band_steps[(size_t)r];
    }
    return NK_OK;
}

int nk_tally_bands_state(nk_ctx *ctx, double *F, double *N) {
    NK_ARG(ctx && F && N, "nk_tally_bands_state: bad arguments");
    NK_ARG(ctx->band_B > 0, "nk_tally_bands_state: no bands were set (nk_set_bands)");
    int rc = nk_check_ready(ctx);
    if (rc) return rc;
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    if ((rc = nk_normalize(ctx))) return rc;
    if (ctx->pending_relax) {                          // the state the caller means includes the deferred relaxation
        k_relax<<<nk_sweep_grid(ctx), NK_WG, nk_lds(ctx, false), ctx->stream>>>(d, 0);
        ctx->pending_relax = false;
    }
    if ((rc = nk_band_ensure(ctx, 1))) return rc;
    if ((rc = nk_band_pass(ctx, true, ctx->band_rows_d))) return rc;
    const size_t sb = (size_t)d.S * ctx->band_B;
    std::vector<double> h(4 * sb);
    NK_HIP(hipMemcpyAsync(h.data(), ctx->band_rows_d, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->comm && (rc = nk_comm_allreduce(ctx, h.data(), (int64_t)h.size()))) return rc;
    memcpy(F, h.data(), 3 * sb * sizeof(double));
    memcpy(N, h.data() + 3 * sb, sb * sizeof(double));
    return NK_OK;
}

// ---- spatial field maps: Population.plot_figures (Population.py:1841-1979, drawn at :123 and every 100 steps at :1735) as sums
// on a grid instead of a scatter of every particle
int nk_set_field(nk_ctx *ctx, const nk_field *f) {
    NK_ARG(ctx && f, "nk_set_field: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    nk_field_free(ctx->field);
    nk_fgroups_free(ctx->fgroups);
    if (f->n[0] == 0 && f->n[1] == 0 && f->n[2] == 0) return NK_OK;
    NK_ARG(ctx->have_material && ctx->have_sv, "nk_set_field: set the material and the subvolumes first");
    const NkDev &d = ctx->d;
    std::vector<double> vg((size_t)d.M * 3);
    NK_HIP(hipMemcpy(vg.data(), ctx->d_vg, vg.size() * sizeof(double), hipMemcpyDeviceToHost));
    double vmax = 0.0;
    for (int m = 0; m < d.M; ++m) vmax = std::max(vmax, sqrt(vg[3 * m] * vg[3 * m] + vg[3 * m + 1] * vg[3 * m + 1] + vg[3 * m + 2] * vg[3 * m + 2]));
    const double T_hi = std::max(ctx->h_Tgrid.empty() ? 0.0 : ctx->h_Tgrid.back(), d.Tfill_hi);
    int rc = nk_field_configure(ctx->field, f, ctx->params.flux_every, d.kb, T_hi, vmax, ctx->err);
    if (rc) return rc;
    NK_ARG(f->capacity >= 0, "nk_set_field: capacity must not be negative");
    nk_field_scale(ctx->field, std::max<int64_t>(std::max<int64_t>(d.cap, 1), f->capacity));   // (this rank's slots; nk_step looks again, over all ranks)
    return NK_OK;
}

int nk_get_field(nk_ctx *ctx, double *N, double *E, double *F, int64_t *samples, int64_t *clamped, int32_t reset) {
    NK_ARG(ctx, "nk_get_field: bad arguments");
    NK_ARG(ctx->field.on, "nk_get_field: no field was set (nk_set_field)");
    return nk_field_get(ctx, false, "nk_get_field", N, E, F, samples, clamped, NK_FIELD_ST_CLAMPED, reset);
}

// The raw integers of the state as it is now, of either grid: [lines][8], and the header's counts.  The ready check, the
// normalisation and the deferred relaxation of every state-mode tally, then refresh, one pass, copy-out, clear, header check.
static int nk_field_tally_state(nk_ctx *ctx, bool grouped, const char *who, int64_t *raw, int64_t *clamped, int64_t *ungrouped) {
    int rc = nk_check_ready(ctx);
    if (rc) return rc;
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    if ((rc = nk_normalize(ctx))) return rc;
    if (ctx->pending_relax) {                          // the state the caller means includes the deferred relaxation
        k_relax<<<nk_sweep_grid(ctx), NK_WG, nk_lds(ctx, false), ctx->stream>>>(d, 0);
        ctx->pending_relax = false;
    }
    if ((rc = nk_field_refresh(ctx))) return rc;
    if (grouped && (rc = nk_fgroups_refresh(ctx))) return rc;
    if ((rc = nk_field_sample(ctx, grouped, true))) return rc;
    NkFieldGrid &g = nk_field_grid(ctx, grouped);
    const size_t nl = (size_t)g.lines;
    std::vector<int64_t> h((nl + 1) * 8);
    NK_HIP(hipMemcpyAsync(h.data(), g.grid, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(nk_field_clear_grid(g, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t *hdr = h.data() + nl * 8;
    if (hdr[NK_FIELD_OVE] || hdr[NK_FIELD_OVF]) {
        ctx->err = nk_field_overflow(ctx, grouped, who, (long long)hdr[NK_FIELD_OVE], (long long)hdr[NK_FIELD_OVF]) + (grouped ? NK_FIELD_LEFT_OUT : "");
        return NK_ERR_CAPACITY;
    }
    memcpy(raw, h.data(), nl * 8 * sizeof(int64_t));
    if (clamped) *clamped = hdr[NK_FIELD_CLAMPED];
    if (ungrouped) *ungrouped = hdr[NK_FIELD_UNGROUPED];
    return NK_OK;
}

int nk_tally_field_state(nk_ctx *ctx, int64_t *raw, int64_t *clamped) {
    NK_ARG(ctx && raw, "nk_tally_field_state: bad arguments");
    NK_ARG(ctx->field.on, "nk_tally_field_state: no field was set (nk_set_field)");
    return nk_field_tally_state(ctx, false, "nk_tally_field_state", raw, clamped, nullptr);
}

int nk_field_info(nk_ctx *ctx, nk_field_report *out) {
    NK_ARG(ctx && out, "nk_field_info: NULL argument");
    memset(out, 0, sizeof(*out));
    const NkFieldHost &fh = ctx->field;
    if (!fh.on) return NK_OK;
    for (int a = 0; a < 3; ++a) out->n[a] = fh.cfg.n[a];
    out->every = fh.cfg.every;
    out->ncells = fh.ncells;
    out->k_E = fh.kE; out->k_F = fh.kF;
    out->B_E = fh.BE; out->B_F = fh.BF;
    out->capacity = fh.capacity;
    out->bytes = fh.g.bytes;
    out->lds_path = nk_field_lds_bins(fh.g, fh.force_global, nk_lds(ctx, false)) ? 1 : 0;      // (what nk_field_pass asks, too)
    out->on = 1;
    return NK_OK;
}

// ---- grouped field maps: the field's sums per (cell, group of modes)
int nk_set_field_groups(nk_ctx *ctx, int32_t ngroups, const int32_t *group_of_mode) {
    NK_ARG(ctx, "nk_set_field_groups: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    nk_fgroups_free(ctx->fgroups);
    if (ngroups == 0) return NK_OK;
    NK_ARG(ngroups > 0 && group_of_mode, "nk_set_field_groups: ngroups must not be negative and the table is required");
    int rc = nk_fgroups_configure(ctx->fgroups, ctx->field, ngroups, group_of_mode, ctx->d.M, ctx->err);
    if (rc) return rc;
    if (ctx->d.cap > 0 && (rc = nk_fgroups_refresh(ctx))) return rc;
    return NK_OK;
}

int nk_get_field_groups(nk_ctx *ctx, double *N, double *E, double *F, int64_t *samples, int64_t *ungrouped, int32_t reset) {
    NK_ARG(ctx, "nk_get_field_groups: bad arguments");
    NK_ARG(ctx->fgroups.on, "nk_get_field_groups: no groups were set (nk_set_field_groups)");
    return nk_field_get(ctx, true, "nk_get_field_groups", N, E, F, samples, ungrouped, NK_FIELD_ST_UNGROUPED, reset);
}

int nk_tally_field_groups_state(nk_ctx *ctx, int64_t *raw, int64_t *clamped, int64_t *ungrouped) {
    NK_ARG(ctx && raw, "nk_tally_field_groups_state: bad arguments");
    NK_ARG(ctx->fgroups.on, "nk_tally_field_groups_state: no groups were set (nk_set_field_groups)");
    return nk_field_tally_state(ctx, true, "nk_tally_field_groups_state", raw, clamped, ungrouped);
}

int nk_field_groups_info(nk_ctx *ctx, nk_field_groups_report *out) {
    NK_ARG(ctx && out, "nk_field_groups_info: NULL argument");
    memset(out, 0, sizeof(*out));
    const NkFGroupsHost &Gh = ctx->fgroups;
    if (!Gh.on) return NK_OK;
    out->G = Gh.G;
    out->lines = Gh.g.lines;
    out->bytes = Gh.g.bytes;
    out->lds_path = nk_field_lds_bins(Gh.g, ctx->field.force_global, nk_lds(ctx, false)) ? 1 : 0;      // (what nk_field_pass asks, too)
    out->k_E = ctx->field.kE; out->k_F = ctx->field.kF;
    out->permutes = Gh.permutes;
    out->on = 1;
    return NK_OK;
}

// ---- mode-resolved tally: E and N per (subvolume, mode)
int nk_set_modes(nk_ctx *ctx, const nk_modes *m) {
    NK_ARG(ctx && m, "nk_set_modes: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    nk_modes_free(ctx->modes);
    if (m->every == 0) return NK_OK;
    NK_ARG(ctx->have_material && ctx->have_sv, "nk_set_modes: set the material and the subvolumes first");
    const NkDev &d = ctx->d;
    const double T_hi = std::max(ctx->h_Tgrid.empty() ? 0.0 : ctx->h_Tgrid.back(), d.Tfill_hi);
    int rc = nk_modes_configure(ctx->modes, m, ctx->params.flux_every, (int64_t)d.M * d.S, d.kb, T_hi, ctx->err);
    if (rc) return rc;
    nk_modes_scale(ctx->modes, std::max<int64_t>(std::max<int64_t>(d.cap, 1), m->capacity));   // (this rank's slots; nk_step looks again, over all ranks)
    return NK_OK;
}

int nk_get_modes(nk_ctx *ctx, double *N, double *E, int64_t *samples, int64_t *skipped, int32_t reset) {
    NK_ARG(ctx, "nk_get_modes: bad arguments");
    NkModesHost &Mo = ctx->modes;
    NK_ARG(Mo.on, "nk_get_modes: the mode tally is off (nk_set_modes)");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    const NkDev &d = ctx->d;
    const size_t nb = (size_t)Mo.nbins;
    long long st[4];
    int rc = nk_modes_status(ctx, st, "nk_get_modes");
    if (rc) return rc;
    if (N || E) {
        std::vector<double> a(nb);
        // the accumulators are per rank: summed over the ranks here, once, on a copy (ncclDouble)
        double *tmp = nullptr;
        if (ctx->comm) NK_HIP(hipMalloc((void **)&tmp, nb * 8));
        for (int w = 0; w < 2; ++w) {
            double *out = w ? E : N;
            if (!out) continue;
            const double *src = w ? Mo.accE : Mo.accN;
            if (ctx->comm) {
                hipError_t he = hipMemcpyAsync(tmp, src, nb * 8, hipMemcpyDeviceToDevice, ctx->stream);
                ncclResult_t nrc = he == hipSuccess ? ctx->rccl.AllReduce(tmp, tmp, nb, ncclDouble, ncclSum, ctx->comm, ctx->stream) : ncclSystemError;
                if (he == hipSuccess && nrc == ncclSuccess) he = hipStreamSynchronize(ctx->stream);
                if (he != hipSuccess || nrc != ncclSuccess) { hipFree(tmp); ctx->err = "nk_get_modes: the all-reduce of the accumulators failed"; return NK_ERR_COMM; }
                src = tmp;
            }
            hipError_t he = hipMemcpy(a.data(), src, nb * 8, hipMemcpyDeviceToHost);
            if (he != hipSuccess) { if (tmp) hipFree(tmp); NK_HIP(he); }
            nk_modes_transpose(a.data(), out, d.M, d.S);
        }
        if (tmp) hipFree(tmp);
    }
    if (samples) *samples = st[0];
    if (skipped) *skipped = st[1];
    if (reset) {
        NK_HIP(hipMemset(Mo.accE, 0, nb * 8));
        NK_HIP(hipMemset(Mo.accN, 0, nb * 8));
        NK_HIP(hipMemset(Mo.status, 0, 4 * sizeof(long long)));
    }
    return NK_OK;
}

int nk_tally_modes_state(nk_ctx *ctx, int64_t *N, int64_t *E) {
    NK_ARG(ctx && N && E, "nk_tally_modes_state: bad arguments");
    NkModesHost &Mo = ctx->modes;
    NK_ARG(Mo.on, "nk_tally_modes_state: the mode tally is off (nk_set_modes)");
    int rc = nk_check_ready(ctx);
    if (rc) return rc;
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    if ((rc = nk_normalize(ctx))) return rc;
    if (ctx->pending_relax) {                          // the state the caller means includes the deferred relaxation
        k_relax<<<nk_sweep_grid(ctx), NK_WG, nk_lds(ctx, false), ctx->stream>>>(d, 0);
        ctx->pending_relax = false;
    }
    if ((rc = nk_modes_refresh(ctx))) return rc;
    if ((rc = nk_modes_sample(ctx, true))) return rc;
    const size_t nb = (size_t)Mo.nbins;
    if (ctx->comm) {                                   // integers: the sum does not depend on who held which particle
        ncclResult_t nrc = ctx->rccl.AllReduce(Mo.tE, Mo.tE, nb, ncclInt64, ncclSum, ctx->comm, ctx->stream);
        if (nrc == ncclSuccess) nrc = ctx->rccl.AllReduce(Mo.tN, Mo.tN, nb, ncclInt32, ncclSum, ctx->comm, ctx->stream);
        if (nrc != ncclSuccess) { ctx->err = "ncclAllReduce of the mode table failed"; return NK_ERR_COMM; }
    }
    std::vector<int64_t> hE(nb);
    std::vector<int32_t> hN(nb);
    long long hdr[8];
    NK_HIP(hipMemcpyAsync(hE.data(), Mo.tE, nb * 8, hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipMemcpyAsync(hN.data(), Mo.tN, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipMemcpyAsync(hdr, Mo.hdr, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream));
    NK_HIP(hipMemsetAsync(Mo.hdr, 0, sizeof(hdr), ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    nk_modes_transpose(hE.data(), E, d.M, d.S);
    nk_modes_transpose(hN.data(), N, d.M, d.S);
    if (hdr[0]) {
        ctx->err = "nk_tally_modes_state: mode tally overflow: " + std::to_string(hdr[0]) + " term(s) of E above B_E = " +
                   std::to_string(Mo.BE) + " eV; they were left out of the sums";
        return NK_ERR_CAPACITY;
    }
    return NK_OK;
}

int nk_modes_info(nk_ctx *ctx, nk_modes_report *out) {
    NK_ARG(ctx && out, "nk_modes_info: NULL argument");
    memset(out, 0, sizeof(*out));
    const NkModesHost &Mo = ctx->modes;
    if (!Mo.on) return NK_OK;
    out->every = Mo.cfg.every;
    out->k_E = Mo.kE;
    out->B_E = Mo.BE;
    out->capacity = Mo.capacity;
    out->bytes = Mo.bytes;
    out->owner_path = nk_modes_owner(Mo, ctx->d, nk_lds(ctx, false)) ? 1 : 0;      // (what nk_modes_pass asks, too)
    out->on = 1;
    return NK_OK;
}

int nk_find_boundary(nk_ctx *ctx, int64_t n, const double *x, const double *v, double *xc, double *tc, int32_t *fc) {
    NK_ARG(ctx && ctx->have_mesh && ctx->have_sv && n > 0 && x && v, "nk_find_boundary: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    NK_BUF(double, dx, x, n * 3); NK_BUF(double, dv, v, n * 3);
    NK_BUF(double, dxc, nullptr, n * 3); NK_BUF(double, dtc, nullptr, n); NK_BUF(int32_t, dfc, nullptr, n);
    const bool verbose = getenv("NK_VERBOSE") != nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (verbose) { NK_HIP(hipEventCreate(&e0)); NK_HIP(hipEventCreate(&e1)); NK_HIP(hipEventRecord(e0, ctx->stream)); }
    NK_GEOM_LAUNCH(k_tap_find_boundary, (int)((n + NK_WG - 1) / NK_WG), nk_lds(ctx, true), d, n, dx.p, dv.p, dxc.p, dtc.p, dfc.p);
    NK_HIP(hipGetLastError());
    if (verbose) NK_HIP(hipEventRecord(e1, ctx->stream));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    if (verbose) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        fprintf(stderr, "[nanokappa_hip] find_boundary: %lld rays in %.3f ms\n", (long long)n, ms);
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
    NK_HIP(dxc.get(xc, n * 3)); NK_HIP(dtc.get(tc, n)); NK_HIP(dfc.get(fc, n));
    return NK_OK;
}
int nk_find_boundary_from(nk_ctx *ctx, int64_t n, const double *x, const double *v, const int32_t *from_facet, double *xc, double *tc,
                          int32_t *fc, int32_t *skipped) {
    NK_ARG(ctx && ctx->have_mesh && ctx->have_sv && n > 0 && x && v && from_facet, "nk_find_boundary_from: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    NK_BUF(double, dx, x, n * 3); NK_BUF(double, dv, v, n * 3); NK_BUF(int32_t, dff, from_facet, n);
    NK_BUF(double, dxc, nullptr, n * 3); NK_BUF(double, dtc, nullptr, n); NK_BUF(int32_t, dfc, nullptr, n); NK_BUF(int32_t, dsk, nullptr, n);
    NK_GEOM_LAUNCH(k_tap_find_boundary_from, (int)((n + NK_WG - 1) / NK_WG), nk_lds(ctx, true), d, n, dx.p, dv.p, dff.p, dxc.p, dtc.p, dfc.p, dsk.p);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_HIP(dxc.get(xc, n * 3)); NK_HIP(dtc.get(tc, n)); NK_HIP(dfc.get(fc, n)); NK_HIP(dsk.get(skipped, n));
    return NK_OK;
}
// The face tree as nk_set_mesh left it on the device, read back: nothing is kept on the host but NkDev's few numbers, so the counts
// are taken from the leaf records themselves (a padding slot is a face box no ray enters, lo > hi).
int nk_tree_info(nk_ctx *ctx, nk_tree_report *out, float *family_boxes, float *leaf_boxes) {
    NK_ARG(ctx && out && ctx->have_mesh, "nk_tree_info: no mesh");
    memset(out, 0, sizeof(*out));
    const NkDev &d = ctx->d;
    out->NG = d.NG;
    if (d.NG == 0) return NK_OK;
    NK_HIP(hipSetDevice(ctx->device));
    out->tree_top = d.tree_top;
    out->tree_leaves = d.tree_leaves;
    out->tree_bound = d.tree_bound;
    out->n_families = d.tree_nfam;
    int count = d.tree_leaves;
    for (int l = 0; l <= d.tree_top && l < NK_TREE_LEVELS; ++l) {
        out->level_nodes[l] = count;
        out->tree_base[l] = d.tree_base[l];
        if (l == d.tree_top) out->top_family = count;
        count = (count + 3) / 4;
    }
    std::vector<double> tf((size_t)d.tree_leaves * NK_TREE_LEAF_DOUBLES);
    NK_HIP(hipMemcpy(tf.data(), d.tree_faces, tf.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int leaf = 0; leaf < d.tree_leaves; ++leaf) {
        float fb[24];
        memcpy(fb, &tf[(size_t)leaf * NK_TREE_LEAF_DOUBLES], sizeof(fb));
        for (int c = 0; c < 4; ++c) {
            if (fb[6 * c] > fb[6 * c + 3]) ++out->pad_slots; else ++out->references;
        }
        if (leaf_boxes) memcpy(leaf_boxes + (size_t)leaf * 24, fb, sizeof(fb));
    }
    if (family_boxes)
        NK_HIP(hipMemcpy(family_boxes, d.tree_boxes, (size_t)d.tree_nfam * NK_TREE_FAMILY_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
    return NK_OK;
}
int nk_classify(nk_ctx *ctx, int64_t n, const double *x, int32_t *id) {
    NK_ARG(ctx && ctx->have_sv && n > 0 && x && id, "nk_classify: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_BUF(double, dx, x, n * 3); NK_BUF(int32_t, did, nullptr, n);
    k_tap_classify<<<(int)((n + NK_WG - 1) / NK_WG), NK_WG, nk_lds(ctx, false), ctx->stream>>>(ctx->d, n, dx.p, did.p);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_HIP(did.get(id, n));
    return NK_OK;
}
int nk_box_hit(nk_ctx *ctx, int32_t which, int64_t n, const double *x, const double *v, double *t, int32_t *facet) {
    NK_ARG(ctx && ctx->have_mesh && n > 0 && x && v && t && facet && which >= 0 && which <= 2, "nk_box_hit: bad arguments");
    NK_ARG(ctx->mesh_box, "nk_box_hit: the mesh is not a box (six axis-aligned walls, one facet each)");
    NK_HIP(hipSetDevice(ctx->device));
    NK_BUF(double, dx, x, n * 3); NK_BUF(double, dv, v, n * 3);
    NK_BUF(double, dt, nullptr, n); NK_BUF(int32_t, df, nullptr, n);
    k_tap_box_hit<<<(int)((n + NK_WG - 1) / NK_WG), NK_WG, 0, ctx->stream>>>(ctx->d, which, n, dx.p, dv.p, dt.p, df.p);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_HIP(dt.get(t, n)); NK_HIP(df.get(facet, n));
    return NK_OK;
}
int nk_eval(nk_ctx *ctx, int32_t what, int64_t n, const double *a, const int32_t *mode, double *out) {
    NK_ARG(ctx && ctx->have_material && n > 0 && a && out && what >= 0 && what <= 8, "nk_eval: bad arguments");
    NK_ARG((what > 1 && what != 8) || mode, "nk_eval: mode required");
    NK_ARG(ctx->have_sv, "nk_eval: subvolumes required");
    if (mode) for (int64_t i = 0; i < n; ++i) NK_ARG(mode[i] >= 0 && mode[i] < ctx->d.M, "nk_eval: mode index out of range");
    NK_HIP(hipSetDevice(ctx->device));
    const int64_t na = what == 4 ? 3 * n : (what == 8 ? 4 * n : n);
    NK_BUF(double, da, a, na); NK_BUF(int32_t, dm, mode, n); NK_BUF(double, dout, nullptr, n);
    k_tap_eval<<<(int)((n + NK_WG - 1) / NK_WG), NK_WG, nk_lds(ctx, false), ctx->stream>>>(ctx->d, what, n, da.p, mode ? dm.p : nullptr, dout.p);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_HIP(dout.get(out, n));
    return NK_OK;
}
int nk_mode_segments(nk_ctx *ctx, int32_t *seg, int32_t *nseg) {
    NK_ARG(ctx && seg && nseg, "nk_mode_segments: NULL argument");
    const NkDev &d = ctx->d;
    NK_ARG(d.cap > 0 && d.part && ctx->map_nseg == d.nseg && ctx->h_m2s.size() == (size_t)d.M, "nk_mode_segments: no particle store with partitioned modes");
    for (int m = 0; m < d.M; ++m) seg[m] = nk_mode_seg(ctx, m, d.nseg);
    *nseg = d.nseg;
    return NK_OK;
}
int nk_reflect(nk_ctx *ctx, int64_t n, const int32_t *facet, const int32_t *mode_in, const double *col_pos,
               const double *n_in, const double *omega_in, const double *r_spec, const double *r_deg,
               const double *r_diff, int32_t *mode_out, double *n_out, double *omega_out) {
    NK_ARG(ctx && ctx->have_material && ctx->have_sv && ctx->have_mesh && ctx->d.Fr > 0 && n > 0, "nk_reflect: engine not configured");
    NK_ARG(facet && mode_in && col_pos && n_in && omega_in && r_spec && r_diff, "nk_reflect: NULL input");
    for (int64_t i = 0; i < n; ++i)
        NK_ARG(facet[i] >= 0 && facet[i] < ctx->d.Fc && ctx->host_facets[facet[i]].rough >= 0, "nk_reflect: facet is not rough");
    NK_HIP(hipSetDevice(ctx->device));
    NK_BUF(int32_t, df, facet, n); NK_BUF(int32_t, dm, mode_in, n); NK_BUF(double, dc, col_pos, n * 3);
    NK_BUF(double, dn, n_in, n); NK_BUF(double, dom, omega_in, n); NK_BUF(double, drs, r_spec, n);
    NK_BUF(double, drd, r_deg, n); NK_BUF(double, drf, r_diff, n);
    NK_BUF(int32_t, dmo, nullptr, n); NK_BUF(double, dno, nullptr, n); NK_BUF(double, doo, nullptr, n);
    k_tap_reflect<<<(int)((n + NK_WG - 1) / NK_WG), NK_WG, nk_lds(ctx, false), ctx->stream>>>(
        ctx->d, n, df.p, dm.p, dc.p, dn.p, dom.p, drs.p, r_deg ? drd.p : nullptr, drf.p, dmo.p, dno.p, doo.p);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_HIP(dmo.get(mode_out, n)); NK_HIP(dno.get(n_out, n)); NK_HIP(doo.get(omega_out, n));
    return NK_OK;
}
int nk_calibrate_stream(nk_ctx *ctx, int32_t launches, int64_t *bytes_read, int64_t *bytes_written) {
    NK_ARG(ctx && launches > 0 && ctx->d.cap > 0, "nk_calibrate_stream: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NkHostParticles h;
    NK_TRY(nk_gather_live(ctx, h, false));
    const int64_t ns = (int64_t)h.x.size();
    for (int k = 0; k < launches; ++k) k_cal_stream<<<nk_sweep_grid(ctx), NK_WG, 0, ctx->stream>>>(ctx->d);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    if (const char *pc = getenv("NK_PROBE_COPY")) {      // developer probe: copy floor of the sweep's wave structure
        hipEvent_t e0, e1;
        NK_HIP(hipEventCreate(&e0)); NK_HIP(hipEventCreate(&e1));
        const int g = ctx->g_sweep > 0 ? ctx->g_sweep : ctx->num_cu * 3;
        for (int w = 8; w <= 16; w += 8) {
            if (atoi(pc) != w && atoi(pc) != 0) continue;
            for (int rep = 0; rep < 3; ++rep) {
                NK_HIP(hipEventRecord(e0, ctx->stream));
                for (int k = 0; k < 10; ++k) { if (w == 8) k_probe_copy<8><<<g, NK_WG, 0, ctx->stream>>>(ctx->d); else k_probe_copy<16><<<g, NK_WG, 0, ctx->stream>>>(ctx->d); }
                NK_HIP(hipEventRecord(e1, ctx->stream));
                NK_HIP(hipStreamSynchronize(ctx->stream));
                float ms = 0.f;
                hipEventElapsedTime(&ms, e0, e1);
                fprintf(stderr, "[nanokappa_hip] copy probe, %d-byte accesses: %.1f us per pass over %lld particles (%.2f TB/s)\n", w, 100.0 * ms,
                        (long long)ns, (ctx->d.nts ? 88.0 : 72.0) * ns / (ms * 1e-4) / 1e12);
            }
        }
        hipEventDestroy(e0); hipEventDestroy(e1);
    }
    if (bytes_read) *bytes_read = ns * (ctx->d.nts ? 44 : 36);
    if (bytes_written) *bytes_written = ns * (ctx->d.nts ? 32 : 24);
    return NK_OK;
}
int nk_uniform2(uint64_t seed, uint64_t pid, uint32_t step, uint32_t tag, double *u0, double *u1) {
    if (!u0 || !u1) return NK_ERR_ARG;
    double *dout = nullptr, h[2];
    if (hipMalloc((void **)&dout, 16) != hipSuccess) return NK_ERR_HIP;
    k_tap_uniform<<<1, 1>>>(seed, pid, step, tag, dout);
    if (hipMemcpy(h, dout, 16, hipMemcpyDeviceToHost) != hipSuccess) { hipFree(dout); return NK_ERR_HIP; }
    hipFree(dout);
    *u0 = h[0]; *u1 = h[1];
    return NK_OK;
}

}  // extern "C"


// ------------------------------------------------------------------------------ set-up table builder
static void nk_specular_free(nk_ctx *ctx) {
    for (void *p : {(void *)ctx->spec_v, (void *)ctx->spec_om, (void *)ctx->spec_dl, (void *)ctx->spec_modes,
                    (void *)ctx->spec_in, (void *)ctx->spec_out, (void *)ctx->spec_count, (void *)ctx->spec_svx,
                    (void *)ctx->spec_rank, (void *)ctx->ks_kv, (void *)ctx->ks_mat})
        if (p) hipFree(p);
    ctx->ks_kv = ctx->ks_mat = nullptr; ctx->ks_Q = 0;
    ctx->spec_v = ctx->spec_om = ctx->spec_dl = ctx->spec_svx = nullptr;
    ctx->spec_rank = nullptr;
    ctx->spec_modes = nullptr; ctx->spec_in = ctx->spec_out = nullptr; ctx->spec_count = nullptr;
    ctx->spec_M = 0; ctx->spec_cap = 0;
}
int nk_specular_begin(nk_ctx *ctx, int64_t M, const double *group_vel, const double *omega, const double *delta_omega) {
    NK_ARG(ctx && M > 0 && M < (1ll << 31) && group_vel && omega && delta_omega, "nk_specular_begin: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    nk_specular_free(ctx);
    NK_HIP(hipMalloc((void **)&ctx->spec_v, (size_t)M * 24));
    NK_HIP(hipMalloc((void **)&ctx->spec_om, (size_t)M * 8));
    NK_HIP(hipMalloc((void **)&ctx->spec_dl, (size_t)M * 8));
    NK_HIP(hipMalloc((void **)&ctx->spec_modes, (size_t)M * sizeof(NkSpecMode)));
    NK_HIP(hipMalloc((void **)&ctx->spec_count, 8));
    NK_HIP(hipMemcpy(ctx->spec_v, group_vel, (size_t)M * 24, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->spec_om, omega, (size_t)M * 8, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->spec_dl, delta_omega, (size_t)M * 8, hipMemcpyHostToDevice));
    // order of the x-velocities (the pair search only scans a window of it), rank of every mode in it, largest |v|
    std::vector<int32_t> order((size_t)M), rank((size_t)M);
    for (int64_t m = 0; m < M; ++m) order[(size_t)m] = (int32_t)m;
    std::stable_sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return group_vel[3 * (size_t)p] < group_vel[3 * (size_t)q]; });
    std::vector<double> svx((size_t)M);
    double vmax = 0.0;
    for (int64_t k = 0; k < M; ++k) {
        const size_t m = (size_t)order[(size_t)k];
        rank[m] = (int32_t)k;
        svx[(size_t)k] = group_vel[3 * m];
        const double vx = group_vel[3 * m], vy = group_vel[3 * m + 1], vz = group_vel[3 * m + 2];
        vmax = std::max(vmax, sqrt((vx * vx + vy * vy) + vz * vz));
    }
    NK_HIP(hipMalloc((void **)&ctx->spec_rank, (size_t)M * 4));
    NK_HIP(hipMalloc((void **)&ctx->spec_svx, (size_t)M * 8));
    NK_HIP(hipMemcpy(ctx->spec_rank, rank.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->spec_svx, svx.data(), (size_t)M * 8, hipMemcpyHostToDevice));
    ctx->spec_vmax = vmax;
    ctx->spec_M = M;
    return NK_OK;
}
int nk_specular_pairs(nk_ctx *ctx, const double *normal, double crit, int64_t cap, int32_t *pair_in, int32_t *pair_out,
                      int64_t *n_pairs) {
    NK_ARG(ctx && normal && n_pairs && cap >= 0 && ((pair_in != nullptr) == (pair_out != nullptr)), "nk_specular_pairs: bad arguments");
    NK_ARG(ctx->spec_M > 0, "nk_specular_pairs: call nk_specular_begin first");
    NK_HIP(hipSetDevice(ctx->device));
    const int M = (int)ctx->spec_M;
    if (cap > ctx->spec_cap) {
        if (ctx->spec_in) hipFree(ctx->spec_in);
        if (ctx->spec_out) hipFree(ctx->spec_out);
        ctx->spec_in = ctx->spec_out = nullptr;
        NK_HIP(hipMalloc((void **)&ctx->spec_in, (size_t)cap * 4));
        NK_HIP(hipMalloc((void **)&ctx->spec_out, (size_t)cap * 4));
        ctx->spec_cap = cap;
    }
    const int blocks = (M + NK_WG - 1) / NK_WG;
    NK_HIP(hipMemsetAsync(ctx->spec_count, 0, 8, ctx->stream));
    k_specular_prepare<<<blocks, NK_WG, 0, ctx->stream>>>(M, ctx->spec_v, ctx->spec_om, ctx->spec_dl, ctx->spec_rank, normal[0],
                                                          normal[1], normal[2], ctx->spec_modes);
    k_specular_pairs<<<blocks, NK_WG, 0, ctx->stream>>>(M, ctx->spec_modes, ctx->spec_svx, ctx->spec_vmax, normal[0], normal[1],
                                                        normal[2], crit, cap, ctx->spec_in, ctx->spec_out, ctx->spec_count);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    unsigned long long n = 0;
    NK_HIP(hipMemcpy(&n, ctx->spec_count, 8, hipMemcpyDeviceToHost));
    *n_pairs = (int64_t)n;
    const int64_t got = (int64_t)n < cap ? (int64_t)n : cap;
    ctx->spec_last = (int64_t)n <= cap ? (int64_t)n : -1;      // -1: truncated, the caller asks again with more room
    if (got > 0 && pair_in) {                          // (NULL arrays: the pairs stay on the device for nk_rough_pairs)
        NK_HIP(hipMemcpy(pair_in, ctx->spec_in, (size_t)got * 4, hipMemcpyDeviceToHost));
        NK_HIP(hipMemcpy(pair_out, ctx->spec_out, (size_t)got * 4, hipMemcpyDeviceToHost));
    }
    return NK_OK;
}
// 'k' / wavevector model (Population.py:1056-1240): the same calls as the 'velocity' search, between nk_specular_begin and
// nk_specular_end; the pairs land where nk_rough_pairs expects them.
int nk_kspec_begin(nk_ctx *ctx, int64_t Q, const double *wavevectors, const double *k_to_q, const double *q_to_k, const double *tol) {
    NK_ARG(ctx && Q > 0 && wavevectors && k_to_q && q_to_k && tol, "nk_kspec_begin: bad arguments");
    NK_ARG(ctx->spec_M > 0 && ctx->spec_M % Q == 0, "nk_kspec_begin: call nk_specular_begin first (M = Q x J modes)");
    NK_HIP(hipSetDevice(ctx->device));
    if (ctx->ks_kv) hipFree(ctx->ks_kv);
    if (ctx->ks_mat) hipFree(ctx->ks_mat);
    ctx->ks_kv = ctx->ks_mat = nullptr;
    NK_HIP(hipMalloc((void **)&ctx->ks_kv, (size_t)Q * 24));
    NK_HIP(hipMalloc((void **)&ctx->ks_mat, 18 * 8));
    NK_HIP(hipMemcpy(ctx->ks_kv, wavevectors, (size_t)Q * 24, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->ks_mat, k_to_q, 72, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->ks_mat + 9, q_to_k, 72, hipMemcpyHostToDevice));
    for (int c = 0; c < 3; ++c) ctx->ks_tol[c] = tol[c];
    ctx->ks_Q = Q;
    return NK_OK;
}
int nk_kspec_pairs(nk_ctx *ctx, const double *normal, int64_t cap, int32_t *pair_in, int32_t *pair_out, int64_t *n_pairs) {
    NK_ARG(ctx && normal && n_pairs && cap >= 0 && ((pair_in != nullptr) == (pair_out != nullptr)), "nk_kspec_pairs: bad arguments");
    NK_ARG(ctx->ks_Q > 0 && ctx->spec_M > 0, "nk_kspec_pairs: call nk_specular_begin and nk_kspec_begin first");
    NK_HIP(hipSetDevice(ctx->device));
    const int Q = (int)ctx->ks_Q, J = (int)(ctx->spec_M / ctx->ks_Q);
    if (cap > ctx->spec_cap) {
        if (ctx->spec_in) hipFree(ctx->spec_in);
        if (ctx->spec_out) hipFree(ctx->spec_out);
        ctx->spec_in = ctx->spec_out = nullptr;
        NK_HIP(hipMalloc((void **)&ctx->spec_in, (size_t)cap * 4));
        NK_HIP(hipMalloc((void **)&ctx->spec_out, (size_t)cap * 4));
        ctx->spec_cap = cap;
    }
    NK_HIP(hipMemsetAsync(ctx->spec_count, 0, 8, ctx->stream));
    k_kspec_pairs<<<(Q + NK_WG - 1) / NK_WG, NK_WG, 0, ctx->stream>>>(Q, J, ctx->spec_v, ctx->spec_om, ctx->ks_kv, ctx->ks_mat, ctx->ks_mat + 9,
                                                                      ctx->ks_tol[0], ctx->ks_tol[1], ctx->ks_tol[2], normal[0], normal[1], normal[2],
                                                                      cap, ctx->spec_in, ctx->spec_out, ctx->spec_count);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    unsigned long long n = 0;
    NK_HIP(hipMemcpy(&n, ctx->spec_count, 8, hipMemcpyDeviceToHost));
    *n_pairs = (int64_t)n;
    const int64_t got = (int64_t)n < cap ? (int64_t)n : cap;
    ctx->spec_last = (int64_t)n <= cap ? (int64_t)n : -1;
    if (got > 0 && pair_in) {
        NK_HIP(hipMemcpy(pair_in, ctx->spec_in, (size_t)got * 4, hipMemcpyDeviceToHost));
        NK_HIP(hipMemcpy(pair_out, ctx->spec_out, (size_t)got * 4, hipMemcpyDeviceToHost));
    }
    return NK_OK;
}
int nk_specular_end(nk_ctx *ctx) {
    NK_ARG(ctx, "nk_specular_end: NULL context");
    NK_HIP(hipSetDevice(ctx->device));
    nk_specular_free(ctx);
    return NK_OK;
}

// ---- the rough-facet tables built on the device (header: nk_rough_begin / nk_rough_pairs / nk_rough_finish)
static void nk_rough_build_free(nk_ctx *ctx, bool tables) {
    for (void *p : {(void *)ctx->rb_k2, (void *)ctx->rb_nin, (void *)ctx->rb_eta, (void *)ctx->rb_sub}) if (p) hipFree(p);
    ctx->rb_k2 = ctx->rb_nin = ctx->rb_eta = ctx->rb_sub = nullptr;
    if (tables) {
        for (void *p : {(void *)ctx->rb_spec, (void *)ctx->rb_roul, (void *)ctx->rb_ts, (void *)ctx->rb_map}) if (p) hipFree(p);
        ctx->rb_spec = ctx->rb_roul = nullptr; ctx->rb_ts = nullptr; ctx->rb_map = nullptr;
    }
}
int nk_rough_begin(nk_ctx *ctx, int32_t Fr, const int32_t *facet, const double *normal_in, const double *eta, const double *k_norm) {
    NK_ARG(ctx && Fr > 0 && facet && normal_in && eta && k_norm, "nk_rough_begin: bad arguments");
    NK_ARG(ctx->have_material && ctx->have_mesh, "nk_rough_begin: set material and mesh first");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    nk_rough_build_free(ctx, true);
    for (int i = 0; i < Fr; ++i) NK_ARG(facet[i] >= 0 && facet[i] < d.Fc, "nk_rough_begin: facet index");
    const size_t n = (size_t)Fr * d.M;
    std::vector<double> k2((size_t)d.Q);
    for (int q = 0; q < d.Q; ++q) k2[(size_t)q] = k_norm[q] * k_norm[q];
    NK_HIP(hipMalloc((void **)&ctx->rb_k2, (size_t)d.Q * 8));
    NK_HIP(hipMalloc((void **)&ctx->rb_nin, (size_t)Fr * 24));
    NK_HIP(hipMalloc((void **)&ctx->rb_eta, (size_t)Fr * 8));
    NK_HIP(hipMalloc((void **)&ctx->rb_sub, n * 8));
    NK_HIP(hipMalloc((void **)&ctx->rb_spec, n * 8));
    NK_HIP(hipMalloc((void **)&ctx->rb_roul, n * 8));
    NK_HIP(hipMalloc((void **)&ctx->rb_ts, n));
    NK_HIP(hipMalloc((void **)&ctx->rb_map, n * 4));
    NK_HIP(hipMemcpy(ctx->rb_k2, k2.data(), (size_t)d.Q * 8, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->rb_nin, normal_in, (size_t)Fr * 24, hipMemcpyHostToDevice));
    NK_HIP(hipMemcpy(ctx->rb_eta, eta, (size_t)Fr * 8, hipMemcpyHostToDevice));
    NK_HIP(hipMemsetAsync(ctx->rb_sub, 0, n * 8, ctx->stream));
    NK_HIP(hipMemsetAsync(ctx->rb_ts, 0, n, ctx->stream));
    k_fill_u32<<<(int)((n + 255) / 256), 256, 0, ctx->stream>>>(ctx->rb_map, (int64_t)n, 0xFFFFFFFFu);
    NK_HIP(hipGetLastError());
    ctx->rb_Fr = Fr;
    ctx->rb_facet.assign(facet, facet + Fr);
    return NK_OK;
}
int nk_rough_pairs(nk_ctx *ctx, int32_t nf, const int32_t *fidx) {
    NK_ARG(ctx && nf > 0 && fidx && ctx->rb_Fr > 0, "nk_rough_pairs: call nk_rough_begin first");
    NK_ARG(ctx->spec_last >= 0, "nk_rough_pairs: the last nk_specular_pairs call was truncated");
    for (int i = 0; i < nf; ++i) NK_ARG(fidx[i] >= 0 && fidx[i] < ctx->rb_Fr, "nk_rough_pairs: rough-facet index");
    if (ctx->spec_last == 0) return NK_OK;
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    NK_BUF(int32_t, df, fidx, nf);
    k_rough_pairs<<<(int)((ctx->spec_last + NK_WG - 1) / NK_WG), NK_WG, 0, ctx->stream>>>(d.M, d.J, ctx->spec_v, ctx->rb_k2, ctx->spec_last,
                                                                                         ctx->spec_in, ctx->spec_out, nf, df.p, ctx->rb_nin,
                                                                                         ctx->rb_eta, ctx->rb_ts, ctx->rb_map, ctx->rb_sub);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    return NK_OK;
}
int nk_rough_finish(nk_ctx *ctx) { return nk_rough_finish_k(ctx, 0, nullptr, nullptr); }
// the same with the 'k' model's degenerate branches (find_degeneracies, Population.py:1017-1040: rows q, j1, j2): their
// creation rates are averaged (:926-930) and the reflection flips a coin between them (:963-969; degen_j2 [M] as in nk_rough)
int nk_rough_finish_k(nk_ctx *ctx, int32_t nd, const int32_t *degen, const int32_t *degen_j2) {
    NK_ARG(ctx && ctx->rb_Fr > 0 && ctx->spec_v, "nk_rough_finish: call nk_rough_begin (inside nk_specular_begin .. end) first");
    NK_ARG(nd >= 0 && (nd == 0 || degen), "nk_rough_finish_k: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    const int Fr = ctx->rb_Fr;
    const size_t n = (size_t)Fr * d.M;
    k_rough_finish<<<(int)((n + NK_WG - 1) / NK_WG), NK_WG, 0, ctx->stream>>>(Fr, d.M, d.J, ctx->spec_v, ctx->rb_k2, ctx->rb_nin, ctx->rb_eta,
                                                                              ctx->rb_ts, (int32_t *)ctx->rb_map, ctx->rb_sub, ctx->rb_spec,
                                                                              ctx->rb_roul, nd == 0 ? 1 : 0);
    const int32_t *dj2 = nullptr;
    if (nd > 0) {
        for (int i = 0; i < nd; ++i)
            NK_ARG(degen[3 * i] >= 0 && degen[3 * i] < d.M / d.J && degen[3 * i + 1] >= 0 && degen[3 * i + 1] < d.J && degen[3 * i + 2] >= 0 &&
                       degen[3 * i + 2] < d.J, "nk_rough_finish_k: degeneracy row out of range");
        NK_BUF(int32_t, dg, degen, (int64_t)nd * 3);
        k_rough_degen<<<(Fr + 63) / 64, 64, 0, ctx->stream>>>(Fr, d.M, d.J, nd, dg.p, ctx->rb_roul);
        k_rough_round<<<(int)((n + NK_WG - 1) / NK_WG), NK_WG, 0, ctx->stream>>>((int64_t)n, ctx->rb_roul);
        NK_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (degen_j2) NK_UP(degen_j2, (size_t)d.M, &dj2);
    k_rough_cumsum<<<Fr, 64, 0, ctx->stream>>>(d.M, ctx->rb_roul);
    int nlut = 1024;
    while (nlut < 65536 && (int64_t)nlut * 4 < d.M) nlut *= 2;
    int32_t *lut = nullptr;
    NK_HIP(hipMalloc((void **)&lut, (size_t)Fr * (nlut + 1) * 4));
    ctx->allocs.push_back(lut);
    k_rough_lut<<<(int)(((size_t)Fr * (nlut + 1) + NK_WG - 1) / NK_WG), NK_WG, 0, ctx->stream>>>(Fr, d.M, nlut, ctx->rb_roul, lut);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    // install, as nk_set_rough does (the tables now belong to the context)
    d.Fr = Fr;
    ctx->g_sweep = 0;
    d.specularity = ctx->rb_spec; d.true_spec = ctx->rb_ts; d.spec_map = (const int32_t *)ctx->rb_map; d.roulette = ctx->rb_roul;
    d.roul_lut = lut; d.roul_nlut = nlut; d.degen_j2 = dj2;
    for (void *p : {(void *)ctx->rb_spec, (void *)ctx->rb_roul, (void *)ctx->rb_ts, (void *)ctx->rb_map}) ctx->allocs.push_back(p);
    ctx->rb_spec = ctx->rb_roul = nullptr; ctx->rb_ts = nullptr; ctx->rb_map = nullptr;
    nk_rough_build_free(ctx, false);
    for (int i = 0; i < Fr; ++i) ctx->host_facets[ctx->rb_facet[(size_t)i]].rough = i;
    ctx->rb_Fr = 0;
    return nk_patch_facets(ctx);
}
int nk_rough_download(nk_ctx *ctx, double *specularity, uint8_t *true_spec, int32_t *spec_map, double *roulette) {
    NK_ARG(ctx && ctx->d.Fr > 0, "nk_rough_download: no rough tables");
    NK_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->d.Fr * ctx->d.M;
    if (specularity) NK_HIP(hipMemcpy(specularity, ctx->d.specularity, n * 8, hipMemcpyDeviceToHost));
    if (true_spec) NK_HIP(hipMemcpy(true_spec, ctx->d.true_spec, n, hipMemcpyDeviceToHost));
    if (spec_map) NK_HIP(hipMemcpy(spec_map, ctx->d.spec_map, n * 4, hipMemcpyDeviceToHost));
    if (roulette) NK_HIP(hipMemcpy(roulette, ctx->d.roulette, n * 8, hipMemcpyDeviceToHost));
    return NK_OK;
}
int nk_build_enter_prob(nk_ctx *ctx, int32_t R, const double *normal_in, const double *thickness, double dt, double *out) {
    NK_ARG(ctx && R > 0 && normal_in && thickness && out && ctx->have_material, "nk_build_enter_prob: bad arguments");
    NK_HIP(hipSetDevice(ctx->device));
    NkDev &d = ctx->d;
    const size_t n = (size_t)R * d.M;
    NK_BUF(double, dn, normal_in, (int64_t)R * 3); NK_BUF(double, dth, thickness, R); NK_BUF(double, dout, nullptr, (int64_t)n);
    k_enter_prob<<<(int)((n + NK_WG - 1) / NK_WG), NK_WG, 0, ctx->stream>>>(R, d.M, ctx->d_vg, dn.p, dth.p, dt, dout.p);
    NK_HIP(hipGetLastError());
    NK_HIP(hipStreamSynchronize(ctx->stream));
    NK_HIP(dout.get(out, (int64_t)n));
    return NK_OK;
}

// ------------------------------------------------------------------------------------- free-path sampling
// What nk_free_paths, nk_free_paths_columns and nk_free_paths_map share.  A call weighs its rays with K lifetime tables: K = 1
// for the plain call and the map, the leading axis of tau, of the rows and of the per-ray outputs (but x0) for the columns.

// The refusals, in the words of the entry point `who`; tau_holds: what its message says a->tau is, K its tables.  Sets the list's
// length and the ray count.  A lifetime lives when it is positive, and then it must be finite (W tau g with tau = inf is inf 0);
// the start points must be finite: neither reaches a kernel.
static int nk_free_refuse(nk_ctx *ctx, const std::string &who, const nk_free_path_args *a, const char *tau_holds, int64_t K, int64_t &nlist, int64_t &rays) {
    NK_ARG(ctx->have_material, who + ": no material (nk_set_material first)");
    NK_ARG(ctx->have_mesh, who + ": no mesh (nk_set_mesh first)");
    const NkDev &d = ctx->d;
    NK_ARG(a->tau, who + ": tau is NULL (" + tau_holds + ")");
    NK_ARG(a->n_samples > 0, who + ": n_samples = " + std::to_string(a->n_samples) + " must be positive");
    NK_ARG(a->max_segments >= 0 && a->w_min >= 0.0, who + ": max_segments and w_min must not be negative");
    nlist = a->modes ? (int64_t)a->n_modes : (int64_t)d.M;
    NK_ARG(nlist >= 0, who + ": n_modes must not be negative");
    if (a->modes)
        for (int64_t i = 0; i < nlist; ++i)
            NK_ARG(a->modes[i] >= 0 && a->modes[i] < d.M, who + ": mode " + std::to_string(a->modes[i]) + " (entry " + std::to_string((long long)i) +
                                                              " of the list) is out of range [0, " + std::to_string(d.M) + ")");
    for (int fc = 0; fc < d.Fc; ++fc)
        NK_ARG(ctx->host_facets[fc].bc != 'R' || (ctx->host_facets[fc].rough >= 0 && ctx->host_facets[fc].rough < d.Fr && d.specularity),
               who + ": facet " + std::to_string(fc) + " is rough ('R') but no rough tables are installed (nk_set_rough or nk_rough_finish)");
    NK_ARG(a->x0 || d.nS > 0, who + ": no start points (x0) and the mesh was set without its volume tables (simplices)");
    rays = nlist * (int64_t)a->n_samples;
    NK_ARG(rays < (1ll << 31), who + ": " + std::to_string((long long)rays) + " rays are more than one call takes (2^31)");
    for (int64_t i = 0; i < K * (int64_t)d.M; ++i)
        NK_ARG(!(a->tau[i] > 0.0) || std::isfinite(a->tau[i]), who + ": tau of mode " + std::to_string((long long)(i % d.M)) + " is not finite" +
                                                                   (K > 1 ? " (column " + std::to_string((long long)(i / d.M)) + ")" : std::string()));
    if (a->x0)
        for (int64_t i = 0; i < rays * 3; ++i)
            NK_ARG(std::isfinite(a->x0[i]), who + ": x0 of list entry " + std::to_string((long long)(i / 3 / a->n_samples)) + ", sample " +
                                                std::to_string((long long)(i / 3 % a->n_samples)) + " is not finite");
    return NK_OK;
}

// The buffers of a call -- everything nk_free_path_args and nk_free_path_rays imply --, freed on every return path.
struct NkFreeCall {
    const nk_free_path_args *a;
    const nk_free_path_rays *pr;     // null when no per-ray output is asked for
    int64_t K, M, nlist, rays;
    NkDevBuf<int32_t> modes;
    NkDevBuf<double> tau, x0, rows;
    NkDevBuf<unsigned long long> cnt;
    NkDevBuf<double> rD, rT, rx;
    NkDevBuf<int32_t> rs, re;
    NkFreeCall(const nk_ctx *ctx, const nk_free_path_args *a_, const nk_free_path_rays *p, int64_t K_, int64_t nlist_, int64_t rays_)
        : a(a_), pr(p && (p->D || p->T || p->segments || p->end || p->x0) ? p : nullptr), K(K_), M(ctx->d.M), nlist(nlist_), rays(rays_),
          modes(a->modes, a->modes ? nlist : 0), tau(a->tau, K * M), x0(a->x0, a->x0 ? rays * 3 : 0),
          rows(nullptr, K * nlist * NK_FP_ROW), cnt(nullptr, K * nlist * NK_FP_CNT),
          rD(nullptr, (pr && pr->D) ? K * rays * 3 : 0), rT(nullptr, (pr && pr->T) ? K * rays : 0), rx(nullptr, (pr && pr->x0) ? rays * 3 : 0),
          rs(nullptr, (pr && pr->segments) ? K * rays : 0), re(nullptr, (pr && pr->end) ? K * rays : 0) {}
    hipError_t err() const {
        for (hipError_t e : {modes.err, tau.err, x0.err, rows.err, cnt.err, rD.err, rT.err, rx.err, rs.err, re.err})
            if (e != hipSuccess) return e;
        return hipSuccess;
    }
    // the kernels' record, with the defaults of the arguments
    NkFreeDev dev(const nk_ctx *ctx) const {
        NkFreeDev f;
        f.modes = a->modes ? modes.p : nullptr;
        f.nlist = (int32_t)nlist; f.n = a->n_samples;
        f.max_segments = a->max_segments > 0 ? a->max_segments : 65536;
        f.w_min = a->w_min > 0.0 ? a->w_min : ldexp(1.0, -40);
        f.tau = tau.p; f.vg = ctx->d_vg; f.x0 = a->x0 ? x0.p : nullptr;
        f.seed = a->seed ? a->seed : ctx->d.seed;
        f.rows = rows.p; f.counts = cnt.p;
        f.ray_D = (pr && pr->D) ? rD.p : nullptr; f.ray_T = (pr && pr->T) ? rT.p : nullptr;
        f.ray_x0 = (pr && pr->x0) ? rx.p : nullptr;
        f.ray_seg = (pr && pr->segments) ? rs.p : nullptr; f.ray_end = (pr && pr->end) ? re.p : nullptr;
        return f;
    }
    // bytes of these buffers as the reports count them
    int64_t bytes() const {
        return (a->modes ? nlist * 4 : 0) + K * M * 8 + (a->x0 ? rays * 24 : 0) + K * nlist * (NK_FP_ROW + NK_FP_CNT) * 8 +
               ((pr && pr->D) ? K * rays * 24 : 0) + ((pr && pr->T) ? K * rays * 8 : 0) + ((pr && pr->x0) ? rays * 24 : 0) +
               ((pr && pr->segments) ? K * rays * 4 : 0) + ((pr && pr->end) ? K * rays * 4 : 0);
    }
    // the rows into pm (with the column axis), the counts into casts, missed, capped [K], the per-ray outputs into pr
    int copy_out(nk_ctx *ctx, const nk_free_path_modes *pm, int64_t *casts, int64_t *missed, int64_t *capped) const {
        std::vector<double> hrows((size_t)(K * nlist) * NK_FP_ROW);
        std::vector<unsigned long long> hcnt((size_t)(K * nlist) * NK_FP_CNT);
        NK_HIP(rows.get(hrows.data(), K * nlist * NK_FP_ROW));
        NK_HIP(cnt.get(hcnt.data(), K * nlist * NK_FP_CNT));
        for (int64_t c = 0; c < K; ++c)
            for (int64_t i = 0; i < nlist; ++i) {
                const int64_t ci = c * nlist + i;
                const double *w = &hrows[(size_t)ci * NK_FP_ROW];
                if (pm) {
                    for (int x = 0; x < 3; ++x) { if (pm->D) pm->D[3 * ci + x] = w[x]; if (pm->D2) pm->D2[3 * ci + x] = w[3 + x]; }
                    if (pm->T) pm->T[ci] = w[6];
                    if (pm->hits) pm->hits[ci] = w[7];
                    if (pm->p_res) pm->p_res[ci] = w[8];
                    if (pm->p_wall) pm->p_wall[ci] = w[9];
                    if (pm->w_left) pm->w_left[ci] = w[10];
                    if (pm->p_int) pm->p_int[ci] = w[11];
                }
                casts[c] += (int64_t)hcnt[(size_t)ci * NK_FP_CNT]; missed[c] += (int64_t)hcnt[(size_t)ci * NK_FP_CNT + 1];
                capped[c] += (int64_t)hcnt[(size_t)ci * NK_FP_CNT + 2];
            }
        if (pr) {
            if (pr->D) NK_HIP(rD.get(pr->D, K * rays * 3));
            if (pr->T) NK_HIP(rT.get(pr->T, K * rays));
            if (pr->x0) NK_HIP(rx.get(pr->x0, rays * 3));
            if (pr->segments) NK_HIP(rs.get(pr->segments, K * rays));
            if (pr->end) NK_HIP(re.get(pr->end, K * rays));
        }
        return NK_OK;
    }
};

// launch() between two events on the stream, waited for: the device seconds of what it launched
template <class Launch>
static hipError_t nk_free_timed(hipStream_t stream, double &seconds, Launch launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, stream);
    if (e == hipSuccess) e = launch();
    if (e == hipSuccess) e = hipEventRecord(e1, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    seconds = 1e-3 * (double)ms;
    return e;
}

// k_free_paths (nk_freepath.hip) on buffers of this call alone: the particle store, its counters, the step counter and the
// emission bookkeeping are neither read nor written.
int nk_free_paths(nk_ctx *ctx, const nk_free_path_args *a, const nk_free_path_modes *pm, const nk_free_path_rays *pr, nk_free_path_report *rep) {
    if (rep) memset(rep, 0, sizeof(*rep));
    NK_ARG(ctx && a, "nk_free_paths: NULL argument");
    int64_t nlist, rays;
    NK_TRY(nk_free_refuse(ctx, "nk_free_paths", a, "the lifetimes of all Q*J modes at the temperature of the estimate", 1, nlist, rays));
    NK_HIP(hipSetDevice(ctx->device));
    NkFreeCall call(ctx, a, pr, 1, nlist, rays);
    NK_HIP(call.err());
    const NkFreeDev f = call.dev(ctx);
    nk_free_path_report r;
    memset(&r, 0, sizeof(r));
    r.rays = rays;
    r.geometry_mode = nk_geom_mode(ctx);
    r.calls = ctx->fp_last.calls + 1;
    r.bytes = call.bytes();
    NK_HIP(nk_free_timed(ctx->stream, r.seconds, [&] { return nk_free_paths_launch(ctx->d, f, nullptr, r.geometry_mode, nk_lds(ctx, true), ctx->stream); }));
    NK_TRY(call.copy_out(ctx, pm, &r.casts, &r.missed, &r.capped));
    ctx->fp_last = r;
    if (rep) *rep = r;
    return NK_OK;
}
int nk_free_paths_info(nk_ctx *ctx, nk_free_path_report *out) {
    NK_ARG(ctx && out, "nk_free_paths_info: NULL argument");
    *out = ctx->fp_last;
    return NK_OK;
}

// k_free_columns (nk_freecols.hip): the rays of nk_free_paths cast once and weighed with K lifetime tables.  Buffers of this call
// alone, as above; a call with more than NK_FC_TILE columns is flown in tiles of that many (one launch each, the casts repeated).
int nk_free_paths_columns(nk_ctx *ctx, const nk_free_path_args *a, int32_t n_columns, const nk_free_path_modes *pm, const nk_free_path_rays *pr,
                          nk_free_path_columns_report *rep) {
    if (rep) memset(rep, 0, sizeof(*rep));
    NK_ARG(ctx && a, "nk_free_paths_columns: NULL argument");
    NK_ARG(n_columns >= 1 && n_columns <= NK_FREE_PATH_MAX_COLUMNS, "nk_free_paths_columns: n_columns = " + std::to_string(n_columns) +
                                                                        " must be 1 .. " + std::to_string(NK_FREE_PATH_MAX_COLUMNS));
    int64_t nlist, rays;
    NK_TRY(nk_free_refuse(ctx, "nk_free_paths_columns", a, "per column the lifetimes of all Q*J modes", n_columns, nlist, rays));
    NK_HIP(hipSetDevice(ctx->device));
    const int64_t K = n_columns;
    const int ntiles = (int)((K + NK_FC_TILE - 1) / NK_FC_TILE);
    const unsigned grid = nk_free_columns_grid(nlist, a->n_samples);
    const int64_t nacc = a->n_samples > 64 ? (int64_t)grid * NK_FP_WAVES * (K < NK_FC_TILE ? K : NK_FC_TILE) * NK_FC_ACC * 64 : 0;
    NkFreeCall call(ctx, a, pr, K, nlist, rays);
    NK_HIP(call.err());
    NK_BUF(unsigned long long, dshared, nullptr, (int64_t)ntiles * nlist);
    NK_BUF(double, dacc, nullptr, nacc);
    NkFreeColsDev q;
    q.f = call.dev(ctx);
    q.M = ctx->d.M; q.rays = rays; q.acc = nacc ? dacc.p : nullptr;
    nk_free_path_columns_report r;
    memset(&r, 0, sizeof(r));
    r.rays = rays;
    r.n_columns = n_columns; r.tile = NK_FC_TILE; r.launches = nlist > 0 ? ntiles : 0;
    r.geometry_mode = nk_geom_mode(ctx);
    r.calls = ctx->fc_calls + 1;
    r.bytes = call.bytes() + (int64_t)ntiles * nlist * 8 + nacc * 8;
    NK_HIP(nk_free_timed(ctx->stream, r.seconds, [&] {
        hipError_t e = hipSuccess;
        for (int t = 0; t < ntiles && e == hipSuccess; ++t) {
            q.c0 = t * NK_FC_TILE;
            q.kc = (int32_t)(K - q.c0 < NK_FC_TILE ? K - q.c0 : NK_FC_TILE);
            q.shared = dshared.p + (int64_t)t * nlist;
            e = nk_free_columns_launch(ctx->d, q, r.geometry_mode, nk_lds(ctx, true), grid, ctx->stream);
        }
        return e;
    }));
    std::vector<unsigned long long> shared((size_t)ntiles * nlist);
    NK_HIP(dshared.get(shared.data(), (int64_t)ntiles * nlist));
    for (unsigned long long v : shared) r.casts_shared += (int64_t)v;
    NK_TRY(call.copy_out(ctx, pm, r.casts, r.missed, r.capped));
    ctx->fc_calls = r.calls;
    if (rep) *rep = r;
    return NK_OK;
}

// k_free_paths<*, true> (nk_freepath.hip): the rays of nk_free_paths binned by their start cell.  Buffers of this call alone, as
// above; the field, the mode tally and nk_free_paths' own report (fp_last) are not touched.
int nk_free_paths_map(nk_ctx *ctx, const nk_free_path_args *a, const nk_free_path_grid *gr, int64_t *cells, const nk_free_path_modes *pm,
                      const nk_free_path_rays *pr, nk_free_path_map_report *rep) {
    if (rep) memset(rep, 0, sizeof(*rep));
    NK_ARG(ctx && a && gr, "nk_free_paths_map: NULL argument");
    int64_t nlist, rays;
    NK_TRY(nk_free_refuse(ctx, "nk_free_paths_map", a, "the lifetimes of all Q*J modes at the temperature of the estimate", 1, nlist, rays));
    NkDev &d = ctx->d;
    // the map's own arguments
    NK_ARG(gr->weight, "nk_free_paths_map: weight is NULL (a weight vector per list entry, C_m v_m / (Q V))");
    double wmax = 0.0;
    for (int64_t i = 0; i < nlist * 3; ++i) {
        NK_ARG(std::isfinite(gr->weight[i]), "nk_free_paths_map: weight of list entry " + std::to_string((long long)(i / 3)) + " is not finite");
        wmax = std::max(wmax, fabs(gr->weight[i]));
    }
    NK_ARG(gr->n[0] > 0 && gr->n[1] > 0 && gr->n[2] > 0, "nk_free_paths_map: the cell counts n must be positive");
    for (int c = 0; c < 3; ++c)
        NK_ARG(gr->h[c] > 0.0 && std::isfinite(gr->h[c]) && std::isfinite(gr->lo[c]), "nk_free_paths_map: the cell sizes h must be positive (and lo finite)");
    const int64_t ncells = (int64_t)gr->n[0] * gr->n[1] * gr->n[2];
    NK_ARG(ncells <= (1ll << 24), "nk_free_paths_map: " + std::to_string((long long)ncells) + " cells are more than the grid takes (2^24)");
    NK_ARG(cells, "nk_free_paths_map: cells is NULL (the result, [ncells * 16] 64-bit integers)");
    NK_ARG(gr->capacity >= 0 && gr->weight_bound >= 0.0 && std::isfinite(gr->weight_bound), "nk_free_paths_map: capacity and weight_bound must not be negative");
    NK_ARG(ctx->h_vg.size() == (size_t)d.M * 3, "nk_free_paths_map: no group velocities (nk_set_material first)");
    // bounds and scales (DESIGN.md "Free-path maps"): over a ray sum W g <= 1, so |D_b| <= Lambda_max and T <= tau_max
    double lam = 0.0, tmax = 0.0;
    for (int64_t m = 0; m < d.M; ++m) {
        const double t = a->tau[m];
        if (!(t > 0.0)) continue;                               // (positive lifetimes are finite: nk_free_refuse)
        const double *v = &ctx->h_vg[3 * (size_t)m];
        const double vi = std::max(std::max(fabs(v[0]), fabs(v[1])), fabs(v[2]));
        lam = std::max(lam, vi * t);
        tmax = std::max(tmax, t);
    }
    nk_free_path_map_report r;
    memset(&r, 0, sizeof(r));
    r.rays = rays;
    r.B_K = std::max(wmax, gr->weight_bound) * lam;
    r.B_T = tmax;
    const int64_t cap = std::max<int64_t>(rays, gr->capacity);
    r.k_K = nk_field_k(r.B_K, cap); r.k_P = nk_field_k(1.0, cap); r.k_T = nk_field_k(r.B_T, cap);
    NK_HIP(hipSetDevice(ctx->device));
    NkFreeCall call(ctx, a, pr, 1, nlist, rays);
    NK_HIP(call.err());
    NK_BUF(double, dwt, gr->weight, nlist * 3);
    NK_BUF(unsigned long long, dgrid, nullptr, (ncells + 1) * NK_FREE_MAP_LINE);
    NK_BUF(int32_t, drc, nullptr, gr->ray_cell ? rays : 0);
    NK_BUF(double, drw, nullptr, gr->ray_w ? rays : 0);
    const NkFreeDev f = call.dev(ctx);
    NkFreeMapDev g;
    for (int c = 0; c < 3; ++c) { g.lo[c] = gr->lo[c]; g.inv_h[c] = 1.0 / gr->h[c]; g.n[c] = gr->n[c]; }
    g.ncells = (int32_t)ncells;
    g.weight = dwt.p;
    g.sK = ldexp(1.0, r.k_K); g.sP = ldexp(1.0, r.k_P); g.sT = ldexp(1.0, r.k_T);
    g.BK = r.B_K; g.BP = 1.0; g.BT = r.B_T;
    g.grid = dgrid.p;
    g.ray_cell = gr->ray_cell ? drc.p : nullptr; g.ray_w = gr->ray_w ? drw.p : nullptr;
    r.geometry_mode = nk_geom_mode(ctx);
    r.calls = ctx->fm_last.calls + 1;
    r.bytes = call.bytes() + nlist * 24 + (ncells + 1) * NK_FREE_MAP_LINE * 8 + (g.ray_cell ? rays * 4 : 0) + (g.ray_w ? rays * 8 : 0);
    NK_HIP(hipMemsetAsync(dgrid.p, 0, (size_t)(ncells + 1) * NK_FREE_MAP_LINE * 8, ctx->stream));      // (outside the timed window)
    NK_HIP(nk_free_timed(ctx->stream, r.seconds, [&] { return nk_free_paths_launch(d, f, &g, r.geometry_mode, nk_lds(ctx, true), ctx->stream); }));
    NK_TRY(call.copy_out(ctx, pm, &r.casts, &r.missed, &r.capped));
    if (gr->ray_cell) NK_HIP(drc.get(gr->ray_cell, rays));
    if (gr->ray_w) NK_HIP(drw.get(gr->ray_w, rays));
    NK_HIP(hipMemcpy(cells, dgrid.p, (size_t)ncells * NK_FREE_MAP_LINE * 8, hipMemcpyDeviceToHost));
    unsigned long long hdr[NK_FREE_MAP_LINE];
    NK_HIP(hipMemcpy(hdr, dgrid.p + (size_t)ncells * NK_FREE_MAP_LINE, sizeof(hdr), hipMemcpyDeviceToHost));
    r.clamped = (int64_t)hdr[NK_FM_CLAMPED];
    r.overflow = (int64_t)(hdr[NK_FM_OVK] + hdr[NK_FM_OVP] + hdr[NK_FM_OVT]);
    ctx->fm_last = r;
    if (rep) *rep = r;
    if (r.overflow) {
        ctx->err = "nk_free_paths_map: map overflow: " + std::to_string((long long)hdr[NK_FM_OVK]) + " term(s) of w D above B_K = " + std::to_string(r.B_K) +
                   ", " + std::to_string((long long)hdr[NK_FM_OVP]) + " weight(s) above B_P = 1, " + std::to_string((long long)hdr[NK_FM_OVT]) +
                   " flight time(s) above B_T = " + std::to_string(r.B_T) + "; they were left out of the sums";
        return NK_ERR_CAPACITY;
    }
    return NK_OK;
}
int nk_free_paths_map_info(nk_ctx *ctx, nk_free_path_map_report *out) {
    NK_ARG(ctx && out, "nk_free_paths_map_info: NULL argument");
    *out = ctx->fm_last;
    return NK_OK;
}

// ------------------------------------------------------------------------------------- kinetic flights
// k_kinetic (nk_kinetic.hip) on buffers of this call alone: the particle store, its counters, the step counter and the emission
// bookkeeping are neither read nor written.
static int nk_kin_table(nk_ctx *ctx, const char *name, const double *t, int64_t M) {
    NK_ARG(t, std::string("nk_kinetic_flights: ") + name + " is NULL (a cumulative table over all Q*J modes)");
    double prev = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        NK_ARG(t[m] >= prev && t[m] <= 1.0, std::string("nk_kinetic_flights: ") + name + " is not a cumulative table (entry " + std::to_string((long long)m) + ")");
        prev = t[m];
    }
    NK_ARG(M > 0 && t[M - 1] == 1.0, std::string("nk_kinetic_flights: ") + name + " does not end at 1 (no live mode?)");
    return NK_OK;
}
// The three entries: nk_kinetic_flights is this function without groups (g and gout null) and without a map (is_map false; gr and
// mout null); nk_kinetic_flights_map is it with the grid gr (never with groups).
static int nk_kin_run(nk_ctx *ctx, const nk_kinetic_args *a, const nk_kinetic_groups *g, const nk_kinetic_out *out,
                      const nk_kinetic_group_out *gout, const nk_kinetic_rays *pr, nk_kinetic_report *rep, bool is_map = false,
                      const nk_kinetic_grid *gr = nullptr, const nk_kinetic_map_out *mout = nullptr) {
    if (rep) memset(rep, 0, sizeof(*rep));
    if (!ctx) return NK_ERR_ARG;                                // (no context to hold a text)
    NK_ARG(a, "nk_kinetic_flights: NULL argument");
    NK_ARG(ctx->have_material, "nk_kinetic_flights: no material (nk_set_material first)");
    NK_ARG(ctx->have_mesh, "nk_kinetic_flights: no mesh (nk_set_mesh first)");
    NK_ARG(ctx->have_sv, "nk_kinetic_flights: no subvolumes (nk_set_subvolumes first)");
    const NkDev &d = ctx->d;
    const int64_t M = d.M;
    NK_ARG(ctx->h_vg.size() == (size_t)M * 3, "nk_kinetic_flights: no group velocities (nk_set_material first)");
    NK_ARG(a->n_samples > 0, "nk_kinetic_flights: n_samples = " + std::to_string(a->n_samples) + " must be positive");
    NK_ARG(a->max_events >= 0 && a->max_events <= (1 << 30), "nk_kinetic_flights: max_events must be 0 .. 2^30");
    NK_ARG(a->rays_per_wave >= 0, "nk_kinetic_flights: rays_per_wave must not be negative");
    NK_ARG(a->tau, "nk_kinetic_flights: tau is NULL (the lifetimes of all Q*J modes)");
    nk_kinetic_report r;
    memset(&r, 0, sizeof(r));
    NkKinDev f;
    memset(&f, 0, sizeof(f));
    for (int fc = 0; fc < d.Fc; ++fc) {
        const NkFacet &q = ctx->host_facets[fc];
        NK_ARG(q.bc != 'F', "nk_kinetic_flights: facet " + std::to_string(fc) + " has boundary condition 'F' (a fixed heat flux): the kinetic flights take reservoirs 'T', periodic 'P' and rough 'R' facets only");
        if (q.bc == 'T') {
            NK_ARG(r.n_sources < NK_KIN_MAX_SOURCES, "nk_kinetic_flights: more than " + std::to_string(NK_KIN_MAX_SOURCES) + " facets with boundary condition 'T' (the sources)");
            NK_ARG(ctx->h_ffo[fc + 1] > ctx->h_ffo[fc], "nk_kinetic_flights: source facet " + std::to_string(fc) + " has no faces");
            f.src_facet[r.n_sources] = fc; r.source_facet[r.n_sources] = fc;
            ++r.n_sources;
        }
    }
    NK_ARG(r.n_sources > 0, "nk_kinetic_flights: no facet with boundary condition 'T': nothing emits");
    for (int fc = 0; fc < d.Fc; ++fc) {
        const NkFacet &q = ctx->host_facets[fc];
        NK_ARG(q.bc != 'R' || (q.rough >= 0 && q.rough < d.Fr && d.specularity),
               "nk_kinetic_flights: facet " + std::to_string(fc) + " is rough ('R') but no rough tables are installed (nk_set_rough or nk_rough_finish)");
    }
    NK_TRY(nk_kin_table(ctx, "cdf_scatter", a->cdf_scatter, M));
    NK_TRY(nk_kin_table(ctx, "cdf_flux", a->cdf_flux, M));
    const int64_t n = a->n_samples, rays = n * r.n_sources;
    NK_ARG(rays < (1ll << 31), "nk_kinetic_flights: " + std::to_string((long long)rays) + " rays are more than one call takes (2^31)");
    // kinetic groups: n_groups + 1 columns, the last one for the modes whose entry is -1
    int32_t GC = 0;
    if (g) {
        NK_ARG(g->n_groups >= 1 && g->n_groups <= NK_KIN_MAX_GROUPS, "nk_kinetic_flights_groups: n_groups = " + std::to_string(g->n_groups) +
                                                                         " must be 1 .. " + std::to_string(NK_KIN_MAX_GROUPS));
        GC = g->n_groups + 1;                                   // (after the range check: no overflow)
        NK_ARG(g->group_of_mode, "nk_kinetic_flights_groups: group_of_mode is NULL (the group of all Q*J modes, -1 .. n_groups-1)");
        for (int64_t m = 0; m < M; ++m)
            NK_ARG(g->group_of_mode[m] >= -1 && g->group_of_mode[m] < g->n_groups,
                   "nk_kinetic_flights_groups: group_of_mode[" + std::to_string((long long)m) + "] = " + std::to_string(g->group_of_mode[m]) +
                       " is outside -1 .. " + std::to_string(g->n_groups - 1));
        const int64_t words = (int64_t)r.n_sources * d.S * GC * 4;
        NK_ARG(words <= NK_KIN_MAX_GROUP_WORDS, "nk_kinetic_flights_groups: " + std::to_string(r.n_sources) + " sources x " + std::to_string(d.S) +
                                                    " subvolumes x " + std::to_string(GC) + " columns x 4 = " + std::to_string((long long)words) +
                                                    " words are more than a call takes (2^24)");
    }
    // kinetic maps: the field's grid; the lines of (source, cell) live in memory for the length of the call
    int64_t ncells = 0, nmap = 0;
    if (is_map) {
        NK_ARG(gr, "nk_kinetic_flights_map: grid is NULL (the cell counts n, the corner lo and the cell sizes h)");
        NK_ARG(gr->n[0] > 0 && gr->n[1] > 0 && gr->n[2] > 0, "nk_kinetic_flights_map: the cell counts n must be positive");
        for (int c = 0; c < 3; ++c) {
            NK_ARG(gr->h[c] > 0.0 && std::isfinite(gr->h[c]), "nk_kinetic_flights_map: the cell sizes h must be positive and finite");
            NK_ARG(std::isfinite(gr->lo[c]), "nk_kinetic_flights_map: the corner lo must be finite");
        }
        ncells = (int64_t)gr->n[0] * gr->n[1] * gr->n[2];
        NK_ARG(ncells <= NK_KIN_MAX_MAP_CELLS, "nk_kinetic_flights_map: " + std::to_string((long long)ncells) + " cells are more than the grid takes (2^24)");
        nmap = (int64_t)r.n_sources * ncells * 4;
        NK_ARG(nmap <= NK_KIN_MAX_MAP_WORDS, "nk_kinetic_flights_map: " + std::to_string(r.n_sources) + " sources x " + std::to_string((long long)ncells) +
                                                 " cells x 4 = " + std::to_string((long long)nmap) + " words are more than a call takes (2^27)");
    }
    // bounds and scales: a segment lasts min(t_s, t_c), t_s <= 38 tau (u >= 2^-54) and, cast from inside the mesh, t_c <= 2 diagonal / |v|
    double diag = 0.0;
    for (int c = 0; c < 3; ++c) diag += (d.bbox[3 + c] - d.bbox[c]) * (d.bbox[3 + c] - d.bbox[c]);
    diag = sqrt(diag);
    double Bt = 0.0, Bx = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        const bool live = a->cdf_scatter[m] > (m ? a->cdf_scatter[m - 1] : 0.0);
        if (!live) continue;
        const double t = a->tau[m];
        NK_ARG(t > 0.0 && !std::isnan(t), "nk_kinetic_flights: mode " + std::to_string((long long)m) + " is drawn by cdf_scatter but its tau is not positive");
        const double *v = &ctx->h_vg[3 * (size_t)m];
        const double sp = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        const double tb = sp > 0.0 ? std::min(38.0 * t, 2.0 * diag / sp) : 38.0 * t;
        NK_ARG(std::isfinite(tb), "nk_kinetic_flights: mode " + std::to_string((long long)m) + " does not move and never scatters (tau is not finite)");
        Bt = std::max(Bt, tb);
        Bx = std::max(Bx, tb * std::max(std::max(fabs(v[0]), fabs(v[1])), fabs(v[2])));
    }
    NK_ARG(Bt > 0.0, "nk_kinetic_flights: no live mode");
    Bx = std::max(Bx, 1e-300);
    f.nsrc = r.n_sources; f.n = a->n_samples;
    f.max_events = a->max_events > 0 ? a->max_events : (1 << 20);
    f.rays_per_wave = a->rays_per_wave > 0 ? a->rays_per_wave : 512;
    f.blocks = (int32_t)((n + f.rays_per_wave - 1) / f.rays_per_wave);
    f.M = (int32_t)M;
    f.seed = a->seed ? a->seed : d.seed;
    r.B_t = Bt; r.B_x = Bx;
    f.Bt = Bt; f.Bx = Bx; f.BT = 1024.0 * Bt; f.BD = 1024.0 * Bx; f.BD2 = (32.0 * Bx) * (32.0 * Bx);
    const int64_t cap_seg = n * (int64_t)f.max_events;          // (< 2^61)
    r.k_t = nk_field_k(f.Bt, cap_seg); r.k_x = nk_field_k(f.Bx, cap_seg);
    r.k_T = nk_field_k(f.BT, n); r.k_D = nk_field_k(f.BD, n); r.k_D2 = nk_field_k(f.BD2, n);
    f.st = ldexp(1.0, r.k_t); f.sx = ldexp(1.0, r.k_x); f.sT = ldexp(1.0, r.k_T); f.sD = ldexp(1.0, r.k_D); f.sD2 = ldexp(1.0, r.k_D2);
    r.rays = rays; r.n_subvolumes = d.S;
    r.geometry_mode = nk_geom_mode(ctx);
    const size_t lds0 = (nk_lds(ctx, true) + 15) & ~(size_t)15;
    const int64_t nsub = (int64_t)r.n_sources * d.S * 4;
    const int64_t ngrp = nsub * GC;                             // the columns' words; with groups the bins hold these
    const int64_t nbins = g ? ngrp : nsub;
    r.lds_bins = (!a->no_bins && lds0 + (size_t)nbins * 8 <= 64 * 1024) ? 1 : 0;
    f.bins_off = (int32_t)lds0;
    const size_t lds = r.lds_bins ? lds0 + (size_t)nbins * 8 : nk_lds(ctx, true);
    r.grid = (f.nsrc * f.blocks + NK_KIN_WAVES - 1) / NK_KIN_WAVES;
    r.calls = ctx->kin_calls + 1;
    NK_HIP(hipSetDevice(ctx->device));
    const bool w = pr != nullptr;
    NK_BUF(double, dtau, a->tau, M); NK_BUF(double, dcs, a->cdf_scatter, M); NK_BUF(double, dcf, a->cdf_flux, M);
    NK_BUF(unsigned long long, drows, nullptr, (int64_t)r.n_sources * NK_KIN_ROW); NK_BUF(unsigned long long, dsub, nullptr, nsub);
    NK_BUF(double, rx, nullptr, (w && pr->x0) ? rays * 3 : 0); NK_BUF(double, rD, nullptr, (w && pr->D) ? rays * 3 : 0);
    NK_BUF(double, rT, nullptr, (w && pr->dwell) ? rays : 0);
    NK_BUF(int32_t, rm, nullptr, (w && pr->mode) ? rays : 0); NK_BUF(int32_t, re, nullptr, (w && pr->end) ? rays : 0);
    NK_BUF(int32_t, rv, nullptr, (w && pr->events) ? rays : 0); NK_BUF(int32_t, rc, nullptr, (w && pr->casts) ? rays : 0);
    NK_BUF(unsigned long long, rh, nullptr, (w && pr->hash) ? rays : 0);
    std::unique_ptr<NkDevBuf<int32_t>> dcol;                    // (a call without groups allocates neither)
    std::unique_ptr<NkDevBuf<unsigned long long>> dgrp;
    if (g) {
        std::vector<int32_t> hcol((size_t)M);
        for (int64_t m = 0; m < M; ++m) hcol[(size_t)m] = g->group_of_mode[m] < 0 ? g->n_groups : g->group_of_mode[m];
        dcol.reset(new NkDevBuf<int32_t>(hcol.data(), M)); NK_HIP(dcol->err);
        dgrp.reset(new NkDevBuf<unsigned long long>(nullptr, ngrp)); NK_HIP(dgrp->err);
        f.group = dcol->p; f.GC = GC; f.grp = dgrp->p;
    }
    std::unique_ptr<NkDevBuf<unsigned long long>> dmap;
    if (is_map) {
        dmap.reset(new NkDevBuf<unsigned long long>(nullptr, nmap)); NK_HIP(dmap->err);
        for (int c = 0; c < 3; ++c) { f.gn[c] = gr->n[c]; f.lo[c] = gr->lo[c]; f.inv_h[c] = 1.0 / gr->h[c]; }
        f.ncells = (int32_t)ncells; f.map = dmap->p;
    }
    f.tau = dtau.p; f.vg = ctx->d_vg; f.cdf_scatter = dcs.p; f.cdf_flux = dcf.p;
    f.rows = drows.p; f.sub = dsub.p;
    f.ray_x0 = (w && pr->x0) ? rx.p : nullptr; f.ray_D = (w && pr->D) ? rD.p : nullptr; f.ray_T = (w && pr->dwell) ? rT.p : nullptr;
    f.ray_mode = (w && pr->mode) ? rm.p : nullptr; f.ray_end = (w && pr->end) ? re.p : nullptr;
    f.ray_events = (w && pr->events) ? rv.p : nullptr; f.ray_casts = (w && pr->casts) ? rc.p : nullptr;
    f.ray_hash = (w && pr->hash) ? rh.p : nullptr;
    r.bytes = M * 24 + ((int64_t)r.n_sources * NK_KIN_ROW + nsub) * 8 + (f.ray_x0 ? rays * 24 : 0) + (f.ray_D ? rays * 24 : 0) + (f.ray_T ? rays * 8 : 0) +
              (f.ray_mode ? rays * 4 : 0) + (f.ray_end ? rays * 4 : 0) + (f.ray_events ? rays * 4 : 0) + (f.ray_casts ? rays * 4 : 0) + (f.ray_hash ? rays * 8 : 0) +
              (g ? M * 4 + ngrp * 8 : 0) + nmap * 8;
    NK_HIP(hipMemsetAsync(drows.p, 0, (size_t)r.n_sources * NK_KIN_ROW * 8, ctx->stream));      // (outside the timed window)
    NK_HIP(hipMemsetAsync(dsub.p, 0, (size_t)std::max<int64_t>(nsub, 1) * 8, ctx->stream));
    if (g) NK_HIP(hipMemsetAsync(dgrp->p, 0, (size_t)std::max<int64_t>(ngrp, 1) * 8, ctx->stream));
    if (is_map) NK_HIP(hipMemsetAsync(dmap->p, 0, (size_t)nmap * 8, ctx->stream));
    NK_HIP(nk_free_timed(ctx->stream, r.seconds, [&] { return nk_kinetic_launch(d, f, r.geometry_mode, lds, r.lds_bins != 0, ctx->stream); }));
    std::vector<unsigned long long> hrows((size_t)r.n_sources * NK_KIN_ROW);
    NK_HIP(drows.get(hrows.data(), (int64_t)hrows.size()));
    int64_t ov[5] = {0, 0, 0, 0, 0};
    for (int s = 0; s < r.n_sources; ++s) {
        const unsigned long long *q = &hrows[(size_t)s * NK_KIN_ROW];
        r.lost += (int64_t)q[NK_KR_LOST]; r.missed += (int64_t)q[NK_KR_MISSED]; r.capped += (int64_t)q[NK_KR_CAPPED];
        r.events += (int64_t)q[NK_KR_EVENTS]; r.casts += (int64_t)q[NK_KR_CASTS];
        for (int j = 0; j < 5; ++j) ov[j] += (int64_t)q[NK_KR_OVD + j];
    }
    r.overflow = ov[0] + ov[1] + ov[2] + ov[3] + ov[4];
    if (out && out->rows) memcpy(out->rows, hrows.data(), hrows.size() * 8);
    if (out && out->sub) NK_HIP(hipMemcpy(out->sub, dsub.p, (size_t)nsub * 8, hipMemcpyDeviceToHost));
    if (g && gout && gout->grp) NK_HIP(hipMemcpy(gout->grp, dgrp->p, (size_t)ngrp * 8, hipMemcpyDeviceToHost));
    if (is_map && mout && mout->cells) NK_HIP(hipMemcpy(mout->cells, dmap->p, (size_t)nmap * 8, hipMemcpyDeviceToHost));
    if (w) {
        NK_HIP(rx.get(pr->x0, rays * 3)); NK_HIP(rD.get(pr->D, rays * 3)); NK_HIP(rT.get(pr->dwell, rays));
        NK_HIP(rm.get(pr->mode, rays)); NK_HIP(re.get(pr->end, rays)); NK_HIP(rv.get(pr->events, rays)); NK_HIP(rc.get(pr->casts, rays));
        NK_HIP(rh.get((unsigned long long *)pr->hash, rays));
    }
    ctx->kin_calls = r.calls;
    if (rep) *rep = r;
    if (r.overflow) {
        ctx->err = "nk_kinetic_flights: overflow: " + std::to_string((long long)ov[0]) + " displacement(s), " + std::to_string((long long)ov[1]) +
                   " squared displacement(s) and " + std::to_string((long long)ov[2]) + " dwell time(s) of a ray, " + std::to_string((long long)ov[3]) +
                   " time(s) and " + std::to_string((long long)ov[4]) + " displacement(s) of a segment above their bounds; they were left out of the sums";
        return NK_ERR_CAPACITY;
    }
    return NK_OK;
}
int nk_kinetic_flights(nk_ctx *ctx, const nk_kinetic_args *a, const nk_kinetic_out *out, const nk_kinetic_rays *pr, nk_kinetic_report *rep) {
    return nk_kin_run(ctx, a, nullptr, out, nullptr, pr, rep);
}
int nk_kinetic_flights_groups(nk_ctx *ctx, const nk_kinetic_args *a, const nk_kinetic_groups *g, const nk_kinetic_out *out,
                              const nk_kinetic_group_out *gout, const nk_kinetic_rays *pr, nk_kinetic_report *rep) {
    if (ctx && !g) {                                            // (everything else is nk_kin_run's to check)
        if (rep) memset(rep, 0, sizeof(*rep));
        NK_ARG(g, "nk_kinetic_flights_groups: groups is NULL (n_groups and the group of every mode)");
    }
    return nk_kin_run(ctx, a, g, out, gout, pr, rep);
}
int nk_kinetic_flights_map(nk_ctx *ctx, const nk_kinetic_args *a, const nk_kinetic_grid *gr, const nk_kinetic_out *out,
                           const nk_kinetic_map_out *mout, const nk_kinetic_rays *pr, nk_kinetic_report *rep) {
    return nk_kin_run(ctx, a, nullptr, out, nullptr, pr, rep, true, gr, mout);
}

/* nanokappa_hip.h -- C ABI of libnanokappa_hip.so: the MI355X (gfx950) engine for Nano-kappa's
 * Population timestep loop.
 *
 * The reference (brunohs1993/Nanokappa) is pure Python with no FFI layer; the boundary this
 * library replaces is the body of `Population.run_timestep` (classes/Population.py:1724-1769)
 * and the helpers it calls.  Each entry point names the reference interface it stands for.
 * Python binds it with ctypes (nanokappa_amd/engine.py); INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions: plain pointers + sizes, caller owns every host buffer (the library copies, never
 * frees caller memory), the library owns device memory.  Every function returns 0 on success or a
 * negative nk_status; nk_last_error() gives the text.  A context is used from one host thread.
 * Units are the reference's: angstrom, ps, K, eV, rad/ps.  All real data is IEEE double.
 */
#ifndef NANOKAPPA_HIP_H
#define NANOKAPPA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nk_ctx nk_ctx;

enum nk_status {
    NK_OK = 0,
    NK_ERR_HIP = -1,        /* a HIP runtime call failed */
    NK_ERR_ARG = -2,        /* invalid argument / call order */
    NK_ERR_CAPACITY = -3,   /* particle capacity exceeded (raise it with nk_reserve) */
    NK_ERR_COMM = -4,       /* RCCL failure */
    NK_ERR_NODEVICE = -5    /* no usable gfx950 device */
};

/* Phonon tables, reference classes/Phonon.py (attributes read by Population: omega :165-167,
 * group_vel :181-183, lifetime :326-336, temperature_function / crystal_energy_function :372-390,
 * normalise_to_density :392-401, number_of_active_modes :126) */
typedef struct {
    int32_t Q, J, NT;
    const double *omega;         /* [Q*J]    rad/ps */
    const double *group_vel;     /* [Q*J*3]  angstrom/ps */
    const double *T_grid;        /* [NT]     K, ascending */
    const double *lifetime;      /* [NT*Q*J] ps; 0 means "relax fully" */
    int32_t nE;                  /* length of the E(T) table */
    double T_fill_lo, T_fill_hi; /* clamp values of T(E) outside the table */
    const double *T_array;       /* [nE] */
    const double *energy_array;  /* [nE] eV/angstrom^3, ascending */
    double hbar, kb;             /* classes/Constants.py:7-8 */
    double QV;                   /* number_of_qpoints * volume_unitcell */
    int32_t active_modes;
} nk_material;

/* Triangle mesh + boundary conditions, reference classes/Mesh.py:205-242, :314-327 and
 * classes/Geometry.py:652-709 (bound_cond), :711-726 (connected_facets) */
typedef struct {
    int32_t F;                     /* triangular faces */
    const double *normals;         /* [F*3] face_normals */
    const double *k;               /* [F]   face_k */
    const double *bounds_lo;       /* [F*3] face_bounds[0] */
    const double *bounds_hi;       /* [F*3] face_bounds[1] */
    const double *basis;           /* [F*9] face_basis_matrix (F,3,3) */
    const double *origins;         /* [F*3] face_origins */
    const int32_t *face_facet;     /* [F]   face_facets */
    const double *vertices;        /* [F*9] corners of each face (surface sampling, Mesh.py:939) */
    const double *face_area;       /* [F] */
    int32_t Fc;                    /* facets (groups of coplanar adjacent faces) */
    const int8_t *facet_bc;        /* [Fc] 'T', 'F', 'P' or 'R' */
    const int32_t *facet_partner;  /* [Fc] periodic partner facet, -1 if none */
    const double *facet_centroid;  /* [Fc*3] */
    const double *facet_normal;    /* [Fc*3] */
    const int32_t *facet_face_off; /* [Fc+1] CSR: faces of each facet */
    const int32_t *facet_face_idx;
    double tol;                    /* Mesh.tol (1e-10) */
    double bbox[6];                /* Geometry.bounds: lo xyz, hi xyz */
    int32_t nS;                    /* volume simplices for Mesh.sample_volume (Mesh.py:890-904) */
    const double *simplex_pts;     /* [nS*12] */
    const double *simplex_vol;     /* [nS] */
} nk_mesh;

/* Subvolumes, reference classes/Geometry.py:446-544 and SubvolClassifier :1198-1213 */
typedef struct {
    int32_t S;
    int32_t kind;            /* 0 slice (centres ascending along `axis`), 1 general nearest centre */
    int32_t axis;
    int32_t interp;          /* per-particle T: 0 interp1d 'nearest' on slices, 1 'linear' on slices,
                                2 nearest centre, 3 cubic radial basis functions = scipy RBFInterpolator
                                (Population.py:570-590, :694-702) */
    const double *centers;   /* [S*3] */
    const double *volumes;   /* [S] */
    /* interp 3 only (else NULL / 0): inverse of the RBF system of these centres, row-major (P x P), P = S + n_used
     * + 1; shift and scale of its polynomial part; which coordinates take part (Population.py:651-656) */
    const double *rbf_inv;
    const double *rbf_shift; /* [3] */
    const double *rbf_scale; /* [3] */
    int32_t rbf_used[3];
} nk_subvols;

/* Reservoirs, reference Population.py:323-354 (initialise_reservoirs), :146-161 (enter_probability) */
typedef struct {
    int32_t R;
    const int32_t *facet;      /* [R] facet index of each reservoir */
    const double *T;           /* [R] imposed temperature */
    const double *enter_prob;  /* [R*Q*J] */
    const double *counter;     /* [R*Q*J] initial res_counter (Population.py:343) */
    int32_t gen;               /* 0 'constant', 1 'fixed_rate', 2 'one_to_one' (Population.py:358-489) */
    const int64_t *n_leaving;  /* [R] 'one_to_one' only: particles to emit at the first step (Population.py:344:
                                * round(sum of enter_prob)), all ranks together; afterwards the engine emits what
                                * left through each reservoir at the previous step (:466, :1585).  NULL otherwise */
} nk_reservoirs;

/* Rough facets, reference Population.py:852-877 (specularity), :1042-1461 (specular map),
 * :879-939 (creation_roulette), :1017-1040 (degeneracies) */
typedef struct {
    int32_t Fr;
    const int32_t *facet;       /* [Fr] */
    const double *specularity;  /* [Fr*Q*J] */
    const uint8_t *true_spec;   /* [Fr*Q*J] */
    const int32_t *spec_map;    /* [Fr*Q*J] flat out-mode (q*J+j), -1 where not specular */
    const double *roulette;     /* [Fr*Q*J] cumulative, last = 1 */
    const int32_t *degen_j2;    /* [Q*J] partner branch for the 'k' model, or NULL */
} nk_rough;

/* Scalars of Population.__init__ (Population.py:41-95) */
typedef struct {
    double dt;                /* --timestep */
    int32_t norm_fixed;       /* --energy_normal: 0 'mean', 1 'fixed' */
    double particle_density;
    int32_t T_ref_local;      /* --reference_temp local */
    double T_ref;
    int32_t flux_every;       /* tally the subvolume heat flux every this many steps (n_dt_to_conv = 10) */
    int32_t contains_every;   /* contains_check period (100, Population.py:1729-1734); 0 = never */
    int32_t track_ids;        /* 0: 64-bit particle ids are stored only when the configuration draws random numbers per
                               *    particle (rough facets) -- 44 instead of 52 bytes of state per particle; downloads then
                               *    return pid = 0.  1: always stored (ids as uploaded / as nk_upload_particles numbers them).
                               *    The reference has no particle ids; they only key the counter-based RNG. */
} nk_params;

/* Per-step results of nk_step; every pointer may be NULL.  Row r describes the r-th step of the call.
 * Raw sums are un-normalised (the host applies Population.py:719-728 / :738-747 scalings where the
 * library has not already done so).  All sums are over ALL ranks once nk_comm_init was called. */
typedef struct {
    double *T_sv;        /* [nsteps*S]   subvol_temperature after the step (Population.py:692) */
    double *E_sv;        /* [nsteps*S]   subvol_energy, normalised + reference (Population.py:724-728) */
    double *E_raw;       /* [nsteps*S]   sum_i hbar*omega_i*dn_i per subvolume (Population.py:715-717) */
    double *N_sv;        /* [nsteps*S]   subvol_N_p (Population.py:679) */
    double *flux_raw;    /* [nsteps*S*3] sum_i v_i*e_i (Population.py:736); NaN on steps without flux tally */
    double *N_leaving;   /* [nsteps*R]   particles absorbed by each reservoir (Population.py:1585) */
    double *res_energy;  /* [nsteps*R]   this step's increment of res_energy_balance (Population.py:1595) */
    double *res_flux;    /* [nsteps*R*3] this step's increment of res_heat_flux (Population.py:1602) */
    double *N_emitted;   /* [nsteps]     particles that entered from reservoirs (Population.py:370) */
} nk_tally;

/* Kernel timing of the last nk_step call, from HIP events on the library's stream. */
typedef struct {
    double step_kernel_ms;   /* mean duration of k_sweep: relax + drift + boundary events + emission + tally */
    double emit_kernel_ms;   /* mean duration of the reservoir emission (k_emit; + k_emit_one_to_one for that generator) */
    double events_kernel_ms; /* mean duration of the step's tail: k_reduce (+ all-reduce) + k_update (+ the band pass of
                              * nk_set_bands on heat-flux steps) */
    double total_ms;         /* wall time of the whole call on the stream */
    int64_t slots;           /* particle capacity (nseg * segcap) */
    int64_t live;            /* live particles after the call (this rank) */
    /* housekeeping that can land inside a timed region, counted since nk_create: a benchmark reads them per region */
    int64_t regrows;         /* times the particle store was grown on the device after a halt request */
    int64_t halts;           /* batches that ended early on a halt request (every rank at the same step) */
    int64_t tau_rebuilds;    /* rebuilds of the packed mode records (lifetime window / E0 reference moved, or new segmentation) */
    int64_t batches;         /* nk_step_batch calls = stream drains + history copies */
    int64_t emit_fused;      /* 1: the next step's emission ran inside the tail launch (k_tail) in the last call: emit_kernel_ms then
                              *    covers only a batch's first step, events_kernel_ms the reduce / update WITH the emission beside it */
    int64_t place_tries;     /* allocations of the particle store that were timed when it was last (re)allocated (0: small store, not
                              * timed): where a store lies in memory decides between two speeds of the sweep, 15 % apart */
    double place_gbps;       /* GB/s of an in-place copy pass over the store that was kept ... */
    double place_worst_gbps; /* ... and over the slowest candidate */
    int64_t box_store;       /* 1: the particle store holds no cached next hit (axis-aligned box meshes: the hit is read off the
                                position, the reference's expression of Mesh.py:818 at event time); 36 B per particle, else 44 */
} nk_timing;

/* lifetime: `Population.__init__` / end of run */
int nk_device_count(void);                            /* HIP devices this process sees (0 if none) */
/* Set-up helper of the host geometry (no context): for every ray o + t d, t > 0 the number of triangles (v0, e1 = v1 - v0,
 * e2 = v2 - v0; arrays [n*3]) it crosses, crossings at the same distance (to 1e-8) counted once; skip_self: ray i ignores
 * triangle i.  The inside tests of nanokappa_amd.mesh (role of trimesh's ray queries in the reference's Mesh.py) run this on
 * large meshes; counts[i] = -1 where a ray has more than 24 distinct crossings (the caller counts that ray itself). */
int nk_mesh_crossings(int device, int64_t n_rays, const double *origins, const double *dirs, int64_t n_faces, const double *v0,
                      const double *e1, const double *e2, int skip_self, int32_t *counts);
int nk_create(nk_ctx **out, int device_id, uint64_t seed);
void nk_destroy(nk_ctx *ctx);
const char *nk_last_error(const nk_ctx *ctx);        /* ctx may be NULL: error of a failed nk_create */

/* setup tables (copied to HBM) */
int nk_set_material(nk_ctx *ctx, const nk_material *m);
int nk_set_mesh(nk_ctx *ctx, const nk_mesh *m);
int nk_set_subvolumes(nk_ctx *ctx, const nk_subvols *s, const double *T_sv_init /* [S] */);
int nk_set_reservoirs(nk_ctx *ctx, const nk_reservoirs *r);
int nk_set_rough(nk_ctx *ctx, const nk_rough *r);
int nk_set_params(nk_ctx *ctx, const nk_params *p);

/* particle state: Population.initialise_all_particles (Population.py:186-321) hands over positions, modes
 * and occupations; n_ts/facet/pid may be NULL (then nk_init_boundaries computes the first two, and pid = index
 * + pid_offset) */
int nk_reserve(nk_ctx *ctx, int64_t capacity);
int nk_upload_particles(nk_ctx *ctx, int64_t N, const double *x, const double *y, const double *z,
                        const int32_t *mode, const double *occ, const double *n_ts, const int32_t *facet,
                        const uint64_t *pid, uint64_t pid_offset);
/* Population.timesteps_to_boundary for the whole population (Population.py:310-314) */
int nk_init_boundaries(nk_ctx *ctx);
/* Population.initialise_all_particles on the device (Population.py:186-321), instead of nk_reserve + nk_upload_particles, for
 * the common case: modes tiled over the particle ids (initialise_modes, :127-144: particle p has mode unique_modes[p %
 * n_unique], flat indices q * J + j of the active modes), ids pid_lo .. pid_lo + N - 1, positions uniform in the solid
 * (Mesh.sample_volume, Mesh.py:890-904; sv_first NULL = 'random_domain') or uniform in the subvolume the particle's id
 * belongs to (sv_first[S + 1] ascending from 0: id p in [sv_first[s], sv_first[s + 1]) lies in subvolume s =
 * 'random_subvol', :222-246; ids, not local indices, so that the shards of several ranks make up the single-rank ensemble), occupations Bose-Einstein at the subvolume's temperature (:280).  Needs nk_set_material,
 * nk_set_mesh (with the volume tables), nk_set_subvolumes and the boundary-condition tables; nk_init_boundaries follows. */
int nk_init_particles(nk_ctx *ctx, int64_t N, int64_t capacity, uint64_t pid_lo, const int32_t *unique_modes, int64_t n_unique,
                      const int64_t *sv_first);
/* calculate_energy and the heat-flux sums of the particles where they stand, before normalisation (Population.py:704-717,
 * :734-736; the reference's t = 0 row): E_raw[S], N_sv[S], flux_raw[S * 3].  This rank's particles only. */
int nk_tally_state(nk_ctx *ctx, double *E_raw, double *N_sv, double *flux_raw);
/* Population.run_timestep x nsteps (Population.py:1724-1769) without the file output.  The particle store grows by
 * itself (on the device, nothing is dropped) when the ensemble outgrows it, like the reference's arrays do; NK_ERR_CAPACITY
 * only if that growth fails (out of memory), with the state of the last completed step intact. */
int nk_step(nk_ctx *ctx, int32_t nsteps, nk_tally *out);
/* live particles, in slot order; arrays may be NULL; *N_out receives the count (call with capacity 0 to query) */
int nk_download_particles(nk_ctx *ctx, int64_t capacity, double *x, double *y, double *z, int32_t *mode,
                          double *occ, double *n_ts, int32_t *facet, uint64_t *pid, int64_t *N_out);
int nk_get_subvol_temperature(nk_ctx *ctx, double *T_sv /* [S] */);
int nk_set_subvol_temperature(nk_ctx *ctx, const double *T_sv /* [S] */);
int nk_get_step(nk_ctx *ctx, int64_t *step);
int nk_get_timing(nk_ctx *ctx, nk_timing *t);

/* multi-GPU: one context per rank; tallies are all-reduced (sum, f64) over RCCL every step */
int nk_comm_unique_id(void *id128 /* 128 bytes out */);
/* Joins the communicator and PROVES it before returning: the rank count and this rank's index are read back from RCCL
 * (ncclCommCount / ncclCommUserRank) and a vector {1, rank + 1} is all-reduced on the context's stream; NK_ERR_COMM unless
 * the sums are nranks and nranks (nranks + 1) / 2, i.e. unless exactly the expected ranks took part. */
int nk_comm_init(nk_ctx *ctx, const void *id128, int rank, int nranks);
/* What the communicator itself says (not what the caller passed): for logs and the bench line. */
typedef struct {
    int32_t rank, nranks;            /* as given to nk_comm_init (1 rank before it is called) */
    int32_t comm_rank, comm_nranks;  /* ncclCommUserRank / ncclCommCount; -1 / 0 when there is no communicator (one rank, dry run) */
    int32_t device;                  /* HIP device of this context */
    int32_t selftest_ok;             /* 1: the all-reduce of ones at nk_comm_init returned nranks */
    double selftest_sum;             /* what that all-reduce returned (0 without communicator) */
    char pci_bus_id[32];             /* hipDeviceGetPCIBusId of that device */
} nk_comm_report;
int nk_comm_info(nk_ctx *ctx, nk_comm_report *out);
/* Sum of a small host vector over the ranks of the communicator (in place; unchanged when there is none): the t = 0 tallies
 * of the shards (Population.py:282, :318-321 on an ensemble that is spread over the ranks). */
int nk_comm_allreduce(nk_ctx *ctx, double *inout, int64_t n);

/* Frequency-resolved conductivity (reference Visualisation.flux_contribution, Visualisation.py:592-651): the heat flux tallied
 * per subvolume AND band.  band_of_mode [M] gives the band (0 .. nbands - 1, or -1 for none) of every global mode index q*J+j;
 * what a band is (frequency, branch, mean free path) is the caller's choice.  nbands = 0 turns the feature off (the default):
 * then nothing is launched or allocated for it.  Needs nk_set_material and nk_set_subvolumes; NK_ERR_ARG when the S x nbands
 * bins do not fit the pass's LDS even one band at a time.  While bands are on, the resident kernel (NK_RESIDENT) is not used.
 * Rows: F [S][nbands][3] = sum of v_i e_i and N [S][nbands] = particle counts, e_i = hbar omega_i (n_i - n0) exactly as the
 * flux_raw row computes it, so that sum over the bands of F[s] = flux_raw[s] of the same step (up to the order of the sums). */
int nk_set_bands(nk_ctx *ctx, int32_t nbands, const int32_t *band_of_mode);
/* The rows of the heat-flux steps of the last nk_step call ((step + 1) % flux_every == 0), tallied after the step's sweep --
 * the particles and occupations that step's flux_raw summed, against the same temperatures -- and the absolute step of each.
 * A heat-flux step at which migrating particles (rough facets) did not fit their new segment, so that the store grows before
 * they are delivered, has no row: the pass did not see them.  The pass is timed with the tail (events_kernel_ms).
 * F [nrows*S*nbands*3], N [nrows*S*nbands], steps [nrows]; any may be NULL; *nrows receives the count (cap 0: query only;
 * otherwise cap must hold every row).  Summed over all ranks (one all-reduce per nk_step call) once nk_comm_init was called. */
int nk_get_band_rows(nk_ctx *ctx, double *F, double *N, int64_t *steps, int32_t cap, int32_t *nrows);
/* The same sums for the particles where they stand, after the deferred relaxation, with n0 at each particle's interpolated
 * temperature (the one the relaxation uses; the reference's Population.temperatures) and the current T_sv:
 * F [S*nbands*3], N [S*nbands], summed over the ranks with a communicator. */
int nk_tally_bands_state(nk_ctx *ctx, double *F, double *N);

/* Spatial field maps (the GPU-native counterpart of the reference's particle scatter plots, Population.plot_figures,
 * Population.py:1841-1979, drawn at :123 and every 100 steps at :1735): particle count N, deviational energy E = sum e_i and
 * heat flux F = sum v_i e_i on a uniform grid of n[0] x n[1] x n[2] cells of size h from corner lo, independent of the
 * subvolumes.  Cell of a particle: floor((x - lo) * (1 / h)) per axis, an index outside [0, n) CLAMPED into the edge cell
 * (and counted in `clamped`); cell index (ix * n[1] + iy) * n[2] + iz.  The sums are accumulated as 64-bit integers of terms
 * scaled by 2^k_E / 2^k_F (nk_field_report): for given per-particle terms and scales the sums are the same bits whatever the
 * order of the adds, the path (LDS / global) or the split of the particles over ranks, and every rank of a communicator holds
 * the same field.  (Two RUNS of one ensemble on different rank counts still differ in the last bits of their subvolume
 * temperatures, hence of the terms.) */
typedef struct {
    double lo[3], h[3];
    int32_t n[3];            /* {0, 0, 0}: off (the default) -- nothing is launched or allocated */
    int32_t every;           /* field steps: (step + 1) % every == 0; a positive multiple of nk_params.flux_every */
    int32_t flags;           /* NK_FIELD_GLOBAL | NK_FIELD_TEST_SMALL_BOUND */
    int64_t capacity;        /* 0: the scales follow the particle slots of the store(s); > 0: they allow for at least this many,
                              * so that runs on stores of different sizes (other rank counts) derive the same k_E, k_F and
                              * their integers can be compared or added */
} nk_field;
#define NK_FIELD_GLOBAL 1            /* never keep the bins in LDS (also: environment NK_FIELD_PATH=global); the result is the same bits */
#define NK_FIELD_TEST_SMALL_BOUND 2  /* test hook: divide the bound B_E by 2^40, so that ordinary terms exceed it */
/* NK_ERR_ARG: every <= 0 or not a multiple of flux_every, h <= 0, more than 2^24 cells, or before nk_set_material /
 * nk_set_subvolumes / nk_set_params.  While a field is on, the resident kernel (NK_RESIDENT) is not used.  Step mode tallies
 * right after the sweep of a field step with the tally's own e_i (so cells and the step's E_raw / flux_raw row sum the same
 * terms); each field step's integer grid is summed over the ranks (ncclInt64) and added to a double accumulator. */
int nk_set_field(nk_ctx *ctx, const nk_field *f);
/* The sums over the field steps since the last reset: N [ncells], E [ncells], F [ncells*3] (any may be NULL), the number of
 * field steps in them and the particles that were clamped; reset != 0 starts a new average.  A field step whose rough-wall
 * migrants were not delivered is skipped and not counted in samples.  The same on every rank of a communicator. */
int nk_get_field(nk_ctx *ctx, double *N, double *E, double *F, int64_t *samples, int64_t *clamped, int32_t reset);
/* State mode: the particles where they stand, after the deferred relaxation, e_i against the occupation at each particle's
 * interpolated temperature (or T_ref), as nk_tally_bands_state.  raw [ncells*8]: per cell the integers {N, E 2^k_E, Fx 2^k_F,
 * Fy 2^k_F, Fz 2^k_F, 0, 0, 0} of this call alone (summed over the ranks of a communicator).  NK_ERR_CAPACITY, naming the
 * sum, when a term exceeded its bound (never a silent wrap); nk_step reports the same for its field steps. */
int nk_tally_field_state(nk_ctx *ctx, int64_t *raw, int64_t *clamped);
typedef struct {
    int32_t n[3], every;
    int64_t ncells;
    int32_t k_E, k_F;        /* the integers hold e_i 2^k_E and v_i e_i 2^k_F, rounded to nearest */
    double B_E, B_F;         /* bounds of |e_i| (eV) and |v_i e_i| the scales were derived from */
    int64_t capacity;        /* particle slots of all ranks the scales allow for */
    int64_t bytes;           /* device memory allocated for the field (0 when off) */
    int32_t lds_path;        /* 1: bins in LDS with one flush per workgroup, 0: global integer adds directly */
    int32_t on;
} nk_field_report;
int nk_field_info(nk_ctx *ctx, nk_field_report *out);

/* Grouped field maps: the field's three sums per (cell, group of modes) -- N, E = sum e_i and F = sum v_i e_i over the
 * particles of cell c whose mode m has group_of_mode[m] = g.  A group is whatever the caller says (a frequency bin, a branch,
 * a mean-free-path bin, a direction bin); -1 puts a mode in no group: its particles are added nowhere and counted in
 * `ungrouped`.  The grid, the cadence (nk_field.every), the bounds, the scales 2^k_E / 2^k_F and the capacity are the
 * field's, the terms and the cell rule are k_field's, and a sample is taken or dropped together with the field's, so the two
 * windows always hold the same steps: for a table that groups every mode the sums over g of the integers of a cell are the
 * field's integers of that cell, bit for bit.  Line of (cell c, group g): c * ngroups + g.  Same bits on the LDS and the
 * global path (NK_FIELD_GLOBAL and NK_FIELD_PATH=global force the latter here too), from run to run and for any split of
 * the particles over ranks.
 * ngroups = 0: off (the default) -- nothing is launched or allocated, everything is freed.  group_of_mode [M], M = Q*J.
 * NK_ERR_ARG: no field (nk_set_field first), an entry outside [-1, ngroups), more than 2^24 lines (cells x groups);
 * NK_ERR_HIP (with the byte count) when the allocation fails.  nk_set_field, with a new grid or to switch the field off,
 * switches the groups off.  While they are on the resident kernel is not used, and a replica group refuses the context (as
 * for the field). */
int nk_set_field_groups(nk_ctx *ctx, int32_t ngroups, const int32_t *group_of_mode);
/* The sums over the field steps since the last reset: N [ncells*G], E [ncells*G], F [ncells*G*3] (any may be NULL), the
 * number of field steps in them and the particles of ungrouped modes they met; reset != 0 starts a new window (reset the
 * field's at the same time to keep the two in step).  NK_ERR_CAPACITY, naming the sum, when a term exceeded its bound. */
int nk_get_field_groups(nk_ctx *ctx, double *N, double *E, double *F, int64_t *samples, int64_t *ungrouped, int32_t reset);
/* State mode, as nk_tally_field_state: raw [ncells*G*8], per line the integers {N, E 2^k_E, Fx 2^k_F, Fy 2^k_F, Fz 2^k_F, 0,
 * 0, 0} of this call alone (summed over the ranks of a communicator); clamped counts grouped particles outside the grid. */
int nk_tally_field_groups_state(nk_ctx *ctx, int64_t *raw, int64_t *clamped, int64_t *ungrouped);
typedef struct {
    int32_t G;               /* groups */
    int32_t lds_path;        /* 1: bins in LDS with one flush per workgroup, 0: global integer adds directly */
    int64_t lines;           /* ncells * G */
    int64_t bytes;           /* device memory allocated for the groups (0 when off) */
    int32_t k_E, k_F;        /* the field's scales */
    int64_t permutes;        /* times the table was brought into the segments' order (a new table, mode map or store size) */
    int32_t on, pad_;
} nk_field_groups_report;
int nk_field_groups_info(nk_ctx *ctx, nk_field_groups_report *out);

/* ---- Solid fraction of the field's cells.  A set-up helper of the host geometry (no context), as nk_mesh_crossings: V[c],
 * the volume of solid in cell c = (ix * n[1] + iy) * n[2] + iz of the grid lo / h / n (the convention of nk_field), for a closed
 * triangle mesh whose faces are wound so that their normals point out of the solid (tri: three vertices per face).  Exact
 * for the triangles -- no sampling, no quadrature: every triangle is clipped to the cells of its bounding box, the clipped
 * polygon gives the signed area a of its projection on the yz plane and p = the integral of (x - x_lo) over it, both summed
 * per cell as 64-bit integers (scaled by 2^k_A, 2^k_P, rounded to nearest; the same bits from call to call), and
 * V[ix] = P[ix] + h_x sum_{ix' > ix} A[ix'] along x in every (iy, iz) column.  The arithmetic is done in grid units
 * (x - lo) / h, so the scales stand for areas and volumes in cells.  A triangle is offered to the cells floor((x - lo) / h) of
 * its bounding box, clamped into [0, n), and clipped against closed slabs: a face lying in a grid plane perpendicular to x is
 * counted in exactly one cell, one in the grid's upper x boundary in the last cell.  The grid must contain the bounding box of
 * the triangles and may be larger (cells outside the solid get 0); a vertex within 1e-9 cells outside it (rounding of a grid
 * made from the mesh's own bounds) is moved onto the boundary.  nanokappa_amd.field.solid_volume is the same rule in NumPy.
 * NK_ERR_ARG, with a text that names the cause (nk_solid_last_error): n_faces <= 0, h <= 0, more than 2^24 cells, a grid
 * that does not contain the triangles; NK_ERR_NODEVICE without a gfx950 device. */
typedef struct {
    int64_t ncells, pairs;   /* cells; (triangle, yz column) work items of the clipping kernel */
    int32_t k_A, k_P;        /* the integers hold a 2^k_A and p 2^k_P (a, p in grid units) */
    double seconds;          /* device time of the two kernels */
} nk_solid_report;
int nk_cell_solid_volume(int device, int64_t n_faces, const double *tri /* [n_faces*9], outward */, const double lo[3],
                         const double h[3], const int32_t n[3], double *V /* [ncells] */, nk_solid_report *rep /* may be NULL */);
const char *nk_solid_last_error(void);               /* text of this thread's last failed nk_cell_solid_volume */

/* Mode-resolved tally: the distribution itself, E[s][m] = sum e_i and N[s][m] over the particles of subvolume s in mode
 * m = q*J + j, at full resolution (S x M bins).  The group velocity is a property of the mode, so the heat flux of a mode is
 * v_m E[s][m] exactly, and any band sum of nk_set_bands is a sum of entries of this table.  One pass over the store per mode
 * step, one wave per segment: the modes are partitioned over the segments, so a wave keeps the bins of its segment's modes
 * in LDS and writes its rows of the table with plain stores (owner path); without the partition, or when the bins do not fit,
 * the adds go to the table in global memory (global path).  The sums are 64-bit integers of terms scaled by 2^k_E
 * (nk_modes_report; the field's bound and scale rule): the same bits on either path, from run to run and for any split of the
 * particles over ranks. */
typedef struct {
    int32_t every;           /* 0: off (the default) -- nothing is launched or allocated; else mode steps are the steps with
                              * (step + 1) % every == 0, a positive multiple of nk_params.flux_every */
    int32_t flags;           /* NK_MODES_GLOBAL | NK_MODES_TEST_SMALL_BOUND */
    int64_t capacity;        /* as nk_field.capacity: a floor under the particle slots the scale allows for */
} nk_modes;
#define NK_MODES_GLOBAL 1            /* never keep the bins in LDS (also: environment NK_MODES_PATH=global); the result is the same bits */
#define NK_MODES_TEST_SMALL_BOUND 2  /* test hook: divide the bound B_E by 2^40, so that ordinary terms exceed it */
/* NK_ERR_ARG: every < 0 or not a multiple of flux_every, or before nk_set_material / nk_set_subvolumes / nk_set_params;
 * NK_ERR_HIP (with the size) when the tables cannot be allocated.  While the tally is on, the resident kernel (NK_RESIDENT)
 * is not used.  Step mode tallies right after the sweep of a mode step with the tally's own e_i (so the table and the step's
 * E_raw / N_sv / flux_raw row sum the same terms). */
int nk_set_modes(nk_ctx *ctx, const nk_modes *m);
/* The sums over the mode steps since the last reset: N [S*M], E [S*M] (index s*M + m, m = q*J + j; either may be NULL), the
 * number of mode steps in them and of mode steps that were skipped (rough-wall migrants not delivered on some rank); all
 * ranks together (every rank takes or drops the same samples); reset != 0 starts a new average.  NK_ERR_CAPACITY, naming
 * the sum, when a term exceeded its bound (never a silent wrap); nk_step reports the same for its mode steps. */
int nk_get_modes(nk_ctx *ctx, double *N, double *E, int64_t *samples, int64_t *skipped, int32_t reset);
/* State mode: the particles where they stand, after the deferred relaxation, e_i against the occupation at each particle's
 * interpolated temperature (or T_ref), as nk_tally_field_state.  The raw integers N [S*M], E 2^k_E [S*M] of this call alone,
 * summed over the ranks of a communicator. */
int nk_tally_modes_state(nk_ctx *ctx, int64_t *N, int64_t *E);
typedef struct {
    int32_t every, k_E;      /* the integers hold e_i 2^k_E */
    double B_E;              /* bound of |e_i| (eV) the scale was derived from */
    int64_t capacity;        /* particle slots of all ranks the scale allows for */
    int64_t bytes;           /* device memory allocated for the tally (0 when off) */
    int32_t owner_path;      /* 1: wave-private bins in LDS and plain stores, 0: global integer adds */
    int32_t on;
} nk_modes_report;
int nk_modes_info(nk_ctx *ctx, nk_modes_report *out);

/* Free-path sampling: what conductivity the geometry and the material alone allow, read off ray casts before a single step.
 * For every mode of the list n_samples rays start uniformly in the solid and fly along the mode's group velocity, W = 1:
 * per cast (the general cast of the mesh's geometry mode), with tc the time to the hit and a = tc / tau: g = -expm1(-a),
 * D += W tau g v, T += W tau g, p_int += W g, W *= exp(-a), hits += W; a miss takes g = 1 and ends the ray.  At a hit the
 * facet decides: 'T' / 'F' p_res += W, end; 'P' go on from the hit point + the facet's translation; 'R' draws (r0, r1): specular
 * iff true_spec && r0 <= specularity -- go on from the hit point in mode spec_map (its degenerate partner when degen_j2 names one
 * and r1 >= 0.5) -- else diffuse: p_wall += W, end.  A ray also ends when W < w_min or after max_segments hits (its W goes to
 * w_left).  A mode with v = 0 or tau <= 0 takes no cast (p_int = its whole weight).  Per mode p_res + p_wall + w_left + p_int =
 * n_samples.  An ESTIMATE of the conductivity (kappa_ab = sum_m C_m v_a D_b / (n QV), the host's part): exact (Fuchs-Sondheimer)
 * where the walls that end the flights are parallel to the transport direction, an approximation where reservoirs end them along
 * it.  The pass has device buffers of its own for the length of the call and touches neither the particle store nor the step
 * counter: it may be called at any point between nk_step calls, with or without particles.  No atomics: a mode's row is the same
 * bits whatever the other modes of the list. */
typedef struct {
    int32_t n_modes;             /* entries of `modes`; ignored when it is NULL */
    const int32_t *modes;        /* [n_modes] global mode indices q*J + j, or NULL: all Q*J modes, in order */
    int32_t n_samples;           /* rays per mode */
    int32_t max_segments;        /* hits after which a ray is cut off; 0 = 65536 */
    double w_min;                /* weight below which a ray ends; 0 = 2^-40 */
    const double *tau;           /* [Q*J] lifetimes (ps) at the temperature of the estimate */
    const double *x0;            /* [rays*3] start points, ray = list index * n_samples + sample, or NULL: drawn on the device */
    uint64_t seed;               /* Philox key; 0 = the context's */
} nk_free_path_args;
typedef struct {                 /* per mode of the list; any pointer may be NULL */
    double *D;                   /* [n*3] sum of the rays' displacements (angstrom) */
    double *D2;                  /* [n*3] sum of their squares, per component */
    double *T;                   /* [n]   sum of the flight times (ps) */
    double *hits;                /* [n]   sum over the hits of the weight that arrived */
    double *p_res, *p_wall;      /* [n]   weight absorbed by reservoirs / scattered diffusely by walls */
    double *w_left;              /* [n]   weight of the rays cut off (w_min, max_segments) */
    double *p_int;               /* [n]   weight scattered intrinsically: sum of T / tau per segment */
} nk_free_path_modes;
typedef struct {                 /* per ray (tests and small calls); any pointer may be NULL */
    double *D;                   /* [rays*3] */
    double *T;                   /* [rays] */
    int32_t *segments;           /* [rays] casts of the ray */
    int32_t *end;                /* [rays] 0 weight exhausted, 1 reservoir, 2 diffuse wall, 3 miss, 4 cap */
    double *x0;                  /* [rays*3] the start points used */
} nk_free_path_rays;
typedef struct {
    int64_t rays, casts, missed, capped;
    int32_t geometry_mode;       /* 1 planes and faces in LDS, 2 tables in global memory (face tree) */
    int32_t calls;               /* nk_free_paths calls on this context so far */
    int64_t bytes;               /* device memory the last call allocated (and freed) */
    double seconds;              /* device time of the kernel, from HIP events */
} nk_free_path_report;
/* NK_ERR_ARG, with a text that names the cause: no material or mesh, 'R' facets without rough tables (nk_set_rough /
 * nk_rough_finish), no x0 on a mesh that was set without its volume tables, n_samples <= 0, a mode out of range, tau NULL, a
 * lifetime that is positive and not finite in any entry of tau ("tau of mode m is not finite"; a lifetime that is not positive -- 0,
 * negative, -inf, NaN -- is a mode that does not live and is taken), a coordinate of x0 that is not finite ("x0 of list entry i,
 * sample s is not finite").  Nothing is launched or allocated then and the report is all zero. */
int nk_free_paths(nk_ctx *ctx, const nk_free_path_args *args, const nk_free_path_modes *modes, const nk_free_path_rays *rays,
                  nk_free_path_report *report);
/* The report of the last call; all zero on a context that never made one (nothing was launched or allocated). */
int nk_free_paths_info(nk_ctx *ctx, nk_free_path_report *out);

/* Free-path sweeps: the rays of nk_free_paths weighed with K lifetime tables at once.  The path of a ray -- start point, facets,
 * translations, specular / diffuse draws, the modes it is reflected into -- does not depend on the lifetimes, so every ray is
 * cast once per segment and every column c keeps weights of its own {W, D, T}: while it is alive it takes the statements of
 * nk_free_paths with tau = column c; it starts dead where the start mode has v = 0 or tau_c <= 0, and ends by the rules above
 * (its own W against w_min; the hit count against max_segments is the ray's).  The ray flies while any column is alive.
 * Column c of the result equals nk_free_paths called with tau = row c of `tau` on the same list, n_samples, x0 or seed,
 * max_segments and w_min, bit for bit: per-mode sums, per-ray outputs and counts; it depends neither on the other modes of the
 * list nor on the other columns of the call.  args->tau is [n_columns][Q*J] (row c = column c); every array of `modes` and of
 * `rays` has a leading column axis ([n_columns][n*3], [n_columns][rays], ...) except rays->x0 [rays*3], which is the ray's.
 * Up to `tile` columns share a cast; a call with more is flown in ceil(n_columns / tile) launches that repeat the casts.
 * A geometry scaled by s with unchanged roughness is the same flight with lifetimes tau / s and displacements s D; a temperature
 * enters through tau(T) alone: the host builds both sweeps on this call.  Buffers of the call alone, as nk_free_paths. */
#define NK_FREE_PATH_MAX_COLUMNS 32
typedef struct {
    int64_t rays;                /* rays flown (per tile of columns) */
    int64_t casts_shared;        /* casts made: = casts[0] for one column, never more than the sum of the columns' */
    int64_t casts[NK_FREE_PATH_MAX_COLUMNS];     /* per column: casts made while it was alive (nk_free_paths' `casts`) */
    int64_t missed[NK_FREE_PATH_MAX_COLUMNS], capped[NK_FREE_PATH_MAX_COLUMNS];
    int32_t n_columns;
    int32_t tile;                /* columns that share a cast */
    int32_t launches;            /* kernel launches of the call: tiles of columns */
    int32_t geometry_mode;       /* as nk_free_path_report */
    int32_t calls;               /* nk_free_paths_columns calls on this context so far */
    int32_t pad_;
    int64_t bytes;               /* device memory the call allocated (and freed) */
    double seconds;              /* device time of the launches, from HIP events */
} nk_free_path_columns_report;
/* NK_ERR_ARG, with a text that names the cause: n_columns outside 1 .. NK_FREE_PATH_MAX_COLUMNS, and every refusal of
 * nk_free_paths, in its words (a lifetime in any of the n_columns tables; with more than one the text adds "(column c)"); nothing
 * is launched or allocated then and the report is all zero. */
int nk_free_paths_columns(nk_ctx *ctx, const nk_free_path_args *args, int32_t n_columns, const nk_free_path_modes *modes,
                          const nk_free_path_rays *rays, nk_free_path_columns_report *report);

/* Free-path maps: the rays of nk_free_paths binned on the device by the cell of their START point -- where in the structure
 * the walls cut the heat flow (the Fuchs-Sondheimer local conductivity).  The flight, the per-mode sums and the per-ray
 * outputs are those of nk_free_paths with the same arguments, bit for bit.  The grid is the field's (nk_field): cell of a
 * start point = floor((x - lo) * (1 / h)) per axis, an index outside [0, n) or a NaN clamped into the edge cell and counted in
 * `clamped`; cell order (ix * ny + iy) * nz + iz.  Per cell one line of NK_FREE_MAP_LINE 64-bit integers:
 *   0          N, the rays that started in the cell
 *   1 + 3a + b the sum of w_a D_b 2^k_K, w = `weight` of the ray's LIST ENTRY (on the host C_m v_m / (Q V); also after
 *              reflections into other modes), D the ray's displacement
 *   10, 11, 12 the sums of the rays' final weights 2^k_P that ended at a reservoir (p_res), at a diffuse wall (p_wall), or were
 *              cut off by w_min or max_segments (w_left); a miss, a reflection into a mode that does not live and a ray
 *              without a cast add nothing: p_int of a cell = N - p_res - p_wall - w_left
 *   13         the sum of the flight times 2^k_T
 *   14, 15     zero
 * Every term is rounded to nearest even after the scaling and added as an integer in two's complement (an exact zero is not
 * added), so the cells are the same bits in any order of the rays and sums of calls with equal scales are the cells of the
 * joint call.  Scales: k = the largest with cap B 2^k <= 2^62, cap = max(rays of the call, `capacity`), B_K = max(largest
 * |weight| component, `weight_bound`) x the largest |v_m| component x tau_m over ALL modes with tau > 0, B_P = 1, B_T = the
 * largest positive tau.  A term above its bound is left out and counted in `overflow`, and the call returns NK_ERR_CAPACITY with a
 * text that names the sum: a sum never wraps silently.  For a mode set with inversion symmetry sum_m C_m v_a E[D_b | x0 = x] is
 * the local conductivity tensor at x in the relaxation-time picture: exact on the terms that make the global estimate exact,
 * an approximation otherwise (reservoirs that end flights along the transport direction): an estimate, not a replacement for
 * the run's field.  Buffers of the call alone; neither the particle store, the step counter, the field, the mode tally nor
 * the state of nk_free_paths (nk_free_paths_info) is touched. */
#define NK_FREE_MAP_LINE 16
typedef struct {
    int32_t n[3]; int32_t pad_;
    double lo[3], h[3];          /* the field's grid convention */
    const double *weight;        /* [n_list * 3] per list entry (n_list = Q*J when args->modes is NULL) */
    int64_t capacity;            /* floor under the ray count when the scales are derived; 0: none */
    double weight_bound;         /* floor under max |weight|; 0: none */
    int32_t *ray_cell;           /* [rays] the start cell of every ray, or NULL */
    double *ray_w;               /* [rays] the weight that went to word 10, 11 or 12, zero otherwise, or NULL */
} nk_free_path_grid;
typedef struct {
    int64_t rays, casts, missed, capped, clamped, overflow;
    int32_t k_K, k_P, k_T, geometry_mode, calls, pad_;
    double B_K, B_T;
    int64_t bytes;               /* device memory the last call allocated (and freed) */
    double seconds;              /* device time of the kernel, from HIP events */
} nk_free_path_map_report;
/* NK_ERR_ARG, with a text that names the cause: every refusal of nk_free_paths, in its words; `weight` NULL or not finite; n or h
 * not positive; more than 2^24 cells; `cells` NULL.  Nothing is launched or allocated then and the report is all zero. */
int nk_free_paths_map(nk_ctx *ctx, const nk_free_path_args *args, const nk_free_path_grid *grid, int64_t *cells /* [ncells*16] */,
                      const nk_free_path_modes *modes, const nk_free_path_rays *rays, nk_free_path_map_report *report);
/* The report of the last map call; all zero on a context that never made one. */
int nk_free_paths_map_info(nk_ctx *ctx, nk_free_path_map_report *out);

/* Kinetic flights: the deviational, time-step-free Monte Carlo of the steady linearised BTE in the relaxation-time picture.
 * Sources are the facets with boundary condition 'T', in ascending order (at most NK_KIN_MAX_SOURCES).  From every source
 * n_samples energy packets are emitted uniformly over the facet in a mode drawn in proportion to c_m (v_m . n)+ (by rejection from
 * cdf_flux, n the facet's inward normal; 64 refusals: `lost`).  A packet flies along its group velocity for min(t_s, t_c), t_s =
 * -tau ln(u) the free time and t_c the time to the next facet (the general cast of the mesh's geometry mode; a mode with v = 0 sits
 * for t_s).  Then it scatters into a mode drawn from cdf_scatter (t_s < t_c), or the facet decides: 'T' absorbs it (its end is that
 * facet's source index), 'P' translates it, 'R' takes the specular test of nk_free_paths and on the diffuse outcome RE-EMITS it
 * from the hit point by the emission's rule with that facet's inward normal.  A miss ends the ray (`missed`), and so do
 * max_events events (`capped`).  Every segment adds t v to the ray's displacement and t to its dwell time, and t and t v to the
 * words of (source, subvolume of one uniform point of the segment).  Ray id = (source index << 32) | sample; the draws and their
 * tags are listed in nanokappa_amd/csrc/nk_kinetic.h.  Every sum is a 64-bit integer at a power-of-two scale 2^k (k in the
 * report): a result depends neither on the order of the adds nor on the launch grid.  A term above its bound is left out and
 * counted, and the call then returns NK_ERR_CAPACITY with a text (the sums are still returned).  Bounds: a segment lasts at most
 * B_t = max over the live modes of min(38 tau, 2 diagonal / |v|) and moves at most B_x (likewise, per component); a ray's
 * displacement and dwell time are bounded by 1024 B_x and 1024 B_t, its squared displacement by (32 B_x)^2.
 * The pass has device buffers of its own for the length of the call and touches neither the particle store, its counters nor the
 * step counter. */
#define NK_KIN_MAX_SOURCES 8
#define NK_KIN_ROW_WORDS 32
typedef struct {
    int32_t n_samples;           /* rays per source */
    int32_t max_events;          /* events after which a ray is cut off; 0 = 2^20 */
    int32_t rays_per_wave;       /* rays of a source that one wave flies (the launch grid follows from it); 0 = 512 */
    int32_t no_bins;             /* 1: the per-subvolume words go straight to memory, not through LDS bins (the same bits) */
    const double *tau;           /* [Q*J] lifetimes (ps) */
    const double *cdf_scatter;   /* [Q*J] cumulative c_m / tau_m over the live modes, ending at 1 */
    const double *cdf_flux;      /* [Q*J] cumulative c_m |v_m| over the live modes, ending at 1 */
    uint64_t seed;               /* Philox key; 0 = the context's */
} nk_kinetic_args;
typedef struct {                 /* any pointer may be NULL */
    int64_t *rows;               /* [n_sources * NK_KIN_ROW_WORDS] per source: ends[8], lost, missed, capped, events, casts, D[3] 2^k_D,
                                  * D^2[3] 2^k_D2, dwell 2^k_T, then the terms left out: of D, D^2, the dwell, a segment's t, its t v;
                                  * word 25: the segment points clamped into the grid (nk_kinetic_flights_map only, 0 otherwise) */
    int64_t *sub;                /* [n_sources * S * 4] per (source, subvolume): dwell 2^k_t, t v_x, t v_y, t v_z 2^k_x */
} nk_kinetic_out;
typedef struct {                 /* per ray (ray = source index * n_samples + sample); any pointer may be NULL */
    double *x0;                  /* [rays*3] start points */
    int32_t *mode;               /* [rays] start mode (-1: lost at the emission) */
    int32_t *end;                /* [rays] >= 0 the source index that absorbed it, -1 lost, -2 missed, -3 capped */
    int32_t *events, *casts;     /* [rays] */
    double *D;                   /* [rays*3] displacement */
    double *dwell;               /* [rays] */
    uint64_t *hash;              /* [rays] of the event sequence: h = h 1000003 + (1 for a scattering, facet + 2 for a hit) */
} nk_kinetic_rays;
typedef struct {
    int64_t rays, events, casts, lost, missed, capped, overflow;
    int32_t n_sources, n_subvolumes;
    int32_t source_facet[NK_KIN_MAX_SOURCES];
    int32_t k_D, k_D2, k_T, k_t, k_x;
    int32_t geometry_mode;       /* as nk_free_path_report */
    int32_t lds_bins;            /* 1: the per-subvolume words went through LDS bins */
    int32_t grid;                /* workgroups launched */
    int32_t calls, pad_;         /* nk_kinetic_flights calls on this context so far */
    double B_t, B_x;
    int64_t bytes;               /* device memory the call allocated (and freed) */
    double seconds;              /* device time of the kernel, from HIP events */
} nk_kinetic_report;
/* NK_ERR_ARG, with a text that names the cause: no material, mesh or subvolumes; no 'T' facet; more than NK_KIN_MAX_SOURCES of
 * them; a facet with boundary condition 'F'; 'R' facets without rough tables; n_samples <= 0; a table NULL or not a cumulative
 * table that ends at 1; no live mode.  Nothing is launched or allocated then and the report is all zero. */
int nk_kinetic_flights(nk_ctx *ctx, const nk_kinetic_args *args, const nk_kinetic_out *out, const nk_kinetic_rays *rays,
                       nk_kinetic_report *report);

/* Kinetic groups: nk_kinetic_flights with the per-subvolume words also split by group of modes -- which phonons carry the heat.
 * The table names the group 0 .. n_groups-1 of every mode, or -1; a segment's four words {t, t v_x, t v_y, t v_z} (the same
 * quantised integers as `sub`) go to the column of the mode the segment was FLOWN in (the mode before the event that ends it
 * changes it).  There are n_groups + 1 columns: the last one, the REST column, takes every mode whose entry is -1 (a live mode
 * that does not move has no mean free path and no direction), so the columns of a (source, subvolume) always add up to its words
 * in `sub` -- as integers, bit for bit: the kernel tallies the columns only and `sub` is folded from them by integer adds
 * (k_kinetic_fold), which gives the bits of an ungrouped call.  Everything else -- rows, the per-ray outputs, the report -- is what
 * nk_kinetic_flights returns for the same arguments; both entries run through one host function.  The columns are gathered in
 * LDS bins where n_sources * S * (n_groups + 1) * 4 words fit behind the mesh tables in 64 KB and go straight to memory otherwise
 * (the report's lds_bins says which; the same bits). */
#define NK_KIN_MAX_GROUPS 256
#define NK_KIN_MAX_GROUP_WORDS (1 << 24)
typedef struct {
    int32_t n_groups;            /* 1 .. NK_KIN_MAX_GROUPS */
    const int32_t *group_of_mode; /* [Q*J], -1 .. n_groups-1 */
} nk_kinetic_groups;
typedef struct {                 /* the pointer may be NULL */
    int64_t *grp;                /* [n_sources * S * (n_groups + 1) * 4] per (source, subvolume, column): dwell 2^k_t, t v_x, t v_y,
                                  * t v_z 2^k_x; column n_groups is the rest column */
} nk_kinetic_group_out;
/* NK_ERR_ARG as nk_kinetic_flights, and with a text that names the cause: groups or its table NULL; n_groups < 1 or >
 * NK_KIN_MAX_GROUPS; a table entry outside -1 .. n_groups-1; n_sources * S * (n_groups + 1) * 4 above NK_KIN_MAX_GROUP_WORDS.
 * Nothing is launched or allocated then. */
int nk_kinetic_flights_groups(nk_ctx *ctx, const nk_kinetic_args *args, const nk_kinetic_groups *groups, const nk_kinetic_out *out,
                              const nk_kinetic_group_out *group_out, const nk_kinetic_rays *rays, nk_kinetic_report *report);

/* Kinetic maps: nk_kinetic_flights with the segments' words also binned on a 3-D grid -- the steady temperature and heat-flux field
 * of the structure.  The grid is the field's: cell of a point = floor((x_a - lo_a) * (1 / h_a)) per axis, an index outside [0, n_a)
 * or a NaN clamped into the edge cell and counted; cell order (ix * ny + iy) * nz + iz.  Every segment that adds its four integers
 * {t, t v_x, t v_y, t v_z} to the words of (source, subvolume of x_p) adds the SAME four integers to the line of (source, cell of
 * x_p), x_p the same uniform point of the segment: no second rounding, no new bound, no new random number.  So for every source and
 * word the cells add up to the subvolumes of `sub` bit for bit.  The lines go straight to memory; `sub` keeps its LDS bins.  The
 * points clamped are counted per source in word 25 of the source's row (0 in a call of the two entries above).  Everything else --
 * rows, sub, the per-ray outputs, the report -- is what nk_kinetic_flights returns for the same arguments; the three entries run
 * through one host function. */
#define NK_KIN_ROW_CLAMPED 25
#define NK_KIN_MAX_MAP_CELLS (1 << 24)
#define NK_KIN_MAX_MAP_WORDS (1 << 27)
typedef struct {
    int32_t n[3];                /* cells per axis, > 0; at most NK_KIN_MAX_MAP_CELLS in all */
    int32_t pad_;
    double lo[3], h[3];          /* the corner of cell (0, 0, 0) and the cell sizes (angstrom), h > 0 */
} nk_kinetic_grid;
typedef struct {                 /* the pointer may be NULL */
    int64_t *cells;              /* [n_sources * ncells * 4] per (source, cell): dwell 2^k_t, t v_x, t v_y, t v_z 2^k_x */
} nk_kinetic_map_out;
/* NK_ERR_ARG as nk_kinetic_flights, and with a text that names the cause: grid NULL; n or h not positive or h not finite; lo not
 * finite; more than NK_KIN_MAX_MAP_CELLS cells; n_sources * ncells * 4 above NK_KIN_MAX_MAP_WORDS.  Nothing is launched or
 * allocated then and the report is all zero. */
int nk_kinetic_flights_map(nk_ctx *ctx, const nk_kinetic_args *args, const nk_kinetic_grid *grid, const nk_kinetic_out *out,
                           const nk_kinetic_map_out *map_out, const nk_kinetic_rays *rays, nk_kinetic_report *report);

/* Replica groups: R contexts that hold the same problem under different seeds (the runs behind an error bar) are stepped by
 * shared launches -- per step ONE sweep and ONE tail launch for all of them instead of R of each, and one wait per call.  A
 * workgroup of the shared launch finds its member and runs that member's step exactly as nk_step would: the rows and the
 * particles of a member are the bits a solo run gives, whatever the group.  The fast path covers what one launch pair can
 * express: tables in LDS (small meshes), no rough facets, no RBF temperatures, generators 'constant' / 'fixed_rate', one rank,
 * bands / field / mode tally off; the resident kernel is never used for a group. */
typedef struct nk_group nk_group;
#define NK_GROUP_MAX_MEMBERS 32
typedef struct {
    int32_t R;                   /* members */
    int32_t halted;              /* members whose store had to grow in the middle of a call, since nk_group_create */
    int32_t finished_alone;      /* ... and that then finished the remaining steps of a call alone */
    int32_t grid_sweep;          /* workgroups of the last k_sweep_group launch: the members' sweep grids, concatenated */
    int32_t grid_tail;           /* ... and of the last k_tail_group launch: per member NB reduce workgroups + its emission's */
    int32_t pad_;
    int64_t steps;               /* steps taken through the group (every member took each of them) */
    int64_t sweep_launches;      /* k_sweep_group launches issued */
    int64_t tail_launches;       /* k_tail_group launches issued */
    int64_t member_launches;     /* launches issued for ONE member: the preludes of contains_check steps (k_anchor, k_relax,
                                  * k_contains), a first emission that no tail has run ahead, and the steps of stragglers
                                  * (counted as 2 each) */
    double sweep_kernel_ms;      /* mean duration of k_sweep_group, from HIP events on the first 4 steps of the last call of at */
    double tail_kernel_ms;       /* least 4 steps (the convention of nk_timing); ... of k_tail_group */
    double total_ms;             /* wall time of the last call's grouped steps on the stream */
} nk_group_report;
/* NK_ERR_ARG, with a reason that names the member (its index in `members`) and the condition, when R < 1 or R >
 * NK_GROUP_MAX_MEMBERS, a context appears twice, the members are on different devices, a member is not ready (nk_step would
 * refuse it) or outside the fast path, or the members disagree on what the shared launch bakes in: the kernel instantiation,
 * S, R, NB, flux_every, contains_every, dt, the generator, the current step.  They may differ in seed, particles,
 * temperatures and store size (hence in segments and in the LDS they need: a launch asks for the largest need, at most 64 KB).
 * Nothing is launched then.  *out = NULL on failure; nk_group_last_error(NULL) has the reason. */
int nk_group_create(nk_group **out, nk_ctx *const *members, int32_t R);
void nk_group_destroy(nk_group *g);     /* never touches the members; destroy it before any member */
/* nk_step(members[r], nsteps, &outs[r]) for every member; outs (or any of its entries' pointers) may be NULL.  A member whose
 * store fills up stops on its own while the others run on; after the shared launches the host grows its store and finishes its
 * remaining steps alone: nothing is dropped, every member has taken nsteps steps and delivered nsteps rows.  Between calls a
 * member may be stepped alone with nk_step; NK_ERR_ARG when the members are then no longer at the same step. */
int nk_group_step(nk_group *g, int32_t nsteps, nk_tally *outs /* [R] */);
int nk_group_info(nk_group *g, nk_group_report *out);
const char *nk_group_last_error(const nk_group *g);   /* g may be NULL: error of a failed nk_group_create */

/* device versions of the reference's primitives, for parity tests (tests/ -m gpu) */
int nk_find_boundary(nk_ctx *ctx, int64_t n, const double *x /* [n*3] */, const double *v /* [n*3] */,
                     double *xc, double *tc, int32_t *fc);                       /* Mesh.py:806-856 */
/* The same cast for rays that start on a named facet, as an entering particle starts on its reservoir: per ray the facet skip
 * is formed as the sweep forms it (nk_tree_skip: the facet's centroid and normal, the ray) and handed to the walk of the face
 * tree.  from_facet[i] = -1 or any value outside [0, facets): no skip.  skipped[i] = 1 where the walk left out the nodes that
 * hold only faces of from_facet[i]; 0 everywhere on a mesh of at most 256 faces and facets (no tree).  (xc, tc, fc) as above:
 * the skip never changes a result. */
int nk_find_boundary_from(nk_ctx *ctx, int64_t n, const double *x /* [n*3] */, const double *v /* [n*3] */,
                          const int32_t *from_facet /* [n] */, double *xc, double *tc, int32_t *fc, int32_t *skipped /* [n] */);
/* A read-only view of the face tree that nk_set_mesh built (meshes of more than 256 faces or facets; NG = 0 and all else 0
 * without one).  Level 0 holds one box per leaf (the union of the boxes of its four slots), level l + 1 one box per four nodes of
 * level l, up to tree_top, whose nodes are the top family. */
typedef struct {
    int32_t NG;                  /* 1: the casts walk the tree, 0: they sweep all planes */
    int32_t tree_top;            /* index of the top level */
    int32_t level_nodes[8];      /* nodes per level (without the padding nodes that fill a level up to a multiple of 4) */
    int32_t tree_base[8];        /* first box of each level in family_boxes, in boxes of 6 floats */
    int32_t top_family;          /* nodes of the top level: 2..4 (1 for a tree of a single leaf) */
    int32_t tree_leaves;         /* leaf records, 4 slots each */
    int32_t references;          /* face references in the leaves (a sliver is referred to several times) */
    int32_t pad_slots;           /* leaf slots without a face */
    int32_t n_families;          /* families of four boxes over all levels */
    int32_t pad_;
    double tree_bound;           /* largest |coordinate| of a box */
} nk_tree_report;
/* family_boxes [n_families * 24] floats (per family four boxes lo(3) hi(3); padding boxes have lo > hi), leaf_boxes
 * [tree_leaves * 24] floats (the boxes of a leaf's four slots); either may be NULL.  Call once with NULLs for the sizes. */
int nk_tree_info(nk_ctx *ctx, nk_tree_report *out, float *family_boxes, float *leaf_boxes);
int nk_classify(nk_ctx *ctx, int64_t n, const double *x, int32_t *id);           /* Geometry.py:1212 */
/* The box store's wall functions (nk_device.h) on n rays, with the context's walls, tol and dt; NK_ERR_ARG unless nk_set_mesh
 * found a box.  which: 0 nk_box_out (t = 1.0 / 0.0, facet = -1; x is the end-of-step position), 1 nk_box_first_hit (t = the
 * crossing time in timesteps from the end of the step, negative; its facet), 2 nk_box_next_hit (t = time to the next wall,
 * its facet; inf, -1 on a miss).  Needs no particle store. */
int nk_box_hit(nk_ctx *ctx, int32_t which, int64_t n, const double *x /* [n*3] */, const double *v /* [n*3] */,
               double *t /* [n] */, int32_t *facet /* [n] */);
int nk_eval(nk_ctx *ctx, int32_t what, int64_t n, const double *a, const int32_t *mode, double *out);
/* what: 0 occupation(T=a[i], omega[mode[i]]) Phonon.py:338; 1 lifetime(T=a[i], mode[i]) Phonon.py:336;
 *       2 T(E=a[i]) Phonon.py:387; 3 E(T=a[i]) Phonon.py:390; 4 per-particle T at x=a[3i..] Population.py:696;
 *       5 the kernels' own exp(a[i]); 6 their short series exp(a[i]), |a[i]| <= 1/8; 7 their reciprocal 1 / a[i];
 *       8 their relaxation of one particle, a[4i..] = x, y, z, occupation, of mode[i], with the context's dt, subvolume
 *         temperatures and lifetimes (Population.py:1701-1710); 64 consecutive i make one wave, which picks the exponential */
/* The segment of the particle store that holds the particles of every mode (seg[M]) and the number of segments, once particles
 * are uploaded.  nk_download_particles returns the segments one after another, each in slot order, and a wave of the sweep takes
 * 64 consecutive slots of one segment: with this map a test can tell which particles shared a wave. */
int nk_mode_segments(nk_ctx *ctx, int32_t *seg, int32_t *nseg);
int nk_reflect(nk_ctx *ctx, int64_t n, const int32_t *facet, const int32_t *mode_in, const double *col_pos,
               const double *n_in, const double *omega_in, const double *r_spec, const double *r_deg,
               const double *r_diff, int32_t *mode_out, double *n_out, double *omega_out); /* Population.py:941-1015 */
int nk_uniform2(uint64_t seed, uint64_t pid, uint32_t step, uint32_t tag, double *u0, double *u1);

/* measurement helper: `launches` sweeps of the particle arrays with a known byte count per launch (returned), in
 * the access shape of the step kernel, so that rocprofv3 FETCH_SIZE / WRITE_SIZE readings can be calibrated */
int nk_calibrate_stream(nk_ctx *ctx, int32_t launches, int64_t *bytes_read, int64_t *bytes_written);

/* Set-up table builder: find_specular_correspondences, 'velocity' model
 * (Population.py:1241-1454) for one surface normal.  group_vel [M*3], omega [M], delta_omega [M] (the grid tolerance
 * of :1245-1247) are uploaded by nk_specular_begin; nk_specular_pairs returns every (in-mode, out-mode) pair of flat
 * mode indices, unordered, for the (rounded, inward) normal; *n_pairs receives the count (call again with a larger
 * `cap` when it exceeds it).  pair_in = pair_out = NULL: the pairs stay on the device (for nk_rough_pairs), none returned. */
int nk_specular_begin(nk_ctx *ctx, int64_t M, const double *group_vel, const double *omega, const double *delta_omega);
int nk_specular_pairs(nk_ctx *ctx, const double *normal /* [3] */, double crit, int64_t cap, int32_t *pair_in,
                      int32_t *pair_out, int64_t *n_pairs);
int nk_specular_end(nk_ctx *ctx);


/* The rough-facet tables built on the device and installed in place of nk_set_rough ('velocity' reflection model):
 * calculate_fbz_specularity (Population.py:852-877), true_specular and the specular map of find_specular_correspondences
 * (:1457-1459), diffuse_scat_probability (:879-939).  Protocol, inside nk_specular_begin .. nk_specular_end:
 *   nk_rough_begin(Fr, facet[Fr], inward normals [Fr*3] (= -facets_normal), eta [Fr], |k| per q-point [Q]);
 *   for every distinct (rounded) normal: nk_specular_pairs(normal, ...), then nk_rough_pairs(the rough-facet indices that
 *   share it) -- the pairs are taken from the device, where the search left them;
 *   nk_rough_finish(): specularity, creation rates, their cumulative roulette and its bucket index; the tables stay on the
 *   device.  nk_rough_download copies them back (tests, host attributes); any pointer may be NULL. */
int nk_rough_begin(nk_ctx *ctx, int32_t Fr, const int32_t *facet, const double *normal_in, const double *eta, const double *k_norm);
int nk_rough_pairs(nk_ctx *ctx, int32_t nf, const int32_t *fidx);
int nk_rough_finish(nk_ctx *ctx);
/* The 'k' / wavevector reflection model (Population.py:1056-1240) through the same calls: after nk_specular_begin,
 * nk_kspec_begin uploads the wavevectors [Q*3] with Phonon.k_to_q / q_to_k as row-major 3 x 3 matrices (q = k . k_to_q,
 * k = q . q_to_k) and tol[3] = q_to_k(|1 / (2 mesh)|); nk_kspec_pairs is nk_specular_pairs for that model (one partner per
 * in-mode); nk_rough_finish_k also averages the creation rates of the degenerate branches (find_degeneracies :1017-1040:
 * nd rows q, j1, j2, applied in order, :926-930) and installs degen_j2 [M] (as in nk_rough) for the reflection's coin flip. */
int nk_kspec_begin(nk_ctx *ctx, int64_t Q, const double *wavevectors, const double *k_to_q, const double *q_to_k, const double *tol);
int nk_kspec_pairs(nk_ctx *ctx, const double *normal /* [3] */, int64_t cap, int32_t *pair_in, int32_t *pair_out, int64_t *n_pairs);
int nk_rough_finish_k(nk_ctx *ctx, int32_t nd, const int32_t *degen /* [nd*3] */, const int32_t *degen_j2 /* [M] or NULL */);
int nk_rough_download(nk_ctx *ctx, double *specularity, uint8_t *true_spec, int32_t *spec_map, double *roulette);
/* enter_probability (Population.py:146-161) on the device: out[r*M + m] = max(0, v_m . n_in_r) * dt / thickness_r */
int nk_build_enter_prob(nk_ctx *ctx, int32_t R, const double *normal_in, const double *thickness, double dt, double *out);

#ifdef __cplusplus
}
#endif
#endif

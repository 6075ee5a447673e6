"""ctypes binding of libnanokappa_hip.so (include/nanokappa_hip.h) and a thin `Engine` object.

No CPU fallback: if the library is missing it must be built (`python -c "import __graft_entry__ as g;
g.build()"` or `make -C nanokappa_amd/csrc`), and `Engine()` raises when no gfx950 device is present.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get('NK_LIBNAME', 'libnanokappa_hip.so'))   # NK_LIBNAME: developer builds

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int32)
c_bp = C.POINTER(C.c_int8)
c_up = C.POINTER(C.c_uint8)
c_u64p = C.POINTER(C.c_uint64)


class NkError(RuntimeError):
    pass


class nk_material(C.Structure):
    _fields_ = [('Q', C.c_int32), ('J', C.c_int32), ('NT', C.c_int32),
                ('omega', c_dp), ('group_vel', c_dp), ('T_grid', c_dp), ('lifetime', c_dp),
                ('nE', C.c_int32), ('T_fill_lo', C.c_double), ('T_fill_hi', C.c_double),
                ('T_array', c_dp), ('energy_array', c_dp),
                ('hbar', C.c_double), ('kb', C.c_double), ('QV', C.c_double), ('active_modes', C.c_int32)]


class nk_mesh(C.Structure):
    _fields_ = [('F', C.c_int32), ('normals', c_dp), ('k', c_dp), ('bounds_lo', c_dp), ('bounds_hi', c_dp),
                ('basis', c_dp), ('origins', c_dp), ('face_facet', c_ip), ('vertices', c_dp), ('face_area', c_dp),
                ('Fc', C.c_int32), ('facet_bc', c_bp), ('facet_partner', c_ip), ('facet_centroid', c_dp),
                ('facet_normal', c_dp), ('facet_face_off', c_ip), ('facet_face_idx', c_ip),
                ('tol', C.c_double), ('bbox', C.c_double * 6),
                ('nS', C.c_int32), ('simplex_pts', c_dp), ('simplex_vol', c_dp)]


class nk_subvols(C.Structure):
    _fields_ = [('S', C.c_int32), ('kind', C.c_int32), ('axis', C.c_int32), ('interp', C.c_int32),
                ('centers', c_dp), ('volumes', c_dp), ('rbf_inv', c_dp), ('rbf_shift', c_dp), ('rbf_scale', c_dp),
                ('rbf_used', C.c_int32 * 3)]


class nk_reservoirs(C.Structure):
    _fields_ = [('R', C.c_int32), ('facet', c_ip), ('T', c_dp), ('enter_prob', c_dp), ('counter', c_dp),
                ('gen', C.c_int32), ('n_leaving', C.POINTER(C.c_int64))]


class nk_rough(C.Structure):
    _fields_ = [('Fr', C.c_int32), ('facet', c_ip), ('specularity', c_dp), ('true_spec', c_up),
                ('spec_map', c_ip), ('roulette', c_dp), ('degen_j2', c_ip)]


class nk_params(C.Structure):
    _fields_ = [('dt', C.c_double), ('norm_fixed', C.c_int32), ('particle_density', C.c_double),
                ('T_ref_local', C.c_int32), ('T_ref', C.c_double), ('flux_every', C.c_int32),
                ('contains_every', C.c_int32), ('track_ids', C.c_int32)]


class nk_tally(C.Structure):
    _fields_ = [('T_sv', c_dp), ('E_sv', c_dp), ('E_raw', c_dp), ('N_sv', c_dp), ('flux_raw', c_dp),
                ('N_leaving', c_dp), ('res_energy', c_dp), ('res_flux', c_dp), ('N_emitted', c_dp)]


class nk_timing(C.Structure):
    _fields_ = [('step_kernel_ms', C.c_double), ('emit_kernel_ms', C.c_double), ('events_kernel_ms', C.c_double),
                ('total_ms', C.c_double),
                ('slots', C.c_int64), ('live', C.c_int64),
                ('regrows', C.c_int64), ('halts', C.c_int64), ('tau_rebuilds', C.c_int64), ('batches', C.c_int64),
                ('emit_fused', C.c_int64), ('place_tries', C.c_int64), ('place_gbps', C.c_double), ('place_worst_gbps', C.c_double),
                ('box_store', C.c_int64)]


class nk_comm_report(C.Structure):
    _fields_ = [('rank', C.c_int32), ('nranks', C.c_int32), ('comm_rank', C.c_int32), ('comm_nranks', C.c_int32),
                ('device', C.c_int32), ('selftest_ok', C.c_int32), ('selftest_sum', C.c_double), ('pci_bus_id', C.c_char * 32)]


EXPORTS = ['nk_device_count', 'nk_create', 'nk_destroy', 'nk_last_error', 'nk_set_material', 'nk_set_mesh', 'nk_set_subvolumes',
           'nk_set_reservoirs', 'nk_set_rough', 'nk_set_params', 'nk_reserve', 'nk_upload_particles',
           'nk_init_boundaries', 'nk_step', 'nk_download_particles', 'nk_get_subvol_temperature',
           'nk_set_subvol_temperature', 'nk_get_step', 'nk_get_timing', 'nk_comm_unique_id', 'nk_comm_init',
           'nk_find_boundary', 'nk_find_boundary_from', 'nk_tree_info', 'nk_classify', 'nk_box_hit', 'nk_eval', 'nk_mode_segments', 'nk_reflect', 'nk_uniform2', 'nk_calibrate_stream',
           'nk_specular_begin', 'nk_specular_pairs', 'nk_specular_end', 'nk_rough_begin', 'nk_rough_pairs', 'nk_rough_finish',
           'nk_rough_download', 'nk_build_enter_prob', 'nk_init_particles', 'nk_tally_state', 'nk_kspec_begin', 'nk_kspec_pairs',
           'nk_rough_finish_k', 'nk_mesh_crossings', 'nk_comm_info', 'nk_comm_allreduce', 'nk_set_bands', 'nk_get_band_rows',
           'nk_tally_bands_state', 'nk_set_field', 'nk_get_field', 'nk_tally_field_state', 'nk_field_info',
           'nk_set_field_groups', 'nk_get_field_groups', 'nk_tally_field_groups_state', 'nk_field_groups_info',
           'nk_set_modes', 'nk_get_modes', 'nk_tally_modes_state', 'nk_modes_info',
           'nk_group_create', 'nk_group_destroy', 'nk_group_step', 'nk_group_info', 'nk_group_last_error',
           'nk_cell_solid_volume', 'nk_solid_last_error', 'nk_free_paths', 'nk_free_paths_info', 'nk_free_paths_columns',
           'nk_free_paths_map', 'nk_free_paths_map_info', 'nk_kinetic_flights', 'nk_kinetic_flights_groups', 'nk_kinetic_flights_map']

class nk_field(C.Structure):
    _fields_ = [('lo', C.c_double * 3), ('h', C.c_double * 3), ('n', C.c_int32 * 3), ('every', C.c_int32), ('flags', C.c_int32),
                ('capacity', C.c_int64)]


class nk_field_report(C.Structure):
    _fields_ = [('n', C.c_int32 * 3), ('every', C.c_int32), ('ncells', C.c_int64), ('k_E', C.c_int32), ('k_F', C.c_int32),
                ('B_E', C.c_double), ('B_F', C.c_double), ('capacity', C.c_int64), ('bytes', C.c_int64),
                ('lds_path', C.c_int32), ('on', C.c_int32)]


class nk_field_groups_report(C.Structure):
    _fields_ = [('G', C.c_int32), ('lds_path', C.c_int32), ('lines', C.c_int64), ('bytes', C.c_int64), ('k_E', C.c_int32),
                ('k_F', C.c_int32), ('permutes', C.c_int64), ('on', C.c_int32), ('pad_', C.c_int32)]


class nk_modes(C.Structure):
    _fields_ = [('every', C.c_int32), ('flags', C.c_int32), ('capacity', C.c_int64)]


class nk_modes_report(C.Structure):
    _fields_ = [('every', C.c_int32), ('k_E', C.c_int32), ('B_E', C.c_double), ('capacity', C.c_int64), ('bytes', C.c_int64),
                ('owner_path', C.c_int32), ('on', C.c_int32)]


class nk_tree_report(C.Structure):
    _fields_ = [('NG', C.c_int32), ('tree_top', C.c_int32), ('level_nodes', C.c_int32 * 8), ('tree_base', C.c_int32 * 8),
                ('top_family', C.c_int32), ('tree_leaves', C.c_int32), ('references', C.c_int32), ('pad_slots', C.c_int32),
                ('n_families', C.c_int32), ('pad_', C.c_int32), ('tree_bound', C.c_double)]


class nk_solid_report(C.Structure):
    _fields_ = [('ncells', C.c_int64), ('pairs', C.c_int64), ('k_A', C.c_int32), ('k_P', C.c_int32), ('seconds', C.c_double)]


class nk_free_path_args(C.Structure):
    _fields_ = [('n_modes', C.c_int32), ('modes', c_ip), ('n_samples', C.c_int32), ('max_segments', C.c_int32),
                ('w_min', C.c_double), ('tau', c_dp), ('x0', c_dp), ('seed', C.c_uint64)]


class nk_free_path_modes(C.Structure):
    _fields_ = [('D', c_dp), ('D2', c_dp), ('T', c_dp), ('hits', c_dp), ('p_res', c_dp), ('p_wall', c_dp), ('w_left', c_dp),
                ('p_int', c_dp)]


class nk_free_path_rays(C.Structure):
    _fields_ = [('D', c_dp), ('T', c_dp), ('segments', c_ip), ('end', c_ip), ('x0', c_dp)]


class nk_free_path_report(C.Structure):
    _fields_ = [('rays', C.c_int64), ('casts', C.c_int64), ('missed', C.c_int64), ('capped', C.c_int64),
                ('geometry_mode', C.c_int32), ('calls', C.c_int32), ('bytes', C.c_int64), ('seconds', C.c_double)]


FREE_PATH_MAX_COLUMNS = 32   # NK_FREE_PATH_MAX_COLUMNS (include/nanokappa_hip.h)


class nk_free_path_columns_report(C.Structure):
    _fields_ = [('rays', C.c_int64), ('casts_shared', C.c_int64), ('casts', C.c_int64 * FREE_PATH_MAX_COLUMNS),
                ('missed', C.c_int64 * FREE_PATH_MAX_COLUMNS), ('capped', C.c_int64 * FREE_PATH_MAX_COLUMNS),
                ('n_columns', C.c_int32), ('tile', C.c_int32), ('launches', C.c_int32), ('geometry_mode', C.c_int32),
                ('calls', C.c_int32), ('pad_', C.c_int32), ('bytes', C.c_int64), ('seconds', C.c_double)]


FREE_MAP_LINE = 16           # NK_FREE_MAP_LINE


class nk_free_path_grid(C.Structure):
    _fields_ = [('n', C.c_int32 * 3), ('pad_', C.c_int32), ('lo', C.c_double * 3), ('h', C.c_double * 3), ('weight', c_dp),
                ('capacity', C.c_int64), ('weight_bound', C.c_double), ('ray_cell', c_ip), ('ray_w', c_dp)]


class nk_free_path_map_report(C.Structure):
    _fields_ = [('rays', C.c_int64), ('casts', C.c_int64), ('missed', C.c_int64), ('capped', C.c_int64), ('clamped', C.c_int64),
                ('overflow', C.c_int64), ('k_K', C.c_int32), ('k_P', C.c_int32), ('k_T', C.c_int32), ('geometry_mode', C.c_int32),
                ('calls', C.c_int32), ('pad_', C.c_int32), ('B_K', C.c_double), ('B_T', C.c_double), ('bytes', C.c_int64),
                ('seconds', C.c_double)]


KIN_MAX_SOURCES = 8          # NK_KIN_MAX_SOURCES (include/nanokappa_hip.h)
KIN_ROW_WORDS = 32           # NK_KIN_ROW_WORDS
KIN_MAX_GROUPS = 256         # NK_KIN_MAX_GROUPS
KIN_MAX_GROUP_WORDS = 1 << 24  # NK_KIN_MAX_GROUP_WORDS
KIN_ROW_CLAMPED = 25         # NK_KIN_ROW_CLAMPED
KIN_MAX_MAP_CELLS = 1 << 24  # NK_KIN_MAX_MAP_CELLS
KIN_MAX_MAP_WORDS = 1 << 27  # NK_KIN_MAX_MAP_WORDS


class nk_kinetic_args(C.Structure):
    _fields_ = [('n_samples', C.c_int32), ('max_events', C.c_int32), ('rays_per_wave', C.c_int32), ('no_bins', C.c_int32),
                ('tau', c_dp), ('cdf_scatter', c_dp), ('cdf_flux', c_dp), ('seed', C.c_uint64)]


class nk_kinetic_out(C.Structure):
    _fields_ = [('rows', C.POINTER(C.c_int64)), ('sub', C.POINTER(C.c_int64))]


class nk_kinetic_groups(C.Structure):
    _fields_ = [('n_groups', C.c_int32), ('group_of_mode', c_ip)]


class nk_kinetic_group_out(C.Structure):
    _fields_ = [('grp', C.POINTER(C.c_int64))]


class nk_kinetic_grid(C.Structure):
    _fields_ = [('n', C.c_int32 * 3), ('pad_', C.c_int32), ('lo', C.c_double * 3), ('h', C.c_double * 3)]


class nk_kinetic_map_out(C.Structure):
    _fields_ = [('cells', C.POINTER(C.c_int64))]


class nk_kinetic_rays(C.Structure):
    _fields_ = [('x0', c_dp), ('mode', c_ip), ('end', c_ip), ('events', c_ip), ('casts', c_ip), ('D', c_dp), ('dwell', c_dp),
                ('hash', c_u64p)]


class nk_kinetic_report(C.Structure):
    _fields_ = [('rays', C.c_int64), ('events', C.c_int64), ('casts', C.c_int64), ('lost', C.c_int64), ('missed', C.c_int64),
                ('capped', C.c_int64), ('overflow', C.c_int64), ('n_sources', C.c_int32), ('n_subvolumes', C.c_int32),
                ('source_facet', C.c_int32 * KIN_MAX_SOURCES), ('k_D', C.c_int32), ('k_D2', C.c_int32), ('k_T', C.c_int32),
                ('k_t', C.c_int32), ('k_x', C.c_int32), ('geometry_mode', C.c_int32), ('lds_bins', C.c_int32), ('grid', C.c_int32),
                ('calls', C.c_int32), ('pad_', C.c_int32), ('B_t', C.c_double), ('B_x', C.c_double), ('bytes', C.c_int64),
                ('seconds', C.c_double)]


class nk_group_report(C.Structure):
    _fields_ = [('R', C.c_int32), ('halted', C.c_int32), ('finished_alone', C.c_int32), ('grid_sweep', C.c_int32),
                ('grid_tail', C.c_int32), ('pad_', C.c_int32), ('steps', C.c_int64), ('sweep_launches', C.c_int64),
                ('tail_launches', C.c_int64), ('member_launches', C.c_int64), ('sweep_kernel_ms', C.c_double),
                ('tail_kernel_ms', C.c_double), ('total_ms', C.c_double)]


ERR_ARG = -2                 # NK_ERR_ARG (include/nanokappa_hip.h)
ERR_CAPACITY = -3            # NK_ERR_CAPACITY
GROUP_MAX_MEMBERS = 32       # NK_GROUP_MAX_MEMBERS
MODES_GLOBAL = 1             # nk_set_modes flags (include/nanokappa_hip.h)
MODES_TEST_SMALL_BOUND = 2
FIELD_GLOBAL = 1             # nk_set_field flags (include/nanokappa_hip.h)
FIELD_TEST_SMALL_BOUND = 2

_lib = None


def load_library(path=None, optional=()):
    """Load libnanokappa_hip.so; raises NkError with build instructions when it is missing.  path: another build of the library
    (a developer's A/B run, Engine(library=...)): loaded beside the package's own and not kept; `optional` names entry points that
    build may lack (one from before they existed) -- calling one of those raises AttributeError."""
    global _lib
    if path is not None:
        if not os.path.exists(path):
            raise NkError('%s not found' % path)
        return _bind(C.CDLL(path), tuple(optional))
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NkError('%s not found: build it with `make -C %s` (needs hipcc); there is no CPU fallback'
                      % (LIB_PATH, os.path.join(_HERE, 'csrc')))
    _lib = _bind(C.CDLL(LIB_PATH), ())
    return _lib


def _bind(L, optional):
    L.nk_last_error.restype = C.c_char_p
    L.nk_last_error.argtypes = [C.c_void_p]
    L.nk_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_uint64]
    L.nk_destroy.argtypes = [C.c_void_p]
    L.nk_destroy.restype = None
    for name, st in (('nk_set_material', nk_material), ('nk_set_mesh', nk_mesh), ('nk_set_reservoirs', nk_reservoirs),
                     ('nk_set_rough', nk_rough), ('nk_set_params', nk_params)):
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(st)]
    L.nk_set_subvolumes.argtypes = [C.c_void_p, C.POINTER(nk_subvols), c_dp]
    L.nk_reserve.argtypes = [C.c_void_p, C.c_int64]
    L.nk_upload_particles.argtypes = [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp, c_ip, c_dp, c_dp, c_ip, c_u64p, C.c_uint64]
    L.nk_init_boundaries.argtypes = [C.c_void_p]
    L.nk_init_particles.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, c_ip, C.c_int64, C.POINTER(C.c_int64)]
    L.nk_tally_state.argtypes = [C.c_void_p, c_dp, c_dp, c_dp]
    L.nk_mesh_crossings.argtypes = [C.c_int, C.c_int64, c_dp, c_dp, C.c_int64, c_dp, c_dp, c_dp, C.c_int, c_ip]
    L.nk_step.argtypes = [C.c_void_p, C.c_int32, C.POINTER(nk_tally)]
    L.nk_download_particles.argtypes = [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp, c_ip, c_dp, c_dp, c_ip, c_u64p,
                                        C.POINTER(C.c_int64)]
    L.nk_get_subvol_temperature.argtypes = [C.c_void_p, c_dp]
    L.nk_set_subvol_temperature.argtypes = [C.c_void_p, c_dp]
    L.nk_get_step.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.nk_get_timing.argtypes = [C.c_void_p, C.POINTER(nk_timing)]
    L.nk_comm_unique_id.argtypes = [C.c_void_p]
    L.nk_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.nk_comm_info.argtypes = [C.c_void_p, C.POINTER(nk_comm_report)]
    L.nk_comm_allreduce.argtypes = [C.c_void_p, c_dp, C.c_int64]
    L.nk_find_boundary.argtypes = [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp, c_dp, c_ip]
    L.nk_find_boundary_from.argtypes = [C.c_void_p, C.c_int64, c_dp, c_dp, c_ip, c_dp, c_dp, c_ip, c_ip]
    L.nk_tree_info.argtypes = [C.c_void_p, C.POINTER(nk_tree_report), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.nk_classify.argtypes = [C.c_void_p, C.c_int64, c_dp, c_ip]
    L.nk_box_hit.argtypes = [C.c_void_p, C.c_int32, C.c_int64, c_dp, c_dp, c_dp, c_ip]
    L.nk_eval.argtypes = [C.c_void_p, C.c_int32, C.c_int64, c_dp, c_ip, c_dp]
    L.nk_mode_segments.argtypes = [C.c_void_p, c_ip, C.POINTER(C.c_int32)]
    L.nk_reflect.argtypes = [C.c_void_p, C.c_int64, c_ip, c_ip, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, c_dp, c_dp]
    L.nk_uniform2.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, c_dp, c_dp]
    L.nk_calibrate_stream.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.nk_specular_begin.argtypes = [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp]
    L.nk_specular_pairs.argtypes = [C.c_void_p, c_dp, C.c_double, C.c_int64, c_ip, c_ip, C.POINTER(C.c_int64)]
    L.nk_specular_end.argtypes = [C.c_void_p]
    L.nk_rough_begin.argtypes = [C.c_void_p, C.c_int32, c_ip, c_dp, c_dp, c_dp]
    L.nk_rough_pairs.argtypes = [C.c_void_p, C.c_int32, c_ip]
    L.nk_rough_finish.argtypes = [C.c_void_p]
    L.nk_rough_finish_k.argtypes = [C.c_void_p, C.c_int32, c_ip, c_ip]
    L.nk_kspec_begin.argtypes = [C.c_void_p, C.c_int64, c_dp, c_dp, c_dp, c_dp]
    L.nk_kspec_pairs.argtypes = [C.c_void_p, c_dp, C.c_int64, c_ip, c_ip, C.POINTER(C.c_int64)]
    L.nk_rough_download.argtypes = [C.c_void_p, c_dp, c_up, c_ip, c_dp]
    L.nk_build_enter_prob.argtypes = [C.c_void_p, C.c_int32, c_dp, c_dp, C.c_double, c_dp]
    L.nk_set_bands.argtypes = [C.c_void_p, C.c_int32, c_ip]
    L.nk_get_band_rows.argtypes = [C.c_void_p, c_dp, c_dp, C.POINTER(C.c_int64), C.c_int32, c_ip]
    L.nk_tally_bands_state.argtypes = [C.c_void_p, c_dp, c_dp]
    c_i64p = C.POINTER(C.c_int64)
    L.nk_set_field.argtypes = [C.c_void_p, C.POINTER(nk_field)]
    L.nk_get_field.argtypes = [C.c_void_p, c_dp, c_dp, c_dp, c_i64p, c_i64p, C.c_int32]
    L.nk_tally_field_state.argtypes = [C.c_void_p, c_i64p, c_i64p]
    L.nk_field_info.argtypes = [C.c_void_p, C.POINTER(nk_field_report)]
    L.nk_set_field_groups.argtypes = [C.c_void_p, C.c_int32, c_ip]
    L.nk_get_field_groups.argtypes = [C.c_void_p, c_dp, c_dp, c_dp, c_i64p, c_i64p, C.c_int32]
    L.nk_tally_field_groups_state.argtypes = [C.c_void_p, c_i64p, c_i64p, c_i64p]
    L.nk_field_groups_info.argtypes = [C.c_void_p, C.POINTER(nk_field_groups_report)]
    L.nk_set_modes.argtypes = [C.c_void_p, C.POINTER(nk_modes)]
    L.nk_get_modes.argtypes = [C.c_void_p, c_dp, c_dp, c_i64p, c_i64p, C.c_int32]
    L.nk_tally_modes_state.argtypes = [C.c_void_p, c_i64p, c_i64p]
    L.nk_modes_info.argtypes = [C.c_void_p, C.POINTER(nk_modes_report)]
    L.nk_group_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32]
    L.nk_group_destroy.argtypes = [C.c_void_p]
    L.nk_group_destroy.restype = None
    L.nk_group_step.argtypes = [C.c_void_p, C.c_int32, C.POINTER(nk_tally)]
    L.nk_group_info.argtypes = [C.c_void_p, C.POINTER(nk_group_report)]
    L.nk_group_last_error.restype = C.c_char_p
    L.nk_group_last_error.argtypes = [C.c_void_p]
    L.nk_cell_solid_volume.argtypes = [C.c_int, C.c_int64, c_dp, c_dp, c_dp, c_ip, c_dp, C.POINTER(nk_solid_report)]
    L.nk_solid_last_error.restype = C.c_char_p
    L.nk_solid_last_error.argtypes = []
    L.nk_free_paths.argtypes = [C.c_void_p, C.POINTER(nk_free_path_args), C.POINTER(nk_free_path_modes), C.POINTER(nk_free_path_rays),
                                C.POINTER(nk_free_path_report)]
    L.nk_free_paths_info.argtypes = [C.c_void_p, C.POINTER(nk_free_path_report)]
    L.nk_free_paths_map.argtypes = [C.c_void_p, C.POINTER(nk_free_path_args), C.POINTER(nk_free_path_grid), C.POINTER(C.c_int64),
                                    C.POINTER(nk_free_path_modes), C.POINTER(nk_free_path_rays), C.POINTER(nk_free_path_map_report)]
    L.nk_free_paths_map_info.argtypes = [C.c_void_p, C.POINTER(nk_free_path_map_report)]
    L.nk_free_paths_columns.argtypes = [C.c_void_p, C.POINTER(nk_free_path_args), C.c_int32, C.POINTER(nk_free_path_modes),
                                        C.POINTER(nk_free_path_rays), C.POINTER(nk_free_path_columns_report)]
    L.nk_kinetic_flights.argtypes = [C.c_void_p, C.POINTER(nk_kinetic_args), C.POINTER(nk_kinetic_out), C.POINTER(nk_kinetic_rays),
                                     C.POINTER(nk_kinetic_report)]
    if 'nk_kinetic_flights_groups' not in optional or hasattr(L, 'nk_kinetic_flights_groups'):
        L.nk_kinetic_flights_groups.argtypes = [C.c_void_p, C.POINTER(nk_kinetic_args), C.POINTER(nk_kinetic_groups), C.POINTER(nk_kinetic_out),
                                                C.POINTER(nk_kinetic_group_out), C.POINTER(nk_kinetic_rays), C.POINTER(nk_kinetic_report)]
    if 'nk_kinetic_flights_map' not in optional or hasattr(L, 'nk_kinetic_flights_map'):
        L.nk_kinetic_flights_map.argtypes = [C.c_void_p, C.POINTER(nk_kinetic_args), C.POINTER(nk_kinetic_grid), C.POINTER(nk_kinetic_out),
                                             C.POINTER(nk_kinetic_map_out), C.POINTER(nk_kinetic_rays), C.POINTER(nk_kinetic_report)]
    return L


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t=c_dp):
    return None if a is None else a.ctypes.data_as(t)


def bc_codes(bound_cond):
    """'T'/'P'/'R' strings (Geometry.bound_cond) or int8 codes -> int8 codes."""
    a = np.asarray(bound_cond)
    if a.dtype.kind in 'US':
        return np.array([ord(str(c)[0]) for c in a], dtype=np.int8)
    return np.ascontiguousarray(a, dtype=np.int8)


def device_count():
    """HIP devices this process sees."""
    return int(load_library().nk_device_count())


def _set_up_device(L, device):
    """The device of a context-free set-up helper: NK_MESH_DEVICE, else LOCAL_RANK, modulo the devices this process sees."""
    if device is None:
        device = int(os.environ.get('NK_MESH_DEVICE', os.environ.get('LOCAL_RANK', '0')))
        nd = L.nk_device_count()
        device = device % nd if nd > 0 else 0
    return int(device)


def mesh_crossings(origins, dirs, v0, e1, e2, skip_self=False, device=None):
    """Triangles crossed by every open ray (nk_mesh_crossings; -1 where a ray has too many distinct crossings).
    device: HIP device index; default NK_MESH_DEVICE, else this process's LOCAL_RANK (a rank's geometry set-up stays on the
    rank's own GPU), modulo the devices this process sees."""
    L = load_library()
    device = _set_up_device(L, device)
    o, d = _d(origins), _d(dirs)
    a, b, c = _d(v0), _d(e1), _d(e2)
    out = np.zeros(o.shape[0], dtype=np.int32)
    rc = L.nk_mesh_crossings(int(device), o.shape[0], _p(o), _p(d), a.shape[0], _p(a), _p(b), _p(c), int(bool(skip_self)), _p(out, c_ip))
    if rc != 0:
        raise RuntimeError('nk_mesh_crossings failed (%d)' % rc)
    return out


def cell_solid_volume(vertices, faces, lo, h, n, device=None, report=False):
    """Volume of solid in every cell of the grid lo / h / n, (nx, ny, nz) float64, for a closed triangle mesh with outward
    faces (mesh.Mesh's vertices / faces), exact for the triangles (nk_cell_solid_volume; field.solid_volume is the same rule
    in NumPy).  device as for mesh_crossings.  report=True: (V, dict ncells, pairs, k_A, k_P, seconds).  NkError, with the
    library's text, for no faces, h <= 0, more than 2^24 cells or a grid that does not contain the mesh."""
    L = load_library()
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tri = _d(v[f]) if f.shape[0] else np.zeros(9)
    lo3, h3 = _d(np.asarray(lo, dtype=np.float64).reshape(3)), _d(np.asarray(h, dtype=np.float64).reshape(3))
    n3 = _i(np.asarray(n).reshape(3))
    nc = int(n3[0]) * int(n3[1]) * int(n3[2])
    V = np.zeros(nc if 0 < nc <= (1 << 24) and int(n3.min()) > 0 else 1)        # (a bad grid is refused before V is touched)
    rep = nk_solid_report()
    rc = L.nk_cell_solid_volume(_set_up_device(L, device), f.shape[0], _p(tri), _p(lo3), _p(h3), _p(n3, c_ip), _p(V), C.byref(rep))
    if rc != 0:
        raise NkError('nk_cell_solid_volume failed (%d): %s' % (rc, L.nk_solid_last_error().decode()))
    V = V.reshape(tuple(int(k) for k in n3))
    if report:
        return V, dict(ncells=int(rep.ncells), pairs=int(rep.pairs), k_A=int(rep.k_A), k_P=int(rep.k_P), seconds=float(rep.seconds))
    return V


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, every rank passes it to Engine.comm_init)."""
    L = load_library()
    buf = C.create_string_buffer(128)
    rc = L.nk_comm_unique_id(buf)
    if rc != 0:
        raise NkError('nk_comm_unique_id failed: %s' % L.nk_last_error(None).decode())
    return buf.raw


class Engine(object):
    """One nk_ctx: tables + particle store on one MI355X."""

    def __init__(self, device=0, seed=0, library=None):
        self.L = library if library is not None else load_library()           # library: load_library(path)'s, for A/B runs
        h = C.c_void_p()
        rc = self.L.nk_create(C.byref(h), int(device), C.c_uint64(int(seed)))
        if rc != 0:
            raise NkError('nk_create failed (%d): %s' % (rc, self.L.nk_last_error(None).decode()))
        self.h = h
        self.S = self.R = self.J = self.M = 0
        self.nbands = 0

    def close(self):
        if getattr(self, 'h', None):
            self.L.nk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise NkError('%s failed (%d): %s' % (what, rc, self.L.nk_last_error(self.h).decode()))

    # ------------------------------------------------------------------ tables
    def set_material(self, t):
        """t: Phonon.tables()"""
        m = nk_material()
        om, vg, tg, lt = _d(t['omega']), _d(t['group_vel']), _d(t['T_grid']), _d(t['lifetime'])
        ta, ea = _d(t['T_array']), _d(t['energy_array'])
        m.Q, m.J = om.shape
        m.NT = tg.shape[0]
        m.omega, m.group_vel, m.T_grid, m.lifetime = _p(om), _p(vg), _p(tg), _p(lt)
        m.nE = ta.shape[0]
        m.T_fill_lo, m.T_fill_hi = float(tg.min()), float(tg.max())
        m.T_array, m.energy_array = _p(ta), _p(ea)
        m.hbar, m.kb, m.QV = float(t['hbar']), float(t['kb']), float(t['QV'])
        m.active_modes = int(t['active_modes'])
        self._ck(self.L.nk_set_material(self.h, C.byref(m)), 'nk_set_material')
        self.J = int(m.J)
        self.M = int(m.Q * m.J)
        self._vg = vg.reshape(-1, 3).copy()            # (free_paths: the default mode list)

    def set_mesh(self, g):
        """g: mapping with the reference's Mesh/Geometry attribute names (face_normals, face_k, face_bounds,
        face_basis_matrix, face_origins, face_facets, vertices, faces, face_areas, bound_cond, connected_facets,
        facet_centroid, facets_normal, facets | facets_flat+facets_len, bounds, simplices*)."""
        m = nk_mesh()
        nrm, k = _d(g['face_normals']), _d(g['face_k'])
        fb = np.asarray(g['face_bounds'], dtype=np.float64)
        lo, hi = _d(fb[0]), _d(fb[1])
        basis, org, ff = _d(g['face_basis_matrix']), _d(g['face_origins']), _i(g['face_facets'])
        verts = _d(np.asarray(g['vertices'])[np.asarray(g['faces'], dtype=int)])
        area = _d(g['face_areas'])
        m.F = nrm.shape[0]
        m.normals, m.k, m.bounds_lo, m.bounds_hi = _p(nrm), _p(k), _p(lo), _p(hi)
        m.basis, m.origins, m.face_facet, m.vertices, m.face_area = _p(basis), _p(org), _p(ff, c_ip), _p(verts), _p(area)
        bc = bc_codes(g['bound_cond'])
        Fc = bc.shape[0]
        partner = -np.ones(Fc, dtype=np.int32)
        for a, b in np.asarray(g.get('connected_facets', np.zeros((0, 2))), dtype=int).reshape(-1, 2):
            partner[a], partner[b] = b, a
        cen, fn = _d(g['facet_centroid']), _d(g['facets_normal'])
        if 'facets_flat' in g:
            flat, ln = _i(g['facets_flat']), np.asarray(g['facets_len'], dtype=int)
        else:
            flat, ln = _i(np.concatenate(g['facets'])), np.array([len(f) for f in g['facets']])
        off = _i(np.concatenate(([0], np.cumsum(ln))))
        m.Fc = Fc
        m.facet_bc, m.facet_partner, m.facet_centroid, m.facet_normal = _p(bc, c_bp), _p(partner, c_ip), _p(cen), _p(fn)
        m.facet_face_off, m.facet_face_idx = _p(off, c_ip), _p(flat, c_ip)
        m.tol = float(g.get('tol', 1e-10))
        b = np.asarray(g['bounds'], dtype=np.float64)
        for d in range(3):
            m.bbox[d], m.bbox[3 + d] = b[0, d], b[1, d]
        if 'simplices' in g and len(g['simplices']):
            sp = _d(np.asarray(g['simplices_points'])[np.asarray(g['simplices'], dtype=int)])
            sv = _d(g['simplices_volumes'])
            m.nS = sv.shape[0]
            m.simplex_pts, m.simplex_vol = _p(sp), _p(sv)
        else:
            m.nS = 0
        self._ck(self.L.nk_set_mesh(self.h, C.byref(m)), 'nk_set_mesh')

    def set_subvolumes(self, centers, volumes, kind, axis, interp, T_sv, rbf=None):
        """interp 3 (cubic RBF) needs rbf = (inv, shift, scale, used) from setup_tables.rbf_system."""
        s = nk_subvols()
        c, v, t = _d(centers), _d(volumes), _d(T_sv)
        s.S = c.shape[0]
        s.kind, s.axis, s.interp = int(kind), int(axis), int(interp)
        s.centers, s.volumes = _p(c), _p(v)
        if rbf is not None:
            inv, sh, sc = _d(rbf[0]), _d(rbf[1]), _d(rbf[2])
            s.rbf_inv, s.rbf_shift, s.rbf_scale = _p(inv), _p(sh), _p(sc)
            for k in range(3):
                s.rbf_used[k] = int(rbf[3][k])
        self._ck(self.L.nk_set_subvolumes(self.h, C.byref(s), _p(t)), 'nk_set_subvolumes')
        self.S = int(s.S)

    def set_reservoirs(self, facets, T, enter_prob, counter, gen=0, n_leaving=None):
        """gen: 0 'constant', 1 'fixed_rate', 2 'one_to_one' (needs n_leaving[R], the first step's emission)."""
        r = nk_reservoirs()
        f, t, ep, cn = _i(facets), _d(T), _d(enter_prob), _d(counter)
        r.R = f.shape[0]
        r.facet, r.T, r.enter_prob, r.counter = _p(f, c_ip), _p(t), _p(ep), _p(cn)
        r.gen = int(gen)
        nl = None if n_leaving is None else np.ascontiguousarray(n_leaving, dtype=np.int64)
        r.n_leaving = None if nl is None else nl.ctypes.data_as(C.POINTER(C.c_int64))
        self._ck(self.L.nk_set_reservoirs(self.h, C.byref(r)), 'nk_set_reservoirs')
        self.R = int(r.R)

    def set_rough(self, facets, specularity, true_spec, spec_map, roulette, degen_j2=None):
        r = nk_rough()
        f, sp, ts = _i(facets), _d(specularity), np.ascontiguousarray(true_spec, dtype=np.uint8)
        sm, ro = _i(spec_map), _d(roulette)
        dj = None if degen_j2 is None else _i(degen_j2)
        r.Fr = f.shape[0]
        r.facet, r.specularity, r.true_spec, r.spec_map, r.roulette = _p(f, c_ip), _p(sp), _p(ts, c_up), _p(sm, c_ip), _p(ro)
        r.degen_j2 = _p(dj, c_ip)
        self._ck(self.L.nk_set_rough(self.h, C.byref(r)), 'nk_set_rough')

    def set_params(self, dt=1.0, norm_fixed=False, particle_density=0.0, T_ref=None, flux_every=10, contains_every=100,
                   track_ids=False):
        """track_ids: store 64-bit particle ids even when nothing draws random numbers per particle (then downloads
        return them; otherwise pid comes back as zeros unless the mesh has rough facets)."""
        p = nk_params()
        p.track_ids = int(bool(track_ids))
        p.dt, p.norm_fixed, p.particle_density = float(dt), int(bool(norm_fixed)), float(particle_density)
        p.T_ref_local = 1 if T_ref is None else 0
        p.T_ref = 0.0 if T_ref is None else float(T_ref)
        p.flux_every, p.contains_every = int(flux_every), int(contains_every)
        self._ck(self.L.nk_set_params(self.h, C.byref(p)), 'nk_set_params')

    # --------------------------------------------------------------- particles
    def reserve(self, capacity):
        self._ck(self.L.nk_reserve(self.h, int(capacity)), 'nk_reserve')

    def upload(self, positions, mode, occ, n_ts=None, facet=None, pid=None, pid_offset=0):
        pos = np.asarray(positions, dtype=np.float64)
        x, y, z = _d(pos[:, 0]), _d(pos[:, 1]), _d(pos[:, 2])
        m, o = _i(mode), _d(occ)
        nt = None if n_ts is None else _d(n_ts)
        fc = None if facet is None else _i(facet)
        pi = None if pid is None else np.ascontiguousarray(pid, dtype=np.uint64)
        self._ck(self.L.nk_upload_particles(self.h, x.shape[0], _p(x), _p(y), _p(z), _p(m, c_ip), _p(o), _p(nt),
                                            _p(fc, c_ip), _p(pi, c_u64p), C.c_uint64(int(pid_offset))),
                 'nk_upload_particles')

    def init_boundaries(self):
        self._ck(self.L.nk_init_boundaries(self.h), 'nk_init_boundaries')

    def init_particles(self, n, capacity, pid_lo, unique_modes, sv_first=None):
        """initialise_all_particles on the device (tiled modes; sv_first: first particle index of every subvolume's share)."""
        um = _i(unique_modes)
        sf = None if sv_first is None else np.ascontiguousarray(sv_first, dtype=np.int64)
        self._ck(self.L.nk_init_particles(self.h, int(n), int(capacity), int(pid_lo), um.ctypes.data_as(c_ip), um.shape[0],
                                          None if sf is None else sf.ctypes.data_as(C.POINTER(C.c_int64))), 'nk_init_particles')

    def tally_state(self):
        """E_raw[S], N_sv[S], flux_raw[S, 3] of the particles where they stand (this rank's)."""
        S = self.S
        E, N, F = np.zeros(S), np.zeros(S), np.zeros((S, 3))
        self._ck(self.L.nk_tally_state(self.h, E.ctypes.data_as(c_dp), N.ctypes.data_as(c_dp), F.ctypes.data_as(c_dp)), 'nk_tally_state')
        return E, N, F

    def _tally_block(self, nsteps):
        """The dict of per-step arrays step() returns (views of ONE block) and the nk_tally that points into it."""
        S, R = self.S, max(self.R, 0)
        shapes = (('T_sv', (nsteps, S)), ('E_sv', (nsteps, S)), ('E_raw', (nsteps, S)), ('N_sv', (nsteps, S)), ('flux_raw', (nsteps, S, 3)),
                  ('N_leaving', (nsteps, R)), ('res_energy', (nsteps, R)), ('res_flux', (nsteps, R, 3)), ('N_emitted', (nsteps,)))
        total = nsteps * (7 * S + 5 * R + 1)
        block = np.zeros(total if total > 0 else 1)
        base = block.ctypes.data
        out, t, off = {}, nk_tally(), 0
        for k, shp in shapes:
            n = int(np.prod(shp))
            out[k] = block[off:off + n].reshape(shp)
            setattr(t, k, C.cast(base + 8 * off, c_dp))
            off += n
        return out, t

    def step(self, nsteps=1):
        """Run nsteps timesteps; returns a dict of per-step arrays (see nk_tally in the header).  The arrays are views of ONE block
        (a driver that steps one by one calls this a thousand times a second: one allocation and one address instead of nine)."""
        out, t = self._tally_block(nsteps)
        self._ck(self.L.nk_step(self.h, int(nsteps), C.byref(t)), 'nk_step')
        if self.nbands > 0:
            out['band_F'], out['band_N'], out['band_steps'] = self._band_rows()
        return out

    # ------------------------------------------------------- band-resolved heat flux
    def set_bands(self, band_of_mode, nbands):
        """Tally the heat flux per band as well (nk_set_bands): band_of_mode[M] = band of every global mode q*J+j, -1 = none
        (setup_tables.band_map builds the usual ones).  nbands = 0 turns it off.  Then step() also returns, for the heat-flux
        steps of the call, band_F [rows, S, nbands, 3], band_N [rows, S, nbands] and band_steps [rows] (absolute steps)."""
        nbands = int(nbands)
        bm = None if nbands == 0 else _i(band_of_mode).ravel()
        if bm is not None and bm.shape[0] != self.M:
            raise NkError('set_bands: band_of_mode has %d entries, the material %d modes' % (bm.shape[0], self.M))
        self._ck(self.L.nk_set_bands(self.h, nbands, _p(bm, c_ip)), 'nk_set_bands')
        self.nbands = nbands

    def _band_rows(self):
        S, B = self.S, self.nbands
        n = C.c_int32(0)
        self._ck(self.L.nk_get_band_rows(self.h, None, None, None, 0, C.byref(n)), 'nk_get_band_rows')
        r = int(n.value)
        F, N, st = np.zeros((r, S, B, 3)), np.zeros((r, S, B)), np.zeros(r, dtype=np.int64)
        if r > 0:
            self._ck(self.L.nk_get_band_rows(self.h, _p(F), _p(N), st.ctypes.data_as(C.POINTER(C.c_int64)), r, C.byref(n)),
                     'nk_get_band_rows')
        return F, N, st

    def tally_bands_state(self):
        """Band sums of the particles where they stand, after the relaxation, against each particle's interpolated temperature:
        F [S, nbands, 3], N [S, nbands] (nk_tally_bands_state; all ranks)."""
        S, B = self.S, self.nbands
        F, N = np.zeros((S, B, 3)), np.zeros((S, B))
        self._ck(self.L.nk_tally_bands_state(self.h, _p(F), _p(N)), 'nk_tally_bands_state')
        return F, N

    # ------------------------------------------------------- spatial field maps
    def set_field(self, lo, h, n, every, flags=0, capacity=0):
        """Sum particle count, deviational energy and heat flux on a uniform grid of n = (nx, ny, nz) cells of size h from
        corner lo, on every step with (step + 1) % every == 0 (a multiple of flux_every) (nk_set_field; k_field).  n = (0, 0, 0)
        turns it off.  flags: FIELD_GLOBAL forces the global-memory path (same bits as the LDS path).  capacity > 0: derive the
        integer scales for at least this many particle slots (the same k_E, k_F on stores of different sizes)."""
        f = nk_field()
        n = [int(v) for v in np.ravel(n)]
        if len(n) != 3:
            raise NkError('set_field: n must have three entries')
        if any(n):
            lo, h = _d(lo).ravel(), _d(h).ravel()
            if lo.shape[0] != 3 or h.shape[0] != 3:
                raise NkError('set_field: lo and h must have three entries')
            for a in range(3):
                f.lo[a], f.h[a] = lo[a], h[a]
        for a in range(3):
            f.n[a] = n[a]
        f.every, f.flags, f.capacity = int(every), int(flags), int(capacity)
        self._field_n = None
        self._fgroups_G = 0                                 # (nk_set_field switches the groups off)
        self._ck(self.L.nk_set_field(self.h, C.byref(f)), 'nk_set_field')
        self._field_n = tuple(n) if any(n) else None

    def field_info(self):
        """nk_field_info: cells, scales (the integers hold e 2^k_E and v e 2^k_F), bounds, bytes allocated, path in use."""
        r = nk_field_report()
        self._ck(self.L.nk_field_info(self.h, C.byref(r)), 'nk_field_info')
        return dict(n=tuple(r.n), every=int(r.every), ncells=int(r.ncells), k_E=int(r.k_E), k_F=int(r.k_F), B_E=r.B_E, B_F=r.B_F,
                    capacity=int(r.capacity), bytes=int(r.bytes), lds_path=int(r.lds_path), on=int(r.on))

    def field(self, reset=False):
        """The sums over the field steps since the last reset (all ranks): dict N, E (nx, ny, nz), F (nx, ny, nz, 3), samples
        (field steps in the sums) and clamped (particles outside the grid, counted in its edge cells)."""
        if getattr(self, '_field_n', None) is None:
            raise NkError('field: no field was set (set_field)')
        n = self._field_n
        N, E, F = np.zeros(n), np.zeros(n), np.zeros(n + (3,))
        sm, cl = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.nk_get_field(self.h, _p(N), _p(E), _p(F), C.byref(sm), C.byref(cl), 1 if reset else 0), 'nk_get_field')
        return dict(N=N, E=E, F=F, samples=int(sm.value), clamped=int(cl.value))

    def tally_field_state(self):
        """State mode (nk_tally_field_state): the raw integers of the particles where they stand, after the relaxation, e
        against each particle's interpolated temperature.  dict raw (nx, ny, nz, 8) int64 = {N, E 2^k_E, F 2^k_F (3), 0, 0, 0},
        k_E, k_F, clamped, and the reals N, E, F they stand for."""
        if getattr(self, '_field_n', None) is None:
            raise NkError('tally_field_state: no field was set (set_field)')
        n = self._field_n
        raw = np.zeros(n + (8,), dtype=np.int64)
        cl = C.c_int64(0)
        self._ck(self.L.nk_tally_field_state(self.h, raw.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cl)), 'nk_tally_field_state')
        info = self.field_info()
        kE, kF = info['k_E'], info['k_F']
        return dict(raw=raw, k_E=kE, k_F=kF, clamped=int(cl.value), N=raw[..., 0].astype(np.float64),
                    E=np.ldexp(raw[..., 1].astype(np.float64), -kE), F=np.ldexp(raw[..., 2:5].astype(np.float64), -kF))

    # ------------------------------------------------------- grouped field maps
    def set_field_groups(self, group_of_mode, ngroups):
        """The field's sums per (cell, group of modes) (nk_set_field_groups; k_field_groups): group_of_mode [M] gives every
        mode its group in [0, ngroups) or -1 for none.  Needs a field (set_field): grid, cadence and scales are the field's.
        ngroups = 0 turns it off and frees its tables."""
        ngroups = int(ngroups)
        self._fgroups_G = 0
        if ngroups == 0:
            self._ck(self.L.nk_set_field_groups(self.h, 0, None), 'nk_set_field_groups')
            return
        g = _i(np.ravel(group_of_mode))
        if g.shape[0] != self.M:
            raise NkError('set_field_groups: group_of_mode needs one entry per mode (%d), got %d' % (self.M, g.shape[0]))
        self._ck(self.L.nk_set_field_groups(self.h, ngroups, _p(g, c_ip)), 'nk_set_field_groups')
        self._fgroups_G = ngroups

    def field_groups_info(self):
        """nk_field_groups_info: groups, lines (cells x groups), bytes allocated, path in use, the field's scales, and how often
        the table was brought into the segments' order."""
        r = nk_field_groups_report()
        self._ck(self.L.nk_field_groups_info(self.h, C.byref(r)), 'nk_field_groups_info')
        return dict(G=int(r.G), lines=int(r.lines), bytes=int(r.bytes), lds_path=int(r.lds_path), k_E=int(r.k_E), k_F=int(r.k_F),
                    permutes=int(r.permutes), on=int(r.on))

    def _fgroups_shape(self, who):
        if not getattr(self, '_fgroups_G', 0) or getattr(self, '_field_n', None) is None:
            raise NkError('%s: no groups were set (set_field_groups)' % who)
        return self._field_n + (self._fgroups_G,)

    def field_groups(self, reset=False):
        """The sums over the field steps since the last reset (all ranks): dict N, E (nx, ny, nz, G), F (nx, ny, nz, G, 3),
        samples (field steps in the sums) and ungrouped (particles of modes in no group)."""
        n = self._fgroups_shape('field_groups')
        N, E, F = np.zeros(n), np.zeros(n), np.zeros(n + (3,))
        sm, ug = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.nk_get_field_groups(self.h, _p(N), _p(E), _p(F), C.byref(sm), C.byref(ug), 1 if reset else 0), 'nk_get_field_groups')
        return dict(N=N, E=E, F=F, samples=int(sm.value), ungrouped=int(ug.value))

    def tally_field_groups_state(self):
        """State mode (nk_tally_field_groups_state), as tally_field_state: dict raw (nx, ny, nz, G, 8) int64 = {N, E 2^k_E,
        F 2^k_F (3), 0, 0, 0}, k_E, k_F, clamped, ungrouped, and the reals N, E, F they stand for."""
        n = self._fgroups_shape('tally_field_groups_state')
        raw = np.zeros(n + (8,), dtype=np.int64)
        cl, ug = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.nk_tally_field_groups_state(self.h, raw.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(cl), C.byref(ug)),
                 'nk_tally_field_groups_state')
        info = self.field_groups_info()
        kE, kF = info['k_E'], info['k_F']
        return dict(raw=raw, k_E=kE, k_F=kF, clamped=int(cl.value), ungrouped=int(ug.value), N=raw[..., 0].astype(np.float64),
                    E=np.ldexp(raw[..., 1].astype(np.float64), -kE), F=np.ldexp(raw[..., 2:5].astype(np.float64), -kF))

    # ------------------------------------------------------- mode-resolved tally
    def set_modes(self, every, flags=0, capacity=0):
        """Tally energy and particle count per (subvolume, mode) on every step with (step + 1) % every == 0 (a multiple of
        flux_every) (nk_set_modes; k_modes).  every = 0 turns it off and frees its tables.  flags: MODES_GLOBAL forces the
        global-memory path (same bits as the owner path).  capacity > 0: derive the integer scale for at least this many
        particle slots (the same k_E on stores of different sizes)."""
        m = nk_modes()
        m.every, m.flags, m.capacity = int(every), int(flags), int(capacity)
        self._modes_on = False
        self._ck(self.L.nk_set_modes(self.h, C.byref(m)), 'nk_set_modes')
        self._modes_on = int(every) != 0

    def modes_info(self):
        """nk_modes_info: cadence, scale (the integers hold e 2^k_E), bound, bytes allocated, path in use."""
        r = nk_modes_report()
        self._ck(self.L.nk_modes_info(self.h, C.byref(r)), 'nk_modes_info')
        return dict(every=int(r.every), k_E=int(r.k_E), B_E=r.B_E, capacity=int(r.capacity), bytes=int(r.bytes),
                    owner_path=int(r.owner_path), on=int(r.on))

    def modes(self, reset=False):
        """The sums over the mode steps since the last reset (all ranks): dict N, E [S, Q, J], samples (mode steps in the
        sums) and skipped (mode steps dropped because rough-wall migrants were waiting undelivered)."""
        if not getattr(self, '_modes_on', False):
            raise NkError('modes: the mode tally is off (set_modes)')
        shape = (self.S, self.M // self.J, self.J)
        N, E = np.zeros(shape), np.zeros(shape)
        sm, sk = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.nk_get_modes(self.h, _p(N), _p(E), C.byref(sm), C.byref(sk), 1 if reset else 0), 'nk_get_modes')
        return dict(N=N, E=E, samples=int(sm.value), skipped=int(sk.value))

    def tally_modes_state(self):
        """State mode (nk_tally_modes_state): the raw integers of the particles where they stand, after the relaxation, e
        against each particle's interpolated temperature (or T_ref).  dict N_raw, E_raw [S, Q, J] int64 (E 2^k_E), k_E, and
        the reals N, E they stand for."""
        if not getattr(self, '_modes_on', False):
            raise NkError('tally_modes_state: the mode tally is off (set_modes)')
        shape = (self.S, self.M // self.J, self.J)
        N, E = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
        self._ck(self.L.nk_tally_modes_state(self.h, N.ctypes.data_as(C.POINTER(C.c_int64)), E.ctypes.data_as(C.POINTER(C.c_int64))), 'nk_tally_modes_state')
        kE = self.modes_info()['k_E']
        return dict(N_raw=N, E_raw=E, k_E=kE, N=N.astype(np.float64), E=np.ldexp(E.astype(np.float64), -kE))

    # ------------------------------------------------------- free-path sampling
    @staticmethod
    def _free_path_report(r):
        return dict(rays=int(r.rays), casts=int(r.casts), missed=int(r.missed), capped=int(r.capped),
                    geometry_mode=int(r.geometry_mode), calls=int(r.calls), bytes=int(r.bytes), seconds=float(r.seconds))

    def _free_path_call(self, who, tau, n, modes, max_segments, w_min, x0, seed, rays, columns=False):
        """What free_paths, free_path_columns and free_path_map hand to the library.  tau [Q*J], or [K, Q*J] with `columns`;
        modes None = every mode with |v| > 0 and tau > 0 (in at least one column).  `who` opens the messages.  Returns
        (args, modes struct, rays struct or None, out, list or None): out holds the zeroed result arrays the structs point to,
        with a leading K axis for the columns."""
        if columns:
            t = None if tau is None else _d(tau)
            if t is not None and (t.ndim != 2 or (self.M > 0 and t.shape[1] != self.M)):
                raise NkError('%s: taus must be [K, %d] (a row of lifetimes per column), got shape %s' % (who, self.M, t.shape))
            lead = (0 if t is None else min(int(t.shape[0]), FREE_PATH_MAX_COLUMNS),)                 # (a refused call writes nothing)
        else:
            t = None if tau is None else _d(np.ravel(tau))
            if t is not None and self.M > 0 and t.shape[0] != self.M:
                raise NkError('%s: tau has %d entries, the material %d modes' % (who, t.shape[0], self.M))
            lead = ()
        if modes is None and t is not None and self.M > 0 and t.shape[0] > 0:
            modes = np.nonzero((np.abs(self._vg).max(axis=1) > 0) & ((t > 0).any(axis=0) if columns else t > 0))[0]
        ml = None if (modes is None or isinstance(modes, str)) else _i(np.ravel(modes))
        L = self.M if ml is None else int(ml.shape[0])
        nn = max(n, 0)
        xs = None
        if x0 is not None:
            xs = _d(x0)
            if xs.size != L * nn * 3:
                raise NkError('%s: x0 needs %d x %d x 3 entries, got %d' % (who, L, n, xs.size))
        a = nk_free_path_args()
        a.n_modes, a.modes, a.n_samples, a.max_segments = L, _p(ml, c_ip), n, int(max_segments)
        a.w_min, a.tau, a.x0, a.seed = float(w_min), _p(t), _p(xs), int(seed)
        a._keep = (t, xs, ml)                                # (the arrays the pointers refer to)
        rows = lead + (L,)
        out = dict(D=np.zeros(rows + (3,)), D2=np.zeros(rows + (3,)), T=np.zeros(rows), hits=np.zeros(rows), p_res=np.zeros(rows),
                   p_wall=np.zeros(rows), w_left=np.zeros(rows), p_int=np.zeros(rows))
        pm = nk_free_path_modes()
        for k in out:
            setattr(pm, k, _p(out[k]))
        pr = None
        if rays:
            per = rows + (nn,)
            ro = dict(ray_D=np.zeros(per + (3,)), ray_T=np.zeros(per), ray_segments=np.zeros(per, dtype=np.int32),
                      ray_end=np.zeros(per, dtype=np.int32), ray_x0=np.zeros((L, nn, 3)))
            pr = nk_free_path_rays()
            pr.D, pr.T, pr.x0 = _p(ro['ray_D']), _p(ro['ray_T']), _p(ro['ray_x0'])
            pr.segments, pr.end = _p(ro['ray_segments'], c_ip), _p(ro['ray_end'], c_ip)
            out.update(ro)
        return a, pm, pr, out, ml

    def free_paths(self, tau, n=64, modes=None, max_segments=0, w_min=0.0, x0=None, seed=0, rays=False):
        """Free-path sampling (nk_free_paths; k_free_paths): n rays for every mode of `modes` (global indices q*J + j; None =
        every mode with |v| > 0 and tau > 0; 'all' = all Q*J modes), flown along the mode's group velocity until a boundary or the lifetime tau [Q*J] ends them.  x0
        [len(modes), n, 3]: the start points (None: drawn uniformly in the solid on the device); seed 0 = the engine's;
        max_segments 0 = 65536, w_min 0 = 2^-40.  Returns a dict: modes, n, the per-mode sums D, D2 [L, 3], T, hits, p_res,
        p_wall, w_left, p_int [L], and report (rays, casts, missed, capped, geometry_mode, calls, bytes, seconds); with
        rays=True also ray_D [L, n, 3], ray_T, ray_segments, ray_end, ray_x0 (end codes: 0 weight exhausted, 1 reservoir,
        2 diffuse wall, 3 miss, 4 cap).  Touches neither the particles nor the step counter."""
        n = int(n)
        a, pm, pr, out, ml = self._free_path_call('free_paths', tau, n, modes, max_segments, w_min, x0, seed, rays)
        rep = nk_free_path_report()
        self._ck(self.L.nk_free_paths(self.h, C.byref(a), C.byref(pm), C.byref(pr) if pr else None, C.byref(rep)), 'nk_free_paths')
        out.update(modes=(np.arange(self.M, dtype=np.int32) if ml is None else ml.copy()), n=n, report=self._free_path_report(rep))
        return out

    def free_paths_info(self):
        """The report of the last free_paths call on this engine; all zero (calls = 0, bytes = 0) when there was none."""
        rep = nk_free_path_report()
        self._ck(self.L.nk_free_paths_info(self.h, C.byref(rep)), 'nk_free_paths_info')
        return self._free_path_report(rep)

    def free_path_columns(self, taus, n=64, modes=None, max_segments=0, w_min=0.0, x0=None, seed=0, rays=False):
        """Free-path sampling with K lifetime columns (nk_free_paths_columns; k_free_columns): the rays of free_paths, cast once
        and weighed with every row of taus [K, Q*J], 1 <= K <= 32.  Column c of the result is free_paths(taus[c], ...) on the
        same list bit for bit.  modes None = every mode with |v| > 0 and tau > 0 in at least one column; the other arguments as
        free_paths.  Returns a dict: modes, n, columns (K), the per-mode sums with a leading column axis (D, D2 [K, L, 3], T,
        hits, p_res, p_wall, w_left, p_int [K, L]), casts, missed, capped [K] and report (rays, casts_shared -- the casts
        actually made --, n_columns, tile -- the columns that share a cast; more are flown in tiles that repeat the casts --,
        launches, geometry_mode, calls, bytes, seconds); with rays=True also ray_D [K, L, n, 3], ray_T, ray_segments, ray_end
        [K, L, n] and ray_x0 [L, n, 3].  free_sweep.column(res, c) gives column c in the shape of a free_paths result."""
        n = int(n)
        a, pm, pr, out, ml = self._free_path_call('free_path_columns failed (%d)' % ERR_ARG, taus, n, modes, max_segments, w_min, x0, seed, rays, columns=True)
        K = 0 if taus is None else int(np.shape(taus)[0])
        rep = nk_free_path_columns_report()
        self._ck(self.L.nk_free_paths_columns(self.h, C.byref(a), K if taus is not None else 1, C.byref(pm), C.byref(pr) if pr else None, C.byref(rep)),
                 'nk_free_paths_columns')
        out.update(modes=(np.arange(self.M, dtype=np.int32) if ml is None else ml.copy()), n=n, columns=K,
                   casts=np.array(rep.casts[:K], dtype=np.int64), missed=np.array(rep.missed[:K], dtype=np.int64),
                   capped=np.array(rep.capped[:K], dtype=np.int64),
                   report=dict(rays=int(rep.rays), casts_shared=int(rep.casts_shared), n_columns=int(rep.n_columns), tile=int(rep.tile),
                               launches=int(rep.launches), geometry_mode=int(rep.geometry_mode), calls=int(rep.calls),
                               bytes=int(rep.bytes), seconds=float(rep.seconds)))
        return out

    @staticmethod
    def _free_path_map_report(r):
        return dict(rays=int(r.rays), casts=int(r.casts), missed=int(r.missed), capped=int(r.capped), clamped=int(r.clamped),
                    overflow=int(r.overflow), k_K=int(r.k_K), k_P=int(r.k_P), k_T=int(r.k_T), geometry_mode=int(r.geometry_mode),
                    calls=int(r.calls), B_K=float(r.B_K), B_T=float(r.B_T), bytes=int(r.bytes), seconds=float(r.seconds))

    def free_path_map(self, tau, weight, lo, h, n_cells, n=64, modes=None, max_segments=0, w_min=0.0, x0=None, seed=0, rays=True,
                      capacity=0, weight_bound=0.0):
        """Free-path map (nk_free_paths_map; k_free_paths with its map statements): the rays of free_paths(tau, n, modes, ...) binned on the device by the
        cell of their START point on the grid (lo, h, n_cells) -- the field's convention.  weight [L, 3]: per list entry the
        vector w whose products w_a D_b are summed (free_map.weights: C_m v_m / (Q V)); capacity / weight_bound: floors under the
        ray count and under max |weight| when the scales are derived (pin them to add the cells of several calls).  Returns the
        dict of free_paths -- the same bits -- plus cells [nx, ny, nz, 16] int64 (free_map.tally states the layout) and the map's
        report (rays, casts, missed, capped, clamped, overflow, k_K, k_P, k_T, B_K, B_T, geometry_mode, calls, bytes, seconds);
        with rays=True also the per-ray outputs of free_paths and ray_cell [L, n] (flat cell index), ray_w [L, n] (the final weight
        that went to p_res, p_wall or w_left; 0 otherwise).  Touches neither the particles, the step counter, the field nor
        free_paths_info()."""
        n = int(n)
        a, pm, pr, out, ml = self._free_path_call('free_path_map', tau, n, modes, max_segments, w_min, x0, seed, rays)
        L = a.n_modes
        w = None
        if weight is not None:
            w = _d(weight)
            if w.size != L * 3:
                raise NkError('free_path_map: weight needs %d x 3 entries (a vector per list entry), got %d' % (L, w.size))
        nc = [int(k) for k in np.ravel(n_cells)]
        g = nk_free_path_grid()
        g.n[:] = nc
        g.lo[:] = [float(x) for x in np.ravel(lo)]
        g.h[:] = [float(x) for x in np.ravel(h)]
        g.weight, g.capacity, g.weight_bound = _p(w), int(capacity), float(weight_bound)
        ok = min(nc) > 0 and nc[0] * nc[1] * nc[2] <= (1 << 24)         # (a refused call writes nothing)
        cells = np.zeros(tuple(nc) + (FREE_MAP_LINE,) if ok else (1,), dtype=np.int64)
        if rays:
            ro = dict(ray_cell=np.zeros((L, max(n, 0)), dtype=np.int32), ray_w=np.zeros((L, max(n, 0))))
            g.ray_cell, g.ray_w = _p(ro['ray_cell'], c_ip), _p(ro['ray_w'])
            out.update(ro)
        rep = nk_free_path_map_report()
        self._ck(self.L.nk_free_paths_map(self.h, C.byref(a), C.byref(g), cells.ctypes.data_as(C.POINTER(C.c_int64)) if ok else None,
                                          C.byref(pm), C.byref(pr) if pr else None, C.byref(rep)), 'nk_free_paths_map')
        out.update(modes=(np.arange(self.M, dtype=np.int32) if ml is None else ml.copy()), n=n, cells=cells,
                   report=self._free_path_map_report(rep))
        return out

    def free_path_map_info(self):
        """The report of the last free_path_map call on this engine; all zero (calls = 0, bytes = 0) when there was none."""
        rep = nk_free_path_map_report()
        self._ck(self.L.nk_free_paths_map_info(self.h, C.byref(rep)), 'nk_free_paths_map_info')
        return self._free_path_map_report(rep)

    # ------------------------------------------------------- kinetic flights
    def kinetic_flights(self, tau, c, n=65536, max_events=0, seed=0, rays=False, rays_per_wave=0, lds_bins=True, groups=None, grid=None):
        """Kinetic flights (nk_kinetic_flights; k_kinetic): n energy packets from every 'T' facet, flown, scattered (tau [Q*J], drawn
        in proportion to c / tau, c [Q*J] the volumetric heat capacity per mode), re-emitted by diffuse walls and absorbed by the
        reservoirs -- the steady linearised BTE in the relaxation-time picture (kinetic.py forms conductances and profiles).
        max_events 0 = 2^20, seed 0 = the engine's; rays_per_wave (0 = 512) sets the launch grid and lds_bins=False sends the
        per-subvolume words straight to memory: neither changes a bit of the result.  Returns a dict: n, source_facet [F], ends
        [F, F] (rays from f absorbed at g), lost, missed, capped, events, casts [F], the sums over a source's rays D, D2 [F, 3] and
        dwell_total [F], per subvolume dwell [F, S] and flux [F, S, 3] (the sum of t v), the raw integers rows [F, 32] and sub
        [F, S, 4] with the report's scales k_*, cdf_scatter, cdf_flux, report; with rays=True also ray_x0 [F, n, 3], ray_mode,
        ray_end (>= 0 the absorbing source, -1 lost, -2 missed, -3 capped), ray_events, ray_casts, ray_D [F, n, 3], ray_dwell and
        ray_hash [F, n].  Touches neither the particles nor the step counter.
        groups = (G, table): kinetic groups (nk_kinetic_flights_groups; kinetic_groups.py) -- table [Q*J] holds the group 0 .. G-1
        of every mode or -1; the result then also holds grp [F, S, G + 1, 4] (int64: sub's words per column, the last column for
        the modes with -1; the columns add up to sub bit for bit, and everything else is what the call without groups returns),
        dwell_g [F, S, G + 1] and flux_g [F, S, G + 1, 3].  Without groups the dict and the entry called are the plain ones.
        grid = (lo, h, n_cells): kinetic maps (nk_kinetic_flights_map; kinetic_map.py) -- every segment's four integers also go to
        the line of (source, cell of the segment's point) on the field's grid; the result then also holds map [F, nx, ny, nz, 4]
        (int64; over the cells it adds up to sub over the subvolumes bit for bit), dwell_map [F, nx, ny, nz], flux_map [F, nx, ny,
        nz, 3] and clamped [F] (points outside the grid, tallied in its edge cells; word 25 of rows); everything else is what the
        call without grid returns.  grid together with groups is refused.  Without grid the dict and the entry called are today's."""
        from . import kinetic as KN
        if grid is not None and groups is not None:
            raise NkError('kinetic_flights: grid and groups were both given: a map per (cell, group) is not built; make one call with '
                          'groups and one with grid under the same seed (rows and sub of the two are the same bits)')
        n = int(n)
        t, cc = _d(np.ravel(tau)), _d(np.ravel(c))
        if self.M > 0 and (t.shape[0] != self.M or cc.shape[0] != self.M):
            raise NkError('kinetic_flights: tau has %d and c %d entries, the material %d modes' % (t.shape[0], cc.shape[0], self.M))
        try:
            cs, cf = KN.tables(cc, t, self._vg)
        except ValueError as e:
            raise NkError('kinetic_flights: %s' % e)
        cs, cf = _d(cs), _d(cf)
        a = nk_kinetic_args()
        a.n_samples, a.max_events, a.rays_per_wave, a.no_bins = n, int(max_events), int(rays_per_wave), 0 if lds_bins else 1
        a.tau, a.cdf_scatter, a.cdf_flux, a.seed = _p(t), _p(cs), _p(cf), int(seed)
        F, S, nn = KIN_MAX_SOURCES, max(self.S, 1), max(n, 0)
        rows, sub = np.zeros((F, KIN_ROW_WORDS), dtype=np.int64), np.zeros(F * S * 4, dtype=np.int64)
        o = nk_kinetic_out()
        o.rows, o.sub = rows.ctypes.data_as(C.POINTER(C.c_int64)), sub.ctypes.data_as(C.POINTER(C.c_int64))
        pr, ro = None, {}
        if rays:
            ro = dict(ray_x0=np.zeros((F, nn, 3)), ray_mode=np.zeros((F, nn), dtype=np.int32), ray_end=np.zeros((F, nn), dtype=np.int32),
                      ray_events=np.zeros((F, nn), dtype=np.int32), ray_casts=np.zeros((F, nn), dtype=np.int32), ray_D=np.zeros((F, nn, 3)),
                      ray_dwell=np.zeros((F, nn)), ray_hash=np.zeros((F, nn), dtype=np.uint64))
            pr = nk_kinetic_rays()
            pr.x0, pr.D, pr.dwell = _p(ro['ray_x0']), _p(ro['ray_D']), _p(ro['ray_dwell'])
            pr.mode, pr.end, pr.events, pr.casts = (_p(ro[k], c_ip) for k in ('ray_mode', 'ray_end', 'ray_events', 'ray_casts'))
            pr.hash = _p(ro['ray_hash'], c_u64p)
        rep = nk_kinetic_report()
        if grid is not None:
            # (the library refuses a bad grid by name; the buffer is sized here, so the counts are read with care)
            glo, gh = _d(np.ravel(grid[0])), _d(np.ravel(grid[1]))
            try:
                nc = [int(k) for k in np.ravel(grid[2])]
            except (TypeError, ValueError):
                nc = []
            if glo.shape[0] != 3 or gh.shape[0] != 3 or len(nc) != 3:
                raise NkError('kinetic_flights: grid must be (lo [3], h [3], n_cells [3])')
            gg, mo = nk_kinetic_grid(), nk_kinetic_map_out()
            ok = min(nc) > 0 and max(nc) < (1 << 31) and nc[0] * nc[1] * nc[2] <= KIN_MAX_MAP_CELLS
            gg.n[:] = [k if -(1 << 31) <= k < (1 << 31) else -1 for k in nc]
            gg.lo[:], gg.h[:] = [float(x) for x in glo], [float(x) for x in gh]
            ncells = nc[0] * nc[1] * nc[2] if ok else 0
            cells = np.zeros(max(min(F * ncells * 4, KIN_MAX_MAP_WORDS), 1), dtype=np.int64)        # (a call never returns more words)
            mo.cells = cells.ctypes.data_as(C.POINTER(C.c_int64))
            rc = self.L.nk_kinetic_flights_map(self.h, C.byref(a), C.byref(gg), C.byref(o), C.byref(mo), C.byref(pr) if pr else None,
                                               C.byref(rep))
        elif groups is None:
            rc = self.L.nk_kinetic_flights(self.h, C.byref(a), C.byref(o), C.byref(pr) if pr else None, C.byref(rep))
        else:
            # (the library refuses a bad G or table by name; only the table's length is checked here, since it reads M entries)
            G, table = int(groups[0]), groups[1]
            gs, go = nk_kinetic_groups(), nk_kinetic_group_out()
            gs.n_groups = G
            if table is not None:
                table = np.ascontiguousarray(np.ravel(table), dtype=np.int32)
                if table.shape[0] != self.M:
                    raise NkError('kinetic_flights: the group table has %d entries, the material %d modes' % (table.shape[0], self.M))
                gs.group_of_mode = _p(table, c_ip)
            GC = G + 1 if 1 <= G <= KIN_MAX_GROUPS else 1
            grp = np.zeros(min(F * S * GC * 4, KIN_MAX_GROUP_WORDS), dtype=np.int64)     # (a call never returns more words)
            go.grp = grp.ctypes.data_as(C.POINTER(C.c_int64))
            rc = self.L.nk_kinetic_flights_groups(self.h, C.byref(a), C.byref(gs), C.byref(o), C.byref(go), C.byref(pr) if pr else None,
                                                  C.byref(rep))
        r = {k: (list(getattr(rep, k)) if k == 'source_facet' else getattr(rep, k)) for k, _ in nk_kinetic_report._fields_ if k != 'pad_'}
        if rc != 0 and not (rc == ERR_CAPACITY and r['overflow'] > 0):
            self._ck(rc, 'nk_kinetic_flights_map' if grid is not None else 'nk_kinetic_flights' if groups is None else 'nk_kinetic_flights_groups')
        nf = int(rep.n_sources)
        r['source_facet'] = r['source_facet'][:nf]
        r['message'] = self.L.nk_last_error(self.h).decode() if rc != 0 else ''
        rows, sub = rows[:nf].copy(), sub[:nf * S * 4].reshape(nf, S, 4).copy()
        grp = None if groups is None else grp[:nf * S * GC * 4].reshape(nf, S, GC, 4).copy()
        m = None if grid is None else cells[:nf * ncells * 4].reshape((nf,) + tuple(nc) + (4,)).copy()
        out = dict(n=n, source_facet=np.array(r['source_facet'], dtype=np.int32), **KN.derived(rows, sub, r, grp=grp, map=m),
                   cdf_scatter=cs, cdf_flux=cf, report=r)
        for k, v in ro.items():
            out[k] = v[:nf].copy()
        return out

    def get_step(self):
        """Timesteps this engine has completed (the library's absolute step counter: flux and contains_check cadence)."""
        n = C.c_int64(0)
        self._ck(self.L.nk_get_step(self.h, C.byref(n)), 'nk_get_step')
        return int(n.value)

    def download(self):
        n = C.c_int64(0)
        self._ck(self.L.nk_download_particles(self.h, 0, None, None, None, None, None, None, None, None, C.byref(n)),
                 'nk_download_particles')
        N = int(n.value)
        x, y, z, occ, nts = (np.zeros(N) for _ in range(5))
        mode, facet = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        pid = np.zeros(N, dtype=np.uint64)
        if N:
            self._ck(self.L.nk_download_particles(self.h, N, _p(x), _p(y), _p(z), _p(mode, c_ip), _p(occ), _p(nts),
                                                  _p(facet, c_ip), _p(pid, c_u64p), C.byref(n)), 'nk_download_particles')
        return dict(positions=np.stack((x, y, z), axis=1), mode=mode, occupation=occ, n_timesteps=nts, facet=facet, pid=pid)

    def subvol_temperature(self):
        t = np.zeros(self.S)
        self._ck(self.L.nk_get_subvol_temperature(self.h, _p(t)), 'nk_get_subvol_temperature')
        return t

    def set_subvol_temperature(self, T):
        t = _d(T)
        self._ck(self.L.nk_set_subvol_temperature(self.h, _p(t)), 'nk_set_subvol_temperature')

    def timing(self):
        t = nk_timing()
        self._ck(self.L.nk_get_timing(self.h, C.byref(t)), 'nk_get_timing')
        return dict(step_kernel_ms=t.step_kernel_ms, emit_kernel_ms=t.emit_kernel_ms, events_kernel_ms=t.events_kernel_ms,
                    total_ms=t.total_ms,
                    slots=int(t.slots), live=int(t.live), regrows=int(t.regrows), halts=int(t.halts),
                    tau_rebuilds=int(t.tau_rebuilds), batches=int(t.batches), emit_fused=int(t.emit_fused),
                    place_tries=int(t.place_tries), place_gbps=t.place_gbps, place_worst_gbps=t.place_worst_gbps,
                    box_store=int(t.box_store))

    # ---- set-up table builder (find_specular_correspondences 'velocity', Population.py:1241-1454)
    def specular_begin(self, group_vel, omega, delta_omega):
        v, om, dl = _d(np.asarray(group_vel).reshape(-1, 3)), _d(np.ravel(omega)), _d(np.ravel(delta_omega))
        self._ck(self.L.nk_specular_begin(self.h, om.shape[0], _p(v), _p(om), _p(dl)), 'nk_specular_begin')
        self._spec_M = om.shape[0]

    def specular_pairs(self, normal, crit=1e-3, download=True):
        """(in, out) flat mode indices of every specular pair for one normal, unordered.  download=False: the pairs stay on
        the device for nk_rough_pairs and nothing is returned."""
        nrm = _d(np.asarray(normal, dtype=float))
        cap = getattr(self, '_spec_cap', 4 * self._spec_M)
        while True:
            n = C.c_int64(0)
            if download:
                pi, po = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
                self._ck(self.L.nk_specular_pairs(self.h, _p(nrm), float(crit), cap, _p(pi, c_ip), _p(po, c_ip), C.byref(n)),
                         'nk_specular_pairs')
            else:
                self._ck(self.L.nk_specular_pairs(self.h, _p(nrm), float(crit), cap, None, None, C.byref(n)), 'nk_specular_pairs')
            if n.value <= cap:
                return (pi[:n.value].astype(np.int64), po[:n.value].astype(np.int64)) if download else None
            cap = self._spec_cap = int(n.value)

    def specular_end(self):
        self._ck(self.L.nk_specular_end(self.h), 'nk_specular_end')

    # ---- rough-facet tables built on the device (between specular_begin and specular_end; 'velocity' model)
    def rough_begin(self, facets, normal_in, eta, k_norm):
        f, n, e, k = _i(facets), _d(normal_in), _d(eta), _d(k_norm)
        self._rough_Fr = f.shape[0]
        self._ck(self.L.nk_rough_begin(self.h, f.shape[0], _p(f, c_ip), _p(n), _p(e), _p(k)), 'nk_rough_begin')

    def rough_pairs(self, rough_facet_indices):
        """The pairs of the last specular_pairs call (still on the device) for the rough facets that share its normal."""
        f = _i(rough_facet_indices)
        self._ck(self.L.nk_rough_pairs(self.h, f.shape[0], _p(f, c_ip)), 'nk_rough_pairs')

    def rough_finish(self, degeneracies=None, degen_j2=None):
        """degeneracies [nd, 3] (q, j1, j2) and degen_j2 [M]: the 'k' model's degenerate branches (nk_rough_finish_k)."""
        if degeneracies is None:
            self._ck(self.L.nk_rough_finish(self.h), 'nk_rough_finish')
            return
        dg = _i(np.asarray(degeneracies, dtype=np.int32).reshape(-1, 3))
        dj = None if degen_j2 is None else _i(degen_j2)
        self._ck(self.L.nk_rough_finish_k(self.h, dg.shape[0], _p(dg, c_ip), _p(dj, c_ip)), 'nk_rough_finish_k')

    def kspec_begin(self, wavevectors, k_to_q, q_to_k, tol):
        """'k' model pair search (after specular_begin): q = k . k_to_q, k = q . q_to_k (3 x 3), tol [3]."""
        kv, a, b, t = _d(wavevectors), _d(np.asarray(k_to_q, dtype=float).reshape(3, 3)), _d(np.asarray(q_to_k, dtype=float).reshape(3, 3)), _d(tol)
        self._ck(self.L.nk_kspec_begin(self.h, kv.shape[0], _p(kv), _p(a), _p(b), _p(t)), 'nk_kspec_begin')

    def kspec_pairs(self, normal, download=True):
        """(in, out) flat mode indices of the 'k' model's specular pairs for one normal (one partner per in-mode)."""
        nrm = _d(np.asarray(normal, dtype=float))
        cap = self._spec_M
        n = C.c_int64(0)
        if download:
            pi, po = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int32)
            self._ck(self.L.nk_kspec_pairs(self.h, _p(nrm), cap, _p(pi, c_ip), _p(po, c_ip), C.byref(n)), 'nk_kspec_pairs')
            return pi[:n.value].astype(np.int64), po[:n.value].astype(np.int64)
        self._ck(self.L.nk_kspec_pairs(self.h, _p(nrm), cap, None, None, C.byref(n)), 'nk_kspec_pairs')
        return None

    def rough_download(self):
        """(specularity, true_spec, spec_map, roulette), each [Fr, M]."""
        Fr, M = self._rough_Fr, self.M
        sp, ts = np.zeros((Fr, M)), np.zeros((Fr, M), dtype=np.uint8)
        sm, ro = np.zeros((Fr, M), dtype=np.int32), np.zeros((Fr, M))
        self._ck(self.L.nk_rough_download(self.h, _p(sp), _p(ts, c_up), _p(sm, c_ip), _p(ro)), 'nk_rough_download')
        return sp, ts, sm, ro

    def build_enter_prob(self, normal_in, thickness, dt):
        n, t = _d(normal_in), _d(thickness)
        out = np.zeros((t.shape[0], self.M))
        self._ck(self.L.nk_build_enter_prob(self.h, t.shape[0], _p(n), _p(t), float(dt), _p(out)), 'nk_build_enter_prob')
        return out

    def calibrate_stream(self, launches=3):
        """Known-traffic sweeps for counter calibration; returns (bytes_read, bytes_written) per launch."""
        r, w = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.nk_calibrate_stream(self.h, int(launches), C.byref(r), C.byref(w)), 'nk_calibrate_stream')
        return int(r.value), int(w.value)

    def comm_init(self, unique_id, rank, nranks):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._ck(self.L.nk_comm_init(self.h, buf, int(rank), int(nranks)), 'nk_comm_init')

    def comm_allreduce(self, *arrays):
        """Sum of small host arrays over the ranks of the communicator; returns them unchanged when there is none."""
        flat = _d(np.concatenate([np.ravel(np.asarray(a, dtype=float)) for a in arrays]))
        self._ck(self.L.nk_comm_allreduce(self.h, _p(flat), flat.shape[0]), 'nk_comm_allreduce')
        out, off = [], 0
        for a in arrays:
            a = np.asarray(a)
            out.append(flat[off:off + a.size].reshape(a.shape).copy())
            off += a.size
        return out

    def comm_info(self):
        """What RCCL itself reports about this context's communicator (rank count, own rank, the self-test all-reduce of
        nk_comm_init), the HIP device and its PCI bus id."""
        r = nk_comm_report()
        self._ck(self.L.nk_comm_info(self.h, C.byref(r)), 'nk_comm_info')
        return dict(rank=int(r.rank), nranks=int(r.nranks), comm_rank=int(r.comm_rank), comm_nranks=int(r.comm_nranks),
                    device=int(r.device), selftest_ok=bool(r.selftest_ok), selftest_sum=float(r.selftest_sum),
                    pci_bus_id=r.pci_bus_id.decode(errors='replace'))

    # -------------------------------------------------------------------- taps
    def find_boundary(self, x, v, from_facet=None):
        """(xc, tc, fc) of the rays (x, v).  from_facet [n]: the facet every ray starts on (-1: none), for which the walk of the
        face tree forms its facet skip as the sweep does; then also `skipped` [n] (1 where the skip engaged)."""
        x, v = _d(x), _d(v)
        n = x.shape[0]
        xc, tc, fc = np.zeros((n, 3)), np.zeros(n), np.zeros(n, dtype=np.int32)
        if from_facet is None:
            self._ck(self.L.nk_find_boundary(self.h, n, _p(x), _p(v), _p(xc), _p(tc), _p(fc, c_ip)), 'nk_find_boundary')
            return xc, tc, fc
        ff, sk = _i(np.broadcast_to(np.asarray(from_facet, dtype=np.int32), (n,))), np.zeros(n, dtype=np.int32)
        self._ck(self.L.nk_find_boundary_from(self.h, n, _p(x), _p(v), _p(ff, c_ip), _p(xc), _p(tc), _p(fc, c_ip), _p(sk, c_ip)),
                 'nk_find_boundary_from')
        return xc, tc, fc, sk

    def tree_info(self, boxes=False):
        """The face tree of the mesh (nk_tree_info): NG, tree_top, level_nodes [tree_top + 1], top_family, tree_leaves, references,
        pad_slots, tree_bound, tree_base.  boxes=True adds family_boxes [levels][nodes incl. padding, 6] (lo(3), hi(3) as float32;
        padding boxes have lo > hi) and leaf_boxes [tree_leaves, 4, 6].  Reads only."""
        r = nk_tree_report()
        self._ck(self.L.nk_tree_info(self.h, C.byref(r), None, None), 'nk_tree_info')
        nl = int(r.tree_top) + 1 if r.NG else 0
        out = dict(NG=int(r.NG), tree_top=int(r.tree_top), level_nodes=[int(r.level_nodes[l]) for l in range(nl)],
                   tree_base=[int(r.tree_base[l]) for l in range(nl)], top_family=int(r.top_family), tree_leaves=int(r.tree_leaves),
                   references=int(r.references), pad_slots=int(r.pad_slots), n_families=int(r.n_families), tree_bound=float(r.tree_bound))
        if boxes and r.NG:
            fb = np.zeros(int(r.n_families) * 24, dtype=np.float32)
            lb = np.zeros(int(r.tree_leaves) * 24, dtype=np.float32)
            c_fp = C.POINTER(C.c_float)
            self._ck(self.L.nk_tree_info(self.h, C.byref(r), _p(fb, c_fp), _p(lb, c_fp)), 'nk_tree_info')
            fb = fb.reshape(-1, 6)
            ends = out['tree_base'][1:] + [fb.shape[0]]
            out['family_boxes'] = [fb[a:b].copy() for a, b in zip(out['tree_base'], ends)]
            out['leaf_boxes'] = lb.reshape(-1, 4, 6)
        return out

    def classify(self, x):
        x = _d(x)
        out = np.zeros(x.shape[0], dtype=np.int32)
        self._ck(self.L.nk_classify(self.h, x.shape[0], _p(x), _p(out, c_ip)), 'nk_classify')
        return out

    def box_hit(self, which, x, v):
        """The box store's wall functions on rays (x, v): which = 0 nk_box_out -> (1.0 / 0.0, -1), 1 nk_box_first_hit -> (n_timesteps,
        facet), 2 nk_box_next_hit -> (t, facet).  Only on a mesh that nk_set_mesh found to be a box."""
        x, v = _d(x), _d(v)
        n = x.shape[0]
        t, f = np.zeros(n), np.zeros(n, dtype=np.int32)
        self._ck(self.L.nk_box_hit(self.h, int(which), n, _p(x), _p(v), _p(t), _p(f, c_ip)), 'nk_box_hit')
        return t, f

    def eval(self, what, a, mode=None):
        code = {'occupation': 0, 'lifetime': 1, 'T_of_E': 2, 'E_of_T': 3, 'interp_T': 4, 'exp': 5, 'exp_small': 6, 'rcp': 7,
                'relax': 8}[what]                      # 'relax': a[n, 4] = x, y, z, occupation
        a = _d(a)
        n = a.shape[0]
        m = None if mode is None else _i(mode)
        out = np.zeros(n)
        self._ck(self.L.nk_eval(self.h, code, n, _p(a), _p(m, c_ip), _p(out)), 'nk_eval')
        return out

    def mode_segments(self):
        """(segment of the particle store that holds every mode's particles [M], number of segments).  download() returns the
        segments one after another, and a wave of the sweep takes 64 consecutive particles of one segment."""
        seg, n = np.zeros(self.M, dtype=np.int32), C.c_int32(0)
        self._ck(self.L.nk_mode_segments(self.h, _p(seg, c_ip), C.byref(n)), 'nk_mode_segments')
        return seg, int(n.value)

    def reflect(self, facet, mode_in, col_pos, n_in, omega_in, r_spec, r_deg, r_diff):
        f, m, c = _i(facet), _i(mode_in), _d(col_pos)
        n = f.shape[0]
        a = [_d(v) for v in (n_in, omega_in, r_spec)]
        rd = None if r_deg is None else _d(r_deg)
        rf = _d(r_diff)
        mo, no, oo = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
        self._ck(self.L.nk_reflect(self.h, n, _p(f, c_ip), _p(m, c_ip), _p(c), _p(a[0]), _p(a[1]), _p(a[2]), _p(rd),
                                   _p(rf), _p(mo, c_ip), _p(no), _p(oo)), 'nk_reflect')
        return mo, no, oo

    def uniform2(self, seed, pid, step, tag):
        u0, u1 = C.c_double(), C.c_double()
        rc = self.L.nk_uniform2(C.c_uint64(seed), C.c_uint64(pid), C.c_uint32(step), C.c_uint32(tag), C.byref(u0), C.byref(u1))
        if rc != 0:
            raise NkError('nk_uniform2 failed')
        return u0.value, u1.value


class EngineGroup(object):
    """One nk_group: engines that hold the same problem under different seeds, stepped by shared launches (one sweep and one
    tail launch per step for all of them).  Raises NkError (its `code` is ERR_ARG; the message names the member and the reason) when the
    engines cannot be grouped; the engines themselves stay usable, before, between and after group calls."""

    def __init__(self, engines):
        self.engines = list(engines)             # kept alive: the group must be destroyed before any member
        self.L = load_library()
        self.h = None
        n = len(self.engines)
        arr = (C.c_void_p * max(n, 1))(*[e.h for e in self.engines])
        h = C.c_void_p()
        rc = self.L.nk_group_create(C.byref(h), arr, n)
        if rc != 0:
            err = NkError('nk_group_create failed (%d): %s' % (rc, self.L.nk_group_last_error(None).decode()))
            err.code = rc
            raise err
        self.h = h

    def close(self):
        if getattr(self, 'h', None):
            self.L.nk_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, nsteps=1):
        """nsteps timesteps of every member; a list of the dicts Engine.step returns, one per member."""
        blocks = [e._tally_block(nsteps) for e in self.engines]
        ts = (nk_tally * len(blocks))(*[t for _, t in blocks])
        rc = self.L.nk_group_step(self.h, int(nsteps), ts)
        if rc != 0:
            err = NkError('nk_group_step failed (%d): %s' % (rc, self.L.nk_group_last_error(self.h).decode()))
            err.code = rc
            raise err
        return [out for out, _ in blocks]

    def info(self):
        r = nk_group_report()
        rc = self.L.nk_group_info(self.h, C.byref(r))
        if rc != 0:
            raise NkError('nk_group_info failed (%d)' % rc)
        return {k: getattr(r, k) for k, _ in nk_group_report._fields_ if k != 'pad_'}

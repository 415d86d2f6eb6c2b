"""ctypes binding of libgroan_hip.so (the C ABI declared in include/groan_hip.h).

The shared library is the product; this module only declares argument types.  It fails loudly if
the library has not been built (`python -c "import __graft_entry__ as g; g.build()"` or
`make -C groan_rs_amd/csrc`): there is no Python/CPU fallback for any operation.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GR_LIB_PATH") or os.path.join(_HERE, "libgroan_hip.so")   # GR_LIB_PATH: A/B builds only

c_u64p = C.POINTER(C.c_uint64)
c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int)

# status codes (include/groan_hip.h)
(OK, E_NO_BOX, E_NOT_ORTHOGONAL, E_ZERO_BOX, E_EMPTY_GROUP, E_INCONSISTENT_GROUP, E_NO_POSITION, E_NO_MASS,
 E_GROUP_NOT_FOUND, E_OUT_OF_RANGE, E_INVALID_ARG, E_GROUP_EXISTS, E_HIP, E_NO_DEVICE, E_UNSUPPORTED_BOX, E_IO, E_FORMAT,
 E_INVALID_NAME, E_EMPTY_CHAIN, E_NONEXISTENT_CHAIN, E_DUPLICATE_PAIR, E_UNUSED_CHAIN, E_INVALID_BOND, E_INVALID_SPAN,
 E_INVALID_TILE) = range(25)

CENTER_NAIVE, CENTER_ESTIMATE, CENTER_PBC = 0, 1, 2
GM_COUNT, GM_X, GM_Y, GM_Z = 0, 1, 2, 3
GM_WRAP, GM_FORCE_GLOBAL = 1, 2
GM_STAT_LDS_LAUNCHES, GM_STAT_GLOBAL_LAUNCHES, GM_STAT_LDS_BUDGET = 1, 2, 3
GM_STAT_LAST_RANGE_GROUPS, GM_STAT_LAST_FRAME_GROUPS, GM_STAT_LAST_CHECK_GROUPS = 4, 5, 6
SEG_STAT_TEAM4, SEG_STAT_TEAM16, SEG_STAT_WAVE, SEG_STAT_WORKGROUP, SEG_STAT_LAST_LAUNCHES, SEG_STAT_LAST_LAUNCH_SETS = 1, 2, 3, 4, 5, 6
SEG_STAT_LAST_PIECES = 7
RG_STAT_LAST_LAUNCHES, RG_STAT_LAST_PIECES, RG_STAT_LAST_TOTAL, RG_STAT_CHUNK = 1, 2, 3, 4
CT_STAT_LAST_LAUNCHES, CT_STAT_LAST_PIECES, CT_STAT_LAST_TOTAL, CT_STAT_TILE = 1, 2, 3, 4
CT_STAT_LAST_RUNS, CT_STAT_LAST_CELLS, CT_STAT_LAST_RUN_CELLS_MIN, CT_STAT_LAST_RUN_CELLS_MAX, CT_STAT_LAST_WALK_GROUPS = 5, 6, 7, 8, 9
FL_STAT_LAUNCHES, FL_STAT_LAST_RANGE_GROUPS, FL_STAT_LAST_CHECK_GROUPS, FL_STAT_FORM, FL_STAT_AHEAD = 1, 2, 3, 4, 5
CV_STAT_LAUNCHES, CV_STAT_LAST_PRODUCT_GROUPS, CV_STAT_LAST_CHECK_GROUPS, CV_STAT_BLOCK_EDGE, CV_STAT_TRIP_FRAMES, CV_STAT_BLOCKS = 1, 2, 3, 4, 5, 6
CV_MASS_WEIGHTED = 1
CV_MAX_ATOMS = 4096
MSD_X, MSD_Y, MSD_Z, MSD_NOJUMP = 1, 2, 4, 8
MSD_MAX_PANEL_BYTES = 17179869184
MSD_STAT_LAUNCHES, MSD_STAT_LAST_WALK_GROUPS, MSD_STAT_LAST_GRAM_GROUPS, MSD_STAT_BLOCK_EDGE, MSD_STAT_TRIP_VALUES = 1, 2, 3, 4, 5
MSD_STAT_LAST_BLOCKS, MSD_STAT_LAGS, MSD_STAT_N_PAD, MSD_STAT_COUNTED = 6, 7, 8, 9
IC_DISTANCE, IC_ANGLE, IC_DIHEDRAL, IC_AXIS = 1, 2, 3, 4
IC_PBC = 1
IC_MAX_WS_BYTES = 64 << 20
IC_STAT_LAUNCHES, IC_STAT_LAST_RANGE_GROUPS, IC_STAT_LAST_FRAME_GROUPS, IC_STAT_LAST_CHECK_GROUPS, IC_STAT_ARITY, IC_STAT_UNIQUE_ATOMS, IC_STAT_AHEAD = 1, 2, 3, 4, 5, 6, 7
VCORR_PBC, VCORR_UNIT, VCORR_P1, VCORR_P2 = 1, 2, 4, 8
VCORR_MAX_EACH_BYTES = 1 << 30
VCORR_STAT_LAUNCHES, VCORR_STAT_N_PAD, VCORR_STAT_LAGS, VCORR_STAT_LAST_WALK_GROUPS, VCORR_STAT_LAST_GRAM_GROUPS = 1, 2, 3, 4, 5
VCORR_STAT_LAST_EACH_GROUPS, VCORR_STAT_LAST_BLOCKS, VCORR_STAT_COUNTED = 6, 7, 8
CT_MAX_BINS = 4096
MAX_SHAPES = 8

# every symbol include/groan_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "gr_version": (C.c_char_p, []),
    "gr_status_string": (C.c_char_p, [C.c_int]),
    "gr_device_count": (C.c_int, [c_i32p]),
    "gr_ctx_create": (C.c_void_p, [C.c_int, C.c_uint64, C.c_uint32, c_i32p]),
    "gr_ctx_destroy": (None, [C.c_void_p]),
    "gr_last_error": (C.c_char_p, [C.c_void_p]),
    "gr_last_error_index": (C.c_uint64, [C.c_void_p]),
    "gr_last_error_counts": (None, [C.c_void_p, c_u64p]),
    "gr_ctx_set_strict_orthogonal": (C.c_int, [C.c_void_p, C.c_int]),
    "gr_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_n_slots": (C.c_uint32, [C.c_void_p]),
    "gr_sync": (C.c_int, [C.c_void_p]),
    "gr_set_masses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "gr_container_from_indices": (C.c_size_t, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p]),
    "gr_container_from_ranges": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p]),
    "gr_container_union": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gr_container_intersection": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gr_container_n_atoms": (C.c_uint64, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "gr_container_expand": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gr_container_isin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]),
    "gr_container_validate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, c_u64p]),
    "gr_group_create_from_ranges": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "gr_group_create_from_indices": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "gr_group_remove": (C.c_int, [C.c_void_p, C.c_char_p]),
    "gr_group_exists": (C.c_int, [C.c_void_p, C.c_char_p]),
    "gr_group_count": (C.c_uint64, [C.c_void_p]),
    "gr_group_name": (C.c_int, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]),
    "gr_group_n_atoms": (C.c_int, [C.c_void_p, C.c_char_p, c_u64p]),
    "gr_group_n_blocks": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t)]),
    "gr_group_blocks": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]),
    "gr_frame_upload": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gr_frame_upload_wait": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_frame_download": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gr_frame_set_box": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gr_frame_get_box": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "gr_frame_copy": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "gr_host_alloc": (C.c_void_p, [C.c_size_t]),
    "gr_host_free": (None, [C.c_void_p]),
    "gr_group_center": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_void_p]),
    "gr_sel_center": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]),
    "gr_sel_translate": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gr_sel_wrap": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]),
    "gr_sel_all_distances": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]),
    "gr_sel_filter_geometry": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t), c_u64p]),
    "gr_group_distance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, c_f32p]),
    "gr_atoms_distance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, c_f32p]),
    "gr_group_all_distances": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "gr_group_all_distances_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), c_u64p, c_u64p]),
    "gr_group_all_distances_batch_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), c_u64p, c_u64p, C.c_void_p]),
    "gr_group_all_distances_reduce": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_size_t]),
    "gr_group_all_distances_reduce_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gr_device_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "gr_trr_open": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "gr_trr_close": (None, [C.c_void_p]),
    "gr_trr_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_trr_n_frames": (C.c_uint64, [C.c_void_p]),
    "gr_trr_frame_info": (C.c_int, [C.c_void_p, C.c_uint64, c_u64p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gr_trr_read_frame": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_u64p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "gr_trr_writer_open": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "gr_trr_writer_close": (C.c_int, [C.c_void_p]),
    "gr_trr_write_frame": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float]),
    "gr_trr_read_frames_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gr_group_translate": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p]),
    "gr_group_wrap": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "gr_atoms_center": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int]),
    "gr_calc_rmsd": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, c_f32p, C.c_void_p]),
    "gr_calc_rmsd_and_fit": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, c_f32p]),
    "gr_rmsd_plan_create": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_char_p, c_i32p]),
    "gr_rmsd_plan_destroy": (None, [C.c_void_p]),
    "gr_rmsd_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_rmsd_fit_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gr_rmsd_batch_begin": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]),
    "gr_rmsd_batch_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_rmsd_plan_last_fallbacks": (C.c_uint32, [C.c_void_p]),
    "gr_rmsd_plan_force_exact": (C.c_int, [C.c_void_p, C.c_int]),
    "gr_ctx_set_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_int64]),
    "gr_ctx_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_ctx_set_center_onepass_min": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_center_fallbacks": (C.c_uint64, [C.c_void_p]),
    "gr_gro_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "gr_structure_free": (None, [C.c_void_p]),
    "gr_structure_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_structure_title": (C.c_char_p, [C.c_void_p]),
    "gr_structure_box": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_structure_positions": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_structure_velocities": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_structure_atom": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_char_p, C.c_char_p]),
    "gr_ndx_read": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
    "gr_ndx_free": (None, [C.c_void_p]),
    "gr_ndx_n_groups": (C.c_size_t, [C.c_void_p]),
    "gr_ndx_group_name": (C.c_char_p, [C.c_void_p, C.c_size_t]),
    "gr_ndx_group_size": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "gr_ndx_group_indices": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "gr_ndx_install": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "gr_group_pairs_within": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "gr_hbond_plan_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_float, C.c_float, c_i32p]),
    "gr_hbond_plan_destroy": (None, [C.c_void_p]),
    "gr_hbond_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 c_u64p, C.c_void_p]),
    "gr_add_bond": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "gr_add_bonds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "gr_clear_bonds": (C.c_int, [C.c_void_p]),
    "gr_has_bonds": (C.c_int, [C.c_void_p]),
    "gr_mol_references": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, c_u64p]),
    "gr_molecule_atoms": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, c_u64p]),
    "gr_make_molecules_whole": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_make_molecules_whole_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_make_group_whole": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "gr_make_group_whole_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p]),
    "gr_gridmap_len": (C.c_int, [C.c_void_p, C.c_float, c_u64p]),
    "gr_gridmap_coord2index": (C.c_int64, [C.c_float, C.c_float, C.c_float]),
    "gr_gridmap_index2coord": (C.c_float, [C.c_float, C.c_float, C.c_uint64]),
    "gr_gridmap_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_i32p]),
    "gr_gridmap_from_box": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_void_p, c_i32p]),
    "gr_gridmap_destroy": (None, [C.c_void_p]),
    "gr_gridmap_dims": (C.c_int, [C.c_void_p, c_u64p, c_u64p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_gridmap_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_gridmap_set_launch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "gr_gridmap_clear": (C.c_int, [C.c_void_p]),
    "gr_gridmap_accumulate_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gr_gridmap_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_segments_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, c_i32p]),
    "gr_segments_from_labels": (C.c_void_p, [C.c_void_p, C.c_char_p, C.c_void_p, c_i32p]),
    "gr_segments_from_molecules": (C.c_void_p, [C.c_void_p, c_i32p]),
    "gr_segments_destroy": (None, [C.c_void_p]),
    "gr_segments_count": (C.c_uint64, [C.c_void_p]),
    "gr_segments_sizes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_segments_atoms": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, c_u64p]),
    "gr_segments_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_segments_center_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gr_segments_center_batch_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p), c_u64p, C.c_void_p]),
    "gr_segments_gyration_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_segments_gyration_batch_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_u64p,
                                                    C.c_void_p]),
    "gr_segments_set_piece_frames": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_region_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, c_i32p]),
    "gr_region_destroy": (None, [C.c_void_p]),
    "gr_region_select_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_region_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, c_u64p]),
    "gr_region_read_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_u64p, c_u64p]),
    "gr_region_group": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "gr_region_set_piece_frames": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_region_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_contacts_create": (C.c_void_p, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_float, c_i32p]),
    "gr_contacts_destroy": (None, [C.c_void_p]),
    "gr_contacts_pairs_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, c_u64p, C.c_void_p]),
    "gr_contacts_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, c_u64p]),
    "gr_contacts_read_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_u64p, c_u64p]),
    "gr_contacts_count_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_contacts_hist_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gr_contacts_sizes": (C.c_int, [C.c_void_p, c_u64p, c_u64p]),
    "gr_contacts_set_piece_frames": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_contacts_set_walk_groups": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_contacts_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_rmsd_panel_create": (C.c_void_p, [C.c_void_p, C.c_char_p, C.c_uint32, c_i32p]),
    "gr_rmsd_panel_destroy": (None, [C.c_void_p]),
    "gr_rmsd_panel_append_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_rmsd_panel_clear": (C.c_int, [C.c_void_p]),
    "gr_rmsd_panel_frames": (C.c_uint32, [C.c_void_p]),
    "gr_rmsd_panel_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_rmsd_panel_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_rmsd_panel_set_block_entries": (C.c_int, [C.c_void_p, C.c_uint64]),
    "gr_rmsd_matrix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_rmsd_matrix_device": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "gr_fluct_create": (C.c_void_p, [C.c_void_p, C.c_char_p, c_i32p]),
    "gr_fluct_destroy": (None, [C.c_void_p]),
    "gr_fluct_accumulate_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_fluct_clear": (C.c_int, [C.c_void_p]),
    "gr_fluct_frames": (C.c_uint64, [C.c_void_p]),
    "gr_fluct_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_fluct_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_fluct_read_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_u64p]),
    "gr_fluct_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_fluct_store_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "gr_fluct_set_launch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "gr_fluct_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_covar_create": (C.c_void_p, [C.c_void_p, C.c_char_p, c_i32p]),
    "gr_covar_destroy": (None, [C.c_void_p]),
    "gr_covar_accumulate_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_covar_clear": (C.c_int, [C.c_void_p]),
    "gr_covar_frames": (C.c_uint64, [C.c_void_p]),
    "gr_covar_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_covar_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "gr_covar_read_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_u64p]),
    "gr_covar_read_dccm": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_covar_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_covar_set_launch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "gr_covar_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_msd_create": (C.c_void_p, [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, c_i32p]),
    "gr_msd_destroy": (None, [C.c_void_p]),
    "gr_msd_append_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_msd_clear": (C.c_int, [C.c_void_p]),
    "gr_msd_frames": (C.c_uint64, [C.c_void_p]),
    "gr_msd_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_msd_capacity": (C.c_uint64, [C.c_void_p]),
    "gr_msd_compute": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_msd_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_msd_read_from_origin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_msd_read_displacements": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_msd_set_launch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "gr_msd_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_internals_create": (C.c_void_p, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, c_i32p]),
    "gr_internals_destroy": (None, [C.c_void_p]),
    "gr_internals_count": (C.c_uint64, [C.c_void_p]),
    "gr_internals_frames": (C.c_uint64, [C.c_void_p]),
    "gr_internals_values_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gr_internals_values_batch_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
    "gr_internals_accumulate_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_internals_clear": (C.c_int, [C.c_void_p]),
    "gr_internals_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_internals_read_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_u64p]),
    "gr_internals_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gr_internals_set_launch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "gr_internals_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_vcorr_create": (C.c_void_p, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, c_i32p]),
    "gr_vcorr_destroy": (None, [C.c_void_p]),
    "gr_vcorr_count": (C.c_uint64, [C.c_void_p]),
    "gr_vcorr_frames": (C.c_uint64, [C.c_void_p]),
    "gr_vcorr_capacity": (C.c_uint64, [C.c_void_p]),
    "gr_vcorr_append_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_vcorr_clear": (C.c_int, [C.c_void_p]),
    "gr_vcorr_compute": (C.c_int, [C.c_void_p, C.c_uint32]),
    "gr_vcorr_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gr_vcorr_compute_each": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gr_vcorr_read_vectors": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "gr_vcorr_set_launch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "gr_vcorr_stat": (C.c_int, [C.c_void_p, C.c_int, c_u64p]),
    "gr_group_center_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gr_group_translate_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p]),
    "gr_group_wrap_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p]),
    "gr_atoms_center_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_void_p]),
    "gr_xtc_writer_open": (C.c_void_p, [C.c_char_p, C.POINTER(C.c_int)]),
    "gr_xtc_writer_close": (C.c_int, [C.c_void_p]),
    "gr_xtc_write_frame": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float]),
    "gr_xtc_write_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int]),
    "gr_xtc_read_frames_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "gr_xtc_read_frame_prefix": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, c_u64p, c_f32p, c_f32p, c_u64p]),
    "gr_xtc_read_frames_device_group": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]),
    "gr_shape_sphere": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float]),
    "gr_shape_rectangular": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "gr_shape_cylinder": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int]),
    "gr_shape_triangular_prism": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]),
    "gr_shape_inside": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "gr_group_create_from_geometries": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]),
    "gr_xtc_open": (C.c_void_p, [C.c_char_p, c_i32p]),
    "gr_xtc_close": (None, [C.c_void_p]),
    "gr_xtc_n_atoms": (C.c_uint64, [C.c_void_p]),
    "gr_xtc_n_frames": (C.c_uint64, [C.c_void_p]),
    "gr_xtc_frame_info": (C.c_int, [C.c_void_p, C.c_uint64, c_u64p, c_f32p, C.c_void_p, c_f32p]),
    "gr_xtc_read_frame": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, c_u64p, c_f32p, c_f32p]),
    "gr_pool_create": (C.c_void_p, [C.POINTER(C.c_int), C.c_int, C.c_uint64, C.c_uint32, c_i32p]),
    "gr_pool_destroy": (None, [C.c_void_p]),
    "gr_pool_size": (C.c_int, [C.c_void_p]),
    "gr_pool_ctx": (C.c_void_p, [C.c_void_p, C.c_int]),
    "gr_pool_last_error": (C.c_char_p, [C.c_void_p]),
    "gr_pool_map": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, c_u64p, c_u64p]),
    "gr_pool_map_range": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, c_u64p, c_u64p]),
    "gr_comm_unique_id": (C.c_int, [C.c_void_p]),
    "gr_comm_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_void_p, c_i32p]),
    "gr_comm_destroy": (None, [C.c_void_p]),
    "gr_comm_last_error": (C.c_char_p, [C.c_void_p]),
    "gr_comm_library": (C.c_char_p, []),
    "gr_comm_set_library": (C.c_int, [C.c_char_p]),
    "gr_comm_gather_per_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_void_p]),
    "gr_comm_any_error": (C.c_int, [C.c_void_p, C.c_int, c_i32p]),
    "gr_shard_deinterleave": (None, [C.c_void_p, C.c_int, C.c_uint64, C.c_size_t, C.c_void_p]),
    "gr_timer_start": (C.c_int, [C.c_void_p]),
    "gr_timer_stop": (C.c_int, [C.c_void_p, c_f32p]),
    "gr_synth_reference": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_float, C.c_uint64]),
    "gr_synth_frames": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_float, C.c_uint64]),
    "gr_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "gr_profile_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), c_u64p, c_u64p]),
    "gr_synth_uniform": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
}

_LIB = None


class LibraryMissing(RuntimeError):
    pass


def load():
    """dlopen libgroan_hip.so and declare every entry point.  Raises if the HIP library is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            "groan_rs_amd/libgroan_hip.so has not been built (run __graft_entry__.build() or "
            "`make -C groan_rs_amd/csrc`); the HIP extension is required, there is no CPU fallback")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("GR_LIB_PATH") and not hasattr(lib, name):
            continue              # A/B builds of older sources (tools/ab_bench.sh) may lack newer entry points
        fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib

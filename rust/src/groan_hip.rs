//! Bindings of libgroan_hip.so (include/groan_hip.h) for groan_rs, in the style of the crate's existing
//! xdrfile FFI (`src/io/xdrfile.rs:27-120`): raw `extern "C"` declarations, an opaque `#[repr(C)]` handle,
//! an RAII owner with `Drop`, and safe methods returning the crate's own error enums.
//!
//! NOT COMPILED in the build container (no cargo/rustc there).  Feature-gate as `hip` in Cargo.toml and
//! link with `println!("cargo:rustc-link-lib=dylib=groan_hip")` from build.rs.
#![allow(non_camel_case_types)]

use std::ffi::{c_char, c_float, c_int, c_void, CString};
use std::marker::PhantomData;

use crate::errors::{AtomError, CellGridError, GroupError, HBondError, MassError, PositionError, RMSDError, SimBoxError};
use crate::structures::{container::AtomContainer, dimension::Dimension, group::Group, simbox::SimBox, vector3d::Vector3D};
use crate::system::System;
use crate::structures::traj_convert::{FrameAnalyze, FrameConvertAnalyze};

#[repr(C)] pub struct gr_ctx { _private: [u8; 0] }
#[repr(C)] pub struct gr_rmsd_plan { _private: [u8; 0] }

pub const GR_OK: c_int = 0;
pub const GR_E_NO_BOX: c_int = 1;
pub const GR_E_NOT_ORTHOGONAL: c_int = 2;
pub const GR_E_ZERO_BOX: c_int = 3;
pub const GR_E_EMPTY_GROUP: c_int = 4;
pub const GR_E_INCONSISTENT_GROUP: c_int = 5;
pub const GR_E_NO_POSITION: c_int = 6;
pub const GR_E_NO_MASS: c_int = 7;
pub const GR_E_GROUP_NOT_FOUND: c_int = 8;
pub const GR_E_OUT_OF_RANGE: c_int = 9;
pub const GR_E_INVALID_ARG: c_int = 10;
pub const GR_E_EMPTY_CHAIN: c_int = 18;
pub const GR_E_NONEXISTENT_CHAIN: c_int = 19;
pub const GR_E_DUPLICATE_PAIR: c_int = 20;
pub const GR_E_UNUSED_CHAIN: c_int = 21;
pub const GR_E_INVALID_BOND: c_int = 22;
pub const GR_E_INVALID_SPAN: c_int = 23;
pub const GR_E_INVALID_TILE: c_int = 24;
pub const GR_GM_COUNT: c_int = 0;
pub const GR_GM_X: c_int = 1;
pub const GR_GM_Y: c_int = 2;
pub const GR_GM_Z: c_int = 3;
pub const GR_GM_WRAP: c_int = 1;
pub const GR_GM_FORCE_GLOBAL: c_int = 2;
pub const GR_GM_STAT_LDS_LAUNCHES: c_int = 1;
pub const GR_GM_STAT_GLOBAL_LAUNCHES: c_int = 2;
pub const GR_GM_STAT_LDS_BUDGET: c_int = 3;
pub const GR_GM_STAT_LAST_RANGE_GROUPS: c_int = 4;
pub const GR_GM_STAT_LAST_FRAME_GROUPS: c_int = 5;
pub const GR_GM_STAT_LAST_CHECK_GROUPS: c_int = 6;
pub const GR_SEG_STAT_TEAM4: c_int = 1;
pub const GR_SEG_STAT_TEAM16: c_int = 2;
pub const GR_SEG_STAT_WAVE: c_int = 3;
pub const GR_SEG_STAT_WORKGROUP: c_int = 4;
pub const GR_SEG_STAT_LAST_LAUNCHES: c_int = 5;
pub const GR_SEG_STAT_LAST_LAUNCH_SETS: c_int = 6;
pub const GR_SEG_STAT_LAST_PIECES: c_int = 7;
pub const GR_RG_STAT_LAST_LAUNCHES: c_int = 1;
pub const GR_RG_STAT_LAST_PIECES: c_int = 2;
pub const GR_RG_STAT_LAST_TOTAL: c_int = 3;
pub const GR_RG_STAT_CHUNK: c_int = 4;
pub const GR_CT_STAT_LAST_LAUNCHES: c_int = 1;
pub const GR_CT_STAT_LAST_PIECES: c_int = 2;
pub const GR_CT_STAT_LAST_TOTAL: c_int = 3;
pub const GR_CT_STAT_TILE: c_int = 4;
pub const GR_CT_STAT_LAST_RUNS: c_int = 5;
pub const GR_CT_STAT_LAST_CELLS: c_int = 6;
pub const GR_CT_STAT_LAST_RUN_CELLS_MIN: c_int = 7;
pub const GR_CT_STAT_LAST_RUN_CELLS_MAX: c_int = 8;
pub const GR_CT_STAT_LAST_WALK_GROUPS: c_int = 9;
pub const GR_MSD_X: u32 = 1;
pub const GR_MSD_Y: u32 = 2;
pub const GR_MSD_Z: u32 = 4;
pub const GR_MSD_NOJUMP: u32 = 8;
pub const GR_MSD_STAT_LAUNCHES: c_int = 1;
pub const GR_MSD_STAT_LAST_WALK_GROUPS: c_int = 2;
pub const GR_MSD_STAT_LAST_GRAM_GROUPS: c_int = 3;
pub const GR_MSD_STAT_BLOCK_EDGE: c_int = 4;
pub const GR_MSD_STAT_TRIP_VALUES: c_int = 5;
pub const GR_MSD_STAT_LAST_BLOCKS: c_int = 6;
pub const GR_MSD_STAT_LAGS: c_int = 7;
pub const GR_MSD_STAT_N_PAD: c_int = 8;
pub const GR_MSD_STAT_COUNTED: c_int = 9;
pub const GR_VCORR_PBC: u32 = 1;
pub const GR_VCORR_UNIT: u32 = 2;
pub const GR_VCORR_P1: u32 = 4;
pub const GR_VCORR_P2: u32 = 8;
pub const GR_VCORR_MAX_EACH_BYTES: u64 = 1073741824;
pub const GR_VCORR_STAT_LAUNCHES: c_int = 1;
pub const GR_VCORR_STAT_N_PAD: c_int = 2;
pub const GR_VCORR_STAT_LAGS: c_int = 3;
pub const GR_VCORR_STAT_LAST_WALK_GROUPS: c_int = 4;
pub const GR_VCORR_STAT_LAST_GRAM_GROUPS: c_int = 5;
pub const GR_VCORR_STAT_LAST_EACH_GROUPS: c_int = 6;
pub const GR_VCORR_STAT_LAST_BLOCKS: c_int = 7;
pub const GR_VCORR_STAT_COUNTED: c_int = 8;

#[repr(C)] pub struct gr_hbond_plan { _private: [u8; 0] }
#[repr(C)] pub struct gr_gridmap { _private: [u8; 0] }
#[repr(C)] pub struct gr_segments { _private: [u8; 0] }
#[repr(C)] pub struct gr_region { _private: [u8; 0] }
#[repr(C)] pub struct gr_contacts { _private: [u8; 0] }
#[repr(C)] pub struct gr_rmsd_panel { _private: [u8; 0] }
#[repr(C)] pub struct gr_fluct { _private: [u8; 0] }
#[repr(C)] pub struct gr_covar { _private: [u8; 0] }
#[repr(C)] pub struct gr_msd { _private: [u8; 0] }
#[repr(C)] pub struct gr_internals { _private: [u8; 0] }
#[repr(C)] pub struct gr_vcorr { _private: [u8; 0] }
#[repr(C)] pub struct gr_pool { _private: [u8; 0] }
#[repr(C)] pub struct gr_comm { _private: [u8; 0] }
/// `body(ctx, worker, frame, user, result)` of gr_pool_map: non-zero return = the frame's error (the first one wins)
/// `progress(user, status, frame, frames_done)` of gr_pool_map_range: GR_PROGRESS_RUNNING = 0 after every frame of worker 0,
/// then once GR_PROGRESS_COMPLETED = 1 / GR_PROGRESS_FAILED = 2 (ProgressPrinter + ProgressStatus, src/progress.rs)
pub type gr_pool_progress = Option<unsafe extern "C" fn(user: *mut c_void, status: c_int, frame: u64, frames_done: u64)>;
pub type gr_pool_body = Option<unsafe extern "C" fn(ctx: *mut gr_ctx, worker: c_int, frame: u64, user: *mut c_void, result: *mut c_float) -> c_int>;
extern "C" {
    pub fn gr_ctx_create(device: c_int, n_atoms: u64, n_slots: u32, status: *mut c_int) -> *mut gr_ctx;
    pub fn gr_ctx_destroy(ctx: *mut gr_ctx);
    pub fn gr_last_error_index(ctx: *const gr_ctx) -> u64;
    pub fn gr_last_error_counts(ctx: *const gr_ctx, counts: *mut u64);
    pub fn gr_ctx_set_strict_orthogonal(ctx: *mut gr_ctx, on: c_int) -> c_int;
    pub fn gr_set_masses(ctx: *mut gr_ctx, masses: *const c_float, n: u64) -> c_int;
    pub fn gr_group_create_from_ranges(ctx: *mut gr_ctx, name: *const c_char, start: *const u64, end: *const u64, n: usize) -> c_int;
    pub fn gr_frame_upload(ctx: *mut gr_ctx, slot: u32, xyz: *const c_float, box9: *const c_float) -> c_int;
    pub fn gr_frame_download(ctx: *mut gr_ctx, slot: u32, xyz: *mut c_float) -> c_int;
    pub fn gr_group_center(ctx: *mut gr_ctx, slot: u32, group: *const c_char, kind: c_int, weighted: c_int, out: *mut c_float) -> c_int;
    pub fn gr_group_distance(ctx: *mut gr_ctx, slot: u32, g1: *const c_char, g2: *const c_char, dim: c_int, out: *mut c_float) -> c_int;
    pub fn gr_group_all_distances(ctx: *mut gr_ctx, slot: u32, g1: *const c_char, g2: *const c_char, dim: c_int, out: *mut c_float, cap: usize) -> c_int;
    pub fn gr_group_all_distances_batch_device(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, g1: *const c_char, g2: *const c_char, dim: c_int,
                                               out_dev: *mut *mut c_float, n1: *mut u64, n2: *mut u64, status_out: *mut c_int) -> c_int;
    // group_all_distances + the reduction its callers apply (analysis.rs:1420-1451), without the matrix: GR_PD_MIN = 1, _MAX = 2, _COUNT_BELOW = 3, _HIST = 4
    pub fn gr_group_all_distances_reduce(ctx: *mut gr_ctx, slot: u32, g1: *const c_char, g2: *const c_char, dim: c_int, op: c_int, per_row: c_int, param: c_float,
                                         nbins: u32, out: *mut c_void, out_capacity_bytes: usize) -> c_int;
    pub fn gr_group_all_distances_reduce_batch(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, g1: *const c_char, g2: *const c_char, dim: c_int, op: c_int,
                                               per_row: c_int, param: c_float, nbins: u32, out: *mut c_void, out_capacity_bytes: usize, status_out: *mut c_int) -> c_int;
    // hydrogen bonds over a batch of resident frames (hbonds.rs:154-373); groups = n_chains x (acceptors, donors, hydrogens)
    pub fn gr_hbond_plan_create(ctx: *mut gr_ctx, groups: *const *const c_char, n_chains: u32, pairs: *const u32, n_pairs: u32, bonds: *const u64, n_bonds: u64,
                                max_distance: c_float, min_angle: c_float, status: *mut c_int) -> *mut gr_hbond_plan;
    pub fn gr_hbond_plan_destroy(plan: *mut gr_hbond_plan);
    pub fn gr_hbond_batch(plan: *mut gr_hbond_plan, first_slot: u32, n_frames: u32, max_bonds: u64, donor: *mut u32, hydrogen: *mut u32, acceptor: *mut u32,
                          distance: *mut c_float, angle: *mut c_float, offsets: *mut u64, n_total: *mut u64, status_out: *mut c_int) -> c_int;
    pub fn gr_trr_open(path: *const c_char, status: *mut c_int) -> *mut gr_trr;
    pub fn gr_trr_close(trr: *mut gr_trr);
    pub fn gr_trr_n_atoms(trr: *const gr_trr) -> u64;
    pub fn gr_trr_n_frames(trr: *const gr_trr) -> u64;
    pub fn gr_trr_frame_info(trr: *const gr_trr, frame: u64, step: *mut u64, time: *mut c_float, lambda: *mut c_float, box9: *mut c_float, sections: *mut c_int, double_precision: *mut c_int) -> c_int;
    pub fn gr_trr_read_frame(trr: *const gr_trr, frame: u64, xyz: *mut c_float, vel: *mut c_float, force: *mut c_float, box9: *mut c_float, step: *mut u64, time: *mut c_float, lambda: *mut c_float) -> c_int;
    pub fn gr_trr_writer_open(path: *const c_char, status: *mut c_int) -> *mut gr_trr_writer;
    pub fn gr_trr_writer_close(w: *mut gr_trr_writer) -> c_int;
    pub fn gr_trr_write_frame(w: *mut gr_trr_writer, n_atoms: u64, xyz: *const c_float, vel: *const c_float, force: *const c_float, box9: *const c_float, step: i64, time: c_float, lambda: c_float) -> c_int;
    pub fn gr_trr_read_frames_device(trr: *const gr_trr, first_frame: u64, n_frames: u32, frame_step: u64, ctx: *mut gr_ctx, first_slot: u32, steps: *mut u64, times: *mut c_float) -> c_int;
    pub fn gr_group_count(ctx: *const gr_ctx) -> u64;
    pub fn gr_group_name(ctx: *const gr_ctx, i: u64, name: *mut c_char, capacity: usize) -> c_int;
    pub fn gr_ctx_set_center_onepass_min(ctx: *mut gr_ctx, min_atoms: u32) -> c_int;
    pub fn gr_center_fallbacks(ctx: *const gr_ctx) -> u64;
    pub fn gr_device_read(ctx: *mut gr_ctx, dev: *const c_void, host: *mut c_void, bytes: usize) -> c_int;
    pub fn gr_group_translate(ctx: *mut gr_ctx, slot: u32, group: *const c_char, v: *const c_float) -> c_int;
    pub fn gr_group_wrap(ctx: *mut gr_ctx, slot: u32, group: *const c_char) -> c_int;
    pub fn gr_atoms_center(ctx: *mut gr_ctx, slot: u32, group: *const c_char, dim: c_int, weighted: c_int) -> c_int;
    pub fn gr_rmsd_plan_create(reference: *mut gr_ctx, ref_slot: u32, target: *mut gr_ctx, group: *const c_char, status: *mut c_int) -> *mut gr_rmsd_plan;
    pub fn gr_rmsd_plan_destroy(plan: *mut gr_rmsd_plan);
    pub fn gr_rmsd_batch(plan: *mut gr_rmsd_plan, first_slot: u32, n: u32, rmsd: *mut c_float, status: *mut c_int, rot: *mut c_float) -> c_int;
    pub fn gr_rmsd_fit_batch(plan: *mut gr_rmsd_plan, first_slot: u32, n: u32, rmsd: *mut c_float, status: *mut c_int) -> c_int;
    // anonymous selections = the iterator-level surface (src/structures/iterators.rs:886-1554): AtomContainer blocks in, no group name
    pub fn gr_sel_center(ctx: *mut gr_ctx, slot: u32, start: *const u64, end: *const u64, n_blocks: usize, kind: c_int, weighted: c_int, out: *mut c_float) -> c_int;
    pub fn gr_sel_translate(ctx: *mut gr_ctx, slot: u32, start: *const u64, end: *const u64, n_blocks: usize, v: *const c_float) -> c_int;
    pub fn gr_sel_wrap(ctx: *mut gr_ctx, slot: u32, start: *const u64, end: *const u64, n_blocks: usize) -> c_int;
    pub fn gr_sel_all_distances(ctx: *mut gr_ctx, slot: u32, s1: *const u64, e1: *const u64, n1: usize, s2: *const u64, e2: *const u64, n2: usize,
                                dim: c_int, out: *mut c_float, cap: usize) -> c_int;
    pub fn gr_sel_filter_geometry(ctx: *mut gr_ctx, slot: u32, start: *const u64, end: *const u64, n_blocks: usize, shapes: *const gr_shape, n_shapes: usize,
                                  naive: c_int, out_start: *mut u64, out_end: *mut u64, cap_blocks: usize, n_out_blocks: *mut usize, n_out_atoms: *mut u64) -> c_int;
    pub fn gr_frame_upload_wait(ctx: *mut gr_ctx, slot: u32) -> c_int;
    // geometry selection (src/structures/shape.rs, src/system/groups.rs:94-188)
    pub fn gr_shape_sphere(s: *mut gr_shape, position: *const c_float, radius: c_float) -> c_int;
    pub fn gr_shape_rectangular(s: *mut gr_shape, position: *const c_float, x: c_float, y: c_float, z: c_float) -> c_int;
    pub fn gr_shape_cylinder(s: *mut gr_shape, position: *const c_float, radius: c_float, height: c_float, orientation: c_int) -> c_int;
    pub fn gr_shape_triangular_prism(s: *mut gr_shape, b1: *const c_float, b2: *const c_float, b3: *const c_float, height: c_float) -> c_int;
    pub fn gr_group_create_from_geometries(ctx: *mut gr_ctx, slot: u32, name: *const c_char, source: *const c_char,
                                           shapes: *const gr_shape, n: usize, naive: c_int) -> c_int;
    // xtc frames unpacked on the device straight into frame slots (src/io/xtc_io/*: XtcReader + update_system)
    pub fn gr_xtc_open(path: *const c_char, status: *mut c_int) -> *mut gr_xtc;
    pub fn gr_xtc_close(xtc: *mut gr_xtc);
    pub fn gr_xtc_read_frames_device(xtc: *const gr_xtc, first_frame: u64, n_frames: u32, frame_step: u64, ctx: *mut gr_ctx,
                                     first_slot: u32, host_threads: c_int, steps: *mut u64, times: *mut c_float) -> c_int;
    // asynchronous batches, one-shot calls, batched per-frame calls, tuning, host memory, diagnostics
    pub fn gr_rmsd_batch_begin(plan: *mut gr_rmsd_plan, first_slot: u32, n_frames: u32, fit: c_int) -> c_int;
    pub fn gr_rmsd_batch_end(plan: *mut gr_rmsd_plan, rmsd: *mut c_float, status: *mut c_int, rot: *mut c_float) -> c_int;
    pub fn gr_rmsd_plan_last_fallbacks(plan: *const gr_rmsd_plan) -> u32;
    pub fn gr_calc_rmsd(ctx: *mut gr_ctx, slot: u32, reference: *mut gr_ctx, ref_slot: u32, group: *const c_char, rmsd: *mut c_float, rot: *mut c_float) -> c_int;
    pub fn gr_calc_rmsd_and_fit(ctx: *mut gr_ctx, slot: u32, reference: *mut gr_ctx, ref_slot: u32, group: *const c_char, rmsd: *mut c_float) -> c_int;
    pub fn gr_group_center_batch(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, group: *const c_char, kind: c_int, weighted: c_int, out: *mut c_float, status: *mut c_int) -> c_int;
    pub fn gr_group_translate_batch(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, group: *const c_char, v: *const c_float, status: *mut c_int) -> c_int;
    pub fn gr_group_wrap_batch(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, group: *const c_char, status: *mut c_int) -> c_int;
    pub fn gr_atoms_center_batch(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, ref_group: *const c_char, dim: c_int, weighted: c_int, status: *mut c_int) -> c_int;
    // bond topology and whole molecules (modifying.rs:235-487, iterating.rs:238-245,399-432)
    pub fn gr_add_bond(ctx: *mut gr_ctx, i: u64, j: u64) -> c_int;
    pub fn gr_add_bonds(ctx: *mut gr_ctx, pairs: *const u64, n_pairs: u64) -> c_int;
    pub fn gr_clear_bonds(ctx: *mut gr_ctx) -> c_int;
    pub fn gr_has_bonds(ctx: *const gr_ctx) -> c_int;
    pub fn gr_mol_references(ctx: *mut gr_ctx, out: *mut u64, cap: u64, n: *mut u64) -> c_int;
    pub fn gr_molecule_atoms(ctx: *mut gr_ctx, index: u64, out: *mut u64, cap: u64, n: *mut u64) -> c_int;
    pub fn gr_make_molecules_whole(ctx: *mut gr_ctx, slot: u32) -> c_int;
    pub fn gr_make_molecules_whole_batch(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, status: *mut c_int) -> c_int;
    pub fn gr_make_group_whole(ctx: *mut gr_ctx, slot: u32, group: *const c_char) -> c_int;
    pub fn gr_make_group_whole_batch(ctx: *mut gr_ctx, first_slot: u32, n_frames: u32, group: *const c_char, status: *mut c_int) -> c_int;
    // GridMap (src/structures/gridmap.rs) accumulated over batches of resident frames: count and integer coordinate sum per tile
    pub fn gr_gridmap_len(span: *const c_float, tile: c_float, n: *mut u64) -> c_int;
    pub fn gr_gridmap_coord2index(span0: c_float, tile: c_float, coord: c_float) -> i64;
    pub fn gr_gridmap_index2coord(span0: c_float, tile: c_float, index: u64) -> c_float;
    pub fn gr_gridmap_create(ctx: *mut gr_ctx, span_x: *const c_float, span_y: *const c_float, tile_dim: *const c_float, status: *mut c_int) -> *mut gr_gridmap;
    pub fn gr_gridmap_from_box(ctx: *mut gr_ctx, slot: u32, tile_dim: *const c_float, status: *mut c_int) -> *mut gr_gridmap;
    pub fn gr_gridmap_destroy(map: *mut gr_gridmap);
    pub fn gr_gridmap_dims(map: *const gr_gridmap, nx: *mut u64, ny: *mut u64, span_x: *mut c_float, span_y: *mut c_float, tile_dim: *mut c_float) -> c_int;
    pub fn gr_gridmap_stat(map: *const gr_gridmap, key: c_int, value: *mut u64) -> c_int;
    pub fn gr_gridmap_set_launch(map: *mut gr_gridmap, range_groups: u32, frame_groups: u32, check_groups: u32) -> c_int;
    pub fn gr_gridmap_clear(map: *mut gr_gridmap) -> c_int;
    pub fn gr_gridmap_accumulate_batch(map: *mut gr_gridmap, first_slot: u32, n_frames: u32, group: *const c_char, value: c_int, offset: *const c_float,
                                       flags: c_int, n_outside: *mut u64, status_out: *mut c_int) -> c_int;
    pub fn gr_gridmap_read(map: *mut gr_gridmap, count: *mut u64, sum_q: *mut i64, mean: *mut c_float) -> c_int;
    // Segments: the loop over group_split_by_resid / molecule_iter + group_get_com of each part (groups.rs:344-435, iterating.rs:238-245) as one call
    pub fn gr_segments_create(ctx: *mut gr_ctx, offsets: *const u64, atoms: *const u64, n_segments: u64, status: *mut c_int) -> *mut gr_segments;
    pub fn gr_segments_from_labels(ctx: *mut gr_ctx, group: *const c_char, labels: *const u64, status: *mut c_int) -> *mut gr_segments;
    pub fn gr_segments_from_molecules(ctx: *mut gr_ctx, status: *mut c_int) -> *mut gr_segments;
    pub fn gr_segments_destroy(seg: *mut gr_segments);
    pub fn gr_segments_count(seg: *const gr_segments) -> u64;
    pub fn gr_segments_sizes(seg: *const gr_segments, out: *mut u64) -> c_int;
    pub fn gr_segments_atoms(seg: *const gr_segments, s: u64, out: *mut u64, cap: u64, n: *mut u64) -> c_int;
    pub fn gr_segments_stat(seg: *const gr_segments, key: c_int, value: *mut u64) -> c_int;
    pub fn gr_segments_center_batch(seg: *mut gr_segments, first_slot: u32, n_frames: u32, kind: c_int, weighted: c_int, out: *mut c_float, status_out: *mut c_int) -> c_int;
    pub fn gr_segments_center_batch_device(seg: *mut gr_segments, first_slot: u32, n_frames: u32, kind: c_int, weighted: c_int,
                                           out_dev: *mut *mut c_float, n_segments: *mut u64, status_out: *mut c_int) -> c_int;
    // ... and their shape: centre, Rg and gyration tensor ([n_frames][M][10]), eigenvalues and principal axes ([n_frames][M][12])
    pub fn gr_segments_gyration_batch(seg: *mut gr_segments, first_slot: u32, n_frames: u32, kind: c_int, weighted: c_int, moments: *mut c_float, axes: *mut c_float,
                                      status_out: *mut c_int) -> c_int;
    pub fn gr_segments_gyration_batch_device(seg: *mut gr_segments, first_slot: u32, n_frames: u32, kind: c_int, weighted: c_int, want_axes: c_int,
                                             moments_dev: *mut *mut c_float, axes_dev: *mut *mut c_float, n_segments: *mut u64, status_out: *mut c_int) -> c_int;
    pub fn gr_segments_set_piece_frames(seg: *mut gr_segments, n: u32) -> c_int;
    // Region: group_iter(..).filter_geometry(..) / group_create_from_geometries for every frame of a block of resident slots
    pub fn gr_region_create(ctx: *mut gr_ctx, shapes: *const gr_shape, n_shapes: usize, naive: c_int, status: *mut c_int) -> *mut gr_region;
    pub fn gr_region_destroy(r: *mut gr_region);
    pub fn gr_region_select_batch(r: *mut gr_region, first_slot: u32, n_frames: u32, group: *const c_char, anchor: *const c_float,
                                  n_inside: *mut u64, status_out: *mut c_int) -> c_int;
    pub fn gr_region_read(r: *mut gr_region, offsets: *mut u64, atoms: *mut u64, cap: u64, n_total: *mut u64) -> c_int;
    pub fn gr_region_read_device(r: *mut gr_region, atoms_dev: *mut *const u32, offsets_dev: *mut *const u64, n_frames: *mut u64, n_total: *mut u64) -> c_int;
    pub fn gr_region_group(r: *mut gr_region, frame: u32, name: *const c_char) -> c_int;
    pub fn gr_region_set_piece_frames(r: *mut gr_region, n: u32) -> c_int;
    pub fn gr_region_stat(r: *const gr_region, key: c_int, value: *mut u64) -> c_int;
    // Contacts: CellGrid::new + neighbors_iter + distance filter for every frame of a block of resident slots
    pub fn gr_contacts_create(ctx: *mut gr_ctx, group1: *const c_char, group2: *const c_char, cutoff: c_float, status: *mut c_int) -> *mut gr_contacts;
    pub fn gr_contacts_destroy(ct: *mut gr_contacts);
    pub fn gr_contacts_pairs_batch(ct: *mut gr_contacts, first_slot: u32, n_frames: u32, max_pairs: u64, n_pairs: *mut u64, n_total: *mut u64,
                                   status_out: *mut c_int) -> c_int;
    pub fn gr_contacts_read(ct: *mut gr_contacts, offsets: *mut u64, i: *mut u32, j: *mut u32, d: *mut c_float, cap: u64, n_total: *mut u64) -> c_int;
    pub fn gr_contacts_read_device(ct: *mut gr_contacts, i_dev: *mut *const u32, j_dev: *mut *const u32, d_dev: *mut *const c_float,
                                   offsets_dev: *mut *const u64, n_frames: *mut u64, n_total: *mut u64) -> c_int;
    pub fn gr_contacts_count_batch(ct: *mut gr_contacts, first_slot: u32, n_frames: u32, per_atom: *mut u32, n_pairs: *mut u64, status_out: *mut c_int) -> c_int;
    pub fn gr_contacts_hist_batch(ct: *mut gr_contacts, first_slot: u32, n_frames: u32, nbins: u32, hist: *mut u64, status_out: *mut c_int) -> c_int;
    pub fn gr_contacts_sizes(ct: *const gr_contacts, n1: *mut u64, n2: *mut u64) -> c_int;
    pub fn gr_contacts_set_piece_frames(ct: *mut gr_contacts, n: u32) -> c_int;
    pub fn gr_contacts_set_walk_groups(ct: *mut gr_contacts, n: u32) -> c_int;
    pub fn gr_contacts_stat(ct: *const gr_contacts, key: c_int, value: *mut u64) -> c_int;
    // RMSDPanel: packed centred frames of a group and the all-pairs RMSD matrix of two panels (cols may be null: rows against itself)
    pub fn gr_rmsd_panel_create(ctx: *mut gr_ctx, group: *const c_char, capacity_frames: u32, status: *mut c_int) -> *mut gr_rmsd_panel;
    pub fn gr_rmsd_panel_destroy(p: *mut gr_rmsd_panel);
    pub fn gr_rmsd_panel_append_batch(p: *mut gr_rmsd_panel, first_slot: u32, n_frames: u32, status_out: *mut c_int) -> c_int;
    pub fn gr_rmsd_panel_clear(p: *mut gr_rmsd_panel) -> c_int;
    pub fn gr_rmsd_panel_frames(p: *const gr_rmsd_panel) -> u32;
    pub fn gr_rmsd_panel_n_atoms(p: *const gr_rmsd_panel) -> u64;
    pub fn gr_rmsd_panel_status(p: *const gr_rmsd_panel, out: *mut c_int) -> c_int;
    pub fn gr_rmsd_panel_set_block_entries(p: *mut gr_rmsd_panel, n: u64) -> c_int;
    pub fn gr_rmsd_matrix(rows: *mut gr_rmsd_panel, cols: *mut gr_rmsd_panel, out: *mut c_float) -> c_int;
    pub fn gr_rmsd_matrix_device(rows: *mut gr_rmsd_panel, cols: *mut gr_rmsd_panel, out_dev: *mut *mut c_float, n_rows: *mut u32, n_cols: *mut u32) -> c_int;
    // Fluctuations: mean structure and per-atom RMSF of a group accumulated over resident frames (status_out and the outputs of read / read_raw may be null)
    pub fn gr_fluct_create(ctx: *mut gr_ctx, group: *const c_char, status: *mut c_int) -> *mut gr_fluct;
    pub fn gr_fluct_destroy(f: *mut gr_fluct);
    pub fn gr_fluct_accumulate_batch(f: *mut gr_fluct, first_slot: u32, n_frames: u32, status_out: *mut c_int) -> c_int;
    pub fn gr_fluct_clear(f: *mut gr_fluct) -> c_int;
    pub fn gr_fluct_frames(f: *const gr_fluct) -> u64;
    pub fn gr_fluct_n_atoms(f: *const gr_fluct) -> u64;
    pub fn gr_fluct_read(f: *mut gr_fluct, mean: *mut f64, var: *mut f64, rmsf: *mut f64) -> c_int;
    pub fn gr_fluct_read_raw(f: *mut gr_fluct, origin: *mut c_float, sum: *mut f64, sumsq: *mut f64, n: *mut u64) -> c_int;
    pub fn gr_fluct_merge(dst: *mut gr_fluct, src: *mut gr_fluct) -> c_int;
    pub fn gr_fluct_store_mean(f: *mut gr_fluct, dst: *mut gr_ctx, slot: u32) -> c_int;
    pub fn gr_fluct_set_launch(f: *mut gr_fluct, range_groups: u32, check_groups: u32) -> c_int;
    pub fn gr_fluct_stat(f: *const gr_fluct, key: c_int, value: *mut u64) -> c_int;
    // Covariance: positional covariance matrix and DCCM of a group accumulated over resident frames (status_out and the outputs of read / read_raw may be null)
    pub fn gr_covar_create(ctx: *mut gr_ctx, group: *const c_char, status: *mut c_int) -> *mut gr_covar;
    pub fn gr_covar_destroy(cv: *mut gr_covar);
    pub fn gr_covar_accumulate_batch(cv: *mut gr_covar, first_slot: u32, n_frames: u32, status_out: *mut c_int) -> c_int;
    pub fn gr_covar_clear(cv: *mut gr_covar) -> c_int;
    pub fn gr_covar_frames(cv: *const gr_covar) -> u64;
    pub fn gr_covar_n_atoms(cv: *const gr_covar) -> u64;
    pub fn gr_covar_read(cv: *mut gr_covar, mean: *mut f64, cov: *mut f64, flags: u32) -> c_int;
    pub fn gr_covar_read_raw(cv: *mut gr_covar, origin: *mut c_float, sum: *mut f64, q: *mut f64, n: *mut u64) -> c_int;
    pub fn gr_covar_read_dccm(cv: *mut gr_covar, corr: *mut f64) -> c_int;
    pub fn gr_covar_merge(dst: *mut gr_covar, src: *mut gr_covar) -> c_int;
    pub fn gr_covar_set_launch(cv: *mut gr_covar, product_groups: u32, check_groups: u32) -> c_int;
    pub fn gr_covar_stat(cv: *const gr_covar, key: c_int, value: *mut u64) -> c_int;
    // MSD: nojump unwrapping and the windowed mean-squared displacement of a group over resident frames (flags: GR_MSD_X | _Y | _Z, GR_MSD_NOJUMP; status_out, msd and pairs may be null)
    pub fn gr_msd_create(ctx: *mut gr_ctx, group: *const c_char, capacity_frames: u32, flags: u32, status: *mut c_int) -> *mut gr_msd;
    pub fn gr_msd_destroy(m: *mut gr_msd);
    pub fn gr_msd_append_batch(m: *mut gr_msd, first_slot: u32, n_frames: u32, status_out: *mut c_int) -> c_int;
    pub fn gr_msd_clear(m: *mut gr_msd) -> c_int;
    pub fn gr_msd_frames(m: *const gr_msd) -> u64;
    pub fn gr_msd_n_atoms(m: *const gr_msd) -> u64;
    pub fn gr_msd_capacity(m: *const gr_msd) -> u64;
    pub fn gr_msd_compute(m: *mut gr_msd, max_lag: u32) -> c_int;
    pub fn gr_msd_read(m: *mut gr_msd, msd: *mut f64, pairs: *mut u64) -> c_int;
    pub fn gr_msd_read_from_origin(m: *mut gr_msd, out: *mut f64) -> c_int;
    pub fn gr_msd_read_displacements(m: *mut gr_msd, t0: u32, nt: u32, out: *mut c_float) -> c_int;
    pub fn gr_msd_set_launch(m: *mut gr_msd, walk_groups: u32, gram_groups: u32) -> c_int;
    pub fn gr_msd_stat(m: *const gr_msd, key: c_int, value: *mut u64) -> c_int;
    // Internals: distance (kind 1), angle (2), dihedral (3) and axis-cosine (4) series of atom tuples over resident frames and their running statistics (flags: GR_IC_PBC = 1; axis: 3 floats for kind 4, else null; status_out, mean, var, origin, sum, sumsq and n may be null)
    pub fn gr_internals_create(ctx: *mut gr_ctx, kind: c_int, atoms: *const u64, n_tuples: u64, flags: u32, axis: *const c_float, status: *mut c_int) -> *mut gr_internals;
    pub fn gr_internals_destroy(ic: *mut gr_internals);
    pub fn gr_internals_count(ic: *const gr_internals) -> u64;
    pub fn gr_internals_frames(ic: *const gr_internals) -> u64;
    pub fn gr_internals_values_batch(ic: *mut gr_internals, first_slot: u32, n_frames: u32, out: *mut c_float, status_out: *mut c_int) -> c_int;
    pub fn gr_internals_values_batch_device(ic: *mut gr_internals, first_slot: u32, n_frames: u32, out_dev: *mut c_float, ld: u64, status_out: *mut c_int) -> c_int;
    pub fn gr_internals_accumulate_batch(ic: *mut gr_internals, first_slot: u32, n_frames: u32, status_out: *mut c_int) -> c_int;
    pub fn gr_internals_clear(ic: *mut gr_internals) -> c_int;
    pub fn gr_internals_read(ic: *mut gr_internals, mean: *mut f64, var: *mut f64) -> c_int;
    pub fn gr_internals_read_raw(ic: *mut gr_internals, origin: *mut c_float, sum: *mut f64, sumsq: *mut f64, n: *mut u64) -> c_int;
    pub fn gr_internals_merge(dst: *mut gr_internals, src: *mut gr_internals) -> c_int;
    pub fn gr_internals_set_launch(ic: *mut gr_internals, tuple_ranges: u32, frame_chunk: u32) -> c_int;
    pub fn gr_internals_stat(ic: *const gr_internals, key: c_int, value: *mut u64) -> c_int;
    // VectorCorrelation: P1 / P2 reorientation autocorrelation of V bond vectors over resident frames (atoms: [V][2]; flags: GR_VCORR_PBC | _UNIT | _P1 | _P2; status_out, c1, c2, pairs and one of c1_out / c2_out may be null)
    pub fn gr_vcorr_create(ctx: *mut gr_ctx, atoms: *const u64, n_vectors: u64, capacity_frames: u32, flags: u32, status: *mut c_int) -> *mut gr_vcorr;
    pub fn gr_vcorr_destroy(vc: *mut gr_vcorr);
    pub fn gr_vcorr_count(vc: *const gr_vcorr) -> u64;
    pub fn gr_vcorr_frames(vc: *const gr_vcorr) -> u64;
    pub fn gr_vcorr_capacity(vc: *const gr_vcorr) -> u64;
    pub fn gr_vcorr_append_batch(vc: *mut gr_vcorr, first_slot: u32, n_frames: u32, status_out: *mut c_int) -> c_int;
    pub fn gr_vcorr_clear(vc: *mut gr_vcorr) -> c_int;
    pub fn gr_vcorr_compute(vc: *mut gr_vcorr, max_lag: u32) -> c_int;
    pub fn gr_vcorr_read(vc: *mut gr_vcorr, c1: *mut f64, c2: *mut f64, pairs: *mut u64) -> c_int;
    pub fn gr_vcorr_compute_each(vc: *mut gr_vcorr, max_lag: u32, c1_out: *mut f64, c2_out: *mut f64) -> c_int;
    pub fn gr_vcorr_read_vectors(vc: *mut gr_vcorr, t0: u32, nt: u32, out: *mut c_float) -> c_int;
    pub fn gr_vcorr_set_launch(vc: *mut gr_vcorr, walk_groups: u32, gram_groups: u32, each_groups: u32) -> c_int;
    pub fn gr_vcorr_stat(vc: *const gr_vcorr, key: c_int, value: *mut u64) -> c_int;
    pub fn gr_ctx_set_tuning(ctx: *mut gr_ctx, key: c_int, value: i64) -> c_int;   // GR_TUNE_* (include/groan_hip.h)
    pub fn gr_host_alloc(bytes: usize) -> *mut c_void;                              // pinned memory: asynchronous gr_frame_upload
    pub fn gr_host_free(p: *mut c_void);
    pub fn gr_sync(ctx: *mut gr_ctx) -> c_int;
    pub fn gr_last_error(ctx: *const gr_ctx) -> *const c_char;
    pub fn gr_status_string(status: c_int) -> *const c_char;
    // traj_iter_map_reduce across GPUs (src/system/parallel.rs:208-481): in one process ...
    pub fn gr_pool_create(devices: *const c_int, n_workers: c_int, n_atoms: u64, n_slots: u32, status: *mut c_int) -> *mut gr_pool;
    pub fn gr_pool_destroy(pool: *mut gr_pool);
    pub fn gr_pool_size(pool: *const gr_pool) -> c_int;
    pub fn gr_pool_ctx(pool: *mut gr_pool, worker: c_int) -> *mut gr_ctx;
    pub fn gr_pool_last_error(pool: *const gr_pool) -> *const c_char;
    pub fn gr_pool_map(pool: *mut gr_pool, n_frames: u64, body: gr_pool_body, user: *mut c_void, width: usize, results: *mut c_float,
                       frames_done: *mut u64, error_frame: *mut u64) -> c_int;
    /// traj_iter_map_reduce's start_time / end_time / step (frame-index form) and its progress printer (parallel.rs:208-222,417-448)
    pub fn gr_pool_map_range(pool: *mut gr_pool, first_frame: u64, end_frame: u64, step: u64, body: gr_pool_body, user: *mut c_void, width: usize,
                             results: *mut c_float, progress: gr_pool_progress, progress_user: *mut c_void, frames_done: *mut u64, error_frame: *mut u64) -> c_int;
    pub fn gr_comm_set_library(path: *const c_char) -> c_int;
    pub fn gr_ctx_stat(ctx: *const gr_ctx, key: c_int, value: *mut u64) -> c_int;   // GR_STAT_* (include/groan_hip.h)
    // ... and one process per GPU (RCCL over xGMI: one final all-gather + the shared error flag)
    pub fn gr_comm_unique_id(id128: *mut c_void) -> c_int;
    pub fn gr_comm_create(device: c_int, rank: c_int, world: c_int, id128: *const c_void, status: *mut c_int) -> *mut gr_comm;
    pub fn gr_comm_destroy(comm: *mut gr_comm);
    pub fn gr_comm_last_error(comm: *const gr_comm) -> *const c_char;
    pub fn gr_comm_library() -> *const c_char;
    pub fn gr_comm_gather_per_frame(comm: *mut gr_comm, local: *const c_float, n_total: u64, width: usize, out: *mut c_float) -> c_int;
    pub fn gr_comm_any_error(comm: *mut gr_comm, local_flag: c_int, any: *mut c_int) -> c_int;
    pub fn gr_shard_deinterleave(gathered: *const c_float, world: c_int, n_total: u64, width: usize, out: *mut c_float);
    // GroupXtcReader (partial-frame reads, molly_xtc.rs:475-560)
    pub fn gr_xtc_read_frame_prefix(xtc: *const gr_xtc, frame: u64, n_prefix: u64, xyz: *mut c_float, box9: *mut c_float, step: *mut u64, time: *mut c_float,
                                    precision: *mut c_float, stream_bytes_read: *mut u64) -> c_int;
    pub fn gr_xtc_read_frames_device_group(xtc: *const gr_xtc, first_frame: u64, n_frames: u32, frame_step: u64, ctx: *mut gr_ctx, first_slot: u32,
                                           group: *const c_char, host_threads: c_int, steps: *mut u64, times: *mut c_float) -> c_int;
}

#[repr(C)] pub struct gr_xtc { _private: [u8; 0] }
#[repr(C)] pub struct gr_trr { _private: [u8; 0] }
#[repr(C)] pub struct gr_trr_writer { _private: [u8; 0] }
/// `gr_shape` of include/groan_hip.h: filled by the `gr_shape_*` constructors from the fields of
/// `Sphere` / `Rectangular` / `Cylinder` / `TriangularPrism` (src/structures/shape.rs:17-68).
#[repr(C)] #[derive(Clone, Copy, Default)]
pub struct gr_shape { pub kind: c_int, pub position: [c_float; 3], pub size: [c_float; 3], pub base2: [c_float; 3], pub base3: [c_float; 3],
                      pub orientation: c_int, pub plane: c_int }

/// Device mirror of one `System` (one per worker thread / per GPU, like the clones of `traj_iter_map_reduce`).
pub struct HipSystem { ctx: *mut gr_ctx, n_atoms: usize, _not_sync: PhantomData<*mut ()> }
unsafe impl Send for HipSystem {}

impl Drop for HipSystem { fn drop(&mut self) { unsafe { gr_ctx_destroy(self.ctx) } } }

fn simbox_err(status: c_int) -> SimBoxError {
    if status == GR_E_NOT_ORTHOGONAL { SimBoxError::NotOrthogonal } else { SimBoxError::DoesNotExist }
}

impl HipSystem {
    /// Mirror masses and groups of `system` on `device`; positions follow with `upload`.
    pub fn new(system: &System, device: i32, n_slots: u32) -> Option<Self> {
        let mut st = 0;
        let n = system.get_n_atoms();
        let ctx = unsafe { gr_ctx_create(device, n as u64, n_slots, &mut st) };
        if ctx.is_null() { return None; }
        let masses: Vec<f32> = system.atoms_iter().map(|a| a.get_mass().unwrap_or(f32::NAN)).collect();
        unsafe { gr_set_masses(ctx, masses.as_ptr(), n as u64) };
        let me = HipSystem { ctx, n_atoms: n, _not_sync: PhantomData };
        for (name, group) in system.get_groups().iter() {
            me.group_from_container(name, group.get_atoms());
        }
        Some(me)
    }

    pub fn group_from_container(&self, name: &str, container: &AtomContainer) {
        let (s, e): (Vec<u64>, Vec<u64>) = container.blocks().map(|(a, b)| (a as u64, b as u64)).unzip();
        let cname = CString::new(name).unwrap();
        unsafe { gr_group_create_from_ranges(self.ctx, cname.as_ptr(), s.as_ptr(), e.as_ptr(), s.len()) };
    }

    /// `TrajRead::update_system` for the device copy: `coords` is the `[[f32; 3]]` the xtc readers produce.
    pub fn upload(&self, slot: u32, coords: &[[f32; 3]], simbox: Option<&SimBox>) {
        assert_eq!(coords.len(), self.n_atoms);
        let b9 = simbox.map(|b| [b.v1x, b.v2y, b.v3z, b.v1y, b.v1z, b.v2x, b.v2z, b.v3x, b.v3y]);
        let bp = b9.as_ref().map_or(std::ptr::null(), |b| b.as_ptr());
        unsafe { gr_frame_upload(self.ctx, slot, coords.as_ptr() as *const c_float, bp) };
    }

    fn group_error(&self, status: c_int, name: &str) -> GroupError {
        let idx = unsafe { gr_last_error_index(self.ctx) } as usize;
        match status {
            GR_E_GROUP_NOT_FOUND => GroupError::NotFound(name.to_owned()),
            GR_E_EMPTY_GROUP => GroupError::EmptyGroup(name.to_owned()),
            GR_E_NO_POSITION => GroupError::InvalidPosition(PositionError::NoPosition(idx)),
            GR_E_NO_MASS => GroupError::InvalidMass(MassError::NoMass(idx)),
            s => GroupError::InvalidSimBox(simbox_err(s)),
        }
    }

    /// `System::group_get_com` (src/system/analysis.rs:258-274)
    pub fn group_get_com(&self, slot: u32, name: &str) -> Result<Vector3D, GroupError> {
        let cname = CString::new(name).unwrap();
        let mut out = [0f32; 3];
        match unsafe { gr_group_center(self.ctx, slot, cname.as_ptr(), 2, 1, out.as_mut_ptr()) } {
            GR_OK => Ok(Vector3D::new(out[0], out[1], out[2])),
            s => Err(self.group_error(s, name)),
        }
    }

    /// `System::group_distance` (analysis.rs:348-360)
    pub fn group_distance(&self, slot: u32, g1: &str, g2: &str, dim: Dimension) -> Result<f32, GroupError> {
        let (a, b) = (CString::new(g1).unwrap(), CString::new(g2).unwrap());
        let mut out = 0f32;
        match unsafe { gr_group_distance(self.ctx, slot, a.as_ptr(), b.as_ptr(), dim as c_int, &mut out) } {
            GR_OK => Ok(out),
            s => Err(self.group_error(s, g1)),
        }
    }
}

/// Bond topology and whole molecules on the device (`System::add_bond` / `clear_bonds` / `has_bonds` / `make_molecules_whole` /
/// `make_group_whole`, src/system/modifying.rs:235-487).  Copy the system's bonds once with `add_bonds`; a frame that fails is
/// left untouched (the reference has already moved the molecules before the failing one).
impl HipSystem {
    fn bond_error(&self, status: c_int) -> AtomError {
        if status == GR_E_INVALID_BOND {
            let mut c = [0u64; 2];
            unsafe { gr_last_error_counts(self.ctx, c.as_mut_ptr()) };
            return AtomError::InvalidBond(c[0] as usize, c[1] as usize);
        }
        self.atom_error(status)
    }
    pub fn add_bond(&self, i: usize, j: usize) -> Result<(), AtomError> {
        match unsafe { gr_add_bond(self.ctx, i as u64, j as u64) } { GR_OK => Ok(()), s => Err(self.bond_error(s)) }
    }
    /// the bonds of `system` (each once, i < j), e.g. after `add_bonds_from_pdb`
    pub fn add_bonds_from(&self, system: &System) -> Result<(), AtomError> {
        let mut flat: Vec<u64> = Vec::new();
        for atom in system.atoms_iter() {
            for j in atom.get_bonded().iter() {
                if atom.get_index() < j { flat.push(atom.get_index() as u64); flat.push(j as u64); }
            }
        }
        match unsafe { gr_add_bonds(self.ctx, flat.as_ptr(), (flat.len() / 2) as u64) } { GR_OK => Ok(()), s => Err(self.bond_error(s)) }
    }
    pub fn clear_bonds(&self) { unsafe { gr_clear_bonds(self.ctx) }; }
    pub fn has_bonds(&self) -> bool { unsafe { gr_has_bonds(self.ctx) != 0 } }
    pub fn get_mol_references(&self) -> Vec<usize> {
        let mut n = 0u64;
        unsafe { gr_mol_references(self.ctx, std::ptr::null_mut(), 0, &mut n) };
        let mut out = vec![0u64; n as usize];
        unsafe { gr_mol_references(self.ctx, out.as_mut_ptr(), n, &mut n) };
        out.into_iter().map(|x| x as usize).collect()
    }
    /// `molecule_iter(index)` order (iterating.rs:399-432)
    pub fn molecule_indices(&self, index: usize) -> Result<Vec<usize>, AtomError> {
        let mut n = 0u64;
        let st = unsafe { gr_molecule_atoms(self.ctx, index as u64, std::ptr::null_mut(), 0, &mut n) };
        if st != GR_OK { return Err(self.atom_error(st)); }
        let mut out = vec![0u64; n as usize];
        unsafe { gr_molecule_atoms(self.ctx, index as u64, out.as_mut_ptr(), n, &mut n) };
        Ok(out.into_iter().map(|x| x as usize).collect())
    }
    pub fn make_molecules_whole(&self, slot: u32) -> Result<(), AtomError> {
        match unsafe { gr_make_molecules_whole(self.ctx, slot) } { GR_OK => Ok(()), s => Err(self.atom_error(s)) }
    }
    /// per-frame results of `n_frames` consecutive slots (one set of launches, one read-back)
    pub fn make_molecules_whole_batch(&self, first_slot: u32, n_frames: u32) -> Vec<Result<(), AtomError>> {
        let mut st = vec![0 as c_int; n_frames as usize];
        unsafe { gr_make_molecules_whole_batch(self.ctx, first_slot, n_frames, st.as_mut_ptr()) };
        st.into_iter().map(|s| if s == GR_OK { Ok(()) } else { Err(self.atom_error_plain(s)) }).collect()
    }
    pub fn make_group_whole(&self, slot: u32, name: &str) -> Result<(), GroupError> {
        let cname = CString::new(name).unwrap();
        match unsafe { gr_make_group_whole(self.ctx, slot, cname.as_ptr()) } { GR_OK => Ok(()), s => Err(self.group_error(s, name)) }
    }
    /// the per-frame statuses (GR_OK or the frame's error); Err for the call-level group errors
    pub fn make_group_whole_batch(&self, first_slot: u32, n_frames: u32, name: &str) -> Result<Vec<c_int>, GroupError> {
        let cname = CString::new(name).unwrap();
        let mut st = vec![0 as c_int; n_frames as usize];
        match unsafe { gr_make_group_whole_batch(self.ctx, first_slot, n_frames, cname.as_ptr(), st.as_mut_ptr()) } {
            s @ (GR_E_GROUP_NOT_FOUND | GR_E_EMPTY_GROUP) => Err(self.group_error(s, name)),
            _ => Ok(st),
        }
    }
    /// a frame's status without its atom index (only the first failed frame's index is kept by the library)
    fn atom_error_plain(&self, status: c_int) -> AtomError {
        match status {
            GR_E_NO_POSITION => AtomError::InvalidPosition(PositionError::NoPosition(usize::MAX)),
            s => AtomError::InvalidSimBox(simbox_err(s)),
        }
    }
}

/// The iterator-level surface on the device: what `AtomIterable` / `AtomIteratorWithBox` / `MutAtomIteratorWithBox`
/// (src/structures/iterators.rs:842-1554) compute for an `AtomContainer`, as ONE call each into the anonymous-selection entry
/// points -- no named group is created.  Obtain one from `HipSystem::iter_container` with the container of
/// `system.group_iter(..)`, `atoms_iter()`, a union / intersection (`container.rs:268-291`) ...
/// Error behaviour is the iterator traits': box first (`AtomError::InvalidSimBox`), then the first atom without position /
/// mass; an empty container yields `Vector3D(NaN, NaN, NaN)`, not an error (iterators.rs:1186-1188).
pub struct HipAtomIterator<'a> { sys: &'a HipSystem, slot: u32, start: Vec<u64>, end: Vec<u64> }

impl HipSystem {
    pub fn iter_container(&self, slot: u32, container: &AtomContainer) -> HipAtomIterator<'_> {
        let (start, end): (Vec<u64>, Vec<u64>) = container.blocks().map(|(a, b)| (a as u64, b as u64)).unzip();
        HipAtomIterator { sys: self, slot, start, end }
    }
    fn atom_error(&self, status: c_int) -> AtomError {
        let idx = unsafe { gr_last_error_index(self.ctx) } as usize;
        match status {
            GR_E_NO_POSITION => AtomError::InvalidPosition(PositionError::NoPosition(idx)),
            GR_E_NO_MASS => AtomError::InvalidMass(MassError::NoMass(idx)),
            9 /* GR_E_OUT_OF_RANGE */ => AtomError::OutOfRange(idx),
            s => AtomError::InvalidSimBox(simbox_err(s)),
        }
    }
}

impl<'a> HipAtomIterator<'a> {
    fn center(&self, kind: c_int, weighted: c_int) -> Result<Vector3D, AtomError> {
        let mut out = [0f32; 3];
        match unsafe { gr_sel_center(self.sys.ctx, self.slot, self.start.as_ptr(), self.end.as_ptr(), self.start.len(), kind, weighted, out.as_mut_ptr()) } {
            GR_OK => Ok(Vector3D::new(out[0], out[1], out[2])),
            s => Err(self.sys.atom_error(s)),
        }
    }
    pub fn get_center_naive(&self) -> Result<Vector3D, AtomError> { self.center(0, 0) }   // iterators.rs:886-903
    pub fn get_com_naive(&self) -> Result<Vector3D, AtomError> { self.center(0, 1) }      // :946-967
    pub fn estimate_center(&self) -> Result<Vector3D, AtomError> { self.center(1, 0) }    // :1152-1191
    pub fn estimate_com(&self) -> Result<Vector3D, AtomError> { self.center(1, 1) }       // :1314-1357
    pub fn get_center(&self) -> Result<Vector3D, AtomError> { self.center(2, 0) }         // :1237-1266
    pub fn get_com(&self) -> Result<Vector3D, AtomError> { self.center(2, 1) }            // :1404-1438
    /// `MutAtomIteratorWithBox::translate` (:1520-1524)
    pub fn translate(&self, v: &Vector3D) -> Result<(), AtomError> {
        let a = [v.x, v.y, v.z];
        match unsafe { gr_sel_translate(self.sys.ctx, self.slot, self.start.as_ptr(), self.end.as_ptr(), self.start.len(), a.as_ptr()) } { GR_OK => Ok(()), s => Err(self.sys.atom_error(s)) }
    }
    /// `MutAtomIteratorWithBox::wrap` (:1548-1553)
    pub fn wrap(&self) -> Result<(), AtomError> {
        match unsafe { gr_sel_wrap(self.sys.ctx, self.slot, self.start.as_ptr(), self.end.as_ptr(), self.start.len()) } { GR_OK => Ok(()), s => Err(self.sys.atom_error(s)) }
    }
    /// `AtomIteratorWithBox::filter_geometry` / `filter_geometry_naive` (:994-1004,1094-1105): the blocks of the filtered container
    pub fn filter_geometry(&self, shape: &gr_shape, naive: bool) -> Result<Vec<(usize, usize)>, AtomError> {
        let cap = self.start.iter().zip(&self.end).map(|(a, b)| (b - a + 1) as usize).sum::<usize>().max(1);
        let (mut os, mut oe) = (vec![0u64; cap], vec![0u64; cap]);
        let (mut nb, mut na) = (0usize, 0u64);
        match unsafe { gr_sel_filter_geometry(self.sys.ctx, self.slot, self.start.as_ptr(), self.end.as_ptr(), self.start.len(), shape, 1, naive as c_int,
                                              os.as_mut_ptr(), oe.as_mut_ptr(), cap, &mut nb, &mut na) } {
            GR_OK => Ok(os[..nb].iter().zip(&oe[..nb]).map(|(a, b)| (*a as usize, *b as usize)).collect()),
            s => Err(self.sys.atom_error(s)),
        }
    }
}

/// Batched form of `HipRmsd` for trajectory loops that can look ahead: `push` stages a frame into the next free slot (one
/// copy out of the `System`, one asynchronous upload), `flush` runs ONE `gr_rmsd_batch` over everything staged -- the
/// library's batched path instead of one launch + synchronisation per frame.
/// THIS is the adapter to use for throughput.  The per-frame `HipRmsd` below keeps the reference's `FrameAnalyze` contract (one
/// result per `analyze` call) and therefore runs batches of ONE frame: a launch + a synchronisation per frame and, for systems
/// that fill the chip, never the single-pass resident kernel (which needs >= 16 frames per call) --
/// about a tenth of the batched rate at 1e6 atoms.  Use a capacity of >= 64 (256-1024 for large systems).
pub struct HipRmsdBatch { inner: HipRmsd, staged: u32, capacity: u32, pinned: Vec<Vec<[f32; 3]>> }
impl HipRmsdBatch {
    pub fn new(reference: &System, target: &System, group: &str, device: i32, capacity: u32) -> Result<Self, RMSDError> {
        let mut inner = HipRmsd::new(reference, target, group, device)?;
        inner.target = HipSystem::new(target, device, capacity).ok_or_else(|| RMSDError::NonexistentGroup(group.to_owned()))?;
        let cname = CString::new(group).unwrap();
        let mut st = 0;
        unsafe { gr_rmsd_plan_destroy(inner.plan) };
        inner.plan = unsafe { gr_rmsd_plan_create(inner._reference.ctx, 0, inner.target.ctx, cname.as_ptr(), &mut st) };
        if inner.plan.is_null() { return Err(rmsd_error(&inner._reference, st, group)); }
        Ok(HipRmsdBatch { inner, staged: 0, capacity, pinned: (0..capacity).map(|_| Vec::new()).collect() })
    }
    pub fn is_full(&self) -> bool { self.staged == self.capacity }
    pub fn push(&mut self, system: &System) {
        let buf = &mut self.pinned[self.staged as usize];
        buf.clear();
        buf.extend(system.atoms_iter().map(|a| a.get_position().map_or([f32::NAN; 3], |p| [p.x, p.y, p.z])));
        self.inner.target.upload(self.staged, buf, system.get_box());
        self.staged += 1;
    }
    pub fn flush(&mut self) -> Result<Vec<f32>, RMSDError> {
        let n = self.staged;
        self.staged = 0;
        let (mut r, mut st) = (vec![0f32; n as usize], vec![0 as c_int; n as usize]);
        match unsafe { gr_rmsd_batch(self.inner.plan, 0, n, r.as_mut_ptr(), st.as_mut_ptr(), std::ptr::null_mut()) } {
            GR_OK => Ok(r),
            s => Err(rmsd_error(&self.inner.target, s, &self.inner.group)),
        }
    }
}

/// `RMSDConverterAnalyzer` (src/system/rmsd.rs:170-251) on the GPU: same trait impls, so
/// `system.xtc_iter(f)?.analyze(HipRmsd::new(..)?)` / `.convert_and_analyze(..)` work unchanged.
pub struct HipRmsd { plan: *mut gr_rmsd_plan, target: HipSystem, _reference: HipSystem, group: String, scratch: Vec<[f32; 3]> }

impl Drop for HipRmsd { fn drop(&mut self) { unsafe { gr_rmsd_plan_destroy(self.plan) } } }

impl HipRmsd {
    pub fn new(reference: &System, target: &System, group: &str, device: i32) -> Result<Self, RMSDError> {
        let r = HipSystem::new(reference, device, 1).ok_or_else(|| RMSDError::NonexistentGroup(group.to_owned()))?;
        let t = HipSystem::new(target, device, 1).ok_or_else(|| RMSDError::NonexistentGroup(group.to_owned()))?;
        let coords: Vec<[f32; 3]> = reference.atoms_iter().map(|a| a.get_position().map_or([f32::NAN; 3], |p| [p.x, p.y, p.z])).collect();
        r.upload(0, &coords, reference.get_box());
        let cname = CString::new(group).unwrap();
        let mut st = 0;
        let plan = unsafe { gr_rmsd_plan_create(r.ctx, 0, t.ctx, cname.as_ptr(), &mut st) };
        if plan.is_null() { return Err(rmsd_error(&r, st, group)); }
        Ok(HipRmsd { plan, target: t, _reference: r, group: group.to_owned(), scratch: Vec::new() })
    }

    fn stage(&mut self, system: &System) {
        self.scratch.clear();
        self.scratch.extend(system.atoms_iter().map(|a| a.get_position().map_or([f32::NAN; 3], |p| [p.x, p.y, p.z])));
        self.target.upload(0, &self.scratch, system.get_box());
    }
}

fn rmsd_error(sys: &HipSystem, status: c_int, group: &str) -> RMSDError {
    let idx = unsafe { gr_last_error_index(sys.ctx) } as usize;
    match status {
        GR_E_GROUP_NOT_FOUND => RMSDError::NonexistentGroup(group.to_owned()),
        GR_E_EMPTY_GROUP => RMSDError::EmptyGroup(group.to_owned()),
        GR_E_NO_POSITION => RMSDError::InvalidPosition(PositionError::NoPosition(idx)),
        GR_E_NO_MASS => RMSDError::InvalidMass(MassError::NoMass(idx)),
        GR_E_INCONSISTENT_GROUP => {
            let mut c = [0u64; 2];
            unsafe { gr_last_error_counts(sys.ctx, c.as_mut_ptr()) };
            RMSDError::InconsistentGroup(group.to_owned(), c[0] as usize, c[1] as usize)
        }
        s => RMSDError::InvalidSimBox(simbox_err(s)),
    }
}

impl FrameAnalyze for HipRmsd {
    type Error = RMSDError;
    type AnalysisResult = f32;
    fn analyze(&mut self, system: &System) -> Result<f32, RMSDError> {
        self.stage(system);
        let (mut r, mut st) = (0f32, 0);
        match unsafe { gr_rmsd_batch(self.plan, 0, 1, &mut r, &mut st, std::ptr::null_mut()) } {
            GR_OK => Ok(r),
            s => Err(rmsd_error(&self.target, s, &self.group)),
        }
    }
}

impl FrameConvertAnalyze for HipRmsd {
    type Error = RMSDError;
    type AnalysisResult = f32;
    fn convert_analyze(&mut self, system: &mut System) -> Result<f32, RMSDError> {
        self.stage(system);
        let (mut r, mut st) = (0f32, 0);
        match unsafe { gr_rmsd_fit_batch(self.plan, 0, 1, &mut r, &mut st) } {
            GR_OK => {
                unsafe { gr_frame_download(self.target.ctx, 0, self.scratch.as_mut_ptr() as *mut c_float) };
                for (atom, p) in system.atoms_iter_mut().zip(self.scratch.iter()) {
                    atom.set_position(Vector3D::new(p[0], p[1], p[2]));
                }
                Ok(r)
            }
            s => Err(rmsd_error(&self.target, s, &self.group)),
        }
    }
}

/// One hydrogen bond as `HBond` reports it (hbonds.rs:51-70, whose constructor is private to its module): the same getters.
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct HipHBond { donor: usize, hydrogen: usize, acceptor: usize, distance: f32, angle: f32 }

impl HipHBond {
    pub fn donor(&self) -> usize { self.donor }
    pub fn hydrogen(&self) -> usize { self.hydrogen }
    pub fn acceptor(&self) -> usize { self.acceptor }
    pub fn distance(&self) -> f32 { self.distance }
    pub fn angle(&self) -> f32 { self.angle }
}

/// `HBondAnalysis` (src/system/hbonds.rs:154-373) on the GPU: chains are (acceptors, donors, hydrogens) GSL queries as in
/// `HBondChain::new`, the bonds are the System's own.  `system.xtc_iter(f)?.analyze(HipHBonds::new(..)?)` yields, per frame,
/// the bonds of every requested pair in the reference's order.
pub struct HipHBonds { plan: *mut gr_hbond_plan, sys: HipSystem, pairs: Vec<(usize, usize)>, scratch: Vec<[f32; 3]>, cap: u64 }

impl Drop for HipHBonds { fn drop(&mut self) { unsafe { gr_hbond_plan_destroy(self.plan) } } }

impl HipHBonds {
    pub fn new(system: &System, chains: &[(&str, &str, &str)], pairs: Vec<(usize, usize)>, max_distance: f32, min_angle: f32, device: i32)
        -> Result<Self, HBondError> {
        let sys = HipSystem::new(system, device, 1).ok_or(HBondError::EmptyChain)?;
        let mut names = Vec::new();
        for (k, (a, d, h)) in chains.iter().enumerate() {
            for (r, q) in [a, d, h].iter().enumerate() {
                let group = Group::from_query(q, system).map_err(HBondError::SelectError)?;
                let name = format!("__hbond_{}_{}", k, r);
                sys.group_from_container(&name, group.get_atoms());
                names.push(CString::new(name).unwrap());
            }
        }
        let ptrs: Vec<*const c_char> = names.iter().map(|n| n.as_ptr()).collect();
        let flat: Vec<u32> = pairs.iter().flat_map(|&(a, b)| [a as u32, b as u32]).collect();
        let mut bonds = Vec::new();
        for i in 0..system.get_n_atoms() {
            for j in system.bonded_atoms_iter(i).unwrap() {
                if j.get_index() > i { bonds.push(i as u64); bonds.push(j.get_index() as u64); }
            }
        }
        let mut st = 0;
        let plan = unsafe { gr_hbond_plan_create(sys.ctx, ptrs.as_ptr(), chains.len() as u32, flat.as_ptr(), pairs.len() as u32, bonds.as_ptr(),
                                                 (bonds.len() / 2) as u64, max_distance, min_angle, &mut st) };
        if plan.is_null() { return Err(hbond_error(&sys, st, &pairs, true)); }
        Ok(HipHBonds { plan, sys, pairs, scratch: Vec::new(), cap: 0 })
    }
}

fn hbond_error(sys: &HipSystem, status: c_int, pairs: &[(usize, usize)], plan: bool) -> HBondError {
    let idx = unsafe { gr_last_error_index(sys.ctx) } as usize;
    match status {
        GR_E_EMPTY_CHAIN => HBondError::EmptyChain,
        GR_E_NONEXISTENT_CHAIN => HBondError::NonexistentChain(idx),
        GR_E_DUPLICATE_PAIR => HBondError::PairSpecifiedMultipleTimes(pairs[idx].0, pairs[idx].1),
        GR_E_UNUSED_CHAIN => HBondError::UnusedChain,
        GR_E_INVALID_ARG if plan => HBondError::CellGridError(CellGridError::InvalidCellSize),
        GR_E_NO_POSITION => HBondError::AtomError(AtomError::InvalidPosition(PositionError::NoPosition(idx))),
        GR_E_OUT_OF_RANGE => HBondError::AtomError(AtomError::OutOfRange(idx)),
        s => HBondError::InvalidSimBox(simbox_err(s)),
    }
}

impl FrameAnalyze for HipHBonds {
    type Error = HBondError;
    /// per requested pair, in the order of `pairs`: ((chain1, chain2), bonds) -- the entries of the reference's HBondMap
    type AnalysisResult = Vec<((usize, usize), Vec<HipHBond>)>;
    fn analyze(&mut self, system: &System) -> Result<Self::AnalysisResult, HBondError> {
        self.scratch.clear();
        self.scratch.extend(system.atoms_iter().map(|a| a.get_position().map_or([f32::NAN; 3], |p| [p.x, p.y, p.z])));
        self.sys.upload(0, &self.scratch, system.get_box());
        let np = self.pairs.len();
        let mut offs = vec![0u64; np + 1];
        let (mut total, mut st) = (0u64, 0);
        loop {
            let n = self.cap as usize + 1;
            let (mut d, mut h, mut a) = (vec![0u32; n], vec![0u32; n], vec![0u32; n]);
            let (mut dist, mut ang) = (vec![0f32; n], vec![0f32; n]);
            let r = unsafe { gr_hbond_batch(self.plan, 0, 1, self.cap, d.as_mut_ptr(), h.as_mut_ptr(), a.as_mut_ptr(), dist.as_mut_ptr(), ang.as_mut_ptr(),
                                            offs.as_mut_ptr(), &mut total, &mut st) };
            if r != GR_OK { return Err(hbond_error(&self.sys, r, &self.pairs, false)); }
            if total > self.cap { self.cap = total + total / 4; continue; }
            return Ok(self.pairs.iter().enumerate().map(|(p, &key)| {
                let bonds = (offs[p] as usize..offs[p + 1] as usize)
                    .map(|k| HipHBond { donor: d[k] as usize, hydrogen: h[k] as usize, acceptor: a[k] as usize, distance: dist[k], angle: ang[k] })
                    .collect();
                (key, bonds)
            }).collect());
        }
    }
}

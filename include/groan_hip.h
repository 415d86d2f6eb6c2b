/*
 * groan_hip.h -- C ABI of libgroan_hip.so: the MI355X (gfx950) per-frame geometry engine that
 * replaces groan_rs's CPU hot path (PBC distances, centres of geometry/mass, Kabsch RMSD / RMSD-fit,
 * translate / wrap / centre).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Each entry point names the reference interface it replaces (file:line relative to the groan_rs
 * v0.11.3 root).  INTEGRATION.md shows the Rust `extern "C"` block + safe wrappers that bind these,
 * in the style of the reference's existing xdrfile FFI (src/io/xdrfile.rs:27-120).
 *
 * Model
 *   gr_ctx   device mirror of one `System` (src/system/mod.rs:38-73): n_atoms, masses, named groups
 *            (AtomContainer block lists), and `n_slots` resident frames (positions float[n][3] + box).
 *            Not re-entrant; distinct contexts are independent (one per worker / per GPU), like the
 *            per-thread System clones of traj_iter_map_reduce (src/system/parallel.rs:236).
 *   slot     one frame resident in HBM.  A trajectory reader uploads decoded frames into slots
 *            (gr_frame_upload takes the rvec[n] + box exactly as xdrfile/molly deliver them,
 *            src/io/xdrfile.rs:28-36, src/io/xtc_io/molly_xtc.rs:294-307).
 *   plan     cached reference-side RMSD data = RMSDConverterAnalyzer (src/system/rmsd.rs:170-203).
 *
 * Conventions
 *   box9     gro order v1x v2y v3z v1y v1z v2x v2z v3x v3y (src/structures/simbox.rs:13-26); NULL = no box
 *   Option   a missing position / mass (Rust None) is NaN in x / in the mass (the library stores such an atom with NaN in y and z as well:
 *            gr_frame_download returns NaN, NaN, NaN for it whatever y and z the caller had sent)
 *   matrices rotation matrices are column-major (nalgebra storage)
 *   status   every call returns an int: 0 = OK (xdrfile convention, src/io/xtc_io/xdrfile_xtc.rs:63-83)
 *   Non-orthogonal boxes: the reference rejects them (SimBoxError::NotOrthogonal,
 *   src/structures/simbox.rs:230-236).  By default this library computes with the triclinic extension
 *   described in DESIGN.md; gr_ctx_set_strict_orthogonal(ctx,1) restores the reference's error.
 */
#ifndef GROAN_HIP_H
#define GROAN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gr_ctx gr_ctx;
typedef struct gr_rmsd_plan gr_rmsd_plan;
typedef struct gr_hbond_plan gr_hbond_plan;
typedef struct gr_gridmap gr_gridmap;
typedef struct gr_segments gr_segments;
typedef struct gr_region gr_region;
typedef struct gr_contacts gr_contacts;
typedef struct gr_rmsd_panel gr_rmsd_panel;
typedef struct gr_fluct gr_fluct;
typedef struct gr_covar gr_covar;
typedef struct gr_msd gr_msd;
typedef struct gr_internals gr_internals;
typedef struct gr_vcorr gr_vcorr;
typedef struct gr_xtc gr_xtc;

/* status codes; 1..7 map onto the reference's error enums (src/errors.rs) */
enum {
    GR_OK = 0,
    GR_E_NO_BOX = 1,             /* SimBoxError::DoesNotExist            errors.rs:556-566 */
    GR_E_NOT_ORTHOGONAL = 2,     /* SimBoxError::NotOrthogonal (strict mode only)           */
    GR_E_ZERO_BOX = 3,           /* reference panics: vector3d.rs:402-404,576-578           */
    GR_E_EMPTY_GROUP = 4,        /* GroupError::EmptyGroup / RMSDError::EmptyGroup          */
    GR_E_INCONSISTENT_GROUP = 5, /* RMSDError::InconsistentGroup(name, n_ref, n_cur)        */
    GR_E_NO_POSITION = 6,        /* PositionError::NoPosition(index)     errors.rs:570-574 */
    GR_E_NO_MASS = 7,            /* MassError::NoMass(index)             errors.rs:578-582 */
    GR_E_GROUP_NOT_FOUND = 8,    /* GroupError::NotFound / RMSDError::NonexistentGroup      */
    GR_E_OUT_OF_RANGE = 9,       /* AtomError::OutOfRange(index)         errors.rs:290-305 */
    GR_E_INVALID_ARG = 10,       /* bad slot / NULL pointer / size mismatch (caller bug)    */
    GR_E_GROUP_EXISTS = 11,      /* GroupError::AlreadyExistsWarning                        */
    GR_E_HIP = 12,               /* HIP runtime failure: see gr_last_error                  */
    GR_E_NO_DEVICE = 13,         /* no usable gfx950 device: the library has NO CPU fallback */
    GR_E_UNSUPPORTED_BOX = 14,   /* non-orthogonal box that needs more than 16 +- pairs of lattice vectors in the minimum-image table
                                    (a FLAT cell: one box vector much shorter than the skew of the others); ordinary triclinic,
                                    dodecahedral and octahedral cells need 4-8.  Refused rather than answered approximately. */
    GR_E_IO = 15,                /* ReadTrajError::FileNotFound / read failure              */
    GR_E_FORMAT = 16,            /* ReadTrajError::NotXtc / FrameNotFound (corrupt stream)  */
    GR_E_INVALID_NAME = 17,      /* GroupError::InvalidName (auxiliary.rs:37-51)            */
    GR_E_EMPTY_CHAIN = 18,       /* HBondError::EmptyChain (errors.rs:675-677); index = chain   */
    GR_E_NONEXISTENT_CHAIN = 19, /* HBondError::NonexistentChain(chain); index = chain          */
    GR_E_DUPLICATE_PAIR = 20,    /* HBondError::PairSpecifiedMultipleTimes; index = ordinal of the repeated pair */
    GR_E_UNUSED_CHAIN = 21,      /* HBondError::UnusedChain                                      */
    GR_E_INVALID_BOND = 22,      /* AtomError::InvalidBond(i, j)          errors.rs:295-296; gr_last_error_counts = (i, j) */
    GR_E_INVALID_SPAN = 23,      /* GridMapError::InvalidSpan             gridmap.rs:146-150 */
    GR_E_INVALID_TILE = 24       /* GridMapError::InvalidGridTile         gridmap.rs:152-154 */
};

/* Dimension (src/structures/dimension.rs:13-23) */
enum { GR_DIM_NONE = 0, GR_DIM_X, GR_DIM_Y, GR_DIM_Z, GR_DIM_XY, GR_DIM_XZ, GR_DIM_YZ, GR_DIM_XYZ };

/* centre kinds: group_get_center_naive / group_estimate_center / group_get_center and the _com
 * variants (src/system/analysis.rs:52-320) */
enum { GR_CENTER_NAIVE = 0, GR_CENTER_ESTIMATE = 1, GR_CENTER_PBC = 2 };

/* ---------------------------------------------------------------- library / context */
const char *gr_version(void);
const char *gr_status_string(int status);
int gr_device_count(int *count);

/* System::new / System::clone per worker.  device = HIP ordinal.  n_slots resident frames. */
gr_ctx *gr_ctx_create(int device, uint64_t n_atoms, uint32_t n_slots, int *status);
void gr_ctx_destroy(gr_ctx *ctx);
const char *gr_last_error(const gr_ctx *ctx);
/* detail of the last GR_E_NO_POSITION / GR_E_NO_MASS / GR_E_OUT_OF_RANGE (atom index) and of
 * GR_E_INCONSISTENT_GROUP (n_ref, n_cur): what the reference carries inside its error variants */
uint64_t gr_last_error_index(const gr_ctx *ctx);
void gr_last_error_counts(const gr_ctx *ctx, uint64_t counts[2]);
int gr_ctx_set_strict_orthogonal(gr_ctx *ctx, int on);
uint64_t gr_n_atoms(const gr_ctx *ctx);
uint32_t gr_n_slots(const gr_ctx *ctx);
int gr_sync(gr_ctx *ctx);

/* Atom::set_mass for all atoms (src/structures/atom.rs).  masses[n_atoms], NaN = no mass. */
int gr_set_masses(gr_ctx *ctx, const float *masses, uint64_t n);

/* ---------------------------------------------------------------- AtomContainer (host, bit-exact)
 * Pure functions mirroring src/structures/container.rs; blocks are inclusive [start,end].
 * Each returns the number of blocks written (capacity needed: the number of inputs). */
size_t gr_container_from_indices(const uint64_t *indices, size_t n, uint64_t n_atoms,
                                 uint64_t *out_start, uint64_t *out_end);          /* container.rs:51-104  */
size_t gr_container_from_ranges(const uint64_t *start, const uint64_t *end, size_t n, uint64_t n_atoms,
                                uint64_t *out_start, uint64_t *out_end);           /* container.rs:122-215 */
size_t gr_container_union(const uint64_t *s1, const uint64_t *e1, size_t n1,
                          const uint64_t *s2, const uint64_t *e2, size_t n2,
                          uint64_t *out_start, uint64_t *out_end);                 /* container.rs:268-276 */
size_t gr_container_intersection(const uint64_t *s1, const uint64_t *e1, size_t n1,
                                 const uint64_t *s2, const uint64_t *e2, size_t n2,
                                 uint64_t *out_start, uint64_t *out_end);          /* container.rs:278-291 */
uint64_t gr_container_n_atoms(const uint64_t *s, const uint64_t *e, size_t n);     /* container.rs:161-165 */
size_t gr_container_expand(const uint64_t *s, const uint64_t *e, size_t n, uint64_t *out); /* :381-411 */
int gr_container_isin(const uint64_t *s, const uint64_t *e, size_t n, uint64_t index);     /* :241-258 */
/* May this block list index a system of n_atoms atoms?  GR_OK, or GR_E_OUT_OF_RANGE with *bad_index = the offending index.
 * AtomContainer::from_indices never range-checks its smallest index (container.rs:66): from_indices([n], n) is the block
 * (n, n) and the reference panics on the first access through it.  Every entry point that takes a selection (groups,
 * gr_sel_*) applies this check and creates / computes nothing when it fails -- no kernel bounds-checks a selection. */
int gr_container_validate(const uint64_t *s, const uint64_t *e, size_t n, uint64_t n_atoms, uint64_t *bad_index);

/* ---------------------------------------------------------------- groups (src/system/groups.rs)
 * System::group_create_from_ranges / _from_indices.  "all" exists from creation (System::new).
 * Creating an existing name overwrites it and returns GR_E_GROUP_EXISTS (the reference's warning).
 * A block outside [0, n_atoms) (see gr_container_validate) is GR_E_OUT_OF_RANGE + gr_last_error_index; no group is created. */
int gr_group_create_from_ranges(gr_ctx *ctx, const char *name, const uint64_t *start,
                                const uint64_t *end_inclusive, size_t n_ranges);
int gr_group_create_from_indices(gr_ctx *ctx, const char *name, const uint64_t *indices, size_t n);
int gr_group_remove(gr_ctx *ctx, const char *name);
int gr_group_exists(const gr_ctx *ctx, const char *name);
/* the context's groups, for front ends that match group names (the selection language's `group r'...'`): */
uint64_t gr_group_count(const gr_ctx *ctx);
int gr_group_name(const gr_ctx *ctx, uint64_t i, char *name, size_t capacity);
int gr_group_n_atoms(const gr_ctx *ctx, const char *name, uint64_t *n);            /* group_get_n_atoms */
int gr_group_n_blocks(const gr_ctx *ctx, const char *name, size_t *n_blocks);
int gr_group_blocks(const gr_ctx *ctx, const char *name, uint64_t *out_start, uint64_t *out_end);

/* ---------------------------------------------------------------- frames
 * TrajRead::update_system (src/io/traj_read.rs:160-186; molly_xtc.rs:294-307; xdrfile_xtc.rs:88-104):
 * positions as the xtc readers deliver them (rvec[n_atoms], 12-byte records) + box.  The copy runs on the
 * context's own copy stream, asynchronously when xyz is pinned host memory (gr_host_alloc): kernels on other
 * slots keep running (double buffering); any later call that touches `slot` waits for it, and the copy itself
 * waits for kernels that still read the slot.  Keep xyz valid until gr_frame_upload_wait / gr_sync. */
int gr_frame_upload(gr_ctx *ctx, uint32_t slot, const float *xyz, const float *box9);
/* block until the upload into `slot` has left the host buffer (the staging buffer may then be reused) */
int gr_frame_upload_wait(gr_ctx *ctx, uint32_t slot);
int gr_frame_download(gr_ctx *ctx, uint32_t slot, float *xyz);        /* blocking */
int gr_frame_set_box(gr_ctx *ctx, uint32_t slot, const float *box9); /* System::set_box / reset_box (NULL) */
int gr_frame_get_box(const gr_ctx *ctx, uint32_t slot, float box9[9]); /* GR_E_NO_BOX if none */
int gr_frame_copy(gr_ctx *ctx, uint32_t dst_slot, uint32_t src_slot);
/* pinned host staging buffers for the decode -> H2D double buffer */
void *gr_host_alloc(size_t bytes);
void gr_host_free(void *p);

/* ---------------------------------------------------------------- centres
 * System::group_get_center_naive / group_estimate_center / group_get_center (weighted = 0) and
 * group_get_com_naive / group_estimate_com / group_get_com (weighted = 1): analysis.rs:52-320 over
 * iterators.rs:886-967,1152-1191,1237-1266,1314-1357,1404-1438.
 * Check order as in the reference: group exists -> non-empty -> box -> positions/masses. */
int gr_group_center(gr_ctx *ctx, uint32_t slot, const char *group, int kind, int weighted, float out[3]);
/* GR_CENTER_PBC (get_center / get_com) of a contiguous group of at least `min_atoms` atoms is computed in ONE pass over the
 * frame instead of the reference's two dependent ones (Bai-Breen estimate, then the unwrapped mean): images about the
 * group's first atom + a proof that they are the images the reference would unwrap to.  Frames whose centre lies within the
 * proof's bound of a cell face additionally run the estimate pass (it selects the periodic copy the result lies in), frames
 * where the proof fails (groups wider than half a box) both passes -- one masked launch over the batch either way.
 * min_atoms = 0 switches the one-pass path off; default 4096.  gr_center_fallbacks counts the
 * frames that needed those extra passes since the context was created. */
int gr_ctx_set_center_onepass_min(gr_ctx *ctx, uint32_t min_atoms);
uint64_t gr_center_fallbacks(const gr_ctx *ctx);

/* ---------------------------------------------------------------- distances
 * System::group_distance analysis.rs:348-360; atoms_distance :459-471; group_all_distances :401-427
 * (row-major n1 x n2, signed for 1-D dims).  out_host may be pinned or pageable. */
int gr_group_distance(gr_ctx *ctx, uint32_t slot, const char *group1, const char *group2, int dim, float *out);
int gr_atoms_distance(gr_ctx *ctx, uint32_t slot, uint64_t index1, uint64_t index2, int dim, float *out);
int gr_group_all_distances(gr_ctx *ctx, uint32_t slot, const char *group1, const char *group2, int dim,
                           float *out_host, size_t out_capacity_floats);
/* same, result left in HBM (freed by the context; valid until the next call of this function);
 * *out_dev receives the device pointer, for consumers that keep working on the GPU */
int gr_group_all_distances_device(gr_ctx *ctx, uint32_t slot, const char *group1, const char *group2, int dim,
                                  float **out_dev, uint64_t *n1, uint64_t *n2);
/* the matrices of `n_frames` consecutive slots in one launch and one synchronisation (a trajectory loop of
 * group_all_distances over resident frames): matrix f starts at *out_dev + f * n1 * n2.  The caller bounds the memory
 * through n_frames (4 * n1 * n2 bytes each).  status_out[f] (may be NULL) is the frame's status -- a failed frame's
 * matrix is undefined -- and the return value is the first frame's error, as for the other batch calls. */
int gr_group_all_distances_batch_device(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *group1, const char *group2, int dim,
                                        float **out_dev, uint64_t *n1, uint64_t *n2, int *status_out);
/* group_all_distances + what its callers do with the matrix (analysis.rs:401-427; :1420-1451 take its maximum and minimum), WITHOUT the
 * matrix: the kernels compute the same tiles, bit for bit, and only the reduction reaches memory (a 1e4 x 1e4 matrix is 400 MB per frame).
 *   GR_PD_MIN / GR_PD_MAX     out = float[n_frames][per_row ? n1 : 1]: the smallest / largest entry of every row, or of the matrix
 *                             (1-D dimensions are signed, as in the matrix)
 *   GR_PD_COUNT_BELOW         out = uint64_t[n_frames][per_row ? n1 : 1]: entries < param
 *   GR_PD_HIST                out = uint64_t[n_frames][nbins]: nbins (<= 4096) bins over [0, param); per_row must be 0.  Exactly:
 *                             bin = (uint32_t)(d * s), s = (float)nbins / param in f32; counted iff d >= 0 and d * s < nbins
 *                             (one f32 product per entry: near bin edges this differs from (d * nbins) / param)
 * Errors and statuses as gr_group_all_distances_batch_device; the results equal the same reduction of that call's matrix exactly. */
enum { GR_PD_MIN = 1, GR_PD_MAX = 2, GR_PD_COUNT_BELOW = 3, GR_PD_HIST = 4 };
int gr_group_all_distances_reduce(gr_ctx *ctx, uint32_t slot, const char *group1, const char *group2, int dim, int op, int per_row, float param,
                                  uint32_t nbins, void *out, size_t out_capacity_bytes);
int gr_group_all_distances_reduce_batch(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *group1, const char *group2, int dim, int op,
                                        int per_row, float param, uint32_t nbins, void *out, size_t out_capacity_bytes, int *status_out);
/* copy `bytes` from a device pointer this library handed out (e.g. *out_dev above) into host memory, after the
 * context's stream has drained */
int gr_device_read(gr_ctx *ctx, const void *dev, void *host, size_t bytes);

/* ---------------------------------------------------------------- translate / wrap / centre
 * System::atoms_translate / group_translate (modifying.rs:45-75), atoms_wrap / group_wrap (:201-222),
 * atoms_center / atoms_center_mass (utility.rs:109-185).  group == NULL means all atoms. */
int gr_group_translate(gr_ctx *ctx, uint32_t slot, const char *group, const float v[3]);
int gr_group_wrap(gr_ctx *ctx, uint32_t slot, const char *group);
int gr_atoms_center(gr_ctx *ctx, uint32_t slot, const char *reference_group, int dim, int weighted);

/* ---------------------------------------------------------------- anonymous selections: the iterator-level surface
 * The reference's atom iterators carry an AtomContainer (inclusive index blocks, container.rs:23-31) and a box, no name
 * (System::group_iter / atoms_iter / selection_iter, src/system/iterating.rs:43-140; unions and intersections of containers,
 * iterators.rs:1563-1604).  These entry points take the blocks directly -- (start[], end_inclusive[], n_blocks), exactly the
 * AtomBlock layout -- and compute what the iterator traits compute, with THEIR error behaviour, which differs from the
 * System-level calls in one place: an EMPTY selection is not an error, its centre is (NaN, NaN, NaN)
 * (iterators.rs:1186-1188,1259-1261).  Blocks are validated like groups (gr_container_validate: GR_E_OUT_OF_RANGE).
 *   gr_sel_center          AtomIterable::get_center_naive / get_com_naive (:886-967), AtomIteratorWithBox::estimate_center /
 *                          get_center / estimate_com / get_com (:1152-1438); kind / weighted as gr_group_center
 *   gr_sel_translate/wrap  MutAtomIteratorWithBox::translate / wrap (:1520-1553)
 *   gr_sel_all_distances   the double loop of group_all_distances (analysis.rs:414-424) over two iterators, row-major n1 x n2
 *   gr_sel_filter_geometry AtomIteratorWithBox::filter_geometry / ImmutableAtomIterable::filter_geometry_naive (:994-1004,
 *                          1094-1105): the atoms of the selection that have a position and lie inside every shape, returned as
 *                          the blocks of a new container (*n_out_blocks of them, *n_out_atoms atoms; pass NULL buffers to count) */
int gr_sel_center(gr_ctx *ctx, uint32_t slot, const uint64_t *start, const uint64_t *end_inclusive, size_t n_blocks, int kind, int weighted, float out[3]);
int gr_sel_translate(gr_ctx *ctx, uint32_t slot, const uint64_t *start, const uint64_t *end_inclusive, size_t n_blocks, const float v[3]);
int gr_sel_wrap(gr_ctx *ctx, uint32_t slot, const uint64_t *start, const uint64_t *end_inclusive, size_t n_blocks);
int gr_sel_all_distances(gr_ctx *ctx, uint32_t slot, const uint64_t *start1, const uint64_t *end1, size_t n_blocks1,
                         const uint64_t *start2, const uint64_t *end2, size_t n_blocks2, int dim, float *out_host, size_t out_capacity_floats);
struct gr_shape;
int gr_sel_filter_geometry(gr_ctx *ctx, uint32_t slot, const uint64_t *start, const uint64_t *end_inclusive, size_t n_blocks,
                           const struct gr_shape *shapes, size_t n_shapes, int naive,
                           uint64_t *out_start, uint64_t *out_end, size_t capacity_blocks, size_t *n_out_blocks, uint64_t *n_out_atoms);

/* ---------------------------------------------------------------- RMSD / RMSD-fit
 * gr_calc_rmsd / gr_calc_rmsd_and_fit = System::calc_rmsd / calc_rmsd_and_fit (rmsd.rs:75-166):
 * reference and current frame are two (context, slot) pairs on the same device (they may be the same
 * context); the group must exist in both; weights are the REFERENCE's masses (rmsd.rs:154-155).
 * R (optional, may be NULL) = optimal rotation, column-major. */
int gr_calc_rmsd(gr_ctx *ctx, uint32_t slot, gr_ctx *reference, uint32_t ref_slot, const char *group,
                 float *rmsd, float *R_colmajor9);
int gr_calc_rmsd_and_fit(gr_ctx *ctx, uint32_t slot, gr_ctx *reference, uint32_t ref_slot,
                         const char *group, float *rmsd);

/* RMSDConverterAnalyzer::new (rmsd.rs:186-203): extract + cache the reference side once. */
gr_rmsd_plan *gr_rmsd_plan_create(gr_ctx *reference, uint32_t ref_slot, gr_ctx *target,
                                  const char *group, int *status);
void gr_rmsd_plan_destroy(gr_rmsd_plan *plan);
/* FrameAnalyze::analyze (rmsd.rs:228-236) on `n_frames` consecutive slots in one batch.
 * rmsd_out[n_frames]; status_out[n_frames] per-frame status (may be NULL); R_out optional [n][9].
 * Returns the first non-OK per-frame status (error detail = that frame), else GR_OK. */
int gr_rmsd_batch(gr_rmsd_plan *plan, uint32_t first_slot, uint32_t n_frames,
                  float *rmsd_out, int *status_out, float *R_out);
/* FrameConvertAnalyze::convert_analyze (rmsd.rs:238-251): RMSD + in-place fit of ALL atoms of each
 * frame; a frame whose analysis fails is left unmodified (rmsd.rs:91). */
int gr_rmsd_fit_batch(gr_rmsd_plan *plan, uint32_t first_slot, uint32_t n_frames,
                      float *rmsd_out, int *status_out);
/* The same in two halves, for pipelines that keep the GPU busy while the host decodes / uploads the next frames:
 * begin issues every launch for `n_frames` (<= 1024) consecutive slots and returns without waiting; end waits and
 * delivers the results.  One batch in flight per CONTEXT; between the two calls the context accepts gr_frame_upload /
 * gr_frame_upload_wait / gr_xtc_read_frames_device / gr_trr_read_frames_device into slots OUTSIDE the batch and gr_host_*
 * only (uploads run on the copy stream beside the kernels) -- every other call, and an upload into one of the batch's own
 * slots (gr_rmsd_batch_end may still need those frames: it redoes the ones whose image proof failed), returns
 * GR_E_INVALID_ARG and changes nothing. */
int gr_rmsd_batch_begin(gr_rmsd_plan *plan, uint32_t first_slot, uint32_t n_frames, int fit);
int gr_rmsd_batch_end(gr_rmsd_plan *plan, float *rmsd_out, int *status_out, float *R_out);
/* number of frames of the last batch that left the single-pass path for the multi-pass exact path */
uint32_t gr_rmsd_plan_last_fallbacks(const gr_rmsd_plan *plan);
/* force the multi-pass exact path (parity testing of both paths) */
int gr_rmsd_plan_force_exact(gr_rmsd_plan *plan, int on);
/* Launch geometry and path selection of the batched RMSD calls.  Nothing in the library reads the environment for these:
 * results of a call depend on its arguments and on what the caller set here, never on the caller's environment, nor on earlier calls
 * on the same context (`tests/test_gpu_history.py`).
 *   GR_TUNE_SUB_BATCH  frames per sums -> fit launch group (1 .. 1024, default 256)
 *   GR_TUNE_CHUNKS     workgroups per frame of the reduction kernels (0 = automatic)
 *   GR_TUNE_FIT_WGS    workgroups per frame of the fit kernel (0 = automatic: one 256-atom tile per wave)
 *   GR_TUNE_FUSE       1 (default): the sums kernel's last workgroup per frame closes the frame; 0: separate finalize launch
 *   GR_TUNE_TWO_PASS   1 (default): RMSD-fit = sums pass + fit pass that evaluates the rmsd; 0: closed-form single-pass rmsd
 *   GR_TUNE_RESIDENT   RMSD-fit as ONE pass over HBM, the frame waiting on chip for its rotation (gr_resident.h: one launch per
 *                      segment whose workgroups wait for one another; needs n_atoms <= ~1.04e6 on MI355X).  1 (default): when the
 *                      frames in flight (GR_TUNE_RESIDENT_STREAMS) fill at least 10/16 of the chip, the selection is at least 45 %
 *                      of the system and every stream gets 16 frames of the call or more; 0: never; 2: whenever it
 *                      fits.  One such launch runs per device and process at a time (a context that finds the device taken uses
 *                      the two-pass path); a launch whose workgroups do not all get onto the chip (a device shared with another
 *                      process) leaves without touching a frame and the segment runs on the two-pass path.  Same results as the two-pass path up to the order of the partial sums.
 *                      A launch in which a wait runs out of patience (a workgroup made no progress for seconds) is aborted from inside:
 *                      frames it had completed keep their results, frames nobody had touched are redone on the two-pass path, and a
 *                      frame that was caught half fitted -- possible only in the instant of the abort -- is reported as GR_E_HIP
 *                      in status_out with its index in gr_last_error_index (gr_ctx_stat counts aborts and redone frames).
 *   GR_TUNE_RESIDENT_STREAMS frames that fill half of the chip or less run as several frame STREAMS side by side in one resident
 *                      launch (stream s of S owns frames s, s + S, ... of the segment and its own share of the CUs).  0 (default):
 *                      as many as fit, up to 32, when GR_TUNE_RESIDENT is 1 (each stream needs 16 frames of the segment), one when
 *                      it is 2; 1 .. 32: at most so many.  Results do not depend on the number of streams.
 *   GR_TUNE_RESIDENT_FILL    sixteenths of the chip (1 .. 16, default 1; 10 until round 5) the streams of a launch must fill together
 *                      for GR_TUNE_RESIDENT = 1 to choose the pass
 *   GR_TUNE_RESIDENT_WG_GROUPS  4-atom groups per streaming workgroup of the resident pass: 0 (default) = 1024, two per lane; 64 ..
 *                      1024 in steps of 64 cuts a frame into more, smaller workgroups.  An experiment's knob: a turn of the pass is
 *                      bound by instruction issue and latency, not by the work per CU -- 768 groups instead of 1024 gave 5 % at
 *                      600 000 atoms, where frame streams give 40 % (DESIGN.md "Frame streams").  Same results to rounding.
 *   GR_TUNE_PAIRDIST_SYMMETRIC  1 (default): the all-pairs matrix of a group with ITSELF computes the tiles on and above the
 *                      diagonal and writes each of them twice (the mirror image transposed on chip); 0: every element on its own.
 *                      Same bits either way.
 *   GR_TUNE_RESIDENT_GROUPS  retired (round 3 removed the one-group shape of the resident pass): only the value 2 is accepted
 *   GR_TUNE_RMSD_FAST  1 (default): the RMSD WITHOUT fit (gr_rmsd_batch, gr_calc_rmsd) of a contiguous mass-weighted selection of at
 *                      least GR_TUNE_RMSD_FAST_MIN atoms runs as the fit path's sums pass with the closed-form RMSD's sums kept as short
 *                      f32 chains widened to fp64; a frame whose rmsd is too close to the rounding of those sums (a rigid copy of the
 *                      reference) is redone by the exact-product pass, counted in GR_STAT_RMSD_EXACT_REDOS.  0: always the exact pass
 *   GR_TUNE_RMSD_FAST_MIN  smallest selection (atoms, default 16384) that takes it
 *   GR_TUNE_RESIDENT_METRO_NS  the resident pass's METRONOME (gr_resident.h): the period, in nanoseconds per turn, at which the launch's
 *                      row requests sweep each frame in address order.  1 (default) = off, the waves run free; 0 = chosen and kept up to date
 *                      by the library from what its own launches report (GR_STAT_RES_METRO_PERIOD_NS / _LAST_TURN_NS / _LATE_PERMILLE: the
 *                      default for most of round 5 -- it bought 3 % while the pass was paced by memory, nothing since, and could settle on a
 *                      slow period after a cold first launch); 100 .. 1 000 000 = this period.  Results do not depend on it.
 *   GR_TUNE_RESIDENT_FIT_LAST  order of a turn of the resident pass: 1 = the fit of frame i - 6, then the sums of frame i (rounds 2-4);
 *                      2 = the sums first (the frame's record is needed later and published earlier: one more turn for the finalizers);
 *                      0 (default) = sums first when the streaming workgroups fill 9/10 of the chip.  Same results either way.
 *   GR_TUNE_STREAM_WGS_PER_CU  workgroups per CU of the grid-launched read-modify-write streams (translate / wrap / centre, the two-pass fit):
 *                      1 .. 8, 0 (default) = the library's choice.  A copy is fastest with 20-32 KiB of loads in flight per CU.
 *   GR_TUNE_CENTER_RESIDENT  1 (default): gr_atoms_center_batch about a contiguous reference group of at least 15 % of the system (3 % in non-orthogonal cells) runs as ONE pass
 *                      over HBM where the resident pass can take it (gr_resident.h MODE 1: every frame read once, written once -- 24 instead of
 *                      36 bytes per atom); 0: always the two passes (centre estimate, then translate + wrap).  Same bits either way.
 *   GR_TUNE_TRANSLATE_ROWS  1 (default): translate / wrap / centring of a contiguous selection in an ORTHORHOMBIC cell runs one 16-byte load and
 *                      store per lane, a 256-atom tile per workgroup (every coordinate wraps on its own there); 0: the three-rows-per-lane walk
 *                      that non-orthogonal cells and scattered selections take.  Same bits either way. */
enum { GR_TUNE_SUB_BATCH = 1, GR_TUNE_CHUNKS = 2, GR_TUNE_FIT_WGS = 3, GR_TUNE_FUSE = 4, GR_TUNE_TWO_PASS = 5, GR_TUNE_RESIDENT = 6, GR_TUNE_RESIDENT_GROUPS = 7,
       GR_TUNE_RESIDENT_STREAMS = 8, GR_TUNE_RESIDENT_FILL = 9, GR_TUNE_PAIRDIST_SYMMETRIC = 10, GR_TUNE_RESIDENT_WG_GROUPS = 11,
       GR_TUNE_RMSD_FAST = 12, GR_TUNE_RMSD_FAST_MIN = 13, GR_TUNE_RESIDENT_METRO_NS = 18, GR_TUNE_RESIDENT_FIT_LAST = 19, GR_TUNE_STREAM_WGS_PER_CU = 20, GR_TUNE_CENTER_RESIDENT = 21, GR_TUNE_TRANSLATE_ROWS = 22,
       GR_TUNE_MASKED_SELECTIONS = 15 /* 1 (default): a scattered selection that covers at least an eighth of the atoms between its first and its last one (>= 4096
                                         atoms) also gets a bit mask, and RMSD / RMSD-fit / get_com read its span coalesced instead of gathering it atom by atom;
                                         0: groups created afterwards keep to their index lists.  Same results to rounding. */,
       GR_TUNE_XTC_DEVICE_ENCODE = 16 /* 1 (default): gr_xtc_write_slots compresses outputs of >= 200 000 atoms (frames x atoms) on the device -- the same bytes as the
                                         host encoder, only the compressed stream crosses PCIe and no host thread encodes (GR_STAT_XTC_DEVICE_FRAMES counts the
                                         frames); 0: host threads encode (host_threads of the call).  2.0 / 2.5 k frames/s of 5e5 atoms (water-like / one dense chain)
                                         against 1.4-1.6 / 2.1-2.8 k for 16 host encoders: the rate the file takes on the test box (tools/xtc_write_bench.py) */,
       GR_TUNE_RMSD_FAST_SIGMAS = 14 /* multiples (default 6) of the pass's own rounding estimate a frame's rmsd must stand clear of to be kept; 0 keeps every frame: calibration runs only (tools/rmsd_calibrate.py) */,
       GR_TUNE_SMALL_CALLS = 17 /* largest selection (atoms; default 4096, 0 = never) for which ONE-frame calls -- gr_group_center, gr_sel_center, gr_rmsd /
                                    gr_rmsd_batch of one frame -- run as one single-wave dispatch whose result the host reads out of coherent host
                                    memory instead of a chain of launches, two small copies and a stream synchronisation (gr_small.h: 36 -> ~10 us for the
                                    centre of mass, 55 -> ~14 us for the RMSD of a 363-atom selection); same closing arithmetic, sums in another order */,
       GR_TUNE_TEST_RESIDENT_NO_START = 100 /* tests: the next resident launch behaves as if its workgroups never got onto the chip */,
       GR_TUNE_TEST_RESIDENT_ABORT_AT = 101 /* tests: the next resident launch is aborted from inside when it reaches this frame of its segment (< 0: never) */ };
int gr_ctx_set_tuning(gr_ctx *ctx, int key, int64_t value);
/* Read-only facts about a context and its device, and counters of what the batched RMSD path did since the context was created
 * (unknown key: GR_E_INVALID_ARG).
 *   GR_STAT_N_CUS                  compute units of the device
 *   GR_STAT_RES_MAX_WGS            workgroups of the resident pass the device holds at once (0: the pass cannot run / was switched off)
 *   GR_STAT_RES_LAUNCHES           resident launches that ran to the end
 *   GR_STAT_RES_HANDSHAKE_MISSES   resident launches that closed themselves at the start handshake (the segment then took the two-pass path)
 *   GR_STAT_RES_ABORTS             resident launches in which a wait ran out of patience (see gr_rmsd_fit_batch)
 *   GR_STAT_RES_REDONE_FRAMES      frames of such launches that were still untouched and were redone on the two-pass path
 *   GR_STAT_RES_LAST_STREAMS       frame streams of the context's last resident launch (GR_TUNE_RESIDENT_STREAMS)
 *   GR_STAT_RES_METRO_PERIOD_NS    the metronome period the last resident launch ran with (0: it ran free)
 *   GR_STAT_RES_LAST_TURN_NS       what a turn of that launch took on the device clock (first slot to the last wave's exit, per turn)
 *   GR_STAT_RES_LATE_PERMILLE      thousandths of its metronome slots that waves reached more than a quarter period late
 *   GR_STAT_RES_SCLK_MHZ           shader clock that launch ran at (shader-clock ticks over device-clock ticks of its first workgroup's walk)
 *   GR_STAT_CENTER_RES_LAUNCHES    resident atoms_center launches that started (GR_TUNE_CENTER_RESIDENT)
 *   GR_STAT_CENTER_RES_REDONE      frames those launches handed back to the two passes (an atom without position or mass, sums that are not finite, an abort)
 *   GR_STAT_RES_LEAN_SEGMENTS      resident launches (RMSD-fit and atoms_center) that started and whose frames had all passed the host's checks: no state was zeroed or uploaded for them
 *   GR_STAT_RES_SYNC_FALLBACKS     resident launches whose results the host gave up polling for (20 ms) and synchronised the stream instead */
enum { GR_STAT_N_CUS = 1, GR_STAT_RES_MAX_WGS = 2, GR_STAT_RES_LAUNCHES = 3, GR_STAT_RES_HANDSHAKE_MISSES = 4, GR_STAT_RES_ABORTS = 5, GR_STAT_RES_REDONE_FRAMES = 6, GR_STAT_RES_LAST_STREAMS = 7,
       GR_STAT_RMSD_FAST_FRAMES = 8 /* frames of RMSD-without-fit calls closed by the f32-chain pass (GR_TUNE_RMSD_FAST) */,
       GR_STAT_RMSD_EXACT_REDOS = 9 /* ... and frames that pass handed back to the exact-product pass */,
       GR_STAT_XTC_DEVICE_FRAMES = 10 /* frames gr_xtc_write_slots compressed on the device (GR_TUNE_XTC_DEVICE_ENCODE) */,
       GR_STAT_SMALL_CALLS = 11 /* one-frame calls answered by a single-wave dispatch (GR_TUNE_SMALL_CALLS) */,
       GR_STAT_SMALL_SYNC_FALLBACKS = 12 /* ... of which the host gave up polling for the result (20 ms) and synchronised the stream instead */,
       GR_STAT_RES_METRO_PERIOD_NS = 13, GR_STAT_RES_LAST_TURN_NS = 14, GR_STAT_RES_LATE_PERMILLE = 15, GR_STAT_RES_SCLK_MHZ = 16,
       GR_STAT_CENTER_RES_LAUNCHES = 17, GR_STAT_CENTER_RES_REDONE = 18, GR_STAT_RES_LEAN_SEGMENTS = 19, GR_STAT_RES_SYNC_FALLBACKS = 20 };
int gr_ctx_stat(const gr_ctx *ctx, int key, uint64_t *value);

/* ---------------------------------------------------------------- text front end: gro structures, ndx index groups (host side)
 * read_gro (src/io/gro_io/structure.rs:120-231, gro_io/mod.rs:21-72) and Groups::from_ndx (src/io/ndx_io.rs:104-230): what is
 * needed to run the path from files -- positions, box, atom / residue names and numbers, index groups.  A failed parse returns
 * GR_E_IO (file not found) or GR_E_FORMAT with *detail_code = the reference's error variant and `detail` = its payload
 * (the offending line / number), exactly as the reference's tests pin them. */
enum { GR_PARSE_OK = 0, GR_PARSE_FILE_NOT_FOUND, GR_PARSE_LINE_NOT_FOUND, GR_PARSE_LINE, GR_PARSE_ATOM_LINE, GR_PARSE_BOX_LINE,
       GR_PARSE_UNSUPPORTED_BOX, GR_PARSE_INVALID_FLOAT, GR_PARSE_GROUP_NAME, GR_PARSE_INVALID_ATOM_INDEX };
typedef struct gr_structure gr_structure;
int gr_gro_read(const char *path, gr_structure **out, int *detail_code, char *detail, size_t detail_cap);
void gr_structure_free(gr_structure *s);
uint64_t gr_structure_n_atoms(const gr_structure *s);
const char *gr_structure_title(const gr_structure *s);
int gr_structure_box(const gr_structure *s, float box9[9]);          /* GR_E_NO_BOX when the box line is all zeros */
int gr_structure_positions(const gr_structure *s, float *xyz);       /* [n][3] */
int gr_structure_velocities(const gr_structure *s, float *vel);      /* [n][3], NaN rows for atoms without velocity */
int gr_structure_atom(const gr_structure *s, uint64_t i, uint64_t *resid, uint64_t *atomid, char resname[8], char atomname[8]);
typedef struct gr_ndx gr_ndx;
int gr_ndx_read(const char *path, uint64_t n_atoms, gr_ndx **out, int *detail_code, char *detail, size_t detail_cap);
void gr_ndx_free(gr_ndx *x);
size_t gr_ndx_n_groups(const gr_ndx *x);                             /* groups in file order (a repeated name appears again) */
const char *gr_ndx_group_name(const gr_ndx *x, size_t g);
size_t gr_ndx_group_size(const gr_ndx *x, size_t g);                 /* indices as written: 0-based, file order, duplicates kept */
int gr_ndx_group_indices(const gr_ndx *x, size_t g, uint64_t *out);
/* System::read_ndx: create the groups on a context (Group::from_indices); a group with an invalid name is skipped and counted,
 * a repeated / already existing name is overwritten and counted (the reference's two warnings) */
int gr_ndx_install(const gr_ndx *x, gr_ctx *ctx, size_t *n_invalid_names, size_t *n_duplicate_names);

/* ---------------------------------------------------------------- cut-off pair search (cell grid on the device)
 * What a CellGrid walk with a distance filter produces (CellGrid::new + neighbors_iter, src/structures/cellgrid.rs:301-409,
 * as src/system/hbonds.rs:248-265 uses them): all pairs (i in group1, j in group2, i != j) with distance(x_j, x_i) <= cutoff,
 * ordered by i then j (the reference leaves the order undefined).  The grid (cells of at least `cutoff`, periodic 27-cell
 * neighbourhood) is built on the device; it replaces the S1 x S2 distance matrix when only near pairs are wanted.
 * Needs a box (GR_E_NO_BOX); non-orthogonal boxes -- which the reference's CellGrid rejects (cellgrid.rs:411-430), and so does
 * this call in strict-orthogonal mode (GR_E_NOT_ORTHOGONAL) -- are binned in fractional coordinates with the triclinic
 * minimum-image distance as the filter; cutoff > 0 (GR_E_INVALID_ARG, the reference's
 * CellGridError::InvalidCellSize), positions for every atom of both groups (GR_E_NO_POSITION + index: group2 is checked
 * first, as the grid is built before it is queried).  *n_pairs receives the number of pairs found; at most max_pairs are
 * written -- when *n_pairs > max_pairs call again with larger buffers (the buffers may be NULL to just count). */
int gr_group_pairs_within(gr_ctx *ctx, uint32_t slot, const char *group1, const char *group2, float cutoff, uint64_t max_pairs,
                          uint32_t *i_out, uint32_t *j_out, float *dist_out, uint64_t *n_pairs);

/* ---------------------------------------------------------------- hydrogen bonds over a batch of resident frames
 * HBondAnalysis / HBondTrajRead::hbonds_analyze (src/system/hbonds.rs:154-373).  A plan is built once: `groups` holds
 * n_chains x 3 group names of the context (acceptors, donors, hydrogens of each chain), `pairs` n_pairs x 2 chain indices,
 * `bonds` n_bonds x 2 atom indices (either order; the plan does not read the context's bonds (gr_add_bond): the caller passes them).  A donor
 * is kept when it is bonded to an atom of its chain's hydrogen group; its hydrogens are taken in index order.  Plan errors, in
 * the reference's order: GR_E_OUT_OF_RANGE (a bonded atom outside the system, index = the atom), per chain GR_E_GROUP_NOT_FOUND
 * and GR_E_EMPTY_CHAIN (index = the chain), then the pairs: GR_E_NONEXISTENT_CHAIN (index = the chain), GR_E_DUPLICATE_PAIR
 * ((0,1) after (1,0) counts; index = the ordinal of the repeated pair), GR_E_UNUSED_CHAIN; then max_distance <= 0
 * (GR_E_INVALID_ARG: the reference's CellGridError::InvalidCellSize).  The plan keeps a pointer to the context: destroy it first.
 *
 * gr_hbond_batch analyses the n_frames (<= 1024) slots from first_slot.  The bonds of frame f and pair p are the entries
 * offsets[f * n_pairs + p] .. offsets[f * n_pairs + p + 1] (offsets holds n_frames * n_pairs + 1 values and is always written),
 * ordered as the reference's segments ((a, a): donors of a to acceptors of a; (a, b): donors of b to acceptors of a, then donors
 * of a to acceptors of b), then by donor (group order), acceptor index and hydrogen index.  distance = acceptor.distance(donor)
 * in nm; angle = the donor-hydrogen...acceptor angle in degrees (a NaN angle is 180 when the hydrogen is closer to the acceptor
 * than the donor, else 0).  *n_total receives the batch's number of bonds; when it exceeds max_bonds, or any output pointer is
 * NULL, no bond is written (count only).  Every frame is judged on its own: status_out[f] (may be NULL) receives GR_OK,
 * GR_E_NO_BOX / GR_E_ZERO_BOX / GR_E_NOT_ORTHOGONAL (strict mode) / GR_E_UNSUPPORTED_BOX, or GR_E_NO_POSITION -- the first
 * acceptor (chains in order, then group order), else the first donor without position, else, for the first donor with an
 * acceptor within max_distance, its first hydrogen without position; a failed frame has empty segments.  The return value is
 * the first failed frame's status (message and gr_last_error_index as for the single calls).  Non-orthogonal boxes are
 * supported outside strict mode, as in gr_group_pairs_within. */
gr_hbond_plan *gr_hbond_plan_create(gr_ctx *ctx, const char *const *groups, uint32_t n_chains, const uint32_t *pairs, uint32_t n_pairs,
                                    const uint64_t *bonds, uint64_t n_bonds, float max_distance, float min_angle, int *status);
void gr_hbond_plan_destroy(gr_hbond_plan *plan);
int gr_hbond_batch(gr_hbond_plan *plan, uint32_t first_slot, uint32_t n_frames, uint64_t max_bonds, uint32_t *donor, uint32_t *hydrogen,
                   uint32_t *acceptor, float *distance, float *angle, uint64_t *offsets, uint64_t *n_total, int *status_out);

/* ---------------------------------------------------------------- bond topology, whole molecules / groups
 * The context's bonds (Atom::get_bonded, a sorted container) and what the reference derives from them.  Every bond change resets
 * the molecules, which are computed again on first use (reset_mol_references, mod.rs:349-377), and the per-atom map the device
 * reads (uploaded once per topology, not per frame).
 *   gr_add_bond            System::add_bond (modifying.rs:235-252): i == j is GR_E_INVALID_BOND (counts = (i, j)), checked before
 *                          GR_E_OUT_OF_RANGE of i, then of j (gr_last_error_index = the index); a bond that exists is kept once
 *   gr_add_bonds           pairs[n_pairs][2] in order; on the first bad pair nothing of the call is applied
 *   gr_clear_bonds         System::clear_bonds (modifying.rs:480-487); gr_has_bonds: System::has_bonds (mod.rs:437), 1 or 0
 *   gr_mol_references      what create_mol_references yields (modifying.rs:258-283): the lowest atom of every polyatomic molecule,
 *                          ascending; *n = their number, at most `cap` are written (out may be NULL to count)
 *   gr_molecule_atoms      molecule_iter (iterating.rs:238-245,399-432): breadth-first from `index`, neighbours ascending; an atom
 *                          without bonds yields itself; GR_E_OUT_OF_RANGE for index >= n_atoms
 *   gr_make_molecules_whole  System::make_molecules_whole (modifying.rs:338-392): every reference atom wrapped into the box, every
 *                          other atom of its molecule placed at ref_w + vector_to(ref_w, p); atoms outside polyatomic molecules are
 *                          never touched.  Errors: the box (GR_E_NO_BOX / GR_E_ZERO_BOX / GR_E_NOT_ORTHOGONAL in strict mode /
 *                          GR_E_UNSUPPORTED_BOX, even without bonds), then GR_E_NO_POSITION with the atom the reference stops on:
 *                          of the molecules holding an atom without position the one with the lowest reference, in it the reference
 *                          when it has no position, else the first such atom in breadth-first order.
 *   gr_make_group_whole    System::make_group_whole (modifying.rs:447-475): c = group_estimate_center, then every atom of the group
 *                          becomes c + vector_to(c, p); the errors are exactly those of gr_group_center(.., GR_CENTER_ESTIMATE, 0, ..)
 * A frame that fails is left bit for bit untouched -- unlike the reference, which has already moved the molecules before the
 * failing one.  The _batch forms take n_frames consecutive slots and follow the batch rules below (status_out may be NULL; the
 * return value is the first failed frame's status, message and gr_last_error_index).  Non-orthogonal cells outside strict mode
 * use the library's triclinic wrap and vector_to, as every other call. */
int gr_add_bond(gr_ctx *ctx, uint64_t i, uint64_t j);                                            /* modifying.rs:235-252 */
int gr_add_bonds(gr_ctx *ctx, const uint64_t *pairs, uint64_t n_pairs);
int gr_clear_bonds(gr_ctx *ctx);                                                                 /* modifying.rs:480-487 */
int gr_has_bonds(const gr_ctx *ctx);                                                             /* mod.rs:437 */
int gr_mol_references(gr_ctx *ctx, uint64_t *out, uint64_t cap, uint64_t *n);                    /* modifying.rs:258-283 */
int gr_molecule_atoms(gr_ctx *ctx, uint64_t index, uint64_t *out, uint64_t cap, uint64_t *n);    /* iterating.rs:238-245,399-432 */
int gr_make_molecules_whole(gr_ctx *ctx, uint32_t slot);                                         /* modifying.rs:338-392 */
int gr_make_molecules_whole_batch(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, int *status_out);
int gr_make_group_whole(gr_ctx *ctx, uint32_t slot, const char *group);                          /* modifying.rs:447-475 */
int gr_make_group_whole_batch(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *group, int *status_out);

/* ---------------------------------------------------------------- GridMap: xy tile maps accumulated over resident frames
 * GridMap (src/structures/gridmap.rs): nx x ny tiles over (span_x, span_y), tile (ix, iy) centred on (span_x[0] + ix * tile_dim[0],
 * span_y[0] + iy * tile_dim[1]) -- the map really covers span0 - tile / 2 .. span1 + tile / 2.  The reference is a container its
 * user's trajectory loop fills atom by atom; here the loop runs on the device over a batch of resident frames, and the map holds,
 * per tile, a COUNT and the SUM of one coordinate of the atoms that fell into it -- what density, height and thickness maps are
 * made of.  All arithmetic is the reference's, in f32:
 *   gr_gridmap_len          get_len (gridmap.rs:146-157): span[1] - span[0] < 0 is GR_E_INVALID_SPAN; tile > that difference or
 *                           tile == 0 is GR_E_INVALID_TILE; else *n = round(diff / tile) + 1.  NaN in the span or the tile and a
 *                           negative tile are GR_E_INVALID_ARG, and so is a map of more than 2^26 tiles (create / from_box).
 *   gr_gridmap_coord2index  x2index / y2index (:715-724): round((coord - span0) / tile), half away from zero, converted like Rust's
 *                           `as isize` (NaN -> 0, +-inf and huge values -> INT64_MAX / INT64_MIN).  A point is INSIDE the map when
 *                           0 <= ix < nx and 0 <= iy < ny.
 *   gr_gridmap_index2coord  index2x / index2y (:729-738): (float)index * tile + span0, two roundings (never an fma), the same bits
 *                           on the host and on the device.
 *   gr_gridmap_create       GridMap::new (:122-140); gr_gridmap_from_box: GridMap::from_box (:164-173), spans (0, box.x), (0, box.y)
 *                           of the slot's box: GR_E_NO_BOX without one, GR_E_NOT_ORTHOGONAL for a non-orthogonal box in EVERY mode
 *                           (the tile plane of a skewed cell is not defined).  The map keeps a pointer to the context: destroy it first.
 *   gr_gridmap_accumulate_batch  for every frame f of the n_frames slots from first_slot that passes its checks, and every atom of
 *                           `group`: (x, y, z) = its position -- with GR_GM_WRAP the position gr_group_wrap would give it (the frame
 *                           is not modified; needs the frame's box: GR_E_NO_BOX / GR_E_ZERO_BOX / GR_E_NOT_ORTHOGONAL in strict mode
 *                           / GR_E_UNSUPPORTED_BOX; without GR_GM_WRAP no box is needed, as in the reference); ix, iy as above; an
 *                           atom that is not inside adds 1 to n_outside[f] and nothing else; otherwise count[ix, iy] += 1 and, for
 *                           value = GR_GM_X / _Y / _Z, sum_q[ix, iy] += (int64) rint((double) v * 2^20) with v = coordinate -
 *                           offset[f] in f32 (offset NULL: 0).  An atom whose v is not finite or has |v| >= 2^31 counts as outside.
 *                           The sums are 64-bit INTEGERS in units of 2^-20 nm (far below xtc precision): integer adds commute, so a
 *                           map is the same bit for bit whatever the order of the adds -- on every path, across calls and across
 *                           runs.  Capacity of a tile: 2^32 contributions of 2048 nm.
 *                           Errors: GR_E_GROUP_NOT_FOUND, GR_E_EMPTY_GROUP; per frame (batch rules below: status_out[f], the return
 *                           value is the first failed frame's status, message and gr_last_error_index) the box statuses above and
 *                           GR_E_NO_POSITION with index = the first atom of the group, in group order, without position.  A failed
 *                           frame contributes NOTHING and has n_outside[f] = 0 (the reference's loop would have binned the atoms in
 *                           front of the failing one).  Any number of frames, as gr_group_center_batch.
 *                           A map whose privatised copy fits 64 KiB of LDS (12 bytes per tile, 4 when only counting) is accumulated
 *                           per workgroup in LDS over many frames and flushed once; larger maps, and GR_GM_FORCE_GLOBAL, add to
 *                           global memory directly (gr_gridmap_stat counts the launches of either kind).  Same bits either way.
 *   gr_gridmap_set_launch   caps the grids of the two launches of a segment (tests aim at the kernels' loops with it): the ranges the
 *                           group is cut into, min(range_groups, units) -- units: 4-atom groups of the group's span, or its list
 *                           entries; never fewer than ceil(units / 2^18) --, the workgroups that share the frames of a range,
 *                           min(frame_groups, frames of the segment), and the workgroups of the position check, min(check_groups, its
 *                           default).  0 restores the default of that value.  GR_GM_STAT_LAST_RANGE_GROUPS / _FRAME_GROUPS /
 *                           _CHECK_GROUPS: the grid of the last segment that was launched (0: none yet).
 *   gr_gridmap_read         count, sum_q, mean = (float)((double) sum_q * 2^-20 / (double) count) (NaN where count == 0), each
 *                           [nx * ny], row-major with x the outer index; any may be NULL.  gr_gridmap_clear zeroes the map. */
enum { GR_GM_COUNT = 0, GR_GM_X = 1, GR_GM_Y = 2, GR_GM_Z = 3 };          /* what is summed per tile besides the count */
enum { GR_GM_WRAP = 1, GR_GM_FORCE_GLOBAL = 2 };                           /* flags */
enum { GR_GM_STAT_LDS_LAUNCHES = 1, GR_GM_STAT_GLOBAL_LAUNCHES = 2, GR_GM_STAT_LDS_BUDGET = 3 /* bytes */,
       GR_GM_STAT_LAST_RANGE_GROUPS = 4, GR_GM_STAT_LAST_FRAME_GROUPS = 5, GR_GM_STAT_LAST_CHECK_GROUPS = 6 };
int gr_gridmap_len(const float span[2], float tile, uint64_t *n);
int64_t gr_gridmap_coord2index(float span0, float tile, float coord);
float gr_gridmap_index2coord(float span0, float tile, uint64_t index);
gr_gridmap *gr_gridmap_create(gr_ctx *ctx, const float span_x[2], const float span_y[2], const float tile_dim[2], int *status);
gr_gridmap *gr_gridmap_from_box(gr_ctx *ctx, uint32_t slot, const float tile_dim[2], int *status);
void gr_gridmap_destroy(gr_gridmap *map);
int gr_gridmap_dims(const gr_gridmap *map, uint64_t *nx, uint64_t *ny, float span_x[2], float span_y[2], float tile_dim[2]);
int gr_gridmap_stat(const gr_gridmap *map, int key, uint64_t *value);
int gr_gridmap_set_launch(gr_gridmap *map, uint32_t range_groups, uint32_t frame_groups, uint32_t check_groups);   /* 0: default; the result never depends on it */
int gr_gridmap_clear(gr_gridmap *map);
int gr_gridmap_accumulate_batch(gr_gridmap *map, uint32_t first_slot, uint32_t n_frames, const char *group, int value,
                                const float *offset /* [n_frames] or NULL */, int flags,
                                uint64_t *n_outside /* [n_frames] or NULL */, int *status_out /* [n_frames] or NULL */);
int gr_gridmap_read(gr_gridmap *map, uint64_t *count, int64_t *sum_q, float *mean);

/* ---------------------------------------------------------------- Segments: per-residue / per-molecule centres over resident frames
 * The loop `for part in group_split_by_resid(..) { group_get_com(part) }` (src/system/groups.rs:344-435, :514-558) or over
 * molecule_iter (iterating.rs:238-245), run every frame: here the parts are ONE object -- an ordered list of M non-empty, strictly
 * ascending atom lists ("segments"; they may overlap, atoms may belong to none) -- and the centres of all of them, for a block of
 * resident frames, are one call.  The object keeps a pointer to its context: destroy it first.
 *   gr_segments_create         explicit lists, CSR: offsets[n_segments + 1] into `atoms`.  GR_E_INVALID_ARG for NULL pointers, offsets
 *                              that decrease or a list that is not strictly ascending; GR_E_EMPTY_GROUP for n_segments == 0 or an empty
 *                              segment; GR_E_OUT_OF_RANGE (gr_last_error_index = the atom) for an atom >= n_atoms.
 *   gr_segments_from_labels    group_split_by_resid / group_split_by_resname (groups.rs:391-435, :514-558) with labels[n_atoms] (the
 *                              residue numbers; for names, one number per distinct name): the atoms of `group` (NULL: all atoms) in
 *                              index order, an atom joins the segment of its label, a label seen for the first time opens a new
 *                              segment at the END (the reference's IndexMap order, "the order of residues in the system"); atoms of one
 *                              label that are not adjacent land in the same segment.  GR_E_GROUP_NOT_FOUND, GR_E_EMPTY_GROUP.
 *   gr_segments_from_molecules one segment per molecule of the bond topology (gr_add_bond), ordered by lowest atom, atoms ascending; an
 *                              atom without bonds is a segment of its own (what molecule_iter yields for it).  A snapshot: later bond
 *                              changes do not change the object.
 *   gr_segments_count, _sizes (out[M]), _atoms (segment s: *n = its size, at most `cap` atoms written, out may be NULL)
 *   gr_segments_stat           GR_SEG_STAT_TEAM4 / _TEAM16 / _WAVE / _WORKGROUP: segments of each team class (below);
 *                              GR_SEG_STAT_LAST_LAUNCHES / _LAST_LAUNCH_SETS: kernel launches / launch sets of the last centre call
 *   gr_segments_center_batch   out[f][s][0..2] = the centre gr_group_center_batch(kind, weighted) gives for segment s as a group in
 *                              frame f, for the n_frames slots from first_slot: GR_CENTER_NAIVE, _ESTIMATE or _PBC, the same per-atom
 *                              arithmetic and closing formulas (the f32 terms added in f64), the same box checks per frame (none for
 *                              GR_CENTER_NAIVE; strict mode included).  Segments are independent calls in the reference: a segment
 *                              with an atom without position (or mass, when weighted) is NaN, every other segment of the frame keeps
 *                              its value; status_out[f] is the status of the FIRST failing segment in segment order, with the index
 *                              gr_group_center_batch reports for that segment as a group.  A frame that fails its box check is NaN
 *                              everywhere.  Return value, message and gr_last_error_index: the first failed frame (batch rules below).
 *                              Any number of frames (the device block holds one 1024-frame piece at a time).
 *   gr_segments_center_batch_device  the same, left on the device: *out_dev -> [n_frames][M][3], valid until the next call on the same
 *                              object, read with gr_device_read; at most 1024 frames (GR_E_INVALID_ARG beyond); *n_segments = M
 *                              (out_dev and n_segments may each be NULL).
 *   gr_segments_gyration_batch the shape of every segment in every frame (gmx gyrate / gmx principal per residue, lipid or chain):
 *                              moments[f][s][0..9] = the centre (0..2: the very bits gr_segments_center_batch(kind, weighted) gives, nm),
 *                              the radius of gyration Rg (3, nm) and the gyration tensor S (4..9: xx yy zz xy xz yz, nm^2),
 *                              S_ab = sum w (r_a - <r_a>)(r_b - <r_b>) / sum w with w the mass (weighted) or 1, Rg = sqrt(tr S).  The
 *                              atoms are taken as x - centre (GR_CENTER_NAIVE) or as the minimum image vector from the centre
 *                              (_ESTIMATE, _PBC: a segment split by the cell faces is measured whole); the sums are f64 and S is taken
 *                              about the weighted MEAN of those vectors, so it does not depend on the centre's rounding or on
 *                              _ESTIMATE being an estimate.  A diagonal entry below zero is stored as zero.  A segment of ONE atom
 *                              has S = 0, Rg = 0, eigenvalues 0 and the identity as axes.
 *                              axes (may be NULL) [f][s][0..11] = the eigenvalues lambda_1 >= lambda_2 >= lambda_3 of the RETURNED f32
 *                              tensor (0..2, nm^2) and the unit eigenvectors v_1, v_2, v_3 as rows (3..11).  Sign convention: v_1 and
 *                              v_2 are each flipped so that their component of largest magnitude is positive (the first such
 *                              component on ties), v_3 = v_1 x v_2 (right-handed).  Equal eigenvalues keep the solver's order.
 *                              Box checks, strict mode, slot checks, NaN rows (all 10 / 12 values of a failed segment, every
 *                              segment of a frame that fails its box check), status_out, return value, message and
 *                              gr_last_error_index are those of gr_segments_center_batch for the same kind.  moments == NULL or an
 *                              unknown kind: GR_E_INVALID_ARG.  A segment above 4096 atoms is owned by one 256-lane workgroup per
 *                              frame: a whole large system as ONE segment works but is slow.
 *   gr_segments_gyration_batch_device  the same, left on the device: *moments_dev -> [n_frames][M][10], *axes_dev -> [n_frames][M][12]
 *                              (NULL unless want_axes), valid until the next call on the same object, read with gr_device_read;
 *                              at most one piece of frames (GR_E_INVALID_ARG beyond).  The pointers may each be NULL.
 *   gr_segments_set_piece_frames  a 1024-frame segment of a gyration call is worked in PIECES of frames so that the device block
 *                              (88 bytes per frame and segment) stays within 256 MiB (one frame if that alone is more; at most 1024
 *                              frames); n forces pieces of n frames, 0 restores the default.  No result depends on the piece size.
 *                              GR_SEG_STAT_LAST_PIECES: pieces of the last gyration call; GR_SEG_STAT_LAST_LAUNCHES then counts one
 *                              kernel per class that has segments per piece, plus one for the axes per piece when asked.
 * Every segment is owned by exactly one TEAM of lanes, chosen by its size when the object is made: <= 4 atoms 4 lanes (16 segments per
 * wave at a time), <= 16 atoms 16 lanes, <= 4096 atoms one wave, larger one 256-lane workgroup; a call is one launch per class that
 * has segments.  The team adds its lanes' f64 totals in a fixed tree and runs both stages of a GR_CENTER_PBC centre back to back;
 * no atomics touch the sums, so a segment's result depends on its atoms, its class and the frame only -- not on its neighbours, the
 * batch or the run. */
enum { GR_SEG_STAT_TEAM4 = 1, GR_SEG_STAT_TEAM16 = 2, GR_SEG_STAT_WAVE = 3, GR_SEG_STAT_WORKGROUP = 4, GR_SEG_STAT_LAST_LAUNCHES = 5,
       GR_SEG_STAT_LAST_LAUNCH_SETS = 6, GR_SEG_STAT_LAST_PIECES = 7 };
gr_segments *gr_segments_create(gr_ctx *ctx, const uint64_t *offsets, const uint64_t *atoms, uint64_t n_segments, int *status);
gr_segments *gr_segments_from_labels(gr_ctx *ctx, const char *group, const uint64_t *labels /* [n_atoms] */, int *status);
gr_segments *gr_segments_from_molecules(gr_ctx *ctx, int *status);
void gr_segments_destroy(gr_segments *seg);
uint64_t gr_segments_count(const gr_segments *seg);
int gr_segments_sizes(const gr_segments *seg, uint64_t *out /* [M] */);
int gr_segments_atoms(const gr_segments *seg, uint64_t s, uint64_t *out, uint64_t cap, uint64_t *n);
int gr_segments_stat(const gr_segments *seg, int key, uint64_t *value);
int gr_segments_center_batch(gr_segments *seg, uint32_t first_slot, uint32_t n_frames, int kind, int weighted,
                             float *out /* [n_frames][M][3] */, int *status_out /* [n_frames] or NULL */);
int gr_segments_center_batch_device(gr_segments *seg, uint32_t first_slot, uint32_t n_frames, int kind, int weighted,
                                    float **out_dev, uint64_t *n_segments, int *status_out);
int gr_segments_gyration_batch(gr_segments *seg, uint32_t first_slot, uint32_t n_frames, int kind, int weighted,
                               float *moments /* [n_frames][M][10] */, float *axes /* [n_frames][M][12] or NULL */,
                               int *status_out /* [n_frames] or NULL */);
int gr_segments_gyration_batch_device(gr_segments *seg, uint32_t first_slot, uint32_t n_frames, int kind, int weighted, int want_axes,
                                      float **moments_dev, float **axes_dev, uint64_t *n_segments, int *status_out);
int gr_segments_set_piece_frames(gr_segments *seg, uint32_t n);

/* ---------------------------------------------------------------- per-frame analyses over a batch of slots
 * The calls above for `n_frames` consecutive slots in ONE set of launches and one read-back (a trajectory loop of
 * group_get_com / atoms_center / atoms_wrap over resident frames; per-frame calls cost a launch + a synchronisation each).
 * Every frame is judged on its own: status_out[f] (may be NULL) receives the frame's status, a failed frame yields NaN /
 * is left untouched, and the return value is the first frame's error (message and index as for the single calls). */
int gr_group_center_batch(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *group, int kind, int weighted,
                          float *out /* [n_frames][3] */, int *status_out);
int gr_group_translate_batch(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *group, const float v[3], int *status_out);
int gr_group_wrap_batch(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *group, int *status_out);
int gr_atoms_center_batch(gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *ref_group, int dim, int weighted, int *status_out);

/* ---------------------------------------------------------------- trr reader
 * TrrReader / TrrFrameData (src/io/trr_io.rs:30-135 over the vendored xdrfile's read_trr): an own reader of the GROMACS trr
 * format.  gr_trr_open indexes the file (frames are random-access, reads are thread-safe).  A frame carries any of positions /
 * velocities / forces / box, in single or double precision; *sections = 1 positions | 2 velocities | 4 forces | 8 box.
 * gr_trr_read_frame converts to f32 into the caller's buffers (any may be NULL); a section the frame does not carry reads as
 * zeros, which the reference turns into "no position / velocity / force" (trr_io.rs:101-126).  gr_trr_read_frames_device
 * copies the raw big-endian position sections of a batch of frames to the GPU and converts them there, straight into the
 * slots (asynchronous like gr_frame_upload; all-zero positions become the NaN marker of a missing position). */
typedef struct gr_trr gr_trr;
gr_trr *gr_trr_open(const char *path, int *status);
void gr_trr_close(gr_trr *trr);
uint64_t gr_trr_n_atoms(const gr_trr *trr);
uint64_t gr_trr_n_frames(const gr_trr *trr);
int gr_trr_frame_info(const gr_trr *trr, uint64_t frame, uint64_t *step, float *time, float *lambda, float box9[9], int *sections, int *double_precision);
int gr_trr_read_frame(const gr_trr *trr, uint64_t frame, float *xyz, float *velocities, float *forces, float box9[9], uint64_t *step, float *time, float *lambda);
int gr_trr_read_frames_device(const gr_trr *trr, uint64_t first_frame, uint32_t n_frames, uint64_t frame_step, gr_ctx *ctx, uint32_t first_slot,
                              uint64_t *steps, float *times);
/* TrrWriter (src/io/trr_io.rs:441-520 over xdrfile's write_trr): single precision, box + the sections whose array is not
 * NULL (the reference always writes positions, velocities and forces, zeros where an atom has none), byte for byte the
 * reference writer's frames.  A position without value (NaN in x) is written as zeros; box9 NULL writes a zero matrix. */
typedef struct gr_trr_writer gr_trr_writer;
gr_trr_writer *gr_trr_writer_open(const char *path, int *status);
int gr_trr_writer_close(gr_trr_writer *w);
int gr_trr_write_frame(gr_trr_writer *w, uint64_t n_atoms, const float *xyz, const float *velocities, const float *forces, const float box9[9],
                       int64_t step, float time, float lambda);

/* ---------------------------------------------------------------- xtc writer (host side; the step after calc_rmsd_and_fit)
 * XtcWriter::new / write_frame (src/io/xtc_io/mod.rs:256-331 over xdrfile's write_xtc): the library's own encoder, byte for
 * byte the stream the reference writes for the same coordinates (the reference's golden fitted trajectories are files).
 * Atoms without a position are written as the origin, a frame without box as a zero matrix (xdrfile.rs:188-200).
 * gr_xtc_write_slots streams device frames out: D2H of slot k+1 overlaps the encoding of slot k (`host_threads` encoders,
 * 0 = up to 16), frames are written in slot order; `group` = NULL writes every atom, else the group's atoms in its order
 * (xtc_group_writer_init).  A coordinate whose value x precision does not fit the format's 32-bit integers (or a NaN in
 * y / z) makes the call fail with GR_E_OUT_OF_RANGE and that frame is not written (gr_xtc_write_slots stops there: the frames
 * before it are in the file, as after a loop of write_frame calls) -- the reference's C writer prints "Internal
 * overflow compressing coordinates." and converts anyway (undefined behaviour, external/xdrfile/xdrfile.c:1025-1030). */
typedef struct gr_xtc_writer gr_xtc_writer;
gr_xtc_writer *gr_xtc_writer_open(const char *path, int *status);
int gr_xtc_writer_close(gr_xtc_writer *w);
int gr_xtc_write_frame(gr_xtc_writer *w, uint64_t n_atoms, const float *xyz, const float box9[9], int64_t step, float time, float precision);
int gr_xtc_write_slots(gr_xtc_writer *w, gr_ctx *ctx, uint32_t first_slot, uint32_t n_frames, const char *group,
                       const int64_t *steps, const float *times, float precision, int host_threads);

/* ---------------------------------------------------------------- geometry selection
 * Shape::inside of Sphere / Rectangular / Cylinder / TriangularPrism (src/structures/shape.rs:110-185,252-276,431-461),
 * the PBC-free NaiveShape variants (:466-505), and System::group_create_from_geometry / _geometries
 * (src/system/groups.rs:94-188 over Group::apply_geometries, src/structures/group.rs:119-175): the new group holds, in
 * the source group's order, the atoms that have a position and lie inside EVERY shape.  Needs a box (GR_E_NO_BOX); the reference
 * also needs it orthogonal (groups.rs:108-110: GR_E_NOT_ORTHOGONAL in strict-orthogonal mode) -- otherwise a non-orthogonal box
 * takes the image-enumeration extension (some lattice image of the atom lies inside the shape); the name must be valid (GR_E_INVALID_NAME: empty, or one of
 * '"&|!@()<>= , auxiliary.rs:37-51); an existing group is replaced and GR_E_GROUP_EXISTS returned (the reference's
 * AlreadyExistsWarning).  The predicate runs on the device (one ballot bit per atom), the blocks are built on the host. */
enum { GR_SHAPE_SPHERE = 1, GR_SHAPE_RECTANGULAR = 2, GR_SHAPE_CYLINDER = 3, GR_SHAPE_TRIANGULAR_PRISM = 4 };
#define GR_MAX_SHAPES 8
typedef struct gr_shape {
    int kind;
    float position[3];         /* sphere centre / box origin / centre of the cylinder's base / first vertex of the prism's base */
    float size[3];             /* sphere: radius ; rectangular: x y z ; cylinder: radius, height ; prism: height */
    float base2[3], base3[3];  /* prism: the other two vertices of the base */
    int orientation, plane;    /* GR_DIM_* ; cylinder and prism (filled by the constructors) */
} gr_shape;
int gr_shape_sphere(gr_shape *s, const float position[3], float radius);                                   /* Sphere::new :95-97 */
int gr_shape_rectangular(gr_shape *s, const float position[3], float x, float y, float z);                 /* Rectangular::new :141-143 */
/* Cylinder::new :211-229 -- orientation GR_DIM_X / _Y / _Z, anything else is GR_E_INVALID_ARG (the reference panics) */
int gr_shape_cylinder(gr_shape *s, const float position[3], float radius, float height, int orientation);
/* TriangularPrism::new :343-378 -- GR_E_INVALID_ARG where the reference panics (base not in a coordinate plane / degenerate) */
int gr_shape_triangular_prism(gr_shape *s, const float base1[3], const float base2[3], const float base3[3], float height);
/* Shape::inside / NaiveShape::inside_naive for one point (host; box9 may be NULL when naive) */
int gr_shape_inside(const gr_shape *s, const float point[3], const float box9[9], int naive, int *inside);
int gr_group_create_from_geometries(gr_ctx *ctx, uint32_t slot, const char *name, const char *source_group,
                                    const gr_shape *shapes, size_t n_shapes, int naive);

/* ---------------------------------------------------------------- Region: geometry selections over a block of resident frames
 * The loop `for atom in group_iter(..).filter_geometry(shape)` (src/lib.rs:170-188, iterators.rs:994-1004, :1094-1105) or
 * group_create_from_geometries (groups.rs:94-188), run every frame: here the shapes are ONE object and the selection of a block of resident
 * slots is one call.  For every frame: the atoms of a group that have a position and lie inside EVERY shape, in the source group's
 * iteration order -- the list gr_group_create_from_geometries would make of that frame.  The object keeps a pointer to its context:
 * destroy it first.
 *   gr_region_create           up to GR_MAX_SHAPES shapes and the naive flag, validated as by gr_group_create_from_geometries:
 *                              GR_E_INVALID_ARG for more shapes than that, an invalid kind or orientation, or a prism with `naive`.
 *                              n_shapes == 0 is allowed: every atom with a position is inside.
 *   gr_region_select_batch     selects in the n_frames slots from first_slot among the atoms of `group` (NULL: all atoms).
 *                              anchor (may be NULL: the shapes as stored): the shapes of frame f are the stored ones moved by anchor[f] --
 *                              position, and for the prism base2 and base3, become stored + anchor[f], one f32 add per component (no fma:
 *                              the same bits on the host and on the device).  The stored position thus acts as an offset from a
 *                              per-frame point, e.g. (0, 0, -h/2) from a centre of gr_group_center_batch.  A frame whose anchor has a
 *                              component that is not finite fails with GR_E_INVALID_ARG (naive or not).
 *                              Per-frame checks, none of them when naive: GR_E_NO_BOX, the slot's box status (GR_E_ZERO_BOX ...),
 *                              GR_E_NOT_ORTHOGONAL in strict mode, and GR_E_UNSUPPORTED_BOX where a shape reaches more lattice images
 *                              of a non-orthogonal cell than the selection enumerates.  An atom without a position is inside nothing;
 *                              that is not an error.  A failed frame has n_inside[f] = 0 and an empty list, its neighbours are what they
 *                              are without it; status_out[f] is its status, and the return value, message and gr_last_error_index are
 *                              the first failed frame's (batch rules below).  GR_E_GROUP_NOT_FOUND fails the whole call; an empty
 *                              group is no error and gives empty lists (the reference's iterator).  Any number of frames (walked in
 *                              1024-frame segments); the frames are not modified.  A failed call -- a HIP error, a refused argument --
 *                              leaves the object with an empty result (0 frames).
 *                              The result stays on the device, in the object, until the next gr_region_select_batch on it or its
 *                              destruction: u32 atom indices, frame after frame, and u64 offsets[n_frames + 1] -- offsets[f] ..
 *                              offsets[f + 1] delimit frame f.  The list is grown to what the call actually selects (the counts of
 *                              a piece are read back before its lists are written), never sized n_frames x n_atoms.
 *   gr_region_read             the result on the host, widened to u64: offsets (may be NULL), atoms (NULL: only *n_total is reported;
 *                              cap < total: GR_E_INVALID_ARG), *n_total (may be NULL)
 *   gr_region_read_device      the device pointers (read with gr_device_read), the number of frames and of entries; each may be NULL
 *   gr_region_group            installs frame `frame`'s list as the group `name`: name validation, replacement and GR_E_GROUP_EXISTS as
 *                              gr_group_create_from_geometries; GR_E_INVALID_ARG for a frame beyond the last call's, or one that failed
 *   gr_region_set_piece_frames a segment is worked in pieces of frames so that the mask workspace (n/8 bytes per frame) stays within 8 MiB
 *                              (one frame where that alone is larger); n forces pieces of n frames, 0 restores the default.  The result
 *                              does not depend on the piece size: the call exists so that piece boundaries can be tested at small sizes.
 *   gr_region_stat             GR_RG_STAT_LAST_LAUNCHES / _LAST_PIECES: kernel launches / pieces of the last selection; _LAST_TOTAL: its
 *                              entries; GR_RG_STAT_CHUNK: ordinals of the source group that one workgroup owns (1024)
 * Per piece three launches: ballot words and per-chunk counts (one workgroup owns one chunk of one frame), an exclusive scan of the
 * counts per frame, and the lists, where every position is computed from the scans and popcounts.  No atomic decides a position or a
 * count, so the lists are in ordinal order and the same bits whatever the batch, the piece size, the neighbours or the run. */
enum { GR_RG_STAT_LAST_LAUNCHES = 1, GR_RG_STAT_LAST_PIECES = 2, GR_RG_STAT_LAST_TOTAL = 3, GR_RG_STAT_CHUNK = 4 };
gr_region *gr_region_create(gr_ctx *ctx, const gr_shape *shapes, size_t n_shapes, int naive, int *status);
void gr_region_destroy(gr_region *r);
int gr_region_select_batch(gr_region *r, uint32_t first_slot, uint32_t n_frames, const char *group /* NULL: all atoms */,
                           const float *anchor /* [n_frames][3] or NULL */,
                           uint64_t *n_inside /* [n_frames] or NULL */, int *status_out /* [n_frames] or NULL */);
int gr_region_read(gr_region *r, uint64_t *offsets /* [n_frames + 1] or NULL */, uint64_t *atoms, uint64_t cap, uint64_t *n_total);
int gr_region_read_device(gr_region *r, const uint32_t **atoms_dev, const uint64_t **offsets_dev, uint64_t *n_frames, uint64_t *n_total);
int gr_region_group(gr_region *r, uint32_t frame, const char *name);
int gr_region_set_piece_frames(gr_region *r, uint32_t n);
int gr_region_stat(const gr_region *r, int key, uint64_t *value);

/* ---------------------------------------------------------------- Contacts: cut-off pair search over a block of resident frames
 * The loop CellGrid::new + neighbors_iter + distance filter (src/structures/cellgrid.rs:301-409, :434-476, src/system/hbonds.rs:248-265),
 * run every frame: here the two groups and the cut-off are ONE object and a block of resident slots is one call.  The result of a frame
 * is exactly what gr_group_pairs_within(ctx, slot, group1, group2, cutoff, ...) gives for that slot: all pairs (i in group1, j in group2,
 * i != j) with distance(x_j, x_i) <= cutoff, by i then j, d that distance (the same expression on the same bits).  The object keeps a
 * pointer to its context: destroy it first.
 *   gr_contacts_create         snapshots the atoms of both groups in group order (later changes to the groups do not change the object).
 *                              GR_E_GROUP_NOT_FOUND (group1 is looked up first); GR_E_INVALID_ARG unless cutoff > 0 (cellgrid.rs:323-325).
 *                              Empty groups are allowed.
 *   per-frame statuses         as gr_group_pairs_within, in its order: GR_E_NO_BOX, the slot's box status, GR_E_NOT_ORTHOGONAL in strict
 *                              mode; nothing further when either group is empty (no position is looked at); else GR_E_NO_POSITION with
 *                              gr_last_error_index = the first atom of GROUP 2 (group order) without position, else the first of group 1.
 *                              A failed frame has 0 pairs, an empty list, a zero per_atom row and a zero histogram row; its neighbours
 *                              are what they are without it.  status_out[f] is the frame's status, and the return value, message and
 *                              index are the first failed frame's (batch rules below).  Any number of frames (walked in 1024-frame
 *                              segments); the frames are not modified.  A hard error -- HIP, a refused argument -- leaves the object
 *                              with an empty result of 0 frames.
 *   gr_contacts_pairs_batch    the pair lists of n_frames slots from first_slot, left on the device in the object until the next
 *                              gr_contacts_pairs_batch on it or its destruction: u32 i, u32 j, f32 d, frame after frame, and u64
 *                              offsets[n_frames + 1].  The lists are grown to what the call actually finds (the counts of a piece are
 *                              read back before its lists are written), never sized n1 x n2.  When the call's total exceeds max_pairs no
 *                              list is kept (count only): n_pairs, *n_total and the offsets are still right, gr_contacts_read with list
 *                              pointers returns GR_E_INVALID_ARG, and GR_CT_STAT_LAST_TOTAL reports the total.
 *   gr_contacts_read           the last pairs call on the host: offsets (may be NULL); i, j, d (all NULL: only totals are reported;
 *                              cap < total: GR_E_INVALID_ARG); *n_total (may be NULL)
 *   gr_contacts_read_device    the device pointers (read with gr_device_read; NULL lists after a count-only call), frames and pairs
 *   gr_contacts_count_batch    the same walk without the lists: per_atom[f][k] = pairs of the k-th atom of group1 in frame f,
 *                              n_pairs[f] their sum -- exactly what the lists would give.  Does not touch the stored lists.
 *   gr_contacts_hist_batch     hist[f][b] over [0, cutoff) by the rule of GR_PD_HIST applied to the pairs of the list: s = (float)nbins /
 *                              cutoff in f32, bin = (uint32_t)(d * s), counted iff d * s < nbins (a pair at exactly d == cutoff is in
 *                              the list but may fall outside).  nbins 1 .. 4096, else GR_E_INVALID_ARG.  Integer adds only: exact.
 *   gr_contacts_sizes          atoms in the two snapshots
 *   gr_contacts_set_piece_frames a segment is worked in pieces of frames so that the key, rank and sorted-atom workspace stays within
 *                              256 MiB (one frame where that alone is larger); n forces pieces of n frames, 0 restores the default.
 *                              The result never depends on it.
 *   gr_contacts_stat           GR_CT_STAT_LAST_LAUNCHES / _LAST_PIECES: kernel launches / pieces of the last call; _LAST_TOTAL: pairs of
 *                              the last pairs call; GR_CT_STAT_TILE: candidates that one workgroup stages in LDS at once (512).
 *                              Over the frames of the last call that passed their host checks: _LAST_RUNS: runs of query cells walked;
 *                              _LAST_CELLS: cells of their grids; _LAST_RUN_CELLS_MIN / _MAX: fewest / most query cells per run;
 *                              _LAST_WALK_GROUPS: the largest grid of a walk launch
 *   gr_contacts_set_walk_groups caps the workgroups of a walk launch: min(runs of the piece, n), 0 restores the default (8192).  A
 *                              workgroup then serves several runs, and frames, in turn.  For tests; the result never depends on it.
 * Per piece a fixed number of launches: a counting sort of both groups into the cells of every frame's own grid (one key space for the
 * piece), a count walk, a scan, and the write walk.  The walk works per run of query cells adjacent along x: their candidates are staged
 * once in LDS and ordered by atom index there, a team of lanes shares a query and places its hits by ballot and popcount.  No atomic
 * decides a position or a count, so the lists are the same bits whatever the batch, the piece size, the neighbours or the run. */
enum { GR_CT_STAT_LAST_LAUNCHES = 1, GR_CT_STAT_LAST_PIECES = 2, GR_CT_STAT_LAST_TOTAL = 3, GR_CT_STAT_TILE = 4, GR_CT_STAT_LAST_RUNS = 5,
       GR_CT_STAT_LAST_CELLS = 6, GR_CT_STAT_LAST_RUN_CELLS_MIN = 7, GR_CT_STAT_LAST_RUN_CELLS_MAX = 8, GR_CT_STAT_LAST_WALK_GROUPS = 9 };
gr_contacts *gr_contacts_create(gr_ctx *ctx, const char *group1, const char *group2, float cutoff, int *status);
void gr_contacts_destroy(gr_contacts *ct);
int gr_contacts_pairs_batch(gr_contacts *ct, uint32_t first_slot, uint32_t n_frames, uint64_t max_pairs,
                            uint64_t *n_pairs /* [n_frames] or NULL */, uint64_t *n_total /* or NULL */, int *status_out /* [n_frames] or NULL */);
int gr_contacts_read(gr_contacts *ct, uint64_t *offsets /* [n_frames + 1] or NULL */, uint32_t *i, uint32_t *j, float *d, uint64_t cap, uint64_t *n_total);
int gr_contacts_read_device(gr_contacts *ct, const uint32_t **i_dev, const uint32_t **j_dev, const float **d_dev,
                            const uint64_t **offsets_dev, uint64_t *n_frames, uint64_t *n_total);
int gr_contacts_count_batch(gr_contacts *ct, uint32_t first_slot, uint32_t n_frames,
                            uint32_t *per_atom /* [n_frames][n1] or NULL */, uint64_t *n_pairs /* [n_frames] or NULL */, int *status_out);
int gr_contacts_hist_batch(gr_contacts *ct, uint32_t first_slot, uint32_t n_frames, uint32_t nbins,
                           uint64_t *hist /* [n_frames][nbins] */, int *status_out);
int gr_contacts_sizes(const gr_contacts *ct, uint64_t *n1, uint64_t *n2);
int gr_contacts_set_piece_frames(gr_contacts *ct, uint32_t n);      /* 0: default; the result never depends on it */
int gr_contacts_set_walk_groups(gr_contacts *ct, uint32_t n);       /* 0: default; the result never depends on it */
int gr_contacts_stat(const gr_contacts *ct, int key, uint64_t *value);

/* ---------------------------------------------------------------- RMSDPanel: the all-pairs RMSD matrix over packed frames
 * The double loop of System::calc_rmsd(&other, group) (src/system/rmsd.rs:75-166) over a trajectory.  Each side of calc_rmsd is
 * prepared without its partner (extract_data_from_system :425-446: get_com, shift by box centre - com, wrap; kabsch_rmsd :547-603
 * subtracts the box centre), so a PANEL keeps, per appended frame, the group's centred coordinates (f32) and G = sum w |x|^2 (f64), and
 * the slots the frames came from may be overwritten as soon as the append returns: a trajectory far longer than the context's slots
 * is packed block by block (a 1e4-atom group costs 120 kB per frame).  The matrix of two panels is a dense product in f64
 * (v_mfma_f64_16x16x4_f64) closed per pair by gr_best_rotation: rmsd^2 = (G_p + G_q - 2 tr(R^T Hw)) / W.  The object keeps a pointer to
 * its context: destroy it first.
 *   gr_rmsd_panel_create        snapshots the group's atoms (group order) and their masses; capacity 1 .. 2^20 frames (else
 *                               GR_E_INVALID_ARG).  GR_E_GROUP_NOT_FOUND, GR_E_EMPTY_GROUP; GR_E_NO_MASS with gr_last_error_index = the
 *                               first atom of the group without mass, as the RMSD calls report it.
 *   gr_rmsd_panel_append_batch  packs the n_frames slots from first_slot as the next rows, in one fixed set of launches per 1024-frame
 *                               segment: the centre stages of gr_group_center_batch(GR_CENTER_PBC, weighted) on the device, then the
 *                               pack kernel.  Per frame (batch rules below) the status gr_rmsd_batch gives the slot as the current frame:
 *                               GR_E_NO_BOX, GR_E_NOT_ORTHOGONAL in strict mode, the slot's box status, GR_E_NO_POSITION with the atom's
 *                               index.  A failed frame still takes a row, marked invalid; status_out[f] is the frame's status and the
 *                               return value, message and index are the first failed frame's.  Beyond the capacity: GR_E_INVALID_ARG,
 *                               nothing changes.  GR_E_INVALID_ARG too when the masses of the atoms no longer equal the snapshot.
 *   gr_rmsd_panel_clear         forgets the rows (the capacity stays)
 *   gr_rmsd_panel_frames        rows appended so far, failed ones included;  gr_rmsd_panel_n_atoms: atoms of the snapshot
 *   gr_rmsd_panel_status        the rows' statuses, out[frames]
 *   gr_rmsd_matrix              out[i][j] (host, [n_rows][n_cols]) = calc_rmsd of row frame i as self against column frame j as
 *                               reference; NaN when either frame is invalid.  cols == rows is allowed and NULL is shorthand for it: one
 *                               triangle is computed and mirrored.  Any size: the matrix is worked in column blocks of at most 2^26
 *                               entries (gr_rmsd_panel_set_block_entries on `rows`: another size, 0 the default; the result never depends on it).
 *                               GR_E_INVALID_ARG for an empty panel; GR_E_INCONSISTENT_GROUP (counts = n_cols_atoms, n_rows_atoms)
 *                               when the panels hold different numbers of atoms; GR_E_INVALID_ARG when their mass snapshots are not
 *                               bit-equal or they live on different devices (different contexts of one device are fine).  THIS NARROWS
 *                               THE REFERENCE, which would weight with the reference side's masses: with one set of masses G is a
 *                               constant of the frame, and the RMSD is symmetric in its two frames.
 *   gr_rmsd_matrix_device       the same, left on the device in the `rows` object (read with gr_device_read) until the next matrix call
 *                               on that object or its destruction; n_rows x n_cols <= 2^28 entries, else GR_E_INVALID_ARG.
 * Sums are f64 with exact products, their order depends on the number of atoms alone and no atomic touches them; the closing step
 * works on a canonical orientation of the pair.  So an entry depends on its two frames (as an unordered pair) and on N alone: not on the
 * frames' places in their panels, on how they were appended, on their neighbours or on the run; the matrix of a panel with itself is
 * exactly symmetric. */
gr_rmsd_panel *gr_rmsd_panel_create(gr_ctx *ctx, const char *group, uint32_t capacity_frames, int *status);
void gr_rmsd_panel_destroy(gr_rmsd_panel *p);
int gr_rmsd_panel_append_batch(gr_rmsd_panel *p, uint32_t first_slot, uint32_t n_frames, int *status_out /* [n_frames] or NULL */);
int gr_rmsd_panel_clear(gr_rmsd_panel *p);
uint32_t gr_rmsd_panel_frames(const gr_rmsd_panel *p);
uint64_t gr_rmsd_panel_n_atoms(const gr_rmsd_panel *p);
int gr_rmsd_panel_status(const gr_rmsd_panel *p, int *out /* [frames] */);
int gr_rmsd_panel_set_block_entries(gr_rmsd_panel *p, uint64_t n);  /* 0: default; the result never depends on it */
int gr_rmsd_matrix(gr_rmsd_panel *rows, gr_rmsd_panel *cols /* or NULL */, float *out /* [n_rows][n_cols], host */);
int gr_rmsd_matrix_device(gr_rmsd_panel *rows, gr_rmsd_panel *cols /* or NULL */, float **out_dev, uint32_t *n_rows, uint32_t *n_cols);

/* ---------------------------------------------------------------- Fluctuations: mean structure and per-atom RMSF over resident frames
 * The loop every analysis script writes around calc_rmsd_and_fit (the reference has no function for it): add up the fitted frames, take
 * the average structure and the root mean square fluctuation of every atom.  Per atom and component the object keeps on the device an
 * ORIGIN o (f32: the position in the first frame the object ever counted), s = sum d (f64) and q = sum d * d (f64) with d = x - o, one
 * f32 subtraction that is then widened (d * d is exact in f64).  Frames are added in ascending order, one after another, by the lane that
 * owns the atom: s and q depend on the SEQUENCE of counted frames alone -- not on how it was cut into calls, 1024-frame segments or grids
 * -- and no atomic touches them.  Positions are taken as they are (no box is needed, nothing is unwrapped: the frames are expected to be
 * fitted or whole).  The object keeps a pointer to its context: destroy it first.
 *   gr_fluct_create            snapshots the group's atoms (S atoms, group order); the group may change or go afterwards.
 *                              GR_E_GROUP_NOT_FOUND, GR_E_EMPTY_GROUP.
 *   gr_fluct_accumulate_batch  counts the n_frames slots from first_slot.  A frame in which an atom of the snapshot has no position fails
 *                              with GR_E_NO_POSITION and gr_last_error_index = the lowest such atom, and is counted for NO atom (a check
 *                              kernel decides per frame before anything is added); when the first frame fails the origin comes from the
 *                              first frame that is counted.  Batch rules: status_out[f] is each frame's status, the return value, message
 *                              and index are the first failed frame's, a hard error writes nothing.  Frames and slots are never modified.
 *   gr_fluct_clear             forgets every frame (and the origin)
 *   gr_fluct_frames            counted frames;  gr_fluct_n_atoms: atoms of the snapshot
 *   gr_fluct_read              closes the sums on the host, in f64, with n counted frames: mean[k][c] = o + s / n, var[k][c] =
 *                              max(q - s^2 / n, 0) / n, rmsf[k] = sqrt(var_x + var_y + var_z); group order; each may be NULL.  n == 0:
 *                              all three are NaN and the call returns GR_OK.
 *   gr_fluct_read_raw          o, s, q as they stand ([S][3] each, group order) and n; each may be NULL
 *   gr_fluct_merge             adds src's frames to dst (the shards of gr_pool_* / gr_comm_* runs, two contexts, two devices).  Different
 *                              numbers of atoms: GR_E_INCONSISTENT_GROUP (counts = dst's, src's).  An empty src changes nothing; an empty
 *                              dst takes src's origin and sums unchanged; else src's sums are moved to dst's origin in f64, delta = o_src
 *                              - o_dst: s += s_src + n_src delta, q += q_src + 2 delta s_src + n_src delta^2.  Done on the host (60 B per
 *                              atom).  AFTER A MERGE THE SUMS ARE NO LONGER THOSE OF A SEQUENTIAL WALK: they are as accurate, but bit for
 *                              bit they depend on where the frames were split.  dst == src: GR_E_INVALID_ARG.
 *   gr_fluct_store_mean        writes the mean, rounded to f32, into the snapshot's atoms of `slot` of dst -- any context on the same
 *                              device with the same number of atoms, the object's own included (else GR_E_INVALID_ARG; n == 0 too).  Every
 *                              other atom, the pads and the slot's box stay as they are: the slot is the reference of a new
 *                              gr_rmsd_plan_create ("fit to the average, iterate").  Errors are reported on the object's context.
 *   gr_fluct_set_launch        test hook: the ranges the group is cut into (one wave each; 0: one per 64 units -- 4-atom groups of the
 *                              span, or list entries) and a cap on the grid of the position check.  The result never depends on it.
 *   gr_fluct_stat              GR_FL_STAT_*: launches so far, the grids of the last one, the form the snapshot is walked in (0 a
 *                              contiguous block, 1 an index list, 2 a span with a bit mask: at least half of the span's atoms are the
 *                              group's), the frames a lane has in flight */
enum { GR_FL_STAT_LAUNCHES = 1, GR_FL_STAT_LAST_RANGE_GROUPS = 2, GR_FL_STAT_LAST_CHECK_GROUPS = 3, GR_FL_STAT_FORM = 4, GR_FL_STAT_AHEAD = 5 };
gr_fluct *gr_fluct_create(gr_ctx *ctx, const char *group, int *status);
void gr_fluct_destroy(gr_fluct *f);
int gr_fluct_accumulate_batch(gr_fluct *f, uint32_t first_slot, uint32_t n_frames, int *status_out /* [n_frames] or NULL */);
int gr_fluct_clear(gr_fluct *f);
uint64_t gr_fluct_frames(const gr_fluct *f);
uint64_t gr_fluct_n_atoms(const gr_fluct *f);
int gr_fluct_read(gr_fluct *f, double *mean /* [S][3] */, double *var /* [S][3] */, double *rmsf /* [S] */);
int gr_fluct_read_raw(gr_fluct *f, float *origin /* [S][3] */, double *sum /* [S][3] */, double *sumsq /* [S][3] */, uint64_t *n);
int gr_fluct_merge(gr_fluct *dst, gr_fluct *src);
int gr_fluct_store_mean(gr_fluct *f, gr_ctx *dst, uint32_t slot);
int gr_fluct_set_launch(gr_fluct *f, uint32_t range_groups, uint32_t check_groups);   /* 0: default; the result never depends on it */
int gr_fluct_stat(const gr_fluct *f, int key, uint64_t *value);

/* ---------------------------------------------------------------- Covariance: positional covariance and DCCM over resident frames
 * The step after Fluctuations (the reference has no function for it): the full second moment of the fitted coordinates -- the 3S x 3S
 * covariance matrix of essential dynamics / PCA (gmx covar), optionally mass-weighted, and the S x S dynamical cross-correlation map.
 * For a snapshot of a group's S atoms (group order; D = 3S, dimension 3k + c) the object keeps on the device the ORIGIN o (f32 [D]: the
 * position in the first frame the object ever counted), s = sum d (f64 [D]) and Q = sum d_i d_j (f64 [D][D], the upper block triangle
 * stored) with d = x - o, one f32 subtraction that is then widened (every product is exact in f64).  Q grows by a symmetric rank-K update
 * on the f64 matrix cores: every entry belongs to one wave, which takes the stored value as its accumulator and adds the frames of a
 * segment in ascending trips of GR_CV_STAT_TRIP_FRAMES as one chain -- no split of the frames over waves, no partial sums, no atomics.
 * The bits of the state are therefore a function of the SEQUENCE OF CALLS alone (their frames and where the calls cut them): not of the
 * grid, gr_covar_set_launch, the context's history or the run; failed frames enter as zeros, which are neutral bit for bit.  Q is exactly
 * symmetric.  NOT guaranteed: the same bits when the same frames are cut into calls differently -- one matrix instruction adds four
 * frames in an order the hardware does not document, so different cuts agree to the rounding bound 2 n 2^-53 sum |d_i d_j| only.
 * Positions are taken as they are (frames are expected to be fitted).  The eigen-solve is the caller's (LAPACK dsyevd / numpy.linalg.eigh
 * on gr_covar_read).  The object keeps a pointer to its context: destroy it first.
 *   gr_covar_create            snapshots the group's atoms and their masses.  GR_E_GROUP_NOT_FOUND, GR_E_EMPTY_GROUP; more than
 *                              GR_CV_MAX_ATOMS atoms: GR_E_INVALID_ARG (the message names the cap; Q takes 36 S^2 bytes on the device).
 *   gr_covar_accumulate_batch  counts the n_frames slots from first_slot; Fluctuations' contract: a frame in which an atom of the snapshot
 *                              has no position fails with GR_E_NO_POSITION and gr_last_error_index = the lowest such atom and is counted
 *                              for NO dimension; when the first frame fails the origin comes from the first frame that is counted; a frame
 *                              without a box is counted.  Batch rules: status_out[f] is each frame's status, the return value, message
 *                              and index are the first failed frame's, a hard error writes nothing.  Frames and slots are never modified.
 *   gr_covar_clear             forgets every frame (and the origin)
 *   gr_covar_frames            counted frames;  gr_covar_n_atoms: atoms of the snapshot
 *   gr_covar_read_raw          o [D], s [D], Q [D][D] (the full square, mirrored on the host) as they stand, and n; each may be NULL
 *   gr_covar_read              closes the sums on the host, in f64, with n counted frames: mean[i] = o + s / n, cov[i][j] = (Q_ij - s_i
 *                              s_j / n) / n (divided by n, as gr_fluct_read); flags & GR_CV_MASS_WEIGHTED: times sqrt(m_i) sqrt(m_j), the
 *                              masses of the snapshot (NaN where a mass was never set).  Each may be NULL.  n == 0: NaN, GR_OK.
 *   gr_covar_read_dccm         corr[a][b] = sum_c cov[3a+c][3b+c] / sqrt(tr_a tr_b), tr_a = sum_c cov[3a+c][3a+c], unweighted, f64 [S][S].
 *                              An atom with tr = 0 has 1.0 on the diagonal and NaN elsewhere in its row and column.  n == 0: NaN.
 *   gr_covar_merge             adds src's frames to dst (same S; any context, any device), on the host in f64 with delta = o_src - o_dst:
 *                              s += s_src + n_src delta, Q_ij += Q_src,ij + delta_i s_src,j + s_src,i delta_j + n_src delta_i delta_j.
 *                              An empty src changes nothing, an empty dst takes src's state unchanged.  Different S:
 *                              GR_E_INCONSISTENT_GROUP (counts = dst's, src's); dst == src: GR_E_INVALID_ARG.  AFTER A MERGE THE SUMS ARE
 *                              NO LONGER THOSE OF ONE WALK: they are as accurate, but bit for bit they depend on where the frames were split.
 *   gr_covar_set_launch        test hook: caps on the grid of the product (it then strides over the blocks) and of the position check
 *                              (0: one workgroup per stored block / per 256 units).  The result never depends on it.
 *   gr_covar_stat              GR_CV_STAT_*: launches so far, the grids of the last one, the edge of a block of Q in dimensions, the
 *                              frames per trip of the product, the blocks of Q that are stored and computed */
#define GR_CV_MAX_ATOMS 4096u      /* S at most: 613 MB of Q on the device, 1.2 GB for the square gr_covar_read returns */
#define GR_CV_MASS_WEIGHTED 1u
enum { GR_CV_STAT_LAUNCHES = 1, GR_CV_STAT_LAST_PRODUCT_GROUPS = 2, GR_CV_STAT_LAST_CHECK_GROUPS = 3, GR_CV_STAT_BLOCK_EDGE = 4, GR_CV_STAT_TRIP_FRAMES = 5,
       GR_CV_STAT_BLOCKS = 6 };
gr_covar *gr_covar_create(gr_ctx *ctx, const char *group, int *status);
void gr_covar_destroy(gr_covar *cv);
int gr_covar_accumulate_batch(gr_covar *cv, uint32_t first_slot, uint32_t n_frames, int *status_out /* [n_frames] or NULL */);
int gr_covar_clear(gr_covar *cv);
uint64_t gr_covar_frames(const gr_covar *cv);
uint64_t gr_covar_n_atoms(const gr_covar *cv);
int gr_covar_read(gr_covar *cv, double *mean /* [D] */, double *cov /* [D][D] */, uint32_t flags);
int gr_covar_read_raw(gr_covar *cv, float *origin /* [D] */, double *sum /* [D] */, double *Q /* [D][D] */, uint64_t *n);
int gr_covar_read_dccm(gr_covar *cv, double *corr /* [S][S] */);
int gr_covar_merge(gr_covar *dst, gr_covar *src);
int gr_covar_set_launch(gr_covar *cv, uint32_t product_groups, uint32_t check_groups);   /* 0: default; the result never depends on it */
int gr_covar_stat(const gr_covar *cv, int key, uint64_t *value);

/* ---------------------------------------------------------------- MSD: nojump unwrapping and windowed mean-squared displacement
 * The first dynamical analysis (diffusion of lipids, water, ions; gmx msd); the reference has no function for it.  For a snapshot of a
 * group's S atoms (group order, padded with zeros to n_pad, a multiple of 64) the object keeps per atom the ORIGIN o (f32 x3: the
 * position in the first counted frame), w (f32 x3: the position as stored in the last counted frame) and u (f64 x3: the unwrapped
 * position in the last counted frame), and a PANEL X[capacity][3][n_pad] (f32, component-major): row t is frame t's displacement from
 * the origin; components not selected by the flags are stored as zeros (the unwrapping itself is always 3-D).  With it q[t], the sum of
 * the row's squares (f64), and ok[t].  Once appended, a frame's slot may be overwritten: a trajectory longer than the slots is appended
 * block by block.
 * THE RULE, per atom, for one good frame with stored position x and box B:
 *   first counted frame:  o = w = x, u = (double)x
 *   otherwise:            d = x - w, ONE f32 subtraction per component.  With GR_MSD_NOJUMP d is reduced along c, then b, then a:
 *                         k = rint(d * (1/L)) corrected by +-1 where the remainder lies beyond +-L/2, then d = fmaf(-k, box vector, d)
 *                         (the brick reduction of the library's minimum image, no candidate-table refinement; the box is the frame's
 *                         own); u += (double)d, a sequential f64 chain; w = x.  Without NOJUMP u = (double)x.
 *   panel entry:          (float)(u - (double)o), or 0 for a component that is not selected
 * This sums displacements, so it stays correct when the box changes from frame to frame.  A step of half a box edge or more between
 * two counted frames is ambiguous by nature and is taken as the shorter way round.  Removing centre-of-mass drift is the caller's
 * (translate or fit the frames first); the slots are never written.
 * ORDER OF THE SUMS.  A lane owns its atom for a launch and takes the frames in ascending order; nothing is split over frames, no atomic
 * is used: o, w, u, the panel and q are a function of the SEQUENCE of appended frames alone -- not of how they were cut into calls,
 * 1024-frame segments or grids.  gr_msd_compute forms G = X X^T on the f64 matrix cores (f32 operands widened: exact products, f64
 * sums) for the 64 x 64 blocks of frame pairs on and above the diagonal that touch the band t' - t <= max_lag; an entry belongs to one
 * wave and is one chain over the 3 n_pad values of its rows in ascending trips: its bits depend on its two rows and n_pad alone.
 * D2(t, t') = q_t + q_t' - 2 G(t, t') for t < t' (f64 is required: after a long walk q_t is t times larger than D2(t, t + 1));
 * D2(t, t) IS DEFINED AS 0, so msd[0] is exactly 0.  The entries of one diagonal of a block are added in ascending row order, the blocks'
 * partial sums of a lag in ascending block-row order; no atomic decides a sum.  So sum[tau] is a function of the panel alone, the same
 * bits for every max_lag >= tau, grid and context.  Per pair |D2 - exact| <= (2 K + 4) 2^-53 (q_t + q_t'), K = 3 n_pad.
 * NOT promised: the bits of G, and so of the sums, on another device generation or for another n_pad -- the four values one matrix
 * instruction adds are added in an order the hardware does not document (tests pin that equal rows give equal entries wherever they lie) --
 * and more than the bound above against a direct evaluation of sum |d_t - d_t'|^2.
 *   gr_msd_create             snapshots the group's atoms.  flags: at least one of GR_MSD_X | GR_MSD_Y | GR_MSD_Z (XY: the lateral MSD of
 *                             a membrane), optionally GR_MSD_NOJUMP; anything else, capacity 0, or capacity x 3 x n_pad x 4 B above
 *                             GR_MSD_MAX_PANEL_BYTES: GR_E_INVALID_ARG.  GR_E_GROUP_NOT_FOUND, GR_E_EMPTY_GROUP; GR_E_HIP when the allocation fails.
 *   gr_msd_append_batch       appends the n_frames slots from first_slot as time indices frames() .. frames() + n_frames - 1.  Frame
 *                             handling is Fluctuations': a frame in which an atom of the snapshot has no position fails with
 *                             GR_E_NO_POSITION (gr_last_error_index = the lowest such atom); with NOJUMP a frame without a (usable) box
 *                             fails with the box error.  A FAILED FRAME STILL TAKES A TIME INDEX: its row is zeros, its ok 0, it enters
 *                             no pair; the walk skips it and the next good frame is unwrapped against the last good one.  Batch rules:
 *                             status_out[f] is each frame's status, the return value, message and index are the first failed frame's,
 *                             a hard error writes nothing.  Beyond the capacity: GR_E_INVALID_ARG, nothing is changed.
 *   gr_msd_compute            the band up to max_lag (a max_lag beyond frames() - 1 is CLAMPED to it); no frame appended: GR_E_INVALID_ARG
 *   gr_msd_read               msd[tau] = sum[tau] / (pairs[tau] * S), tau = 0 .. the computed max_lag (GR_MSD_STAT_LAGS values), closed in
 *                             f64; NaN where pairs[tau] == 0; pairs[tau] counts the t with ok[t] and ok[t + tau].  Each may be NULL.
 *                             Before gr_msd_compute, or after an append or clear behind it: GR_E_INVALID_ARG.
 *   gr_msd_read_from_origin   out[t] = q[t] / S for t < frames(): the MSD from the first counted frame; NaN for a failed frame
 *   gr_msd_read_displacements out[nt][S][3] (f32): rows t0 .. t0 + nt - 1 of the panel in group order
 *   gr_msd_frames             time indices taken (failed frames included);  gr_msd_n_atoms;  gr_msd_capacity
 *   gr_msd_clear              forgets every frame (and the origin)
 *   gr_msd_set_launch         test hook: the number of ranges of the walk and a cap on the grid of the product (0: one wave per 64
 *                             atoms / one workgroup per block).  The result never depends on it.
 *   gr_msd_stat               GR_MSD_STAT_*: launches so far, the grids of the last walk and product, the edge of a block in frames, the
 *                             panel values per trip, the blocks of the last compute, its lags, n_pad, the counted frames
 * The object keeps a pointer to its context: destroy it first. */
#define GR_MSD_X 1u
#define GR_MSD_Y 2u
#define GR_MSD_Z 4u
#define GR_MSD_NOJUMP 8u
#define GR_MSD_MAX_PANEL_BYTES 17179869184u      /* 16 GiB of panel at most */
enum { GR_MSD_STAT_LAUNCHES = 1, GR_MSD_STAT_LAST_WALK_GROUPS = 2, GR_MSD_STAT_LAST_GRAM_GROUPS = 3, GR_MSD_STAT_BLOCK_EDGE = 4, GR_MSD_STAT_TRIP_VALUES = 5,
       GR_MSD_STAT_LAST_BLOCKS = 6, GR_MSD_STAT_LAGS = 7, GR_MSD_STAT_N_PAD = 8, GR_MSD_STAT_COUNTED = 9 };
gr_msd *gr_msd_create(gr_ctx *ctx, const char *group, uint32_t capacity_frames, uint32_t flags, int *status);
void gr_msd_destroy(gr_msd *m);
int gr_msd_append_batch(gr_msd *m, uint32_t first_slot, uint32_t n_frames, int *status_out /* [n_frames] or NULL */);
int gr_msd_clear(gr_msd *m);
uint64_t gr_msd_frames(const gr_msd *m);
uint64_t gr_msd_n_atoms(const gr_msd *m);
uint64_t gr_msd_capacity(const gr_msd *m);
int gr_msd_compute(gr_msd *m, uint32_t max_lag);
int gr_msd_read(gr_msd *m, double *msd /* [lags] */, uint64_t *pairs /* [lags] */);
int gr_msd_read_from_origin(gr_msd *m, double *out /* [frames] */);
int gr_msd_read_displacements(gr_msd *m, uint32_t t0, uint32_t nt, float *out /* [nt][S][3] */);
int gr_msd_set_launch(gr_msd *m, uint32_t walk_groups, uint32_t gram_groups);   /* 0: default; the result never depends on it */
int gr_msd_stat(const gr_msd *m, int key, uint64_t *value);

/* ---------------------------------------------------------------- Internals: distance, angle and dihedral series over resident frames
 * "What is this bond length, this angle or this torsion in every frame?" -- Ramachandran maps, side-chain chi angles, distance and angle
 * series between picked atoms, lipid order parameters.  The reference has Vector3D::angle (vector3d.rs:276-278) and distance only: no
 * dihedral and no per-tuple series.  The object holds a fixed list of T atom tuples of one kind and gives, for a block of resident frames,
 * either the value of every tuple in every frame (values) or running per-tuple statistics over any number of calls (accumulate: mean and
 * variance, which for the axis kind is the order parameter) without storing the series.
 * DEFINITIONS.  Displacement d(a->b) = x_b - x_a, one f32 subtraction per component.  With the flag GR_IC_PBC it is followed by
 * gr_min_image_vec with the frame's own box (orthorhombic and triclinic).  Without the flag the raw difference stands and a frame needs no
 * box.  Angles are in RADIANS, as Vector3D::angle gives them.
 *   GR_IC_DISTANCE  (i, j)                     gr_mag3(d(i->j)), nm
 *   GR_IC_ANGLE     (i, j, k), vertex j        u = d(j->i), v = d(j->k): atan2f(|u x v|, u.v) in [0, pi]
 *   GR_IC_DIHEDRAL  (i, j, k, l)               b1 = d(i->j), b2 = d(j->k), b3 = d(k->l), n1 = b1 x b2, n2 = b2 x b3:
 *                                              atan2f(|b2| (b1.n2), n1.n2) in [-pi, pi]
 *   GR_IC_AXIS      (i, j) + a unit vector a   cos theta = (d(i->j).a) / |d(i->j)|; 0 when |d| = 0
 * THE PINS of the dihedral's sign, with i = (0,1,0), j = (0,0,0), k = (1,0,0): l = (1,0,1) gives +pi/2, l = (1,1,0) gives 0 (cis),
 * l = (1,-1,0) gives pi (trans), l = (1,0,-1) gives -pi/2 (the IUPAC sign, as gmx angle and MDAnalysis have it).  The formula and the
 * pins are the definition.  atan2f instead of the reference's acos(dot / (|u||v|)): it stays well conditioned near 0 and pi; the
 * reference's known answers for `angle` come out within 4 ulp(pi).  Every product and sum of these formulas is rounded on its own.
 * Degenerate geometry never produces NaN: coincident atoms give atan2f(0, 0) = 0, a collinear dihedral some finite value in [-pi, pi].
 * STATISTICS.  Per tuple the object keeps an ORIGIN o (f32): the tuple's value in the first frame the object ever counted; and in f64
 * s = sum d and q = sum d * d with d = v - o, ONE f32 subtraction.  THE DIHEDRAL'S WRAP RULE: for GR_IC_DIHEDRAL only, d is reduced once
 * in f32 with PI_F = (float)M_PI: if d > PI_F, subtract 2 PI_F; else if d < -PI_F, add 2 PI_F.  A torsion that oscillates across +-pi
 * therefore has a small variance and a mean near +-pi; THIS HOLDS WHILE THE DISTRIBUTION STAYS WITHIN pi OF THE ORIGIN.
 * ORDER OF THE SUMS.  A lane owns its tuple for a launch and adds the frames in ascending order, one after another, as a single f64
 * chain; nothing is split over frames and no atomic touches a sum.  v in accumulate is the same bits values gives for that frame and
 * tuple.  So o, s, q are a function of the SEQUENCE of counted frames alone -- not of how they were cut into calls, 1024-frame segments
 * or grids -- and tests/internals_ref.py restates them from the rows values returns (f32 subtract, f32 wrap, f64 cumulative add in frame
 * order), bit for bit.
 *   gr_internals_create              atoms: [T][arity] row-major (arity 2, 3, 4, 2), copied.  flags: GR_IC_PBC or 0.  axis: [3] for
 *                                    GR_IC_AXIS (normalised on the host in f64, then rounded to f32), else NULL.  An atom index >= n_atoms:
 *                                    GR_E_OUT_OF_RANGE + gr_last_error_index = that index.  GR_E_INVALID_ARG: an unknown kind or flag,
 *                                    T = 0, an atom that appears twice in one tuple (gr_last_error_index = the tuple); for GR_IC_AXIS a
 *                                    NULL, zero or non-finite axis.  The host keeps the sorted list of unique atoms the tuples name.
 *   gr_internals_count               T;  gr_internals_frames: frames counted by accumulate
 *   gr_internals_values_batch        out[f][t] (host, [n_frames][T]) for the n_frames slots from first_slot.  Per frame: with GR_IC_PBC the
 *                                    box checks (GR_E_NO_BOX / the slot's box status / GR_E_NOT_ORTHOGONAL in strict mode), then a frame in
 *                                    which any atom named by any tuple has no position fails with GR_E_NO_POSITION, gr_last_error_index =
 *                                    the lowest such atom; an atom without position that no tuple names fails nothing.  A FAILED FRAME IS
 *                                    A ROW OF NaN, the other rows are untouched by it.  Batch rules: status_out[f] is each frame's status,
 *                                    the return value, message and index are the first failed frame's, a hard error writes nothing.
 *                                    The device variant runs into a grow-only workspace of at most GR_IC_MAX_WS_BYTES per piece of a
 *                                    segment; no result depends on the piece.
 *   gr_internals_values_batch_device the same into device memory of the context's device: row f starts f * ld floats in, ld >= T (else
 *                                    GR_E_INVALID_ARG); the floats of a row beyond T are not written
 *   gr_internals_accumulate_batch    counts the frames; a failed frame (as above) is counted for NO tuple; when the first frame fails the
 *                                    origin comes from the first frame that is counted.  Nothing is stored per frame.
 *   gr_internals_clear               forgets every frame (and the origin)
 *   gr_internals_read                closes on the host in f64: mean = o + s / n, var = max(q - s^2 / n, 0) / n; a dihedral's mean is
 *                                    brought back into (-pi, pi].  Each may be NULL.  n = 0: GR_E_INVALID_ARG.
 *   gr_internals_read_raw            o, s, q as they stand ([T] each) and n; each may be NULL
 *   gr_internals_merge               adds src's frames to dst after moving its sums to dst's origin in f64, delta = o_src - o_dst (a
 *                                    dihedral's delta is wrapped into (-pi, pi]): s += s_src + n_src delta, q += q_src + 2 delta s_src +
 *                                    n_src delta^2.  An empty src changes nothing, an empty dst takes src's state as it is.
 *                                    GR_E_INCONSISTENT_GROUP if kind, flags, axis, T or the tuples differ; dst == src: GR_E_INVALID_ARG.
 *                                    AFTER A MERGE THE SUMS ARE NO LONGER THOSE OF ONE WALK.
 *   gr_internals_set_launch          test hook: the ranges the tuples are cut into (one wave each; 0: one per 64 tuples) and the frames
 *                                    of one workgroup of values (0: chosen from T and the number of frames).  No result depends on it.
 *   gr_internals_stat                GR_IC_STAT_*: launches so far, the grids of the last launch (tuple ranges, frame chunks, position
 *                                    check), the arity, the unique atoms, the frames a lane has in flight
 * The object keeps a pointer to its context: destroy it first. */
#define GR_IC_PBC 1u
#define GR_IC_MAX_WS_BYTES (64u << 20)     /* the device workspace of gr_internals_values_batch at most: 64 MiB */
enum { GR_IC_DISTANCE = 1, GR_IC_ANGLE = 2, GR_IC_DIHEDRAL = 3, GR_IC_AXIS = 4 };
enum { GR_IC_STAT_LAUNCHES = 1, GR_IC_STAT_LAST_RANGE_GROUPS = 2, GR_IC_STAT_LAST_FRAME_GROUPS = 3, GR_IC_STAT_LAST_CHECK_GROUPS = 4, GR_IC_STAT_ARITY = 5,
       GR_IC_STAT_UNIQUE_ATOMS = 6, GR_IC_STAT_AHEAD = 7 };
gr_internals *gr_internals_create(gr_ctx *ctx, int kind, const uint64_t *atoms /* [T][arity], row-major */, uint64_t n_tuples,
                                  uint32_t flags /* GR_IC_PBC */, const float *axis /* [3], GR_IC_AXIS only, else NULL */, int *status);
void gr_internals_destroy(gr_internals *ic);
uint64_t gr_internals_count(const gr_internals *ic);          /* T */
uint64_t gr_internals_frames(const gr_internals *ic);         /* frames counted by accumulate */
int gr_internals_values_batch(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, float *out /* host [n_frames][T] */, int *status_out);
int gr_internals_values_batch_device(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, float *out_dev, uint64_t ld /* floats per row, >= T */, int *status_out);
int gr_internals_accumulate_batch(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, int *status_out);
int gr_internals_clear(gr_internals *ic);
int gr_internals_read(gr_internals *ic, double *mean /* [T] */, double *var /* [T] */);
int gr_internals_read_raw(gr_internals *ic, float *origin /* [T] */, double *sum /* [T] */, double *sumsq /* [T] */, uint64_t *n);
int gr_internals_merge(gr_internals *dst, gr_internals *src);
int gr_internals_set_launch(gr_internals *ic, uint32_t tuple_ranges, uint32_t frame_chunk);   /* test hook, 0: default; no result depends on it */
int gr_internals_stat(const gr_internals *ic, int key, uint64_t *value);

/* ---------------------------------------------------------------- VectorCorrelation: P1/P2 reorientation curves over resident frames
 * The rotational counterpart of MSD (gmx rotacf): C1(tau) = <u(t) . u(t + tau)> and C2(tau) = <P2(u(t) . u(t + tau))>, P2(x) =
 * (3 x^2 - 1) / 2, of a fixed list of V bond vectors (i, j) -- water reorientation, lipid dynamics, NMR relaxation and the Lipari-Szabo
 * S^2 of every N-H bond; the reference has no function for it.  The object keeps up to two PANELS (f32, component-major, V padded with
 * zeros to n_pad, a multiple of 64) that outlive the slots: X1[capacity][3][n_pad] holds u, X2[capacity][6][n_pad] holds u_x u_x,
 * u_y u_y, u_z u_z, SQRT2_F (u_x u_y), SQRT2_F (u_x u_z), SQRT2_F (u_y u_z) with SQRT2_F = (float)M_SQRT2 -- for unit vectors
 * (u . u')^2 = sum_ab (u_a u_b)(u'_a u'_b), so C2 is a Gram product like C1.  With them ok[t].
 * THE RULE, per good frame and vector, every product and sum rounded on its own, no contraction:
 *   d = x_j - x_i          ONE f32 subtraction per component; with GR_VCORR_PBC followed by the library's minimum image (triclinic
 *                          boxes included) with the frame's own box
 *   with GR_VCORR_UNIT:    len = sqrtf((d_x d_x + d_y d_y) + d_z d_z), correctly rounded; inv = 1.0f / len; u_c = d_c * inv.
 *                          u = 0 WHEN len = 0: such a vector adds nothing to a sum but STILL COUNTS IN THE DENOMINATOR
 *   without UNIT:          u = d
 * ORDER OF THE SUMS.  A lane owns its vector for a launch and takes the frames in ascending order: the panels are a function of the
 * SEQUENCE of appended frames alone -- not of calls, 1024-frame segments or grids.  gr_vcorr_compute forms S[tau] = sum_t sum_k
 * X_t . X_(t + tau) over valid pairs as a banded Gram product G = X X^T on the f64 matrix cores (f32 operands widened: exact products,
 * f64 sums) over the 64 x 64 blocks of frame pairs on and above the diagonal that touch the band; an entry is one chain of one wave over
 * the K = 3 n_pad (6 n_pad) values of its rows; the diagonal t = t' is a valid pair (lag 0).  The entries of one diagonal of a block are
 * added in ascending row order, the blocks' partial sums of a lag in ascending block-row order; no atomic decides a sum.  So S[tau] is a
 * function of the panel alone, the same bits for every max_lag >= tau, grid and context.  gr_vcorr_compute_each closes every
 * (vector, lag) as ONE sequential f64 chain: frames ascending, within a frame the components in panel order, each term
 * fma((double)a, (double)b, s).
 * NOT promised: the bits of S on another device generation or for another n_pad (the four values one matrix instruction adds are
 * added in an order the hardware does not document); C1[0] = C2[0] = 1 exactly (a stored unit vector has |u|^2 = 1 within f32
 * rounding).  Out of scope: cross-correlation between two lists, an FFT closing, a merge of objects (time order makes shards
 * meaningless), S^2 fits and the plateau, normals of three atoms, velocities.
 *   gr_vcorr_create        atoms: [V][2] row-major, copied.  flags: at least one of GR_VCORR_P1 | GR_VCORR_P2 (the panels to keep),
 *                          optionally GR_VCORR_PBC, GR_VCORR_UNIT; P2 without UNIT, anything else, V = 0, capacity 0, i == j
 *                          (gr_last_error_index = the pair), or kept panels above GR_MSD_MAX_PANEL_BYTES: GR_E_INVALID_ARG.  An atom
 *                          index >= n_atoms: GR_E_OUT_OF_RANGE (gr_last_error_index = the index).  GR_E_HIP when the allocation fails.
 *   gr_vcorr_append_batch  appends the n_frames slots from first_slot as time indices frames() .. frames() + n_frames - 1.  Per frame:
 *                          with PBC the box checks come first; a frame in which an atom named by any pair has no position fails with
 *                          GR_E_NO_POSITION (gr_last_error_index = the lowest such atom).  A FAILED FRAME STILL TAKES A TIME INDEX: its
 *                          rows are zeros, its ok 0, it enters no pair.  Batch rules: status_out[f] is each frame's status, the return
 *                          value, message and index are the first failed frame's, a hard error writes nothing.  Beyond the capacity:
 *                          GR_E_INVALID_ARG, nothing is changed.  The slots may be overwritten as soon as the call returns.
 *   gr_vcorr_compute       the band up to max_lag (a max_lag beyond frames() - 1 is CLAMPED to it); no frame appended: GR_E_INVALID_ARG
 *   gr_vcorr_read          closed in f64 on the host: c1[tau] = S1 / (pairs[tau] * V), c2[tau] = 1.5 S2 / (pairs[tau] * V) - 0.5, NaN
 *                          where pairs[tau] == 0; pairs[tau] counts the t with ok[t] and ok[t + tau].  GR_VCORR_STAT_LAGS values each;
 *                          each may be NULL; a curve whose panel is not kept, a read before gr_vcorr_compute or after an append or
 *                          clear behind it: GR_E_INVALID_ARG
 *   gr_vcorr_compute_each  c1_out, c2_out: [V][lags] (host, f64), the curve of every vector: s / pairs[tau] and 1.5 s / pairs[tau] -
 *                          0.5.  Each may be NULL, not both; a curve whose panel is not kept, or V x lags x 8 B above
 *                          GR_VCORR_MAX_EACH_BYTES: GR_E_INVALID_ARG
 *   gr_vcorr_read_vectors  out[nt][V][3] (f32): rows t0 .. t0 + nt - 1 of the rank-1 panel in the caller's order (needs GR_VCORR_P1)
 *   gr_vcorr_count         V;  gr_vcorr_frames: time indices taken (failed frames included);  gr_vcorr_capacity
 *   gr_vcorr_clear         forgets every frame
 *   gr_vcorr_set_launch    test hook: the ranges of the walk, a cap on the grid of the product and on the grid of compute_each (0: the
 *                          default).  No result depends on it.
 *   gr_vcorr_stat          GR_VCORR_STAT_*: launches so far, n_pad, the lags of the last compute, the grids of the last walk, product
 *                          and compute_each, the blocks of the last compute, the counted frames
 * The object keeps a pointer to its context: destroy it first. */
#define GR_VCORR_PBC 1u
#define GR_VCORR_UNIT 2u
#define GR_VCORR_P1 4u
#define GR_VCORR_P2 8u
#define GR_VCORR_MAX_EACH_BYTES 1073741824u      /* 1 GiB per curve of gr_vcorr_compute_each at most */
enum { GR_VCORR_STAT_LAUNCHES = 1, GR_VCORR_STAT_N_PAD = 2, GR_VCORR_STAT_LAGS = 3, GR_VCORR_STAT_LAST_WALK_GROUPS = 4, GR_VCORR_STAT_LAST_GRAM_GROUPS = 5,
       GR_VCORR_STAT_LAST_EACH_GROUPS = 6, GR_VCORR_STAT_LAST_BLOCKS = 7, GR_VCORR_STAT_COUNTED = 8 };
gr_vcorr *gr_vcorr_create(gr_ctx *ctx, const uint64_t *atoms /* [V][2], row-major */, uint64_t n_vectors, uint32_t capacity_frames, uint32_t flags, int *status);
void gr_vcorr_destroy(gr_vcorr *vc);
uint64_t gr_vcorr_count(const gr_vcorr *vc);
uint64_t gr_vcorr_frames(const gr_vcorr *vc);
uint64_t gr_vcorr_capacity(const gr_vcorr *vc);
int gr_vcorr_append_batch(gr_vcorr *vc, uint32_t first_slot, uint32_t n_frames, int *status_out /* [n_frames] or NULL */);
int gr_vcorr_clear(gr_vcorr *vc);
int gr_vcorr_compute(gr_vcorr *vc, uint32_t max_lag);
int gr_vcorr_read(gr_vcorr *vc, double *c1 /* [lags] */, double *c2 /* [lags] */, uint64_t *pairs /* [lags] */);
int gr_vcorr_compute_each(gr_vcorr *vc, uint32_t max_lag, double *c1_out /* [V][lags] */, double *c2_out /* [V][lags] */);
int gr_vcorr_read_vectors(gr_vcorr *vc, uint32_t t0, uint32_t nt, float *out /* [nt][V][3] */);
int gr_vcorr_set_launch(gr_vcorr *vc, uint32_t walk_groups, uint32_t gram_groups, uint32_t each_groups);   /* test hook, 0: default; no result depends on it */
int gr_vcorr_stat(const gr_vcorr *vc, int key, uint64_t *value);

/* ---------------------------------------------------------------- xtc reader (host side)
 * The stage in front of the path: XtcReader (src/io/xtc_io/mod.rs, molly_xtc.rs:96-308, xdrfile_xtc.rs:42-104).
 * gr_xtc_open indexes the file (frame offsets, steps, times, boxes) so frames are random-access -- what the
 * reference's with_range / with_step / per-thread skipping (traj_read.rs:215-246, parallel.rs:424-448) need -- and
 * gr_xtc_read_frame is thread-safe: one frame per host thread, decoded straight into the caller's buffer
 * (pinned memory from gr_host_alloc feeds gr_frame_upload without another copy).
 * step is the u32-wrapped simulation step (xdrfile_xtc.rs:98-100); box9 in gro order (xdrfile.rs:170-187). */
gr_xtc *gr_xtc_open(const char *path, int *status);
void gr_xtc_close(gr_xtc *xtc);
uint64_t gr_xtc_n_atoms(const gr_xtc *xtc);
uint64_t gr_xtc_n_frames(const gr_xtc *xtc);
int gr_xtc_frame_info(const gr_xtc *xtc, uint64_t frame, uint64_t *step, float *time, float box9[9], float *precision);
int gr_xtc_read_frame(const gr_xtc *xtc, uint64_t frame, float *xyz, float box9[9], uint64_t *step, float *time, float *precision);
/* The same for a batch, unpacked ON THE DEVICE: frames first_frame, first_frame + frame_step, ... (n_frames of them) land
 * in slots first_slot .. first_slot + n_frames - 1 of `ctx` with their boxes, like n gr_frame_upload calls -- but what
 * crosses PCIe is the compressed bit stream (~3.5 B/atom instead of 12) and the host only skims the group framing
 * (`host_threads` workers, 0 = one per frame up to 16), the unpacking of all frames runs as one kernel on the copy stream.
 * Asynchronous like gr_frame_upload (kernels that use the slots are ordered behind it; gr_frame_upload_wait to block).
 * Results are bit-identical to gr_xtc_read_frame.  steps / times may be NULL. */
int gr_xtc_read_frames_device(const gr_xtc *xtc, uint64_t first_frame, uint32_t n_frames, uint64_t frame_step, gr_ctx *ctx,
                              uint32_t first_slot, int host_threads, uint64_t *steps, float *times);

/* ---------------------------------------------------------------- frame-sharded map-reduce over several GPUs
 * System::traj_iter_map_reduce (src/system/parallel.rs:208-481): frames are independent units; worker w of T takes frames
 * w, w + T, ... (parallel.rs:424-448); every worker owns a clone of the System; a shared error flag, polled every 10 frames,
 * stops the others when one fails (parallel.rs:28,453-475) and the call as a whole fails (:288-321); the per-worker results
 * are merged at the end (ParallelTrajData::reduce, :31-49).  Bulk frame data never crosses GPUs: no data-path collective.
 *
 * In-process form (one host process, several GPUs or several workers per GPU): gr_pool_create makes one context per entry of
 * `devices` (System::clone per worker) -- set masses / groups / plans on them through gr_pool_ctx.  gr_pool_map runs `body`
 * for frames 0 .. n_frames - 1 on the workers' own threads (worker w: frames w, w + T, ...); the body loads its frame into its
 * context (gr_frame_upload, gr_xtc_read_frames_device ...: the xtc / trr handles are thread-safe), analyses it and writes
 * `width` floats to `result`, which IS the frame's row of `results` -- the order is restored by construction, the gather is
 * host memory.  A non-zero return is the frame's error: the first one wins, becomes the return value of gr_pool_map
 * (*error_frame = its frame), and the other workers stop at their next flag check; *frames_done counts completed frames. */
typedef struct gr_pool gr_pool;
typedef int (*gr_pool_body)(gr_ctx *ctx, int worker, uint64_t frame, void *user, float *result);
gr_pool *gr_pool_create(const int *devices, int n_workers, uint64_t n_atoms, uint32_t n_slots, int *status);
void gr_pool_destroy(gr_pool *pool);
int gr_pool_size(const gr_pool *pool);
gr_ctx *gr_pool_ctx(gr_pool *pool, int worker);
const char *gr_pool_last_error(const gr_pool *pool);
int gr_pool_map(gr_pool *pool, uint64_t n_frames, gr_pool_body body, void *user, size_t width, float *results,
                uint64_t *frames_done, uint64_t *error_frame);
/* The same with the reference's range / step arguments and its progress printer (traj_iter_map_reduce's start_time, end_time, step,
 * progress_printer, parallel.rs:208-222; frame-index form: a reader's index turns times into frame numbers, gr_xtc_frame_info):
 * the frames visited are first_frame + k * step for k = 0, 1, ... while < end_frame; worker w of T takes k = w, w + T, ... -- it skips
 * w * step frames and then advances by step * T, exactly parallel.rs:425-448 -- and `result` is row k of `results` (rows in visiting
 * order, ceil((end_frame - first_frame) / step) of them).  `body` receives the FRAME number.  `progress` (may be NULL) is the
 * ProgressPrinter: called on worker 0's thread after every frame that worker completes (GR_PROGRESS_RUNNING; the reference
 * attaches the printer to the master thread's iterator only, parallel.rs:417-422) and once after all workers have joined with
 * GR_PROGRESS_COMPLETED and the last frame any worker read, or GR_PROGRESS_FAILED and the frame that failed (:288-321).
 * step = 0 is GR_E_INVALID_ARG (the reference's ReadTrajError::InvalidStep). */
enum { GR_PROGRESS_RUNNING = 0, GR_PROGRESS_COMPLETED = 1, GR_PROGRESS_FAILED = 2 };
typedef void (*gr_pool_progress)(void *progress_user, int status, uint64_t frame, uint64_t frames_done);
int gr_pool_map_range(gr_pool *pool, uint64_t first_frame, uint64_t end_frame, uint64_t step, gr_pool_body body, void *user,
                      size_t width, float *results, gr_pool_progress progress, void *progress_user,
                      uint64_t *frames_done, uint64_t *error_frame);
/* Multi-process form (one process per GPU, e.g. under torchrun / mpirun): an RCCL communicator over xGMI for the two exchanges
 * the path has -- the final gather of the per-frame results and the shared error flag.  Rank 0 calls gr_comm_unique_id and
 * hands the 128 bytes to every rank by whatever the launcher offers (a file, MPI_Bcast, torch.distributed ...); every rank
 * then calls gr_comm_create (collective).  gr_comm_gather_per_frame: `local` holds this rank's frames rank, rank + G, ...
 * ([n_local][width], host memory); every rank receives all n_total rows in frame order (out[f] = shard[f mod G][f div G]): ONE
 * ncclAllGather of ceil(n_total / G) x width floats per rank.  gr_comm_any_error: 1-int ncclAllReduce(MAX) of the flag.
 * RCCL is resolved at run time (gr_comm_library says from where); without it these calls return GR_E_NO_DEVICE. */
typedef struct gr_comm gr_comm;
int gr_comm_unique_id(void *id128);
gr_comm *gr_comm_create(int device, int rank, int world, const void *id128, int *status);
void gr_comm_destroy(gr_comm *comm);
const char *gr_comm_last_error(const gr_comm *comm);
const char *gr_comm_library(void);
/* use this RCCL build instead of the default search (the process's own copy, then librccl.so.1); call before the first gr_comm_* call
 * of the process -- the library is resolved once, and a call that comes after that returns GR_E_INVALID_ARG (thread-safe against a
 * concurrent first gr_comm_* call).  A path that cannot be loaded makes every gr_comm_* call return GR_E_NO_DEVICE and
 * gr_comm_library() say why. */
int gr_comm_set_library(const char *path);
int gr_comm_gather_per_frame(gr_comm *comm, const float *local, uint64_t n_total, size_t width, float *out);
int gr_comm_any_error(gr_comm *comm, int local_flag, int *any);
/* the host half of the gather on its own (no device, no RCCL): `gathered` = G shards of ceil(n_total / G) rows -> frame order */
void gr_shard_deinterleave(const float *gathered, int world, uint64_t n_total, size_t width, float *out);

/* Partial-frame reading = GroupXtcReader / System::group_xtc_iter (src/io/xtc_io/molly_xtc.rs:475-620 over the molly crate):
 * only the atoms of a group change, "all other atoms are left unchanged", the frame's box / step / time are set as usual.  The
 * bit stream is sequential, so everything UP TO the group's last atom is walked -- and nothing behind it: for a group near the
 * start of the structure (a peptide in front of its membrane and water) that is a small fraction of the frame.
 *   gr_xtc_read_frame_prefix        host decode of the first n_prefix atoms (= last atom of the group + 1) into xyz[n_prefix][3];
 *                                   reads only the needed prefix of the frame's stream (*stream_bytes_read, may be NULL)
 *   gr_xtc_read_frames_device_group like gr_xtc_read_frames_device, but the host reads + skims only up to the group's last atom,
 *                                   only that prefix crosses PCIe, and the unpack kernel writes the group's atoms only
 * Both are bit-identical to the full decode on the atoms they deliver. */
int gr_xtc_read_frame_prefix(const gr_xtc *xtc, uint64_t frame, uint64_t n_prefix, float *xyz, float box9[9], uint64_t *step, float *time, float *precision,
                             uint64_t *stream_bytes_read);
int gr_xtc_read_frames_device_group(const gr_xtc *xtc, uint64_t first_frame, uint32_t n_frames, uint64_t frame_step, gr_ctx *ctx,
                                    uint32_t first_slot, const char *group, int host_threads, uint64_t *steps, float *times);

/* ---------------------------------------------------------------- measurement / synthetic data
 * HIP-event timing on the context's stream (the stream the kernels are launched on). */
int gr_timer_start(gr_ctx *ctx);
int gr_timer_stop(gr_ctx *ctx, float *milliseconds);
/* Per-kernel HIP-event profile of the batched RMSD path, recorded on the context's stream around
 * each launch while enabled: kernel 0 = sums pass (k_sums_pk / k_rmsd_accum), 1 = k_rmsd_finalize (separate launch only), 2 = fit pass (k_fit_pk), 3 = the resident single pass (k_fit_resident).  Enabling resets
 * the counters.  ms_total / launches = average launch duration; frames = frames those launches covered. */
int gr_profile_enable(gr_ctx *ctx, int on);
int gr_profile_read(const gr_ctx *ctx, int kernel, double *ms_total, uint64_t *launches, uint64_t *frames);
/* Seeded synthetic workload of SURVEY.md section 8(d), generated directly in HBM:
 *  gr_synth_reference: n_atoms points uniform in a ball of `radius` about the box centre -> slot
 *  gr_synth_frames   : frame f = R_f (x0 - c) + c + t_f + noise, wrapped into the cell, for
 *                      n_frames consecutive slots; R_f, t_f, noise from a counter-based hash of
 *                      (seed, first_frame_index + f*frame_index_stride, atom): a rank of a G-way
 *                      round-robin shard passes (rank, G).  Every slot inherits the reference slot's box.
 *  gr_synth_uniform  : n_atoms points uniform in the unit cell (config 3). */
int gr_synth_reference(gr_ctx *ctx, uint32_t slot, const float *box9, float radius, uint64_t seed);
int gr_synth_frames(gr_ctx *ctx, uint32_t ref_slot, uint32_t first_slot, uint32_t n_frames,
                    uint64_t first_frame_index, uint64_t frame_index_stride, float noise_sigma, uint64_t seed);
int gr_synth_uniform(gr_ctx *ctx, uint32_t slot, const float *box9, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* GROAN_HIP_H */

// gr_rmsd_panel.h -- RMSDPanel: the all-pairs RMSD matrix over packed frames.
//
// Reference: a double loop of System::calc_rmsd(&other, group) (src/system/rmsd.rs:75-166).  Each side of calc_rmsd is prepared without
// its partner: extract_data_from_system (:425-446) takes get_com, shifts by box centre - com and wraps, kabsch_rmsd (:547-603) subtracts
// the box centre.  So a frame has ONE centred coordinate set X_f (N x 3), and a pair (p = reference, q = current) needs
//   H  = sum p q^T               (unweighted, :567-570)  -> the rotation R (gr_best_rotation)
//   Hw = sum w p q^T,  G_f = sum w |x_f|^2               -> rmsd^2 = (G_p + G_q - 2 sum_ab R_ab Hw_ab) / W      (= :592-599 expanded)
// A PANEL keeps X_f (f32, component-major, atoms zero-padded to GR_RP_KSTEP) and G_f (f64) of the frames appended to it; the slots they
// came from may be overwritten at once.  The matrix of two panels is the dense product C = A B^T (A: six rows per row frame -- x, y, z,
// w x, w y, w z, the weighting applied in registers --, B: three rows per column frame) on v_mfma_f64_16x16x4_f64, closed per pair in
// the same kernel:
//   k_rp_pack    one workgroup per appended frame, behind the library's centre stages (pbc_center_stages: get_com): q = wrap(x + shift)
//                - box centre with gr_flush4<1>'s expressions, G_f by a fixed-order block sum; a failed frame's row is zeros, marked invalid
//   k_rp_matrix  one workgroup (4 waves) per 48 x 48 block of C = 8 row frames x 16 column frames.  Wave v takes the 16-atom groups
//                v, v + 4, ... in ascending order: a lane loads one float4 per operand row (atoms 16 g + 4 (lane >> 4) + j, j = 0..3; lane
//                & 15 = the row / column of the tile) and issues 4 x 9 MFMAs, k-step j taking element j of every lane.  The four
//                waves' tiles are added in LDS in wave order, then 128 lanes close one pair each and store one f32.
// Sums are f64 and every product entering them is exact (f32 x f32, and (w x) y inside the fused multiply-add), their order depends on N
// alone, and no atomic touches them: swapping the two frames of a pair TRANSPOSES H and Hw bit for bit.  The closing lane then puts
// the pair into a canonical orientation (the lexicographically smaller of (H, Hw) and its transpose), so an entry is a symmetric
// function of its two frames and of N -- whatever their places in the panels, the neighbours in the block or the run.
#pragma once
#include "gr_series.h"

#if defined(__HIPCC__)

#define GR_RP_KSTEP 16u                          /* atoms per trip of a wave; rows are padded to it */
#define GR_RP_ROW_FRAMES 8u                      /* row frames of a block (48 rows of C) */
#define GR_RP_COL_FRAMES 16u                     /* column frames of a block (48 columns of C) */
#define GR_RP_LD 49u                             /* leading dimension of the block in LDS (doubles) */
#define GR_RP_MAX_FRAMES (1u << 20)              /* capacity of a panel, at most */
#define GR_RP_MAX_DEVICE_ENTRIES (1ull << 28)    /* n_rows x n_cols of gr_rmsd_matrix_device, at most (1 GiB of f32) */
#define GR_RP_BLOCK_ENTRIES (1ull << 26)         /* entries of one column block of gr_rmsd_matrix */

struct gr_rmsd_panel {
    gr_ctx *c = nullptr;
    std::string group;
    uint32_t n = 0, n_pad = 0, capacity = 0, frames = 0;
    // the group's atoms at create, for the centre stages always as an INDEX LIST (the gather form): a group's sums are then added in the
    // order of its ordinals whatever its shape in the system (a scattered group gives the bits of the same atoms laid out contiguously)
    GrSnapshot snap;
    std::vector<float> w_host;                   // their masses
    double W = 0.0;                              // sum of the masses, group order
    uint64_t epoch = 0;                          // context epoch at which the masses were last compared with the snapshot
    grbuf::Dev<uint32_t> ok_dev;                 // [capacity]
    grbuf::Dev<float> w_dev, x;                  // [n_pad], [capacity][3][n_pad]
    grbuf::Dev<double> G;                        // [capacity]
    std::vector<int> status;                     // [frames]
    grbuf::Dev<float> out;                       // the last matrix (or its last column block)
    uint64_t block_entries = 0;                  // 0: GR_RP_BLOCK_ENTRIES
};

typedef double gr_rp_d4 __attribute__((ext_vector_type(4)));

// frame f of the batch -> row f of `x` (the caller passes the panel's next rows)
__global__ __launch_bounds__(GR_WG) void k_rp_pack(const float *__restrict__ frames, size_t stride, uint32_t slot0, const uint32_t *__restrict__ atoms,
                                                   const float *__restrict__ w, uint32_t n, uint32_t n_pad, const GrBox *__restrict__ boxes,
                                                   const GrFrameState *__restrict__ state, float *__restrict__ x, double *__restrict__ G, uint32_t *__restrict__ ok) {
    __shared__ GrBox box;
    __shared__ double lds[GR_WG / 64];
    const uint32_t f = blockIdx.x;
    gr_stage_box(&box, boxes + slot0 + f);
    const bool good = state[f].status == 0;
    const float sx = state[f].shift[0], sy = state[f].shift[1], sz = state[f].shift[2];
    const float *xyz = frames + (size_t)(slot0 + f) * stride;
    float *row = x + (size_t)f * 3u * n_pad;
    double acc[1] = { 0.0 };
    for (uint32_t k = threadIdx.x; k < n_pad; k += GR_WG) {
        float vx = 0.0f, vy = 0.0f, vz = 0.0f;
        if (good && k < n) {
            gr_pos_load(xyz, atoms[k], vx, vy, vz);
            vx += sx; vy += sy; vz += sz;
            gr_wrap(vx, vy, vz, box);
            vx -= box.bcx; vy -= box.bcy; vz -= box.bcz;
            const double dx = vx, dy = vy, dz = vz;
            acc[0] = fma((double)w[k], fma(dx, dx, fma(dy, dy, dz * dz)), acc[0]);
        }
        row[k] = vx; row[(size_t)n_pad + k] = vy; row[2u * (size_t)n_pad + k] = vz;
    }
    gr_block_sum<1>(acc, lds);
    if (threadIdx.x == 0) { G[f] = good ? acc[0] : 0.0; ok[f] = good ? 1u : 0u; }
}

// block (blockIdx.x, blockIdx.y) = row frames 8 x .. 8 x + 7, column frames col0 + 16 y .. col0 + 16 y + 15 (of n_cols from col0);
// out[i * ld + j], j relative to col0.  SYM (the same panel on both sides, all of its columns): entries with i <= j are computed and
// stored at (i, j) and (j, i); a block wholly below the diagonal leaves at once
template <bool SYM>
__global__ __launch_bounds__(256) void k_rp_matrix(const float *__restrict__ xr, const double *__restrict__ Gr, const uint32_t *__restrict__ okr, uint32_t n_rows,
                                                   const float *__restrict__ xc, const double *__restrict__ Gc, const uint32_t *__restrict__ okc, uint32_t col0,
                                                   uint32_t n_cols, const float *__restrict__ w, uint32_t n_pad, double W, float *__restrict__ out, size_t ld) {
    __shared__ double C[48u * GR_RP_LD];
    const uint32_t r0 = blockIdx.x * GR_RP_ROW_FRAMES, c0 = blockIdx.y * GR_RP_COL_FRAMES;
    if (SYM && r0 > c0 + (GR_RP_COL_FRAMES - 1u)) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, m = lane & 15u, kg = lane >> 4;
    const size_t fstride = 3u * (size_t)n_pad;
    // operand rows of this lane: tile t of A holds rows 16 t + m of the block (frame r / 6; component r % 6: x y z wx wy wz), tile t of B
    // columns 16 t + m (frame c / 3, component c % 3).  Frames beyond the panel's last are read as the last (never closed).
    auto row_of = [&](uint32_t t) {
        const uint32_t r = 16u * t + m, rf = min(r0 + r / 6u, n_rows - 1u);
        return xr + (size_t)rf * fstride + (size_t)(r % 3u) * n_pad + 4u * kg;         // (r % 6) % 3 == r % 3
    };
    auto col_of = [&](uint32_t t) {
        const uint32_t r = 16u * t + m, cf = col0 + min(c0 + r / 3u, n_cols - 1u);
        return xc + (size_t)cf * fstride + (size_t)(r % 3u) * n_pad + 4u * kg;
    };
    const float *const pa[3] = { row_of(0u), row_of(1u), row_of(2u) }, *const pb[3] = { col_of(0u), col_of(1u), col_of(2u) };
    const bool wt[3] = { m % 6u >= 3u, (16u + m) % 6u >= 3u, (32u + m) % 6u >= 3u };
    const float *pw = w + 4u * kg;
    gr_rp_d4 acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[a][b] = (gr_rp_d4){ 0.0, 0.0, 0.0, 0.0 };
    const uint32_t ng = n_pad / GR_RP_KSTEP;
    for (uint32_t g = wave; g < ng; g += 4u) {
        const size_t off = (size_t)g * GR_RP_KSTEP;
        float4 a4[3], b4[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) { a4[t] = *reinterpret_cast<const float4 *>(pa[t] + off); b4[t] = *reinterpret_cast<const float4 *>(pb[t] + off); }
        const float4 w4 = *reinterpret_cast<const float4 *>(pw + off);
        const float av[3][4] = { { a4[0].x, a4[0].y, a4[0].z, a4[0].w }, { a4[1].x, a4[1].y, a4[1].z, a4[1].w }, { a4[2].x, a4[2].y, a4[2].z, a4[2].w } };
        const float bv[3][4] = { { b4[0].x, b4[0].y, b4[0].z, b4[0].w }, { b4[1].x, b4[1].y, b4[1].z, b4[1].w }, { b4[2].x, b4[2].y, b4[2].z, b4[2].w } };
        const float wv[4] = { w4.x, w4.y, w4.z, w4.w };
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double da[3], db[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                da[t] = wt[t] ? (double)wv[j] * (double)av[t][j] : (double)av[t][j];     // exact: 48 bits
                db[t] = (double)bv[t][j];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[a], db[b], acc[a][b], 0, 0, 0);
        }
    }
    // C/D map of the f64 form: lane holds column lane & 15, rows (lane >> 4) + 4 q of its tile.  The waves add in wave order.
    for (uint32_t v = 0; v < 4u; ++v) {
        if (wave == v) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint32_t at = (16u * a + kg + 4u * q) * GR_RP_LD + 16u * b + m;
                        C[at] = v == 0u ? acc[a][b][q] : C[at] + acc[a][b][q];
                    }
        }
        __syncthreads();
    }
    if (threadIdx.x >= GR_RP_ROW_FRAMES * GR_RP_COL_FRAMES) return;
    const uint32_t i = threadIdx.x >> 4, j = threadIdx.x & 15u, gi = r0 + i, gj = c0 + j;
    if (gi >= n_rows || gj >= n_cols || (SYM && gi > gj)) return;
    float res = NAN;
    if (okr[gi] && okc[col0 + gj]) {
        // H[a][c] = sum p_a q_c, p the column (reference) frame, q the row (current) frame
        double H[3][3], Hw[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                H[a][c] = C[(6u * i + c) * GR_RP_LD + 3u * j + a];
                Hw[a][c] = C[(6u * i + 3u + c) * GR_RP_LD + 3u * j + a];
            }
        // the canonical orientation of the pair: the lexicographically smaller of (H, Hw) and (H^T, Hw^T)
        const double up[6] = { H[0][1], H[0][2], H[1][2], Hw[0][1], Hw[0][2], Hw[1][2] }, lo[6] = { H[1][0], H[2][0], H[2][1], Hw[1][0], Hw[2][0], Hw[2][1] };
        bool swap = false, decided = false;
#pragma unroll
        for (int k = 0; k < 6; ++k) if (!decided && up[k] != lo[k]) { swap = lo[k] < up[k]; decided = true; }
        if (swap) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = a + 1; c < 3; ++c) {
                    double t = H[a][c]; H[a][c] = H[c][a]; H[c][a] = t;
                    t = Hw[a][c]; Hw[a][c] = Hw[c][a]; Hw[c][a] = t;
                }
        }
        double R[3][3];
        gr_best_rotation(H, R);
        double tr = 0.0;
        for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) tr += R[a][c] * Hw[a][c];
        double r2 = (Gr[gi] + Gc[col0 + gj] - 2.0 * tr) / W;
        if (r2 < 0.0) r2 = 0.0;
        res = (float)sqrt(r2);
    }
    out[(size_t)gi * ld + gj] = res;
    if (SYM) out[(size_t)gj * ld + gi] = res;
}

namespace {

int rp_append(gr_rmsd_panel *p, uint32_t first_slot, uint32_t n_frames, int *status_out) {
    gr_ctx *c = p->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    if ((uint64_t)p->frames + n_frames > p->capacity) return fail(c, GR_E_INVALID_ARG, "rmsd panel: append beyond the panel's capacity");
    if (p->epoch != c->epoch) {           // masses or groups changed: the weights must still be the context's masses of these atoms
        for (uint32_t k = 0; k < p->n; ++k) if (memcmp(&c->masses_host[p->snap.atoms[k]], &p->w_host[k], sizeof(float)) != 0)
            return fail(c, GR_E_INVALID_ARG, "rmsd panel: the masses of its atoms have changed since it was created", p->snap.atoms[k]);
        p->epoch = c->epoch;
    }
    (void)hipSetDevice(c->device);
    const GrSel sel = p->snap.sel;
    std::vector<int> stat(n_frames, GR_OK);
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, [&](uint32_t slot) { return box_check(c, slot); });
        SlotUse use(c, s0, nb);
        st = states_from_prechecks(c, pre); if (st) return st;
        if (pre.any_ok) { st = pbc_center_stages(c, s0, nb, sel, 1); if (st) return st; }
        const size_t at = (size_t)p->frames + b0;
        k_rp_pack<<<dim3(nb), dim3(GR_WG), 0, c->stream>>>(c->frames, c->frame_stride, s0, p->snap.atoms_dev.get(), p->w_dev.get(), p->n, p->n_pad, c->boxes_dev, c->state_dev,
                                                          p->x.get() + at * 3u * p->n_pad, p->G.get() + at, p->ok_dev.get() + at);
        HIPCHK(c, hipGetLastError());
        st = fetch_states(c, nb); if (st) return st;
        for (uint32_t f = 0; f < nb; ++f) stat[(size_t)b0 + f] = grb::close_frame(c, fe, pre, f, status_out, [&] { return frame_status(c, c->state_host[f]); });
    }
    p->status.insert(p->status.end(), stat.begin(), stat.end());
    p->frames += n_frames;
    return fe.finish(c);
}

// the checks of a matrix call; `cols` is never null here
int rp_matrix_check(gr_rmsd_panel *rows, gr_rmsd_panel *cols) {
    gr_ctx *c = rows->c;
    int st = busy_check(c); if (st) return st;
    if (cols->c != c) { st = busy_check(cols->c); if (st) return fail(c, st, cols->c->err); }
    if (rows->frames == 0 || cols->frames == 0) return fail(c, GR_E_INVALID_ARG, "rmsd matrix: a panel holds no frame");
    if (rows->n != cols->n) { c->counts[0] = cols->n; c->counts[1] = rows->n; return fail(c, GR_E_INCONSISTENT_GROUP, rows->group); }
    if (cols->c->device != c->device) return fail(c, GR_E_INVALID_ARG, "rmsd matrix: the panels live on different devices");
    if (memcmp(rows->w_host.data(), cols->w_host.data(), (size_t)rows->n * sizeof(float)) != 0)
        return fail(c, GR_E_INVALID_ARG, "rmsd matrix: the panels carry different masses");
    return GR_OK;
}

// columns [col0, col0 + ncb) of the matrix into rows->out, row-major with leading dimension ncb
int rp_launch(gr_rmsd_panel *rows, gr_rmsd_panel *cols, uint32_t col0, uint32_t ncb) {
    gr_ctx *c = rows->c;
    const uint32_t nr = rows->frames;
    const dim3 grid((nr + GR_RP_ROW_FRAMES - 1u) / GR_RP_ROW_FRAMES, (ncb + GR_RP_COL_FRAMES - 1u) / GR_RP_COL_FRAMES);
    const bool sym = rows == cols && col0 == 0u && ncb == nr;
    if (sym) k_rp_matrix<true><<<grid, dim3(256), 0, c->stream>>>(rows->x.get(), rows->G.get(), rows->ok_dev.get(), nr, cols->x.get(), cols->G.get(), cols->ok_dev.get(), col0, ncb,
                                                                 rows->w_dev.get(), rows->n_pad, rows->W, rows->out.get(), ncb);
    else k_rp_matrix<false><<<grid, dim3(256), 0, c->stream>>>(rows->x.get(), rows->G.get(), rows->ok_dev.get(), nr, cols->x.get(), cols->G.get(), cols->ok_dev.get(), col0, ncb,
                                                              rows->w_dev.get(), rows->n_pad, rows->W, rows->out.get(), ncb);
    HIPCHK(c, hipGetLastError());
    return GR_OK;
}

}  // namespace

extern "C" {

gr_rmsd_panel *gr_rmsd_panel_create(gr_ctx *c, const char *group, uint32_t capacity_frames, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    const Group *g = need_group(c, group, *status, true); if (!g) return nullptr;
    if (capacity_frames == 0 || capacity_frames > GR_RP_MAX_FRAMES) { *status = fail(c, GR_E_INVALID_ARG, "rmsd panel: capacity of 1 .. 2^20 frames"); return nullptr; }
    std::unique_ptr<gr_rmsd_panel> p(new gr_rmsd_panel());
    p->c = c; p->group = group; p->capacity = capacity_frames; p->epoch = c->epoch;
    std::vector<uint32_t> atoms = hb_group_atoms(*g);
    p->n = (uint32_t)atoms.size();
    p->n_pad = (p->n + GR_RP_KSTEP - 1u) & ~(GR_RP_KSTEP - 1u);
    p->w_host.assign(p->n_pad, 0.0f);
    for (uint32_t k = 0; k < p->n; ++k) {
        const float m = c->masses_host[atoms[k]];
        if (m != m) { *status = fail(c, GR_E_NO_MASS, "atom has no mass", atoms[k]); return nullptr; }
        p->w_host[k] = m; p->W += (double)m;
    }
    (void)hipSetDevice(c->device);
    bool ok = p->snap.build(c, std::move(atoms), true) && p->w_dev.reserve(p->n_pad, grbuf::exact) == hipSuccess &&
              p->x.reserve((size_t)capacity_frames * 3u * p->n_pad, grbuf::exact) == hipSuccess && p->G.reserve(capacity_frames, grbuf::exact) == hipSuccess &&
              p->ok_dev.reserve(capacity_frames, grbuf::exact) == hipSuccess;
    ok = ok && hipMemcpy(p->w_dev.get(), p->w_host.data(), 4 * (size_t)p->n_pad, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        *status = fail(c, GR_E_HIP, "rmsd panel: device allocation failed");
        return nullptr;
    }
    p->w_host.resize(p->n);
    *status = GR_OK;
    return p.release();
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_rmsd_panel_destroy(gr_rmsd_panel *p) try { gr_object_destroy(p); } catch (...) { }

int gr_rmsd_panel_append_batch(gr_rmsd_panel *p, uint32_t first_slot, uint32_t n_frames, int *status_out) try {
    if (!p) return GR_E_INVALID_ARG;
    return rp_append(p, first_slot, n_frames, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_rmsd_panel_clear(gr_rmsd_panel *p) try {
    if (!p) return GR_E_INVALID_ARG;
    p->frames = 0; p->status.clear();
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

uint32_t gr_rmsd_panel_frames(const gr_rmsd_panel *p) { return p ? p->frames : 0u; }
uint64_t gr_rmsd_panel_n_atoms(const gr_rmsd_panel *p) { return p ? p->n : 0u; }

int gr_rmsd_panel_status(const gr_rmsd_panel *p, int *out) try {
    if (!p || (!out && p->frames)) return GR_E_INVALID_ARG;
    if (p->frames) memcpy(out, p->status.data(), (size_t)p->frames * sizeof(int));
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_rmsd_panel_set_block_entries(gr_rmsd_panel *p, uint64_t n) try {
    if (!p) return GR_E_INVALID_ARG;
    p->block_entries = n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_rmsd_matrix_device(gr_rmsd_panel *rows, gr_rmsd_panel *cols, float **out_dev, uint32_t *n_rows, uint32_t *n_cols) try {
    if (!rows) return GR_E_INVALID_ARG;
    if (!cols) cols = rows;
    gr_ctx *c = rows->c;
    if (out_dev) *out_dev = nullptr;
    int st = rp_matrix_check(rows, cols); if (st) return st;
    if (!out_dev) return fail(c, GR_E_INVALID_ARG, "NULL pointer");
    const uint64_t total = (uint64_t)rows->frames * cols->frames;
    if (total > GR_RP_MAX_DEVICE_ENTRIES) return fail(c, GR_E_INVALID_ARG, "rmsd matrix: more than 2^28 entries (gr_rmsd_matrix works in column blocks)");
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));            // the last reader of the previous result
    HIPCHK(c, rows->out.reserve((size_t)total, grbuf::exact));
    st = rp_launch(rows, cols, 0u, cols->frames); if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out_dev = rows->out.get();
    if (n_rows) *n_rows = rows->frames;
    if (n_cols) *n_cols = cols->frames;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_rmsd_matrix(gr_rmsd_panel *rows, gr_rmsd_panel *cols, float *out) try {
    if (!rows) return GR_E_INVALID_ARG;
    if (!cols) cols = rows;
    gr_ctx *c = rows->c;
    int st = rp_matrix_check(rows, cols); if (st) return st;
    if (!out) return fail(c, GR_E_INVALID_ARG, "NULL pointer");
    (void)hipSetDevice(c->device);
    const uint32_t nr = rows->frames, nc = cols->frames;
    const uint64_t budget = rows->block_entries ? rows->block_entries : GR_RP_BLOCK_ENTRIES;
    // columns per block: everything when it fits, else a multiple of the column tile
    uint32_t cb = nc;
    if ((uint64_t)nr * nc > budget) cb = (uint32_t)std::min<uint64_t>(nc, std::max<uint64_t>(GR_RP_COL_FRAMES, budget / nr / GR_RP_COL_FRAMES * GR_RP_COL_FRAMES));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, rows->out.reserve((size_t)nr * cb, grbuf::exact));
    for (uint32_t col0 = 0; col0 < nc; col0 += cb) {
        const uint32_t ncb = std::min<uint32_t>(cb, nc - col0);
        st = rp_launch(rows, cols, col0, ncb); if (st) return st;
        HIPCHK(c, hipMemcpy2DAsync(out + col0, (size_t)nc * sizeof(float), rows->out.get(), (size_t)ncb * sizeof(float), (size_t)ncb * sizeof(float), nr, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

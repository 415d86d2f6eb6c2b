// gr_msd.h -- MSD: "nojump" unwrapping and the windowed mean-squared displacement of a group over resident frames -- the first DYNAMICAL
// analysis of the library (diffusion of lipids, water, ions; gmx msd).  The reference has no function for it: its users download every
// frame, undo the periodic jumps in numpy and run a double loop over time origins.
//
// Per atom of the snapshot (group order, S atoms, padded with zeros to n_pad, a multiple of 64) the object keeps on the device
//   o  (f32 x3)  the ORIGIN: the atom's position in the first counted frame
//   w  (f32 x3)  the atom's position as stored in the last counted frame
//   u  (f64 x3)  the atom's unwrapped position in the last counted frame
// and the PANEL X[capacity][3][n_pad] (f32, component-major, RMSDPanel's layout): row t is frame t's displacement from the origin,
// components that GR_MSD_X / _Y / _Z do not select stored as zeros (the unwrapping itself is always 3-D), with q[t] = sum of the row's
// squares (f64) and ok[t].  A frame's slot may be overwritten as soon as the frame is appended.
// THE RULE for one good frame with stored position x and box B, per atom:
//   first counted frame:  o = w = x, u = (double)x
//   otherwise:            d = x - w, ONE f32 subtraction per component; with GR_MSD_NOJUMP d is reduced along c, then b, then a with
//                         k = gr_minimg_k(...) and fmaf(-k, ., .) -- the brick-reduction lines of gr_min_image_vec's non-orthogonal branch,
//                         no candidate-table refinement (in an orthorhombic cell the off-diagonal terms are zero), the box the frame's
//                         own -- then u += (double)d, a sequential f64 chain, and w = x.  Without NOJUMP u = (double)x.
//   panel entry:          (float)(u - (double)o), or 0 for a component that is not selected
// This is the displacement-summing scheme: it stays correct when the box changes from frame to frame (summing image counts times the
// current box vectors does not).  A step of half a box edge or more between two counted frames is ambiguous by nature: it is taken as
// the shorter way round.  A FAILED frame (an atom of the group without position; with NOJUMP a frame without a usable box) still takes
// a time index: its row is zeros, its ok 0, it enters no pair, the walk skips it (w and u stay) and the next good frame is unwrapped
// against the last good one.
//   k_fl_check    (gr_series.h) the first atom of the group without position, per frame
//   k_msd_walk    k_fl_accumulate's walk: a lane owns ONE atom of the snapshot for the launch and takes the segment's frames in ascending
//                 order, the rows of GR_FL_AHEAD frames in flight (buffer loads, no load under a condition), and writes its atoms' panel
//                 entries: consecutive lanes hold consecutive atoms, every component of every frame is one contiguous store per wave.
//                 All three forms of a group (block, masked span, index list) are walked through the snapshot's INDEX LIST: the panel is
//                 in group order whatever the form, so the row form of Fluctuations (four atoms per lane in slot order) would have to
//                 scatter its stores and compact masked spans; one walk, one order, and the three forms give the same bits by construction.
//   k_msd_norms   one workgroup per appended frame: q[t] by a fixed-order block sum (gr_block_sum), ok[t]
//   k_band_gram<true>, k_band_lags   (gr_band.h, shared with VectorCorrelation) the band product: D2 = q_t + q_t' - 2 G over the 64 x 64
//                 blocks of frame pairs that touch the band t' - t <= max_lag, G = X X^T on the matrix cores, every entry ONE chain of
//                 ONE wave; the blocks' diagonals are added in a fixed order, then the blocks of a lag.  D2(t, t) IS DEFINED AS 0, so
//                 msd[0] is exactly 0.
// No atomic decides a sum.  o, w, u, the panel and q are a function of the SEQUENCE of appended frames alone -- not of how they were cut
// into calls, 1024-frame segments or grids; sum[tau] is a function of the panel (and so is a prefix of the full curve's for any max_lag).
// The pair counts are integer work on the ok flags, done on the host.  CAP: capacity x 3 x n_pad x 4 B <= GR_MSD_MAX_PANEL_BYTES.
#pragma once
#include "gr_band.h"
#include "gr_fluct.h"

#if defined(__HIPCC__)

#define GR_MSD_MAX_WALK (1u << 22)        /* k_msd_walk's grid at most */
#define GR_MSD_DIMS (GR_MSD_X | GR_MSD_Y | GR_MSD_Z)

struct GrMsdState {
    float *o, *w;                         // [3][n_pad]
    double *u;                            // [3][n_pad]
    uint32_t npad;
};

struct gr_msd {
    gr_ctx *c = nullptr;
    std::string group;
    GrSnapshot snap;                      // the group's atoms at create (the check walks it in its form, the walk takes the index list)
    GrVerdicts verdicts;
    uint32_t n_atoms = 0, n_pad = 0, capacity = 0, flags = 0;
    grbuf::Dev<uint32_t> ok_dev;          // [capacity]
    grbuf::Dev<float> o, w, X;            // [3][n_pad], [3][n_pad], [capacity][3][n_pad]
    grbuf::Dev<double> u, q;              // [3][n_pad], [capacity]
    GrBandWork band;                      // compute
    std::vector<uint8_t> ok_host;         // [frames]
    uint32_t frames = 0;                  // time indices taken
    uint64_t n_good = 0;                  // counted frames
    bool computed = false;
    std::vector<double> sum_host;         // [lags] of the last compute
    std::vector<uint64_t> pairs_host;
    uint32_t walk_groups = 0;             // gr_msd_set_launch; 0: the default
    uint32_t last_walk = 0;
    uint64_t launches = 0;
};

namespace {

// frames [s0, s0 + nf) of `frames` -> rows 0 .. nf - 1 of X (the caller passes the panel's next rows); verdict as k_fl_accumulate
__global__ __launch_bounds__(GR_FL_WG) void k_msd_walk(const float *__restrict__ frames, size_t stride, uint32_t slot_bytes, uint32_t s0, uint32_t nf,
                                                       const uint32_t *__restrict__ idx, uint32_t n, const GrBox *__restrict__ boxes,
                                                       const uint32_t *__restrict__ verdict, GrMsdState S, uint32_t have_origin, uint32_t flags, float *__restrict__ X) {
    const uint32_t units = S.npad;
    const uint32_t per = (units + gridDim.x - 1u) / gridDim.x;
    const uint32_t u0 = (uint32_t)min((uint64_t)blockIdx.x * per, (uint64_t)units), u1 = (uint32_t)min((uint64_t)u0 + per, (uint64_t)units);
    const size_t up = S.npad;
    const bool nojump = (flags & GR_MSD_NOJUMP) != 0u;
    const bool dim[3] = { (flags & GR_MSD_X) != 0u, (flags & GR_MSD_Y) != 0u, (flags & GR_MSD_Z) != 0u };
    // the frame's slot as a buffer: zero records beyond the segment (and then the last frame's address, so that nothing points outside the slots)
    auto slot_of = [&](uint32_t f) {
        return gr_buf_rsrc(frames + (size_t)(s0 + min(f, nf - 1u)) * stride, f < nf ? slot_bytes : 0u);
    };
    for (uint32_t ub = u0; ub < u1; ub += GR_FL_WG) {
        const uint32_t k = ub + threadIdx.x;
        const bool live = k < u1;
        // where the lane's atom lies inside a slot; a pad (k >= n) or an idle lane reads zeros from beyond every slot
        uint32_t off[3] = { GR_BUF_NOWHERE, GR_BUF_NOWHERE, GR_BUF_NOWHERE };
        if (live && k < n) {
            const uint32_t i = idx[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) off[c] = (uint32_t)gr_tile_index(i, c) * 4u;
        }
        auto request = [&](uint32_t f, float (&v)[3]) {
            const __amdgpu_buffer_rsrc_t rs = slot_of(f);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = fl_buf_load_f32_stream(rs, off[c]);
        };
        // the atom's state, requested before the first rows (loads return in order)
        float o[3] = { 0.0f, 0.0f, 0.0f }, w[3] = { 0.0f, 0.0f, 0.0f };
        double u[3] = { 0.0, 0.0, 0.0 };
        if (live) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { o[c] = S.o[c * up + k]; w[c] = S.w[c * up + k]; u[c] = S.u[c * up + k]; }
        }
        float ring[GR_FL_AHEAD][3];
#pragma unroll
        for (int r = 0; r < GR_FL_AHEAD; ++r) {
            request((uint32_t)r, ring[r]);
            __builtin_amdgcn_sched_barrier(0);      // in frame order (k_fl_accumulate)
        }
        bool have = have_origin != 0u;
        uint32_t vnext[GR_FL_AHEAD];
#pragma unroll
        for (int r = 0; r < GR_FL_AHEAD; ++r) vnext[r] = verdict[r];
        for (uint32_t base = 0; base < nf; base += GR_FL_AHEAD) {
            uint32_t vcur[GR_FL_AHEAD];
#pragma unroll
            for (int r = 0; r < GR_FL_AHEAD; ++r) { vcur[r] = vnext[r]; vnext[r] = verdict[base + GR_FL_AHEAD + (uint32_t)r]; }
#pragma unroll
            for (int r = 0; r < GR_FL_AHEAD; ++r) {
                const uint32_t f = base + (uint32_t)r;
                const float (&x)[3] = ring[r];
                if (f < nf) {                                       // (the same in every lane, as is every branch on the verdict)
                    float e[3] = { 0.0f, 0.0f, 0.0f };
                    if (vcur[r] == GR_NOIDX) {
                        if (!have) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) { o[c] = w[c] = x[c]; u[c] = (double)x[c]; }
                            have = true;
                        } else if (nojump) {
                            const GrBox &b = boxes[s0 + f];
                            float dx = x[0] - w[0], dy = x[1] - w[1], dz = x[2] - w[2];
                            float kk = gr_minimg_k(dz, b.cz, b.icz, b.cz / 2.0f);
                            dx = fmaf(-kk, b.cx, dx); dy = fmaf(-kk, b.cy, dy); dz = fmaf(-kk, b.cz, dz);
                            kk = gr_minimg_k(dy, b.by, b.iby, b.by / 2.0f);
                            dx = fmaf(-kk, b.bx, dx); dy = fmaf(-kk, b.by, dy);
                            kk = gr_minimg_k(dx, b.ax, b.iax, b.ax / 2.0f);
                            dx = fmaf(-kk, b.ax, dx);
                            u[0] += (double)dx; u[1] += (double)dy; u[2] += (double)dz;
#pragma unroll
                            for (int c = 0; c < 3; ++c) w[c] = x[c];
                        } else {
#pragma unroll
                            for (int c = 0; c < 3; ++c) { u[c] = (double)x[c]; w[c] = x[c]; }
                        }
#pragma unroll
                        for (int c = 0; c < 3; ++c) e[c] = dim[c] ? (float)(u[c] - (double)o[c]) : 0.0f;
                    }
                    if (live) {
                        float *row = X + (size_t)f * 3u * up + k;
#pragma unroll
                        for (int c = 0; c < 3; ++c) row[c * up] = e[c];
                    }
                }
                request(f + GR_FL_AHEAD, ring[r]);                 // behind the frame's work: into the registers it has just left
            }
        }
        if (live) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { S.o[c * up + k] = o[c]; S.w[c * up + k] = w[c]; S.u[c * up + k] = u[c]; }
        }
    }
}

// frame f of the segment: q and ok of row f of X (K = 3 n_pad values)
__global__ __launch_bounds__(GR_WG) void k_msd_norms(const float *__restrict__ X, uint32_t K, const uint32_t *__restrict__ verdict, double *__restrict__ q,
                                                     uint32_t *__restrict__ ok) {
    __shared__ double lds[GR_WG / 64];
    const uint32_t f = blockIdx.x;
    const float *row = X + (size_t)f * K;
    double acc[1] = { 0.0 };
    for (uint32_t k = threadIdx.x; k < K; k += GR_WG) {
        const double v = (double)row[k];
        acc[0] = fma(v, v, acc[0]);
    }
    gr_block_sum<1>(acc, lds);
    if (threadIdx.x == 0) {
        const bool good = verdict[f] == GR_NOIDX;
        q[f] = good ? acc[0] : 0.0;
        ok[f] = good ? 1u : 0u;
    }
}

size_t msd_state_len(const gr_msd *m) { return 3u * (size_t)m->n_pad; }
size_t msd_row_len(const gr_msd *m) { return 3u * (size_t)m->n_pad; }

int msd_zero(gr_msd *m) {
    gr_ctx *c = m->c;
    const size_t len = msd_state_len(m);
    HIPCHK(c, hipMemsetAsync(m->o.get(), 0, len * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(m->w.get(), 0, len * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(m->u.get(), 0, len * sizeof(double), c->stream));
    m->frames = 0; m->n_good = 0; m->computed = false;
    m->ok_host.clear(); m->sum_host.clear(); m->pairs_host.clear();
    return GR_OK;
}

int msd_append(gr_msd *m, uint32_t first_slot, uint32_t n_frames, int *status_out) {
    gr_ctx *c = m->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    if ((uint64_t)m->frames + n_frames > m->capacity) return fail(c, GR_E_INVALID_ARG, "msd: append beyond the object's capacity");
    (void)hipSetDevice(c->device);
    const bool nojump = (m->flags & GR_MSD_NOJUMP) != 0u;
    const uint32_t slot_bytes = (uint32_t)(c->frame_stride * sizeof(float));
    const GrMsdState S = { m->o.get(), m->w.get(), m->u.get(), m->n_pad };
    const uint32_t K = (uint32_t)msd_row_len(m);
    GrVerdicts &V = m->verdicts;
    const uint32_t *vd = V.dev.get();
    m->computed = false;
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, nojump));
        {
            // (launched even when every frame failed its checks: the rows of failed frames are written as zeros)
            SlotUse use(c, s0, nb);
            st = V.begin(c, pre, nb); if (st) return st;
            // launch geometry: one wave per 64 atoms of the padded snapshot, one workgroup per frame of the norms; gr_msd_set_launch
            // replaces the number of the walk's ranges
            const uint32_t wx = std::min<uint32_t>(m->walk_groups ? m->walk_groups : m->n_pad / GR_FL_WG, GR_MSD_MAX_WALK);
            const size_t at = (size_t)m->frames + b0;
            float *rows = m->X.get() + at * K;
            if (pre.any_ok) V.check(c, m->snap, s0, nb);
            k_msd_walk<<<dim3(wx), dim3(GR_FL_WG), 0, c->stream>>>(c->frames, c->frame_stride, slot_bytes, s0, nb, m->snap.atoms_dev.get(), m->n_atoms, c->boxes_dev, vd, S,
                                                                  m->n_good ? 1u : 0u, m->flags, rows);
            k_msd_norms<<<dim3(nb), dim3(GR_WG), 0, c->stream>>>(rows, K, vd, m->q.get() + at, m->ok_dev.get() + at);
            HIPCHK(c, hipGetLastError());
            ++m->launches; m->last_walk = wx;
            st = V.end(c, nb); if (st) return st;
        }
        for (uint32_t k = 0; k < nb; ++k) {
            const int s = grb::close_frame(c, fe, pre, k, status_out, [&] { return V.judge(c, k); });
            m->ok_host.push_back(s == GR_OK ? 1 : 0);
            if (s == GR_OK) ++m->n_good;
        }
    }
    m->frames += n_frames;
    return fe.finish(c);
}

int msd_compute(gr_msd *m, uint32_t max_lag) {
    gr_ctx *c = m->c;
    int st = busy_check(c); if (st) return st;
    if (m->frames == 0) return fail(c, GR_E_INVALID_ARG, "msd: no frame has been appended");
    (void)hipSetDevice(c->device);
    grband::Geometry g;
    st = band_reserve(c, "msd", m->band, m->frames, max_lag, 1u, g); if (st) return st;
    st = band_launch<true>(c, m->band, g, 1u, m->X.get(), (uint32_t)msd_row_len(m), nullptr, 0u, m->q.get(), m->ok_dev.get(), m->frames); if (st) return st;
    ++m->launches;
    m->sum_host.assign(g.lags, 0.0);
    HIPCHK(c, hipMemcpyAsync(m->sum_host.data(), m->band.sums.get(), g.lags * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    grband::pair_counts(m->ok_host.data(), m->frames, g.lags, m->pairs_host);     // meanwhile
    HIPCHK(c, hipStreamSynchronize(c->stream));
    m->computed = true;
    return GR_OK;
}

}  // namespace

extern "C" {

gr_msd *gr_msd_create(gr_ctx *c, const char *group, uint32_t capacity_frames, uint32_t flags, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    const Group *g = need_group(c, group, *status, true); if (!g) return nullptr;
    if ((flags & ~(uint32_t)(GR_MSD_DIMS | GR_MSD_NOJUMP)) || !(flags & GR_MSD_DIMS)) {
        *status = fail(c, GR_E_INVALID_ARG, "msd: flags select at least one of GR_MSD_X, GR_MSD_Y, GR_MSD_Z and beside them GR_MSD_NOJUMP only");
        return nullptr;
    }
    if (capacity_frames == 0) { *status = fail(c, GR_E_INVALID_ARG, "msd: the capacity is at least one frame"); return nullptr; }
    if (c->frame_stride * sizeof(float) >= GR_BUF_NOWHERE) { *status = fail(c, GR_E_INVALID_ARG, "msd: a slot of this system is too large for a buffer resource"); return nullptr; }
    std::unique_ptr<gr_msd> m(new gr_msd());
    m->c = c; m->group = group; m->flags = flags; m->capacity = capacity_frames;
    std::vector<uint32_t> atoms = hb_group_atoms(*g);
    m->n_atoms = (uint32_t)atoms.size();
    m->n_pad = (m->n_atoms + GR_FL_WG - 1u) & ~(GR_FL_WG - 1u);
    const uint64_t panel_bytes = (uint64_t)capacity_frames * 3u * m->n_pad * sizeof(float);
    if (panel_bytes > GR_MSD_MAX_PANEL_BYTES) {
        *status = fail(c, GR_E_INVALID_ARG, "msd: capacity x 3 x n_pad x 4 B exceeds GR_MSD_MAX_PANEL_BYTES = " + std::to_string((unsigned long long)GR_MSD_MAX_PANEL_BYTES));
        return nullptr;
    }
    (void)hipSetDevice(c->device);
    const size_t len = msd_state_len(m.get());
    bool ok = m->snap.build(c, std::move(atoms)) && m->verdicts.reserve(2u * GR_FL_AHEAD) && m->o.reserve(len, grbuf::exact) == hipSuccess &&
              m->w.reserve(len, grbuf::exact) == hipSuccess && m->u.reserve(len, grbuf::exact) == hipSuccess &&
              m->X.reserve((size_t)capacity_frames * msd_row_len(m.get()), grbuf::exact) == hipSuccess && m->q.reserve(capacity_frames, grbuf::exact) == hipSuccess &&
              m->ok_dev.reserve(capacity_frames, grbuf::exact) == hipSuccess;
    ok = ok && msd_zero(m.get()) == GR_OK && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        *status = fail(c, GR_E_HIP, "msd: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return m.release();
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_msd_destroy(gr_msd *m) try { gr_object_destroy(m); } catch (...) { }

int gr_msd_append_batch(gr_msd *m, uint32_t first_slot, uint32_t n_frames, int *status_out) try {
    if (!m) return GR_E_INVALID_ARG;
    return msd_append(m, first_slot, n_frames, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_msd_clear(gr_msd *m) try {
    if (!m) return GR_E_INVALID_ARG;
    int st = busy_check(m->c); if (st) return st;
    (void)hipSetDevice(m->c->device);
    return msd_zero(m);
} catch (...) { return gr_abi_guard(); }

uint64_t gr_msd_frames(const gr_msd *m) { return m ? m->frames : 0u; }
uint64_t gr_msd_n_atoms(const gr_msd *m) { return m ? m->n_atoms : 0u; }
uint64_t gr_msd_capacity(const gr_msd *m) { return m ? m->capacity : 0u; }

int gr_msd_compute(gr_msd *m, uint32_t max_lag) try {
    if (!m) return GR_E_INVALID_ARG;
    return msd_compute(m, max_lag);
} catch (...) { return gr_abi_guard(); }

int gr_msd_read(gr_msd *m, double *msd, uint64_t *pairs) try {
    if (!m) return GR_E_INVALID_ARG;
    int st = busy_check(m->c); if (st) return st;
    if (!m->computed) return fail(m->c, GR_E_INVALID_ARG, "msd: read before gr_msd_compute (or after an append or clear behind it)");
    const double S = (double)m->n_atoms;
    for (size_t tau = 0; tau < m->sum_host.size(); ++tau) {
        if (msd) msd[tau] = m->pairs_host[tau] ? m->sum_host[tau] / ((double)m->pairs_host[tau] * S) : (double)NAN;
        if (pairs) pairs[tau] = m->pairs_host[tau];
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_msd_read_from_origin(gr_msd *m, double *out) try {
    if (!m || !out) return GR_E_INVALID_ARG;
    gr_ctx *c = m->c;
    int st = busy_check(c); if (st) return st;
    if (m->frames == 0) return GR_OK;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, m->q.get(), (size_t)m->frames * sizeof(double), hipMemcpyDeviceToHost));
    const double S = (double)m->n_atoms;
    for (uint32_t t = 0; t < m->frames; ++t) out[t] = m->ok_host[t] ? out[t] / S : (double)NAN;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_msd_read_displacements(gr_msd *m, uint32_t t0, uint32_t nt, float *out) try {
    if (!m || !out) return GR_E_INVALID_ARG;
    gr_ctx *c = m->c;
    int st = busy_check(c); if (st) return st;
    if ((uint64_t)t0 + nt > m->frames || nt == 0) return fail(c, GR_E_INVALID_ARG, "msd: frames out of range");
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t K = msd_row_len(m), np = m->n_pad, S = m->n_atoms;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, ((size_t)1 << 24) / K);       // rows per copy: 64 MiB at most
    std::vector<float> rows;
    for (uint32_t a = 0; a < nt; a += chunk) {
        const uint32_t n = std::min(chunk, nt - a);
        rows.resize((size_t)n * K);
        HIPCHK(c, hipMemcpy(rows.data(), m->X.get() + ((size_t)t0 + a) * K, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (uint32_t f = 0; f < n; ++f) {
            const float *r = rows.data() + (size_t)f * K;
            float *o = out + ((size_t)a + f) * 3u * S;
            for (size_t k = 0; k < S; ++k) { o[3 * k] = r[k]; o[3 * k + 1] = r[np + k]; o[3 * k + 2] = r[2 * np + k]; }
        }
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_msd_set_launch(gr_msd *m, uint32_t walk_groups, uint32_t gram_groups) try {
    if (!m) return GR_E_INVALID_ARG;
    m->walk_groups = walk_groups; m->band.gram_groups = gram_groups;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_msd_stat(const gr_msd *m, int key, uint64_t *value) try {
    if (!m || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_MSD_STAT_LAUNCHES: *value = m->launches; return GR_OK;
    case GR_MSD_STAT_LAST_WALK_GROUPS: *value = m->last_walk; return GR_OK;
    case GR_MSD_STAT_LAST_GRAM_GROUPS: *value = m->band.last_gram; return GR_OK;
    case GR_MSD_STAT_BLOCK_EDGE: *value = GR_BAND_BLOCK; return GR_OK;
    case GR_MSD_STAT_TRIP_VALUES: *value = GR_BAND_TRIP; return GR_OK;
    case GR_MSD_STAT_LAST_BLOCKS: *value = m->band.blocks; return GR_OK;
    case GR_MSD_STAT_LAGS: *value = m->computed ? m->sum_host.size() : 0u; return GR_OK;
    case GR_MSD_STAT_N_PAD: *value = m->n_pad; return GR_OK;
    case GR_MSD_STAT_COUNTED: *value = m->n_good; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

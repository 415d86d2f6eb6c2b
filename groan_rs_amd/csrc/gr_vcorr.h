// gr_vcorr.h -- VectorCorrelation: the reorientation autocorrelation functions of V bond vectors over resident frames,
//   C1(tau) = <u(t) . u(t + tau)>   and   C2(tau) = <P2(u(t) . u(t + tau))>,  P2(x) = (3 x^2 - 1) / 2     (gmx rotacf)
// -- water reorientation times, lipid tail and head-group dynamics, NMR relaxation and the Lipari-Szabo S^2 of every N-H bond.  The
// rotational counterpart of MSD (gr_msd.h); the reference has no function for it: its users download every frame, gather the vectors
// and run a double loop over time origins.
//
// The object holds a fixed list of V atom pairs (i, j), padded to n_pad (a multiple of 64), and up to two PANELS that outlive the slots:
//   X1[capacity][3][n_pad]  (GR_VCORR_P1)  u
//   X2[capacity][6][n_pad]  (GR_VCORR_P2)  u_x u_x, u_y u_y, u_z u_z, SQRT2_F (u_x u_y), SQRT2_F (u_x u_z), SQRT2_F (u_y u_z)
// f32, component-major, the pads zeros, with ok[t] per frame.  For unit vectors (u . u')^2 = sum_ab (u_a u_b)(u'_a u'_b): C2 is a Gram
// product over the six independent components of the rank-2 tensor u u^T, the off-diagonal ones scaled by sqrt 2 -- the same
// matrix-core path as C1 and as MSD's G.
// THE RULE for one good frame and vector k = (i, j), every product and sum rounded on its own, NO contraction (vc_vector is compiled with
// contraction off):
//   d = x_j - x_i            ONE f32 subtraction per component; with GR_VCORR_PBC followed by gr_min_image_vec with the frame's own box
//   with GR_VCORR_UNIT:      len = sqrtf((d_x d_x + d_y d_y) + d_z d_z), the CORRECTLY ROUNDED square root (gr_mag3_exact: gr_mag3's
//                            device form is the hardware's 1-ulp root over a contracted sum, whose bits no restatement can give);
//                            inv = 1.0f / len; u_c = d_c * inv.  u = 0 WHEN len = 0: such a vector adds nothing to a sum but STILL
//                            COUNTS IN THE DENOMINATOR (the mean is over V vectors, whatever their length)
//   without UNIT:            u = d
//   X2 entries:              p = u_a * u_b, then SQRT2_F * p for a != b; SQRT2_F = (float)M_SQRT2
// A FAILED frame (with PBC a frame without a usable box -- the box checks come first; a frame in which an atom named by any pair has
// no position: GR_E_NO_POSITION and the lowest such atom) still takes a time index: its rows are zeros, its ok 0, it enters no pair.
//   k_fl_check    (gr_series.h; index-list form over the UNIQUE atoms the pairs name) the lowest atom without position, per frame
//   k_vc_walk     <PBC, UNIT>: k_msd_walk's walk.  A lane owns ONE vector for the launch: it loads its two atom indices once (the table
//                 is uint32 [2][n_pad], a wave's index loads are contiguous), turns them into six byte offsets and takes the segment's
//                 frames in ascending order with the loads of GR_VC_AHEAD frames in flight (buffer loads, no load under a condition: a
//                 frame beyond the segment is a resource of zero records, a pad an offset beyond every slot).  Consecutive lanes hold
//                 consecutive vectors: every component of every frame is one contiguous store per wave.  Lane 0 of workgroup 0 writes ok.
//   k_band_gram<false>, k_band_lags   (gr_band.h, shared with MSD) the band product of the kept panels, K = 3 n_pad or 6 n_pad values
//                 per row; blockIdx.y is the panel, one launch serves both.  Unlike MSD the block's value is G itself and the
//                 diagonal t = t' is a valid pair (lag 0).
//   k_vc_each     the curve of EVERY vector: the band closed per vector contracts 3 or 6 values only, so it is a direct VALU kernel.  A
//                 wave owns 64 consecutive vectors and one lag; every (vector, lag) is ONE sequential f64 chain, frames ascending, within a
//                 frame the components in panel order, each term fma((double)a, (double)b, s) -- the product of two f32 is exact in
//                 f64, so numpy's s + a * b gives the same bits.  Only pairs with ok on both sides enter.  Every panel read is one
//                 coalesced row piece.
// No atomic decides a sum.  The panels are a function of the SEQUENCE of appended frames alone -- not of calls, 1024-frame segments or
// grids; S[tau] is a function of the panel (and so a prefix of the full curve's for any max_lag); no result depends on a grid.
// CAPS: capacity x (3 + 6) x n_pad x 4 B over the kept panels <= GR_MSD_MAX_PANEL_BYTES; V x lags x 8 B of gr_vcorr_compute_each's
// output per curve <= GR_VCORR_MAX_EACH_BYTES.
#pragma once
#include "gr_band.h"
#include "gr_series.h"

#if defined(__HIPCC__)

#define GR_VC_AHEAD 4                     /* frames whose loads a lane of the walk has in flight: 4 x 6 = 24 loads */
#define GR_VC_WG 64u                      /* lanes of a workgroup of k_vc_walk: one wave */
#define GR_VC_MAX_WALK (1u << 22)         /* k_vc_walk's grid at most */
#define GR_VC_MAX_EACH (1u << 20)         /* k_vc_each's grid at most */
#define GR_VC_RANKS (GR_VCORR_P1 | GR_VCORR_P2)

struct gr_vcorr {
    gr_ctx *c = nullptr;
    uint32_t flags = 0, V = 0, n_pad = 0, capacity = 0;
    GrTuples tab;                         // the pairs, the atoms they name, the device table [2][n_pad]
    GrVerdicts verdicts;
    grbuf::Dev<uint32_t> ok_dev;          // [capacity]
    grbuf::Dev<float> X1, X2;             // [capacity][3][n_pad], [capacity][6][n_pad]; a panel that is not kept is empty
    GrBandWork band;                      // compute
    grbuf::Dev<double> each;              // compute_each: [V][lags]
    std::vector<uint8_t> ok_host;         // [frames]
    uint32_t frames = 0;                  // time indices taken
    uint64_t n_good = 0;
    bool computed = false;
    std::vector<double> sum_host[2];      // [lags] of the last compute, per panel
    std::vector<uint64_t> pairs_host;
    uint32_t walk_groups = 0, each_groups = 0;        // gr_vcorr_set_launch; 0: the default
    uint32_t last_walk = 0, last_each = 0, last_lags = 0;
    uint64_t launches = 0;
};

namespace {

// THE RULE: u of one vector from the positions of its atoms, p = x_i, y_i, z_i, x_j, y_j, z_j
template <bool PBC, bool UNIT>
__device__ __forceinline__ void vc_vector(const float (&p)[6], const GrBox &box, float (&u)[3]) {
#pragma clang fp contract(off)
    float dx = p[3] - p[0], dy = p[4] - p[1], dz = p[5] - p[2];
    if (PBC) gr_min_image_vec(dx, dy, dz, box);
    if (UNIT) {
        const float len = gr_mag3_exact(dx, dy, dz);
        const float inv = 1.0f / len;
        const bool some = len > 0.0f;
        u[0] = some ? dx * inv : 0.0f; u[1] = some ? dy * inv : 0.0f; u[2] = some ? dz * inv : 0.0f;
    } else {
        u[0] = dx; u[1] = dy; u[2] = dz;
    }
}

// the six rank-2 entries of u, panel order
__device__ __forceinline__ void vc_rank2(const float (&u)[3], float (&e)[6]) {
#pragma clang fp contract(off)
    const float SQRT2_F = (float)M_SQRT2;
    e[0] = u[0] * u[0]; e[1] = u[1] * u[1]; e[2] = u[2] * u[2];
    const float xy = u[0] * u[1], xz = u[0] * u[2], yz = u[1] * u[2];
    e[3] = SQRT2_F * xy; e[4] = SQRT2_F * xz; e[5] = SQRT2_F * yz;
}

// frames [s0, s0 + nf) of `frames` -> rows 0 .. nf - 1 of X1 and X2 (the caller passes the panels' next rows; nullptr: the panel is not
// kept) and of ok; verdict[f] per frame, readable up to verdict[nf + 2 * GR_VC_AHEAD); table: [2][npad]
template <bool PBC, bool UNIT>
__global__ __launch_bounds__(GR_VC_WG) void k_vc_walk(const float *__restrict__ frames, size_t stride, uint32_t slot_bytes, uint32_t s0, uint32_t nf,
                                                      const uint32_t *__restrict__ table, uint32_t V, uint32_t npad, const GrBox *__restrict__ boxes,
                                                      const uint32_t *__restrict__ verdict, float *__restrict__ X1, float *__restrict__ X2, uint32_t *__restrict__ ok) {
    const uint32_t per = (npad + gridDim.x - 1u) / gridDim.x;
    const uint32_t u0 = (uint32_t)min((uint64_t)blockIdx.x * per, (uint64_t)npad), u1 = (uint32_t)min((uint64_t)u0 + per, (uint64_t)npad);
    const size_t up = npad;
    // the frame's slot as a buffer: zero records beyond the segment (and then the last frame's address, so that nothing points outside the slots)
    auto slot_of = [&](uint32_t f) {
        return gr_buf_rsrc(frames + (size_t)(s0 + min(f, nf - 1u)) * stride, f < nf ? slot_bytes : 0u);
    };
    for (uint32_t ub = u0; ub < u1; ub += GR_VC_WG) {
        const uint32_t k = ub + threadIdx.x;
        const bool live = k < u1;
        const bool writes_ok = blockIdx.x == 0u && ub == 0u && threadIdx.x == 0u;
        // where the lane's two atoms lie inside a slot; a pad (k >= V) or an idle lane reads zeros from beyond every slot
        uint32_t off[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) off[j] = GR_BUF_NOWHERE;
        if (live && k < V) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const uint32_t i = table[(size_t)a * up + k];
#pragma unroll
                for (int c = 0; c < 3; ++c) off[3 * a + c] = (uint32_t)gr_tile_index(i, c) * 4u;
            }
        }
        auto request = [&](uint32_t f, float (&v)[6]) {
            const __amdgpu_buffer_rsrc_t rs = slot_of(f);
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = gr_buf_load_f32(rs, off[j]);
        };
        float ring[GR_VC_AHEAD][6];
#pragma unroll
        for (int r = 0; r < GR_VC_AHEAD; ++r) {
            request((uint32_t)r, ring[r]);
            __builtin_amdgcn_sched_barrier(0);      // in frame order (k_fl_accumulate)
        }
        // the verdicts of a turn of the ring are requested one turn ahead (k_fl_accumulate)
        uint32_t vnext[GR_VC_AHEAD];
#pragma unroll
        for (int r = 0; r < GR_VC_AHEAD; ++r) vnext[r] = verdict[r];
        for (uint32_t base = 0; base < nf; base += GR_VC_AHEAD) {
            uint32_t vcur[GR_VC_AHEAD];
#pragma unroll
            for (int r = 0; r < GR_VC_AHEAD; ++r) { vcur[r] = vnext[r]; vnext[r] = verdict[base + GR_VC_AHEAD + (uint32_t)r]; }
#pragma unroll
            for (int r = 0; r < GR_VC_AHEAD; ++r) {
                const uint32_t f = base + (uint32_t)r;
                if (f < nf) {                                       // (the same in every lane, as is the branch on the verdict)
                    const bool good = vcur[r] == GR_NOIDX;
                    float u[3] = { 0.0f, 0.0f, 0.0f };
                    if (good) vc_vector<PBC, UNIT>(ring[r], boxes[s0 + f], u);
                    if (live) {
                        if (X1) {
                            float *row = X1 + (size_t)f * 3u * up + k;
#pragma unroll
                            for (int c = 0; c < 3; ++c) row[c * up] = u[c];
                        }
                        if (X2) {
                            float e[6];
                            vc_rank2(u, e);
                            float *row = X2 + (size_t)f * 6u * up + k;
#pragma unroll
                            for (int c = 0; c < 6; ++c) row[c * up] = e[c];
                        }
                    }
                    if (writes_ok) ok[f] = good ? 1u : 0u;
                }
                request(f + GR_VC_AHEAD, ring[r]);                 // behind the frame's work: into the registers it has just left
            }
        }
    }
}

typedef void (*vc_walk_t)(const float *, size_t, uint32_t, uint32_t, uint32_t, const uint32_t *, uint32_t, uint32_t, const GrBox *, const uint32_t *, float *, float *,
                          uint32_t *);

vc_walk_t vc_walk_kernel(uint32_t flags) {
    const bool pbc = (flags & GR_VCORR_PBC) != 0u, unit = (flags & GR_VCORR_UNIT) != 0u;
    if (pbc) return unit ? k_vc_walk<true, true> : k_vc_walk<true, false>;
    return unit ? k_vc_walk<false, true> : k_vc_walk<false, false>;
}

// out[k][tau] = the chain of vector k and lag tau over a panel of C components; a wave takes 64 consecutive vectors and one lag
template <int C>
__global__ __launch_bounds__(256) void k_vc_each(const float *__restrict__ X, uint32_t npad, uint32_t V, const uint32_t *__restrict__ ok, uint32_t T, uint32_t lags,
                                                 double *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t vblocks = npad / 64u;
    const uint64_t units = (uint64_t)vblocks * lags;
    const size_t K = (size_t)C * npad;
    for (uint64_t w = (uint64_t)blockIdx.x * 4u + wave; w < units; w += (uint64_t)gridDim.x * 4u) {
        const uint32_t tau = (uint32_t)(w / vblocks), k = 64u * (uint32_t)(w % vblocks) + lane;      // neighbouring waves: the same lag
        const float *a = X + k, *b = X + (size_t)tau * K + k;
        double s = 0.0;
#pragma unroll 4
        for (uint32_t t = 0; t + tau < T; ++t) {
            float av[C], bv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { av[c] = a[(size_t)t * K + (size_t)c * npad]; bv[c] = b[(size_t)t * K + (size_t)c * npad]; }
            if (ok[t] != 0u && ok[t + tau] != 0u) {                // (the same in every lane)
#pragma unroll
                for (int c = 0; c < C; ++c) s = fma((double)av[c], (double)bv[c], s);
            }
        }
        if (k < V) out[(size_t)k * lags + tau] = s;
    }
}

uint32_t vc_ranks(const gr_vcorr *v) { return ((v->flags & GR_VCORR_P1) ? 1u : 0u) + ((v->flags & GR_VCORR_P2) ? 1u : 0u); }

int vc_zero(gr_vcorr *v) {
    v->frames = 0; v->n_good = 0; v->computed = false; v->last_lags = 0;
    v->ok_host.clear(); v->sum_host[0].clear(); v->sum_host[1].clear(); v->pairs_host.clear();
    return GR_OK;
}

int vc_append(gr_vcorr *v, uint32_t first_slot, uint32_t n_frames, int *status_out) {
    gr_ctx *c = v->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    if ((uint64_t)v->frames + n_frames > v->capacity) return fail(c, GR_E_INVALID_ARG, "vcorr: append beyond the object's capacity");
    (void)hipSetDevice(c->device);
    const bool pbc = (v->flags & GR_VCORR_PBC) != 0u;
    const uint32_t slot_bytes = (uint32_t)(c->frame_stride * sizeof(float));
    const vc_walk_t kernel = vc_walk_kernel(v->flags);
    const size_t np = v->n_pad;
    GrVerdicts &R = v->verdicts;
    const uint32_t *vd = R.dev.get();
    v->computed = false;
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, pbc));
        {
            // (launched even when every frame failed its checks: the rows of failed frames are written as zeros)
            SlotUse use(c, s0, nb);
            st = R.begin(c, pre, nb); if (st) return st;
            // launch geometry: one wave per 64 vectors of the padded list; gr_vcorr_set_launch replaces the number of the walk's ranges
            const uint32_t wx = std::min<uint32_t>(v->walk_groups ? v->walk_groups : v->n_pad / GR_VC_WG, GR_VC_MAX_WALK);
            const size_t at = (size_t)v->frames + b0;
            float *r1 = (v->flags & GR_VCORR_P1) ? v->X1.get() + at * 3u * np : nullptr;
            float *r2 = (v->flags & GR_VCORR_P2) ? v->X2.get() + at * 6u * np : nullptr;
            if (pre.any_ok) R.check(c, v->tab.uniq, s0, nb);
            kernel<<<dim3(wx), dim3(GR_VC_WG), 0, c->stream>>>(c->frames, c->frame_stride, slot_bytes, s0, nb, v->tab.table_dev.get(), v->V, v->n_pad, c->boxes_dev, vd, r1, r2,
                                                               v->ok_dev.get() + at);
            HIPCHK(c, hipGetLastError());
            ++v->launches; v->last_walk = wx;
            st = R.end(c, nb); if (st) return st;
        }
        for (uint32_t k = 0; k < nb; ++k) {
            const int s = grb::close_frame(c, fe, pre, k, status_out, [&] { return R.judge(c, k); });
            v->ok_host.push_back(s == GR_OK ? 1 : 0);
            if (s == GR_OK) ++v->n_good;
        }
    }
    v->frames += n_frames;
    return fe.finish(c);
}

int vc_compute(gr_vcorr *v, uint32_t max_lag) {
    gr_ctx *c = v->c;
    int st = busy_check(c); if (st) return st;
    if (v->frames == 0) return fail(c, GR_E_INVALID_ARG, "vcorr: no frame has been appended");
    (void)hipSetDevice(c->device);
    const uint32_t ranks = vc_ranks(v);
    grband::Geometry g;
    st = band_reserve(c, "vcorr", v->band, v->frames, max_lag, ranks, g); if (st) return st;
    const uint32_t lags = g.lags;
    // the kept panels in rank order: panel 0 of the launch is X1 when it is kept
    const bool p1 = (v->flags & GR_VCORR_P1) != 0u;
    st = band_launch<false>(c, v->band, g, ranks, p1 ? v->X1.get() : v->X2.get(), (p1 ? 3u : 6u) * v->n_pad, v->X2.get(), 6u * v->n_pad, nullptr, v->ok_dev.get(), v->frames);
    if (st) return st;
    ++v->launches;
    v->sum_host[0].clear(); v->sum_host[1].clear();
    for (uint32_t r = 0; r < ranks; ++r) {
        std::vector<double> &dst = v->sum_host[(r == 0 && p1) ? 0 : 1];
        dst.assign(lags, 0.0);
        HIPCHK(c, hipMemcpyAsync(dst.data(), v->band.sums.get() + (size_t)r * lags, lags * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    grband::pair_counts(v->ok_host.data(), v->frames, lags, v->pairs_host);      // meanwhile
    HIPCHK(c, hipStreamSynchronize(c->stream));
    v->computed = true; v->last_lags = lags;
    return GR_OK;
}

int vc_compute_each(gr_vcorr *v, uint32_t max_lag, double *c1, double *c2) {
    gr_ctx *c = v->c;
    int st = busy_check(c); if (st) return st;
    if (!c1 && !c2) return fail(c, GR_E_INVALID_ARG, "vcorr: no output array");
    if ((c1 && !(v->flags & GR_VCORR_P1)) || (c2 && !(v->flags & GR_VCORR_P2))) return fail(c, GR_E_INVALID_ARG, "vcorr: a curve was asked for whose panel is not kept");
    if (v->frames == 0) return fail(c, GR_E_INVALID_ARG, "vcorr: no frame has been appended");
    const uint32_t T = v->frames;
    max_lag = std::min(max_lag, T - 1u);
    const uint32_t lags = max_lag + 1u;
    const uint64_t cells = (uint64_t)v->V * lags;
    if (cells * sizeof(double) > GR_VCORR_MAX_EACH_BYTES)
        return fail(c, GR_E_INVALID_ARG, "vcorr: V x lags x 8 B exceeds GR_VCORR_MAX_EACH_BYTES = " + std::to_string((unsigned long long)GR_VCORR_MAX_EACH_BYTES));
    (void)hipSetDevice(c->device);
    if (v->each.reserve((size_t)cells, grbuf::exact) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, GR_E_HIP, "vcorr: device allocation failed");
    }
    std::vector<uint64_t> pairs;
    grband::pair_counts(v->ok_host.data(), T, lags, pairs);
    const uint64_t units = (uint64_t)(v->n_pad / 64u) * lags;
    uint32_t grid = (uint32_t)std::min<uint64_t>((units + 3u) / 4u, GR_VC_MAX_EACH);
    if (v->each_groups && v->each_groups < grid) grid = v->each_groups;
    for (int rank = 1; rank <= 2; ++rank) {
        double *out = rank == 1 ? c1 : c2;
        if (!out) continue;
        if (rank == 1) k_vc_each<3><<<dim3(grid), dim3(256), 0, c->stream>>>(v->X1.get(), v->n_pad, v->V, v->ok_dev.get(), T, lags, v->each.get());
        else k_vc_each<6><<<dim3(grid), dim3(256), 0, c->stream>>>(v->X2.get(), v->n_pad, v->V, v->ok_dev.get(), T, lags, v->each.get());
        HIPCHK(c, hipGetLastError());
        ++v->launches; v->last_each = grid;
        HIPCHK(c, hipMemcpyAsync(out, v->each.get(), (size_t)cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        // closed on the host in f64: C1 = s / pairs, C2 = (1.5 s) / pairs - 0.5; NaN where there is no pair
        for (uint64_t k = 0; k < v->V; ++k) {
            double *row = out + k * lags;
            for (uint32_t tau = 0; tau < lags; ++tau) {
                if (!pairs[tau]) { row[tau] = (double)NAN; continue; }
                const double p = (double)pairs[tau];
                if (rank == 1) row[tau] = row[tau] / p;
                else { const double a = 1.5 * row[tau]; const double b = a / p; row[tau] = b - 0.5; }
            }
        }
    }
    return GR_OK;
}

}  // namespace

extern "C" {

gr_vcorr *gr_vcorr_create(gr_ctx *c, const uint64_t *atoms, uint64_t n_vectors, uint32_t capacity_frames, uint32_t flags, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    if (!atoms || n_vectors == 0 || n_vectors > 0x7FFFFFC0u) { *status = fail(c, GR_E_INVALID_ARG, "vcorr: the list of pairs is empty (or holds 2^31 pairs or more)"); return nullptr; }
    if ((flags & ~(uint32_t)(GR_VCORR_PBC | GR_VCORR_UNIT | GR_VC_RANKS)) || !(flags & GR_VC_RANKS)) {
        *status = fail(c, GR_E_INVALID_ARG, "vcorr: flags select at least one of GR_VCORR_P1, GR_VCORR_P2 and beside them GR_VCORR_PBC and GR_VCORR_UNIT only");
        return nullptr;
    }
    if ((flags & GR_VCORR_P2) && !(flags & GR_VCORR_UNIT)) { *status = fail(c, GR_E_INVALID_ARG, "vcorr: GR_VCORR_P2 needs GR_VCORR_UNIT (the rank-2 product is P2 for unit vectors only)"); return nullptr; }
    if (capacity_frames == 0) { *status = fail(c, GR_E_INVALID_ARG, "vcorr: the capacity is at least one frame"); return nullptr; }
    if (c->frame_stride * sizeof(float) >= GR_BUF_NOWHERE) { *status = fail(c, GR_E_INVALID_ARG, "vcorr: a slot of this system is too large for a buffer resource"); return nullptr; }
    std::unique_ptr<gr_vcorr> v(new gr_vcorr());
    v->c = c; v->flags = flags; v->capacity = capacity_frames; v->V = (uint32_t)n_vectors;
    v->n_pad = (v->V + GR_VC_WG - 1u) & ~(GR_VC_WG - 1u);
    const uint64_t comps = ((flags & GR_VCORR_P1) ? 3u : 0u) + ((flags & GR_VCORR_P2) ? 6u : 0u);
    const uint64_t panel_bytes = (uint64_t)capacity_frames * comps * v->n_pad * sizeof(float);
    if (panel_bytes > GR_MSD_MAX_PANEL_BYTES) {
        *status = fail(c, GR_E_INVALID_ARG, "vcorr: the panels (capacity x 3 and x 6 x n_pad x 4 B) exceed GR_MSD_MAX_PANEL_BYTES = " + std::to_string((unsigned long long)GR_MSD_MAX_PANEL_BYTES));
        return nullptr;
    }
    *status = v->tab.build(c, "vcorr", "a pair names one atom twice", atoms, n_vectors, 2u, v->n_pad); if (*status) return nullptr;
    const size_t np = v->n_pad;
    bool ok = v->verdicts.reserve(2u * GR_VC_AHEAD) && v->ok_dev.reserve(capacity_frames, grbuf::exact) == hipSuccess;
    if (flags & GR_VCORR_P1) ok = ok && v->X1.reserve((size_t)capacity_frames * 3u * np, grbuf::exact) == hipSuccess;
    if (flags & GR_VCORR_P2) ok = ok && v->X2.reserve((size_t)capacity_frames * 6u * np, grbuf::exact) == hipSuccess;
    ok = ok && vc_zero(v.get()) == GR_OK && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        *status = fail(c, GR_E_HIP, "vcorr: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return v.release();
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_vcorr_destroy(gr_vcorr *v) try { gr_object_destroy(v); } catch (...) { }

uint64_t gr_vcorr_count(const gr_vcorr *v) { return v ? v->V : 0u; }
uint64_t gr_vcorr_frames(const gr_vcorr *v) { return v ? v->frames : 0u; }
uint64_t gr_vcorr_capacity(const gr_vcorr *v) { return v ? v->capacity : 0u; }

int gr_vcorr_append_batch(gr_vcorr *v, uint32_t first_slot, uint32_t n_frames, int *status_out) try {
    if (!v) return GR_E_INVALID_ARG;
    int st = busy_check(v->c); if (st) return st;
    return vc_append(v, first_slot, n_frames, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_vcorr_clear(gr_vcorr *v) try {
    if (!v) return GR_E_INVALID_ARG;
    int st = busy_check(v->c); if (st) return st;
    return vc_zero(v);
} catch (...) { return gr_abi_guard(); }

int gr_vcorr_compute(gr_vcorr *v, uint32_t max_lag) try {
    if (!v) return GR_E_INVALID_ARG;
    return vc_compute(v, max_lag);
} catch (...) { return gr_abi_guard(); }

int gr_vcorr_read(gr_vcorr *v, double *c1, double *c2, uint64_t *pairs) try {
    if (!v) return GR_E_INVALID_ARG;
    int st = busy_check(v->c); if (st) return st;
    if (!v->computed) return fail(v->c, GR_E_INVALID_ARG, "vcorr: read before gr_vcorr_compute (or after an append or clear behind it)");
    if ((c1 && !(v->flags & GR_VCORR_P1)) || (c2 && !(v->flags & GR_VCORR_P2))) return fail(v->c, GR_E_INVALID_ARG, "vcorr: a curve was asked for whose panel is not kept");
    const double V = (double)v->V;
    for (size_t tau = 0; tau < v->pairs_host.size(); ++tau) {
        const uint64_t n = v->pairs_host[tau];
        const double den = (double)n * V;
        if (c1) c1[tau] = n ? v->sum_host[0][tau] / den : (double)NAN;
        if (c2) {
            if (n) { const double a = 1.5 * v->sum_host[1][tau]; const double b = a / den; c2[tau] = b - 0.5; }
            else c2[tau] = (double)NAN;
        }
        if (pairs) pairs[tau] = n;
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_vcorr_compute_each(gr_vcorr *v, uint32_t max_lag, double *c1_out, double *c2_out) try {
    if (!v) return GR_E_INVALID_ARG;
    return vc_compute_each(v, max_lag, c1_out, c2_out);
} catch (...) { return gr_abi_guard(); }

int gr_vcorr_read_vectors(gr_vcorr *v, uint32_t t0, uint32_t nt, float *out) try {
    if (!v || !out) return GR_E_INVALID_ARG;
    gr_ctx *c = v->c;
    int st = busy_check(c); if (st) return st;
    if (!(v->flags & GR_VCORR_P1)) return fail(c, GR_E_INVALID_ARG, "vcorr: the vectors are the rank-1 panel, which is not kept");
    if ((uint64_t)t0 + nt > v->frames || nt == 0) return fail(c, GR_E_INVALID_ARG, "vcorr: frames out of range");
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t np = v->n_pad, K = 3u * np, V = v->V;
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, ((size_t)1 << 24) / K);       // rows per copy: 64 MiB at most
    std::vector<float> rows;
    for (uint32_t a = 0; a < nt; a += chunk) {
        const uint32_t n = std::min(chunk, nt - a);
        rows.resize((size_t)n * K);
        HIPCHK(c, hipMemcpy(rows.data(), v->X1.get() + ((size_t)t0 + a) * K, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (uint32_t f = 0; f < n; ++f) {
            const float *r = rows.data() + (size_t)f * K;
            float *o = out + ((size_t)a + f) * 3u * V;
            for (size_t k = 0; k < V; ++k) { o[3 * k] = r[k]; o[3 * k + 1] = r[np + k]; o[3 * k + 2] = r[2 * np + k]; }
        }
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_vcorr_set_launch(gr_vcorr *v, uint32_t walk_groups, uint32_t gram_groups, uint32_t each_groups) try {
    if (!v) return GR_E_INVALID_ARG;
    v->walk_groups = walk_groups; v->band.gram_groups = gram_groups; v->each_groups = each_groups;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_vcorr_stat(const gr_vcorr *v, int key, uint64_t *value) try {
    if (!v || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_VCORR_STAT_LAUNCHES: *value = v->launches; return GR_OK;
    case GR_VCORR_STAT_N_PAD: *value = v->n_pad; return GR_OK;
    case GR_VCORR_STAT_LAGS: *value = v->computed ? v->last_lags : 0u; return GR_OK;
    case GR_VCORR_STAT_LAST_WALK_GROUPS: *value = v->last_walk; return GR_OK;
    case GR_VCORR_STAT_LAST_GRAM_GROUPS: *value = v->band.last_gram; return GR_OK;
    case GR_VCORR_STAT_LAST_EACH_GROUPS: *value = v->last_each; return GR_OK;
    case GR_VCORR_STAT_LAST_BLOCKS: *value = v->band.blocks; return GR_OK;
    case GR_VCORR_STAT_COUNTED: *value = v->n_good; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

// gr_gyration.h -- Segments: the gyration tensor, the radius of gyration and the principal axes of EVERY segment of a partition, for a
// block of resident frames (gmx gyrate / gmx principal per residue, lipid, chain; asphericity, tilt of a long axis).
//
// The reference has no such call: its users download each frame and loop over molecules on the host.  Here the partition, the team
// classes and the centre are those of gr_segments.h; what is new is one more walk over the segment's atoms and an eigen-solve.
//
// The first part of this file is the CLOSING arithmetic, host and device: it compiles without HIP (tests/test_gyration_host.py includes
// it from a plain g++ driver).
//   gr_gyr_close   ten f64 sums about an origin c -- W = sum w, sum w d_a, sum w d_a d_b with d = x - c -- become the tensor about the
//                  weighted MEAN: m_a = sum w d_a / W, S_ab = sum w d_a d_b / W - m_a m_b (parallel axes).  c only has to be close
//                  enough to the segment for the minimum image to unwrap it: its rounding, or its being an estimate, drops out.
//                  A diagonal entry below zero (rounding) is stored as zero; a segment of one atom has S = 0 by definition (its d is
//                  an ulp of c, whose square would otherwise survive as 1e-29 nm^2).  Rg = sqrt(S_xx + S_yy + S_zz).
//   gr_gyr_order   the Jacobi solver's eigenpairs in the order lambda_1 >= lambda_2 >= lambda_3 (ties keep the solver's order), v_1 and
//                  v_2 flipped so that their component of largest magnitude is positive (the first such component on ties),
//                  v_3 = v_1 x v_2: a right-handed frame that depends on the tensor only.
//   gr_gyr_axes    tensor (xx yy zz xy xz yz) -> eigenvalues and rows v_1 .. v_3: gr_jacobi_eig3 + gr_gyr_order
//
// The second part (hipcc only) holds the kernels and the C ABI; gr_api.hip includes this file behind gr_segments.h.
//   k_segment_moments<TEAM>   the grid, records, team classes and frame_ok handling of k_segment_centers<TEAM>.  The team first runs the
//                  centre's stages -- the same gr_seg_stage calls in the same order, so centre, status and error key are those of
//                  gr_segments_center_batch bit for bit -- then walks its atoms once more (gr_gyr_stage: the same trips, the loads of U
//                  trips in flight, atoms added in trip order): d = x - c in f32 (NAIVE) or gr_vector_to(c, x) (ESTIMATE, PBC), and
//                  the ten sums in f64 with explicit fma (products of f32 values are exact in f64; one rounding per term).  The sums
//                  are reduced like the centre's: __shfl_xor in the fixed tree, the workgroup class's four waves through an LDS block
//                  of their own, added in wave order; no atomics.  The team's first lane closes and stores moments[f][s][0..9].
//   k_gyration_axes   one lane per (frame, segment): reads the six f32 tensor entries BACK from moments, so the axes are a function of
//                  the returned tensor alone, and every lane of a wave solves a matrix (inside the team kernel one lane in 4 .. 256
//                  would).  A NaN tensor gives a NaN row.
// A segment of the batch is worked in PIECES of frames so that the device block (moments + axes: 88 bytes per frame and segment) stays
// within GR_GYR_BLOCK_BYTES, or one frame's share if that alone is more; the host form copies out per piece.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gr_rotation.h"

#if defined(__HIPCC__)
#define GR_GYR_HD __host__ __device__ inline
#else
#define GR_GYR_HD inline
#endif

#define GR_GYR_SUMS 10       /* W, w d (3), w d d (xx yy zz xy xz yz) */
#define GR_GYR_MOMENTS 10    /* floats per (frame, segment): centre (3), Rg, S (xx yy zz xy xz yz) */
#define GR_GYR_AXES 12       /* floats per (frame, segment): eigenvalues (3), rows v1 v2 v3 */

// s[GR_GYR_SUMS] about any origin, n = atoms of the segment -> *rg (nm) and S[6] (nm^2: xx yy zz xy xz yz) about the weighted mean
GR_GYR_HD void gr_gyr_close(const double *s, uint32_t n, double *rg, double *S) {
    if (n == 1u && s[0] == s[0] && s[0] != 0.0) {
        for (int k = 0; k < 6; ++k) S[k] = 0.0;
        *rg = 0.0;
        return;
    }
    const double W = s[0];
    const double mx = s[1] / W, my = s[2] / W, mz = s[3] / W;
    S[0] = fma(-mx, mx, s[4] / W); S[1] = fma(-my, my, s[5] / W); S[2] = fma(-mz, mz, s[6] / W);
    S[3] = fma(-mx, my, s[7] / W); S[4] = fma(-mx, mz, s[8] / W); S[5] = fma(-my, mz, s[9] / W);
    for (int k = 0; k < 3; ++k) if (S[k] < 0.0) S[k] = 0.0;
    *rg = sqrt(S[0] + S[1] + S[2]);
}

// w[3], V[3][3] with the eigenvectors in COLUMNS (what gr_jacobi_eig3 leaves) -> lam[3] descending, R[3][3] with v1, v2, v3 in ROWS
GR_GYR_HD void gr_gyr_order(const double *w, const double V[3][3], double *lam, double R[3][3]) {
    int o0 = 0, o1 = 1, o2 = 2;       // a stable sort of three: an entry moves in front of another only when it is strictly larger
    if (w[o1] > w[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (w[o2] > w[o1]) { const int t = o1; o1 = o2; o2 = t; }
    if (w[o1] > w[o0]) { const int t = o0; o0 = o1; o1 = t; }
    lam[0] = w[o0]; lam[1] = w[o1]; lam[2] = w[o2];
    for (int i = 0; i < 3; ++i) { R[0][i] = V[i][o0]; R[1][i] = V[i][o1]; }
    for (int k = 0; k < 2; ++k) {
        int big = 0;
        if (fabs(R[k][1]) > fabs(R[k][big])) big = 1;
        if (fabs(R[k][2]) > fabs(R[k][big])) big = 2;
        if (R[k][big] < 0.0) { R[k][0] = -R[k][0]; R[k][1] = -R[k][1]; R[k][2] = -R[k][2]; }
    }
    R[2][0] = R[0][1] * R[1][2] - R[0][2] * R[1][1];
    R[2][1] = R[0][2] * R[1][0] - R[0][0] * R[1][2];
    R[2][2] = R[0][0] * R[1][1] - R[0][1] * R[1][0];
}

// S[6] (xx yy zz xy xz yz) -> lam[3], R[3][3] (rows)
GR_GYR_HD void gr_gyr_axes(const double *S, double *lam, double R[3][3]) {
    double A[3][3] = { { S[0], S[3], S[4] }, { S[3], S[1], S[5] }, { S[4], S[5], S[2] } }, V[3][3];
    gr_jacobi_eig3(A, V);
    const double w[3] = { A[0][0], A[1][1], A[2][2] };
    gr_gyr_order(w, V, lam, R);
}

#if defined(__HIPCC__)

#define GR_GYR_BLOCK_BYTES (256ull << 20)      /* the device block of a piece: moments + axes */
#define GR_GYR_FRAME_FLOATS (GR_GYR_MOMENTS + GR_GYR_AXES)
static_assert(GR_GYR_FRAME_FLOATS * sizeof(float) == 88, "include/groan_hip.h documents 88 bytes per frame and segment");

namespace {

// the moment sums of one segment about (cx, cy, cz) by its team: afterwards EVERY lane of the team holds the totals
// (lds: the workgroup class's exchange block of this stage, [TEAM / 64][GR_GYR_SUMS])
template <int PBC, int TEAM, int U>
__device__ __forceinline__ void gr_gyr_stage(const float *__restrict__ xyz, const float *__restrict__ masses, const uint32_t *__restrict__ list, const uint32_t first,
                                             const uint32_t n, const GrBox &box, const int weighted, const float cx, const float cy, const float cz, const uint32_t tl,
                                             double *lds, double (&acc)[GR_GYR_SUMS]) {
#pragma unroll
    for (int k = 0; k < GR_GYR_SUMS; ++k) acc[k] = 0.0;
    for (uint32_t j0 = tl; j0 < n; j0 += (uint32_t)(U * TEAM)) {
        float x[U], y[U], z[U], m[U];
        uint32_t ii[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const uint32_t j = j0 + (uint32_t)(k * TEAM);
            const uint32_t jj = j < n ? j : 0u;
            ii[k] = list ? list[jj] : first + jj;
        }
#pragma unroll
        for (int k = 0; k < U; ++k) { gr_pos_load(xyz, ii[k], x[k], y[k], z[k]); m[k] = weighted ? masses[ii[k]] : 1.0f; }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            if (j0 + (uint32_t)(k * TEAM) >= n) continue;
            float vx, vy, vz;
            if (PBC) gr_vector_to(cx, cy, cz, x[k], y[k], z[k], box, vx, vy, vz);
            else { vx = x[k] - cx; vy = y[k] - cy; vz = z[k] - cz; }
            const double w = (double)m[k], dx = (double)vx, dy = (double)vy, dz = (double)vz;
            const double wx = w * dx, wy = w * dy, wz = w * dz;          // (exact: 24 x 24 bits)
            acc[0] += w; acc[1] += wx; acc[2] += wy; acc[3] += wz;
            acc[4] = fma(wx, dx, acc[4]); acc[5] = fma(wy, dy, acc[5]); acc[6] = fma(wz, dz, acc[6]);
            acc[7] = fma(wx, dy, acc[7]); acc[8] = fma(wx, dz, acc[8]); acc[9] = fma(wy, dz, acc[9]);
        }
    }
    constexpr int W = TEAM < 64 ? TEAM : 64;
#pragma unroll
    for (int q = 0; q < GR_GYR_SUMS; ++q) acc[q] = gr_seg_team_sum<W>(acc[q]);
    if (TEAM > 64) {    // the four waves' totals through LDS, added in wave order by every lane
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
            for (int q = 0; q < GR_GYR_SUMS; ++q) lds[wave * GR_GYR_SUMS + q] = acc[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GR_GYR_SUMS; ++q) {
            double s = lds[q];
#pragma unroll
            for (int wv = 1; wv < TEAM / 64; ++wv) s += lds[wv * GR_GYR_SUMS + q];
            acc[q] = s;
        }
    }
}

// grid (teams of the class / teams per workgroup, frames of the piece); `recs` = the class's records; first_slot, keys and frame_ok
// are the piece's own (frame 0 of the grid is the piece's first frame)
template <int TEAM>
__global__ __launch_bounds__(256) void k_segment_moments(const float *__restrict__ frames, size_t frame_stride, uint32_t first_slot, const float *__restrict__ masses,
                                                         const grs::Rec *__restrict__ recs, uint32_t n_recs, const uint32_t *__restrict__ atoms,
                                                         const GrBox *__restrict__ boxes, int kind, int weighted, float *__restrict__ moments, uint32_t n_segments,
                                                         unsigned long long *keys, const uint32_t *__restrict__ frame_ok) {
    constexpr int U = TEAM <= 16 ? 1 : 4;
    __shared__ double lds[2][TEAM > 64 ? (TEAM / 64) * (GR_CEN_K + 1) : 1];
    __shared__ double lds_m[TEAM > 64 ? (TEAM / 64) * GR_GYR_SUMS : 1];      // (a block of its own: no barrier is shared with the centre stages)
    const uint32_t f = blockIdx.y;
    const uint32_t team = blockIdx.x * (256u / TEAM) + threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
    const bool active = team < n_recs;                       // (a team behind the class walks the last segment again and stores nothing)
    const grs::Rec r = recs[active ? team : n_recs - 1u];
    const uint32_t n = r.n_flag & ~GR_SEG_CONTIGUOUS;
    const uint32_t *list = (r.n_flag & GR_SEG_CONTIGUOUS) ? nullptr : atoms + r.begin;
    float *o = moments + ((size_t)f * n_segments + r.ordinal) * GR_GYR_MOMENTS;
    const bool writer = active && tl == 0u;
    if (frame_ok && !frame_ok[f]) {                          // the frame failed its host checks: NaN everywhere, nothing read
        if (writer) {
#pragma unroll
            for (int k = 0; k < GR_GYR_MOMENTS; ++k) o[k] = NAN;
        }
        return;
    }
    const GrBox &box = boxes[first_slot + f];
    const float *xyz = frames + (size_t)(first_slot + f) * frame_stride;
    GrFrameState st = {};
    st.err_index = GR_NOIDX;
    // the centre: k_segment_centers' stages, call for call
    if (kind == 0) gr_seg_stage<0, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, 0, 1, st, tl, lds[0]);
    else if (kind == 1) gr_seg_stage<1, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, 1, 1, st, tl, lds[0]);
    else {
        gr_seg_stage<1, TEAM, U>(xyz, masses, list, r.begin, n, box, 0, 0, 0, st, tl, lds[0]);
        if (st.status == 0) gr_seg_stage<2, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, 0, 1, st, tl, lds[1]);
    }
    if (st.status != 0) {                                    // (the status is the team's: no lane parts)
        if (!writer) return;
#pragma unroll
        for (int k = 0; k < GR_GYR_MOMENTS; ++k) o[k] = NAN;
        atomicMin(&keys[f], ((unsigned long long)r.ordinal << 33) | ((unsigned long long)(st.status == 7 ? 1u : 0u) << 32) | st.err_index);
        return;
    }
    double acc[GR_GYR_SUMS];
    if (kind == 0) gr_gyr_stage<0, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, st.com[0], st.com[1], st.com[2], tl, lds_m, acc);
    else gr_gyr_stage<1, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, st.com[0], st.com[1], st.com[2], tl, lds_m, acc);
    if (!writer) return;
    double rg, S[6];
    gr_gyr_close(acc, n, &rg, S);
    o[0] = st.com[0]; o[1] = st.com[1]; o[2] = st.com[2]; o[3] = (float)rg;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[4 + k] = (float)S[k];
}

// one lane per (frame, segment) of the piece
__global__ __launch_bounds__(256) void k_gyration_axes(const float *__restrict__ moments, float *__restrict__ axes, uint64_t n_rows) {
    const uint64_t row = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (row >= n_rows) return;
    const float *m = moments + row * GR_GYR_MOMENTS + 4;
    float *o = axes + row * GR_GYR_AXES;
    double S[6];
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) { const float v = m[k]; S[k] = (double)v; nan = nan || v != v; }
    if (nan) {
#pragma unroll
        for (int k = 0; k < GR_GYR_AXES; ++k) o[k] = NAN;
        return;
    }
    double lam[3], R[3][3];
    gr_gyr_axes(S, lam, R);
    o[0] = (float)lam[0]; o[1] = (float)lam[1]; o[2] = (float)lam[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[3 + 3 * k] = (float)R[k][0]; o[4 + 3 * k] = (float)R[k][1]; o[5 + 3 * k] = (float)R[k][2]; }
}

template <int TEAM>
void gyr_launch(gr_segments *S, int cls, uint32_t s0, uint32_t np, uint32_t p0, int kind, int weighted, const uint32_t *ok_dev) {
    gr_ctx *c = S->c;
    const uint32_t n_recs = (uint32_t)(S->start[cls + 1] - S->start[cls]);
    if (n_recs == 0) return;
    const uint32_t per = 256u / TEAM;
    k_segment_moments<TEAM><<<dim3((n_recs + per - 1u) / per, np), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0 + p0, c->masses, S->recs_dev + S->start[cls], n_recs,
                                                                                           S->atoms_dev, c->boxes_dev, kind, weighted, S->gyr.get(), (uint32_t)S->P.count(),
                                                                                           S->key_dev + p0, ok_dev ? ok_dev + p0 : nullptr);
    ++S->last_launches;
}

// frames of a piece: what was forced, else what GR_GYR_BLOCK_BYTES holds; at least one, at most a segment of the batch
uint32_t gyr_piece_frames(const gr_segments *S) {
    const uint64_t p = S->piece_frames ? S->piece_frames : GR_GYR_BLOCK_BYTES / (S->P.count() * GR_GYR_FRAME_FLOATS * sizeof(float));
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(p, 1), GR_MAX_BATCH);
}

// moments_host: [n_frames][M][10] or NULL (the device form: one piece, left in S->gyr); axes_host: [n_frames][M][12] or NULL
int seg_gyration(gr_segments *S, uint32_t first_slot, uint32_t n_frames, int kind, int weighted, bool want_axes, float *moments_host, float *axes_host, int *status_out) {
    gr_ctx *c = S->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    if (kind != GR_CENTER_NAIVE && kind != GR_CENTER_ESTIMATE && kind != GR_CENTER_PBC) return fail(c, GR_E_INVALID_ARG, "unknown centre kind");
    const size_t M = (size_t)S->P.count();
    const uint32_t piece_max = std::max<uint32_t>(std::min<uint32_t>(gyr_piece_frames(S), n_frames), 1u);
    const size_t axes_at = (size_t)piece_max * M * GR_GYR_MOMENTS;      // (the block: the piece's moments, then its axes)
    HIPCHK(c, S->gyr.reserve((size_t)piece_max * M * GR_GYR_FRAME_FLOATS, grbuf::exact));
    S->gyr_axes_at = axes_at;
    S->last_launches = 0; S->last_sets = 0; S->last_pieces = 0;
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, kind != GR_CENTER_NAIVE));
        {
            SlotUse use(c, s0, nb);
            HIPCHK(c, hipMemsetAsync(S->key_dev, 0xFF, nb * sizeof(unsigned long long), c->stream));
            if (!pre.all_ok) {
                for (uint32_t f = 0; f < nb; ++f) S->ok_host[f] = pre.ok(f) ? 1u : 0u;
                HIPCHK(c, hipMemcpyAsync(S->ok_dev, S->ok_host, nb * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            }
            const uint32_t *ok_dev = pre.all_ok ? nullptr : S->ok_dev;
            for (uint32_t p0 = 0; p0 < nb; p0 += piece_max) {
                const uint32_t np = std::min<uint32_t>(piece_max, nb - p0);
                gyr_launch<4>(S, grs::TEAM4, s0, np, p0, kind, weighted, ok_dev);
                gyr_launch<16>(S, grs::TEAM16, s0, np, p0, kind, weighted, ok_dev);
                gyr_launch<64>(S, grs::TEAM_WAVE, s0, np, p0, kind, weighted, ok_dev);
                gyr_launch<256>(S, grs::TEAM_BLOCK, s0, np, p0, kind, weighted, ok_dev);
                const uint64_t rows = (uint64_t)np * M;
                if (want_axes) {
                    k_gyration_axes<<<dim3((unsigned)((rows + 255u) / 256u)), dim3(256), 0, c->stream>>>(S->gyr.get(), S->gyr.get() + axes_at, rows);
                    ++S->last_launches;
                }
                HIPCHK(c, hipGetLastError());
                ++S->last_sets; ++S->last_pieces;
                if (moments_host) {
                    const size_t at = ((size_t)b0 + p0) * M;
                    HIPCHK(c, hipMemcpyAsync(moments_host + at * GR_GYR_MOMENTS, S->gyr.get(), (size_t)rows * GR_GYR_MOMENTS * sizeof(float), hipMemcpyDeviceToHost, c->stream));
                    if (axes_host) HIPCHK(c, hipMemcpyAsync(axes_host + at * GR_GYR_AXES, S->gyr.get() + axes_at, (size_t)rows * GR_GYR_AXES * sizeof(float), hipMemcpyDeviceToHost, c->stream));
                }
            }
            HIPCHK(c, hipMemcpyAsync(S->key_host, S->key_dev, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        for (uint32_t f = 0; f < nb; ++f)
            grb::close_frame(c, fe, pre, f, status_out, [&]() -> int {
                const unsigned long long key = S->key_host[f];
                if (key == GR_SEG_KEY_CLEAR) return GR_OK;
                const uint32_t idx = (uint32_t)key;
                return ((key >> 32) & 1ull) ? fail(c, GR_E_NO_MASS, "atom has no mass", idx) : fail(c, GR_E_NO_POSITION, "atom has no position", idx);
            });
    }
    return fe.finish(c);
}

}  // namespace

extern "C" {

int gr_segments_gyration_batch(gr_segments *S, uint32_t first_slot, uint32_t n_frames, int kind, int weighted, float *moments, float *axes, int *status_out) try {
    if (!S) return GR_E_INVALID_ARG;
    if (!moments) return fail(S->c, GR_E_INVALID_ARG, "segments: moments is NULL");
    return seg_gyration(S, first_slot, n_frames, kind, weighted, axes != nullptr, moments, axes, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_segments_gyration_batch_device(gr_segments *S, uint32_t first_slot, uint32_t n_frames, int kind, int weighted, int want_axes, float **moments_dev, float **axes_dev,
                                      uint64_t *n_segments, int *status_out) try {
    if (!S) return GR_E_INVALID_ARG;
    if (n_frames > gyr_piece_frames(S)) return fail(S->c, GR_E_INVALID_ARG, "segments: the device form takes at most one piece of frames (gr_segments_set_piece_frames)");
    const int st = seg_gyration(S, first_slot, n_frames, kind, weighted, want_axes != 0, nullptr, nullptr, status_out);
    if (moments_dev) *moments_dev = S->gyr.get();
    if (axes_dev) *axes_dev = want_axes && S->gyr.get() ? S->gyr.get() + S->gyr_axes_at : nullptr;
    if (n_segments) *n_segments = S->P.count();
    return st;
} catch (...) { return gr_abi_guard(); }

int gr_segments_set_piece_frames(gr_segments *S, uint32_t n) try {
    if (!S) return GR_E_INVALID_ARG;
    S->piece_frames = n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

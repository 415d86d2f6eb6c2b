// gr_gridmap.h -- GridMap: an xy tile map accumulated over batches of resident frames.
//
// Reference: GridMap (src/structures/gridmap.rs): a container of nx x ny tiles over (span_x, span_y) that the user's trajectory loop
// fills atom by atom (get_mut_at) to build density / height / thickness maps.  Here the loop is the library's: for every frame of a
// batch and every atom of a group, count[ix, iy] += 1 and, for a chosen coordinate, sum[ix, iy] += coordinate - offset[frame].
//
// The first part of this file is the map's GEOMETRY, host and device alike, and compiles without HIP (tests/test_gridmap_host.py
// includes it from a plain g++ driver).  A literal f32 restatement of the reference:
//   get_len               gridmap.rs:146-157   diff < 0 -> InvalidSpan; tile > diff || tile == 0 -> InvalidGridTile; round(diff / tile) + 1
//   x2index / y2index     gridmap.rs:715-724   round((x - span0) / tile) as isize: f32 subtraction, correctly rounded f32 division, round
//                                              half away from zero, Rust's saturating cast (NaN -> 0, +-inf / huge -> isize MAX / MIN)
//   index2x / index2y     gridmap.rs:729-738   (index as f32 * tile) + span0, product and sum rounded on their own (never an fma)
// and the LAUNCH GEOMETRY of a call (gm_launch: ranges of the group x workgroups sharing the frames of a range, the check's grid), which
// the same driver holds against a second statement of its formulas.
// The sums are 64-bit INTEGERS of the coordinate in units of 2^-20 nm (q = rint((double)v * 2^20), exact in double for every f32):
// integer adds commute, so the map is the same bit for bit whatever order the hardware applies the atomics in -- on the LDS and the
// global path, across calls and across runs.  Capacity of a tile: 2^32 contributions of 2048 nm.
//
// The second part (hipcc only) holds the kernels, the map object and its C ABI; gr_api.hip includes this file behind the context.
//   k_gm_check        read-only pass over the x rows: the first atom of the group without position, per frame (atomicMin into the
//                     frame's verdict word).  A frame with such an atom contributes NOTHING (the library's rule: a failed frame is
//                     left untouched; the reference's loop would have binned the atoms in front of the failing one).
//   k_gm_accumulate   a workgroup owns one range of the group's atoms and walks it through MANY frames of the batch.
//                     <true>:  the map is privatised in LDS (u64 sum + u32 count per tile, GR_GM_LDS_BYTES at most), every atom is
//                              two LDS atomics, and the non-zero tiles are flushed once, with one 64-bit global atomic each, when
//                              the workgroup has finished its frames
//                     <false>: maps beyond the budget, and GR_GM_FORCE_GLOBAL: 64-bit global atomics straight from the atoms
// The group is walked like the other group kernels: a contiguous group and a masked (dense scattered) one through the float4 row
// loads of gr_layout.h over their span, an index list atom by atom.  Pad atoms and atoms outside the group are never binned.
#pragma once
#include "gr_math.h"
#include <float.h>
#include <stdint.h>

#if defined(__GNUC__) && !defined(__clang__)
#define GR_GM_NOFMA __attribute__((optimize("fp-contract=off")))
#else
#define GR_GM_NOFMA
#endif

#define GR_GM_MAX_TILES (1ull << 26)
#define GR_GM_Q_SCALE 1048576.0          /* 2^20 quanta per nm */
#define GR_GM_V_LIMIT 2147483648.0f      /* |v| >= 2^31 nm is not accumulated */
#define GR_GM_LDS_BYTES (64u * 1024u)     /* LDS budget of a privatised map: 5461 tiles with sums, 16384 count-only */
#define GR_GM_CU_LDS_BYTES (160u * 1024u) /* LDS of a gfx950 CU */
#define GR_GM_RANGE_UNITS (1u << 18)      /* units of a workgroup's range at most: the u32 LDS counts of 1024 frames stay below 2^32 */
#define GR_GM_CHECK_WGS 4096u             /* k_gm_check's grid along x at most */

namespace grg {

enum { GM_OK = 0, GM_INVALID_SPAN = 1, GM_INVALID_TILE = 2, GM_INVALID_ARG = 3 };

// Rust's `f32 as isize`
GR_HD int64_t gm_sat_i64(float r) {
    if (r != r) return 0;
    if (r >= 9223372036854775808.0f) return INT64_MAX;
    if (r <= -9223372036854775808.0f) return INT64_MIN;
    return (int64_t)r;
}

// GridMap::get_len + the library's own refusals (NaN anywhere, a negative tile: GM_INVALID_ARG)
inline int gm_len(float span0, float span1, float tile, uint64_t *n) {
    if (span0 != span0 || span1 != span1 || tile != tile) return GM_INVALID_ARG;
    const float diff = span1 - span0;
    if (diff < 0.0f) return GM_INVALID_SPAN;
    if (tile < 0.0f) return GM_INVALID_ARG;
    if (tile > diff || tile == 0.0f) return GM_INVALID_TILE;
    const float r = roundf(diff / tile);
    if (r != r) { if (n) *n = 1; return GM_OK; }               // (inf / inf: `NaN as usize` is 0)
    if (n) *n = r >= 18446744073709551615.0f ? UINT64_MAX : (uint64_t)r + 1u;
    return GM_OK;
}

// x2index / y2index
GR_HD int64_t gm_coord2index(float coord, float span0, float tile) {
    const float d = coord - span0;
    const float q = d / tile;
    return gm_sat_i64(roundf(q));
}

// the same decision for a map of n <= 2^26 tiles along the axis, without 64-bit integers: is the coordinate inside, and in which tile
// (an integer-valued f32 below 2^26 converts exactly; NaN is tile 0, as in the saturating cast)
GR_HD bool gm_tile(float coord, float span0, float tile, uint32_t n, uint32_t &index) {
    const float d = coord - span0;
    const float q = d / tile;
    float r = roundf(q);
    r = (r != r) ? 0.0f : r;
    const bool in = r >= 0.0f && r < (float)n;
    index = in ? (uint32_t)r : 0u;
    return in;
}

// index2x / index2y: two roundings on both sides
GR_HD GR_GM_NOFMA float gm_index2coord(uint64_t index, float span0, float tile) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = (float)index * tile;
    return p + span0;
}

// the coordinate (already minus the frame's offset) in quanta of 2^-20 nm; false: not finite or |v| >= 2^31, the atom counts as outside
GR_HD bool gm_quant(float v, int64_t &q) {
    if (!(fabsf(v) < GR_GM_V_LIMIT)) { q = 0; return false; }
    q = (int64_t)rint((double)v * GR_GM_Q_SCALE);
    return true;
}

// mean of a tile as the library reports it
inline float gm_mean(int64_t sum_q, uint64_t count) {
    if (count == 0) return NAN;
    return (float)((double)sum_q * (1.0 / GR_GM_Q_SCALE) / (double)count);
}

// LAUNCH GEOMETRY of one segment of nb frames.  `units`: what a range is cut from (4-atom groups of a span, or list entries); lds_bytes:
// the privatised map of a workgroup, 0 on the global path.  By default: enough workgroups to fill the chip (as many per CU as the
// privatised map leaves room for, 8 at most), each with one range of the group (wx ranges of `per` units) and as many frames of the
// segment as that allows (fy workgroups walk the frames of a range, frame f by workgroup f mod fy); k_gm_check takes 256 units per
// workgroup, up to GR_GM_CHECK_WGS workgroups that stride.  range_groups / frame_groups / check_groups (gr_gridmap_set_launch) replace
// wx / fy and cap check_wgs when they are not 0; a range never exceeds GR_GM_RANGE_UNITS units whatever is asked for.
struct GmLaunch { uint32_t wx, fy, check_wgs, per; };

inline GmLaunch gm_launch(uint64_t units, uint32_t n_cus, uint64_t lds_bytes, uint32_t nb, uint32_t range_groups, uint32_t frame_groups, uint32_t check_groups) {
    if (units == 0) units = 1;
    if (nb == 0) nb = 1;
    const uint64_t per_cu = lds_bytes ? (GR_GM_CU_LDS_BYTES / lds_bytes < 8 ? GR_GM_CU_LDS_BYTES / lds_bytes : 8) : 8;
    const uint64_t target = (uint64_t)(n_cus ? n_cus : 1u) * per_cu;
    const uint64_t tiles256 = (units + 255) / 256, floor_wx = (units + GR_GM_RANGE_UNITS - 1) / GR_GM_RANGE_UNITS;
    uint64_t wx = range_groups ? (range_groups < units ? range_groups : units) : (tiles256 < target ? tiles256 : target);
    if (wx < floor_wx) wx = floor_wx;
    uint64_t fy = frame_groups ? frame_groups : (target / wx ? target / wx : 1);
    if (fy > nb) fy = nb;
    uint64_t check = tiles256 < GR_GM_CHECK_WGS ? tiles256 : GR_GM_CHECK_WGS;
    if (check_groups && check_groups < check) check = check_groups;
    GmLaunch L;
    L.wx = (uint32_t)wx; L.fy = (uint32_t)fy; L.check_wgs = (uint32_t)check; L.per = (uint32_t)((units + wx - 1) / wx);
    return L;
}

}  // namespace grg

#if defined(__HIPCC__)

#define GR_GM_SKIP 0xFFFFFFFEu            /* verdict word: the frame failed its host checks, no kernel touches it (GR_NOIDX: every atom has a position) */

struct GrGmDev {
    float x0, tx, y0, ty;                 // span0 and tile size along x and y
    uint32_t nx, ny, n_tiles;
    int value, wrap;                      // GR_GM_COUNT / _X / _Y / _Z; 1: bin the wrapped position
    unsigned long long *count, *sum;      // [n_tiles], row-major (x outer); sum holds two's-complement int64
    unsigned long long *n_out;            // [frames of the segment]
    const float *offset;                  // [frames of the segment] or NULL
    const uint32_t *verdict;              // [frames of the segment]
};

struct gr_gridmap {
    gr_ctx *c = nullptr;
    float span_x[2] = { 0, 0 }, span_y[2] = { 0, 0 }, tile[2] = { 0, 0 };
    uint64_t nx = 0, ny = 0;
    unsigned long long *count_dev = nullptr, *sum_dev = nullptr, *nout_dev = nullptr, *nout_host = nullptr;
    uint32_t *verdict_dev = nullptr, *verdict_host = nullptr;
    float *off_dev = nullptr, *off_host = nullptr;
    uint64_t lds_launches = 0, global_launches = 0;
    uint32_t range_groups = 0, frame_groups = 0, check_groups = 0;       // gr_gridmap_set_launch; 0: the default
    uint32_t last_wx = 0, last_fy = 0, last_check = 0;                   // grid of the last segment that was launched
};

namespace {

__global__ __launch_bounds__(256) void k_gm_check(const float *__restrict__ frames, size_t stride, uint32_t s0, GrSel sel, int form, uint32_t *verdict) {
    const uint32_t f = blockIdx.y;
    if (verdict[f] == GR_GM_SKIP) return;
    const float *xyz = frames + (size_t)(s0 + f) * stride;
    const uint32_t step = gridDim.x * 256u;
    uint32_t bad = GR_NOIDX;
    if (form == 1) {
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < sel.n; k += step) {
            const uint32_t i = sel.idx[k];
            const float x = xyz[gr_tile_index(i, 0)];
            if (x != x) bad = min(bad, i);
        }
    } else {
        const float4 *f4 = reinterpret_cast<const float4 *>(xyz);
        const uint32_t a0 = sel.start, a1 = sel.start + (form == 0 ? sel.n : sel.span);
        for (uint32_t g = (a0 >> 2) + blockIdx.x * 256u + threadIdx.x; g <= (a1 - 1u) >> 2; g += step) {
            const size_t b = gr_row_index(g, 0);
            const float4 r0 = f4[b], r1 = f4[b + 64];     // x of the lane's atoms: row 0 .x .y, row 1 .z .w
            const float x[4] = { r0.x, r0.y, r1.z, r1.w };
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = 4u * g + (uint32_t)k;
                const bool in = i >= a0 && i < a1 && (form == 0 || ((sel.mask[i >> 5] >> (i & 31u)) & 1u));
                if (in && x[k] != x[k]) bad = min(bad, i);
            }
        }
    }
    // (rare: a wave that has such an atom reduces and reports it, the others do nothing)
    if (__builtin_amdgcn_ballot_w64(bad != GR_NOIDX) != 0ull) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, off, 64));
        if ((threadIdx.x & 63u) == 0u) atomicMin(&verdict[f], bad);
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_gm_accumulate(const float *__restrict__ frames, size_t stride, uint32_t s0, uint32_t nf, GrSel sel, int form,
                                                       const GrBox *__restrict__ boxes, GrGmDev P) {
    extern __shared__ unsigned long long gm_lds[];
    unsigned long long *lsum = gm_lds;                                                       // [n_tiles] when a coordinate is summed
    uint32_t *lcnt = reinterpret_cast<uint32_t *>(gm_lds + (P.value ? P.n_tiles : 0u));      // [n_tiles]
    if (LDS) {
        for (uint32_t t = threadIdx.x; t < P.n_tiles; t += 256u) { lcnt[t] = 0u; if (P.value) lsum[t] = 0ull; }
        __syncthreads();
    }
    // the workgroup's range of units: 4-atom groups of the span (contiguous, masked) or list entries
    const uint32_t a0 = sel.start, a1 = sel.start + (form == 0 ? sel.n : sel.span);
    const uint32_t ubase = form == 1 ? 0u : a0 >> 2;
    const uint32_t units = form == 1 ? sel.n : ((a1 - 1u) >> 2) - (a0 >> 2) + 1u;
    const uint32_t per = (units + gridDim.x - 1u) / gridDim.x;
    const uint32_t u0 = (uint32_t)min((uint64_t)blockIdx.x * per, (uint64_t)units), u1 = (uint32_t)min((uint64_t)u0 + per, (uint64_t)units);
    for (uint32_t f = blockIdx.y; f < nf; f += gridDim.y) {
        if (P.verdict[f] != GR_NOIDX) continue;
        const float *xyz = frames + (size_t)(s0 + f) * stride;
        const GrBox &box = boxes[s0 + f];
        const float off = P.offset ? P.offset[f] : 0.0f;
        uint32_t outside = 0u;
        auto bin = [&](float x, float y, float z) {
            if (P.wrap) gr_wrap(x, y, z, box);
            uint32_t ix, iy;
            bool in = grg::gm_tile(x, P.x0, P.tx, P.nx, ix);
            in = grg::gm_tile(y, P.y0, P.ty, P.ny, iy) && in;
            int64_t q = 0;
            if (P.value) {
                const float v = (P.value == 1 ? x : P.value == 2 ? y : z) - off;
                in = grg::gm_quant(v, q) && in;
            }
            if (!in) { ++outside; return; }
            const uint32_t t = ix * P.ny + iy;
            if (LDS) {
                atomicAdd(&lcnt[t], 1u);
                if (P.value) atomicAdd(&lsum[t], (unsigned long long)q);
            } else {
                atomicAdd(&P.count[t], 1ull);
                if (P.value) atomicAdd(&P.sum[t], (unsigned long long)q);
            }
        };
        if (form == 1) {
            for (uint32_t k = u0 + threadIdx.x; k < u1; k += 256u) {
                float x, y, z;
                gr_pos_load(xyz, sel.idx[k], x, y, z);
                bin(x, y, z);
            }
        } else {
            const float4 *f4 = reinterpret_cast<const float4 *>(xyz);
            for (uint32_t u = u0 + threadIdx.x; u < u1; u += 256u) {
                const uint32_t g = ubase + u;
                float4 r0, r1, r2;
                gr_rows_load(f4, g, r0, r1, r2);
                float x[4], y[4], z[4];
                gr_rows_unpack(r0, r1, r2, x, y, z);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t i = 4u * g + (uint32_t)k;
                    const bool in = i >= a0 && i < a1 && (form == 0 || ((sel.mask[i >> 5] >> (i & 31u)) & 1u));
                    if (in) bin(x[k], y[k], z[k]);
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(outside != 0u) != 0ull) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) outside += (uint32_t)__shfl_xor((int)outside, o, 64);
            if ((threadIdx.x & 63u) == 0u) atomicAdd(&P.n_out[f], (unsigned long long)outside);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < P.n_tiles; t += 256u) {
            const uint32_t cnt = lcnt[t];
            if (cnt == 0u) continue;                       // (a tile without a count has no sum)
            atomicAdd(&P.count[t], (unsigned long long)cnt);
            if (P.value) { const unsigned long long s = lsum[t]; if (s) atomicAdd(&P.sum[t], s); }
        }
    }
}

int gm_status(int st) {
    return st == grg::GM_OK ? GR_OK : st == grg::GM_INVALID_SPAN ? GR_E_INVALID_SPAN : st == grg::GM_INVALID_TILE ? GR_E_INVALID_TILE : GR_E_INVALID_ARG;
}

int gm_dims(const float sx[2], const float sy[2], const float td[2], uint64_t *nx, uint64_t *ny) {
    int st = grg::gm_len(sx[0], sx[1], td[0], nx); if (st) return gm_status(st);
    st = grg::gm_len(sy[0], sy[1], td[1], ny); if (st) return gm_status(st);
    if (*nx > GR_GM_MAX_TILES || *ny > GR_GM_MAX_TILES || *nx * *ny > GR_GM_MAX_TILES) return GR_E_INVALID_ARG;
    return GR_OK;
}

void gm_free(gr_gridmap *m) {
    if (m->count_dev) (void)hipFree(m->count_dev);
    if (m->sum_dev) (void)hipFree(m->sum_dev);
    if (m->nout_dev) (void)hipFree(m->nout_dev);
    if (m->verdict_dev) (void)hipFree(m->verdict_dev);
    if (m->off_dev) (void)hipFree(m->off_dev);
    if (m->nout_host) (void)hipHostFree(m->nout_host);
    if (m->verdict_host) (void)hipHostFree(m->verdict_host);
    if (m->off_host) (void)hipHostFree(m->off_host);
    delete m;
}

gr_gridmap *gm_create(gr_ctx *c, const float sx[2], const float sy[2], const float td[2], int *status) {
    uint64_t nx = 0, ny = 0;
    const int st = gm_dims(sx, sy, td, &nx, &ny);
    if (st) {
        *status = fail(c, st, st == GR_E_INVALID_SPAN ? "invalid span of the grid map" : st == GR_E_INVALID_TILE ? "invalid grid tile" : "grid map: NaN span or tile, negative tile, or more than 2^26 tiles");
        return nullptr;
    }
    (void)hipSetDevice(c->device);
    gr_gridmap *m = new gr_gridmap();
    m->c = c; m->nx = nx; m->ny = ny;
    for (int k = 0; k < 2; ++k) { m->span_x[k] = sx[k]; m->span_y[k] = sy[k]; m->tile[k] = td[k]; }
    const size_t bytes = (size_t)(nx * ny) * sizeof(unsigned long long);
    bool ok = hipMalloc(&m->count_dev, bytes) == hipSuccess && hipMalloc(&m->sum_dev, bytes) == hipSuccess;
    ok = ok && hipMalloc(&m->nout_dev, GR_MAX_BATCH * sizeof(unsigned long long)) == hipSuccess;
    ok = ok && hipMalloc(&m->verdict_dev, GR_MAX_BATCH * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc(&m->off_dev, GR_MAX_BATCH * sizeof(float)) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&m->nout_host), GR_MAX_BATCH * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&m->verdict_host), GR_MAX_BATCH * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&m->off_host), GR_MAX_BATCH * sizeof(float), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMemsetAsync(m->count_dev, 0, bytes, c->stream) == hipSuccess && hipMemsetAsync(m->sum_dev, 0, bytes, c->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        gm_free(m);
        *status = fail(c, GR_E_HIP, "grid map: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return m;
}

int gm_accumulate(gr_gridmap *m, uint32_t first_slot, uint32_t n_frames, const char *group, int value, const float *offset, int flags,
                  uint64_t *n_outside, int *status_out) {
    gr_ctx *c = m->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    if (value < GR_GM_COUNT || value > GR_GM_Z) return fail(c, GR_E_INVALID_ARG, "grid map: unknown value");
    if (flags & ~(GR_GM_WRAP | GR_GM_FORCE_GLOBAL)) return fail(c, GR_E_INVALID_ARG, "grid map: unknown flag");
    const Group *g = need_group(c, group, st, true); if (!g) return st;
    const GrSel sel = make_sel(*g);
    const int form = sel.contiguous ? 0 : (sel.masked & 1u) ? 2 : 1;
    const bool wrap = (flags & GR_GM_WRAP) != 0;
    const uint32_t n_tiles = (uint32_t)(m->nx * m->ny);
    const size_t lds_bytes = (size_t)n_tiles * (value ? 12u : 4u);
    const bool lds = !(flags & GR_GM_FORCE_GLOBAL) && lds_bytes <= GR_GM_LDS_BYTES;
    // launch geometry: grg::gm_launch, per segment
    const uint64_t units = form == 1 ? (uint64_t)sel.n : (uint64_t)(((sel.start + (form == 0 ? sel.n : sel.span) - 1u) >> 2) - (sel.start >> 2)) + 1u;
    GrGmDev P;
    P.x0 = m->span_x[0]; P.tx = m->tile[0]; P.y0 = m->span_y[0]; P.ty = m->tile[1];
    P.nx = (uint32_t)m->nx; P.ny = (uint32_t)m->ny; P.n_tiles = n_tiles; P.value = value; P.wrap = wrap ? 1 : 0;
    P.count = m->count_dev; P.sum = m->sum_dev; P.n_out = m->nout_dev; P.offset = offset ? m->off_dev : nullptr; P.verdict = m->verdict_dev;
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, wrap));
        for (uint32_t f = 0; f < nb; ++f) {
            m->verdict_host[f] = pre.ok(f) ? GR_NOIDX : GR_GM_SKIP;
            m->off_host[f] = offset ? offset[b0 + f] : 0.0f;
            m->nout_host[f] = 0ull;
        }
        if (pre.any_ok) {
            SlotUse use(c, s0, nb);
            HIPCHK(c, hipMemcpyAsync(m->verdict_dev, m->verdict_host, nb * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            if (offset) HIPCHK(c, hipMemcpyAsync(m->off_dev, m->off_host, nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemsetAsync(m->nout_dev, 0, nb * sizeof(unsigned long long), c->stream));
            const grg::GmLaunch L = grg::gm_launch(units, c->n_cus, lds ? lds_bytes : 0, nb, m->range_groups, m->frame_groups, m->check_groups);
            const uint32_t wx = L.wx, fy = L.fy;
            k_gm_check<<<dim3(L.check_wgs, nb), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0, sel, form, m->verdict_dev);
            if (lds) k_gm_accumulate<true><<<dim3(wx, fy), dim3(256), lds_bytes, c->stream>>>(c->frames, c->frame_stride, s0, nb, sel, form, c->boxes_dev, P);
            else k_gm_accumulate<false><<<dim3(wx, fy), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0, nb, sel, form, c->boxes_dev, P);
            HIPCHK(c, hipGetLastError());
            if (lds) ++m->lds_launches; else ++m->global_launches;
            m->last_wx = wx; m->last_fy = fy; m->last_check = L.check_wgs;
            HIPCHK(c, hipMemcpyAsync(m->verdict_host, m->verdict_dev, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(m->nout_host, m->nout_dev, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        for (uint32_t f = 0; f < nb; ++f) {
            const int s = grb::close_frame(c, fe, pre, f, status_out, [&] { return m->verdict_host[f] != GR_NOIDX ? fail(c, GR_E_NO_POSITION, "atom has no position", m->verdict_host[f]) : (int)GR_OK; });
            if (n_outside) n_outside[b0 + f] = s == GR_OK ? m->nout_host[f] : 0ull;
        }
    }
    return fe.finish(c);
}

}  // namespace

extern "C" {

int gr_gridmap_len(const float span[2], float tile, uint64_t *n) try {
    if (!span) return GR_E_INVALID_ARG;
    uint64_t v = 0;
    const int st = gm_status(grg::gm_len(span[0], span[1], tile, &v));
    if (st == GR_OK && n) *n = v;
    return st;
} catch (...) { return gr_abi_guard(); }

int64_t gr_gridmap_coord2index(float span0, float tile, float coord) { return grg::gm_coord2index(coord, span0, tile); }
float gr_gridmap_index2coord(float span0, float tile, uint64_t index) { return grg::gm_index2coord(index, span0, tile); }

gr_gridmap *gr_gridmap_create(gr_ctx *c, const float span_x[2], const float span_y[2], const float tile_dim[2], int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    if (!span_x || !span_y || !tile_dim) { *status = fail(c, GR_E_INVALID_ARG, "grid map: NULL span or tile"); return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    return gm_create(c, span_x, span_y, tile_dim, status);
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

gr_gridmap *gr_gridmap_from_box(gr_ctx *c, uint32_t slot, const float tile_dim[2], int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    if (!tile_dim) { *status = fail(c, GR_E_INVALID_ARG, "grid map: NULL tile"); return nullptr; }
    *status = slot_check(c, slot); if (*status) return nullptr;
    // (the tile plane of a skewed cell is not defined: refused in every mode, not only the strict one)
    if (c->box_status[slot] == GR_E_NO_BOX) { *status = fail(c, GR_E_NO_BOX, "simulation box does not exist"); return nullptr; }
    if (!c->boxes_host[slot].ortho) { *status = fail(c, GR_E_NOT_ORTHOGONAL, "simulation box is not orthogonal"); return nullptr; }
    const float sx[2] = { 0.0f, c->box9_host[9 * (size_t)slot] }, sy[2] = { 0.0f, c->box9_host[9 * (size_t)slot + 1] };
    return gm_create(c, sx, sy, tile_dim, status);
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_gridmap_destroy(gr_gridmap *m) try {
    if (!m) return;
    (void)hipSetDevice(m->c->device);
    (void)hipStreamSynchronize(m->c->stream);
    gm_free(m);
} catch (...) { }

int gr_gridmap_dims(const gr_gridmap *m, uint64_t *nx, uint64_t *ny, float span_x[2], float span_y[2], float tile_dim[2]) try {
    if (!m) return GR_E_INVALID_ARG;
    if (nx) *nx = m->nx;
    if (ny) *ny = m->ny;
    for (int k = 0; k < 2; ++k) {
        if (span_x) span_x[k] = m->span_x[k];
        if (span_y) span_y[k] = m->span_y[k];
        if (tile_dim) tile_dim[k] = m->tile[k];
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_gridmap_stat(const gr_gridmap *m, int key, uint64_t *value) try {
    if (!m || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_GM_STAT_LDS_LAUNCHES: *value = m->lds_launches; return GR_OK;
    case GR_GM_STAT_GLOBAL_LAUNCHES: *value = m->global_launches; return GR_OK;
    case GR_GM_STAT_LDS_BUDGET: *value = GR_GM_LDS_BYTES; return GR_OK;
    case GR_GM_STAT_LAST_RANGE_GROUPS: *value = m->last_wx; return GR_OK;
    case GR_GM_STAT_LAST_FRAME_GROUPS: *value = m->last_fy; return GR_OK;
    case GR_GM_STAT_LAST_CHECK_GROUPS: *value = m->last_check; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

int gr_gridmap_set_launch(gr_gridmap *m, uint32_t range_groups, uint32_t frame_groups, uint32_t check_groups) try {
    if (!m) return GR_E_INVALID_ARG;
    m->range_groups = range_groups; m->frame_groups = frame_groups; m->check_groups = check_groups;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_gridmap_clear(gr_gridmap *m) try {
    if (!m) return GR_E_INVALID_ARG;
    gr_ctx *c = m->c;
    int st = busy_check(c); if (st) return st;
    (void)hipSetDevice(c->device);
    const size_t bytes = (size_t)(m->nx * m->ny) * sizeof(unsigned long long);
    HIPCHK(c, hipMemsetAsync(m->count_dev, 0, bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(m->sum_dev, 0, bytes, c->stream));
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_gridmap_accumulate_batch(gr_gridmap *m, uint32_t first_slot, uint32_t n_frames, const char *group, int value, const float *offset, int flags,
                                uint64_t *n_outside, int *status_out) try {
    if (!m) return GR_E_INVALID_ARG;
    return gm_accumulate(m, first_slot, n_frames, group, value, offset, flags, n_outside, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_gridmap_read(gr_gridmap *m, uint64_t *count, int64_t *sum_q, float *mean) try {
    if (!m) return GR_E_INVALID_ARG;
    gr_ctx *c = m->c;
    int st = busy_check(c); if (st) return st;
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)(m->nx * m->ny);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint64_t> cnt; std::vector<int64_t> sum;
    const bool need_cnt = count || mean, need_sum = sum_q || mean;
    uint64_t *cp = count; int64_t *sp = sum_q;
    if (need_cnt && !cp) { cnt.resize(n); cp = cnt.data(); }
    if (need_sum && !sp) { sum.resize(n); sp = sum.data(); }
    if (need_cnt) HIPCHK(c, hipMemcpy(cp, m->count_dev, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (need_sum) HIPCHK(c, hipMemcpy(sp, m->sum_dev, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (mean) for (size_t t = 0; t < n; ++t) mean[t] = grg::gm_mean(sp[t], cp[t]);
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

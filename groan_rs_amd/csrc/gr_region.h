// gr_region.h -- Region: geometry selections over a block of resident frames.
//
// Reference: `system.group_iter("Water")?.filter_geometry(cylinder)` (src/lib.rs:170-188, iterators.rs:994-1004, :1094-1105) or
// group_create_from_geometries (src/system/groups.rs:94-188) run every frame of a trajectory loop: which atoms of a group have a
// position and lie inside every shape, frame by frame.  Through the per-frame calls that is one launch, one synchronisation and a host
// walk of the n/8-byte mask per frame (geometry_filter, gr_api.hip).  Here the shapes are ONE object and a block of resident slots is one
// call; the per-frame lists are compacted on the device and stay there.
//
// The predicates are gr_shape_inside_pbc / gr_shape_inside_naive (gr_shape.h) unchanged.  A shape that follows a per-frame point (the
// centre of a group, say) is the stored shape moved by anchor[f]: position, base2 and base3 become stored + anchor[f], one f32 add per
// component, done on the host when the frame's shape set is written.
//
// A segment of the batch is worked in PIECES of frames so that the mask workspace stays bounded (GR_RG_MASK_BYTES, or one frame's mask
// where that alone is larger).  Three kernels per piece, over CHUNKS of GR_RG_CHUNK = 1024 ordinals of the source group (16 ballot words):
//   k_rg_mask_count   grid (chunks, frames of the piece): a workgroup owns one chunk of one frame; wave v evaluates words 4v .. 4v + 3 of
//                     the chunk (four positions in flight per lane), stores each __ballot word in mask[f][w] and adds its popcounts;
//                     the four waves' counts meet in LDS and are added in wave order: counts[f][chunk].  No atomics.  A frame that
//                     failed its host checks reads nothing and counts 0 everywhere.
//   k_rg_scan         grid (frames): one workgroup turns the frame's chunk counts into their exclusive prefixes, in place, and stores
//                     the frame's total (lane-serial stretches, a shuffle scan over the lanes, the waves through LDS in wave order).
//                     The totals go to the host -- the one read-back of a piece -- which adds them to the call's offsets and grows
//                     the list buffer to what the call holds SO FAR plus this piece (never n_frames x n_atoms).
//   k_rg_emit         grid (chunks, frames): the lane whose bit is set stores its atom index at
//                     offset[f] + prefix[f][chunk] + popcounts of the chunk's words before its own + popcount(bits below its lane).
//                     Every position is computed, none is handed out by an atomic: the list is in the source group's ordinal order and
//                     the same bits whatever the batch, the piece size, the neighbours or the run.
// The box, the frame's shape set and the verdicts come in through uniform pointers (by value and indexed at run time, a shape set costs
// 816 bytes of scratch per lane: gr_shape.h).  Every GrSel form is walked by ordinal: a contiguous group as start + j, an index list
// and a masked span through the gather list that every non-contiguous group carries.
#pragma once
#include "gr_shape.h"

#if defined(__HIPCC__)

#define GR_RG_CHUNK_WORDS 16u
#define GR_RG_CHUNK (GR_RG_CHUNK_WORDS * 64u)     /* ordinals per chunk: gr_region_stat(GR_RG_STAT_CHUNK) */
#define GR_RG_MASK_BYTES (8ull << 20)             /* mask workspace of a piece */

struct gr_region {
    gr_ctx *c = nullptr;
    GrShapeSet set;                                       // the stored shapes
    uint32_t piece_frames = 0;                            // 0: by GR_RG_MASK_BYTES
    grbuf::Dev<unsigned long long> mask;                  // [frames of a piece][words]
    grbuf::Dev<uint32_t> counts;                          // [frames of a piece][chunks]: counts, then exclusive prefixes
    grbuf::Dev<GrShapeSet> sets_dev; grbuf::Pinned<GrShapeSet> sets_host;   // [frames of a segment] with anchors, [1] without
    uint32_t *ok_dev = nullptr, *ok_host = nullptr;       // [GR_MAX_BATCH]: the frame passed its host checks
    uint32_t *tot_dev = nullptr, *tot_host = nullptr;     // [GR_MAX_BATCH]: atoms inside, per frame of a piece
    grbuf::Dev<uint32_t> list[2]; int cur = 0;            // the result: list[cur]; the other one is where it moves when it has to grow
    grbuf::Dev<uint64_t> off_dev;                         // [n_frames + 1]
    std::vector<uint64_t> off_host;                       // [n_frames + 1] of the last call
    std::vector<uint8_t> frame_ok;                        // [n_frames] of the last call
    uint64_t n_frames = 0, total = 0;                     // the last call's result (0 frames after a failed call)
    uint64_t last_launches = 0, last_pieces = 0;
};

namespace {

// grid (chunks, frames of the piece); frame f of the piece lives in slot s0 + f; sets[f * set_stride] are its shapes
__global__ __launch_bounds__(256) void k_rg_mask_count(const float *__restrict__ frames, size_t stride, uint32_t s0, GrSel sel, const GrBox *__restrict__ boxes,
                                                        const GrShapeSet *__restrict__ sets, uint32_t set_stride, const uint32_t *__restrict__ ok, uint32_t words,
                                                        unsigned long long *__restrict__ mask, uint32_t *__restrict__ counts) {
    __shared__ uint32_t lds[4];
    const uint32_t f = blockIdx.y, chunk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t cnt = 0;
    if (ok[f]) {
        const GrBox &box = boxes[s0 + f];
        const GrShapeSet &shapes = sets[(size_t)f * set_stride];
        const float *xyz = frames + (size_t)(s0 + f) * stride;
        const uint32_t w0 = chunk * GR_RG_CHUNK_WORDS + wave * 4u;
        float x[4], y[4], z[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint64_t j = (uint64_t)(w0 + (uint32_t)t) * 64u + lane;
            x[t] = NAN; y[t] = NAN; z[t] = NAN;             // (an ordinal behind the group: inside nothing, like an atom without position)
            if (j < sel.n) gr_pos_load(xyz, sel.contiguous ? sel.start + (uint32_t)j : sel.idx[j], x[t], y[t], z[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t w = w0 + (uint32_t)t;
            if (w >= words) break;
            bool in = (x[t] == x[t]);
            for (int q = 0; q < shapes.n && in; ++q)
                in = shapes.naive ? gr_shape_inside_naive(shapes.s[q], x[t], y[t], z[t]) : gr_shape_inside_pbc(shapes.s[q], x[t], y[t], z[t], box);
            const unsigned long long bits = __ballot(in);
            if (lane == 0u) mask[(size_t)f * words + w] = bits;
            cnt += (uint32_t)__popcll(bits);
        }
    }
    if (lane == 0u) lds[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0u) counts[(size_t)f * gridDim.x + chunk] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// grid (frames of the piece): counts[f][0 .. chunks) -> their exclusive prefixes, totals[f] = their sum
__global__ __launch_bounds__(256) void k_rg_scan(uint32_t *__restrict__ counts, uint32_t chunks, uint32_t *__restrict__ totals) {
    __shared__ uint32_t lds[4];
    const uint32_t f = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t *c = counts + (size_t)f * chunks;
    const uint32_t per = (chunks + 255u) / 256u;
    const uint32_t a = (uint32_t)min((uint64_t)threadIdx.x * per, (uint64_t)chunks), b = (uint32_t)min((uint64_t)a + per, (uint64_t)chunks);
    uint32_t sum = 0;
    for (uint32_t k = a; k < b; ++k) sum += c[k];
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= (uint32_t)off) incl += v;
    }
    if (lane == 63u) lds[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t v = 0; v < wave; ++v) base += lds[v];
    uint32_t run = base + (incl - sum);
    for (uint32_t k = a; k < b; ++k) { const uint32_t v = c[k]; c[k] = run; run += v; }
    if (threadIdx.x == 0u) totals[f] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// grid (chunks, frames of the piece); offsets = the call's offsets of the piece's frames; list = the call's list
__global__ __launch_bounds__(256) void k_rg_emit(GrSel sel, uint32_t words, const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ prefix,
                                                  const uint32_t *__restrict__ totals, const uint64_t *__restrict__ offsets, uint32_t *__restrict__ list) {
    const uint32_t f = blockIdx.y, chunk = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (totals[f] == 0u) return;                             // nothing inside -- or a failed frame, whose mask was never written
    const uint32_t wc = chunk * GR_RG_CHUNK_WORDS;
    if (wc + wave * 4u >= words) return;                     // the group ends in front of this wave's words
    const unsigned long long *m = mask + (size_t)f * words;
    // the chunk's words before this wave's (all of them exist, as this wave's first one does)
    uint32_t before = 0;
    for (uint32_t k = 0; k < wave * 4u; ++k) before += (uint32_t)__popcll(m[wc + k]);
    uint64_t at = offsets[f] + prefix[(size_t)f * gridDim.x + chunk];
    for (uint32_t t = 0; t < 4u; ++t) {
        const uint32_t w = wc + wave * 4u + t;
        if (w >= words) break;
        const unsigned long long bits = m[w];
        if ((bits >> lane) & 1ull) {
            const uint64_t j = (uint64_t)w * 64u + lane;
            list[at + before + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull))] = sel.contiguous ? sel.start + (uint32_t)j : sel.idx[j];
        }
        before += (uint32_t)__popcll(bits);
    }
}

void rg_free(gr_region *r) {
    if (r->ok_dev) (void)hipFree(r->ok_dev);
    if (r->tot_dev) (void)hipFree(r->tot_dev);
    if (r->ok_host) (void)hipHostFree(r->ok_host);
    if (r->tot_host) (void)hipHostFree(r->tot_host);
    delete r;                                              // (frees the grow-only buffers)
}

// the frame's shapes: the stored ones moved by (ax, ay, az)
void rg_shift(const GrShapeSet &stored, float ax, float ay, float az, GrShapeSet &out) {
    out = stored;
    for (int q = 0; q < stored.n; ++q) {
        GrShapeDev &s = out.s[q];
        s.px = s.px + ax; s.py = s.py + ay; s.pz = s.pz + az;
        if (s.kind == GR_SH_PRISM) { s.b2x = s.b2x + ax; s.b2y = s.b2y + ay; s.b2z = s.b2z + az; s.b3x = s.b3x + ax; s.b3y = s.b3y + ay; s.b3z = s.b3z + az; }
    }
}

// frames of a piece for a group of `words` ballot words
uint32_t rg_piece_frames(const gr_region *r, uint32_t words, uint32_t nb) {
    uint64_t p = r->piece_frames ? r->piece_frames : GR_RG_MASK_BYTES / ((uint64_t)std::max<uint32_t>(words, 1u) * 8u);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(p, 1), nb);
}

// the list buffer holds `keep` entries and is about to receive up to `need` in all: a bigger block takes the entries over
int rg_list_room(gr_region *r, uint64_t keep, uint64_t need) {
    gr_ctx *c = r->c;
    if (need <= r->list[r->cur].cap()) return GR_OK;
    const int other = 1 - r->cur;
    HIPCHK(c, r->list[other].reserve((size_t)need, [](size_t n) { return n + n / 2 + 64; }));      // (geometric: a call of many pieces moves its list a few times)
    if (keep) HIPCHK(c, hipMemcpyAsync(r->list[other].get(), r->list[r->cur].get(), (size_t)keep * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));            // the old block's last reader
    r->list[r->cur].release();
    r->cur = other;
    return GR_OK;
}

int rg_select(gr_region *r, uint32_t first_slot, uint32_t n_frames, const char *group, const float *anchor, uint64_t *n_inside, int *status_out) {
    gr_ctx *c = r->c;
    r->n_frames = 0; r->total = 0; r->last_launches = 0; r->last_pieces = 0;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    const Group *g = need_group(c, group ? group : "all", st); if (!g) return st;
    const GrSel sel = make_sel(*g);
    const bool naive = r->set.naive != 0;
    const uint32_t words = (uint32_t)(((uint64_t)sel.n + 63u) / 64u), chunks = (words + GR_RG_CHUNK_WORDS - 1u) / GR_RG_CHUNK_WORDS;
    const uint32_t piece_max = rg_piece_frames(r, words, std::min<uint32_t>(n_frames, GR_MAX_BATCH));
    HIPCHK(c, r->mask.reserve((size_t)piece_max * words, grbuf::exact));
    HIPCHK(c, r->counts.reserve((size_t)piece_max * chunks, grbuf::exact));
    const uint32_t n_sets = anchor ? std::min<uint32_t>(n_frames, GR_MAX_BATCH) : 1u;
    HIPCHK(c, r->sets_dev.reserve(n_sets, grbuf::exact));
    HIPCHK(c, r->sets_host.reserve(n_sets, grbuf::exact));
    HIPCHK(c, r->off_dev.reserve((size_t)n_frames + 1, grbuf::exact));
    r->off_host.assign((size_t)n_frames + 1, 0);
    r->frame_ok.assign(n_frames, 0);
    uint64_t total = 0;
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        GrShapeSet *sets = r->sets_host.get();
        if (!anchor) sets[0] = r->set;
        const uint32_t seg_b0 = b0, seg_s0 = s0;
        const grb::Prechecks pre(c, { b0, nb, s0 }, [&](uint32_t slot) -> int {
            const uint32_t f = slot - seg_s0;
            const float *a = anchor ? anchor + 3 * (size_t)(seg_b0 + f) : nullptr;
            if (a) sets[f] = r->set;
            if (a && !(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]))) return fail(c, GR_E_INVALID_ARG, "region: the frame's anchor is not finite");
            if (a) rg_shift(r->set, a[0], a[1], a[2], sets[f]);
            if (naive) return GR_OK;
            const int bs = geometry_box_check(c, slot); if (bs) return bs;
            const GrShapeSet &fs = sets[a ? f : 0u];
            for (int q = 0; q < fs.n; ++q)
                if (gr_shape_tric_walk(fs.s[q], c->boxes_host[slot]) > GR_SHAPE_WALK_MAX)
                    return fail(c, GR_E_UNSUPPORTED_BOX, "the shape reaches more lattice images of this cell than the geometry selection enumerates");
            return GR_OK;
        });
        for (uint32_t f = 0; f < nb; ++f) r->ok_host[f] = pre.ok(f) ? 1u : 0u;
        if (sel.n != 0 && pre.any_ok) {
            SlotUse use(c, s0, nb);
            HIPCHK(c, hipMemcpyAsync(r->ok_dev, r->ok_host, nb * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(r->sets_dev.get(), sets, (anchor ? nb : 1u) * sizeof(GrShapeSet), hipMemcpyHostToDevice, c->stream));
            for (uint32_t p0 = 0; p0 < nb; p0 += piece_max) {
                const uint32_t np = std::min<uint32_t>(piece_max, nb - p0);
                k_rg_mask_count<<<dim3(chunks, np), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0 + p0, sel, c->boxes_dev, r->sets_dev.get() + (anchor ? p0 : 0u),
                                                                                 anchor ? 1u : 0u, r->ok_dev + p0, words, r->mask.get(), r->counts.get());
                k_rg_scan<<<dim3(np), dim3(256), 0, c->stream>>>(r->counts.get(), chunks, r->tot_dev + p0);
                HIPCHK(c, hipGetLastError());
                HIPCHK(c, hipMemcpyAsync(r->tot_host + p0, r->tot_dev + p0, np * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                r->last_launches += 2; ++r->last_pieces;
                const uint64_t kept = total;
                for (uint32_t f = p0; f < p0 + np; ++f) { total += r->tot_host[f]; r->off_host[(size_t)b0 + f + 1] = total; }
                if (total == kept) continue;
                st = rg_list_room(r, kept, total); if (st) return st;
                HIPCHK(c, hipMemcpyAsync(r->off_dev.get() + b0 + p0, r->off_host.data() + b0 + p0, ((size_t)np + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
                k_rg_emit<<<dim3(chunks, np), dim3(256), 0, c->stream>>>(sel, words, r->mask.get(), r->counts.get(), r->tot_dev + p0, r->off_dev.get() + b0 + p0, r->list[r->cur].get());
                HIPCHK(c, hipGetLastError());
                ++r->last_launches;
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));        // (off_host is pageable and the next segment rewrites the pinned blocks)
        } else {
            for (uint32_t f = 0; f < nb; ++f) { r->tot_host[f] = 0u; r->off_host[(size_t)b0 + f + 1] = total; }
        }
        for (uint32_t f = 0; f < nb; ++f) {
            const int s = grb::close_frame(c, fe, pre, f, status_out, [] { return (int)GR_OK; });
            r->frame_ok[(size_t)b0 + f] = s == GR_OK ? 1 : 0;
            if (n_inside) n_inside[(size_t)b0 + f] = r->tot_host[f];
        }
    }
    // the offsets as a whole (pieces without an atom inside sent none)
    HIPCHK(c, hipMemcpyAsync(r->off_dev.get(), r->off_host.data(), ((size_t)n_frames + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    r->n_frames = n_frames; r->total = total;
    return fe.finish(c);
}

}  // namespace

extern "C" {

gr_region *gr_region_create(gr_ctx *c, const gr_shape *shapes, size_t n_shapes, int naive, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    if (n_shapes > GR_MAX_SHAPES || (n_shapes && !shapes)) { *status = fail(c, GR_E_INVALID_ARG, "too many shapes"); return nullptr; }
    gr_region *r = new gr_region();
    r->c = c;
    memset(&r->set, 0, sizeof r->set);
    r->set.n = (int)n_shapes; r->set.naive = naive ? 1 : 0;
    for (size_t q = 0; q < n_shapes; ++q)
        if (!shape_to_dev(shapes[q], naive, &r->set.s[q])) { delete r; *status = fail(c, GR_E_INVALID_ARG, "invalid shape"); return nullptr; }
    (void)hipSetDevice(c->device);
    bool ok = hipMalloc(&r->ok_dev, GR_MAX_BATCH * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc(&r->tot_dev, GR_MAX_BATCH * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&r->ok_host), GR_MAX_BATCH * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&r->tot_host), GR_MAX_BATCH * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
    ok = ok && r->off_dev.reserve(1, grbuf::exact) == hipSuccess && r->list[0].reserve(1, grbuf::exact) == hipSuccess;
    ok = ok && hipMemset(r->off_dev.get(), 0, sizeof(uint64_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        rg_free(r);
        *status = fail(c, GR_E_HIP, "region: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return r;
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_region_destroy(gr_region *r) try {
    if (!r) return;
    (void)hipSetDevice(r->c->device);
    (void)hipStreamSynchronize(r->c->stream);
    rg_free(r);
} catch (...) { }

int gr_region_select_batch(gr_region *r, uint32_t first_slot, uint32_t n_frames, const char *group, const float *anchor, uint64_t *n_inside, int *status_out) try {
    if (!r) return GR_E_INVALID_ARG;
    return rg_select(r, first_slot, n_frames, group, anchor, n_inside, status_out);
} catch (...) { if (r) { r->n_frames = 0; r->total = 0; } return gr_abi_guard(); }

int gr_region_read(gr_region *r, uint64_t *offsets, uint64_t *atoms, uint64_t cap, uint64_t *n_total) try {
    if (!r) return GR_E_INVALID_ARG;
    gr_ctx *c = r->c;
    int st = busy_check(c); if (st) return st;
    if (n_total) *n_total = r->total;
    if (offsets) { if (r->n_frames) memcpy(offsets, r->off_host.data(), ((size_t)r->n_frames + 1) * sizeof(uint64_t)); else offsets[0] = 0; }
    if (!atoms) return GR_OK;
    if (cap < r->total) return fail(c, GR_E_INVALID_ARG, "region: the atom buffer is smaller than the result");
    if (!r->total) return GR_OK;
    (void)hipSetDevice(c->device);
    std::vector<uint32_t> narrow((size_t)r->total);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(narrow.data(), r->list[r->cur].get(), narrow.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < narrow.size(); ++k) atoms[k] = narrow[k];
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_region_read_device(gr_region *r, const uint32_t **atoms_dev, const uint64_t **offsets_dev, uint64_t *n_frames, uint64_t *n_total) try {
    if (!r) return GR_E_INVALID_ARG;
    if (atoms_dev) *atoms_dev = r->list[r->cur].get();
    if (offsets_dev) *offsets_dev = r->off_dev.get();
    if (n_frames) *n_frames = r->n_frames;
    if (n_total) *n_total = r->total;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_region_group(gr_region *r, uint32_t frame, const char *name) try {
    if (!r) return GR_E_INVALID_ARG;
    gr_ctx *c = r->c;
    int st = busy_check(c); if (st) return st;
    if (!name_is_valid(name)) return fail(c, GR_E_INVALID_NAME, name ? name : "(null)");
    if (frame >= r->n_frames) return fail(c, GR_E_INVALID_ARG, "region: no such frame in the last selection", frame);
    if (!r->frame_ok[frame]) return fail(c, GR_E_INVALID_ARG, "region: the frame failed in the last selection", frame);
    (void)hipSetDevice(c->device);
    const uint64_t a = r->off_host[frame], n = r->off_host[(size_t)frame + 1] - a;
    std::vector<uint32_t> narrow((size_t)n);
    if (n) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(narrow.data(), r->list[r->cur].get() + a, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    const std::vector<uint64_t> picked(narrow.begin(), narrow.end());
    return install_group(c, name, grc::from_indices(picked, c->n));
} catch (...) { return gr_abi_guard(); }

int gr_region_set_piece_frames(gr_region *r, uint32_t n) try {
    if (!r) return GR_E_INVALID_ARG;
    r->piece_frames = n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_region_stat(const gr_region *r, int key, uint64_t *value) try {
    if (!r || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_RG_STAT_LAST_LAUNCHES: *value = r->last_launches; return GR_OK;
    case GR_RG_STAT_LAST_PIECES: *value = r->last_pieces; return GR_OK;
    case GR_RG_STAT_LAST_TOTAL: *value = r->total; return GR_OK;
    case GR_RG_STAT_CHUNK: *value = GR_RG_CHUNK; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

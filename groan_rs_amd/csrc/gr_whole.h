// gr_whole.h -- bond topology on the context and make_molecules_whole / make_group_whole over a batch of resident frames.
//
// Reference: System::add_bond / clear_bonds / has_bonds / create_mol_references / make_molecules_whole / make_group_whole
// (src/system/modifying.rs:235-283,338-487, src/system/mod.rs:349-377,437) and get_molecule_indices (src/system/iterating.rs:399-432).
// The topology itself is host state (gr_topology.h); the device sees one int32 per atom, uploaded once per topology:
//   ref - i (<= 0)      the atom belongs to the polyatomic molecule whose reference (lowest index) is ref
//   GR_TOPO_FARREF      a reference atom that atoms of later 256-atom tiles read
//   GR_TOPO_NONE        any other atom, and the pad atoms behind the system
//
// make_molecules_whole, one batch: the frames run in chunks that fit the Infinity Cache, each chunk as
//   k_whole_check   read-only: every molecule atom whose x is NaN does an atomicMin of (ref << 32 | breadth-first rank) into its
//                   frame's word -- the smallest such key is the atom the reference stops on (the molecule with the lowest
//                   reference, in it the reference itself, else the first atom in breadth-first order)
//   k_whole_place   frames whose word is still clear: one wave per tile; reference atoms become gr_wrap(p), the wave publishes
//                   them in LDS, every other molecule atom becomes ref_w + gr_vector_to(ref_w, p) with ref_w from LDS when its
//                   reference lies in the tile, else gathered from the slot and wrapped again
//   k_whole_far     only in non-orthogonal cells: the references read across tiles are wrapped after the placement
// and ONE read-back of the words per call.  Why a gathered reference may be read while its own lane stores it: in an orthorhombic
// cell every coordinate is wrapped on its own and wrap is idempotent bit for bit (tests/test_topology_host.py walks the edge
// values), so a read before, after or between the three coordinate stores yields the same ref_w.  A triclinic wrap couples the
// coordinates (z decides the shift of x and y): a torn read would not be safe, so there those references are left alone by the
// placement and wrapped by k_whole_far behind it.
#pragma once
#include "gr_topology.h"

#define GR_WHOLE_CLEAR 0xFFFFFFFFFFFFFFFFull    /* frame word: no molecule atom without position */
#define GR_WHOLE_SKIP  0xFFFFFFFFFFFFFFFEull    /* frame word: the frame failed its host checks, no kernel touches it */
#define GR_WHOLE_CHUNK_BYTES (96ull << 20)      /* frames of a chunk: positions that fit the 256 MiB Infinity Cache with room to spare */

struct GrWhole {
    grt::GrTopology topo;
    uint64_t dev_version = ~0ull;       // topology version of the device map
    int32_t *map_dev = nullptr;         // [n_pad]
    uint32_t *rank_dev = nullptr;       // [n_pad] breadth-first rank in the molecule (read only for atoms without position)
    grbuf::Dev<uint32_t> far_dev; uint64_t n_far = 0;   // GR_TOPO_FARREF atoms
    unsigned long long *words_dev = nullptr, *words_host = nullptr; // [GR_MAX_BATCH] frame words (device, pinned)
    explicit GrWhole(uint64_t n) : topo(n) {}
};

namespace {

__device__ __forceinline__ bool gr_whole_in_mol(int32_t o) { return o <= 0 || o == GR_TOPO_FARREF; }

__global__ __launch_bounds__(256) void k_whole_check(const float *__restrict__ frames, size_t stride, uint32_t s0, uint32_t n_groups,
                                                     const int32_t *__restrict__ map, const uint32_t *__restrict__ rank, unsigned long long *words) {
    const uint32_t f = blockIdx.y;
    if (words[f] == GR_WHOLE_SKIP) return;
    const float4 *f4 = reinterpret_cast<const float4 *>(frames + (size_t)(s0 + f) * stride);
    for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < n_groups; g += gridDim.x * 256u) {
        const size_t b = gr_row_index(g, 0);
        const float4 r0 = f4[b], r1 = f4[b + 64];     // x of the lane's atoms: row 0 .x .y, row 1 .z .w
        const float x[4] = { r0.x, r0.y, r1.z, r1.w };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x[k] == x[k]) continue;
            const uint32_t i = 4u * g + (uint32_t)k;
            const int32_t o = map[i];
            if (!gr_whole_in_mol(o)) continue;
            const uint32_t ref = o == GR_TOPO_FARREF ? i : (uint32_t)((int64_t)i + o);
            atomicMin(&words[f], ((unsigned long long)ref << 32) | rank[i]);
        }
    }
}

__global__ __launch_bounds__(64) void k_whole_place(float *__restrict__ frames, size_t stride, uint32_t s0, const int32_t *__restrict__ map,
                                                    const unsigned long long *__restrict__ words, const GrBox *__restrict__ boxes, int keep_far) {
    const uint32_t f = blockIdx.y;
    if (words[f] != GR_WHOLE_CLEAR) return;
    __shared__ float wx[256], wy[256], wz[256];
    const GrBox &b = boxes[s0 + f];
    float *xyz = frames + (size_t)(s0 + f) * stride;
    float4 *f4 = reinterpret_cast<float4 *>(xyz);
    const uint32_t lane = threadIdx.x, g = blockIdx.x * 64u + lane, base = blockIdx.x << 8;
    const int4 m = reinterpret_cast<const int4 *>(map)[g];
    const int32_t o[4] = { m.x, m.y, m.z, m.w };
    const bool mine = gr_whole_in_mol(o[0]) || gr_whole_in_mol(o[1]) || gr_whole_in_mol(o[2]) || gr_whole_in_mol(o[3]);
    if (__builtin_amdgcn_ballot_w64(mine) == 0ull) return;     // (wave-uniform: the only wave of the workgroup leaves before the barrier)
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    if (mine) gr_rows_load(f4, g, r0, r1, r2);
    float x[4], y[4], z[4];
    gr_rows_unpack(r0, r1, r2, x, y, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (o[k] != 0 && o[k] != GR_TOPO_FARREF) continue;
        float px = x[k], py = y[k], pz = z[k];
        gr_wrap(px, py, pz, b);
        wx[4u * lane + k] = px; wy[4u * lane + k] = py; wz[4u * lane + k] = pz;
        if (o[k] == 0 || !keep_far) { x[k] = px; y[k] = py; z[k] = pz; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (o[k] >= 0) continue;
        const uint32_t i = base + 4u * lane + (uint32_t)k, r = (uint32_t)((int64_t)i + o[k]);
        float rx, ry, rz;
        if (r >= base) { rx = wx[r - base]; ry = wy[r - base]; rz = wz[r - base]; }
        else { gr_pos_load(xyz, r, rx, ry, rz); gr_wrap(rx, ry, rz, b); }
        float vx, vy, vz;
        gr_vector_to(rx, ry, rz, x[k], y[k], z[k], b, vx, vy, vz);
        x[k] = rx + vx; y[k] = ry + vy; z[k] = rz + vz;
    }
    if (mine) {
        gr_rows_pack(x, y, z, r0, r1, r2);
        gr_rows_store(f4, g, r0, r1, r2);
    }
}

// non-orthogonal cells: the references that later tiles read, wrapped once every frame of the chunk has been placed
__global__ __launch_bounds__(256) void k_whole_far(float *__restrict__ frames, size_t stride, uint32_t s0, const uint32_t *__restrict__ far, uint32_t n_far,
                                                   const unsigned long long *__restrict__ words, const GrBox *__restrict__ boxes) {
    const uint32_t f = blockIdx.y, k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_far || words[f] != GR_WHOLE_CLEAR) return;
    float *xyz = frames + (size_t)(s0 + f) * stride;
    float x, y, z;
    gr_pos_load(xyz, far[k], x, y, z);
    gr_wrap(x, y, z, boxes[s0 + f]);
    gr_pos_store(xyz, far[k], x, y, z);
}

// make_group_whole: every atom of the selection becomes c + gr_vector_to(c, p), c = the frame's estimated centre (state[f].com)
//   form 0  contiguous block: 4-atom groups of its span, whole rows
//   form 1  gather list: one lane per listed atom
//   form 2  dense scattered selection: 4-atom groups of its span, the bit mask picks the atoms
__global__ __launch_bounds__(256) void k_group_whole(float *__restrict__ frames, size_t stride, uint32_t s0, GrSel sel, const GrBox *__restrict__ boxes,
                                                     const GrFrameState *__restrict__ state, int form) {
    const uint32_t f = blockIdx.y;
    if (state[f].status != 0) return;
    const GrBox &b = boxes[s0 + f];
    const float cx = state[f].com[0], cy = state[f].com[1], cz = state[f].com[2];
    float *xyz = frames + (size_t)(s0 + f) * stride;
    const uint32_t step = gridDim.x * 256u;
    if (form == 1) {
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < sel.n; k += step) {
            const uint32_t i = sel.idx[k];
            float x, y, z, vx, vy, vz;
            gr_pos_load(xyz, i, x, y, z);
            gr_vector_to(cx, cy, cz, x, y, z, b, vx, vy, vz);
            gr_pos_store(xyz, i, cx + vx, cy + vy, cz + vz);
        }
        return;
    }
    float4 *f4 = reinterpret_cast<float4 *>(xyz);
    const uint32_t a0 = sel.start, a1 = sel.start + (form == 0 ? sel.n : sel.span);
    for (uint32_t g = (a0 >> 2) + blockIdx.x * 256u + threadIdx.x; g <= (a1 - 1u) >> 2; g += step) {
        float4 r0, r1, r2;
        gr_rows_load(f4, g, r0, r1, r2);
        float x[4], y[4], z[4];
        gr_rows_unpack(r0, r1, r2, x, y, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = 4u * g + (uint32_t)k;
            const bool in = i >= a0 && i < a1 && (form == 0 || ((sel.mask[i >> 5] >> (i & 31u)) & 1u));
            if (!in) continue;
            float vx, vy, vz;
            gr_vector_to(cx, cy, cz, x[k], y[k], z[k], b, vx, vy, vz);
            x[k] = cx + vx; y[k] = cy + vy; z[k] = cz + vz;
        }
        gr_rows_pack(x, y, z, r0, r1, r2);
        gr_rows_store(f4, g, r0, r1, r2);
    }
}

GrWhole &whole_of(gr_ctx *c) {
    if (!c->whole) c->whole = new GrWhole(c->n);
    return *c->whole;
}

// the device map of the current topology (once per topology: after a bond change, on the next make_molecules_whole)
int whole_upload(gr_ctx *c, GrWhole &W) {
    if (W.map_dev && W.dev_version == W.topo.version) return GR_OK;
    std::vector<int32_t> map;
    uint64_t n_far = 0;
    W.topo.map(c->n_pad, map, &n_far);
    std::vector<uint32_t> rank(c->n_pad, 0u), far;
    std::copy(W.topo.rank.begin(), W.topo.rank.end(), rank.begin());
    for (uint64_t a = 0; a < c->n; ++a) if (map[a] == GR_TOPO_FARREF) far.push_back((uint32_t)a);
    HIPCHK(c, hipStreamSynchronize(c->stream));            // (kernels of an earlier call may still read the old map)
    if (!W.map_dev) {
        HIPCHK(c, hipMalloc(&W.map_dev, c->n_pad * sizeof(int32_t)));
        HIPCHK(c, hipMalloc(&W.rank_dev, c->n_pad * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc(&W.words_dev, GR_MAX_BATCH * sizeof(unsigned long long)));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void **>(&W.words_host), GR_MAX_BATCH * sizeof(unsigned long long), hipHostMallocDefault));
    }
    HIPCHK(c, W.far_dev.reserve(far.size(), grbuf::exact));
    HIPCHK(c, hipMemcpy(W.map_dev, map.data(), c->n_pad * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(W.rank_dev, rank.data(), c->n_pad * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!far.empty()) HIPCHK(c, hipMemcpy(W.far_dev.get(), far.data(), far.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    W.n_far = far.size();
    W.dev_version = W.topo.version;
    return GR_OK;
}

int topo_status(gr_ctx *c, int st, uint64_t i, uint64_t j, uint64_t bad) {
    if (st == grt::TOPO_INVALID_BOND) {
        c->counts[0] = i; c->counts[1] = j;
        return fail(c, GR_E_INVALID_BOND, "invalid bond", i);
    }
    if (st == grt::TOPO_OUT_OF_RANGE) return fail(c, GR_E_OUT_OF_RANGE, "atom index out of range", bad);
    return GR_OK;
}

int molecules_whole_batch(gr_ctx *c, uint32_t first_slot, uint32_t n_frames, int *status_out) {
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    GrWhole &W = whole_of(c);
    W.topo.molecules();
    const bool any_mol = !W.topo.refs.empty();
    if (any_mol) { st = whole_upload(c, W); if (st) return st; }
    const size_t frame_bytes = c->frame_stride * sizeof(float);
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, GR_WHOLE_CHUNK_BYTES / frame_bytes);
    const uint32_t n_groups = (uint32_t)(c->n_pad >> 2), n_tiles = (uint32_t)(c->n_pad >> 8);
    const uint32_t check_wgs = std::min<uint32_t>((n_groups + 255u) / 256u, 4096u);
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, true));           // simbox_check first, even without bonds (modifying.rs:343-344)
        if (any_mol && pre.any_ok) {
            SlotUse use(c, s0, nb);
            for (uint32_t f = 0; f < nb; ++f) W.words_host[f] = pre.ok(f) ? GR_WHOLE_CLEAR : GR_WHOLE_SKIP;
            HIPCHK(c, hipMemcpyAsync(W.words_dev, W.words_host, nb * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
            for (uint32_t a = 0; a < nb; a += chunk) {
                const uint32_t k = std::min(chunk, nb - a);
                bool tric = false;
                for (uint32_t f = a; f < a + k; ++f) tric = tric || (pre.ok(f) && !c->boxes_host[s0 + f].ortho);
                const int keep_far = tric && W.n_far ? 1 : 0;
                k_whole_check<<<dim3(check_wgs, k), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0 + a, n_groups, W.map_dev, W.rank_dev, W.words_dev + a);
                k_whole_place<<<dim3(n_tiles, k), dim3(64), 0, c->stream>>>(c->frames, c->frame_stride, s0 + a, W.map_dev, W.words_dev + a, c->boxes_dev, keep_far);
                if (keep_far)
                    k_whole_far<<<dim3((uint32_t)((W.n_far + 255) / 256), k), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0 + a, W.far_dev.get(), (uint32_t)W.n_far,
                                                                                                    W.words_dev + a, c->boxes_dev);
                HIPCHK(c, hipGetLastError());
            }
            HIPCHK(c, hipMemcpyAsync(W.words_host, W.words_dev, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        for (uint32_t f = 0; f < nb; ++f)
            grb::close_frame(c, fe, pre, f, status_out, [&]() -> int {
                if (!any_mol || W.words_host[f] == GR_WHOLE_CLEAR) return GR_OK;
                const uint64_t ref = W.words_host[f] >> 32, rk = W.words_host[f] & 0xFFFFFFFFull;
                return fail(c, GR_E_NO_POSITION, "atom has no position", W.topo.mol_atom(W.topo.mol_of[ref], rk));
            });
    }
    return fe.finish(c);
}

int group_whole_batch(gr_ctx *c, uint32_t first_slot, uint32_t n_frames, const char *group, int *status_out) {
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    // group_estimate_center first (modifying.rs:449): its checks in its order -- group exists, non-empty, box, positions
    const Group *g = need_group(c, group, st, true); if (!g) return st;
    const GrSel sel = make_sel(*g);
    const int form = sel.contiguous ? 0 : (sel.masked & 1u) ? 2 : 1;
    const uint64_t units = form == 1 ? (uint64_t)sel.n : ((uint64_t)(form == 0 ? sel.n : sel.span) + 3) / 4 + 1;
    const uint32_t nwg = (uint32_t)std::min<uint64_t>((units + 255) / 256, 4096);
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, true));
        SlotUse use(c, s0, nb);
        st = states_from_prechecks(c, pre); if (st) return st;
        st = center_stage(c, s0, nb, sel, 1, 0, 1, 1); if (st) return st;      // as gr_group_center_batch(GR_CENTER_ESTIMATE, weighted 0)
        k_group_whole<<<dim3(nwg, nb), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0, sel, c->boxes_dev, c->state_dev, form);
        HIPCHK(c, hipGetLastError());
        st = fetch_states(c, nb); if (st) return st;
        for (uint32_t f = 0; f < nb; ++f) grb::close_frame(c, fe, pre, f, status_out, [&] { return frame_status(c, c->state_host[f]); });
    }
    return fe.finish(c);
}

}  // namespace

static void whole_release(gr_ctx *c) {
    GrWhole *W = c->whole;
    if (!W) return;
    if (W->map_dev) (void)hipFree(W->map_dev);
    if (W->rank_dev) (void)hipFree(W->rank_dev);
    if (W->words_dev) (void)hipFree(W->words_dev);
    if (W->words_host) (void)hipHostFree(W->words_host);
    delete W;
    c->whole = nullptr;
}

extern "C" {

int gr_add_bond(gr_ctx *c, uint64_t i, uint64_t j) try {
    if (!c) return GR_E_INVALID_ARG;
    int st = busy_check(c); if (st) return st;
    uint64_t bad = 0;
    return topo_status(c, whole_of(c).topo.add_bond(i, j, &bad), i, j, bad);
} catch (...) { return gr_abi_guard(); }

int gr_add_bonds(gr_ctx *c, const uint64_t *pairs, uint64_t n_pairs) try {
    if (!c) return GR_E_INVALID_ARG;
    if (!pairs && n_pairs) return fail(c, GR_E_INVALID_ARG, "pairs is NULL");
    int st = busy_check(c); if (st) return st;
    if (n_pairs == 0) return GR_OK;
    uint64_t bad = 0, which = 0;
    st = whole_of(c).topo.add_bonds(pairs, pairs + 1, n_pairs, 2, &bad, &which);
    return topo_status(c, st, st ? pairs[2 * which] : 0, st ? pairs[2 * which + 1] : 0, bad);
} catch (...) { return gr_abi_guard(); }

int gr_clear_bonds(gr_ctx *c) try {
    if (!c) return GR_E_INVALID_ARG;
    int st = busy_check(c); if (st) return st;
    whole_of(c).topo.clear();
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_has_bonds(const gr_ctx *c) try {
    if (!c || !c->whole) return 0;
    return c->whole->topo.has_bonds() ? 1 : 0;
} catch (...) { return 0; }

int gr_mol_references(gr_ctx *c, uint64_t *out, uint64_t cap, uint64_t *n) try {
    if (!c) return GR_E_INVALID_ARG;
    GrWhole &W = whole_of(c);
    W.topo.molecules();
    const uint64_t m = W.topo.refs.size();
    if (n) *n = m;
    if (out) for (uint64_t k = 0; k < m && k < cap; ++k) out[k] = W.topo.refs[k];
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_molecule_atoms(gr_ctx *c, uint64_t index, uint64_t *out, uint64_t cap, uint64_t *n) try {
    if (!c) return GR_E_INVALID_ARG;
    std::vector<uint32_t> order;
    if (whole_of(c).topo.molecule_indices(index, order) != grt::TOPO_OK) return fail(c, GR_E_OUT_OF_RANGE, "atom index out of range", index);
    if (n) *n = order.size();
    if (out) for (uint64_t k = 0; k < order.size() && k < cap; ++k) out[k] = order[k];
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_make_molecules_whole(gr_ctx *c, uint32_t slot) try {
    return molecules_whole_batch(c, slot, 1, nullptr);
} catch (...) { return gr_abi_guard(); }

int gr_make_molecules_whole_batch(gr_ctx *c, uint32_t first_slot, uint32_t n_frames, int *status_out) try {
    return molecules_whole_batch(c, first_slot, n_frames, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_make_group_whole(gr_ctx *c, uint32_t slot, const char *group) try {
    return group_whole_batch(c, slot, 1, group, nullptr);
} catch (...) { return gr_abi_guard(); }

int gr_make_group_whole_batch(gr_ctx *c, uint32_t first_slot, uint32_t n_frames, const char *group, int *status_out) try {
    return group_whole_batch(c, first_slot, n_frames, group, status_out);
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

// gr_segments.h -- Segments: a partition of atoms into many small groups (one per residue, per molecule, per explicit list) and the
// centres of ALL of them, for a block of resident frames, in one set of launches.
//
// Reference: the loop `for part in group_split_by_resid(..) { group_get_com(part) }` (src/system/groups.rs:344-435, :514-558) or
// `for mol in molecule_iter(..)` (src/system/iterating.rs:238-245) run every frame: lipid centres for membrane maps, per-residue
// centres of a protein, water molecule centres.  Through the per-group calls that is one launch per part per frame.
//
// The first part of this file is the PARTITION, host only: it compiles without HIP (tests/test_segments_host.py includes it from a
// plain g++ driver).  An ordered list of M non-empty, strictly ascending atom lists, stored as CSR -- off[M + 1], a flat uint32
// atom list, and per segment whether it is contiguous with its first atom.  Segments may overlap, atoms may belong to none.
//   from_lists       explicit lists
//   from_labels      group_split_by_resid / _by_resname (groups.rs:391-435, :514-558): the atoms in index order, an atom joins the
//                    segment of its label, a label seen for the first time opens a new segment at the END (IndexMap order: "the
//                    order of residues in the system"); atoms of one label that are not adjacent land in the same segment
//   from_molecules   one segment per molecule of the bond topology, ordered by lowest atom, atoms ascending; an atom without bonds
//                    is a segment of its own (what molecule_iter yields for it)
// Segments are sorted (stably) into TEAM CLASSES by size: a segment is owned by exactly one team of lanes.
//   <= 4 atoms: 4 lanes     <= 16: 16 lanes     <= 4096 (GR_SMALL_MAX_DEFAULT): one wave     larger: one 256-lane workgroup
//
// The second part (hipcc only) holds the kernel, the object and its C ABI; gr_api.hip includes this file behind the context.
//   k_segment_centers<TEAM>   team t of frame f walks its segment with gr_center_atom<KIND> (the per-atom arithmetic of every other
//                    centre path), adds the f32 terms in f64, reduces the totals over the team with __shfl_xor in a fixed tree (the
//                    workgroup class: its four waves' totals through LDS, added in wave order) and closes with gr_center_close.
//                    Both stages of a PBC centre -- the unweighted Bai-Breen estimate, then the unwrapped mean about it
//                    (iterators.rs:1404-1438) -- run back to back inside the team: no grid-wide step, no atomics on the sums.  A
//                    segment's result therefore depends on its atoms, its class and the frame only: not on its neighbours, the
//                    batch or the run (float atomics add in arrival order; none are used).
//                    The team's first lane stores out[f][s][0..2]; a failing segment stores NaN and takes part in the frame's first
//                    error with an integer atomicMin on a 64-bit key (segment ordinal high, then mass-or-position, then the atom):
//                    integer min does not depend on order either.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "gr_topology.h"

#define GR_SEG_TEAM4_MAX 4u
#define GR_SEG_TEAM16_MAX 16u
#define GR_SEG_WAVE_MAX 4096u                 /* = GR_SMALL_MAX_DEFAULT */
#define GR_SEG_MAX_SEGMENTS (1ull << 30)      /* the ordinal's share of the error key */
#define GR_SEG_MAX_LIST 0xFFFFFFFFull         /* entries of the flat atom list (32-bit offsets on the device) */
#define GR_SEG_CONTIGUOUS 0x80000000u         /* Rec::n_flag: atoms first .. first + n - 1, the list is not read */

namespace grs {

enum { SEG_OK = 0, SEG_INVALID_ARG = 1, SEG_EMPTY = 2, SEG_OUT_OF_RANGE = 3 };
enum { TEAM4 = 0, TEAM16 = 1, TEAM_WAVE = 2, TEAM_BLOCK = 3, N_CLASSES = 4 };

inline int team_class(uint64_t size) {
    return size <= GR_SEG_TEAM4_MAX ? TEAM4 : size <= GR_SEG_TEAM16_MAX ? TEAM16 : size <= GR_SEG_WAVE_MAX ? TEAM_WAVE : TEAM_BLOCK;
}

// what a team reads about its segment: one 16-byte load
struct alignas(16) Rec {
    uint32_t begin;      // contiguous: the first atom; else the segment's offset into the flat atom list
    uint32_t n_flag;     // atoms | GR_SEG_CONTIGUOUS
    uint32_t ordinal;    // the segment's place in the partition (where its result goes)
    uint32_t pad;
};

struct Partition {
    std::vector<uint64_t> off;           // [M + 1]
    std::vector<uint32_t> atoms;         // flat, ascending inside a segment
    std::vector<uint8_t> contiguous;     // [M]
    uint64_t class_count[N_CLASSES] = { 0, 0, 0, 0 };

    uint64_t count() const { return off.empty() ? 0 : off.size() - 1; }
    uint64_t size(uint64_t s) const { return off[s + 1] - off[s]; }
    void clear() { off.clear(); atoms.clear(); contiguous.clear(); for (uint64_t &c : class_count) c = 0; }

    // the flags and class counts of the lists as they stand
    void finish() {
        const uint64_t m = count();
        contiguous.assign(m, 0);
        for (uint64_t &c : class_count) c = 0;
        for (uint64_t s = 0; s < m; ++s) {
            const uint64_t n = size(s);
            contiguous[s] = (uint64_t)atoms[off[s + 1] - 1] - atoms[off[s]] + 1 == n ? 1 : 0;
            ++class_count[team_class(n)];
        }
    }
    // the device records, the classes one after the other (class k: recs[start[k] .. start[k + 1])), segments in order inside a class
    void records(std::vector<Rec> &recs, uint64_t start[N_CLASSES + 1]) const {
        const uint64_t m = count();
        start[0] = 0;
        for (int k = 0; k < N_CLASSES; ++k) start[k + 1] = start[k] + class_count[k];
        uint64_t next[N_CLASSES];
        for (int k = 0; k < N_CLASSES; ++k) next[k] = start[k];
        recs.assign(m, Rec{ 0, 0, 0, 0 });
        for (uint64_t s = 0; s < m; ++s) {
            const uint64_t n = size(s);
            Rec &r = recs[next[team_class(n)]++];
            r.begin = contiguous[s] ? atoms[off[s]] : (uint32_t)off[s];
            r.n_flag = (uint32_t)n | (contiguous[s] ? GR_SEG_CONTIGUOUS : 0u);
            r.ordinal = (uint32_t)s;
        }
    }
};

// explicit lists: offsets[n_segments + 1] into `atoms`.  NULL pointers, offsets that decrease, a list that is not strictly ascending:
// SEG_INVALID_ARG; no segment or an empty one: SEG_EMPTY; an atom >= n_atoms: SEG_OUT_OF_RANGE with *bad = the atom
inline int from_lists(const uint64_t *offsets, const uint64_t *atoms, uint64_t n_segments, uint64_t n_atoms, Partition &P, uint64_t *bad) {
    P.clear();
    if (!offsets || !atoms) return SEG_INVALID_ARG;
    if (n_segments == 0) return SEG_EMPTY;
    if (n_segments > GR_SEG_MAX_SEGMENTS) return SEG_INVALID_ARG;
    for (uint64_t s = 0; s < n_segments; ++s) {
        if (offsets[s + 1] < offsets[s]) return SEG_INVALID_ARG;
        if (offsets[s + 1] == offsets[s]) return SEG_EMPTY;
    }
    const uint64_t base = offsets[0], total = offsets[n_segments] - base;
    if (total > GR_SEG_MAX_LIST) return SEG_INVALID_ARG;
    for (uint64_t s = 0; s < n_segments; ++s)
        for (uint64_t k = offsets[s]; k < offsets[s + 1]; ++k) {
            if (atoms[k] >= n_atoms) { if (bad) *bad = atoms[k]; return SEG_OUT_OF_RANGE; }
            if (k > offsets[s] && atoms[k] <= atoms[k - 1]) return SEG_INVALID_ARG;
        }
    P.off.resize(n_segments + 1);
    for (uint64_t s = 0; s <= n_segments; ++s) P.off[s] = offsets[s] - base;
    P.atoms.resize(total);
    for (uint64_t k = 0; k < total; ++k) P.atoms[k] = (uint32_t)atoms[base + k];
    P.finish();
    return SEG_OK;
}

// group_split_by_resid / _by_resname: `group` = the group's atoms in ascending order (NULL: all n_atoms atoms), labels[n_atoms]
inline int from_labels(const uint64_t *group, uint64_t n_group, uint64_t n_atoms, const uint64_t *labels, Partition &P) {
    P.clear();
    if (!labels) return SEG_INVALID_ARG;
    const uint64_t n = group ? n_group : n_atoms;
    if (n == 0) return SEG_EMPTY;
    if (n > GR_SEG_MAX_LIST) return SEG_INVALID_ARG;
    std::unordered_map<uint64_t, uint32_t> seg_of;              // label -> segment, in order of first appearance
    std::vector<uint32_t> which(n);
    std::vector<uint64_t> sizes;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t a = group ? group[k] : k;
        const auto it = seg_of.emplace(labels[a], (uint32_t)sizes.size());
        if (it.second) sizes.push_back(0);
        which[k] = it.first->second;
        ++sizes[which[k]];
    }
    if (sizes.size() > GR_SEG_MAX_SEGMENTS) { return SEG_INVALID_ARG; }
    P.off.assign(sizes.size() + 1, 0);
    for (size_t s = 0; s < sizes.size(); ++s) P.off[s + 1] = P.off[s] + sizes[s];
    std::vector<uint64_t> fill(P.off.begin(), P.off.end() - 1);
    P.atoms.resize(n);
    for (uint64_t k = 0; k < n; ++k) P.atoms[fill[which[k]]++] = (uint32_t)(group ? group[k] : k);   // (index order: ascending inside a segment)
    P.finish();
    return SEG_OK;
}

// one segment per molecule of the topology as it is NOW (a snapshot), ordered by lowest atom; atoms without bonds on their own
inline int from_molecules(grt::GrTopology &topo, Partition &P) {
    P.clear();
    if (topo.n == 0) return SEG_EMPTY;
    if (topo.n > GR_SEG_MAX_SEGMENTS) return SEG_INVALID_ARG;
    topo.molecules();
    P.off.assign(1, 0);
    P.atoms.reserve(topo.n);
    for (uint64_t a = 0; a < topo.n; ++a) {
        const uint32_t m = topo.mol_of[a];
        if (m == UINT32_MAX) P.atoms.push_back((uint32_t)a);
        else if (topo.refs[m] != a) continue;                  // (listed with its molecule's lowest atom, the reference)
        else {
            const size_t first = P.atoms.size();
            P.atoms.insert(P.atoms.end(), topo.order.begin() + (std::ptrdiff_t)topo.mol_start[m], topo.order.begin() + (std::ptrdiff_t)topo.mol_start[m + 1]);
            std::sort(P.atoms.begin() + (std::ptrdiff_t)first, P.atoms.end());
        }
        P.off.push_back(P.atoms.size());
    }
    P.finish();
    return SEG_OK;
}

}  // namespace grs

#if defined(__HIPCC__)

static_assert(GR_SEG_WAVE_MAX == GR_SMALL_MAX_DEFAULT, "the wave class takes what the single-wave kernels take");

#define GR_SEG_MAX_DEVICE_FRAMES GR_MAX_BATCH /* gr_segments_center_batch_device: one segment of the batch, so `out` holds all of it */
static_assert(GR_SEG_MAX_DEVICE_FRAMES == 1024, "include/groan_hip.h documents 1 024 frames for the device form");
#define GR_SEG_KEY_CLEAR 0xFFFFFFFFFFFFFFFFull

struct gr_segments {
    gr_ctx *c = nullptr;
    grs::Partition P;
    uint64_t start[grs::N_CLASSES + 1] = { 0, 0, 0, 0, 0 };
    grs::Rec *recs_dev = nullptr;
    uint32_t *atoms_dev = nullptr;
    grbuf::Dev<float> out;                               // [frames of a segment of the batch][M][3]
    unsigned long long *key_dev = nullptr, *key_host = nullptr;   // [GR_MAX_BATCH]: the frames' first errors
    uint32_t *ok_dev = nullptr, *ok_host = nullptr;               // [GR_MAX_BATCH]: the frame passed its host checks
    uint64_t last_launches = 0, last_sets = 0;
    // gr_gyration.h: the device block of a piece of frames ([piece][M][10] moments, then [piece][M][12] axes from gyr_axes_at on)
    grbuf::Dev<float> gyr;
    size_t gyr_axes_at = 0;
    uint32_t piece_frames = 0;                           // 0: by GR_GYR_BLOCK_BYTES
    uint64_t last_pieces = 0;
};

namespace {

template <int W>
__device__ __forceinline__ double gr_seg_team_sum(double v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);      // (teams are aligned: lane ^ off stays inside)
    return v;
}
template <int W>
__device__ __forceinline__ uint32_t gr_seg_team_min(uint32_t x) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) { const uint32_t y = (uint32_t)__shfl_xor((int)x, off, 64); x = y < x ? y : x; }
    return x;
}

// one stage of a centre of one segment by its team: afterwards EVERY lane of the team holds the closed state
// (list: the segment's atoms, NULL when it is contiguous from `first`; lds: the workgroup class's exchange block of this stage)
template <int KIND, int TEAM, int U>
__device__ __forceinline__ void gr_seg_stage(const float *__restrict__ xyz, const float *__restrict__ masses, const uint32_t *__restrict__ list, const uint32_t first,
                                             const uint32_t n, const GrBox &box, const int weighted, const int mass_first, const int target, GrFrameState &st,
                                             const uint32_t tl, double *lds) {
    const float PI_X2 = 3.14159265358979323846f * 2.0f;   // auxiliary.rs:15
    const float scx = KIND == 1 ? PI_X2 / box.ax : 0.f, scy = KIND == 1 ? PI_X2 / box.by : 0.f, scz = KIND == 1 ? PI_X2 / box.cz : 0.f;
    const float cx = KIND == 2 ? st.center[0] : 0.f, cy = KIND == 2 ? st.center[1] : 0.f, cz = KIND == 2 ? st.center[2] : 0.f;
    constexpr int K = KIND == 1 ? 7 : 4;
    double acc[GR_CEN_K];
#pragma unroll
    for (int k = 0; k < GR_CEN_K; ++k) acc[k] = 0.0;
    uint32_t bad_pos = GR_NOIDX, bad_mass = GR_NOIDX;
    // (the loads of U trips are requested together, their atoms then added in trip order; a trip that does not exist reads the
    //  segment's first atom again and adds nothing)
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
            float p[7] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
            gr_center_atom<KIND>(ii[k], x[k], y[k], z[k], m[k], weighted, box, scx, scy, scz, cx, cy, cz, bad_pos, bad_mass, p);
#pragma unroll
            for (int q = 0; q < K; ++q) acc[q] += (double)p[q];
        }
    }
    constexpr int W = TEAM < 64 ? TEAM : 64;
#pragma unroll
    for (int q = 0; q < K; ++q) acc[q] = gr_seg_team_sum<W>(acc[q]);
    bad_pos = gr_seg_team_min<W>(bad_pos); bad_mass = gr_seg_team_min<W>(bad_mass);
    if (TEAM > 64) {    // the four waves' totals through LDS, added in wave order by every lane
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
            for (int q = 0; q < K; ++q) lds[wave * (GR_CEN_K + 1) + q] = acc[q];
            lds[wave * (GR_CEN_K + 1) + GR_CEN_K] = __longlong_as_double((long long)(((unsigned long long)bad_pos << 32) | bad_mass));
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < K; ++q) {
            double s = lds[q];
#pragma unroll
            for (int wv = 1; wv < TEAM / 64; ++wv) s += lds[wv * (GR_CEN_K + 1) + q];
            acc[q] = s;
        }
        bad_pos = GR_NOIDX; bad_mass = GR_NOIDX;
#pragma unroll
        for (int wv = 0; wv < TEAM / 64; ++wv) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(lds[wv * (GR_CEN_K + 1) + GR_CEN_K]);
            bad_pos = min(bad_pos, (uint32_t)(b >> 32)); bad_mass = min(bad_mass, (uint32_t)b);
        }
    }
    gr_center_close(acc, bad_pos, bad_mass, box, KIND, weighted, mass_first, target, n, st, 0);
}

// grid (teams of the class / teams per workgroup, frames); `recs` = the class's records
template <int TEAM>
__global__ __launch_bounds__(256) void k_segment_centers(const float *__restrict__ frames, size_t frame_stride, uint32_t first_slot, const float *__restrict__ masses,
                                                         const grs::Rec *__restrict__ recs, uint32_t n_recs, const uint32_t *__restrict__ atoms,
                                                         const GrBox *__restrict__ boxes, int kind, int weighted, float *__restrict__ out, uint32_t n_segments,
                                                         unsigned long long *keys, const uint32_t *__restrict__ frame_ok) {
    constexpr int U = TEAM <= 16 ? 1 : 4;
    __shared__ double lds[2][TEAM > 64 ? (TEAM / 64) * (GR_CEN_K + 1) : 1];
    const uint32_t f = blockIdx.y;
    const uint32_t team = blockIdx.x * (256u / TEAM) + threadIdx.x / TEAM, tl = threadIdx.x % TEAM;
    const bool active = team < n_recs;                       // (a team behind the class walks the last segment again and stores nothing)
    const grs::Rec r = recs[active ? team : n_recs - 1u];
    const uint32_t n = r.n_flag & ~GR_SEG_CONTIGUOUS;
    const uint32_t *list = (r.n_flag & GR_SEG_CONTIGUOUS) ? nullptr : atoms + r.begin;
    float *o = out + ((size_t)f * n_segments + r.ordinal) * 3u;
    const bool writer = active && tl == 0u;
    if (frame_ok && !frame_ok[f]) {                          // the frame failed its host checks: NaN everywhere, nothing read
        if (writer) { o[0] = NAN; o[1] = NAN; o[2] = NAN; }
        return;
    }
    const GrBox &box = boxes[first_slot + f];
    const float *xyz = frames + (size_t)(first_slot + f) * frame_stride;
    GrFrameState st = {};
    st.err_index = GR_NOIDX;
    // the stages of center_stage / pbc_center_stages (gr_api.hip), with their error precedence
    if (kind == 0) gr_seg_stage<0, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, 0, 1, st, tl, lds[0]);            // position first (iterators.rs:946-958)
    else if (kind == 1) gr_seg_stage<1, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, 1, 1, st, tl, lds[0]);       // mass first (:1324-1339)
    else {
        gr_seg_stage<1, TEAM, U>(xyz, masses, list, r.begin, n, box, 0, 0, 0, st, tl, lds[0]);                              // the unweighted estimate (:1405-1407)
        if (st.status == 0) gr_seg_stage<2, TEAM, U>(xyz, masses, list, r.begin, n, box, weighted, 0, 1, st, tl, lds[1]);   // (the status is the team's: no lane parts)
    }
    if (!writer) return;
    if (st.status == 0) { o[0] = st.com[0]; o[1] = st.com[1]; o[2] = st.com[2]; return; }
    o[0] = NAN; o[1] = NAN; o[2] = NAN;
    atomicMin(&keys[f], ((unsigned long long)r.ordinal << 33) | ((unsigned long long)(st.status == 7 ? 1u : 0u) << 32) | st.err_index);
}

void seg_free(gr_segments *S) {
    if (S->recs_dev) (void)hipFree(S->recs_dev);
    if (S->atoms_dev) (void)hipFree(S->atoms_dev);
    if (S->key_dev) (void)hipFree(S->key_dev);
    if (S->ok_dev) (void)hipFree(S->ok_dev);
    if (S->key_host) (void)hipHostFree(S->key_host);
    if (S->ok_host) (void)hipHostFree(S->ok_host);
    delete S;                                              // (frees `out`)
}

// the partition in S->P becomes an object: records and atom list on the device
gr_segments *seg_install(gr_ctx *c, gr_segments *S, int *status) {
    (void)hipSetDevice(c->device);
    S->c = c;
    std::vector<grs::Rec> recs;
    S->P.records(recs, S->start);
    bool ok = hipMalloc(&S->recs_dev, recs.size() * sizeof(grs::Rec)) == hipSuccess;
    ok = ok && hipMalloc(&S->atoms_dev, S->P.atoms.size() * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc(&S->key_dev, GR_MAX_BATCH * sizeof(unsigned long long)) == hipSuccess;
    ok = ok && hipMalloc(&S->ok_dev, GR_MAX_BATCH * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&S->key_host), GR_MAX_BATCH * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void **>(&S->ok_host), GR_MAX_BATCH * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMemcpy(S->recs_dev, recs.data(), recs.size() * sizeof(grs::Rec), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(S->atoms_dev, S->P.atoms.data(), S->P.atoms.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        seg_free(S);
        *status = fail(c, GR_E_HIP, "segments: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return S;
}

int seg_status(gr_ctx *c, int st, uint64_t bad) {
    if (st == grs::SEG_EMPTY) return fail(c, GR_E_EMPTY_GROUP, "segments: no segment, or an empty one");
    if (st == grs::SEG_OUT_OF_RANGE) return fail(c, GR_E_OUT_OF_RANGE, "atom index out of range", bad);
    if (st != grs::SEG_OK) return fail(c, GR_E_INVALID_ARG, "segments: NULL pointer, offsets that decrease, a list that is not strictly ascending, or too many entries");
    return GR_OK;
}

template <int TEAM>
void seg_launch(gr_segments *S, int cls, uint32_t s0, uint32_t nb, int kind, int weighted, const uint32_t *ok_dev) {
    gr_ctx *c = S->c;
    const uint32_t n_recs = (uint32_t)(S->start[cls + 1] - S->start[cls]);
    if (n_recs == 0) return;
    const uint32_t per = 256u / TEAM;
    k_segment_centers<TEAM><<<dim3((n_recs + per - 1u) / per, nb), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0, c->masses, S->recs_dev + S->start[cls], n_recs,
                                                                                           S->atoms_dev, c->boxes_dev, kind, weighted, S->out.get(), (uint32_t)S->P.count(),
                                                                                           S->key_dev, ok_dev);
    ++S->last_launches;
}

// out_host: [n_frames][M][3] or NULL; the device block holds the frames of the LAST segment of the batch (the device form has only one)
int seg_centers(gr_segments *S, uint32_t first_slot, uint32_t n_frames, int kind, int weighted, float *out_host, int *status_out) {
    gr_ctx *c = S->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    if (kind != GR_CENTER_NAIVE && kind != GR_CENTER_ESTIMATE && kind != GR_CENTER_PBC) return fail(c, GR_E_INVALID_ARG, "unknown centre kind");
    const size_t per_frame = (size_t)S->P.count() * 3u;
    // (every call ends behind its own read-back: nobody reads the block of an earlier call any more)
    HIPCHK(c, S->out.reserve(per_frame * std::min<uint32_t>(n_frames, GR_MAX_BATCH), grbuf::exact));
    S->last_launches = 0; S->last_sets = 0;
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
            seg_launch<4>(S, grs::TEAM4, s0, nb, kind, weighted, ok_dev);
            seg_launch<16>(S, grs::TEAM16, s0, nb, kind, weighted, ok_dev);
            seg_launch<64>(S, grs::TEAM_WAVE, s0, nb, kind, weighted, ok_dev);
            seg_launch<256>(S, grs::TEAM_BLOCK, s0, nb, kind, weighted, ok_dev);
            HIPCHK(c, hipGetLastError());
            ++S->last_sets;
            HIPCHK(c, hipMemcpyAsync(S->key_host, S->key_dev, nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            if (out_host) HIPCHK(c, hipMemcpyAsync(out_host + (size_t)b0 * per_frame, S->out.get(), (size_t)nb * per_frame * sizeof(float), hipMemcpyDeviceToHost, c->stream));
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

gr_segments *gr_segments_create(gr_ctx *c, const uint64_t *offsets, const uint64_t *atoms, uint64_t n_segments, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    gr_segments *S = new gr_segments();
    uint64_t bad = 0;
    *status = seg_status(c, grs::from_lists(offsets, atoms, n_segments, c->n, S->P, &bad), bad);
    if (*status) { delete S; return nullptr; }
    return seg_install(c, S, status);
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

gr_segments *gr_segments_from_labels(gr_ctx *c, const char *group, const uint64_t *labels, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    if (!labels) { *status = fail(c, GR_E_INVALID_ARG, "segments: labels is NULL"); return nullptr; }
    std::vector<uint64_t> members;
    if (group) {
        const Group *g = need_group(c, group, *status, true); if (!g) return nullptr;
        members = grc::expand(g->blocks);
    }
    gr_segments *S = new gr_segments();
    *status = seg_status(c, grs::from_labels(group ? members.data() : nullptr, members.size(), c->n, labels, S->P), 0);
    if (*status) { delete S; return nullptr; }
    return seg_install(c, S, status);
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

gr_segments *gr_segments_from_molecules(gr_ctx *c, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    gr_segments *S = new gr_segments();
    *status = seg_status(c, grs::from_molecules(whole_of(c).topo, S->P), 0);
    if (*status) { delete S; return nullptr; }
    return seg_install(c, S, status);
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_segments_destroy(gr_segments *S) try {
    if (!S) return;
    (void)hipSetDevice(S->c->device);
    (void)hipStreamSynchronize(S->c->stream);
    seg_free(S);
} catch (...) { }

uint64_t gr_segments_count(const gr_segments *S) { return S ? S->P.count() : 0; }

int gr_segments_sizes(const gr_segments *S, uint64_t *out) try {
    if (!S || !out) return GR_E_INVALID_ARG;
    for (uint64_t s = 0; s < S->P.count(); ++s) out[s] = S->P.size(s);
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_segments_atoms(const gr_segments *S, uint64_t s, uint64_t *out, uint64_t cap, uint64_t *n) try {
    if (!S) return GR_E_INVALID_ARG;
    if (s >= S->P.count()) return fail(S->c, GR_E_OUT_OF_RANGE, "segment out of range", s);
    const uint64_t m = S->P.size(s);
    if (n) *n = m;
    if (out) for (uint64_t k = 0; k < m && k < cap; ++k) out[k] = S->P.atoms[S->P.off[s] + k];
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_segments_stat(const gr_segments *S, int key, uint64_t *value) try {
    if (!S || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_SEG_STAT_TEAM4: case GR_SEG_STAT_TEAM16: case GR_SEG_STAT_WAVE: case GR_SEG_STAT_WORKGROUP:
        *value = S->P.class_count[key - GR_SEG_STAT_TEAM4]; return GR_OK;
    case GR_SEG_STAT_LAST_LAUNCHES: *value = S->last_launches; return GR_OK;
    case GR_SEG_STAT_LAST_LAUNCH_SETS: *value = S->last_sets; return GR_OK;
    case GR_SEG_STAT_LAST_PIECES: *value = S->last_pieces; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

int gr_segments_center_batch(gr_segments *S, uint32_t first_slot, uint32_t n_frames, int kind, int weighted, float *out, int *status_out) try {
    if (!S) return GR_E_INVALID_ARG;
    return seg_centers(S, first_slot, n_frames, kind, weighted, out, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_segments_center_batch_device(gr_segments *S, uint32_t first_slot, uint32_t n_frames, int kind, int weighted, float **out_dev, uint64_t *n_segments,
                                    int *status_out) try {
    if (!S) return GR_E_INVALID_ARG;
    if (n_frames > GR_SEG_MAX_DEVICE_FRAMES) return fail(S->c, GR_E_INVALID_ARG, "segments: the device form takes at most 1024 frames");
    const int st = seg_centers(S, first_slot, n_frames, kind, weighted, nullptr, status_out);
    if (out_dev) *out_dev = S->out.get();
    if (n_segments) *n_segments = S->P.count();
    return st;
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

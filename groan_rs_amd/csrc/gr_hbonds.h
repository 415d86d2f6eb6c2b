// gr_hbonds.h -- hydrogen-bond analysis over a batch of resident frames (gr_hbond_plan_create / gr_hbond_batch).
//
// Reference: HBondAnalysis (src/system/hbonds.rs:154-373).  A chain is (acceptors, donors, hydrogens); a donor is kept when it
// is bonded to at least one atom of the chain's hydrogen group, its hydrogens in index order (HBondChainGroups::new, :111-151).
// A requested pair (a, b) is one SEGMENT when a == b -- acceptors of a, donors of a -- and two otherwise: acceptors of a with
// donors of b, then acceptors of b with donors of a (:207-227).  In a segment every donor visits the acceptors of the 27 (or
// fewer) cells around it, skips itself, keeps an acceptor at distance <= max_distance (acceptor.distance(donor)), and for each
// of its hydrogens keeps the bond when the D-H...A angle (hydrogen.vector_to(donor) against hydrogen.vector_to(acceptor)) is
// >= min_angle; a NaN angle is 180 degrees when the hydrogen is closer to the acceptor than the donor is, else 0 (:302-338).
// Bonds are reported by segment, then donor (group order), then acceptor index, then hydrogen index -- the reference leaves the
// acceptor order undefined (cellgrid.rs:377).
//
// Device pipeline of one batch (the plan's workspace, the context's stream; the number of launches does not depend on n_frames):
//   k_hb_assign        every acceptor of every (frame, chain) -> key = (frame, chain, cell), rank in its cell by atomicAdd
//   rocprim::exclusive_scan   cell counts -> cell starts (one key space for the batch: a counting sort)
//   k_hb_scatter       acceptors into cell order as float4 (x, y, z, atom index): the walk streams them
//   k_hb_walk<false>   one lane per (frame, segment, donor): count its bonds, report missing positions (atomicMin on ordinals)
//   k_hb_mask          the lanes of a frame that failed count nothing
//   rocprim::exclusive_scan   lane counts -> lane offsets;  k_hb_pack: (frame, pair) offsets next to the error words
//   -- one read-back: offsets + error words --
//   k_hb_walk<true>    the same walk writing at the lane's offset, then the lane sorts its run by (acceptor, hydrogen)
//   -- one read-back: the bonds --
#pragma once
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <vector>
#include "gr_cellgrid.h"

#define GR_HB_HREG 4               /* hydrogens of a donor held in registers; further ones are loaded where they are used */
#define GR_HB_MAX_FRAMES 1024      /* frames per gr_hbond_batch call */
#define GR_HB_DEG 57.2957795130823208767981548141051703f   /* f32::to_degrees */

struct GrHbFrame {        // one frame of the batch, built on the host from boxes_host
    GrCellGrid g;
    uint32_t kbase;       // first key of chain 0's grid; chain c's grid starts at kbase + c * g.ncells
    uint32_t ok;          // 0: the frame failed a host check -- no keys, its lanes count nothing
};
struct GrHbLane { uint32_t donor, h0, nh, chain; };   // donor atom, its hydrogens hyd[h0 .. h0 + nh), the chain whose acceptors it visits

// the reference's Vector3D::angle(..).to_degrees() (vector3d.rs:276-278): left-to-right dot product and norms, no contraction,
// correctly rounded divide and square root
GR_HD float gr_hb_angle_deg(float ux, float uy, float uz, float vx, float vy, float vz) {
#pragma clang fp contract(off)
    const float dot = ux * vx + uy * vy + uz * vz;
    const float lu = sqrtf(ux * ux + uy * uy + uz * uz), lv = sqrtf(vx * vx + vy * vy + vz * vz);
    return acosf(dot / (lu * lv)) * GR_HB_DEG;
}
// calc_angle + handle_nan (hbonds.rs:302-338)
__device__ __forceinline__ float gr_hb_angle(float dx, float dy, float dz, float hx, float hy, float hz, float ax, float ay, float az, const GrBox &box) {
    float ux, uy, uz, vx, vy, vz;
    gr_vector_to(hx, hy, hz, dx, dy, dz, box, ux, uy, uz);
    gr_vector_to(hx, hy, hz, ax, ay, az, box, vx, vy, vz);
    const float a = gr_hb_angle_deg(ux, uy, uz, vx, vy, vz);
    if (a == a) return a;
    return gr_distance<4, true>(hx, hy, hz, ax, ay, az, 7, box) < gr_distance<4, true>(dx, dy, dz, ax, ay, az, 7, box) ? 180.0f : 0.0f;
}

// e = frame * n_acc + r: acceptor r of the batch's frames (chain order, then group order)
__global__ __launch_bounds__(256) void k_hb_assign(const float *__restrict__ frames, size_t stride, uint32_t slot0, const GrBox *__restrict__ boxes,
                                                   const GrHbFrame *__restrict__ fr, const uint32_t *__restrict__ acc_atom, const uint32_t *__restrict__ acc_chain,
                                                   uint32_t n_acc, uint64_t n_el, uint32_t *__restrict__ cell_count, uint32_t *__restrict__ keys,
                                                   uint32_t *__restrict__ ranks, uint32_t *__restrict__ acc_bad) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n_el) return;
    const uint32_t f = (uint32_t)(e / n_acc), r = (uint32_t)(e - (uint64_t)f * n_acc);
    if (!fr[f].ok) { keys[e] = GR_NOIDX; return; }
    const GrCellGrid g = fr[f].g;
    float x, y, z;
    gr_pos_load(frames + (size_t)(slot0 + f) * stride, acc_atom[r], x, y, z);
    if (x != x) { atomicMin(acc_bad + f, r); keys[e] = GR_NOIDX; return; }   // CellGrid::new_from_group: the first acceptor without position
    uint32_t c[3];
    gr_cg_cell_of(x, y, z, boxes[f], g, c);
    const uint32_t key = fr[f].kbase + acc_chain[r] * g.ncells + (c[2] * g.nc[1] + c[1]) * g.nc[0] + c[0];
    keys[e] = key;
    ranks[e] = atomicAdd(cell_count + key, 1u);
}

__global__ __launch_bounds__(256) void k_hb_scatter(const float *__restrict__ frames, size_t stride, uint32_t slot0, const uint32_t *__restrict__ acc_atom,
                                                    uint32_t n_acc, uint64_t n_el, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ ranks,
                                                    const uint32_t *__restrict__ cell_start, float4 *__restrict__ sorted) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n_el) return;
    const uint32_t key = keys[e];
    if (key == GR_NOIDX) return;
    const uint32_t f = (uint32_t)(e / n_acc), r = (uint32_t)(e - (uint64_t)f * n_acc), a = acc_atom[r];
    float x, y, z;
    gr_pos_load(frames + (size_t)(slot0 + f) * stride, a, x, y, z);
    sorted[cell_start[key] + ranks[e]] = make_float4(x, y, z, __uint_as_float(a));
}

// one lane per (frame, lane of the plan); WRITE = false: count (+ missing positions), WRITE = true: write at offs[t] and sort
template <bool WRITE>
__global__ __launch_bounds__(256) void k_hb_walk(const float *__restrict__ frames, size_t stride, uint32_t slot0, const GrBox *__restrict__ boxes,
                                                 const GrHbFrame *__restrict__ fr, const GrHbLane *__restrict__ lanes, const uint32_t *__restrict__ hyd,
                                                 uint32_t n_lanes, uint64_t n_t, const uint32_t *__restrict__ cell_start, const float4 *__restrict__ acc,
                                                 float cutoff, float min_angle, uint32_t *__restrict__ counts, const unsigned long long *__restrict__ offs,
                                                 unsigned long long *__restrict__ don_bad, uint32_t *__restrict__ o_don, uint32_t *__restrict__ o_h,
                                                 uint32_t *__restrict__ o_acc, float *__restrict__ o_d, float *__restrict__ o_ang) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= n_t) return;
    const uint32_t cap = WRITE ? counts[t] : 0u;
    if (WRITE && cap == 0) return;                  // (also every lane of a frame that failed: k_hb_mask zeroed them)
    const uint32_t f = (uint32_t)(t / n_lanes), l = (uint32_t)(t - (uint64_t)f * n_lanes);
    if (!fr[f].ok) { if (!WRITE) counts[t] = 0; return; }
    const GrCellGrid g = fr[f].g;
    const GrHbLane L = lanes[l];
    const GrBox &box = boxes[f];
    const float *xyz = frames + (size_t)(slot0 + f) * stride;
    float dx, dy, dz;
    gr_pos_load(xyz, L.donor, dx, dy, dz);
    if (dx != dx) {                                 // hbonds.rs:240-245
        if (!WRITE) { atomicMin(don_bad + f, ((unsigned long long)l << 32) | 0xFFFFFFFFull); counts[t] = 0; }
        return;
    }
    float hx[GR_HB_HREG], hy[GR_HB_HREG], hz[GR_HB_HREG];
#pragma unroll
    for (int k = 0; k < GR_HB_HREG; ++k) {
        hx[k] = hy[k] = hz[k] = 0.0f;
        if ((uint32_t)k < L.nh) gr_pos_load(xyz, hyd[L.h0 + k], hx[k], hy[k], hz[k]);
    }
    uint32_t c[3];
    gr_cg_cell_of(dx, dy, dz, box, g, c);
    int lo[3], hi[3];                               // CellNeighbors::convert, as k_cg_pairs
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = g.nc[a] >= 3 ? -1 : 0; hi[a] = g.nc[a] >= 2 ? 1 : 0; }
    const uint32_t kb = fr[f].kbase + L.chain * g.ncells;
    const unsigned long long base = WRITE ? offs[t] : 0ull;
    bool checked = WRITE;                           // the hydrogens' positions are verified at the first acceptor in range
    uint32_t n = 0;
    for (int oz = lo[2]; oz <= hi[2]; ++oz)
        for (int oy = lo[1]; oy <= hi[1]; ++oy)
            for (int ox = lo[0]; ox <= hi[0]; ++ox) {
                const uint32_t cx = (uint32_t)((int)c[0] + ox + (int)g.nc[0]) % g.nc[0], cy = (uint32_t)((int)c[1] + oy + (int)g.nc[1]) % g.nc[1],
                               cz = (uint32_t)((int)c[2] + oz + (int)g.nc[2]) % g.nc[2];
                const uint32_t cell = kb + (cz * g.nc[1] + cy) * g.nc[0] + cx;
                const uint32_t q1 = cell_start[cell + 1];
                for (uint32_t q = cell_start[cell]; q < q1; ++q) {
                    const float4 A = acc[q];
                    const uint32_t ai = __float_as_uint(A.w);
                    if (ai == L.donor) continue;                                                 // :247-250
                    const float d = gr_distance<4, true>(A.x, A.y, A.z, dx, dy, dz, 7, box);     // acceptor.distance(donor), :259
                    if (d > cutoff) continue;
                    if (!checked) {                 // :268-274: the first hydrogen (index order) without position
                        checked = true;
                        bool bad = false; uint32_t bk = 0;
#pragma unroll
                        for (int k = GR_HB_HREG - 1; k >= 0; --k)
                            if ((uint32_t)k < L.nh && hx[k] != hx[k]) { bad = true; bk = (uint32_t)k; }
                        for (uint32_t k = GR_HB_HREG; !bad && k < L.nh; ++k) {
                            float x, y, z;
                            gr_pos_load(xyz, hyd[L.h0 + k], x, y, z);
                            if (x != x) { bad = true; bk = k; }
                        }
                        if (bad) { atomicMin(don_bad + f, ((unsigned long long)l << 32) | bk); counts[t] = 0; return; }
                    }
#pragma unroll
                    for (int k = 0; k < GR_HB_HREG; ++k) {
                        if ((uint32_t)k >= L.nh) break;
                        const float ang = gr_hb_angle(dx, dy, dz, hx[k], hy[k], hz[k], A.x, A.y, A.z, box);
                        if (ang < min_angle) continue;
                        if (WRITE && n < cap) { o_don[base + n] = L.donor; o_h[base + n] = hyd[L.h0 + k]; o_acc[base + n] = ai; o_d[base + n] = d; o_ang[base + n] = ang; }
                        ++n;
                    }
                    for (uint32_t k = GR_HB_HREG; k < L.nh; ++k) {
                        float x, y, z;
                        const uint32_t h = hyd[L.h0 + k];
                        gr_pos_load(xyz, h, x, y, z);
                        const float ang = gr_hb_angle(dx, dy, dz, x, y, z, A.x, A.y, A.z, box);
                        if (ang < min_angle) continue;
                        if (WRITE && n < cap) { o_don[base + n] = L.donor; o_h[base + n] = h; o_acc[base + n] = ai; o_d[base + n] = d; o_ang[base + n] = ang; }
                        ++n;
                    }
                }
            }
    if (!WRITE) { counts[t] = n; return; }
    // the run arrived cell by cell, each acceptor's hydrogens in order: a stable insertion sort by acceptor gives (acceptor, hydrogen)
    const uint32_t m = n < cap ? n : cap;
    for (uint32_t a = 1; a < m; ++a) {
        const uint32_t va = o_acc[base + a], vh = o_h[base + a];
        const float vd = o_d[base + a], vg = o_ang[base + a];
        uint32_t b = a;
        while (b > 0 && o_acc[base + b - 1] > va) {
            o_acc[base + b] = o_acc[base + b - 1]; o_h[base + b] = o_h[base + b - 1]; o_d[base + b] = o_d[base + b - 1]; o_ang[base + b] = o_ang[base + b - 1];
            --b;
        }
        o_acc[base + b] = va; o_h[base + b] = vh; o_d[base + b] = vd; o_ang[base + b] = vg;
    }
}

// the lanes of a frame with a missing position count nothing (its segments are empty); counts[n_t] = 0 closes the scan
__global__ __launch_bounds__(256) void k_hb_mask(uint32_t *__restrict__ counts, uint32_t n_lanes, uint64_t n_t, const uint32_t *__restrict__ acc_bad,
                                                 const unsigned long long *__restrict__ don_bad) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t > n_t) return;
    if (t == n_t) { counts[t] = 0; return; }
    const uint32_t f = (uint32_t)(t / n_lanes);
    if (acc_bad[f] != GR_NOIDX || don_bad[f] != ~0ull) counts[t] = 0;
}

// out[f * n_pairs + p] = offset of the first lane of pair p in frame f; out[n_frames * n_pairs] = the batch's total
__global__ __launch_bounds__(256) void k_hb_pack(const unsigned long long *__restrict__ offs, const uint32_t *__restrict__ pair_lane, uint32_t n_pairs,
                                                 uint32_t n_lanes, uint32_t n_frames, unsigned long long *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = n_frames * n_pairs;
    if (i > n) return;
    if (i == n) { out[i] = offs[(uint64_t)n_frames * n_lanes]; return; }
    const uint32_t f = i / n_pairs, p = i - f * n_pairs;
    out[i] = offs[(uint64_t)f * n_lanes + pair_lane[p]];
}

struct gr_hbond_plan {
    gr_ctx *c = nullptr;
    uint32_t n_chains = 0, n_pairs = 0, n_lanes = 0, n_acc = 0, max_chain_acc = 0;
    float cutoff = 0.0f, min_angle = 0.0f;
    std::vector<uint32_t> acc_atom, hyd;       // host copies: error indices
    std::vector<GrHbLane> lanes;
    // device tables (one allocation): acceptors + their chains, hydrogens, lanes, first lane of every pair
    unsigned char *tab = nullptr;
    uint32_t *acc_atom_d = nullptr, *acc_chain_d = nullptr, *hyd_d = nullptr, *pair_lane_d = nullptr;
    GrHbLane *lanes_d = nullptr;
    // workspace, grown on first use: device, pinned host, bond outputs
    grbuf::Dev<unsigned char> ws;
    grbuf::Pinned<unsigned char> hbuf;
    grbuf::Dev<unsigned char> outs;   // bonds: [5][cap] words
};

namespace {

// a grid for the batch's key space: the cut-off's, coarsened where it would hold many more cells than the largest chain has acceptors
// (a coarser grid prunes less but finds the same bonds: every cell is still at least the cut-off thick)
GrCellGrid hb_grid(const GrBox &box, float cutoff, uint32_t max_chain_acc) {
    const uint64_t cap = std::max<uint64_t>(64, 2ull * max_chain_acc);
    float cs = cutoff;
    GrCellGrid g = gr_cellgrid_make(box, cs);
    while (g.ncells > cap && g.ncells > 1) { cs *= 1.25f; g = gr_cellgrid_make(box, cs); }
    return g;
}

// the box checks of one frame in the order the analysis meets them (CellGrid::new_from_group -> check_box, cellgrid.rs:411-430)
int hb_box_check(gr_ctx *c, uint32_t slot) {
    const int s = c->box_status[slot];
    if (s == GR_E_NO_BOX) return fail(c, GR_E_NO_BOX, "simulation box does not exist");
    if (s == GR_E_ZERO_BOX) return fail(c, GR_E_ZERO_BOX, "invalid simulation box");
    if (c->strict && !c->boxes_host[slot].ortho) return fail(c, GR_E_NOT_ORTHOGONAL, "simulation box is not orthogonal");
    if (s != GR_OK) return fail(c, s, "invalid simulation box");
    return GR_OK;
}

std::vector<uint32_t> hb_group_atoms(const Group &g) {
    std::vector<uint32_t> v;
    v.reserve(g.n);
    for (const auto &b : g.blocks) for (uint64_t a = b.first; a <= b.second; ++a) v.push_back((uint32_t)a);
    return v;
}

size_t hb_al(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

void gr_hbond_plan_destroy(gr_hbond_plan *p) try {
    if (!p) return;
    if (p->c) { (void)hipSetDevice(p->c->device); (void)hipStreamSynchronize(p->c->stream); }
    if (p->tab) (void)hipFree(p->tab);
    delete p;      // (frees the workspace, gr_buf.h)
} catch (...) {}

gr_hbond_plan *gr_hbond_plan_create(gr_ctx *c, const char *const *groups, uint32_t n_chains, const uint32_t *pairs, uint32_t n_pairs,
                                    const uint64_t *bonds, uint64_t n_bonds, float max_distance, float min_angle, int *status) try {
    int dummy = 0;
    int &st = status ? *status : dummy;
    st = GR_OK;
    if (!c) { st = GR_E_INVALID_ARG; return nullptr; }
    if ((st = busy_check(c))) return nullptr;
    if ((n_chains && !groups) || (n_pairs && !pairs) || (n_bonds && !bonds)) { st = fail(c, GR_E_INVALID_ARG, "NULL array"); return nullptr; }
    (void)hipSetDevice(c->device);
    // the system's bonds: a neighbour list per atom (Atom::get_bonded is a sorted container)
    for (uint64_t b = 0; b < 2 * n_bonds; ++b)
        if (bonds[b] >= c->n) { st = fail(c, GR_E_OUT_OF_RANGE, "bonded atom out of range", bonds[b]); return nullptr; }
    std::vector<uint64_t> deg(c->n + 1, 0);
    for (uint64_t b = 0; b < n_bonds; ++b) if (bonds[2 * b] != bonds[2 * b + 1]) { ++deg[bonds[2 * b] + 1]; ++deg[bonds[2 * b + 1] + 1]; }
    for (uint64_t a = 0; a < c->n; ++a) deg[a + 1] += deg[a];
    std::vector<uint32_t> nbr(deg[c->n]);
    {
        std::vector<uint64_t> at(deg.begin(), deg.end() - 1);
        for (uint64_t b = 0; b < n_bonds; ++b) {
            const uint64_t i = bonds[2 * b], j = bonds[2 * b + 1];
            if (i == j) continue;
            nbr[at[i]++] = (uint32_t)j; nbr[at[j]++] = (uint32_t)i;
        }
    }
    // chains (HBondChainGroups::new, in order)
    std::vector<std::vector<uint32_t>> acc(n_chains);
    std::vector<std::vector<GrHbLane>> don(n_chains);   // h0 indexes `hyd`
    std::vector<uint32_t> hyd;
    std::vector<uint8_t> is_h(c->n, 0);
    for (uint32_t k = 0; k < n_chains; ++k) {
        const Group *g[3];
        for (int r = 0; r < 3; ++r) {
            const char *name = groups[3 * k + r];
            g[r] = find_group(c, name);
            if (!g[r]) { st = fail(c, GR_E_GROUP_NOT_FOUND, name ? name : "(null)", k); return nullptr; }
        }
        acc[k] = hb_group_atoms(*g[0]);
        const std::vector<uint32_t> hs = hb_group_atoms(*g[2]);
        for (uint32_t h : hs) is_h[h] = 1;
        for (uint32_t d : hb_group_atoms(*g[1])) {
            const uint32_t h0 = (uint32_t)hyd.size();
            for (uint64_t q = deg[d]; q < deg[d + 1]; ++q) if (is_h[nbr[q]]) hyd.push_back(nbr[q]);
            if (hyd.size() == h0) continue;
            std::sort(hyd.begin() + h0, hyd.end());
            hyd.erase(std::unique(hyd.begin() + h0, hyd.end()), hyd.end());
            don[k].push_back(GrHbLane{ d, h0, (uint32_t)hyd.size() - h0, 0 });
        }
        for (uint32_t h : hs) is_h[h] = 0;
        if (acc[k].empty() && don[k].empty()) { st = fail(c, GR_E_EMPTY_CHAIN, "no acceptor and no donor atoms detected for chain", k); return nullptr; }
    }
    // sanity_check_pairs (hbonds.rs:340-373)
    {
        std::set<std::pair<uint32_t, uint32_t>> seen;
        std::vector<uint8_t> used(n_chains, 0);
        for (uint32_t p = 0; p < n_pairs; ++p) {
            const uint32_t a = pairs[2 * p], b = pairs[2 * p + 1];
            if (a >= n_chains) { st = fail(c, GR_E_NONEXISTENT_CHAIN, "chain does not exist", a); return nullptr; }
            if (b >= n_chains) { st = fail(c, GR_E_NONEXISTENT_CHAIN, "chain does not exist", b); return nullptr; }
            const bool fresh = a != b ? (seen.insert({ a, b }).second && seen.insert({ b, a }).second) : seen.insert({ a, b }).second;
            if (!fresh) { st = fail(c, GR_E_DUPLICATE_PAIR, "pair of chains requested multiple times", p); return nullptr; }
            used[a] = used[b] = 1;
        }
        for (uint32_t k = 0; k < n_chains; ++k)
            if (!used[k]) { st = fail(c, GR_E_UNUSED_CHAIN, "not all chains are used", k); return nullptr; }
    }
    if (!(max_distance > 0.0f)) { st = fail(c, GR_E_INVALID_ARG, "cell size (max_distance) must be positive"); return nullptr; }   // CellGridError::InvalidCellSize
    gr_hbond_plan *p = new gr_hbond_plan();
    p->c = c; p->n_chains = n_chains; p->n_pairs = n_pairs; p->cutoff = max_distance; p->min_angle = min_angle; p->hyd = hyd;
    std::vector<uint32_t> acc_chain, pair_lane;
    for (uint32_t k = 0; k < n_chains; ++k) {
        for (uint32_t a : acc[k]) { p->acc_atom.push_back(a); acc_chain.push_back(k); }
        p->max_chain_acc = std::max<uint32_t>(p->max_chain_acc, (uint32_t)acc[k].size());
    }
    auto segment = [&](uint32_t grid_chain, uint32_t donor_chain) {
        for (GrHbLane L : don[donor_chain]) { L.chain = grid_chain; p->lanes.push_back(L); }
    };
    for (uint32_t q = 0; q < n_pairs; ++q) {
        const uint32_t a = pairs[2 * q], b = pairs[2 * q + 1];
        pair_lane.push_back((uint32_t)p->lanes.size());
        if (a == b) segment(a, a);
        else { segment(a, b); segment(b, a); }
    }
    pair_lane.push_back((uint32_t)p->lanes.size());
    p->n_acc = (uint32_t)p->acc_atom.size(); p->n_lanes = (uint32_t)p->lanes.size();
    const size_t o_aa = 0, o_ac = o_aa + hb_al(4 * (size_t)p->n_acc + 4), o_h = o_ac + hb_al(4 * (size_t)p->n_acc + 4), o_l = o_h + hb_al(4 * hyd.size() + 4),
                 o_p = o_l + hb_al(sizeof(GrHbLane) * ((size_t)p->n_lanes + 1)), total = o_p + hb_al(4 * pair_lane.size());
    auto bail = [&](hipError_t e) { st = fail(c, GR_E_HIP, std::string("hbond plan tables: ") + hipGetErrorString(e)); gr_hbond_plan_destroy(p); return nullptr; };
    hipError_t e = hipMalloc((void **)&p->tab, total);
    if (e != hipSuccess) return bail(e);
    p->acc_atom_d = (uint32_t *)(p->tab + o_aa); p->acc_chain_d = (uint32_t *)(p->tab + o_ac); p->hyd_d = (uint32_t *)(p->tab + o_h);
    p->lanes_d = (GrHbLane *)(p->tab + o_l); p->pair_lane_d = (uint32_t *)(p->tab + o_p);
    if (p->n_acc && e == hipSuccess) e = hipMemcpy(p->acc_atom_d, p->acc_atom.data(), 4 * (size_t)p->n_acc, hipMemcpyHostToDevice);
    if (p->n_acc && e == hipSuccess) e = hipMemcpy(p->acc_chain_d, acc_chain.data(), 4 * (size_t)p->n_acc, hipMemcpyHostToDevice);
    if (!hyd.empty() && e == hipSuccess) e = hipMemcpy(p->hyd_d, hyd.data(), 4 * hyd.size(), hipMemcpyHostToDevice);
    if (p->n_lanes && e == hipSuccess) e = hipMemcpy(p->lanes_d, p->lanes.data(), sizeof(GrHbLane) * p->n_lanes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->pair_lane_d, pair_lane.data(), 4 * pair_lane.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(e);
    return p;
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

int gr_hbond_batch(gr_hbond_plan *p, uint32_t first_slot, uint32_t n_frames, uint64_t max_bonds, uint32_t *donor, uint32_t *hydrogen, uint32_t *acceptor,
                   float *distance, float *angle, uint64_t *offsets, uint64_t *n_total, int *status_out) try {
    if (!p) return GR_E_INVALID_ARG;
    gr_ctx *c = p->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    if (n_frames > GR_HB_MAX_FRAMES) return fail(c, GR_E_INVALID_ARG, "more than 1024 frames in one hydrogen-bond batch");
    if (!offsets) return fail(c, GR_E_INVALID_ARG, "offsets is NULL");
    (void)hipSetDevice(c->device);
    const uint32_t nf = n_frames, np = p->n_pairs, nl = p->n_lanes, na = p->n_acc, s0 = first_slot;
    // host checks and the batch's key space
    const grb::Prechecks pre(c, { 0, nf, s0 }, [&](uint32_t slot) { return hb_box_check(c, slot); });
    std::vector<GrHbFrame> frs(nf);
    uint64_t nkeys = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        memset(&frs[f], 0, sizeof(GrHbFrame));
        if (!pre.ok(f)) continue;
        frs[f].g = hb_grid(c->boxes_host[s0 + f], p->cutoff, p->max_chain_acc);
        frs[f].kbase = (uint32_t)nkeys; frs[f].ok = 1;
        nkeys += (uint64_t)p->n_chains * frs[f].g.ncells;
        if (nkeys >= 0x7FFFFFFFull) return fail(c, GR_E_INVALID_ARG, "hydrogen-bond batch too large: split it");
    }
    const uint64_t n_el = (uint64_t)nf * na, n_t = (uint64_t)nf * nl;
    if (n_el >= 0xFFFFFFFFull || n_t >= 0xFFFFFFFFull) return fail(c, GR_E_INVALID_ARG, "hydrogen-bond batch too large: split it");
    // workspace
    size_t tmp_cells = 0, tmp_lanes = 0;
    (void)rocprim::exclusive_scan(nullptr, tmp_cells, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)nkeys + 1, rocprim::plus<uint32_t>(), c->stream);
    (void)rocprim::exclusive_scan(nullptr, tmp_lanes, (uint32_t *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)n_t + 1, rocprim::plus<unsigned long long>(), c->stream);
    const size_t n_rb = (size_t)nf * np + 1;
    const size_t o_fr = 0, o_cc = o_fr + hb_al(sizeof(GrHbFrame) * nf), o_cs = o_cc + hb_al(4 * (nkeys + 1)), o_key = o_cs + hb_al(4 * (nkeys + 1)),
                 o_rank = o_key + hb_al(4 * n_el), o_sort = o_rank + hb_al(4 * n_el), o_cnt = o_sort + hb_al(16 * n_el), o_off = o_cnt + hb_al(4 * (n_t + 1)),
                 o_rb = o_off + hb_al(8 * (n_t + 1)), o_dbad = o_rb + hb_al(8 * n_rb), o_abad = o_dbad + hb_al(8 * (size_t)nf), o_tmp = o_abad + hb_al(4 * (size_t)nf),
                 ws_bytes = o_tmp + hb_al(std::max(tmp_cells, tmp_lanes));
    const size_t rb_bytes = o_tmp - o_rb;                                           // offsets + error words: one read-back
    // every block starts on a 256-byte line, the scans' temporary storage included: rocprim lays its storage out from the pointer it is
    // given and needs its 16-byte look-back states aligned
    if ((o_cc | o_cs | o_key | o_rank | o_sort | o_cnt | o_off | o_rb | o_dbad | o_abad | o_tmp) & 255) return fail(c, GR_E_INVALID_ARG, "hydrogen-bond workspace: a block is off its 256-byte line");
    HIPCHK(c, p->ws.reserve(ws_bytes, grbuf::quarter_aligned256));
    HIPCHK(c, p->hbuf.reserve(hb_al(sizeof(GrHbFrame) * nf) + rb_bytes, grbuf::quarter_aligned256));
    unsigned char *W = p->ws.get();
    GrHbFrame *fr_d = (GrHbFrame *)(W + o_fr);
    uint32_t *cell_count = (uint32_t *)(W + o_cc), *cell_start = (uint32_t *)(W + o_cs), *keys = (uint32_t *)(W + o_key), *ranks = (uint32_t *)(W + o_rank),
             *counts = (uint32_t *)(W + o_cnt), *acc_bad = (uint32_t *)(W + o_abad);
    float4 *sorted = (float4 *)(W + o_sort);
    unsigned long long *offs = (unsigned long long *)(W + o_off), *rb = (unsigned long long *)(W + o_rb), *don_bad = (unsigned long long *)(W + o_dbad);
    GrHbFrame *fr_h = (GrHbFrame *)p->hbuf.get();
    unsigned char *rb_h = p->hbuf.get() + hb_al(sizeof(GrHbFrame) * nf);
    memcpy(fr_h, frs.data(), sizeof(GrHbFrame) * nf);
    const float *xyz = c->frames;
    const size_t stride = c->frame_stride;
    const GrBox *boxes = c->boxes_dev + s0;
    auto blocks = [](uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); };
    SlotUse use(c, s0, nf);
    HIPCHK(c, hipMemcpyAsync(fr_d, fr_h, sizeof(GrHbFrame) * nf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(cell_count, 0, 4 * (nkeys + 1), c->stream));
    HIPCHK(c, hipMemsetAsync(don_bad, 0xFF, o_tmp - o_dbad, c->stream));            // don_bad + acc_bad: "none"
    if (n_el) k_hb_assign<<<blocks(n_el), dim3(256), 0, c->stream>>>(xyz, stride, s0, boxes, fr_d, p->acc_atom_d, p->acc_chain_d, na, n_el, cell_count, keys, ranks, acc_bad);
    size_t tsz = std::max(tmp_cells, tmp_lanes);
    HIPCHK(c, rocprim::exclusive_scan(W + o_tmp, tsz, cell_count, cell_start, 0u, (size_t)nkeys + 1, rocprim::plus<uint32_t>(), c->stream));
    if (n_el) k_hb_scatter<<<blocks(n_el), dim3(256), 0, c->stream>>>(xyz, stride, s0, p->acc_atom_d, na, n_el, keys, ranks, cell_start, sorted);
    if (n_t) k_hb_walk<false><<<blocks(n_t), dim3(256), 0, c->stream>>>(xyz, stride, s0, boxes, fr_d, p->lanes_d, p->hyd_d, nl, n_t, cell_start, sorted, p->cutoff,
                                                                         p->min_angle, counts, nullptr, don_bad, nullptr, nullptr, nullptr, nullptr, nullptr);
    k_hb_mask<<<blocks(n_t + 1), dim3(256), 0, c->stream>>>(counts, nl ? nl : 1u, n_t, acc_bad, don_bad);
    tsz = std::max(tmp_cells, tmp_lanes);
    HIPCHK(c, rocprim::exclusive_scan(W + o_tmp, tsz, counts, offs, 0ull, (size_t)n_t + 1, rocprim::plus<unsigned long long>(), c->stream));
    k_hb_pack<<<blocks(n_rb), dim3(256), 0, c->stream>>>(offs, p->pair_lane_d, np, nl, nf, rb);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rb_h, rb, rb_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long *rb_offs = (const unsigned long long *)rb_h, *rb_dbad = (const unsigned long long *)(rb_h + (o_dbad - o_rb));
    const uint32_t *rb_abad = (const uint32_t *)(rb_h + (o_abad - o_rb));
    // frames' statuses: box checks, then acceptors (grid construction), then the walk's first donor / hydrogen
    grb::FirstError<gr_ctx> fe;
    for (uint32_t f = 0; f < nf; ++f)
        grb::close_frame(c, fe, pre, f, status_out, [&]() -> int {
            if (rb_abad[f] != GR_NOIDX) return fail(c, GR_E_NO_POSITION, "atom has no position", p->acc_atom[rb_abad[f]]);
            if (rb_dbad[f] == ~0ull) return GR_OK;
            const GrHbLane &L = p->lanes[(uint32_t)(rb_dbad[f] >> 32)];
            const uint32_t k = (uint32_t)rb_dbad[f];
            return fail(c, GR_E_NO_POSITION, "atom has no position", k == 0xFFFFFFFFu ? L.donor : p->hyd[L.h0 + k]);
        });
    const unsigned long long total = rb_offs[n_rb - 1];
    memcpy(offsets, rb_offs, 8 * n_rb);
    if (n_total) *n_total = total;
    if (total > 0 && total <= max_bonds && donor && hydrogen && acceptor && distance && angle) {
        HIPCHK(c, p->outs.reserve(20 * (size_t)total, grbuf::quarter_aligned256));
        const size_t cap = p->outs.cap() / 20;
        uint32_t *o_don = (uint32_t *)p->outs.get(), *o_h = o_don + cap, *o_acc = o_h + cap;
        float *o_d = (float *)(o_acc + cap), *o_ang = o_d + cap;
        k_hb_walk<true><<<blocks(n_t), dim3(256), 0, c->stream>>>(xyz, stride, s0, boxes, fr_d, p->lanes_d, p->hyd_d, nl, n_t, cell_start, sorted, p->cutoff,
                                                                   p->min_angle, counts, offs, don_bad, o_don, o_h, o_acc, o_d, o_ang);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(donor, o_don, 4 * total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hydrogen, o_h, 4 * total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(acceptor, o_acc, 4 * total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(distance, o_d, 4 * total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(angle, o_ang, 4 * total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return fe.finish(c);
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

// gr_contacts.h -- Contacts: cut-off pair search over a block of resident frames.
//
// Reference: CellGrid::new + neighbors_iter + the distance filter of its consumer (src/structures/cellgrid.rs:301-409, :434-476,
// src/system/hbonds.rs:248-265), run every frame of a trajectory loop.  Per frame the result is what gr_group_pairs_within gives for that
// slot: all pairs (i in group1, j in group2, i != j) with gr_distance<4, true>(x_j, x_i, 7, box) <= cutoff, by i then j.  Here the two
// groups and the cut-off are ONE object, a block of resident slots is one call, and the lists stay on the device.
//
// A segment of the batch is worked in PIECES of frames so that the key, rank and sorted-atom workspace stays within GR_CT_WS_BYTES
// (256 MiB; one frame where that alone is larger).  The launches of a piece, none of which depends on the number of its frames:
//   k_ct_assign       every atom of both groups of every frame -> key = (table, frame, cell), rank in its cell by atomicAdd; the first
//                     atom without position per (frame, group) by atomicMin on ordinals.  The grid of a frame is gr_cellgrid_make of
//                     its own box, coarsened as hb_grid does to at most max(64, 2 max(n1, n2)) cells; group 2 fills table 0 of the
//                     key space, group 1 table 1 (one table when both groups hold the same atoms)
//   rocprim::exclusive_scan   cell counts -> cell starts, one scan over the whole key space
//   k_ct_scatter      float4 (x, y, z, atom index) and the group ordinal into cell order
//   k_ct_walk<COUNT>  one 64-lane workgroup per RUN of `rx` query cells adjacent along x (grid-stride over the piece's runs).  The
//                     neighbour cells of a run are at most 9 rows of rx + 2 cells, each row one contiguous range of table 0 (plus the
//                     periodic wrap: at most 27 ranges, no cell twice).  The candidates are staged ONCE in an LDS tile of GR_CT_TILE
//                     float4, a (atom index, tile position) key per candidate is sorted in LDS (bitonic network), and every query of
//                     the run is tested against the tile in index order: a team of GR_CT_TEAM lanes shares one query, lane s takes
//                     candidates s, s + TEAM, ...; the hits of a round are placed by __ballot and popcounts within the team.  The
//                     count of a query is a plain store at (frame, query ordinal)
//   k_ct_mask         the queries of a frame with a missing position count nothing
//   rocprim::exclusive_scan   counts -> offsets;  k_ct_pack: frame offsets + the error words, one read-back
//   k_ct_walk<WRITE>  the same walk writing (i, j, d) at offsets[ordinal] + position: ordered by i through the scan and by j through the
//                     sorted tile.  No atomic decides a position or a count, no lane sorts in global memory.
// Candidates beyond one tile (a dense cluster in one cell) are worked tile by tile: counts and bins do not care, and in the write pass the
// runs of a query (one per tile, each ordered) are sorted at the end by the whole workgroup with the same network on its segment.
// counts: the COUNT walk and its per-query stores; hist: the walk with per-workgroup u32 bins in LDS, flushed with 64-bit adds when the
// workgroup's frame changes.  The distance is k_cg_pairs' call expression, argument for argument.
#pragma once
#include <rocprim/rocprim.hpp>
#include "gr_cellgrid.h"

#if defined(__HIPCC__)

#ifndef GR_CT_TILE
#define GR_CT_TILE 512u                      /* candidates staged at once: gr_contacts_stat(GR_CT_STAT_TILE) */
#endif
#ifndef GR_CT_TEAM
#define GR_CT_TEAM 16u                       /* lanes that share a query */
#endif
#ifndef GR_CT_UNROLL
#define GR_CT_UNROLL 2                       /* candidates in flight per lane and round of a team */
#endif
#define GR_CT_RX_MAX 8u                      /* query cells per run, at most */
#define GR_CT_MAX_WG 8192u                   /* workgroups of a walk, at most (grid-stride beyond) */
#define GR_CT_WS_BYTES (256ull << 20)        /* workspace of a piece */
#define GR_CT_MAX_BINS 4096u

struct GrCtFrame {        // one frame of a piece, built on the host from boxes_host
    GrCellGrid g;
    uint32_t kbase;       // first key of the frame's cells in a table
    uint32_t ubase;       // first run of the frame among the piece's runs
    uint32_t rx;          // query cells per run
    uint32_t ok;          // 0: the frame failed a host check -- no keys, no runs
};

enum { GR_CT_COUNT = 0, GR_CT_WRITE = 1, GR_CT_HIST = 2 };

struct gr_contacts {
    gr_ctx *c = nullptr;
    float cutoff = 0.0f;
    uint32_t n1 = 0, n2 = 0;
    bool same = false;                                       // both groups hold the same atoms: one table
    std::vector<uint32_t> atoms1, atoms2;                    // the snapshot, group order
    grbuf::Dev<uint32_t> atoms_dev;                          // [n1 + n2]
    uint32_t piece_frames = 0;                               // 0: by GR_CT_WS_BYTES
    uint32_t walk_groups = 0;                                // 0: GR_CT_MAX_WG
    grbuf::Dev<unsigned char> ws;                            // the piece's workspace
    grbuf::Pinned<unsigned char> hbuf;                       // frames up, offsets + error words down
    grbuf::Dev<uint32_t> li[2], lj[2]; grbuf::Dev<float> ld[2]; int cur = 0;   // the lists: [cur]; the other set is where they move to grow
    grbuf::Dev<uint64_t> off_dev;                            // [n_frames + 1]
    std::vector<uint64_t> off_host;                          // [n_frames + 1] of the last pairs call
    uint64_t n_frames = 0, total = 0;                        // the last pairs call's result (0 frames after a failed call)
    bool have_lists = false;                                 // false: count only (the total exceeded max_pairs)
    uint64_t last_launches = 0, last_pieces = 0;
    uint64_t last_runs = 0, last_cells = 0, last_rx_min = 0, last_rx_max = 0, last_walk_groups = 0;   // over the frames that passed their host checks
};

namespace {

// the all-ascending bitonic network on n elements (virtually padded to a power of two with +inf, which never moves): cx(a, b), a < b < n,
// puts the smaller element at a; barrier() separates the stages
template <class CX, class Barrier>
__device__ __forceinline__ void ct_bitonic(uint32_t n, uint32_t lane, CX cx, Barrier barrier) {
    uint32_t lp = 0; while ((1u << lp) < n) ++lp;                  // P = 2^lp
    const uint32_t half = (1u << lp) >> 1;
    for (uint32_t lk = 1; lk <= lp; ++lk) {                         // blocks of k = 2^lk: the first step mirrors, the others shift
        const uint32_t k = 1u << lk, h = k >> 1;
        for (uint32_t t = lane; t < half; t += 64u) {
            const uint32_t a = ((t >> (lk - 1u)) << lk) | (t & (h - 1u)), b = a ^ (k - 1u);
            if (b < n) cx(a, b);
        }
        barrier();
        for (uint32_t lj = lk - 1u; lj-- > 0u;) {                   // j = 2^lj = h / 2 ... 1
            const uint32_t j = 1u << lj;
            for (uint32_t t = lane; t < half; t += 64u) {
                const uint32_t a = ((t >> lj) << (lj + 1u)) | (t & (j - 1u)), b = a + j;
                if (b < n) cx(a, b);
            }
            barrier();
        }
    }
}

// e = frame * per + r: atom r of the piece's frames (group 2's atoms, then group 1's unless `same`)
__global__ __launch_bounds__(256) void k_ct_assign(const float *__restrict__ frames, size_t stride, uint32_t slot0, const GrBox *__restrict__ boxes,
                                                   const GrCtFrame *__restrict__ fr, const uint32_t *__restrict__ atoms1, const uint32_t *__restrict__ atoms2,
                                                   uint32_t n2, uint32_t per, uint64_t n_el, uint32_t table1, uint32_t *__restrict__ cell_count,
                                                   uint32_t *__restrict__ keys, uint32_t *__restrict__ ranks, uint32_t *__restrict__ bad) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n_el) return;
    const uint32_t f = (uint32_t)(e / per), r = (uint32_t)(e - (uint64_t)f * per);
    if (!fr[f].ok) { keys[e] = GR_NOIDX; return; }
    const uint32_t which = r >= n2 ? 1u : 0u, k = which ? r - n2 : r;
    const GrCellGrid g = fr[f].g;
    float x, y, z;
    gr_pos_load(frames + (size_t)(slot0 + f) * stride, which ? atoms1[k] : atoms2[k], x, y, z);
    if (x != x) { atomicMin(bad + 2u * f + which, k); keys[e] = GR_NOIDX; return; }     // ordinal of the first atom without position (group order)
    uint32_t c[3];
    gr_cg_cell_of(x, y, z, boxes[f], g, c);
    const uint32_t key = which * table1 + fr[f].kbase + (c[2] * g.nc[1] + c[1]) * g.nc[0] + c[0];
    keys[e] = key;
    ranks[e] = atomicAdd(cell_count + key, 1u);
}

__global__ __launch_bounds__(256) void k_ct_scatter(const float *__restrict__ frames, size_t stride, uint32_t slot0, const uint32_t *__restrict__ atoms1,
                                                    const uint32_t *__restrict__ atoms2, uint32_t n2, uint32_t per, uint64_t n_el, const uint32_t *__restrict__ keys,
                                                    const uint32_t *__restrict__ ranks, const uint32_t *__restrict__ cell_start, float4 *__restrict__ sorted,
                                                    uint32_t *__restrict__ ord) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n_el) return;
    const uint32_t key = keys[e];
    if (key == GR_NOIDX) return;
    const uint32_t f = (uint32_t)(e / per), r = (uint32_t)(e - (uint64_t)f * per);
    const uint32_t which = r >= n2 ? 1u : 0u, k = which ? r - n2 : r, a = which ? atoms1[k] : atoms2[k];
    float x, y, z;
    gr_pos_load(frames + (size_t)(slot0 + f) * stride, a, x, y, z);
    const uint32_t at = cell_start[key] + ranks[e];
    sorted[at] = make_float4(x, y, z, __uint_as_float(a));
    ord[at] = k;
}

// grid-stride over the piece's runs, one 64-lane workgroup per run.  COUNT: counts[f * n1 + ordinal]; WRITE: (i, j, d) at
// base + offs[f * n1 + ordinal] (counts is the cursor between tiles); HIST: hist[f * nbins + bin]
template <int MODE>
__global__ __launch_bounds__(64) void k_ct_walk(const GrBox *__restrict__ boxes, const GrCtFrame *__restrict__ fr, uint32_t n_fr, uint32_t n_units, uint32_t table1,
                                                const uint32_t *__restrict__ cell_start, const float4 *__restrict__ sorted, const uint32_t *__restrict__ ord,
                                                uint32_t n1, float cutoff, uint32_t *__restrict__ counts, const unsigned long long *__restrict__ offs,
                                                const uint32_t *__restrict__ bad, unsigned long long base, uint32_t *__restrict__ out_i, uint32_t *__restrict__ out_j,
                                                float *__restrict__ out_d, float bins_per_nm, uint32_t nbins, unsigned long long *__restrict__ hist) {
    __shared__ float4 tile[GR_CT_TILE];
    __shared__ unsigned long long skey[GR_CT_TILE];
    __shared__ uint32_t r_at[27], r_pre[28];
    extern __shared__ uint32_t lhist[];                 // [nbins], HIST only
    const uint32_t lane = threadIdx.x, team = lane / GR_CT_TEAM, sub = lane % GR_CT_TEAM, n_teams = 64u / GR_CT_TEAM;
    const unsigned long long team_mask = (1ull << GR_CT_TEAM) - 1ull;
    uint32_t hist_f = GR_NOIDX;
    if (MODE == GR_CT_HIST) { for (uint32_t b = lane; b < nbins; b += 64u) lhist[b] = 0u; __syncthreads(); }
    for (uint32_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        // the run's frame: the last one whose first run is <= u
        uint32_t f = 0;
        { uint32_t lo = 0, hi = n_fr; while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (fr[mid].ubase <= u) lo = mid; else hi = mid; } f = lo; }
        const GrCtFrame F = fr[f];
        const GrCellGrid g = F.g;
        if (MODE == GR_CT_WRITE && (bad[2u * f] != GR_NOIDX || bad[2u * f + 1u] != GR_NOIDX)) continue;     // a failed frame: its offsets hold no room
        const uint32_t nxr = (g.nc[0] + F.rx - 1u) / F.rx;
        uint32_t v = u - F.ubase;
        const uint32_t xr = v % nxr; v /= nxr;
        const uint32_t cy = v % g.nc[1], cz = v / g.nc[1];
        const uint32_t x0 = xr * F.rx, xe = min(x0 + F.rx, g.nc[0]) - 1u;
        const uint32_t qrow = table1 + F.kbase + (cz * g.nc[1] + cy) * g.nc[0];
        const uint32_t q0 = cell_start[qrow + x0], nq = cell_start[qrow + xe + 1u] - q0;
        if (nq == 0u) continue;
        if (MODE == GR_CT_HIST && hist_f != f) {
            if (hist_f != GR_NOIDX) {
                __syncthreads();
                for (uint32_t b = lane; b < nbins; b += 64u) { const uint32_t h = lhist[b]; if (h) { atomicAdd(hist + (size_t)hist_f * nbins + b, (unsigned long long)h); lhist[b] = 0u; } }
                __syncthreads();
            }
            hist_f = f;
        }
        // the candidates' ranges: 3 x 3 rows (CellNeighbors::convert per axis, as k_cg_pairs: 3 cells -> -1 0 1, 2 -> 0 1, 1 -> 0) of three parts each
        if (lane < 27u) {
            const int lo1 = g.nc[1] >= 3u ? -1 : 0, hi1 = g.nc[1] >= 2u ? 1 : 0, lo2 = g.nc[2] >= 3u ? -1 : 0, hi2 = g.nc[2] >= 2u ? 1 : 0;
            const int dz = lo2 + (int)(lane / 9u), dy = lo1 + (int)((lane / 3u) % 3u);
            const uint32_t part = lane % 3u;
            uint32_t at = 0, len = 0;
            if (dz <= hi2 && dy <= hi1) {
                const uint32_t ry = (uint32_t)((int)cy + dy + (int)g.nc[1]) % g.nc[1], rz = (uint32_t)((int)cz + dz + (int)g.nc[2]) % g.nc[2];
                const uint32_t row = F.kbase + (rz * g.nc[1] + ry) * g.nc[0];
                const bool whole = g.nc[0] < 3u || (xe - x0 + 3u) >= g.nc[0];          // the run and its two neighbours cover the row
                uint32_t a = 1, b = 0;                                                  // cells a .. b of the row (empty)
                if (whole) { if (part == 0u) { a = 0; b = g.nc[0] - 1u; } }
                else if (part == 0u) { a = x0 ? x0 - 1u : 0u; b = min(xe + 1u, g.nc[0] - 1u); }
                else if (part == 1u) { if (x0 == 0u) a = b = g.nc[0] - 1u; }              // the wrap below cell 0
                else { if (xe + 1u == g.nc[0]) a = b = 0u; }                              // the wrap beyond the last cell
                if (a <= b) { at = cell_start[row + a]; len = cell_start[row + b + 1u] - at; }
            }
            r_at[lane] = at; r_pre[lane + 1u] = len;
        }
        __syncthreads();
        if (lane == 0u) { uint32_t s = 0; r_pre[0] = 0; for (uint32_t r = 0; r < 27u; ++r) { s += r_pre[r + 1u]; r_pre[r + 1u] = s; } }
        __syncthreads();
        const uint32_t M = r_pre[27];
        const bool multi = M > GR_CT_TILE;
        const GrBox &box = boxes[f];
        for (uint32_t tb = 0; tb < M; tb += GR_CT_TILE) {
            const uint32_t m = min(GR_CT_TILE, M - tb);
            for (uint32_t t = lane; t < m; t += 64u) {
                const uint32_t e = tb + t;
                uint32_t r = 0;
                while (r < 26u && e >= r_pre[r + 1u]) ++r;
                const float4 A = sorted[r_at[r] + (e - r_pre[r])];
                tile[t] = A;
                skey[t] = ((unsigned long long)__float_as_uint(A.w) << 32) | t;
            }
            __syncthreads();
            ct_bitonic(m, lane, [&](uint32_t a, uint32_t b) { const unsigned long long ka = skey[a], kb = skey[b]; if (kb < ka) { skey[a] = kb; skey[b] = ka; } },
                       [] { __syncthreads(); });
            for (uint32_t qb = 0; qb < nq; qb += n_teams) {
                const uint32_t qi = qb + team;
                const bool qv = qi < nq;
                float4 Q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                uint32_t k = 0;
                if (qv) { Q = sorted[q0 + qi]; k = ord[q0 + qi]; }
                const uint32_t i = __float_as_uint(Q.w);
                const size_t idx = (size_t)f * n1 + k;
                uint32_t cur = 0, room = 0;
                unsigned long long at = 0;
                if (MODE != GR_CT_HIST && qv && tb != 0u) cur = counts[idx];
                if (MODE == GR_CT_WRITE && qv) { at = offs[idx]; room = (uint32_t)(offs[idx + 1u] - at); at += base; }
                for (uint32_t t0 = 0; t0 < m; t0 += GR_CT_TEAM * GR_CT_UNROLL) {
                    bool hit[GR_CT_UNROLL];
                    uint32_t j[GR_CT_UNROLL]; float d[GR_CT_UNROLL];
#pragma unroll
                    for (int v = 0; v < GR_CT_UNROLL; ++v) {
                        const uint32_t t = t0 + (uint32_t)v * GR_CT_TEAM + sub;
                        hit[v] = false; j[v] = 0; d[v] = 0.0f;
                        if (qv && t < m) {
                            const unsigned long long key = skey[t];
                            j[v] = (uint32_t)(key >> 32);
                            const float4 A = tile[(uint32_t)key];
                            if (j[v] != i) {                                                               // hbonds.rs:250
                                d[v] = gr_distance<4, true>(A.x, A.y, A.z, Q.x, Q.y, Q.z, 7, box);         // acceptor.distance(donor), :261
                                hit[v] = !(d[v] > cutoff);                                                 // :262-264
                            }
                        }
                    }
#pragma unroll
                    for (int v = 0; v < GR_CT_UNROLL; ++v) {
                        const unsigned long long bits = (__ballot(hit[v]) >> (team * GR_CT_TEAM)) & team_mask;
                        if (MODE == GR_CT_HIST) {
                            if (hit[v] && d[v] >= 0.0f) { const float fb = d[v] * bins_per_nm; if (fb < (float)nbins) atomicAdd(&lhist[(uint32_t)fb], 1u); }
                        } else {
                            if (MODE == GR_CT_WRITE && hit[v]) {
                                const uint32_t p = cur + (uint32_t)__popcll(bits & ((1ull << sub) - 1ull));
                                if (p < room) { out_i[at + p] = i; out_j[at + p] = j[v]; out_d[at + p] = d[v]; }
                            }
                            cur += (uint32_t)__popcll(bits);
                        }
                    }
                }
                if (MODE != GR_CT_HIST && qv && sub == 0u) counts[idx] = cur;
            }
            if (multi) __threadfence();                 // (the next tile's teams read the cursors)
            __syncthreads();
        }
        if (MODE == GR_CT_WRITE && multi) {
            // the runs of a query arrived tile by tile, each ordered by j: the workgroup sorts the query's segment
            for (uint32_t qi = 0; qi < nq; ++qi) {
                const size_t idx = (size_t)f * n1 + ord[q0 + qi];
                const unsigned long long at = base + offs[idx];
                const uint32_t n = (uint32_t)(offs[idx + 1u] - offs[idx]);
                if (n < 2u) continue;
                uint32_t *pj = out_j + at; float *pd = out_d + at;
                ct_bitonic(n, lane, [&](uint32_t a, uint32_t b) {
                               const uint32_t ja = pj[a], jb = pj[b];
                               if (jb < ja) { const float da = pd[a], db = pd[b]; pj[a] = jb; pj[b] = ja; pd[a] = db; pd[b] = da; }
                           },
                           [] { __threadfence(); __syncthreads(); });
            }
        }
    }
    if (MODE == GR_CT_HIST && hist_f != GR_NOIDX) {
        __syncthreads();
        for (uint32_t b = lane; b < nbins; b += 64u) { const uint32_t h = lhist[b]; if (h) atomicAdd(hist + (size_t)hist_f * nbins + b, (unsigned long long)h); }
    }
}

// the queries of a frame with a missing position count nothing; counts[n_t] = 0 closes the scan
__global__ __launch_bounds__(256) void k_ct_mask(uint32_t *__restrict__ counts, uint32_t n1, uint64_t n_t, const uint32_t *__restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t > n_t) return;
    if (t == n_t) { counts[t] = 0; return; }
    const uint32_t f = (uint32_t)(t / n1);
    if (bad[2u * f] != GR_NOIDX || bad[2u * f + 1u] != GR_NOIDX) counts[t] = 0;
}

// rb[f] = offset of frame f's first query, rb[n_fr] = the piece's total, then the 2 n_fr error words
__global__ __launch_bounds__(256) void k_ct_pack(const unsigned long long *__restrict__ offs, uint32_t n1, uint32_t n_fr, const uint32_t *__restrict__ bad,
                                                 unsigned long long *__restrict__ rb) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t <= n_fr) rb[t] = offs[(uint64_t)t * n1];
    if (t < 2u * n_fr) reinterpret_cast<uint32_t *>(rb + n_fr + 1u)[t] = bad[t];
}

size_t ct_al(size_t v) { return (v + 255) & ~(size_t)255; }

// the box checks of one frame, in gr_group_pairs_within's order and words
int ct_box_check(gr_ctx *c, uint32_t slot) {
    if (c->box_status[slot] == GR_E_NO_BOX) return fail(c, GR_E_NO_BOX, "simulation box does not exist");
    if (c->box_status[slot] != GR_OK) return fail(c, c->box_status[slot], "invalid simulation box");
    if (c->strict && !c->boxes_host[slot].ortho) return fail(c, GR_E_NOT_ORTHOGONAL, "simulation box is not orthogonal");
    return GR_OK;
}

// the cut-off's grid, coarsened as hb_grid does where it would hold many more cells than the larger group has atoms
GrCellGrid ct_grid(const GrBox &box, float cutoff, uint64_t cells_cap) {
    float cs = cutoff;
    GrCellGrid g = gr_cellgrid_make(box, cs);
    while (g.ncells > cells_cap && g.ncells > 1) { cs *= 1.25f; g = gr_cellgrid_make(box, cs); }
    return g;
}
uint64_t ct_cells_cap(const gr_contacts *ct) { return std::max<uint64_t>(64, 2ull * std::max(ct->n1, ct->n2)); }

// query cells per run: the expected candidates of a run (9 rows of rx + 2 cells) fill about half a tile
uint32_t ct_run_cells(const gr_contacts *ct, const GrCellGrid &g) {
    const double per_cell = (double)ct->n2 / (double)g.ncells;
    const double rx = (double)GR_CT_TILE / (2.0 * 9.0 * std::max(per_cell, 1e-3)) - 2.0;
    const uint32_t r = rx >= (double)GR_CT_RX_MAX ? GR_CT_RX_MAX : (rx >= 1.0 ? (uint32_t)rx : 1u);
    return std::min<uint32_t>(r, g.nc[0]);
}

// workspace bytes that one frame of a piece adds, at most
uint64_t ct_frame_bytes(const gr_contacts *ct, uint32_t nbins) {
    const uint64_t per = (uint64_t)ct->n2 + (ct->same ? 0u : ct->n1), tables = ct->same ? 1u : 2u;
    return per * 28u + (uint64_t)ct->n1 * 12u + tables * ct_cells_cap(ct) * 8u + (uint64_t)nbins * 8u + sizeof(GrCtFrame) + 64u;
}
uint32_t ct_piece_frames(const gr_contacts *ct, uint32_t nbins, uint32_t nb) {
    const uint64_t p = ct->piece_frames ? ct->piece_frames : GR_CT_WS_BYTES / ct_frame_bytes(ct, nbins);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(p, 1), nb);
}

// the lists hold `keep` pairs and are about to receive up to `need` in all: bigger blocks take the pairs over
int ct_list_room(gr_contacts *ct, uint64_t keep, uint64_t need) {
    gr_ctx *c = ct->c;
    if (need <= ct->li[ct->cur].cap()) return GR_OK;
    const int other = 1 - ct->cur;
    auto room = [](size_t n) { return n + n / 2 + 64; };                                 // (geometric: a call of many pieces moves its lists a few times)
    HIPCHK(c, ct->li[other].reserve((size_t)need, room));
    HIPCHK(c, ct->lj[other].reserve((size_t)need, room));
    HIPCHK(c, ct->ld[other].reserve((size_t)need, room));
    if (keep) {
        HIPCHK(c, hipMemcpyAsync(ct->li[other].get(), ct->li[ct->cur].get(), (size_t)keep * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(ct->lj[other].get(), ct->lj[ct->cur].get(), (size_t)keep * 4, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(ct->ld[other].get(), ct->ld[ct->cur].get(), (size_t)keep * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));            // the old blocks' last reader
    ct->li[ct->cur].release(); ct->lj[ct->cur].release(); ct->ld[ct->cur].release();
    ct->cur = other;
    return GR_OK;
}

// one batched call.  mode GR_CT_WRITE: pairs (n_pairs, lists in the object); GR_CT_COUNT: per_atom + n_pairs; GR_CT_HIST: hist
int ct_run(gr_contacts *ct, int mode, uint32_t first_slot, uint32_t n_frames, uint64_t max_pairs, uint32_t nbins, uint32_t *per_atom, uint64_t *n_pairs,
           uint64_t *hist, int *status_out) {
    gr_ctx *c = ct->c;
    const bool pairs = mode == GR_CT_WRITE;
    if (pairs) { ct->n_frames = 0; ct->total = 0; ct->have_lists = false; }
    ct->last_launches = 0; ct->last_pieces = 0;
    ct->last_runs = 0; ct->last_cells = 0; ct->last_rx_min = 0; ct->last_rx_max = 0; ct->last_walk_groups = 0;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    if (mode == GR_CT_HIST && (nbins == 0 || nbins > GR_CT_MAX_BINS)) return fail(c, GR_E_INVALID_ARG, "histogram: 1 .. 4096 bins over (0, cutoff)");
    if (mode == GR_CT_HIST && !hist) return fail(c, GR_E_INVALID_ARG, "hist is NULL");
    (void)hipSetDevice(c->device);
    const uint32_t n1 = ct->n1, n2 = ct->n2, tables = ct->same ? 1u : 2u, per = n2 + (ct->same ? 0u : n1);
    const bool work = n1 != 0 && n2 != 0;                    // an empty group: nothing further is checked, no position is looked at
    const uint64_t cells_cap = ct_cells_cap(ct);
    const float bins_per_nm = mode == GR_CT_HIST ? (float)nbins / ct->cutoff : 0.0f;
    if (per_atom && n1) memset(per_atom, 0, (size_t)n_frames * n1 * sizeof(uint32_t));
    if (hist) memset(hist, 0, (size_t)n_frames * nbins * sizeof(uint64_t));
    if (n_pairs) memset(n_pairs, 0, (size_t)n_frames * sizeof(uint64_t));
    std::vector<uint64_t> off_host;
    if (pairs) { HIPCHK(c, ct->off_dev.reserve((size_t)n_frames + 1, grbuf::exact)); off_host.assign((size_t)n_frames + 1, 0); }
    const uint32_t *atoms1_d = ct->atoms_dev.get(), *atoms2_d = ct->atoms_dev.get() + n1;
    uint64_t total = 0;
    bool writing = pairs;                                    // until the running total passes max_pairs
    grb::FirstError<gr_ctx> fe;
    std::vector<uint32_t> seg_bad;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, [&](uint32_t slot) { return ct_box_check(c, slot); });
        seg_bad.assign(2 * (size_t)nb, GR_NOIDX);
        if (work && pre.any_ok) {
            SlotUse use(c, s0, nb);
            const uint32_t piece_max = ct_piece_frames(ct, mode == GR_CT_HIST ? nbins : 0u, nb);
            for (uint32_t p0 = 0; p0 < nb; p0 += piece_max) {
                const uint32_t np = std::min<uint32_t>(piece_max, nb - p0);
                // the piece's frames, key space and runs
                std::vector<GrCtFrame> frs(np);
                uint64_t nkeys = 0, n_units = 0;
                for (uint32_t f = 0; f < np; ++f) {
                    GrCtFrame &F = frs[f];
                    memset(&F, 0, sizeof F);
                    F.kbase = (uint32_t)nkeys; F.ubase = (uint32_t)n_units; F.rx = 1;
                    if (!pre.ok(p0 + f)) continue;
                    F.g = ct_grid(c->boxes_host[s0 + p0 + f], ct->cutoff, cells_cap);
                    F.rx = ct_run_cells(ct, F.g); F.ok = 1;
                    nkeys += F.g.ncells;
                    ct->last_cells += F.g.ncells;
                    ct->last_rx_min = ct->last_rx_max ? std::min<uint64_t>(ct->last_rx_min, F.rx) : F.rx;
                    ct->last_rx_max = std::max<uint64_t>(ct->last_rx_max, F.rx);
                    n_units += (uint64_t)F.g.nc[2] * F.g.nc[1] * ((F.g.nc[0] + F.rx - 1u) / F.rx);
                }
                const uint64_t n_el = (uint64_t)np * per, n_t = (uint64_t)np * n1, n_keys_all = nkeys * tables;
                if (n_el >= 0xFFFFFFFFull || n_t >= 0xFFFFFFFFull || n_keys_all >= 0x7FFFFFFFull || n_units >= 0x7FFFFFFFull)
                    return fail(c, GR_E_INVALID_ARG, "contacts: the piece is too large (gr_contacts_set_piece_frames)");
                ++ct->last_pieces;
                if (n_units == 0) continue;                  // every frame of the piece failed its checks
                ct->last_runs += n_units;
                // workspace
                size_t tmp_cells = 0, tmp_q = 0;
                (void)rocprim::exclusive_scan(nullptr, tmp_cells, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n_keys_all + 1, rocprim::plus<uint32_t>(), c->stream);
                (void)rocprim::exclusive_scan(nullptr, tmp_q, (uint32_t *)nullptr, (unsigned long long *)nullptr, 0ull, (size_t)n_t + 1, rocprim::plus<unsigned long long>(), c->stream);
                const size_t rb_bytes = ct_al(8 * ((size_t)np + 1) + 8 * (size_t)np), hist_bytes = mode == GR_CT_HIST ? ct_al(8 * (size_t)np * nbins) : 0;
                const size_t o_fr = 0, o_cc = o_fr + ct_al(sizeof(GrCtFrame) * np), o_cs = o_cc + ct_al(4 * (n_keys_all + 1)), o_key = o_cs + ct_al(4 * (n_keys_all + 1)),
                             o_rank = o_key + ct_al(4 * n_el), o_sort = o_rank + ct_al(4 * n_el), o_ord = o_sort + ct_al(16 * n_el), o_cnt = o_ord + ct_al(4 * n_el),
                             o_off = o_cnt + ct_al(4 * (n_t + 1)), o_rb = o_off + ct_al(8 * (n_t + 1)), o_bad = o_rb + rb_bytes, o_hist = o_bad + ct_al(8 * (size_t)np),
                             o_tmp = o_hist + hist_bytes, ws_bytes = o_tmp + ct_al(std::max(tmp_cells, tmp_q));
                HIPCHK(c, ct->ws.reserve(ws_bytes, grbuf::quarter_aligned256));
                HIPCHK(c, ct->hbuf.reserve(ct_al(sizeof(GrCtFrame) * np) + rb_bytes, grbuf::quarter_aligned256));
                unsigned char *W = ct->ws.get();
                GrCtFrame *fr_d = (GrCtFrame *)(W + o_fr);
                uint32_t *cell_count = (uint32_t *)(W + o_cc), *cell_start = (uint32_t *)(W + o_cs), *keys = (uint32_t *)(W + o_key), *ranks = (uint32_t *)(W + o_rank),
                         *ord = (uint32_t *)(W + o_ord), *counts = (uint32_t *)(W + o_cnt), *bad = (uint32_t *)(W + o_bad);
                float4 *sorted = (float4 *)(W + o_sort);
                unsigned long long *offs = (unsigned long long *)(W + o_off), *rb = (unsigned long long *)(W + o_rb), *hist_d = (unsigned long long *)(W + o_hist);
                GrCtFrame *fr_h = (GrCtFrame *)ct->hbuf.get();
                unsigned char *rb_h = ct->hbuf.get() + ct_al(sizeof(GrCtFrame) * np);
                memcpy(fr_h, frs.data(), sizeof(GrCtFrame) * np);
                const GrBox *boxes = c->boxes_dev + s0 + p0;
                const uint32_t table1 = ct->same ? 0u : (uint32_t)nkeys;
                auto blocks = [](uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); };
                const dim3 walk_grid((uint32_t)std::min<uint64_t>(n_units, ct->walk_groups ? ct->walk_groups : GR_CT_MAX_WG));
                ct->last_walk_groups = std::max<uint64_t>(ct->last_walk_groups, walk_grid.x);
                HIPCHK(c, hipMemcpyAsync(fr_d, fr_h, sizeof(GrCtFrame) * np, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipMemsetAsync(cell_count, 0, 4 * (n_keys_all + 1), c->stream));
                HIPCHK(c, hipMemsetAsync(bad, 0xFF, 8 * (size_t)np, c->stream));
                if (mode == GR_CT_HIST) HIPCHK(c, hipMemsetAsync(hist_d, 0, 8 * (size_t)np * nbins, c->stream));
                else HIPCHK(c, hipMemsetAsync(counts, 0, 4 * (n_t + 1), c->stream));           // (a query that no run meets -- no position -- counts 0)
                k_ct_assign<<<blocks(n_el), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0 + p0, boxes, fr_d, atoms1_d, atoms2_d, n2, per, n_el, table1,
                                                                       cell_count, keys, ranks, bad);
                size_t tsz = std::max(tmp_cells, tmp_q);
                HIPCHK(c, rocprim::exclusive_scan(W + o_tmp, tsz, cell_count, cell_start, 0u, (size_t)n_keys_all + 1, rocprim::plus<uint32_t>(), c->stream));
                k_ct_scatter<<<blocks(n_el), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0 + p0, atoms1_d, atoms2_d, n2, per, n_el, keys, ranks, cell_start, sorted, ord);
                ct->last_launches += 3;
                if (mode == GR_CT_HIST) {
                    k_ct_walk<GR_CT_HIST><<<walk_grid, dim3(64), nbins * sizeof(uint32_t), c->stream>>>(boxes, fr_d, np, (uint32_t)n_units, table1, cell_start, sorted, ord, n1, ct->cutoff,
                                                                                                       nullptr, nullptr, bad, 0ull, nullptr, nullptr, nullptr, bins_per_nm, nbins, hist_d);
                    HIPCHK(c, hipGetLastError());
                    ct->last_launches += 1;
                    HIPCHK(c, hipMemcpyAsync(hist + ((size_t)b0 + p0) * nbins, hist_d, 8 * (size_t)np * nbins, hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipMemcpyAsync(rb_h, bad, 8 * (size_t)np, hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    memcpy(seg_bad.data() + 2 * (size_t)p0, rb_h, 8 * (size_t)np);
                    continue;
                }
                k_ct_walk<GR_CT_COUNT><<<walk_grid, dim3(64), 0, c->stream>>>(boxes, fr_d, np, (uint32_t)n_units, table1, cell_start, sorted, ord, n1, ct->cutoff, counts, nullptr, bad,
                                                                               0ull, nullptr, nullptr, nullptr, 0.0f, 0u, nullptr);
                k_ct_mask<<<blocks(n_t + 1), dim3(256), 0, c->stream>>>(counts, n1, n_t, bad);
                tsz = std::max(tmp_cells, tmp_q);
                HIPCHK(c, rocprim::exclusive_scan(W + o_tmp, tsz, counts, offs, 0ull, (size_t)n_t + 1, rocprim::plus<unsigned long long>(), c->stream));
                k_ct_pack<<<blocks(2 * (uint64_t)np + 1), dim3(256), 0, c->stream>>>(offs, n1, np, bad, rb);
                HIPCHK(c, hipGetLastError());
                ct->last_launches += 4;
                HIPCHK(c, hipMemcpyAsync(rb_h, rb, 8 * ((size_t)np + 1) + 8 * (size_t)np, hipMemcpyDeviceToHost, c->stream));
                if (per_atom) HIPCHK(c, hipMemcpyAsync(per_atom + ((size_t)b0 + p0) * n1, counts, 4 * (size_t)n_t, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                const unsigned long long *rb_offs = (const unsigned long long *)rb_h;
                memcpy(seg_bad.data() + 2 * (size_t)p0, rb_h + 8 * ((size_t)np + 1), 8 * (size_t)np);
                for (uint32_t f = 0; f < np; ++f) {
                    const uint64_t cnt = rb_offs[f + 1] - rb_offs[f];
                    if (n_pairs) n_pairs[(size_t)b0 + p0 + f] = cnt;
                    if (pairs) off_host[(size_t)b0 + p0 + f + 1] = total + rb_offs[f + 1];
                }
                const uint64_t kept = total;
                total += rb_offs[np];
                if (!pairs || total == kept) continue;
                if (total > max_pairs) writing = false;      // count only from here on; what was written is dropped at the end
                if (!writing) continue;
                st = ct_list_room(ct, kept, total); if (st) return st;
                k_ct_walk<GR_CT_WRITE><<<walk_grid, dim3(64), 0, c->stream>>>(boxes, fr_d, np, (uint32_t)n_units, table1, cell_start, sorted, ord, n1, ct->cutoff, counts, offs, bad, kept,
                                                                               ct->li[ct->cur].get(), ct->lj[ct->cur].get(), ct->ld[ct->cur].get(), 0.0f, 0u, nullptr);
                HIPCHK(c, hipGetLastError());
                ct->last_launches += 1;
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));      // (the next segment rewrites the workspace and the pinned blocks)
        }
        // offsets of frames that no piece worked on
        if (pairs) for (uint32_t f = 0; f < nb; ++f) if (off_host[(size_t)b0 + f + 1] < off_host[(size_t)b0 + f]) off_host[(size_t)b0 + f + 1] = off_host[(size_t)b0 + f];
        for (uint32_t f = 0; f < nb; ++f) {
            const int s = grb::close_frame(c, fe, pre, f, status_out, [&]() -> int {
                if (seg_bad[2 * (size_t)f] != GR_NOIDX) return fail(c, GR_E_NO_POSITION, "atom has no position", ct->atoms2[seg_bad[2 * (size_t)f]]);     // the grid (group 2) first
                if (seg_bad[2 * (size_t)f + 1] != GR_NOIDX) return fail(c, GR_E_NO_POSITION, "atom has no position", ct->atoms1[seg_bad[2 * (size_t)f + 1]]);
                return GR_OK;
            });
            if (s != GR_OK && hist) memset(hist + ((size_t)b0 + f) * nbins, 0, (size_t)nbins * sizeof(uint64_t));
        }
    }
    if (pairs) {
        HIPCHK(c, hipMemcpyAsync(ct->off_dev.get(), off_host.data(), ((size_t)n_frames + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ct->off_host.swap(off_host);
        ct->n_frames = n_frames; ct->total = total; ct->have_lists = writing;
    }
    return fe.finish(c);
}

void ct_reset(gr_contacts *ct) { ct->n_frames = 0; ct->total = 0; ct->have_lists = false; }

}  // namespace

extern "C" {

gr_contacts *gr_contacts_create(gr_ctx *c, const char *group1, const char *group2, float cutoff, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    const Group *a = need_group(c, group1, *status); if (!a) return nullptr;
    const Group *b = need_group(c, group2, *status); if (!b) return nullptr;
    if (!(cutoff > 0.0f)) { *status = fail(c, GR_E_INVALID_ARG, "cell size (cut-off) must be positive"); return nullptr; }              // cellgrid.rs:323-325
    gr_contacts *ct = new gr_contacts();
    ct->c = c; ct->cutoff = cutoff;
    ct->atoms1 = hb_group_atoms(*a); ct->atoms2 = hb_group_atoms(*b);
    ct->n1 = (uint32_t)ct->atoms1.size(); ct->n2 = (uint32_t)ct->atoms2.size();
    ct->same = ct->atoms1 == ct->atoms2;
    (void)hipSetDevice(c->device);
    bool ok = ct->atoms_dev.reserve((size_t)ct->n1 + ct->n2 + 1, grbuf::exact) == hipSuccess;
    if (ok && ct->n1) ok = hipMemcpy(ct->atoms_dev.get(), ct->atoms1.data(), 4 * (size_t)ct->n1, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && ct->n2) ok = hipMemcpy(ct->atoms_dev.get() + ct->n1, ct->atoms2.data(), 4 * (size_t)ct->n2, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && ct->off_dev.reserve(1, grbuf::exact) == hipSuccess && hipMemset(ct->off_dev.get(), 0, sizeof(uint64_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        delete ct;
        *status = fail(c, GR_E_HIP, "contacts: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return ct;
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_contacts_destroy(gr_contacts *ct) try {
    if (!ct) return;
    (void)hipSetDevice(ct->c->device);
    (void)hipStreamSynchronize(ct->c->stream);
    delete ct;                                             // (frees the grow-only buffers)
} catch (...) { }

int gr_contacts_pairs_batch(gr_contacts *ct, uint32_t first_slot, uint32_t n_frames, uint64_t max_pairs, uint64_t *n_pairs, uint64_t *n_total, int *status_out) try {
    if (!ct) return GR_E_INVALID_ARG;
    const int st = ct_run(ct, GR_CT_WRITE, first_slot, n_frames, max_pairs, 0, nullptr, n_pairs, nullptr, status_out);
    if (ct->n_frames != n_frames) ct_reset(ct);            // a hard error: an empty result of 0 frames
    else if (n_total) *n_total = ct->total;
    return st;
} catch (...) { if (ct) ct_reset(ct); return gr_abi_guard(); }

int gr_contacts_read(gr_contacts *ct, uint64_t *offsets, uint32_t *i, uint32_t *j, float *d, uint64_t cap, uint64_t *n_total) try {
    if (!ct) return GR_E_INVALID_ARG;
    gr_ctx *c = ct->c;
    int st = busy_check(c); if (st) return st;
    if (n_total) *n_total = ct->total;
    if (offsets) { if (ct->n_frames) memcpy(offsets, ct->off_host.data(), ((size_t)ct->n_frames + 1) * sizeof(uint64_t)); else offsets[0] = 0; }
    if (!i && !j && !d) return GR_OK;
    if (!i || !j || !d) return fail(c, GR_E_INVALID_ARG, "contacts: i, j and d are read together");
    if (ct->total && !ct->have_lists) return fail(c, GR_E_INVALID_ARG, "contacts: the last call counted only (its total exceeded max_pairs)");
    if (cap < ct->total) return fail(c, GR_E_INVALID_ARG, "contacts: the pair buffers are smaller than the result");
    if (!ct->total) return GR_OK;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(i, ct->li[ct->cur].get(), (size_t)ct->total * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(j, ct->lj[ct->cur].get(), (size_t)ct->total * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(d, ct->ld[ct->cur].get(), (size_t)ct->total * 4, hipMemcpyDeviceToHost));
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_contacts_read_device(gr_contacts *ct, const uint32_t **i_dev, const uint32_t **j_dev, const float **d_dev, const uint64_t **offsets_dev, uint64_t *n_frames,
                            uint64_t *n_total) try {
    if (!ct) return GR_E_INVALID_ARG;
    const bool have = ct->have_lists && ct->total;
    if (i_dev) *i_dev = have ? ct->li[ct->cur].get() : nullptr;
    if (j_dev) *j_dev = have ? ct->lj[ct->cur].get() : nullptr;
    if (d_dev) *d_dev = have ? ct->ld[ct->cur].get() : nullptr;
    if (offsets_dev) *offsets_dev = ct->off_dev.get();
    if (n_frames) *n_frames = ct->n_frames;
    if (n_total) *n_total = ct->total;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_contacts_count_batch(gr_contacts *ct, uint32_t first_slot, uint32_t n_frames, uint32_t *per_atom, uint64_t *n_pairs, int *status_out) try {
    if (!ct) return GR_E_INVALID_ARG;
    return ct_run(ct, GR_CT_COUNT, first_slot, n_frames, 0, 0, per_atom, n_pairs, nullptr, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_contacts_hist_batch(gr_contacts *ct, uint32_t first_slot, uint32_t n_frames, uint32_t nbins, uint64_t *hist, int *status_out) try {
    if (!ct) return GR_E_INVALID_ARG;
    return ct_run(ct, GR_CT_HIST, first_slot, n_frames, 0, nbins, nullptr, nullptr, hist, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_contacts_sizes(const gr_contacts *ct, uint64_t *n1, uint64_t *n2) try {
    if (!ct) return GR_E_INVALID_ARG;
    if (n1) *n1 = ct->n1;
    if (n2) *n2 = ct->n2;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_contacts_set_piece_frames(gr_contacts *ct, uint32_t n) try {
    if (!ct) return GR_E_INVALID_ARG;
    ct->piece_frames = n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_contacts_set_walk_groups(gr_contacts *ct, uint32_t n) try {
    if (!ct) return GR_E_INVALID_ARG;
    ct->walk_groups = n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_contacts_stat(const gr_contacts *ct, int key, uint64_t *value) try {
    if (!ct || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_CT_STAT_LAST_LAUNCHES: *value = ct->last_launches; return GR_OK;
    case GR_CT_STAT_LAST_PIECES: *value = ct->last_pieces; return GR_OK;
    case GR_CT_STAT_LAST_TOTAL: *value = ct->total; return GR_OK;
    case GR_CT_STAT_TILE: *value = GR_CT_TILE; return GR_OK;
    case GR_CT_STAT_LAST_RUNS: *value = ct->last_runs; return GR_OK;
    case GR_CT_STAT_LAST_CELLS: *value = ct->last_cells; return GR_OK;
    case GR_CT_STAT_LAST_RUN_CELLS_MIN: *value = ct->last_rx_min; return GR_OK;
    case GR_CT_STAT_LAST_RUN_CELLS_MAX: *value = ct->last_rx_max; return GR_OK;
    case GR_CT_STAT_LAST_WALK_GROUPS: *value = ct->last_walk_groups; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__

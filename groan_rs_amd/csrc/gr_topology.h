// gr_topology.h -- the bond topology of a context (host only: compiles without HIP, tests/test_topology_host.py includes it).
//
// The reference keeps the bonds inside its atoms (Atom::get_bonded, a sorted container) and derives the molecules from them on
// demand (src/system/modifying.rs:235-283, src/system/iterating.rs:399-432, src/system/mod.rs:349-377):
//   add_bond(i, j)          InvalidBond(i, j) when i == j, checked before OutOfRange(i), OutOfRange(j); a bond that exists is kept once
//   mol references          atoms in index order; the first unvisited atom with a bond starts a molecule: its LOWEST index
//   molecule order          breadth-first from the reference, neighbours in ascending index order
// Here the bonds are a CSR neighbour list (offsets + flat sorted neighbours) rebuilt from the pending pairs when first read, and the
// molecules are computed lazily after every change, as reset_mol_references does.  For the device the topology becomes one int32
// per atom (GrTopology::map): ref - i (<= 0) for an atom of a polyatomic molecule, GR_TOPO_NONE for every other atom and for the pad
// atoms behind the system, GR_TOPO_FARREF for a reference atom whose molecule reaches into a later 256-atom tile.
#pragma once
#include <algorithm>
#include <cstdint>
#include <deque>
#include <utility>
#include <vector>

#define GR_TOPO_NONE 1      /* not part of a polyatomic molecule (monoatomic atoms, pads) */
#define GR_TOPO_FARREF 2    /* a reference atom that atoms of LATER tiles read (long chains) */

namespace grt {

enum { TOPO_OK = 0, TOPO_INVALID_BOND = 1, TOPO_OUT_OF_RANGE = 2 };

struct GrTopology {
    uint64_t n = 0;                                   // atoms of the system
    std::vector<std::pair<uint32_t, uint32_t>> pend;  // bonds added since the CSR was last built (both directions)
    std::vector<uint64_t> off;                        // CSR offsets [n + 1]
    std::vector<uint32_t> nbr;                        // CSR neighbours, ascending per atom, no duplicates
    uint64_t version = 0;                             // bumped by every bond change (device map uploads follow it)
    // molecules, valid while mol_valid
    bool mol_valid = false;
    std::vector<uint64_t> refs;                       // reference atoms, ascending
    std::vector<uint64_t> mol_start;                  // [refs + 1]: molecule m's atoms are order[mol_start[m] .. mol_start[m + 1])
    std::vector<uint32_t> order;                      // breadth-first orders of all molecules, concatenated
    std::vector<uint32_t> rank;                       // per atom: position in its molecule's order (0 = the reference)
    std::vector<uint32_t> mol_of;                     // per atom: molecule index, or UINT32_MAX

    explicit GrTopology(uint64_t n_atoms = 0) : n(n_atoms), off(n_atoms + 1, 0) {}

    // AtomError checks of add_bond: InvalidBond before OutOfRange(i) before OutOfRange(j); *bad = the index
    int check(uint64_t i, uint64_t j, uint64_t *bad) const {
        if (i == j) { *bad = i; return TOPO_INVALID_BOND; }
        if (i >= n) { *bad = i; return TOPO_OUT_OF_RANGE; }
        if (j >= n) { *bad = j; return TOPO_OUT_OF_RANGE; }
        return TOPO_OK;
    }
    int add_bond(uint64_t i, uint64_t j, uint64_t *bad) { return add_bonds(&i, &j, 1, 1, bad, nullptr); }
    // pairs (a[k * stride], b[k * stride]); on the first bad pair nothing of the call is applied (*which = its ordinal)
    int add_bonds(const uint64_t *a, const uint64_t *b, uint64_t count, uint64_t stride, uint64_t *bad, uint64_t *which) {
        for (uint64_t k = 0; k < count; ++k) {
            const int st = check(a[k * stride], b[k * stride], bad);
            if (st != TOPO_OK) { if (which) *which = k; return st; }
        }
        pend.reserve(pend.size() + 2 * count);
        for (uint64_t k = 0; k < count; ++k) {
            const uint32_t i = (uint32_t)a[k * stride], j = (uint32_t)b[k * stride];
            pend.emplace_back(i, j); pend.emplace_back(j, i);
        }
        reset();
        return TOPO_OK;
    }
    void clear() { pend.clear(); nbr.clear(); std::fill(off.begin(), off.end(), 0); reset(); }
    void reset() { mol_valid = false; ++version; }   // reset_mol_references

    // merge the pending pairs into the CSR (sorted, duplicates dropped)
    void flush() {
        if (pend.empty()) return;
        std::vector<std::pair<uint32_t, uint32_t>> all;
        all.reserve(nbr.size() + pend.size());
        for (uint64_t a = 0; a < n; ++a)
            for (uint64_t k = off[a]; k < off[a + 1]; ++k) all.emplace_back((uint32_t)a, nbr[k]);
        all.insert(all.end(), pend.begin(), pend.end());
        pend.clear(); pend.shrink_to_fit();
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        std::fill(off.begin(), off.end(), 0);
        nbr.resize(all.size());
        for (size_t k = 0; k < all.size(); ++k) { off[all[k].first + 1]++; nbr[k] = all[k].second; }
        for (uint64_t a = 0; a < n; ++a) off[a + 1] += off[a];
    }
    bool has_bonds() { flush(); return !nbr.empty(); }
    uint64_t degree(uint64_t a) { flush(); return off[a + 1] - off[a]; }

    // get_molecule_indices: breadth-first from `start`, neighbours ascending (iterating.rs:399-432)
    void bfs(uint64_t start, std::vector<uint32_t> &out, std::vector<uint8_t> &seen) {
        flush();
        const size_t first = out.size();
        out.push_back((uint32_t)start); seen[start] = 1;
        for (size_t q = first; q < out.size(); ++q) {
            const uint32_t a = out[q];
            for (uint64_t k = off[a]; k < off[a + 1]; ++k)
                if (!seen[nbr[k]]) { seen[nbr[k]] = 1; out.push_back(nbr[k]); }
        }
    }
    int molecule_indices(uint64_t start, std::vector<uint32_t> &out) {
        out.clear();
        if (start >= n) return TOPO_OUT_OF_RANGE;
        std::vector<uint8_t> seen(n, 0);
        bfs(start, out, seen);
        return TOPO_OK;
    }

    // create_mol_references (modifying.rs:258-283) + the breadth-first order of every molecule
    void molecules() {
        if (mol_valid) return;
        flush();
        refs.clear(); mol_start.assign(1, 0); order.clear();
        rank.assign(n, 0); mol_of.assign(n, UINT32_MAX);
        std::vector<uint8_t> seen(n, 0);
        for (uint64_t a = 0; a < n; ++a) {
            if (seen[a] || off[a + 1] == off[a]) continue;
            const size_t s = order.size();
            bfs(a, order, seen);
            const uint32_t m = (uint32_t)refs.size();
            for (size_t k = s; k < order.size(); ++k) { rank[order[k]] = (uint32_t)(k - s); mol_of[order[k]] = m; }
            refs.push_back(a);
            mol_start.push_back(order.size());
        }
        mol_valid = true;
    }

    // the device map over n_pad atoms (see the header of this file)
    void map(uint64_t n_pad, std::vector<int32_t> &out, uint64_t *n_farref = nullptr) {
        molecules();
        out.assign(n_pad, GR_TOPO_NONE);
        std::vector<uint8_t> far(refs.size(), 0);
        for (uint64_t a = 0; a < n; ++a) {
            if (mol_of[a] == UINT32_MAX) continue;
            const uint64_t r = refs[mol_of[a]];
            out[a] = (int32_t)((int64_t)r - (int64_t)a);
            if ((a >> 8) != (r >> 8)) far[mol_of[a]] = 1;
        }
        uint64_t nf = 0;
        for (size_t m = 0; m < refs.size(); ++m) if (far[m]) { out[refs[m]] = GR_TOPO_FARREF; ++nf; }
        if (n_farref) *n_farref = nf;
    }
    // atom of molecule `m` at breadth-first position `k`
    uint64_t mol_atom(uint64_t m, uint64_t k) const { return order[mol_start[m] + k]; }
};

}  // namespace grt

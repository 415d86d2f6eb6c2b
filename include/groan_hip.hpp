// groan_hip.hpp -- C++17 host-side mirror of the groan_rs interface for the per-frame geometry path, on top of
// the C ABI (groan_hip.h).  Header-only and thin: same names, argument meaning and error behaviour as the
// reference's Rust API so that host code (and the tests in tests/cpp/) read like the reference's own:
//
//   reference (Rust)                                     here (C++)
//   System::new / clone per worker                       groan::System(n_atoms, device, n_slots)
//   TrajRead::update_system                              System::set_frame(xyz, box9)
//   system.group_create_from_ranges / _from_indices      same
//   Sphere / Rectangular / Cylinder / TriangularPrism    groan::Shape factories; system.group_create_from_geometry(-ies)
//   system.group_get_center / _com / estimate_* / naive  same (return Vector3D)
//   system.group_distance / atoms_distance / group_all_distances
//   system.atoms_translate / atoms_wrap / group_* / atoms_center(_mass)
//   system.calc_rmsd(&reference, group) / calc_rmsd_and_fit
//   FrameAnalyze / FrameConvert / FrameConvertAnalyze    abstract classes with the same single method
//   TrajAnalyzer / TrajConverter / TrajConverterAnalyzer for_each_frame_* adapters over any frame source
//   RMSDConverterAnalyzer                                 groan::RMSDConverterAnalyzer (cached plan)
//   XtcReader / TrrReader (+ with_range / with_step)      groan::XtcReader / TrrReader::frames(start, end, step) as frame sources
//   XtcWriter                                             groan::XtcWriter (host frames and device slots)
//   ParallelTrajData + traj_iter_map_reduce              groan::traj_iter_map_reduce (one worker thread per GPU,
//                                                         frames round-robin, shared error flag, reduce())
//   Result<T, GroupError|AtomError|RMSDError>             exceptions carrying the variant + payload
#pragma once
#include <array>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "groan_hip.h"

namespace groan {

using Vector3D = std::array<float, 3>;
using Box9 = std::array<float, 9>;   // gro order (simbox.rs:13-26)

enum class Dimension : int { None = 0, X, Y, Z, XY, XZ, YZ, XYZ };   // dimension.rs:13-23

// ---- errors (src/errors.rs): variant names as in the reference
struct Error : std::runtime_error {
    std::string kind, variant; int status; uint64_t index; uint64_t counts[2];
    Error(std::string k, std::string v, int st, uint64_t idx = 0, uint64_t c0 = 0, uint64_t c1 = 0)
        : std::runtime_error(k + "::" + v), kind(std::move(k)), variant(std::move(v)), status(st), index(idx), counts{c0, c1} {}
};

inline std::string simbox_variant(int st) { return st == GR_E_NOT_ORTHOGONAL ? "NotOrthogonal" : (st == GR_E_NO_BOX ? "DoesNotExist" : "ZeroLength"); }

// ---- AtomContainer (container.rs): bit-exact block logic lives in the library
struct AtomContainer {
    std::vector<std::pair<uint64_t, uint64_t>> blocks;
    static AtomContainer from_indices(const std::vector<uint64_t> &idx, uint64_t n_atoms) {
        std::vector<uint64_t> s(idx.size() + 1), e(idx.size() + 1);
        size_t nb = gr_container_from_indices(idx.data(), idx.size(), n_atoms, s.data(), e.data());
        return make(s, e, nb);
    }
    static AtomContainer from_ranges(const std::vector<std::pair<uint64_t, uint64_t>> &r, uint64_t n_atoms) {
        std::vector<uint64_t> a(r.size() + 1), b(r.size() + 1), s(r.size() + 1), e(r.size() + 1);
        for (size_t i = 0; i < r.size(); ++i) { a[i] = r[i].first; b[i] = r[i].second; }
        size_t nb = gr_container_from_ranges(a.data(), b.data(), r.size(), n_atoms, s.data(), e.data());
        return make(s, e, nb);
    }
    uint64_t get_n_atoms() const { auto [s, e] = split(); return gr_container_n_atoms(s.data(), e.data(), blocks.size()); }
    bool isin(uint64_t i) const { auto [s, e] = split(); return gr_container_isin(s.data(), e.data(), blocks.size(), i) != 0; }
    std::vector<uint64_t> indices() const {
        auto [s, e] = split();
        std::vector<uint64_t> out(get_n_atoms() + 1);
        out.resize(gr_container_expand(s.data(), e.data(), blocks.size(), out.data()));
        return out;
    }
    static AtomContainer set_union(const AtomContainer &x, const AtomContainer &y) {
        auto [s1, e1] = x.split(); auto [s2, e2] = y.split();
        std::vector<uint64_t> s(x.blocks.size() + y.blocks.size() + 1), e(s.size());
        size_t nb = gr_container_union(s1.data(), e1.data(), x.blocks.size(), s2.data(), e2.data(), y.blocks.size(), s.data(), e.data());
        return make(s, e, nb);
    }
  private:
    static AtomContainer make(const std::vector<uint64_t> &s, const std::vector<uint64_t> &e, size_t nb) {
        AtomContainer c; for (size_t i = 0; i < nb; ++i) c.blocks.emplace_back(s[i], e[i]); return c;
    }
    std::pair<std::vector<uint64_t>, std::vector<uint64_t>> split() const {
        std::vector<uint64_t> s(blocks.size() + 1), e(blocks.size() + 1);
        for (size_t i = 0; i < blocks.size(); ++i) { s[i] = blocks[i].first; e[i] = blocks[i].second; }
        return {s, e};
    }
};

// ---- System (src/system/mod.rs:38-73)
// Shape (src/structures/shape.rs): a value type over gr_shape; the factories throw where the reference panics.
struct Shape {
    gr_shape c{};
    static Shape sphere(const Vector3D &pos, float radius) { Shape s; check(gr_shape_sphere(&s.c, pos.data(), radius), "Sphere::new"); return s; }
    static Shape rectangular(const Vector3D &pos, float x, float y, float z) { Shape s; check(gr_shape_rectangular(&s.c, pos.data(), x, y, z), "Rectangular::new"); return s; }
    static Shape cylinder(const Vector3D &pos, float radius, float height, Dimension orientation) {
        Shape s; check(gr_shape_cylinder(&s.c, pos.data(), radius, height, (int)orientation), "Cylinder::new | Unsupported orientation dimension"); return s;
    }
    static Shape triangular_prism(const Vector3D &b1, const Vector3D &b2, const Vector3D &b3, float height) {
        Shape s; check(gr_shape_triangular_prism(&s.c, b1.data(), b2.data(), b3.data(), height), "TriangularPrism::new | invalid base"); return s;
    }
    bool inside(const Vector3D &point, const Box9 &box) const { int in = 0; check(gr_shape_inside(&c, point.data(), box.data(), 0, &in), "Shape::inside"); return in != 0; }
    bool inside_naive(const Vector3D &point) const { int in = 0; check(gr_shape_inside(&c, point.data(), nullptr, 1, &in), "NaiveShape::inside_naive"); return in != 0; }
private:
    static void check(int st, const char *what) { if (st != GR_OK) throw std::invalid_argument(std::string("FATAL GROAN ERROR | ") + what); }
};

class System {
  public:
    System(uint64_t n_atoms, int device = 0, uint32_t n_slots = 1) : n_(n_atoms), device_(device) {
        int st = 0;
        ctx_ = gr_ctx_create(device, n_atoms, n_slots, &st);
        if (!ctx_) throw Error("DeviceError", gr_status_string(st), st);
    }
    ~System() { if (ctx_) gr_ctx_destroy(ctx_); }
    System(const System &) = delete;
    System &operator=(const System &) = delete;
    System(System &&o) noexcept : ctx_(o.ctx_), n_(o.n_), device_(o.device_) { o.ctx_ = nullptr; }

    gr_ctx *raw() const { return ctx_; }
    // System::atoms_iter / group_iter (src/system/iterating.rs:43,108); defined below AtomIterator
    class AtomIterator atoms_iter(uint32_t slot = 0);
    class AtomIterator group_iter(const std::string &name, uint32_t slot = 0);
    friend class AtomIterator;
    uint64_t get_n_atoms() const { return n_; }
    int device() const { return device_; }
    void set_masses(const std::vector<float> &m) { check_plain(gr_set_masses(ctx_, m.data(), m.size())); }
    void set_strict_orthogonal(bool on) { gr_ctx_set_strict_orthogonal(ctx_, on ? 1 : 0); }

    // TrajRead::update_system (traj_read.rs:160-186): rvec[n] + box as the xtc readers deliver them
    void set_frame(const float *xyz, const Box9 *box, uint32_t slot = 0) {
        check_plain(gr_frame_upload(ctx_, slot, xyz, box ? box->data() : nullptr));
        check_plain(gr_sync(ctx_));
    }
    std::vector<float> get_positions(uint32_t slot = 0) const {
        std::vector<float> out(3 * n_);
        check_plain(gr_frame_download(ctx_, slot, out.data()));
        return out;
    }
    void set_box(const Box9 *box, uint32_t slot = 0) { check_plain(gr_frame_set_box(ctx_, slot, box ? box->data() : nullptr)); }

    bool group_create_from_ranges(const std::string &name, const std::vector<std::pair<uint64_t, uint64_t>> &r) {
        std::vector<uint64_t> s(r.size() + 1), e(r.size() + 1);
        for (size_t i = 0; i < r.size(); ++i) { s[i] = r[i].first; e[i] = r[i].second; }
        int st = gr_group_create_from_ranges(ctx_, name.c_str(), s.data(), e.data(), r.size());
        if (st != GR_OK && st != GR_E_GROUP_EXISTS) group_error(st, name);
        return st == GR_E_GROUP_EXISTS;   // AlreadyExistsWarning
    }
    bool group_create_from_indices(const std::string &name, const std::vector<uint64_t> &idx) {
        int st = gr_group_create_from_indices(ctx_, name.c_str(), idx.data(), idx.size());
        if (st != GR_OK && st != GR_E_GROUP_EXISTS) group_error(st, name);
        return st == GR_E_GROUP_EXISTS;
    }
    // System::group_create_from_geometry / _geometries (groups.rs:94-188) with a source group in place of the query
    bool group_create_from_geometries(const std::string &name, const std::string &source, const std::vector<Shape> &shapes, uint32_t slot = 0, bool naive = false) {
        std::vector<gr_shape> raw;
        for (const Shape &s : shapes) raw.push_back(s.c);
        int st = gr_group_create_from_geometries(ctx_, slot, name.c_str(), source.c_str(), raw.data(), raw.size(), naive ? 1 : 0);
        if (st == GR_E_GROUP_NOT_FOUND) throw Error("GroupError", "InvalidQuery", st);
        if (st == GR_E_INVALID_NAME) throw Error("GroupError", "InvalidName", st);
        if (st != GR_OK && st != GR_E_GROUP_EXISTS) group_error(st, name);
        return st == GR_E_GROUP_EXISTS;
    }
    bool group_create_from_geometry(const std::string &name, const std::string &source, const Shape &shape, uint32_t slot = 0) {
        return group_create_from_geometries(name, source, { shape }, slot);
    }
    uint64_t group_get_n_atoms(const std::string &name) const {
        uint64_t n = 0;
        if (gr_group_n_atoms(ctx_, name.c_str(), &n) != GR_OK) throw Error("GroupError", "NotFound", GR_E_GROUP_NOT_FOUND);
        return n;
    }

    // analysis.rs:52-320
    Vector3D group_get_center_naive(const std::string &g, uint32_t slot = 0) const { return center(g, GR_CENTER_NAIVE, 0, slot); }
    Vector3D group_estimate_center(const std::string &g, uint32_t slot = 0) const { return center(g, GR_CENTER_ESTIMATE, 0, slot); }
    Vector3D group_get_center(const std::string &g, uint32_t slot = 0) const { return center(g, GR_CENTER_PBC, 0, slot); }
    Vector3D group_get_com_naive(const std::string &g, uint32_t slot = 0) const { return center(g, GR_CENTER_NAIVE, 1, slot); }
    Vector3D group_estimate_com(const std::string &g, uint32_t slot = 0) const { return center(g, GR_CENTER_ESTIMATE, 1, slot); }
    Vector3D group_get_com(const std::string &g, uint32_t slot = 0) const { return center(g, GR_CENTER_PBC, 1, slot); }

    // analysis.rs:348-471
    float group_distance(const std::string &g1, const std::string &g2, Dimension dim, uint32_t slot = 0) const {
        float out = 0;
        int st = gr_group_distance(ctx_, slot, g1.c_str(), g2.c_str(), (int)dim, &out);
        if (st) group_error(st, g1);
        return out;
    }
    float atoms_distance(uint64_t i, uint64_t j, Dimension dim, uint32_t slot = 0) const {
        float out = 0;
        int st = gr_atoms_distance(ctx_, slot, i, j, (int)dim, &out);
        if (st) atom_error(st);
        return out;
    }
    // row-major n1 x n2 (ndarray::Array2<f32>)
    std::vector<float> group_all_distances(const std::string &g1, const std::string &g2, Dimension dim, uint32_t slot = 0) const {
        std::vector<float> out((size_t)group_get_n_atoms(g1) * group_get_n_atoms(g2));
        int st = gr_group_all_distances(ctx_, slot, g1.c_str(), g2.c_str(), (int)dim, out.data(), out.size());
        if (st) group_error(st, g1);
        return out;
    }

    // modifying.rs:45-75,201-222 ; utility.rs:109-185
    void atoms_translate(const Vector3D &v, uint32_t slot = 0) { int st = gr_group_translate(ctx_, slot, nullptr, v.data()); if (st) atom_error(st); }
    void group_translate(const std::string &g, const Vector3D &v, uint32_t slot = 0) { int st = gr_group_translate(ctx_, slot, g.c_str(), v.data()); if (st) group_error(st, g); }
    void atoms_wrap(uint32_t slot = 0) { int st = gr_group_wrap(ctx_, slot, nullptr); if (st) atom_error(st); }
    void group_wrap(const std::string &g, uint32_t slot = 0) { int st = gr_group_wrap(ctx_, slot, g.c_str()); if (st) group_error(st, g); }
    void atoms_center(const std::string &g, Dimension dim, uint32_t slot = 0) { int st = gr_atoms_center(ctx_, slot, g.c_str(), (int)dim, 0); if (st) group_error(st, g); }
    void atoms_center_mass(const std::string &g, Dimension dim, uint32_t slot = 0) { int st = gr_atoms_center(ctx_, slot, g.c_str(), (int)dim, 1); if (st) group_error(st, g); }

    // bond topology and whole molecules: modifying.rs:235-487, iterating.rs:238-245,399-432 (a failed frame is left untouched)
    void add_bond(uint64_t i, uint64_t j) { int st = gr_add_bond(ctx_, i, j); if (st) bond_error(st); }
    void add_bonds(const std::vector<std::pair<uint64_t, uint64_t>> &pairs) {
        std::vector<uint64_t> flat;
        flat.reserve(2 * pairs.size());
        for (const auto &p : pairs) { flat.push_back(p.first); flat.push_back(p.second); }
        int st = gr_add_bonds(ctx_, flat.data(), pairs.size());
        if (st) bond_error(st);
    }
    void clear_bonds() { check_plain(gr_clear_bonds(ctx_)); }
    bool has_bonds() const { return gr_has_bonds(ctx_) != 0; }
    std::vector<uint64_t> get_mol_references() {
        uint64_t n = 0;
        check_plain(gr_mol_references(ctx_, nullptr, 0, &n));
        std::vector<uint64_t> out(n);
        check_plain(gr_mol_references(ctx_, out.data(), n, &n));
        return out;
    }
    std::vector<uint64_t> molecule_indices(uint64_t index) {
        uint64_t n = 0;
        int st = gr_molecule_atoms(ctx_, index, nullptr, 0, &n);
        if (st) atom_error(st);
        std::vector<uint64_t> out(n);
        st = gr_molecule_atoms(ctx_, index, out.data(), n, &n);
        if (st) atom_error(st);
        return out;
    }
    void make_molecules_whole(uint32_t slot = 0) { int st = gr_make_molecules_whole(ctx_, slot); if (st) atom_error(st); }
    // per-frame statuses in *status (may be NULL); throws for the first failed frame unless status is given
    void make_molecules_whole_batch(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        if (status) status->assign(n_frames, GR_OK);
        int st = gr_make_molecules_whole_batch(ctx_, first_slot, n_frames, status ? status->data() : nullptr);
        if (st && !status) atom_error(st);
    }
    void make_group_whole(const std::string &g, uint32_t slot = 0) { int st = gr_make_group_whole(ctx_, slot, g.c_str()); if (st) group_error(st, g); }
    void make_group_whole_batch(const std::string &g, uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        if (status) status->assign(n_frames, GR_OK);
        int st = gr_make_group_whole_batch(ctx_, first_slot, n_frames, g.c_str(), status ? status->data() : nullptr);
        if (st && !status) group_error(st, g);
    }

    // rmsd.rs:75-166
    float calc_rmsd(const System &reference, const std::string &group, uint32_t slot = 0, uint32_t ref_slot = 0) const {
        float r = 0;
        int st = gr_calc_rmsd(ctx_, slot, reference.ctx_, ref_slot, group.c_str(), &r, nullptr);
        if (st) rmsd_error(st, group);
        return r;
    }
    float calc_rmsd_and_fit(const System &reference, const std::string &group, uint32_t slot = 0, uint32_t ref_slot = 0) {
        float r = 0;
        int st = gr_calc_rmsd_and_fit(ctx_, slot, reference.ctx_, ref_slot, group.c_str(), &r);
        if (st) rmsd_error(st, group);
        return r;
    }

    [[noreturn]] void rmsd_error(int st, const std::string &group) const {
        uint64_t idx = gr_last_error_index(ctx_);
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("RMSDError", "NonexistentGroup", st);
        case GR_E_EMPTY_GROUP: throw Error("RMSDError", "EmptyGroup", st);
        case GR_E_NO_POSITION: throw Error("RMSDError", "InvalidPosition", st, idx);
        case GR_E_NO_MASS: throw Error("RMSDError", "InvalidMass", st, idx);
        case GR_E_INCONSISTENT_GROUP: { uint64_t c[2]; gr_last_error_counts(ctx_, c); throw Error("RMSDError", "InconsistentGroup", st, 0, c[0], c[1]); }
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("RMSDError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_) + " [" + group + "]", st);
        }
    }

  private:
    Vector3D center(const std::string &g, int kind, int weighted, uint32_t slot) const {
        Vector3D out{};
        int st = gr_group_center(ctx_, slot, g.c_str(), kind, weighted, out.data());
        if (st) group_error(st, g);
        return out;
    }
    void check_plain(int st) const { if (st) throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st); }
    [[noreturn]] void group_error(int st, const std::string &g) const {
        uint64_t idx = gr_last_error_index(ctx_);
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_EMPTY_GROUP: throw Error("GroupError", "EmptyGroup", st);
        case GR_E_NO_POSITION: throw Error("GroupError", "InvalidPosition", st, idx);
        case GR_E_NO_MASS: throw Error("GroupError", "InvalidMass", st, idx);
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("GroupError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_) + " [" + g + "]", st);
        }
    }
    [[noreturn]] void bond_error(int st) const {
        if (st == GR_E_INVALID_BOND) { uint64_t c[2]; gr_last_error_counts(ctx_, c); throw Error("AtomError", "InvalidBond", st, 0, c[0], c[1]); }
        atom_error(st);
    }
    [[noreturn]] void atom_error(int st) const {
        uint64_t idx = gr_last_error_index(ctx_);
        switch (st) {
        case GR_E_OUT_OF_RANGE: throw Error("AtomError", "OutOfRange", st, idx);
        case GR_E_NO_POSITION: throw Error("AtomError", "InvalidPosition", st, idx);
        case GR_E_NO_MASS: throw Error("AtomError", "InvalidMass", st, idx);
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("AtomError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    uint64_t n_;
    int device_;
};

// ---- atom iterators (src/structures/iterators.rs:28-46,350-402,1053-1604; src/system/iterating.rs:43-140)
// An AtomContainer + the System (and slot) it walks.  Each method is one gr_sel_* call: the kernels take the container's
// blocks directly.  Error behaviour is the iterator traits': box first, then the first atom without position / mass; an EMPTY
// iterator is not an error -- its centre is (NaN, NaN, NaN) (iterators.rs:1186-1188).
class AtomIterator {
  public:
    AtomIterator(System &system, AtomContainer container, uint32_t slot = 0) : sys_(&system), c_(std::move(container)), slot_(slot) {}
    const AtomContainer &container() const { return c_; }
    uint64_t get_n_atoms() const { return c_.get_n_atoms(); }
    Vector3D get_center_naive() const { return center(GR_CENTER_NAIVE, 0); }
    Vector3D get_com_naive() const { return center(GR_CENTER_NAIVE, 1); }
    Vector3D estimate_center() const { return center(GR_CENTER_ESTIMATE, 0); }
    Vector3D get_center() const { return center(GR_CENTER_PBC, 0); }
    Vector3D estimate_com() const { return center(GR_CENTER_ESTIMATE, 1); }
    Vector3D get_com() const { return center(GR_CENTER_PBC, 1); }
    AtomIterator filter_geometry(const Shape &shape) const { return filter(shape, false); }          // :1094-1105
    AtomIterator filter_geometry_naive(const Shape &shape) const { return filter(shape, true); }     // :994-1004
    void translate(const Vector3D &v) { auto se = split(); int st = gr_sel_translate(sys_->raw(), slot_, se.first.data(), se.second.data(), c_.blocks.size(), v.data()); if (st) sys_->atom_error(st); }
    void wrap() { auto se = split(); int st = gr_sel_wrap(sys_->raw(), slot_, se.first.data(), se.second.data(), c_.blocks.size()); if (st) sys_->atom_error(st); }
    AtomIterator set_union(const AtomIterator &o) const { return AtomIterator(*sys_, AtomContainer::set_union(c_, o.c_), slot_); }   // OrderedAtomIterator::union :1572
    std::vector<float> all_distances(const AtomIterator &o, Dimension dim) const {
        auto a = split(); auto b = o.split();
        std::vector<float> out((size_t)get_n_atoms() * o.get_n_atoms());
        int st = gr_sel_all_distances(sys_->raw(), slot_, a.first.data(), a.second.data(), c_.blocks.size(), b.first.data(), b.second.data(), o.c_.blocks.size(), (int)dim, out.data(), out.size());
        if (st) sys_->atom_error(st);
        return out;
    }
  private:
    std::pair<std::vector<uint64_t>, std::vector<uint64_t>> split() const {
        std::vector<uint64_t> s(c_.blocks.size() + 1), e(c_.blocks.size() + 1);
        for (size_t i = 0; i < c_.blocks.size(); ++i) { s[i] = c_.blocks[i].first; e[i] = c_.blocks[i].second; }
        return {s, e};
    }
    Vector3D center(int kind, int weighted) const {
        auto se = split(); Vector3D out{};
        int st = gr_sel_center(sys_->raw(), slot_, se.first.data(), se.second.data(), c_.blocks.size(), kind, weighted, out.data());
        if (st) sys_->atom_error(st);
        return out;
    }
    AtomIterator filter(const Shape &shape, bool naive) const {
        auto se = split();
        const size_t cap = (size_t)get_n_atoms() + 1;
        std::vector<uint64_t> os(cap), oe(cap); size_t nb = 0; uint64_t na = 0;
        int st = gr_sel_filter_geometry(sys_->raw(), slot_, se.first.data(), se.second.data(), c_.blocks.size(), &shape.c, 1, naive ? 1 : 0, os.data(), oe.data(), cap, &nb, &na);
        if (st) sys_->atom_error(st);
        AtomContainer out; for (size_t i = 0; i < nb; ++i) out.blocks.emplace_back(os[i], oe[i]);
        return AtomIterator(*sys_, out, slot_);
    }
    System *sys_; AtomContainer c_; uint32_t slot_;
};
inline AtomIterator System::atoms_iter(uint32_t slot) { AtomContainer c; c.blocks.emplace_back(0, n_ - 1); return AtomIterator(*this, c, slot); }
inline AtomIterator System::group_iter(const std::string &name, uint32_t slot) {
    size_t nb = 0;
    if (gr_group_n_blocks(ctx_, name.c_str(), &nb) != GR_OK) throw Error("GroupError", "NotFound", GR_E_GROUP_NOT_FOUND);
    std::vector<uint64_t> s(nb + 1), e(nb + 1);
    gr_group_blocks(ctx_, name.c_str(), s.data(), e.data());
    AtomContainer c; for (size_t i = 0; i < nb; ++i) c.blocks.emplace_back(s[i], e[i]);
    return AtomIterator(*this, c, slot);
}

// ---- plug-in traits (src/structures/traj_convert.rs:30-36,76-83,125-132)
template <typename R> struct FrameAnalyze { virtual ~FrameAnalyze() = default; virtual R analyze(const System &system) = 0; };
struct FrameConvert { virtual ~FrameConvert() = default; virtual void convert(System &system) = 0; };
template <typename R> struct FrameConvertAnalyze { virtual ~FrameConvertAnalyze() = default; virtual R convert_analyze(System &system) = 0; };

// ---- RMSDConverterAnalyzer (src/system/rmsd.rs:170-251)
class RMSDConverterAnalyzer : public FrameAnalyze<float>, public FrameConvertAnalyze<float> {
  public:
    RMSDConverterAnalyzer(const System &reference, System &target, const std::string &group, uint32_t ref_slot = 0)
        : target_(target), group_(group) {
        int st = 0;
        plan_ = gr_rmsd_plan_create(reference.raw(), ref_slot, target.raw(), group.c_str(), &st);
        if (!plan_) reference.rmsd_error(st, group);
    }
    ~RMSDConverterAnalyzer() override { if (plan_) gr_rmsd_plan_destroy(plan_); }
    float analyze(const System &) override { return batch(0, 1, false)[0]; }
    float convert_analyze(System &) override { return batch(0, 1, true)[0]; }
    // many resident frames per call: the shape the GPU wants
    std::vector<float> batch(uint32_t first_slot, uint32_t n, bool fit) {
        std::vector<float> r(n);
        std::vector<int> st(n);
        int s = fit ? gr_rmsd_fit_batch(plan_, first_slot, n, r.data(), st.data()) : gr_rmsd_batch(plan_, first_slot, n, r.data(), st.data(), nullptr);
        if (s) target_.rmsd_error(s, group_);
        return r;
    }
    uint32_t last_fallbacks() const { return gr_rmsd_plan_last_fallbacks(plan_); }
  private:
    gr_rmsd_plan *plan_ = nullptr;
    System &target_;
    std::string group_;
};

// ---- a decoded frame as the xtc readers hand it to update_system
struct Frame { const float *xyz; const Box9 *box; uint64_t step; float time; };

// TrajAnalyzer::next (traj_convert.rs:95-105): update the system with each frame, run the analyzer
template <typename R, typename Source, typename Sink>
void for_each_frame_analyze(System &system, Source &&next_frame, FrameAnalyze<R> &analyzer, Sink &&sink) {
    Frame f;
    while (next_frame(f)) { system.set_frame(f.xyz, f.box); sink(f, analyzer.analyze(system)); }
}
template <typename R, typename Source, typename Sink>
void for_each_frame_convert_analyze(System &system, Source &&next_frame, FrameConvertAnalyze<R> &ca, Sink &&sink) {
    Frame f;
    while (next_frame(f)) { system.set_frame(f.xyz, f.box); sink(f, ca.convert_analyze(system)); }
}

// ---- XtcReader / TrrReader as frame sources (src/io/xtc_io/mod.rs, src/io/trr_io.rs; `with_range` / `with_step` of
// traj_read.rs:609-697 are the `start, end, step` of frames()), XtcWriter (xtc_io/mod.rs:256-331)
class XtcReader {
  public:
    explicit XtcReader(const std::string &path) {
        int st = 0;
        x_ = gr_xtc_open(path.c_str(), &st);
        if (!x_) throw Error("ReadTrajError", st == GR_E_IO ? "FileNotFound" : "NotXtc", st);
        xyz_.resize(3 * (size_t)n_atoms());
    }
    ~XtcReader() { if (x_) gr_xtc_close(x_); }
    XtcReader(const XtcReader &) = delete;
    XtcReader &operator=(const XtcReader &) = delete;
    uint64_t n_atoms() const { return gr_xtc_n_atoms(x_); }
    uint64_t n_frames() const { return gr_xtc_n_frames(x_); }
    const gr_xtc *raw() const { return x_; }
    // frame i decoded into this reader's buffer (valid until the next read)
    Frame read(uint64_t i) {
        float b[9]; uint64_t step = 0; float time = 0, prec = 0;
        const int st = gr_xtc_read_frame(x_, i, xyz_.data(), b, &step, &time, &prec);
        if (st != GR_OK) throw Error("ReadTrajError", "FrameNotFound", st, i);
        for (int k = 0; k < 9; ++k) box_[k] = b[k];
        return Frame{xyz_.data(), &box_, step, time};
    }
    // a Source for for_each_frame_*: frames start, start + step, ... < end
    std::function<bool(Frame &)> frames(uint64_t start = 0, uint64_t end = UINT64_MAX, uint64_t step = 1) {
        auto next = std::make_shared<uint64_t>(start);
        return [this, next, end, step](Frame &out) {
            if (*next >= std::min<uint64_t>(end, n_frames())) return false;
            out = read(*next); *next += step;
            return true;
        };
    }
    // a batch of frames unpacked on the GPU straight into the system's slots (compressed bytes over PCIe)
    void read_frames_device(System &system, uint64_t first_frame, uint32_t n, uint32_t first_slot = 0, uint64_t frame_step = 1, int host_threads = 0) {
        const int st = gr_xtc_read_frames_device(x_, first_frame, n, frame_step, system.raw(), first_slot, host_threads, nullptr, nullptr);
        if (st != GR_OK) throw Error("ReadTrajError", "FrameNotFound", st, first_frame);
    }
  private:
    gr_xtc *x_ = nullptr;
    std::vector<float> xyz_;
    Box9 box_{};
};

class TrrReader {
  public:
    explicit TrrReader(const std::string &path) {
        int st = 0;
        t_ = gr_trr_open(path.c_str(), &st);
        if (!t_) throw Error("ReadTrajError", st == GR_E_IO ? "FileNotFound" : "NotTrr", st);
        xyz_.resize(3 * (size_t)n_atoms());
    }
    ~TrrReader() { if (t_) gr_trr_close(t_); }
    TrrReader(const TrrReader &) = delete;
    TrrReader &operator=(const TrrReader &) = delete;
    uint64_t n_atoms() const { return gr_trr_n_atoms(t_); }
    uint64_t n_frames() const { return gr_trr_n_frames(t_); }
    // positions of frame i (an all-zero position = the reference's "no position": NaN in x, trr_io.rs:108-112)
    Frame read(uint64_t i) {
        float b[9]; uint64_t step = 0; float time = 0, lambda = 0;
        const int st = gr_trr_read_frame(t_, i, xyz_.data(), nullptr, nullptr, b, &step, &time, &lambda);
        if (st != GR_OK) throw Error("ReadTrajError", "FrameNotFound", st, i);
        for (size_t a = 0; a < xyz_.size(); a += 3) if (xyz_[a] == 0.0f && xyz_[a + 1] == 0.0f && xyz_[a + 2] == 0.0f) xyz_[a] = NAN;
        for (int k = 0; k < 9; ++k) box_[k] = b[k];
        return Frame{xyz_.data(), &box_, step, time};
    }
    std::function<bool(Frame &)> frames(uint64_t start = 0, uint64_t end = UINT64_MAX, uint64_t step = 1) {
        auto next = std::make_shared<uint64_t>(start);
        return [this, next, end, step](Frame &out) {
            if (*next >= std::min<uint64_t>(end, n_frames())) return false;
            out = read(*next); *next += step;
            return true;
        };
    }
  private:
    gr_trr *t_ = nullptr;
    std::vector<float> xyz_;
    Box9 box_{};
};

class XtcWriter {
  public:
    explicit XtcWriter(const std::string &path) {
        int st = 0;
        w_ = gr_xtc_writer_open(path.c_str(), &st);
        if (!w_) throw Error("WriteTrajError", "CouldNotCreate", st);
    }
    ~XtcWriter() { if (w_) gr_xtc_writer_close(w_); }
    XtcWriter(const XtcWriter &) = delete;
    XtcWriter &operator=(const XtcWriter &) = delete;
    void write_frame(const float *xyz, uint64_t n_atoms, const Box9 *box, int64_t step, float time, float precision = 1000.0f) {
        const int st = gr_xtc_write_frame(w_, n_atoms, xyz, box ? box->data() : nullptr, step, time, precision);
        if (st != GR_OK) throw Error("WriteTrajError", "CouldNotWrite", st);
    }
    // device frames (e.g. after calc_rmsd_and_fit on a batch of slots), all atoms or a group
    void write_slots(System &system, uint32_t first_slot, uint32_t n_frames, const char *group = nullptr, float precision = 1000.0f, int host_threads = 0) {
        const int st = gr_xtc_write_slots(w_, system.raw(), first_slot, n_frames, group, nullptr, nullptr, precision, host_threads);
        if (st == GR_E_GROUP_NOT_FOUND) throw Error("WriteTrajError", "GroupNotFound", st);
        if (st != GR_OK) throw Error("WriteTrajError", "CouldNotWrite", st);
    }
  private:
    gr_xtc_writer *w_ = nullptr;
};

// ---- ParallelTrajData + traj_iter_map_reduce (src/system/parallel.rs:31-49,208-481)
// One worker thread per device; worker n takes frames n, n+T, ... (parallel.rs:424-448); a shared AtomicBool
// polled every ERROR_FLAG_FREQ = 10 frames stops the others after the first failure (parallel.rs:28,453-475).
// start_frame / end_frame / step = the reference's start_time / end_time / step in frame-index form (a reader's index turns times
// into frame numbers): the frames visited are start_frame + k * step below end_frame, worker n skips n * step of them and then
// advances by step * T (parallel.rs:425-448).  progress = the ProgressPrinter: called from worker 0 after every frame it completes
// (ProgressStatus::Running; the reference attaches the printer to the master thread only, :417-422) and once at the end with
// Completed and the last frame ANY worker read, or Failed and the frame that failed (:288-321).
enum class ProgressStatus { Running, Completed, Failed };
using ProgressPrinter = std::function<void(ProgressStatus, uint64_t frame)>;
template <typename Data>
Data traj_iter_map_reduce(const std::vector<int> &devices, uint64_t n_frames,
                          const std::function<System(int device)> &make_system,                       // System clone per worker
                          const std::function<bool(uint64_t frame_index, Frame &out)> &read_frame,    // random access frame source
                          const std::function<void(System &, Data &)> &body, const Data &init_data,
                          uint64_t start_frame = 0, uint64_t end_frame = UINT64_MAX, uint64_t step = 1,
                          const ProgressPrinter &progress = nullptr) {
    const size_t T = devices.size();
    if (T == 0) throw std::invalid_argument("Number of threads to spawn must be > 0.");
    if (step == 0) throw std::invalid_argument("ReadTrajError::InvalidStep");
    const uint64_t end = std::min(end_frame, n_frames);
    std::vector<Data> data(T, init_data);
    std::vector<std::string> errors(T);
    std::vector<uint64_t> last_frame(T, start_frame), failed_at(T, 0);
    std::atomic<bool> error_flag{false};
    std::vector<std::thread> workers;
    for (size_t n = 0; n < T; ++n) {
        data[n].initialize(n);
        workers.emplace_back([&, n] {
            uint64_t f = start_frame + n * step;
            try {
                System system = make_system(devices[n]);
                for (uint64_t i = 0; f < end; f += step * T, ++i) {
                    if (i % 10 == 0 && error_flag.load(std::memory_order_relaxed)) return;
                    Frame fr;
                    if (!read_frame(f, fr)) return;
                    system.set_frame(fr.xyz, fr.box);
                    body(system, data[n]);
                    last_frame[n] = f;
                    if (n == 0 && progress) progress(ProgressStatus::Running, f);
                }
            } catch (const std::exception &e) {
                error_flag.store(true, std::memory_order_relaxed);
                errors[n] = e.what(); failed_at[n] = f;
            }
        });
    }
    for (auto &w : workers) w.join();
    for (size_t n = 0; n < T; ++n)
        if (!errors[n].empty()) { if (progress) progress(ProgressStatus::Failed, failed_at[n]); throw std::runtime_error(errors[n]); }
    if (progress) progress(ProgressStatus::Completed, *std::max_element(last_frame.begin(), last_frame.end()));
    return Data::reduce(std::move(data));
}

// ---- the `status` argument of every batch method below (HBondPlan::batch .. Covariance::accumulate), one rule for all of them:
// a frame that fails is reported in `status` when it is given (one entry per frame) and thrown -- the first failure -- when it is not.
// A call that was REFUSED AS A WHOLE always throws, `status` given or not: it returned an error while every entry of the status
// vector it filled is GR_OK, so no frame ran (a slot range outside the system, an unknown or empty group, a refused argument,
// a HIP error).  `status` is not touched by a call that throws.
namespace detail {
template <typename Raise>
inline void batch_status(int r, const std::vector<int> &st, std::vector<int> *status, Raise &&raise) {
    if (r != GR_OK && std::all_of(st.begin(), st.end(), [](int s) { return s == GR_OK; })) raise(r);
    if (status) *status = st;
    else if (r != GR_OK) raise(r);
}
}  // namespace detail

// ---- hydrogen bonds over a batch of resident frames (src/system/hbonds.rs): HBondAnalysis as a plan built once
struct HBondChain { std::string acceptors, donors, hydrogens; };   // group names of the System (HBondChain::new)
struct HBond { uint32_t donor, hydrogen, acceptor; float distance, angle; };

class HBondPlan {
  public:
    // bonds: the System's bonds as atom pairs (either order); errors carry the reference's HBondError variant names
    HBondPlan(System &system, const std::vector<HBondChain> &chains, const std::vector<std::pair<uint32_t, uint32_t>> &pairs,
              const std::vector<std::pair<uint64_t, uint64_t>> &bonds, float max_distance, float min_angle)
        : ctx_(system.raw()), pairs_(pairs) {
        std::vector<const char *> names;
        for (const auto &c : chains) { names.push_back(c.acceptors.c_str()); names.push_back(c.donors.c_str()); names.push_back(c.hydrogens.c_str()); }
        std::vector<uint32_t> pr; for (const auto &p : pairs) { pr.push_back(p.first); pr.push_back(p.second); }
        std::vector<uint64_t> bd; for (const auto &b : bonds) { bd.push_back(b.first); bd.push_back(b.second); }
        int st = 0;
        plan_ = gr_hbond_plan_create(ctx_, names.data(), (uint32_t)chains.size(), pr.data(), (uint32_t)pairs.size(), bd.data(), bonds.size(), max_distance, min_angle, &st);
        if (!plan_) raise(st, true);
    }
    ~HBondPlan() { if (plan_) gr_hbond_plan_destroy(plan_); }
    HBondPlan(const HBondPlan &) = delete;
    HBondPlan &operator=(const HBondPlan &) = delete;
    HBondPlan(HBondPlan &&o) noexcept : ctx_(o.ctx_), plan_(o.plan_), pairs_(std::move(o.pairs_)), cap_(o.cap_) { o.plan_ = nullptr; }

    // the bonds of n_frames resident slots: result[f][p] = bonds of frame f and pair p (HBondMap in pair order); a frame that
    // failed throws the first failure unless `status` is given, which then receives every frame's status
    std::vector<std::vector<std::vector<HBond>>> batch(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        const size_t np = pairs_.size();
        std::vector<uint64_t> offs((size_t)n_frames * np + 1);
        std::vector<int> st(n_frames);
        uint64_t total = 0;
        std::vector<uint32_t> d, h, a; std::vector<float> dist, ang;
        int r = GR_OK;
        for (int pass = 0; pass < 2; ++pass) {
            d.resize(cap_ + 1); h.resize(cap_ + 1); a.resize(cap_ + 1); dist.resize(cap_ + 1); ang.resize(cap_ + 1);
            r = gr_hbond_batch(plan_, first_slot, n_frames, cap_, d.data(), h.data(), a.data(), dist.data(), ang.data(), offs.data(), &total, st.data());
            if (total <= cap_) break;
            cap_ = total + total / 4;                                    // capacity hint: one call per batch in steady state
        }
        detail::batch_status(r, st, status, [this](int e) { raise(e, false); });
        std::vector<std::vector<std::vector<HBond>>> out(n_frames, std::vector<std::vector<HBond>>(np));
        for (uint32_t f = 0; f < n_frames; ++f)
            for (size_t p = 0; p < np; ++p)
                for (uint64_t k = offs[f * np + p]; k < offs[f * np + p + 1]; ++k) out[f][p].push_back(HBond{ d[k], h[k], a[k], dist[k], ang[k] });
        return out;
    }
    const std::vector<std::pair<uint32_t, uint32_t>> &pairs() const { return pairs_; }
    gr_hbond_plan *raw() const { return plan_; }

  private:
    [[noreturn]] void raise(int st, bool plan) const {
        const uint64_t idx = gr_last_error_index(ctx_);
        switch (st) {
        case GR_E_EMPTY_CHAIN: throw Error("HBondError", "EmptyChain", st, idx);
        case GR_E_NONEXISTENT_CHAIN: throw Error("HBondError", "NonexistentChain", st, idx);
        case GR_E_DUPLICATE_PAIR: throw Error("HBondError", "PairSpecifiedMultipleTimes", st, idx);   // index = the repeated pair's ordinal
        case GR_E_UNUSED_CHAIN: throw Error("HBondError", "UnusedChain", st);
        case GR_E_GROUP_NOT_FOUND: throw Error("HBondError", "SelectError", st);
        case GR_E_NO_POSITION: throw Error("HBondError", "AtomError(InvalidPosition)", st, idx);
        case GR_E_OUT_OF_RANGE: throw Error("HBondError", "AtomError(OutOfRange)", st, idx);
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("HBondError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default:
            if (plan && st == GR_E_INVALID_ARG) throw Error("HBondError", "CellGridError(InvalidCellSize)", st);
            throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_hbond_plan *plan_ = nullptr;
    std::vector<std::pair<uint32_t, uint32_t>> pairs_;
    uint64_t cap_ = 0;
};

// ---- GridMap (src/structures/gridmap.rs): an xy tile map accumulated over batches of resident frames
enum class GridValue : int { Count = GR_GM_COUNT, X = GR_GM_X, Y = GR_GM_Y, Z = GR_GM_Z };

class GridMap {
  public:
    GridMap(System &system, std::pair<float, float> span_x, std::pair<float, float> span_y, std::pair<float, float> tile_dim) : ctx_(system.raw()) {
        const float sx[2] = { span_x.first, span_x.second }, sy[2] = { span_y.first, span_y.second }, td[2] = { tile_dim.first, tile_dim.second };
        int st = 0;
        map_ = gr_gridmap_create(ctx_, sx, sy, td, &st);
        if (!map_) raise(st);
        dims();
    }
    // GridMap::from_box: spans (0, box.x), (0, box.y) of the slot's box; orthogonal boxes only
    static GridMap from_box(System &system, std::pair<float, float> tile_dim, uint32_t slot = 0) {
        GridMap m(system.raw());
        const float td[2] = { tile_dim.first, tile_dim.second };
        int st = 0;
        m.map_ = gr_gridmap_from_box(m.ctx_, slot, td, &st);
        if (!m.map_) m.raise(st);
        m.dims();
        return m;
    }
    ~GridMap() { if (map_) gr_gridmap_destroy(map_); }
    GridMap(const GridMap &) = delete;
    GridMap &operator=(const GridMap &) = delete;
    GridMap(GridMap &&o) noexcept : ctx_(o.ctx_), map_(o.map_), nx_(o.nx_), ny_(o.ny_), span_x_(o.span_x_), span_y_(o.span_y_), tile_(o.tile_) { o.map_ = nullptr; }

    uint64_t n_tiles_x() const { return nx_; }
    uint64_t n_tiles_y() const { return ny_; }
    uint64_t n_tiles() const { return nx_ * ny_; }
    bool is_inside(float x, float y) const {
        const int64_t ix = gr_gridmap_coord2index(span_x_.first, tile_.first, x), iy = gr_gridmap_coord2index(span_y_.first, tile_.second, y);
        return ix >= 0 && (uint64_t)ix < nx_ && iy >= 0 && (uint64_t)iy < ny_;
    }
    // the tile's coordinates; false outside the map
    bool get_tile(float x, float y, float &tx, float &ty) const {
        if (!is_inside(x, y)) return false;
        tx = gr_gridmap_index2coord(span_x_.first, tile_.first, (uint64_t)gr_gridmap_coord2index(span_x_.first, tile_.first, x));
        ty = gr_gridmap_index2coord(span_y_.first, tile_.second, (uint64_t)gr_gridmap_coord2index(span_y_.first, tile_.second, y));
        return true;
    }
    // bin the atoms of `group` of n_frames resident slots; -> atoms outside the map per frame.  A failed frame throws the first
    // failure unless `status` is given, which then receives every frame's status
    std::vector<uint64_t> accumulate(const std::string &group, uint32_t first_slot, uint32_t n_frames, GridValue value = GridValue::Count,
                                     const std::vector<float> *offset = nullptr, bool wrap = false, std::vector<int> *status = nullptr) {
        if (offset && offset->size() != n_frames) throw std::invalid_argument("GridMap::accumulate | one offset per frame");
        std::vector<uint64_t> outside(n_frames);
        std::vector<int> st(n_frames);
        const int r = gr_gridmap_accumulate_batch(map_, first_slot, n_frames, group.c_str(), (int)value, offset ? offset->data() : nullptr, wrap ? GR_GM_WRAP : 0,
                                                  outside.data(), st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        return outside;
    }
    void clear() { const int st = gr_gridmap_clear(map_); if (st != GR_OK) raise(st); }
    // caps the grids of a call's launches (0: the default); the result never depends on it
    void set_launch(uint32_t range_groups = 0, uint32_t frame_groups = 0, uint32_t check_groups = 0) { gr_gridmap_set_launch(map_, range_groups, frame_groups, check_groups); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_gridmap_stat(map_, key, &v) != GR_OK) throw std::invalid_argument("GridMap::stat | unknown key"); return v; }
    std::vector<uint64_t> counts() { std::vector<uint64_t> v(n_tiles()); read(v.data(), nullptr, nullptr); return v; }      // row-major, x outer
    std::vector<int64_t> sums_q() { std::vector<int64_t> v(n_tiles()); read(nullptr, v.data(), nullptr); return v; }        // units of 2^-20 nm
    std::vector<float> mean() { std::vector<float> v(n_tiles()); read(nullptr, nullptr, v.data()); return v; }              // NaN where nothing was counted
    gr_gridmap *raw() const { return map_; }

  private:
    explicit GridMap(gr_ctx *ctx) : ctx_(ctx) {}
    void dims() {
        float sx[2], sy[2], td[2];
        gr_gridmap_dims(map_, &nx_, &ny_, sx, sy, td);
        span_x_ = { sx[0], sx[1] }; span_y_ = { sy[0], sy[1] }; tile_ = { td[0], td[1] };
    }
    void read(uint64_t *c, int64_t *s, float *m) { const int st = gr_gridmap_read(map_, c, s, m); if (st != GR_OK) raise(st); }
    [[noreturn]] void raise(int st) const {
        const uint64_t idx = gr_last_error_index(ctx_);
        switch (st) {
        case GR_E_INVALID_SPAN: throw Error("GridMapError", "InvalidSpan", st);
        case GR_E_INVALID_TILE: throw Error("GridMapError", "InvalidGridTile", st);
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_EMPTY_GROUP: throw Error("GroupError", "EmptyGroup", st);
        case GR_E_NO_POSITION: throw Error("GroupError", "InvalidPosition", st, idx);
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("GridMapError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_gridmap *map_ = nullptr;
    uint64_t nx_ = 0, ny_ = 0;
    std::pair<float, float> span_x_{ 0.f, 0.f }, span_y_{ 0.f, 0.f }, tile_{ 0.f, 0.f };
};

// ---- Segments: the centres of every residue / molecule / listed part, for a block of resident frames, in one call
// (the loop over group_split_by_resid / molecule_iter + group_get_com of each part: groups.rs:344-435, iterating.rs:238-245)
enum class CenterKind : int { Naive = GR_CENTER_NAIVE, Estimate = GR_CENTER_ESTIMATE, Pbc = GR_CENTER_PBC };

class Segments {
  public:
    // explicit atom lists, each strictly ascending; they may overlap
    static Segments from_lists(System &system, const std::vector<std::vector<uint64_t>> &lists) {
        std::vector<uint64_t> off(lists.size() + 1, 0), atoms;
        for (size_t s = 0; s < lists.size(); ++s) { off[s + 1] = off[s] + lists[s].size(); atoms.insert(atoms.end(), lists[s].begin(), lists[s].end()); }
        if (atoms.empty()) atoms.push_back(0);
        Segments g(system.raw());
        int st = 0;
        g.seg_ = gr_segments_create(g.ctx_, off.data(), atoms.data(), lists.size(), &st);
        if (!g.seg_) g.raise(st);
        return g;
    }
    // group_split_by_resid (labels = residue numbers) / group_split_by_resname (one number per name): labels[n_atoms]; group "" = all atoms
    static Segments from_labels(System &system, const std::vector<uint64_t> &labels, const std::string &group = "") {
        if (labels.size() != gr_n_atoms(system.raw())) throw std::invalid_argument("Segments::from_labels | one label per atom");
        Segments g(system.raw());
        int st = 0;
        g.seg_ = gr_segments_from_labels(g.ctx_, group.empty() ? nullptr : group.c_str(), labels.data(), &st);
        if (!g.seg_) g.raise(st);
        return g;
    }
    // one segment per molecule of the bonds as they are now; an atom without bonds is a segment of its own
    static Segments from_molecules(System &system) {
        Segments g(system.raw());
        int st = 0;
        g.seg_ = gr_segments_from_molecules(g.ctx_, &st);
        if (!g.seg_) g.raise(st);
        return g;
    }
    ~Segments() { if (seg_) gr_segments_destroy(seg_); }
    Segments(const Segments &) = delete;
    Segments &operator=(const Segments &) = delete;
    Segments(Segments &&o) noexcept : ctx_(o.ctx_), seg_(o.seg_) { o.seg_ = nullptr; }

    uint64_t size() const { return gr_segments_count(seg_); }
    std::vector<uint64_t> sizes() const { std::vector<uint64_t> v(size()); gr_segments_sizes(seg_, v.data()); return v; }
    std::vector<uint64_t> atoms(uint64_t s) const {
        uint64_t n = 0;
        int st = gr_segments_atoms(seg_, s, nullptr, 0, &n);
        if (st != GR_OK) raise(st);
        std::vector<uint64_t> v(n);
        gr_segments_atoms(seg_, s, v.data(), n, &n);
        return v;
    }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_segments_stat(seg_, key, &v) != GR_OK) throw std::invalid_argument("Segments::stat | unknown key"); return v; }
    // [n_frames][M][3]; NaN for a segment with an atom without position / mass and for every segment of a frame that fails its box
    // check.  A failed frame throws the first failure unless `status` is given, which then receives every frame's status
    std::vector<float> centers(uint32_t first_slot, uint32_t n_frames, CenterKind kind, bool weighted, std::vector<int> *status = nullptr) {
        std::vector<float> out((size_t)n_frames * size() * 3);
        std::vector<int> st(n_frames);
        const int r = gr_segments_center_batch(seg_, first_slot, n_frames, (int)kind, weighted ? 1 : 0, out.data(), st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        return out;
    }
    std::vector<float> get_com(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) { return centers(first_slot, n_frames, CenterKind::Pbc, true, status); }
    std::vector<float> get_center(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) { return centers(first_slot, n_frames, CenterKind::Pbc, false, status); }
    // the shape of every segment: moments [n_frames][M][10] = centre (3, centers' own bits), Rg, gyration tensor xx yy zz xy xz yz;
    // with `want_axes`, axes [n_frames][M][12] = eigenvalues (descending), rows v1 v2 v3 (largest component of v1 and of v2 positive,
    // v3 = v1 x v2).  NaN rows and `status` as for centers
    struct Gyration { std::vector<float> moments, axes; };
    Gyration gyration(uint32_t first_slot, uint32_t n_frames, CenterKind kind = CenterKind::Pbc, bool weighted = true, bool want_axes = false, std::vector<int> *status = nullptr) {
        Gyration g;
        g.moments.resize((size_t)n_frames * size() * 10);
        if (want_axes) g.axes.resize((size_t)n_frames * size() * 12);
        std::vector<int> st(n_frames);
        const int r = gr_segments_gyration_batch(seg_, first_slot, n_frames, (int)kind, weighted ? 1 : 0, g.moments.data(), want_axes ? g.axes.data() : nullptr, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        return g;
    }
    // the same, left on the device until the next call on this object (read with gr_device_read); at most one piece of frames
    struct GyrationDevice { float *moments = nullptr, *axes = nullptr; };
    GyrationDevice gyration_device(uint32_t first_slot, uint32_t n_frames, CenterKind kind = CenterKind::Pbc, bool weighted = true, bool want_axes = false,
                                   std::vector<int> *status = nullptr) {
        GyrationDevice g;
        std::vector<int> st(n_frames);
        const int r = gr_segments_gyration_batch_device(seg_, first_slot, n_frames, (int)kind, weighted ? 1 : 0, want_axes ? 1 : 0, &g.moments, &g.axes, nullptr, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        return g;
    }
    // frames per piece of a gyration call; 0: as many as 256 MiB hold
    void set_piece_frames(uint32_t n) { const int st = gr_segments_set_piece_frames(seg_, n); if (st != GR_OK) raise(st); }
    gr_segments *raw() const { return seg_; }

  private:
    explicit Segments(gr_ctx *ctx) : ctx_(ctx) {}
    [[noreturn]] void raise(int st) const {
        const uint64_t idx = gr_last_error_index(ctx_);
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_EMPTY_GROUP: throw Error("GroupError", "EmptyGroup", st);
        case GR_E_NO_POSITION: throw Error("GroupError", "InvalidPosition", st, idx);
        case GR_E_NO_MASS: throw Error("GroupError", "InvalidMass", st, idx);
        case GR_E_OUT_OF_RANGE: throw Error("AtomError", "OutOfRange", st, idx);
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("GroupError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_segments *seg_ = nullptr;
};

// ---- Region: which atoms of a group lie inside a set of shapes, for every frame of a block of resident frames, in one call
// (the loop over group_iter(..).filter_geometry(..) / group_create_from_geometries of each frame: src/lib.rs:170-188, groups.rs:94-188)
class Region {
  public:
    Region(System &system, const std::vector<Shape> &shapes, bool naive = false) : ctx_(system.raw()) {
        std::vector<gr_shape> raw;
        for (const Shape &s : shapes) raw.push_back(s.c);
        int st = 0;
        rg_ = gr_region_create(ctx_, raw.data(), raw.size(), naive ? 1 : 0, &st);
        if (!rg_) raise(st);
    }
    ~Region() { if (rg_) gr_region_destroy(rg_); }
    Region(const Region &) = delete;
    Region &operator=(const Region &) = delete;
    Region(Region &&o) noexcept : ctx_(o.ctx_), rg_(o.rg_) { o.rg_ = nullptr; }

    // the atoms of `group` ("" = all atoms) inside the shapes in n_frames slots from first_slot -> the frames' counts (0 for a failed frame).
    // anchors: empty, or [n_frames][3] -- the shapes of frame f are the stored ones moved by anchors[f].  A failed frame throws the
    // first failure unless `status` is given, which then receives every frame's status
    std::vector<uint64_t> select(const std::string &group, uint32_t first_slot, uint32_t n_frames, const std::vector<float> &anchors = {},
                                 std::vector<int> *status = nullptr) {
        if (!anchors.empty() && anchors.size() != (size_t)n_frames * 3) throw std::invalid_argument("Region::select | anchors must hold n_frames x 3 floats");
        std::vector<uint64_t> counts(n_frames);
        std::vector<int> st(n_frames);
        const int r = gr_region_select_batch(rg_, first_slot, n_frames, group.empty() ? nullptr : group.c_str(), anchors.empty() ? nullptr : anchors.data(),
                                             counts.data(), st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        return counts;
    }
    // the last selection: offsets[n_frames + 1] and the atom indices, frame after frame
    std::pair<std::vector<uint64_t>, std::vector<uint64_t>> lists() {
        uint64_t nf = 0, total = 0;
        gr_region_read_device(rg_, nullptr, nullptr, &nf, &total);
        std::vector<uint64_t> off(nf + 1, 0), atoms(total);
        const int st = gr_region_read(rg_, off.data(), total ? atoms.data() : nullptr, total, nullptr);
        if (st != GR_OK) raise(st);
        return { off, atoms };
    }
    std::vector<uint64_t> frame(uint32_t f) {
        auto r = lists();
        if ((size_t)f + 1 >= r.first.size()) throw std::out_of_range("Region::frame | not a frame of the last selection");
        return std::vector<uint64_t>(r.second.begin() + (std::ptrdiff_t)r.first[f], r.second.begin() + (std::ptrdiff_t)r.first[f + 1]);
    }
    // frame f's list becomes the group `name`; true: a group of that name was replaced (AlreadyExistsWarning)
    bool to_group(uint32_t f, const std::string &name) {
        const int st = gr_region_group(rg_, f, name.c_str());
        if (st == GR_E_INVALID_NAME) throw Error("GroupError", "InvalidName", st);
        if (st != GR_OK && st != GR_E_GROUP_EXISTS) raise(st);
        return st == GR_E_GROUP_EXISTS;
    }
    void set_piece_frames(uint32_t n) { gr_region_set_piece_frames(rg_, n); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_region_stat(rg_, key, &v) != GR_OK) throw std::invalid_argument("Region::stat | unknown key"); return v; }
    gr_region *raw() const { return rg_; }

  private:
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("GroupError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_region *rg_ = nullptr;
};

// ---- Contacts: all pairs (i in group1, j in group2, i != j) within a cut-off, for every frame of a block of resident frames, in one call
// (the loop over CellGrid::new + neighbors_iter + distance filter of each frame: cellgrid.rs:301-409, hbonds.rs:248-265)
class Contacts {
  public:
    struct Lists { std::vector<uint64_t> offsets; std::vector<uint32_t> i, j; std::vector<float> d; };

    Contacts(System &system, const std::string &group1, const std::string &group2, float cutoff) : ctx_(system.raw()) {
        int st = 0;
        ct_ = gr_contacts_create(ctx_, group1.c_str(), group2.c_str(), cutoff, &st);
        if (!ct_) raise(st);
        gr_contacts_sizes(ct_, &n1_, &n2_);
    }
    ~Contacts() { if (ct_) gr_contacts_destroy(ct_); }
    Contacts(const Contacts &) = delete;
    Contacts &operator=(const Contacts &) = delete;
    Contacts(Contacts &&o) noexcept : ctx_(o.ctx_), ct_(o.ct_), n1_(o.n1_), n2_(o.n2_) { o.ct_ = nullptr; }

    uint64_t n1() const { return n1_; }
    uint64_t n2() const { return n2_; }
    // searches n_frames slots from first_slot; the lists stay on the device -> the frames' pair counts (0 for a failed frame).  When the
    // total exceeds max_pairs the call only counts.  A failed frame throws the first failure unless `status` is given
    std::vector<uint64_t> pairs(uint32_t first_slot, uint32_t n_frames, uint64_t max_pairs = UINT64_MAX, std::vector<int> *status = nullptr) {
        std::vector<uint64_t> counts(n_frames);
        std::vector<int> st(n_frames);
        const int r = gr_contacts_pairs_batch(ct_, first_slot, n_frames, max_pairs, counts.data(), nullptr, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        return counts;
    }
    // the last pairs call: offsets[n_frames + 1] and (i, j, d), frame after frame
    Lists lists() {
        uint64_t nf = 0, total = 0;
        gr_contacts_read_device(ct_, nullptr, nullptr, nullptr, nullptr, &nf, &total);
        Lists l;
        l.offsets.assign(nf + 1, 0); l.i.resize(total + 1); l.j.resize(total + 1); l.d.resize(total + 1);
        const int st = gr_contacts_read(ct_, l.offsets.data(), l.i.data(), l.j.data(), l.d.data(), total, nullptr);
        if (st != GR_OK) raise(st);
        l.i.resize(total); l.j.resize(total); l.d.resize(total);
        return l;
    }
    // per_atom[f * n1 + k] = pairs of the k-th atom of group1 in frame f; n_pairs (when given) their sums
    std::vector<uint32_t> counts(uint32_t first_slot, uint32_t n_frames, std::vector<uint64_t> *n_pairs = nullptr, std::vector<int> *status = nullptr) {
        std::vector<uint32_t> per_atom((size_t)n_frames * n1_ + 1);
        std::vector<uint64_t> np(n_frames);
        std::vector<int> st(n_frames);
        const int r = gr_contacts_count_batch(ct_, first_slot, n_frames, per_atom.data(), np.data(), st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        if (n_pairs) *n_pairs = np;
        per_atom.resize((size_t)n_frames * n1_);
        return per_atom;
    }
    // hist[f * nbins + b] over [0, cutoff)
    std::vector<uint64_t> hist(uint32_t first_slot, uint32_t n_frames, uint32_t nbins, std::vector<int> *status = nullptr) {
        std::vector<uint64_t> h((size_t)n_frames * nbins + 1);
        std::vector<int> st(n_frames);
        const int r = gr_contacts_hist_batch(ct_, first_slot, n_frames, nbins, h.data(), st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        h.resize((size_t)n_frames * nbins);
        return h;
    }
    void set_piece_frames(uint32_t n) { gr_contacts_set_piece_frames(ct_, n); }
    void set_walk_groups(uint32_t n) { gr_contacts_set_walk_groups(ct_, n); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_contacts_stat(ct_, key, &v) != GR_OK) throw std::invalid_argument("Contacts::stat | unknown key"); return v; }
    gr_contacts *raw() const { return ct_; }

  private:
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_NO_POSITION: throw Error("GroupError", "InvalidPosition", st, gr_last_error_index(ctx_));
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("GroupError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_contacts *ct_ = nullptr;
    uint64_t n1_ = 0, n2_ = 0;
};

// ---- RmsdPanel: the centred coordinates of a group for a block of frames, kept after their slots have moved on, and the all-pairs
// RMSD matrix of two panels (the double loop of System::calc_rmsd, rmsd.rs:75-166, as one f64 product on the matrix cores)
class RmsdPanel {
  public:
    RmsdPanel(System &system, const std::string &group, uint32_t capacity_frames) : ctx_(system.raw()) {
        int st = 0;
        p_ = gr_rmsd_panel_create(ctx_, group.c_str(), capacity_frames, &st);
        if (!p_) raise(st);
    }
    ~RmsdPanel() { if (p_) gr_rmsd_panel_destroy(p_); }
    RmsdPanel(const RmsdPanel &) = delete;
    RmsdPanel &operator=(const RmsdPanel &) = delete;
    RmsdPanel(RmsdPanel &&o) noexcept : ctx_(o.ctx_), p_(o.p_) { o.p_ = nullptr; }

    uint32_t frames() const { return gr_rmsd_panel_frames(p_); }
    uint64_t n_atoms() const { return gr_rmsd_panel_n_atoms(p_); }
    // packs n_frames slots from first_slot as the next rows -> their statuses; a failed frame throws the first failure unless `status` is given
    void append(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        const int r = gr_rmsd_panel_append_batch(p_, first_slot, n_frames, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
    }
    void clear() { gr_rmsd_panel_clear(p_); }
    std::vector<int> status() const { std::vector<int> s(frames() + 1); gr_rmsd_panel_status(p_, s.data()); s.resize(frames()); return s; }
    // m[i * cols.frames() + j] = calc_rmsd of row frame i (self) against column frame j (reference); NaN where either frame is invalid
    std::vector<float> matrix(RmsdPanel &cols) {
        std::vector<float> m((size_t)frames() * cols.frames() + 1);
        const int st = gr_rmsd_matrix(p_, cols.p_, m.data());
        if (st != GR_OK) raise(st);
        m.resize((size_t)frames() * cols.frames());
        return m;
    }
    std::vector<float> matrix() { return matrix(*this); }
    // the same left on the device (gr_device_read), valid until the next matrix call on this object
    float *matrix_device(RmsdPanel *cols, uint32_t *n_rows, uint32_t *n_cols) {
        float *dev = nullptr;
        const int st = gr_rmsd_matrix_device(p_, cols ? cols->p_ : nullptr, &dev, n_rows, n_cols);
        if (st != GR_OK) raise(st);
        return dev;
    }
    void set_block_entries(uint64_t n) { gr_rmsd_panel_set_block_entries(p_, n); }
    gr_rmsd_panel *raw() const { return p_; }

  private:
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("RMSDError", "NonexistentGroup", st);
        case GR_E_EMPTY_GROUP: throw Error("RMSDError", "EmptyGroup", st);
        case GR_E_INCONSISTENT_GROUP: throw Error("RMSDError", "InconsistentGroup", st);
        case GR_E_NO_POSITION: throw Error("RMSDError", "InvalidPosition", st, gr_last_error_index(ctx_));
        case GR_E_NO_MASS: throw Error("RMSDError", "InvalidMass", st, gr_last_error_index(ctx_));
        case GR_E_NO_BOX: case GR_E_NOT_ORTHOGONAL: case GR_E_ZERO_BOX: throw Error("RMSDError", "InvalidSimBox(" + simbox_variant(st) + ")", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_rmsd_panel *p_ = nullptr;
};

// ---- Fluctuations: the mean structure and the per-atom RMSF of a group over blocks of resident frames (the loop users write around
// calc_rmsd_and_fit: the reference has no function for it).  The sums are added frame after frame, so they do not depend on how the
// frames were cut into calls; after merge() they are no longer those of one sequential walk.
class Fluctuations {
  public:
    struct Raw { std::vector<float> origin; std::vector<double> sum, sumsq; uint64_t n = 0; };    // [S][3] each, group order

    Fluctuations(System &system, const std::string &group) : ctx_(system.raw()) {
        int st = 0;
        f_ = gr_fluct_create(ctx_, group.c_str(), &st);
        if (!f_) raise(st);
    }
    ~Fluctuations() { if (f_) gr_fluct_destroy(f_); }
    Fluctuations(const Fluctuations &) = delete;
    Fluctuations &operator=(const Fluctuations &) = delete;
    Fluctuations(Fluctuations &&o) noexcept : ctx_(o.ctx_), f_(o.f_) { o.f_ = nullptr; }

    uint64_t frames() const { return gr_fluct_frames(f_); }
    uint64_t n_atoms() const { return gr_fluct_n_atoms(f_); }
    // counts n_frames slots from first_slot; a failed frame (an atom of the group without position) is counted for no atom and throws
    // the first failure unless `status` is given
    void accumulate(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        const int r = gr_fluct_accumulate_batch(f_, first_slot, n_frames, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
    }
    void clear() { check(gr_fluct_clear(f_)); }
    // mean [S][3], variance per axis [S][3], rmsf [S]: NaN before the first counted frame
    std::vector<double> mean() { std::vector<double> m(3 * n_atoms() + 1); check(gr_fluct_read(f_, m.data(), nullptr, nullptr)); m.resize(3 * n_atoms()); return m; }
    std::vector<double> variance() { std::vector<double> v(3 * n_atoms() + 1); check(gr_fluct_read(f_, nullptr, v.data(), nullptr)); v.resize(3 * n_atoms()); return v; }
    std::vector<double> rmsf() { std::vector<double> r(n_atoms() + 1); check(gr_fluct_read(f_, nullptr, nullptr, r.data())); r.resize(n_atoms()); return r; }
    Raw raw() {
        Raw r;
        const size_t n = 3 * n_atoms();
        r.origin.resize(n + 1); r.sum.resize(n + 1); r.sumsq.resize(n + 1);
        check(gr_fluct_read_raw(f_, r.origin.data(), r.sum.data(), r.sumsq.data(), &r.n));
        r.origin.resize(n); r.sum.resize(n); r.sumsq.resize(n);
        return r;
    }
    void merge(Fluctuations &src) { check(gr_fluct_merge(f_, src.f_)); }
    // the mean, rounded to f32, into the group's atoms of `slot` of `dst` (same device, same number of atoms): the reference of a new RmsdPlan
    void store_mean(System &dst, uint32_t slot) { check(gr_fluct_store_mean(f_, dst.raw(), slot)); }
    void set_launch(uint32_t range_groups, uint32_t check_groups) { gr_fluct_set_launch(f_, range_groups, check_groups); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_fluct_stat(f_, key, &v) != GR_OK) throw std::invalid_argument("Fluctuations::stat | unknown key"); return v; }
    gr_fluct *raw_handle() const { return f_; }

  private:
    void check(int st) const { if (st != GR_OK) raise(st); }
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_EMPTY_GROUP: throw Error("GroupError", "EmptyGroup", st);
        case GR_E_INCONSISTENT_GROUP: throw Error("GroupError", "InconsistentGroup", st);
        case GR_E_NO_POSITION: throw Error("GroupError", "InvalidPosition", st, gr_last_error_index(ctx_));
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_fluct *f_ = nullptr;
};

// ---- Covariance: the positional covariance matrix (3S x 3S, optionally mass-weighted) and the dynamical cross-correlation map (S x S)
// of a group over blocks of resident frames: the step after Fluctuations (essential dynamics; the reference has no function for it).
// The state's bits depend on the sequence of calls alone; after merge() the sums are no longer those of one walk.  The eigen-solve is
// the caller's (LAPACK dsyevd on matrix()).
class Covariance {
  public:
    struct Raw { std::vector<float> origin; std::vector<double> sum, Q; uint64_t n = 0; };    // [D], [D], [D][D] (D = 3S, group order)

    Covariance(System &system, const std::string &group) : ctx_(system.raw()) {
        int st = 0;
        f_ = gr_covar_create(ctx_, group.c_str(), &st);
        if (!f_) raise(st);
    }
    ~Covariance() { if (f_) gr_covar_destroy(f_); }
    Covariance(const Covariance &) = delete;
    Covariance &operator=(const Covariance &) = delete;
    Covariance(Covariance &&o) noexcept : ctx_(o.ctx_), f_(o.f_) { o.f_ = nullptr; }

    uint64_t frames() const { return gr_covar_frames(f_); }
    uint64_t n_atoms() const { return gr_covar_n_atoms(f_); }
    // counts n_frames slots from first_slot; a failed frame (an atom of the group without position) is counted for no dimension and
    // throws the first failure unless `status` is given
    void accumulate(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        const int r = gr_covar_accumulate_batch(f_, first_slot, n_frames, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
    }
    void clear() { check(gr_covar_clear(f_)); }
    // mean [D], covariance [D][D] (divided by n; mass_weighted: times sqrt(m_i m_j)), DCCM [S][S]: NaN before the first counted frame
    std::vector<double> mean() { std::vector<double> m(3 * n_atoms()); check(gr_covar_read(f_, m.data(), nullptr, 0)); return m; }
    std::vector<double> matrix(bool mass_weighted = false) {
        const size_t d = 3 * n_atoms();
        std::vector<double> c(d * d);
        check(gr_covar_read(f_, nullptr, c.data(), mass_weighted ? GR_CV_MASS_WEIGHTED : 0u));
        return c;
    }
    std::vector<double> dccm() { std::vector<double> c(n_atoms() * n_atoms()); check(gr_covar_read_dccm(f_, c.data())); return c; }
    Raw raw() {
        Raw r;
        const size_t d = 3 * n_atoms();
        r.origin.resize(d); r.sum.resize(d); r.Q.resize(d * d);
        check(gr_covar_read_raw(f_, r.origin.data(), r.sum.data(), r.Q.data(), &r.n));
        return r;
    }
    void merge(Covariance &src) { check(gr_covar_merge(f_, src.f_)); }
    void set_launch(uint32_t product_groups, uint32_t check_groups) { gr_covar_set_launch(f_, product_groups, check_groups); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_covar_stat(f_, key, &v) != GR_OK) throw std::invalid_argument("Covariance::stat | unknown key"); return v; }
    gr_covar *raw_handle() const { return f_; }

  private:
    void check(int st) const { if (st != GR_OK) raise(st); }
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_EMPTY_GROUP: throw Error("GroupError", "EmptyGroup", st);
        case GR_E_INCONSISTENT_GROUP: throw Error("GroupError", "InconsistentGroup", st);
        case GR_E_NO_POSITION: throw Error("GroupError", "InvalidPosition", st, gr_last_error_index(ctx_));
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_covar *f_ = nullptr;
};

// ---- Msd: "nojump" unwrapping and the windowed mean-squared displacement of a group over blocks of resident frames (diffusion; the
// reference has no function for it).  append() takes frames as time indices -- a failed frame still takes one and enters no pair --,
// msd(max_lag) closes the band of lags.  Displacements, q and the sums are a function of the sequence of appended frames alone.
class Msd {
  public:
    struct Curve { std::vector<double> msd; std::vector<uint64_t> pairs; };     // [lags] each; msd is NaN where pairs is 0

    Msd(System &system, const std::string &group, uint32_t capacity_frames, uint32_t flags = GR_MSD_X | GR_MSD_Y | GR_MSD_Z | GR_MSD_NOJUMP) : ctx_(system.raw()) {
        int st = 0;
        f_ = gr_msd_create(ctx_, group.c_str(), capacity_frames, flags, &st);
        if (!f_) raise(st);
    }
    ~Msd() { if (f_) gr_msd_destroy(f_); }
    Msd(const Msd &) = delete;
    Msd &operator=(const Msd &) = delete;
    Msd(Msd &&o) noexcept : ctx_(o.ctx_), f_(o.f_) { o.f_ = nullptr; }

    uint64_t frames() const { return gr_msd_frames(f_); }
    uint64_t n_atoms() const { return gr_msd_n_atoms(f_); }
    uint64_t capacity() const { return gr_msd_capacity(f_); }
    // appends n_frames slots from first_slot; a failed frame takes a time index and enters no pair; throws the first failure unless
    // `status` is given.  A refused call (beyond the capacity, slots out of range) always throws
    void append(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        const int r = gr_msd_append_batch(f_, first_slot, n_frames, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
    }
    void clear() { check(gr_msd_clear(f_)); }
    // the curve for lags 0 .. max_lag (clamped to frames() - 1)
    Curve msd(uint32_t max_lag = 0xFFFFFFFFu) {
        check(gr_msd_compute(f_, max_lag));
        Curve c;
        const size_t lags = (size_t)stat(GR_MSD_STAT_LAGS);
        c.msd.resize(lags); c.pairs.resize(lags);
        check(gr_msd_read(f_, c.msd.data(), c.pairs.data()));
        return c;
    }
    std::vector<double> from_origin() { std::vector<double> o(frames()); if (!o.empty()) check(gr_msd_read_from_origin(f_, o.data())); return o; }
    // [nt][S][3]: rows t0 .. t0 + nt - 1 of the panel in group order
    std::vector<float> displacements(uint32_t t0, uint32_t nt) {
        std::vector<float> d((size_t)nt * 3 * n_atoms());
        check(gr_msd_read_displacements(f_, t0, nt, d.data()));
        return d;
    }
    void set_launch(uint32_t walk_groups, uint32_t gram_groups) { gr_msd_set_launch(f_, walk_groups, gram_groups); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_msd_stat(f_, key, &v) != GR_OK) throw std::invalid_argument("Msd::stat | unknown key"); return v; }
    gr_msd *raw_handle() const { return f_; }

  private:
    void check(int st) const { if (st != GR_OK) raise(st); }
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_GROUP_NOT_FOUND: throw Error("GroupError", "NotFound", st);
        case GR_E_EMPTY_GROUP: throw Error("GroupError", "EmptyGroup", st);
        case GR_E_NO_POSITION: throw Error("GroupError", "InvalidPosition", st, gr_last_error_index(ctx_));
        case GR_E_NO_BOX: throw Error("SimBoxError", "DoesNotExist", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_msd *f_ = nullptr;
};

// ---- VectorCorrelation: the P1 / P2 reorientation autocorrelation functions of a fixed list of bond vectors (i, j) over the frames
// handed to append() (gmx rotacf; the rotational counterpart of Msd): correlate() closes the band of lags over all vectors on the f64
// matrix cores, correlate_each() gives the curve of every vector.  groan_hip.h has the rule, the order of the sums and what is not promised.
class VectorCorrelation {
  public:
    struct Curves { std::vector<double> c1, c2; std::vector<uint64_t> pairs; };     // [lags] each; c1 / c2 empty for a rank that is not kept, NaN where pairs is 0
    struct Each { std::vector<double> c1, c2; size_t lags = 0; };                   // [V][lags] each; empty for a rank that is not kept

    // pairs: [V][2] row-major
    VectorCorrelation(System &system, const std::vector<uint64_t> &pairs, uint32_t capacity_frames,
                      uint32_t flags = GR_VCORR_UNIT | GR_VCORR_P1 | GR_VCORR_P2) : ctx_(system.raw()), flags_(flags) {
        int st = 0;
        f_ = gr_vcorr_create(ctx_, pairs.data(), pairs.size() / 2, capacity_frames, flags, &st);
        if (!f_) raise(st);
    }
    ~VectorCorrelation() { if (f_) gr_vcorr_destroy(f_); }
    VectorCorrelation(const VectorCorrelation &) = delete;
    VectorCorrelation &operator=(const VectorCorrelation &) = delete;
    VectorCorrelation(VectorCorrelation &&o) noexcept : ctx_(o.ctx_), f_(o.f_), flags_(o.flags_) { o.f_ = nullptr; }

    uint64_t count() const { return gr_vcorr_count(f_); }
    uint64_t frames() const { return gr_vcorr_frames(f_); }
    uint64_t capacity() const { return gr_vcorr_capacity(f_); }
    // appends n_frames slots from first_slot; a failed frame takes a time index and enters no pair; throws the first failure unless
    // `status` is given.  A refused call (beyond the capacity, slots out of range) always throws
    void append(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        const int r = gr_vcorr_append_batch(f_, first_slot, n_frames, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
    }
    void clear() { check(gr_vcorr_clear(f_)); }
    // the curves over all vectors for lags 0 .. max_lag (clamped to frames() - 1)
    Curves correlate(uint32_t max_lag = 0xFFFFFFFFu) {
        check(gr_vcorr_compute(f_, max_lag));
        Curves c;
        const size_t lags = (size_t)stat(GR_VCORR_STAT_LAGS);
        if (flags_ & GR_VCORR_P1) c.c1.resize(lags);
        if (flags_ & GR_VCORR_P2) c.c2.resize(lags);
        c.pairs.resize(lags);
        check(gr_vcorr_read(f_, c.c1.empty() ? nullptr : c.c1.data(), c.c2.empty() ? nullptr : c.c2.data(), c.pairs.data()));
        return c;
    }
    // the curves of every vector
    Each correlate_each(uint32_t max_lag = 0xFFFFFFFFu) {
        Each e;
        const uint64_t n = frames();
        e.lags = (size_t)std::min<uint64_t>(max_lag, n ? n - 1 : 0) + 1;
        if (flags_ & GR_VCORR_P1) e.c1.resize((size_t)count() * e.lags);
        if (flags_ & GR_VCORR_P2) e.c2.resize((size_t)count() * e.lags);
        check(gr_vcorr_compute_each(f_, max_lag, e.c1.empty() ? nullptr : e.c1.data(), e.c2.empty() ? nullptr : e.c2.data()));
        return e;
    }
    // [nt][V][3]: rows t0 .. t0 + nt - 1 of the rank-1 panel in the caller's order
    std::vector<float> vectors(uint32_t t0, uint32_t nt) {
        std::vector<float> d((size_t)nt * 3 * count());
        check(gr_vcorr_read_vectors(f_, t0, nt, d.data()));
        return d;
    }
    void set_launch(uint32_t walk_groups, uint32_t gram_groups, uint32_t each_groups) { gr_vcorr_set_launch(f_, walk_groups, gram_groups, each_groups); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_vcorr_stat(f_, key, &v) != GR_OK) throw std::invalid_argument("VectorCorrelation::stat | unknown key"); return v; }
    gr_vcorr *raw_handle() const { return f_; }

  private:
    void check(int st) const { if (st != GR_OK) raise(st); }
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_OUT_OF_RANGE: throw Error("AtomError", "OutOfRange", st, gr_last_error_index(ctx_));
        case GR_E_NO_POSITION: throw Error("AtomError", "InvalidPosition", st, gr_last_error_index(ctx_));
        case GR_E_NO_BOX: throw Error("SimBoxError", "DoesNotExist", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_vcorr *f_ = nullptr;
    uint32_t flags_ = 0;
};

// ---- Internals: the distance, angle, dihedral or axis cosine of a fixed list of atom tuples in every frame of a block of resident
// frames (values), or their running mean and variance over any number of calls (accumulate); the reference has Vector3D::angle and
// distance only.  Angles in radians, the dihedral's sign is IUPAC's (groan_hip.h has the definitions).  The sums are added frame after
// frame, so they do not depend on how the frames were cut into calls; after merge() they are no longer those of one walk.
class Internals {
  public:
    struct Raw { std::vector<float> origin; std::vector<double> sum, sumsq; uint64_t n = 0; };    // [T] each
    struct Stats { std::vector<double> mean, var; };                                             // [T] each

    // tuples: [T][arity] row-major (arity 2, 3, 4, 2 for GR_IC_DISTANCE, _ANGLE, _DIHEDRAL, _AXIS); axis: GR_IC_AXIS only
    Internals(System &system, int kind, const std::vector<uint64_t> &tuples, uint32_t flags = GR_IC_PBC, const float *axis = nullptr) : ctx_(system.raw()) {
        const uint64_t arity = kind == GR_IC_ANGLE ? 3 : (kind == GR_IC_DIHEDRAL ? 4 : 2);
        int st = 0;
        f_ = gr_internals_create(ctx_, kind, tuples.data(), tuples.size() / arity, flags, axis, &st);
        if (!f_) raise(st);
    }
    ~Internals() { if (f_) gr_internals_destroy(f_); }
    Internals(const Internals &) = delete;
    Internals &operator=(const Internals &) = delete;
    Internals(Internals &&o) noexcept : ctx_(o.ctx_), f_(o.f_) { o.f_ = nullptr; }

    uint64_t count() const { return gr_internals_count(f_); }
    uint64_t frames() const { return gr_internals_frames(f_); }
    // [n_frames][T]; a failed frame is a row of NaN and throws the first failure unless `status` is given.  A refused call always throws
    std::vector<float> values(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        std::vector<float> out((size_t)n_frames * count() + 1);
        const int r = gr_internals_values_batch(f_, first_slot, n_frames, out.data(), st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
        out.resize((size_t)n_frames * count());
        return out;
    }
    // the same into device memory: row f starts f * ld floats in (ld >= T)
    void values_device(uint32_t first_slot, uint32_t n_frames, float *out_dev, uint64_t ld, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        const int r = gr_internals_values_batch_device(f_, first_slot, n_frames, out_dev, ld, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
    }
    // counts n_frames slots from first_slot; a failed frame is counted for no tuple
    void accumulate(uint32_t first_slot, uint32_t n_frames, std::vector<int> *status = nullptr) {
        std::vector<int> st(n_frames);
        const int r = gr_internals_accumulate_batch(f_, first_slot, n_frames, st.data());
        detail::batch_status(r, st, status, [this](int e) { raise(e); });
    }
    void clear() { check(gr_internals_clear(f_)); }
    // mean and variance (divided by n) per tuple; throws before the first counted frame
    Stats read() { Stats s; s.mean.resize(count()); s.var.resize(count()); check(gr_internals_read(f_, s.mean.data(), s.var.data())); return s; }
    Raw raw() {
        Raw r;
        r.origin.resize(count()); r.sum.resize(count()); r.sumsq.resize(count());
        check(gr_internals_read_raw(f_, r.origin.data(), r.sum.data(), r.sumsq.data(), &r.n));
        return r;
    }
    // S = 1/2 <3 cos^2 - 1> per tuple (GR_IC_AXIS)
    std::vector<double> order_parameter() {
        const Stats s = read();
        std::vector<double> p(s.mean.size());
        for (size_t t = 0; t < p.size(); ++t) p[t] = 1.5 * (s.var[t] + s.mean[t] * s.mean[t]) - 0.5;
        return p;
    }
    void merge(Internals &src) { check(gr_internals_merge(f_, src.f_)); }
    void set_launch(uint32_t tuple_ranges, uint32_t frame_chunk) { gr_internals_set_launch(f_, tuple_ranges, frame_chunk); }
    uint64_t stat(int key) const { uint64_t v = 0; if (gr_internals_stat(f_, key, &v) != GR_OK) throw std::invalid_argument("Internals::stat | unknown key"); return v; }
    gr_internals *raw_handle() const { return f_; }

  private:
    void check(int st) const { if (st != GR_OK) raise(st); }
    [[noreturn]] void raise(int st) const {
        switch (st) {
        case GR_E_OUT_OF_RANGE: throw Error("AtomError", "OutOfRange", st, gr_last_error_index(ctx_));
        case GR_E_NO_POSITION: throw Error("AtomError", "InvalidPosition", st, gr_last_error_index(ctx_));
        case GR_E_INCONSISTENT_GROUP: throw Error("GroupError", "InconsistentGroup", st);
        case GR_E_NO_BOX: throw Error("SimBoxError", "DoesNotExist", st);
        default: throw Error("DeviceError", std::string(gr_status_string(st)) + ": " + gr_last_error(ctx_), st);
        }
    }
    gr_ctx *ctx_ = nullptr;
    gr_internals *f_ = nullptr;
};

}  // namespace groan

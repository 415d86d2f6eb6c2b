// tests/cpp/test_objects.cpp -- the second half of the C++ host mirror (include/groan_hip.hpp): the eight batch objects HBondPlan,
// GridMap, Segments, Region, Contacts, RmsdPanel, Fluctuations and Covariance.  (test_host.cpp covers the first half: System,
// AtomContainer, Shape, the iterators, the RMSD analyzer, the readers and writers.)  Built by __graft_entry__.build() (g++, links
// libgroan_hip.so), run on the GPU box by tests/test_gpu_cpp_objects.py:  test_objects <fixture dir> <output dir>
//
// The fixtures are the world of tests/cpp_objects_world.py (the calls below use that module's numbers), raw little-endian:
//   frames.f32 [NS][N][3] (NaN: no position)  boxes.f32 [NS][9] (a NaN row: no box)  masses.f32 [N]  bonds.u64 [2 N / 3][2]
//   labels.u64 [N]  group_<name>.u64  meta.u64 = N, NS, the slot with an atom without position, the slot without a box, that atom
// Every array a method returns is written to <output dir>/<object>.<call>.<field>.<type>; the Python test compares those files with
// each object's reference and, bit for bit, with the Python class of the same name run through the same calls.  This program decides
// only what needs no reference: the sizes of what comes back, the moves, the errors, and that a repeated call repeats its result.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/groan_hip.hpp"

using namespace groan;
static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #__VA_ARGS__); ++failures; } } while (0)

static std::string out_dir;

template <typename T> static std::vector<T> load(const std::string &path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) { printf("cannot open %s\n", path.c_str()); exit(2); }
    std::vector<T> v((size_t)f.tellg() / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return v;
}

template <typename T> static void dump(const std::string &name, const std::vector<T> &v) {
    std::ofstream f(out_dir + "/" + name, std::ios::binary);
    if (!f) { printf("cannot write %s\n", name.c_str()); exit(2); }
    if (!v.empty()) f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

// once the device has reported an error nothing more may be launched on it: not even the destructors run
[[noreturn]] static void device_failed(const Error &e) {
    printf("the device reported an error, stopping: %s\n", e.what());
    fflush(stdout);
    std::_Exit(3);
}
static void hip_stop(const Error &e) { if (e.status == GR_E_HIP) device_failed(e); }

// `call` must throw a groan::Error for which `cond` holds
#define THROWS(call, cond) do { bool thrown_ = false; try { call; } catch (const Error &e) { hip_stop(e); thrown_ = true; CHECK(cond); } \
                                if (!thrown_) { printf("FAIL %s:%d  no throw: %s\n", __FILE__, __LINE__, #call); ++failures; } } while (0)

template <typename T> static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static uint64_t NAN_ATOM = 0;

// what a batch without `status` must throw when the same batch with `status` reported `st`: the first failure, as raise() words it
static bool is_first_failure(const Error &e, const std::vector<int> &st) {
    int first = GR_OK;
    for (int s : st) if (s != GR_OK) { first = s; break; }
    if (first == GR_OK || e.status != first) return false;
    if (first == GR_E_NO_POSITION) return e.variant.find("InvalidPosition") != std::string::npos && e.index == NAN_ATOM;
    if (first == GR_E_NO_BOX) return e.variant == "InvalidSimBox(DoesNotExist)";
    return false;
}
static bool any_failed(const std::vector<int> &st) { for (int s : st) if (s != GR_OK) return true; return false; }

// result[f][p] flattened in [f][p] order: the bonds' fields and the number of bonds per (frame, pair)
static void dump_bonds(const std::string &name, const std::vector<std::vector<std::vector<HBond>>> &r) {
    std::vector<uint32_t> idx; std::vector<float> val; std::vector<uint64_t> n;
    for (const auto &frame : r)
        for (const auto &pair : frame) {
            n.push_back(pair.size());
            for (const HBond &b : pair) { idx.push_back(b.donor); idx.push_back(b.hydrogen); idx.push_back(b.acceptor); val.push_back(b.distance); val.push_back(b.angle); }
        }
    dump(name + ".atoms.u32", idx); dump(name + ".values.f32", val); dump(name + ".n.u64", n);
}
static bool same_bonds(const std::vector<std::vector<std::vector<HBond>>> &a, const std::vector<std::vector<std::vector<HBond>>> &b) {
    if (a.size() != b.size()) return false;
    for (size_t f = 0; f < a.size(); ++f) {
        if (a[f].size() != b[f].size()) return false;
        for (size_t p = 0; p < a[f].size(); ++p) {
            if (a[f][p].size() != b[f][p].size()) return false;
            for (size_t k = 0; k < a[f][p].size(); ++k)
                if (std::memcmp(&a[f][p][k], &b[f][p][k], sizeof(HBond)) != 0) return false;
        }
    }
    return true;
}

static void run(const std::string &dir) {
    const std::vector<uint64_t> meta = load<uint64_t>(dir + "/meta.u64");
    CHECK(meta.size() == 5);
    const uint64_t N = meta[0];
    const uint32_t NS = (uint32_t)meta[1], NAN_SLOT = (uint32_t)meta[2], NOBOX_SLOT = (uint32_t)meta[3];
    NAN_ATOM = meta[4];
    const std::vector<float> frames = load<float>(dir + "/frames.f32"), boxes = load<float>(dir + "/boxes.f32"), masses = load<float>(dir + "/masses.f32");
    const std::vector<uint64_t> bonds_flat = load<uint64_t>(dir + "/bonds.u64"), labels = load<uint64_t>(dir + "/labels.u64");
    CHECK(frames.size() == (size_t)NS * N * 3 && boxes.size() == (size_t)NS * 9 && masses.size() == N && labels.size() == N);
    CHECK(NAN_SLOT > 0 && NAN_SLOT < NS - 1 && NOBOX_SLOT > 0 && NOBOX_SLOT < NS - 1);     // the failing frames lie inside the batches
    std::vector<std::pair<uint64_t, uint64_t>> bonds;
    for (size_t k = 0; k + 1 < bonds_flat.size(); k += 2) bonds.emplace_back(bonds_flat[k], bonds_flat[k + 1]);

    System sys(N, 0, NS), one(N, 0, 1);             // `one`: the one-slot System that store_mean writes into
    sys.set_masses(masses); one.set_masses(masses);
    for (uint32_t f = 0; f < NS; ++f) {
        Box9 b; for (int k = 0; k < 9; ++k) b[k] = boxes[9 * f + k];
        sys.set_frame(frames.data() + (size_t)f * N * 3, std::isnan(b[0]) ? nullptr : &b, f);
    }
    {
        Box9 b; for (int k = 0; k < 9; ++k) b[k] = boxes[k];
        const std::vector<float> zeros(N * 3, 0.0f);
        one.set_frame(zeros.data(), &b);
    }
    sys.group_create_from_ranges("rng", {{5, 160}});                       // a range that starts neither at atom 0 nor on a multiple of 4
    one.group_create_from_ranges("rng", {{5, 160}});
    for (const char *g : {"lst", "hyd", "oxy", "oxyA", "hydA", "oxyB", "hydB"})        // index lists; hyd: the hydrogens
        sys.group_create_from_indices(g, load<uint64_t>(dir + "/group_" + g + ".u64"));
    sys.add_bonds(bonds);
    const uint64_t n_rng = sys.group_get_n_atoms("rng"), n_lst = sys.group_get_n_atoms("lst"), n_hyd = sys.group_get_n_atoms("hyd");
    const uint32_t PAST = NS - 1;                   // a batch (PAST, 2) ends one past the last slot
    std::vector<int> st;
    const std::vector<int> untouched = {77};

    // ================================================================ HBondPlan
    {
        const std::vector<HBondChain> chains = {{"oxyA", "oxyA", "hydA"}, {"oxyB", "oxyB", "hydB"}};      // two chains, two pairs
        const std::vector<std::pair<uint32_t, uint32_t>> pairs = {{0, 0}, {0, 1}};
        HBondPlan hb(sys, chains, pairs, bonds, 0.31f, 135.0f);
        CHECK(hb.raw() != nullptr && hb.pairs() == pairs);
        // cap_ == 0: the first pass only counts, cap_ grows, the second pass writes; unflattening offs[f * np + p]; failing frames in `st`
        auto all = hb.batch(0, NS, &st);
        CHECK(all.size() == NS && st.size() == NS);
        for (const auto &f : all) CHECK(f.size() == pairs.size());
        dump_bonds("hbond.all", all); dump("hbond.all.status.i32", st);
        // the capacity hint holds now: one pass, the same result
        std::vector<int> st2;
        auto again = hb.batch(0, NS, &st2);
        CHECK(same_bonds(all, again) && st2 == st);
        // without `status`: the first failure is thrown
        if (any_failed(st)) THROWS(hb.batch(0, NS), e.kind == "HBondError" && is_first_failure(e, st));
        else CHECK(same_bonds(all, hb.batch(0, NS)));
        // n_frames == 1, first_slot != 0
        auto single = hb.batch(3, 1);
        CHECK(single.size() == 1 && single[0].size() == 2);
        dump_bonds("hbond.one", single);
        // first_slot != 0, more than one frame
        auto tail = hb.batch(7, 3, &st);
        CHECK(tail.size() == 3 && st.size() == 3);
        dump_bonds("hbond.tail", tail); dump("hbond.tail.status.i32", st);
        // a refused call throws although `status` is given: the slot range ends one past the last slot
        st = untouched;
        THROWS(hb.batch(PAST, 2, &st), e.status == GR_E_INVALID_ARG && e.kind == "DeviceError");
        CHECK(st == untouched);
        // ... and the object still works afterwards
        CHECK(same_bonds(all, hb.batch(0, NS, &st2)));
        // move: the new object owns the plan, its pairs and its capacity hint
        HBondPlan moved(std::move(hb));
        CHECK(hb.raw() == nullptr && moved.raw() != nullptr && moved.pairs() == pairs);
        CHECK(same_bonds(all, moved.batch(0, NS, &st2)) && st2.size() == NS);
        // a plan that finds nothing: cap_ == 0 and total == 0, one pass, every list empty
        HBondPlan none(sys, chains, pairs, bonds, 0.15f, 135.0f);
        auto empty = none.batch(0, 3, &st);
        CHECK(empty.size() == 3 && st.size() == 3);
        for (const auto &f : empty) for (const auto &p : f) CHECK(p.empty());
        dump_bonds("hbond.none", empty); dump("hbond.none.status.i32", st);
        // errors of the constructor keep the reference's names
        THROWS(HBondPlan(sys, {{"oxyA", "oxyA", "nobody"}}, {{0, 0}}, bonds, 0.31f, 135.0f), e.kind == "HBondError" && e.variant == "SelectError");
        THROWS(HBondPlan(sys, chains, {{0, 0}, {0, 2}}, bonds, 0.31f, 135.0f), e.variant == "NonexistentChain" && e.index == 2);
        THROWS(HBondPlan(sys, chains, {{0, 1}, {1, 0}}, bonds, 0.31f, 135.0f), e.variant == "PairSpecifiedMultipleTimes");
        THROWS(HBondPlan(sys, chains, {{0, 0}}, bonds, 0.31f, 135.0f), e.variant == "UnusedChain");
    }

    // ================================================================ GridMap
    {
        GridMap m(sys, {0.5f, 2.5f}, {0.4f, 2.8f}, {0.25f, 0.3f});           // the constructor with spans
        CHECK(m.raw() != nullptr && m.n_tiles() == m.n_tiles_x() * m.n_tiles_y());
        dump("gridmap.m1.dims.u64", std::vector<uint64_t>{m.n_tiles_x(), m.n_tiles_y()});
        // get_tile / is_inside: inside, outside, on the lower edge
        const float pts[7][2] = {{1.0f, 1.0f}, {2.6f, 2.9f}, {0.0f, 1.0f}, {1.0f, 9.0f}, {0.375f, 0.25f}, {0.37f, 1.0f}, {-1.0f, -1.0f}};
        std::vector<int> inside; std::vector<float> tiles;
        for (const auto &p : pts) {
            float tx = NAN, ty = NAN;
            const bool in = m.get_tile(p[0], p[1], tx, ty);
            CHECK(in == m.is_inside(p[0], p[1]) && in == !std::isnan(tx) && in == !std::isnan(ty));
            inside.push_back(in ? 1 : 0); tiles.push_back(tx); tiles.push_back(ty);
        }
        dump("gridmap.m1.inside.i32", inside); dump("gridmap.m1.tiles.f32", tiles);
        auto read_out = [&](GridMap &g, const std::string &name) {
            const auto c = g.counts(); const auto s = g.sums_q(); const auto mean = g.mean();
            CHECK(c.size() == g.n_tiles() && s.size() == g.n_tiles() && mean.size() == g.n_tiles());
            dump(name + ".counts.u64", c); dump(name + ".sums_q.i64", s); dump(name + ".mean.f32", mean);
        };
        // GridValue::Count over every slot, failing frames in `st`
        auto outside = m.accumulate("rng", 0, NS, GridValue::Count, nullptr, false, &st);
        CHECK(outside.size() == NS && st.size() == NS && any_failed(st));
        dump("gridmap.count.outside.u64", outside); dump("gridmap.count.status.i32", st);
        read_out(m, "gridmap.count");
        THROWS(m.accumulate("rng", 0, NS), e.kind == "GroupError" && is_first_failure(e, st));
        m.clear();
        // the move: same handle, same geometry, same bytes
        GridMap moved(std::move(m));
        CHECK(m.raw() == nullptr && moved.raw() != nullptr && moved.n_tiles_x() * moved.n_tiles_y() == moved.n_tiles() && moved.is_inside(1.0f, 1.0f));
        {
            std::vector<int> st2;
            CHECK(same(outside, moved.accumulate("rng", 0, NS, GridValue::Count, nullptr, false, &st2)) && st2 == st);
            CHECK(same(load<uint64_t>(out_dir + "/gridmap.count.counts.u64"), moved.counts()));
        }
        // GridValue::Z with an offset; n_frames == 1, first_slot != 0
        const std::vector<float> off = {0.7f};
        outside = moved.accumulate("lst", 3, 1, GridValue::Z, &off);
        CHECK(outside.size() == 1);
        dump("gridmap.z.outside.u64", outside); read_out(moved, "gridmap.z");
        // GridValue::X on top of it
        outside = moved.accumulate("hyd", 0, 4, GridValue::X);
        CHECK(outside.size() == 4);
        dump("gridmap.x.outside.u64", outside); read_out(moved, "gridmap.x");
        moved.clear();
        read_out(moved, "gridmap.cleared");
        // from_box, GridValue::Y, wrap: the frame without a box fails too
        GridMap fb = GridMap::from_box(sys, {0.4f, 0.5f}, 1);
        dump("gridmap.m2.dims.u64", std::vector<uint64_t>{fb.n_tiles_x(), fb.n_tiles_y()});
        outside = fb.accumulate("hyd", 0, NS, GridValue::Y, nullptr, true, &st);
        CHECK(outside.size() == NS && st.size() == NS);
        dump("gridmap.wrap.outside.u64", outside); dump("gridmap.wrap.status.i32", st);
        read_out(fb, "gridmap.wrap");
        THROWS(fb.accumulate("hyd", 0, NS, GridValue::Y, nullptr, true), is_first_failure(e, st));     // (the frames that did not fail were binned again)
        // set_launch caps the grids of the launches and never changes the result; stat reports what was launched
        {
            const auto before = load<uint64_t>(out_dir + "/gridmap.wrap.counts.u64"); const auto before_q = load<int64_t>(out_dir + "/gridmap.wrap.sums_q.i64");
            std::vector<int> st2;
            fb.clear();
            fb.set_launch(1, 1, 1);
            CHECK(same(outside, fb.accumulate("hyd", 0, NS, GridValue::Y, nullptr, true, &st2)) && st2 == st);
            CHECK(same(before, fb.counts()) && same(before_q, fb.sums_q()) && fb.stat(GR_GM_STAT_LAST_RANGE_GROUPS) == 1);
            CHECK(fb.stat(GR_GM_STAT_LDS_LAUNCHES) + fb.stat(GR_GM_STAT_GLOBAL_LAUNCHES) >= 2);
            try { fb.stat(99); CHECK(false); } catch (const std::invalid_argument &) {}
            fb.set_launch();
        }
        // refused calls throw although `status` is given: the slot range, a group that does not exist
        st = untouched;
        THROWS(fb.accumulate("hyd", PAST, 2, GridValue::Count, nullptr, false, &st), e.status == GR_E_INVALID_ARG);
        THROWS(fb.accumulate("nobody", 0, 4, GridValue::Count, nullptr, false, &st), e.kind == "GroupError" && e.variant == "NotFound");
        CHECK(st == untouched);
        try { fb.accumulate("hyd", 0, 2, GridValue::Z, &off); CHECK(false); } catch (const std::invalid_argument &) {}      // one offset per frame
        THROWS(GridMap(sys, {2.0f, 1.0f}, {0.0f, 1.0f}, {0.1f, 0.1f}), e.kind == "GridMapError" && e.variant == "InvalidSpan");
        THROWS(GridMap(sys, {0.0f, 1.0f}, {0.0f, 1.0f}, {2.0f, 0.1f}), e.variant == "InvalidGridTile");
        THROWS(GridMap::from_box(sys, {0.4f, 0.5f}, NOBOX_SLOT), e.variant == "InvalidSimBox(DoesNotExist)");
    }

    // ================================================================ Segments
    {
        // from_lists: four lists of 9, 5, 4 and 40 atoms, the second overlapping the first, the third holding the atom without position
        std::vector<std::vector<uint64_t>> lists(4);
        for (uint64_t a = 0; a < 9; ++a) lists[0].push_back(a);
        for (uint64_t a = 6; a < 11; ++a) lists[1].push_back(a);
        lists[2] = {23, 24, 25, 50};
        for (uint64_t a = 100; a < 140; ++a) lists[3].push_back(a);
        Segments s1 = Segments::from_lists(sys, lists);
        Segments s2 = Segments::from_labels(sys, labels, "rng");
        Segments s3 = Segments::from_molecules(sys);
        CHECK(s1.size() == 4 && s3.size() == N / 3);
        // the two-call protocol of atoms(): the size first, then the list
        auto dump_parts = [&](const Segments &s, const std::string &name) {
            const auto sizes = s.sizes();
            CHECK(sizes.size() == s.size());
            std::vector<uint64_t> flat;
            for (uint64_t k = 0; k < s.size(); ++k) { const auto a = s.atoms(k); CHECK(a.size() == sizes[k]); flat.insert(flat.end(), a.begin(), a.end()); }
            dump(name + ".sizes.u64", sizes); dump(name + ".atoms.u64", flat);
        };
        dump_parts(s1, "seg1"); dump_parts(s2, "seg2"); dump_parts(s3, "seg3");
        for (uint64_t k = 0; k < 4; ++k) CHECK(s1.atoms(k) == lists[k]);
        THROWS(s1.atoms(4), e.status != GR_OK);
        // [n_frames][M][3] with failing frames in `st`
        auto c = s1.centers(0, NS, CenterKind::Pbc, true, &st);
        CHECK(c.size() == (size_t)NS * 4 * 3 && st.size() == NS && any_failed(st));
        dump("seg1.pbc_w.centers.f32", c); dump("seg1.pbc_w.status.i32", st);
        THROWS(s1.centers(0, NS, CenterKind::Pbc, true), e.kind == "GroupError" && is_first_failure(e, st));
        CHECK(s1.stat(GR_SEG_STAT_LAST_LAUNCHES) >= 1);
        try { s1.stat(99); CHECK(false); } catch (const std::invalid_argument &) {}
        c = s1.centers(0, NS, CenterKind::Naive, false, &st);                   // needs no box
        CHECK(c.size() == (size_t)NS * 4 * 3);
        dump("seg1.naive.centers.f32", c); dump("seg1.naive.status.i32", st);
        // n_frames == 1, first_slot != 0
        c = s2.get_com(2, 1);
        CHECK(c.size() == s2.size() * 3);
        dump("seg2.com_one.centers.f32", c);
        c = s2.centers(0, NS, CenterKind::Estimate, true, &st);
        CHECK(c.size() == (size_t)NS * s2.size() * 3);
        dump("seg2.est_w.centers.f32", c); dump("seg2.est_w.status.i32", st);
        // first_slot != 0, three frames
        c = s3.get_center(7, 3);
        CHECK(c.size() == 3 * s3.size() * 3);
        dump("seg3.center_tail.centers.f32", c);
        // a refused call throws although `status` is given
        st = untouched;
        THROWS(s3.centers(PAST, 2, CenterKind::Pbc, false, &st), e.status == GR_E_INVALID_ARG);
        CHECK(st == untouched);
        Segments moved(std::move(s3));
        CHECK(s3.raw() == nullptr && moved.raw() != nullptr && moved.size() == N / 3);
        CHECK(same(c, moved.get_center(7, 3)));
        THROWS(Segments::from_lists(sys, {{3, 2}}), e.status == GR_E_INVALID_ARG);
        THROWS(Segments::from_lists(sys, {{0, N}}), e.kind == "AtomError" && e.variant == "OutOfRange" && e.index == N);
        THROWS(Segments::from_labels(sys, labels, "nobody"), e.kind == "GroupError" && e.variant == "NotFound");
        try { Segments::from_labels(sys, {1, 2, 3}); CHECK(false); } catch (const std::invalid_argument &) {}
    }

    // ================================================================ Region
    {
        const std::vector<Shape> shapes = {Shape::sphere({1.5f, 1.6f, 1.4f}, 0.55f), Shape::cylinder({1.5f, 1.6f, 0.9f}, 0.5f, 1.0f, Dimension::Z)};   // two shapes
        Region rg(sys, shapes);
        // every slot, failing frames in `st`; then the two-call protocol of lists()
        auto counts = rg.select("hyd", 0, NS, {}, &st);
        CHECK(counts.size() == NS && st.size() == NS && any_failed(st));
        auto l = rg.lists();
        CHECK(l.first.size() == (size_t)NS + 1 && l.second.size() == l.first.back());
        dump("region.a_all.counts.u64", counts); dump("region.a_all.status.i32", st); dump("region.a_all.offsets.u64", l.first); dump("region.a_all.atoms.u64", l.second);
        // frame(): the first, the last, one past it
        const auto f0 = rg.frame(0), f9 = rg.frame(NS - 1);
        CHECK(f0.size() == counts[0] && f9.size() == counts[NS - 1]);
        dump("region.a_all.frame_first.u64", f0); dump("region.a_all.frame_last.u64", f9);
        try { rg.frame(NS); CHECK(false); } catch (const std::out_of_range &) {}
        // to_group: a new name, then an existing one
        CHECK(!rg.to_group(0, "picked") && sys.group_get_n_atoms("picked") == counts[0]);
        CHECK(rg.to_group(NS - 1, "picked") && sys.group_get_n_atoms("picked") == counts[NS - 1]);
        THROWS(rg.to_group(0, "pi>cked"), e.kind == "GroupError" && e.variant == "InvalidName");
        THROWS(rg.select("hyd", 0, NS), e.kind == "GroupError" && is_first_failure(e, st));
        // anchors; n_frames == 1, first_slot != 0
        counts = rg.select("rng", 2, 1, {0.05f, -0.03f, 0.02f});
        l = rg.lists();
        CHECK(counts.size() == 1 && l.first.size() == 2 && l.second.size() == counts[0]);
        dump("region.a_one.counts.u64", counts); dump("region.a_one.offsets.u64", l.first); dump("region.a_one.atoms.u64", l.second);
        // one anchor per frame, first_slot != 0
        const std::vector<float> anchors = {0.1f, 0.0f, -0.05f, -0.07f, 0.04f, 0.0f, 0.0f, -0.11f, 0.06f};
        counts = rg.select("hyd", 7, 3, anchors, &st);
        l = rg.lists();
        CHECK(counts.size() == 3 && st.size() == 3 && l.first.size() == 4 && l.second.size() == l.first.back());
        dump("region.a_anch.counts.u64", counts); dump("region.a_anch.status.i32", st); dump("region.a_anch.offsets.u64", l.first); dump("region.a_anch.atoms.u64", l.second);
        try { rg.select("hyd", 7, 3, {0.1f, 0.0f}); CHECK(false); } catch (const std::invalid_argument &) {}
        // refused calls throw although `status` is given; the last selection is gone or kept, but lists() never lies about its size
        st = untouched;
        THROWS(rg.select("hyd", PAST, 2, {}, &st), e.status == GR_E_INVALID_ARG);
        THROWS(rg.select("nobody", 0, 3, {}, &st), e.kind == "GroupError" && e.variant == "NotFound");
        CHECK(st == untouched);
        l = rg.lists();
        CHECK(l.first.size() >= 1 && l.second.size() == l.first.back());
        Region moved(std::move(rg));
        CHECK(rg.raw() == nullptr && moved.raw() != nullptr);
        {
            std::vector<int> st2;
            CHECK(same(counts, moved.select("hyd", 7, 3, anchors, &st2)));
            CHECK(same(load<uint64_t>(out_dir + "/region.a_anch.atoms.u64"), moved.lists().second));
            // set_piece_frames cuts the call into pieces and never changes the result
            moved.set_piece_frames(1);
            CHECK(same(counts, moved.select("hyd", 7, 3, anchors, &st2)));
            CHECK(same(load<uint64_t>(out_dir + "/region.a_anch.atoms.u64"), moved.lists().second));
            CHECK(moved.stat(GR_RG_STAT_LAST_PIECES) == 3 && moved.stat(GR_RG_STAT_LAST_TOTAL) == moved.lists().first.back());
            try { moved.stat(99); CHECK(false); } catch (const std::invalid_argument &) {}
            moved.set_piece_frames(0);
        }
        // shapes that hold no atom, "" = all atoms: total == 0, atoms.data() of an empty vector
        Region empty(sys, {Shape::sphere({0.3f, 0.3f, 0.3f}, 0.1f)});
        counts = empty.select("", 0, 3);
        l = empty.lists();
        CHECK(counts.size() == 3 && l.first.size() == 4 && l.second.empty() && empty.frame(2).empty());
        dump("region.empty.counts.u64", counts); dump("region.empty.offsets.u64", l.first); dump("region.empty.atoms.u64", l.second);
    }

    // ================================================================ Contacts
    {
        Contacts ct(sys, "rng", "hyd", 0.25f);
        CHECK(ct.n1() == n_rng && ct.n2() == n_hyd && n_rng != n_hyd);
        // every slot, failing frames in `st`; then the two-call protocol of lists(), whose buffers are padded by one
        auto n = ct.pairs(0, NS, UINT64_MAX, &st);
        CHECK(n.size() == NS && st.size() == NS && any_failed(st));
        auto l = ct.lists();
        CHECK(l.offsets.size() == (size_t)NS + 1 && l.i.size() == l.offsets.back() && l.j.size() == l.i.size() && l.d.size() == l.i.size());
        dump("contacts.all.n.u64", n); dump("contacts.all.status.i32", st); dump("contacts.all.offsets.u64", l.offsets);
        dump("contacts.all.i.u32", l.i); dump("contacts.all.j.u32", l.j); dump("contacts.all.d.f32", l.d);
        THROWS(ct.pairs(0, NS), e.kind == "GroupError" && is_first_failure(e, st));
        // per_atom[f * n1 + k] and its sums
        std::vector<uint64_t> np;
        auto per_atom = ct.counts(0, NS, &np, &st);
        CHECK(per_atom.size() == (size_t)NS * ct.n1() && np.size() == NS && st.size() == NS);
        dump("contacts.counts.per_atom.u32", per_atom); dump("contacts.counts.n.u64", np); dump("contacts.counts.status.i32", st);
        THROWS(ct.counts(0, NS), is_first_failure(e, st));
        // hist[f * nbins + b], nbins with no relation to anything
        auto h = ct.hist(0, NS, 13, &st);
        CHECK(h.size() == (size_t)NS * 13 && st.size() == NS);
        dump("contacts.hist.hist.u64", h); dump("contacts.hist.status.i32", st);
        THROWS(ct.hist(0, NS, 13), is_first_failure(e, st));
        // n_frames == 1, first_slot != 0
        n = ct.pairs(5, 1);
        l = ct.lists();
        CHECK(n.size() == 1 && l.offsets.size() == 2 && l.i.size() == n[0]);
        dump("contacts.one.n.u64", n); dump("contacts.one.i.u32", l.i); dump("contacts.one.j.u32", l.j); dump("contacts.one.d.f32", l.d);
        per_atom = ct.counts(7, 3);
        CHECK(per_atom.size() == 3 * ct.n1());
        dump("contacts.counts_tail.per_atom.u32", per_atom);
        h = ct.hist(8, 1, 5);
        CHECK(h.size() == 5);
        dump("contacts.hist_one.hist.u64", h);
        // max_pairs below the total: the call only counts, and lists() has nothing to give
        n = ct.pairs(0, 3, 5, &st);
        CHECK(n.size() == 3 && n[0] + n[1] + n[2] > 5);
        dump("contacts.count_only.n.u64", n);
        THROWS(ct.lists(), e.status == GR_E_INVALID_ARG);
        // refused calls throw although `status` is given
        st = untouched;
        THROWS(ct.pairs(PAST, 2, UINT64_MAX, &st), e.status == GR_E_INVALID_ARG);
        THROWS(ct.counts(PAST, 2, nullptr, &st), e.status == GR_E_INVALID_ARG);
        THROWS(ct.hist(PAST, 2, 13, &st), e.status == GR_E_INVALID_ARG);
        THROWS(ct.hist(0, 2, 0, &st), e.status == GR_E_INVALID_ARG);
        CHECK(st == untouched);
        Contacts moved(std::move(ct));
        CHECK(ct.raw() == nullptr && moved.raw() != nullptr && moved.n1() == n_rng && moved.n2() == n_hyd);
        moved.pairs(5, 1);
        CHECK(same(l.d, moved.lists().d) && same(l.i, moved.lists().i));
        // set_piece_frames / set_walk_groups shape the launches and never change the result
        moved.set_piece_frames(1); moved.set_walk_groups(1);
        {
            const auto np3 = moved.pairs(7, 3);
            CHECK(np3.size() == 3 && moved.stat(GR_CT_STAT_LAST_TOTAL) == np3[0] + np3[1] + np3[2] && moved.stat(GR_CT_STAT_LAST_PIECES) == 3);
            CHECK(moved.stat(GR_CT_STAT_LAST_WALK_GROUPS) == 1);
            CHECK(same(per_atom, moved.counts(7, 3)));
            try { moved.stat(99); CHECK(false); } catch (const std::invalid_argument &) {}
        }
        moved.set_piece_frames(0); moved.set_walk_groups(0);
        // a cut-off below the smallest distance: total == 0
        Contacts none(sys, "oxy", "oxy", 0.05f);
        n = none.pairs(0, 3);
        l = none.lists();
        CHECK(n.size() == 3 && l.offsets.size() == 4 && l.i.empty() && l.j.empty() && l.d.empty());
        dump("contacts.none.n.u64", n); dump("contacts.none.offsets.u64", l.offsets);
        THROWS(Contacts(sys, "rng", "nobody", 0.25f), e.kind == "GroupError" && e.variant == "NotFound");
    }

    // ================================================================ RmsdPanel
    {
        RmsdPanel rows(sys, "rng", NS), cols(sys, "rng", 4);           // panels of 10 and 4 frames
        CHECK(rows.n_atoms() == n_rng && rows.frames() == 0 && rows.status().empty());
        rows.append(0, NS, &st);                                         // failing frames take their rows
        CHECK(st.size() == NS && any_failed(st) && rows.frames() == NS);
        dump("rmsd.rows.append.i32", st);
        auto s = rows.status();
        CHECK(s.size() == NS && s == st);
        dump("rmsd.rows.status.i32", s);
        cols.append(7, 3);                                               // first_slot != 0
        cols.append(2, 1);                                               // n_frames == 1
        CHECK(cols.frames() == 4);
        dump("rmsd.cols.status.i32", cols.status());
        auto m = rows.matrix();
        CHECK(m.size() == (size_t)NS * NS);
        dump("rmsd.self.matrix.f32", m);
        m = rows.matrix(cols);                                           // m[i * cols.frames() + j]
        CHECK(m.size() == (size_t)NS * 4);
        dump("rmsd.rows_cols.matrix.f32", m);
        m = cols.matrix(rows);
        CHECK(m.size() == (size_t)4 * NS);
        dump("rmsd.cols_rows.matrix.f32", m);
        RmsdPanel moved(std::move(cols));
        CHECK(cols.raw() == nullptr && moved.raw() != nullptr && moved.frames() == 4);
        CHECK(same(m, moved.matrix(rows)));
        // the matrix left on the device, and the host form cut into column blocks: the same bits
        {
            uint32_t nr = 0, nc = 0;
            float *dev = moved.matrix_device(&rows, &nr, &nc);
            CHECK(dev != nullptr && nr == 4 && nc == NS);
            std::vector<float> host((size_t)nr * nc);
            CHECK(gr_device_read(sys.raw(), dev, host.data(), host.size() * sizeof(float)) == GR_OK && same(m, host));
            dev = rows.matrix_device(nullptr, &nr, &nc);
            CHECK(dev != nullptr && nr == NS && nc == NS);
            host.assign((size_t)nr * nc, 0.0f);
            CHECK(gr_device_read(sys.raw(), dev, host.data(), host.size() * sizeof(float)) == GR_OK && same(load<float>(out_dir + "/rmsd.self.matrix.f32"), host));
            moved.set_block_entries(8);
            CHECK(same(m, moved.matrix(rows)));
            moved.set_block_entries(0);
        }
        // without `status` the first failure is thrown
        RmsdPanel thrower(sys, "rng", NS);
        THROWS(thrower.append(0, NS), e.kind == "RMSDError" && is_first_failure(e, st));
        // a refused call throws although `status` is given, and appends nothing
        const uint32_t before = rows.frames();
        rows.clear();
        CHECK(rows.frames() == 0 && before == NS);
        st = untouched;
        THROWS(rows.append(PAST, 2, &st), e.status == GR_E_INVALID_ARG);
        CHECK(st == untouched && rows.frames() == 0);
        THROWS(RmsdPanel(sys, "nobody", 4), e.kind == "RMSDError" && e.variant == "NonexistentGroup");
    }

    // ================================================================ Fluctuations
    {
        auto read_out = [&](Fluctuations &f, const std::string &name) {
            const auto mean = f.mean(); const auto var = f.variance(); const auto rmsf = f.rmsf(); const auto raw = f.raw();
            const size_t S = f.n_atoms();
            CHECK(mean.size() == 3 * S && var.size() == 3 * S && rmsf.size() == S && raw.origin.size() == 3 * S && raw.sum.size() == 3 * S && raw.sumsq.size() == 3 * S);
            CHECK(raw.n == f.frames());
            dump(name + ".mean.f64", mean); dump(name + ".variance.f64", var); dump(name + ".rmsf.f64", rmsf);
            dump(name + ".origin.f32", raw.origin); dump(name + ".sum.f64", raw.sum); dump(name + ".sumsq.f64", raw.sumsq); dump(name + ".n.u64", std::vector<uint64_t>{raw.n});
        };
        Fluctuations fl(sys, "rng"), part(sys, "rng");
        CHECK(fl.n_atoms() == n_rng && fl.frames() == 0 && fl.raw_handle() != nullptr);
        fl.accumulate(0, NS, &st);                                       // the frame without a position fails, the one without a box counts
        CHECK(st.size() == NS && any_failed(st) && fl.frames() == NS - 1);
        dump("fluct.all.status.i32", st);
        read_out(fl, "fluct.all");
        part.accumulate(7, 3);                                           // first_slot != 0
        part.accumulate(2, 1);                                           // n_frames == 1
        read_out(part, "fluct.part");
        fl.merge(part);
        CHECK(fl.frames() == NS - 1 + 4);
        read_out(fl, "fluct.merged");
        fl.store_mean(one, 0);                                           // into the group's atoms of the one-slot System
        const auto stored = one.get_positions(0);
        CHECK(stored.size() == 3 * N);
        dump("fluct.merged.stored.f32", stored);
        // set_launch cuts the group into ranges and never changes the result
        {
            Fluctuations cut(sys, "rng");
            std::vector<int> st2;
            cut.set_launch(3, 1);
            cut.accumulate(0, NS, &st2);
            CHECK(st2 == st && same(load<double>(out_dir + "/fluct.all.sumsq.f64"), cut.raw().sumsq) && cut.stat(GR_FL_STAT_LAUNCHES) >= 1);
            try { cut.stat(99); CHECK(false); } catch (const std::invalid_argument &) {}
        }
        Fluctuations thrower(sys, "rng");
        THROWS(thrower.accumulate(0, NS), e.kind == "GroupError" && is_first_failure(e, st));
        st = untouched;
        THROWS(fl.accumulate(PAST, 2, &st), e.status == GR_E_INVALID_ARG);
        CHECK(st == untouched && fl.frames() == NS - 1 + 4);
        Fluctuations moved(std::move(fl));
        CHECK(fl.raw_handle() == nullptr && moved.raw_handle() != nullptr && moved.frames() == NS - 1 + 4);
        CHECK(same(load<double>(out_dir + "/fluct.merged.rmsf.f64"), moved.rmsf()));
        moved.clear();
        CHECK(moved.frames() == 0);
        read_out(moved, "fluct.cleared");
        THROWS(Fluctuations(sys, "nobody"), e.kind == "GroupError" && e.variant == "NotFound");
    }

    // ================================================================ Covariance
    {
        auto read_out = [&](Covariance &c, const std::string &name) {
            const auto mean = c.mean(); const auto cov = c.matrix(false); const auto covw = c.matrix(true); const auto corr = c.dccm(); const auto raw = c.raw();
            const size_t S = c.n_atoms(), D = 3 * S;
            CHECK(mean.size() == D && cov.size() == D * D && covw.size() == D * D && corr.size() == S * S);
            CHECK(raw.origin.size() == D && raw.sum.size() == D && raw.Q.size() == D * D && raw.n == c.frames());
            dump(name + ".mean.f64", mean); dump(name + ".cov.f64", cov); dump(name + ".cov_mw.f64", covw); dump(name + ".dccm.f64", corr);
            dump(name + ".origin.f32", raw.origin); dump(name + ".sum.f64", raw.sum); dump(name + ".Q.f64", raw.Q); dump(name + ".n.u64", std::vector<uint64_t>{raw.n});
        };
        Covariance cv(sys, "lst"), part(sys, "lst");                      // 3 S + 1 = 124 rows: Q spans more than one 64-row block
        CHECK(cv.n_atoms() == n_lst && 3 * n_lst + 1 > 64 && cv.frames() == 0 && cv.raw_handle() != nullptr);
        cv.accumulate(0, NS, &st);
        CHECK(st.size() == NS && any_failed(st) && cv.frames() == NS - 1);
        dump("covar.all.status.i32", st);
        read_out(cv, "covar.all");
        part.accumulate(7, 3);                                           // first_slot != 0
        part.accumulate(2, 1);                                           // n_frames == 1
        read_out(part, "covar.part");
        cv.merge(part);
        CHECK(cv.frames() == NS - 1 + 4);
        read_out(cv, "covar.merged");
        // set_launch caps the grid of the product and never changes the result
        {
            Covariance capped(sys, "lst");
            std::vector<int> st2;
            capped.set_launch(1, 1);
            capped.accumulate(0, NS, &st2);
            CHECK(st2 == st && same(load<double>(out_dir + "/covar.all.Q.f64"), capped.raw().Q) && capped.stat(GR_CV_STAT_LAST_PRODUCT_GROUPS) == 1);
            try { capped.stat(99); CHECK(false); } catch (const std::invalid_argument &) {}
        }
        Covariance thrower(sys, "lst");
        THROWS(thrower.accumulate(0, NS), e.kind == "GroupError" && is_first_failure(e, st));
        st = untouched;
        THROWS(cv.accumulate(PAST, 2, &st), e.status == GR_E_INVALID_ARG);
        CHECK(st == untouched && cv.frames() == NS - 1 + 4);
        Covariance moved(std::move(cv));
        CHECK(cv.raw_handle() == nullptr && moved.raw_handle() != nullptr && moved.frames() == NS - 1 + 4);
        CHECK(same(load<double>(out_dir + "/covar.merged.dccm.f64"), moved.dccm()));
        moved.clear();
        CHECK(moved.frames() == 0);
        read_out(moved, "covar.cleared");
        THROWS(Covariance(sys, "nobody"), e.kind == "GroupError" && e.variant == "NotFound");
    }
}

// An exception nobody expected ends the program where it was thrown: no handler, so no stack is unwound and no destructor
// touches the device after it.
[[noreturn]] static void on_uncaught() {
    try {
        if (std::exception_ptr p = std::current_exception()) std::rethrow_exception(p);
    } catch (const Error &e) {
        hip_stop(e);
        printf("FAIL unexpected groan::Error %s (status %d)\n", e.what(), e.status);
    } catch (const std::exception &e) {
        printf("FAIL unexpected exception %s\n", e.what());
    } catch (...) {
        printf("FAIL unexpected exception\n");
    }
    fflush(stdout);
    std::_Exit(1);
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: test_objects <fixture dir> <output dir>\n"); return 2; }
    out_dir = argv[2];
    std::set_terminate(on_uncaught);
    run(argv[1]);
    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("all passed\n");
    return 0;
}

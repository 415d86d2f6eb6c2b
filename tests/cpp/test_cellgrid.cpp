// Host scan of the cell grid's geometry (groan_rs_amd/csrc/gr_cellgrid.h: gr_cellgrid_make, gr_cg_cell_of) for the one property that
// makes the grid a pruning device and nothing else: two positions whose distance -- gr_distance<4, true>(a, p, 7, box), the call of every
// kernel that walks the grid -- is within the cut-off have cell indices that differ by at most 1 modulo nc, on every axis.
//
// Orthorhombic boxes.  Cubes of edge L, the two positions differ along one axis (x, y and z by turns) and are 1 nm up the other two.
//   box lengths   cs k and the next floats above it for k = 3 .. 1024 (every step of floor(L / cs)), k beyond 1024 (the clamp), ordinary
//                 lengths, and the three boxes in which the rule `cell >= 1.00001 x cutoff` was first predicted to fail
//   coordinates   at every cell border m: the lowest float binned to cell m, the highest binned below it, three floats to either side
//                 of each; those values moved by -L, +L, -2 L and +17 L (one rounded sum: the wrap does not bring them back to where they
//                 came from; +17 L is beyond GR_LOOP_TURNS and takes the closed form)
//   pairs         every value at border m with every value at border m - 1 (periodically); the distance is taken where the cells are
//                 two or more apart
// Triclinic cells (the five of test_pairs_within_in_non_orthogonal_boxes, and each grown to where a direction gains a slab): the same walk
// along each lattice direction and along the normal of its slabs (the shortest way across) in fractional steps of 2^-24, the images
// whole lattice vectors away, the comparison against an fp64 minimum image over lattice images; the property is asked of pairs closer than the
// cut-off minus 2e-6 nm, the margin that test grants a borderline pair.
//
// The scan runs twice: with gr_cellgrid_make, which must give no violating pair, and with `bare`, the rule restated here that makes a
// cell 1.00001 x cutoff thick and no more -- the control, which must give some (a scan that cannot fail proves nothing).  The control
// walks every 16th step of floor(L / cs), all of them with --full-control.
//   test_cellgrid            the scan; one line per cut-off and family of boxes, every box (on one thread) with -v
//   test_cellgrid --dump     cells of a few thousand (L, cutoff, x) triples as hex words, for tests/cellgrid_ref.py
//   test_cellgrid --cells    cells per axis of the benchmark's cell with the control's rule and with gr_cellgrid_make
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <random>
#include <thread>
#include <vector>
#include "../../groan_rs_amd/csrc/gr_cellgrid.h"

typedef GrCellGrid (*MakeFn)(const GrBox &, float);

// the control: a cell 1.00001 x cutoff thick, whatever the box
static GrCellGrid bare(const GrBox &b, float cutoff) {
    GrCellGrid g = gr_cellgrid_make(b, cutoff);
    const float cs = cutoff * 1.00001f;
    double h[3] = { b.ax, b.by, b.cz };
    if (g.tric) {
        const double ax = b.ax, bx = b.bx, by = b.by, cx = b.cx, cy = b.cy, cz = b.cz, V = ax * by * cz;
        h[0] = V / sqrt(by * cz * by * cz + bx * cz * bx * cz + (bx * cy - by * cx) * (bx * cy - by * cx));
        h[1] = V / (ax * sqrt(cz * cz + cy * cy));
    }
    g.ncells = 1;
    for (int a = 0; a < 3; ++a) {
        float n = floorf((float)h[a] / cs);
        if (!(n >= 1.0f)) n = 1.0f;
        if (n > 1024.0f) n = 1024.0f;
        g.nc[a] = (uint32_t)n;
        g.inv_cell[a] = g.tric ? (float)g.nc[a] : (float)g.nc[a] / (float)h[a];
        g.ncells *= g.nc[a];
    }
    return g;
}

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float step(float v, int n) {            // n floats up (down when negative)
    for (; n > 0; --n) v = std::nextafterf(v, INFINITY);
    for (; n < 0; ++n) v = std::nextafterf(v, -INFINITY);
    return v;
}
static GrBox cube(float L) { const float b9[9] = { L, L, L, 0, 0, 0, 0, 0, 0 }; GrBox b; gr_box_setup(b9, &b); return b; }

struct Tally {
    long boxes = 0, pairs = 0, far = 0, bad = 0;     // pairs looked at, pairs two cells apart, those within the cut-off
    double margin = 1e30;                            // smallest d - cutoff among the pairs two cells apart
    void add(const Tally &o) { boxes += o.boxes; pairs += o.pairs; far += o.far; bad += o.bad; margin = std::min(margin, o.margin); }
};
static bool verbose = false;

static uint32_t cell_on(float v, int axis, const GrBox &box, const GrCellGrid &g) {
    float p[3] = { 1.0f, 1.0f, 1.0f };
    p[axis] = v;
    uint32_t c[3];
    gr_cg_cell_of(p[0], p[1], p[2], box, g, c);
    return c[axis];
}
static bool two_apart(uint32_t a, uint32_t b, uint32_t nc) {
    const uint32_t d = (a + nc - b) % nc;
    return nc > 2u && d != 0u && d != 1u && d != nc - 1u;
}
static float dist_on(float a, float p, int axis, const GrBox &box) {
    float A[3] = { 1.0f, 1.0f, 1.0f }, P[3] = { 1.0f, 1.0f, 1.0f };
    A[axis] = a; P[axis] = p;
    return gr_distance<4, true>(A[0], A[1], A[2], P[0], P[1], P[2], 7, box);
}

struct Cand { float v; uint32_t cell; };

// the candidates at border m of the axis: m = 0 .. nc - 1, border 0 is both faces of the box
static void border_candidates(uint32_t m, int axis, float L, const GrBox &box, const GrCellGrid &g, std::vector<Cand> &out) {
    out.clear();
    const uint32_t nc = g.nc[axis];
    float base[2]; int nbase = 1;
    if (m == 0u) { base[0] = 0.0f; base[1] = L; nbase = 2; }
    else {
        // the lowest float of [0, L) binned to cell m: from the border's fp64 position, walked to the step
        float w = (float)((double)m * (double)L / (double)nc);
        for (int it = 0; it < 64 && w > 0.0f && cell_on(std::nextafterf(w, 0.0f), axis, box, g) >= m; ++it) w = std::nextafterf(w, 0.0f);
        for (int it = 0; it < 64 && w < L && cell_on(w, axis, box, g) < m; ++it) w = std::nextafterf(w, INFINITY);
        base[0] = w;
    }
    auto push = [&](float v) {
        for (const Cand &c : out) if (bits(c.v) == bits(v)) return;
        out.push_back({ v, cell_on(v, axis, box, g) });
    };
    static const float turns[4] = { -1.0f, 1.0f, -2.0f, 17.0f };
    for (int q = 0; q < nbase; ++q)
        for (int s = -4; s <= 3; ++s) {                            // the highest float below the step is base - 1: three around each
            const float v = step(base[q], s);
            push(v);
            for (float t : turns) push(v + t * L);
        }
}

static Tally scan_cube(MakeFn make, float L, float cutoff, int axis) {
    Tally t; t.boxes = 1;
    const GrBox box = cube(L);
    const GrCellGrid g = make(box, cutoff);
    const uint32_t nc = g.nc[axis];
    if (nc <= 2u) return t;
    std::vector<Cand> first, prev, cur;
    border_candidates(0u, axis, L, box, g, first);
    prev = first;
    for (uint32_t m = 1; m <= nc; ++m) {
        if (m < nc) border_candidates(m, axis, L, box, g, cur); else cur = first;
        for (const Cand &a : prev)
            for (const Cand &p : cur) {
                ++t.pairs;
                if (!two_apart(a.cell, p.cell, nc)) continue;
                ++t.far;
                const float d = dist_on(a.v, p.v, axis, box);
                t.margin = std::min(t.margin, (double)d - (double)cutoff);
                if (d <= cutoff && t.bad++ < 2 && verbose)
                    printf("    L=%.9g cutoff=%.9g axis %d: %.9g (cell %u) and %.9g (cell %u) of %u, d=%.9g\n", L, cutoff, axis, a.v, a.cell, p.v, p.cell, nc, d);
            }
        prev.swap(cur);
    }
    if (verbose) printf("  cutoff %.9g L %.9g cells %u: margin %.3e, %ld pairs two cells apart, %ld within the cut-off\n", cutoff, L, nc, t.margin, t.far, t.bad);
    return t;
}

// one named pair of the table: the cells, the distance, and whether it breaks the property
static int named_pair(MakeFn make, float cutoff, float L, float xi, float xj) {
    const GrBox box = cube(L);
    const GrCellGrid g = make(box, cutoff);
    const uint32_t ci = cell_on(xi, 0, box, g), cj = cell_on(xj, 0, box, g);
    const float d = dist_on(xj, xi, 0, box);
    const bool broken = d <= cutoff && two_apart(ci, cj, g.nc[0]);
    printf("  cutoff %.9g L %.9g x_i %.9g x_j %.9g: d %.9g, cells %u and %u of %u%s\n", cutoff, L, xi, xj, d, ci, cj, g.nc[0], broken ? "  <- within the cut-off, two cells apart" : "");
    return broken ? 1 : 0;
}

// ------------------------------------------------------------------ triclinic
static void lengths_angles(const double l[3], const double a_deg[3], float box9[9]) {   // simbox.rs:96-123
    const double d2r = M_PI / 180.0, al = a_deg[0] * d2r, be = a_deg[1] * d2r, ga = a_deg[2] * d2r;
    const double ax = l[0], bx = l[1] * cos(ga), by = l[1] * sin(ga), cx = l[2] * cos(be), cy = l[2] * (cos(al) - cos(be) * cos(ga)) / sin(ga);
    const double cz = sqrt(l[2] * l[2] - cx * cx - cy * cy);
    const float v[9] = { (float)ax, (float)by, (float)cz, 0, 0, (float)bx, 0, (float)cx, (float)cy };
    memcpy(box9, v, sizeof v);
}

struct P3 { float x, y, z; uint32_t c[3]; };

// fp64 minimum image: the difference reduced in fractional coordinates, then 7 x 7 x 7 lattice images around it
static double min_image64(const P3 &a, const P3 &p, const GrBox &b) {
    const double lat[3][3] = { { b.ax, 0, 0 }, { b.bx, b.by, 0 }, { b.cx, b.cy, b.cz } };
    double d[3] = { (double)a.x - p.x, (double)a.y - p.y, (double)a.z - p.z };
    const double fc = d[2] / lat[2][2], kc = std::nearbyint(fc);
    for (int q = 0; q < 3; ++q) d[q] -= kc * lat[2][q];
    const double kb = std::nearbyint(d[1] / lat[1][1]);
    for (int q = 0; q < 3; ++q) d[q] -= kb * lat[1][q];
    d[0] -= std::nearbyint(d[0] / lat[0][0]) * lat[0][0];
    double best = 1e300;
    for (int i = -3; i <= 3; ++i) for (int j = -3; j <= 3; ++j) for (int k = -3; k <= 3; ++k) {
        const double x = d[0] + i * lat[0][0] + j * lat[1][0] + k * lat[2][0], y = d[1] + j * lat[1][1] + k * lat[2][1], z = d[2] + k * lat[2][2];
        best = std::min(best, x * x + y * y + z * z);
    }
    return sqrt(best);
}

static Tally scan_tric(MakeFn make, const float box9[9], float cutoff) {
    Tally t; t.boxes = 1;
    GrBox box;
    if (!gr_box_setup(box9, &box) || box.ortho || box.ncand > GR_MAX_CAND) { printf("  (cell refused)\n"); t.bad = 1; return t; }
    const GrCellGrid g = make(box, cutoff);
    const double lat[3][3] = { { box.ax, 0, 0 }, { box.bx, box.by, 0 }, { box.cx, box.cy, box.cz } };
    static const double turns[5] = { 0.0, -1.0, 1.0, -2.0, 17.0 };
    for (int walk = 0; walk < 6; ++walk) {          // along the lattice vector of the direction, then along the normal of its slabs
        const int dir = walk % 3;
        const bool normal = walk >= 3;
        const uint32_t nc = g.nc[dir];
        if (nc <= 2u) continue;
        // the step that takes the fractional coordinate of `dir` from 0 to 1: the lattice vector, or the slab's height along its normal
        const double *u = lat[(dir + 1) % 3], *v = lat[(dir + 2) % 3];
        double nv[3] = { u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0] };
        const double n2 = nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2], vol = nv[0] * lat[dir][0] + nv[1] * lat[dir][1] + nv[2] * lat[dir][2];
        double across[3];
        for (int q = 0; q < 3; ++q) across[q] = normal ? nv[q] * vol / n2 : lat[dir][q];
        auto border = [&](uint32_t m, std::vector<P3> &out) {
            out.clear();
            for (double turn : turns)
                for (int s = -6; s <= 6; ++s) {
                    double f[3] = { 0.37, 0.41, 0.29 };
                    f[dir] = turn;
                    const double t = (double)m / nc + s * 0x1p-24;
                    P3 p;
                    p.x = (float)(f[0] * lat[0][0] + f[1] * lat[1][0] + f[2] * lat[2][0] + t * across[0]);
                    p.y = (float)(f[1] * lat[1][1] + f[2] * lat[2][1] + t * across[1]);
                    p.z = (float)(f[2] * lat[2][2] + t * across[2]);
                    gr_cg_cell_of(p.x, p.y, p.z, box, g, p.c);
                    out.push_back(p);
                }
        };
        std::vector<P3> first, prev, cur;
        border(0u, first);
        prev = first;
        for (uint32_t m = 1; m <= nc; ++m) {
            if (m < nc) border(m, cur); else cur = first;
            for (const P3 &a : prev)
                for (const P3 &p : cur) {
                    ++t.pairs;
                    if (!two_apart(a.c[0], p.c[0], g.nc[0]) && !two_apart(a.c[1], p.c[1], g.nc[1]) && !two_apart(a.c[2], p.c[2], g.nc[2])) continue;
                    ++t.far;
                    const double d = min_image64(a, p, box);
                    t.margin = std::min(t.margin, d - (double)cutoff);
                    if (d < (double)cutoff - 2e-6) ++t.bad;
                }
            prev.swap(cur);
        }
    }
    return t;
}

// ------------------------------------------------------------------ the scan
static const float CUTOFFS[] = { 0.25f, 0.6f, 1.2f };
struct Named { float cutoff, L, xi, xj; };
static const Named NAMED[] = { { 0.25f, 41.25042f, -9.000093f, 32.000324f }, { 0.25f, 50.00051f, -7.500078f, 42.25043f }, { 1.0f, 282.00284f, -51.000526f, 230.0023f } };

static void report(const char *family, float cutoff, const Tally &t) {
    printf("cutoff %.9g %-28s %6ld boxes %10ld pairs two cells apart, margin %.3e, within the cut-off: %ld\n", cutoff, family, t.boxes, t.far, t.margin, t.bad);
}

// the lowest box length that gives k cells: cs k, where the thickness cs may itself depend on L -- looked for, not computed
static float step_length(MakeFn make, float cutoff, uint32_t k) {
    auto cells = [&](float L) { return make(cube(L), cutoff).nc[0]; };
    float lo = cutoff * (float)k, hi = lo;                                   // bare cut-off: fewer than k cells
    while (cells(hi) < k) hi *= 1.001f;
    while (bits(hi) - bits(lo) > 1u) { float mid; const uint32_t mb = bits(lo) + (bits(hi) - bits(lo)) / 2u; memcpy(&mid, &mb, 4); if (cells(mid) < k) lo = mid; else hi = mid; }
    return hi;
}

// the steps k = 3 .. 1024 (every `stride`-th), three lengths each, shared among a few threads (k by turns)
static Tally scan_steps(MakeFn make, float cutoff, uint32_t stride) {
    const unsigned nt = verbose ? 1u : std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<Tally> part(nt);
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < nt; ++w)
        pool.emplace_back([&, w] {
            for (uint32_t k = 3u + w * stride; k <= 1024u; k += nt * stride) {
                const float L = step_length(make, cutoff, k);
                for (int up = 0; up < 3; ++up) part[w].add(scan_cube(make, step(L, up), cutoff, (int)((k + up) % 3u)));
            }
        });
    for (auto &t : pool) t.join();
    Tally all;
    for (const Tally &t : part) all.add(t);
    return all;
}

static long scan(MakeFn make, const char *name, uint32_t stride) {
    printf("== %s\n", name);
    long bad = 0;
    int axis = 0;
    for (float cutoff : CUTOFFS) {
        const Tally steps = scan_steps(make, cutoff, stride);
        Tally clamp, ordinary;
        const float cs0 = cutoff * 1.00001f;
        for (float k : { 1025.0f, 1333.0f, 2048.5f, 5000.0f }) clamp.add(scan_cube(make, cs0 * k, cutoff, axis++ % 3));
        for (float L : { 2.0f, 3.3f, 6.5f, 7.25f, 10.0f, 13.37f, 17.097843f, 24.18f, 41.0f, 64.0f, 100.0f, 150.3f }) ordinary.add(scan_cube(make, L, cutoff, axis++ % 3));
        report("steps of floor(L / cs)", cutoff, steps); report("beyond the 1024 clamp", cutoff, clamp); report("ordinary lengths", cutoff, ordinary);
        bad += steps.bad + clamp.bad + ordinary.bad;
    }
    printf("the three named boxes\n");
    for (const Named &n : NAMED) {
        Tally t = scan_cube(make, n.L, n.cutoff, 0);
        report("named box", n.cutoff, t);
        bad += t.bad + named_pair(make, n.cutoff, n.L, n.xi, n.xj);
    }
    printf("triclinic cells\n");
    const double cells[5][7] = { { 7.0, 6.5, 6.0, 75.0, 80.0, 70.0, 0.45 }, { 6.0, 6.0, 6.0, 60.0, 60.0, 90.0, 0.6 }, { 6.0, 6.0, 6.0, 70.53, 109.47, 70.53, 1.3 },
                                 { 6.5, 7.5, 6.0, 100.0, 95.0, 110.0, 2.4 }, { 8.0, 7.0, 3.0, 60.0, 70.0, 80.0, 0.9 } };
    for (const auto &c : cells) {
        float b9[9];
        lengths_angles(c, c + 3, b9);
        for (float cutoff : { (float)c[6], 0.3f }) {
            Tally t = scan_tric(make, b9, cutoff);
            report("triclinic", cutoff, t);
            bad += t.bad;
        }
        // the same cell grown to where a direction gains a slab: its slabs are then as thin as the rule lets them be
        Tally grown;
        for (int dir = 0; dir < 3; ++dir) {
            auto cells_at = [&](double s, float out[9]) {
                for (int q = 0; q < 9; ++q) out[q] = (float)(b9[q] * s);
                GrBox box; gr_box_setup(out, &box);
                return make(box, (float)c[6]).nc[dir];
            };
            float g9[9];
            const uint32_t n0 = cells_at(1.0, g9);
            double lo = 1.0, hi = 1.0;
            while (cells_at(hi, g9) <= n0) hi *= 1.05;
            for (int it = 0; it < 60; ++it) { const double mid = 0.5 * (lo + hi); if (cells_at(mid, g9) <= n0) lo = mid; else hi = mid; }
            cells_at(hi, g9);
            grown.add(scan_tric(make, g9, (float)c[6]));
        }
        report("triclinic, at a step", (float)c[6], grown);
        bad += grown.bad;
    }
    printf("%s: %ld violating pairs\n", name, bad);
    return bad;
}

// cells of (L, cutoff, x) triples for the numpy restatement: hex words L cutoff x, then nc and the cell
static void dump() {
    std::mt19937_64 rng(11);
    const float Ls[] = { 0.9f, 1.6f, 2.0f, 3.3f, 7.25f, 17.097843f, 41.25042f, 50.00051f, 100.0f, 282.00284f, 400.0f };
    const float cuts[] = { 0.25f, 0.3f, 0.5f, 1.0f, 1.2f };
    for (float L : Ls)
        for (float cutoff : cuts) {
            const GrBox box = cube(L);
            const GrCellGrid g = gr_cellgrid_make(box, cutoff);
            std::vector<float> xs = { 0.0f, -0.0f, L, std::nextafterf(L, 0.0f), std::nextafterf(0.0f, -1.0f), -1e-9f, 1e-42f, -2.0f * L, 2.0f * L, 17.0f * L, -16.0f * L };
            std::uniform_real_distribution<float> near(-2.0f * L, 3.0f * L), farther(-20.0f * L, 20.0f * L);
            for (int k = 0; k < 30; ++k) xs.push_back(near(rng));
            for (int k = 0; k < 10; ++k) xs.push_back(farther(rng));
            std::uniform_int_distribution<uint32_t> border(0, g.nc[0]);
            for (int k = 0; k < 8; ++k) {
                const float w = (float)((double)border(rng) * L / g.nc[0]);
                for (int s = -2; s <= 2; ++s) { xs.push_back(step(w, s)); xs.push_back(step(w, s) - L); xs.push_back(step(w, s) + 17.0f * L); }
            }
            for (float x : xs) printf("%08x %08x %08x %u %u\n", bits(L), bits(cutoff), bits(x), g.nc[0], cell_on(x, 0, box, g));
        }
}

// the benchmark's cell (rhombic dodecahedron, d = 24.18 nm, and the per-frame variants of --box-per-frame) and the example system's box:
// cells per axis with the control's rule and with gr_cellgrid_make
static void compare_cells() {
    for (int v = -5; v <= 5; ++v) {
        const double d = 24.18 * (1.0 + 2.0e-4 * v), l[3] = { d, d, d }, ang[3] = { 60.0, 60.0, 90.0 };
        float b9[9];
        lengths_angles(l, ang, b9);
        GrBox box; gr_box_setup(b9, &box);
        for (float cutoff : { 0.25f, 0.3f, 0.35f, 0.5f, 0.6f, 0.8f, 1.0f, 1.2f }) {
            const GrCellGrid a = bare(box, cutoff), b = gr_cellgrid_make(box, cutoff);
            printf("d %.5f cutoff %.2f: %u x %u x %u -> %u x %u x %u%s\n", d, cutoff, a.nc[0], a.nc[1], a.nc[2], b.nc[0], b.nc[1], b.nc[2], a.ncells == b.ncells ? "" : "  CHANGED");
        }
    }
    for (float L : { 13.01331f, 13.01331f * 0.93f, 13.01331f * 1.08f, 11.0f })
        for (float cutoff : { 0.5f, 0.6f, 0.8f }) {
            const GrBox box = cube(L);
            printf("cube %.5f cutoff %.2f: %u -> %u%s\n", L, cutoff, bare(box, cutoff).nc[0], gr_cellgrid_make(box, cutoff).nc[0], bare(box, cutoff).nc[0] == gr_cellgrid_make(box, cutoff).nc[0] ? "" : "  CHANGED");
        }
}

int main(int argc, char **argv) {
    uint32_t control_stride = 16;                      // the control walks every 16th step: it only has to fail
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--dump")) { dump(); return 0; }
        if (!strcmp(argv[a], "--cells")) { compare_cells(); return 0; }
        if (!strcmp(argv[a], "-v")) verbose = true;
        if (!strcmp(argv[a], "--full-control")) control_stride = 1;
    }
    const long control = scan(bare, "control (a cell 1.00001 x cutoff thick)", control_stride);
    const long bad = scan(gr_cellgrid_make, "gr_cellgrid_make", 1);
    printf("control: %ld violating pairs (must be > 0); gr_cellgrid_make: %ld violating pairs\n", control, bad);
    const bool pass = bad == 0 && control > 0;
    printf("%s\n", pass ? "PASS" : "FAIL");
    return pass ? 0 : 1;
}

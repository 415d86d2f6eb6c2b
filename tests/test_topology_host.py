"""The context's bond topology (groan_rs_amd/csrc/gr_topology.h) on the CPU, against the reference's known answers.

A small C++ driver includes the header directly (it compiles without HIP) and answers line commands.  Pinned here:
  the breadth-first orders from atoms 0, 28 and 49 of conect.pdb            src/system/iterating.rs:911-958
  the molecule references [0, 5, 33] of multiple_molecules_conect.pdb      src/system/modifying.rs:980-992
  references reset by add_bond and clear_bonds                              :994-1006, :480-487
  InvalidBond before OutOfRange, duplicate bonds kept once                  :235-252
and the device map (offsets <= 0, sentinels for monoatomic atoms and pads), the whole-molecule restatement (tests/whole_ref.py)
against the reference's 3-atom cases and the oracle's wrap / vector_to, the idempotence of the library's wrap (orthorhombic and
triclinic) over the edge values tests/cpp/test_wrap.cpp walks, and that the C++ mirror of the new calls compiles."""
import os
import subprocess

import numpy as np
import pytest

import whole_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "groan_rs_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "whole_fixture.npz")

DRIVER = r"""
#include "gr_topology.h"
#include "gr_math.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
static const char *name(int st) { return st == grt::TOPO_OK ? "ok" : st == grt::TOPO_INVALID_BOND ? "invalid_bond" : "out_of_range"; }
// wrap(wrap(p)) == wrap(p) bit for bit over edge values, for one box; prints the number of failures
static int idempotence(const float box9[9]) {
    GrBox b; gr_box_setup(box9, &b);
    const float Ls[3] = { box9[0], box9[1], box9[2] };
    std::vector<float> ts = { 0.0f, -0.0f, 1e-30f, -1e-30f, 1e-7f, -1e-7f, 0.5f, -0.5f };
    for (float L : Ls) {
        float up = L, dn = L;
        for (int k = 0; k < 4; ++k) { up = std::nextafterf(up, INFINITY); dn = std::nextafterf(dn, -INFINITY); ts.push_back(up); ts.push_back(dn); }
        for (int m = -16; m <= 17; ++m) { ts.push_back((float)m * L); ts.push_back(std::nextafterf((float)m * L, INFINITY)); ts.push_back(std::nextafterf((float)m * L, -INFINITY)); ts.push_back(((float)m + 0.5f) * L); }
    }
    // every edge value in each coordinate, against every edge value of up to two turns in the other two
    std::vector<float> near;
    for (float t : ts) if (std::fabs(t) <= 2.0f * std::fmax(Ls[0], std::fmax(Ls[1], Ls[2])) + 1.0f) near.push_back(t);
    int bad = 0;
    auto one = [&](float x, float y, float z) {
        float a = x, c = y, e = z; gr_wrap(a, c, e, b);
        float a2 = a, c2 = c, e2 = e; gr_wrap(a2, c2, e2, b);
        if (memcmp(&a, &a2, 4) || memcmp(&c, &c2, 4) || memcmp(&e, &e2, 4)) ++bad;
    };
    for (float u : ts) for (float v : near) for (float w : near) { one(u, v, w); one(v, u, w); one(v, w, u); }
    return bad;
}
int main() {
    grt::GrTopology t;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op; in >> op;
        uint64_t bad = 0, which = 0;
        if (op == "n") { uint64_t n; in >> n; t = grt::GrTopology(n); std::cout << "ok\n"; }
        else if (op == "bond") { uint64_t i, j; in >> i >> j; int st = t.add_bond(i, j, &bad); std::cout << name(st) << " " << bad << "\n"; }
        else if (op == "bonds") {
            std::vector<uint64_t> a, b; uint64_t i, j;
            while (in >> i >> j) { a.push_back(i); b.push_back(j); }
            int st = t.add_bonds(a.data(), b.data(), a.size(), 1, &bad, &which);
            std::cout << name(st) << " " << bad << " " << which << "\n";
        }
        else if (op == "clear") { t.clear(); std::cout << "ok\n"; }
        else if (op == "has") { std::cout << (t.has_bonds() ? 1 : 0) << "\n"; }
        else if (op == "valid") { std::cout << (t.mol_valid ? 1 : 0) << "\n"; }
        else if (op == "degree") { uint64_t i; in >> i; std::cout << t.degree(i) << "\n"; }
        else if (op == "refs") { t.molecules(); for (uint64_t r : t.refs) std::cout << r << " "; std::cout << "\n"; }
        else if (op == "bfs") {
            uint64_t i; in >> i; std::vector<uint32_t> o;
            if (t.molecule_indices(i, o) != grt::TOPO_OK) { std::cout << "out_of_range\n"; continue; }
            for (uint32_t a : o) std::cout << a << " "; std::cout << "\n";
        }
        else if (op == "rank") { t.molecules(); for (uint32_t r : t.rank) std::cout << r << " "; std::cout << "\n"; }
        else if (op == "map") {
            uint64_t np_; in >> np_; std::vector<int32_t> m; uint64_t nf = 0; t.map(np_, m, &nf);
            std::cout << nf; for (int32_t v : m) std::cout << " " << v; std::cout << "\n";
        }
        else if (op == "idem") { float b9[9]; for (float &v : b9) in >> v; std::cout << idempotence(b9) << "\n"; }
        else { std::cout << "?\n"; }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("topo")
    src, exe = d / "topo_driver.cpp", d / "topo_driver"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*cmds):
        out = subprocess.run([str(exe)], input="\n".join(cmds) + "\n", capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    return run


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


def _bond_cmds(bonds):
    return ["bonds " + " ".join("%d %d" % (int(a), int(b)) for a, b in bonds)]


def _numbers_to_indices(fx, numbers):
    s = {int(v): k for k, v in enumerate(fx["conect_serial"])}
    return [s[v] for v in numbers]


# iterating.rs:911-958 (atom numbers; serial 10 is atom 27 in conect.pdb)
BFS_FROM_0 = [1, 2, 3, 4, 6, 5, 7, 8, 9, 10, 11, 13, 12, 14, 15, 16, 17, 18, 19, 20, 21, 24, 22, 23, 25, 26, 27, 28, 29, 30, 32, 36, 38, 42,
              48, 31, 33, 34, 35, 37, 39, 41, 45, 49, 40, 43, 46, 44, 47]
BFS_FROM_28 = [29, 28, 30, 32, 36, 38, 42, 48, 26, 31, 33, 34, 35, 37, 39, 41, 45, 49, 24, 27, 40, 43, 46, 20, 25, 44, 47, 18, 21, 16, 19, 22,
               23, 15, 17, 13, 14, 10, 8, 11, 6, 9, 12, 3, 7, 1, 4, 2, 5]


def test_fixture_integrity(fx):
    assert fx["conect_pos"].shape == (50, 3) and fx["conect_pos"].dtype == np.float32
    assert np.array_equal(fx["conect_box"], np.full(3, np.float32(60.861) / np.float32(10), np.float32))
    assert fx["conect_serial"][27] == 10 and sorted(fx["conect_serial"].tolist()) == list(range(1, 51))
    assert len(fx["whole_molecules_lines"]) == 53 and fx["whole_group_lines"][-1].split() == ["6.08610"] * 3


@pytest.mark.parametrize("start, numbers", [(0, BFS_FROM_0), (28, BFS_FROM_28), (49, [50])])
def test_bfs_orders(driver, fx, start, numbers):
    want = _numbers_to_indices(fx, numbers)
    out = driver("n 50", *_bond_cmds(fx["conect_bonds"]), "bfs %d" % start)
    assert [int(v) for v in out[-1].split()] == want
    nb = W.neighbours(50, fx["conect_bonds"])
    assert W.bfs(nb, start) == want


def test_mol_references_and_reset(driver, fx):
    out = driver("n 50", *_bond_cmds(fx["multi_bonds"]), "valid", "refs", "valid", "bond 10 15", "valid", "refs", "clear", "valid", "has", "refs")
    out = [v.strip() for v in out]
    assert out[2:5] == ["0", "0 5 33", "1"]                  # modifying.rs:980-992: references computed on first use
    assert out[5] == "ok 0" and out[6] == "0"                 # :994-1006: add_bond resets them
    assert out[7] == "0 5 33"                                 # (atoms 10 and 15 are in molecule 5 already)
    assert out[8:] == ["ok", "0", "0", ""]                    # clear_bonds: no bonds, no molecules
    refs, _ = W.molecules(W.neighbours(50, fx["multi_bonds"]))
    assert refs == [0, 5, 33]


def test_bond_errors_and_duplicates(driver):
    out = driver("n 10", "bond 3 3", "bond 12 12", "bond 12 3", "bond 3 12", "bond 1 2", "bond 2 1", "bond 1 2", "degree 1", "degree 2", "has",
                 "bonds 4 5 6 6 7 8", "degree 4", "bonds 4 5 6 20", "degree 6", "bonds 7 8 9 3", "degree 9")
    assert out[1] == "invalid_bond 3" and out[2] == "invalid_bond 12"      # i == j first, even out of range
    assert out[3] == "out_of_range 12" and out[4] == "out_of_range 12"
    assert out[5:8] == ["ok 0"] * 3 and out[8:11] == ["1", "1", "1"]       # a bond that exists is kept once
    assert out[11] == "invalid_bond 6 1" and out[12] == "0"                 # the call applies nothing
    assert out[13] == "out_of_range 20 1" and out[14] == "0"
    assert out[15] == "ok 0 0" and out[16] == "1"


def test_device_map(driver, fx):
    out = driver("n 600", "bonds 0 1 0 2 3 4 10 300 300 310 520 599 598 599", "map 768", "rank")
    vals = [int(v) for v in out[-2].split()]
    n_far, m = vals[0], np.array(vals[1:])
    assert m.shape == (768,) and n_far == 1                                   # reference 10 reaches a later tile ...
    assert m[10] == 2                                                         # ... GR_TOPO_FARREF
    assert m[0] == 0 and m[3] == 0 and m[520] == 0                            # references read in their own tile only: 0
    assert list(m[[1, 2, 4, 300, 310, 598, 599]]) == [-1, -2, -1, -290, -300, -78, -79]
    none = np.ones(768, bool); none[[0, 1, 2, 3, 4, 10, 300, 310, 520, 598, 599]] = False
    assert (m[none] == 1).all()                                               # monoatomic atoms and pads: GR_TOPO_NONE
    assert (m[~none] <= 2).all() and (m[~none][m[~none] < 1] <= 0).all()
    rank = [int(v) for v in out[-1].split()]
    assert rank[0] == 0 and rank[1] == 1 and rank[2] == 2 and rank[300] == 1 and rank[310] == 2 and rank[599] == 1 and rank[598] == 2


@pytest.mark.parametrize("box9", [
    [5.0, 5.0, 5.0, 0, 0, 0, 0, 0, 0],
    [6.0861, 6.0861, 6.0861, 0, 0, 0, 0, 0, 0],
    [7.0, 6.5, 5.5, 0, 0, 1.5, 0, -2.0, 1.25],                               # general triclinic
    [6.0, 5.656854, 4.898979, 0, 0, 2.0, 0, 2.0, 2.828427],                  # rhombic dodecahedron (xy-square)
])
def test_wrap_is_idempotent(driver, box9):
    assert driver("idem " + " ".join(repr(float(v)) for v in box9)) == ["0"]


def test_reference_three_atom_cases():
    """modifying.rs:1009-1107, exactly"""
    pos = np.array([[6, 6, 2], [1, 4, 2], [4, 1, 2]], np.float32)
    box = np.full(3, 5.0, np.float32)
    refs, orders = W.molecules(W.neighbours(3, [(0, 1), (0, 2)]))
    out, err = W.make_molecules_whole(pos, box, W.ref_of(3, refs, orders), orders)
    assert err is None and out.tolist() == [[1, 1, 2], [1, -1, 2], [-1, 1, 2]]
    refs, orders = W.molecules(W.neighbours(3, [(1, 2)]))
    out, err = W.make_molecules_whole(pos, box, W.ref_of(3, refs, orders), orders)
    assert err is None and out.tolist() == [[6, 6, 2], [1, 4, 2], [-1, 6, 2]]


def test_restatement_against_oracle():
    import oracle_lib as O
    rng = np.random.default_rng(7)
    box = np.array([4.0, 5.5, 3.25], np.float32)
    box9 = np.array([4.0, 5.5, 3.25, 0, 0, 0, 0, 0, 0], np.float32)
    pts = (rng.random((200, 3), np.float32) * 12 - 4).astype(np.float32)
    pts[:6] = [[0, 0, 0], [4.0, 5.5, 3.25], [-1e-8, 0, 0], [8.0, 11.0, 6.5], [-4.0, -5.5, -3.25], [2.0, 2.75, 1.625]]
    for a, b in zip(pts[::2], pts[1::2]):
        assert np.array_equal(W.wrap(a[None], box)[0], O.wrap(a, box9))
        assert np.array_equal(W.vector_to(a[None], b[None], box)[0], O.vector_to(a, b, box9))
    idx = np.arange(0, 200, 3)
    c = O.estimate_center(pts, idx, box9)
    got = W.make_group_whole(pts, idx, box, c)
    want = pts.copy()
    for i in idx:
        want[i] = c + O.vector_to(c, pts[i], box9)
    assert np.array_equal(got, want)


MIRROR = r"""
#include "groan_hip.hpp"
int main() {
    groan::System system(50);
    system.add_bond(0, 1);
    system.add_bonds({{1, 2}, {2, 3}});
    try { system.add_bond(4, 4); } catch (const groan::Error &e) { if (e.variant != "InvalidBond") return 1; }
    std::vector<uint64_t> refs = system.get_mol_references();
    std::vector<uint64_t> mol = system.molecule_indices(2);
    system.make_molecules_whole(0);
    std::vector<int> status;
    system.make_molecules_whole_batch(0, 4, &status);
    system.make_group_whole("all");
    system.make_group_whole_batch("all", 0, 4, &status);
    bool b = system.has_bonds();
    system.clear_bonds();
    return (int)(refs.size() + mol.size()) + (b ? 0 : 1);
}
"""


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "whole_snippet.cpp"
    src.write_text(MIRROR)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

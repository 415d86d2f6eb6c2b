"""The Segments partition (groan_rs_amd/csrc/gr_segments.h, host part) on the CPU, against the reference's known answers.

A small C++ driver includes the header directly (its first part compiles without HIP) and answers line commands.  Pinned here, as
literals, from tests/golden/example_names.npz / example.npz (the reference's test_files/example.gro):
  group_split_by_resid, Protein     29 segments, labels 1..29; residues 1, 2, 15, 29 have 1, 3, 2, 2 atoms     src/system/groups.rs:2389-2415
  group_split_by_resid, Membrane    512 segments of 12 atoms, labels 30..541                                    :2418-2439
  atoms_split_by_resname            GLY 1, LYS 12, VAL 22, LEU 2, ALA 22, CYS 2, POPC 6144, W 10399, ION 240     :2496-2519
and what follows from the specification: all atoms by resid (11 180 segments), a repeated non-adjacent label joins its first
segment, descending labels keep first-appearance order, from_molecules on the multi-molecule fixture equals the molecules of the
topology (sorted) plus singletons, every refusal of the constructors, the class counts on each class boundary; the C++ mirror compiles."""
import os
import subprocess

import numpy as np
import pytest

import whole_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "groan_rs_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
OK, INVALID_ARG, EMPTY, OUT_OF_RANGE = 0, 1, 2, 3          # grs::SEG_*

DRIVER = r"""
#include "gr_segments.h"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
static void dump(int st, uint64_t bad, const grs::Partition &P) {
    printf("%d %" PRIu64 " %" PRIu64 "\n", st, bad, st ? (uint64_t)0 : P.count());
    if (st) return;
    for (uint64_t o : P.off) printf("%" PRIu64 " ", o); printf("\n");
    for (uint32_t a : P.atoms) printf("%u ", a); printf("\n");
    for (uint8_t f : P.contiguous) printf("%d ", (int)f); printf("\n");
    for (uint64_t c : P.class_count) printf("%" PRIu64 " ", c); printf("\n");
    std::vector<grs::Rec> recs; uint64_t start[grs::N_CLASSES + 1];
    P.records(recs, start);
    for (int k = 0; k <= grs::N_CLASSES; ++k) printf("%" PRIu64 " ", start[k]); printf("\n");
    for (const grs::Rec &r : recs) printf("%u %u %u ", r.begin, r.n_flag, r.ordinal); printf("\n");
}
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op; in >> op;
        grs::Partition P;
        if (op == "lists") {          // n_atoms M null_offsets null_atoms | offsets[M + 1] | atoms...
            uint64_t n, m; int no, na; in >> n >> m >> no >> na;
            std::vector<uint64_t> off(m + 1), atoms; for (auto &o : off) in >> o;
            uint64_t a; while (in >> a) atoms.push_back(a);
            atoms.push_back(0);
            uint64_t bad = 0;
            const int st = grs::from_lists(no ? nullptr : off.data(), na ? nullptr : atoms.data(), m, n, P, &bad);
            dump(st, bad, P);
        } else if (op == "labels") {  // n_atoms G (-1: no group) | labels[n_atoms] | group[G]
            uint64_t n; long long g; in >> n >> g;
            std::vector<uint64_t> lab(n), grp(g > 0 ? g : 0); for (auto &l : lab) in >> l; for (auto &a : grp) in >> a;
            grp.push_back(0);
            dump(grs::from_labels(g < 0 ? nullptr : grp.data(), g < 0 ? 0 : (uint64_t)g, n, n ? lab.data() : nullptr, P), 0, P);
        } else if (op == "mols") {    // n_atoms | pairs...
            uint64_t n, a, b, bad; in >> n;
            grt::GrTopology topo(n);
            while (in >> a >> b) topo.add_bond(a, b, &bad);
            dump(grs::from_molecules(topo, P), 0, P);
        } else if (op == "class") { uint64_t s; while (in >> s) printf("%d ", grs::team_class(s)); printf("\n"); }
        else printf("?\n");
    }
    return 0;
}
"""


class Part:
    def __init__(self, lines):
        st, bad, m = [int(v) for v in lines[0].split()]
        self.status, self.bad, self.m = st, bad, m
        if st:
            return
        self.off = [int(v) for v in lines[1].split()]
        atoms = [int(v) for v in lines[2].split()]
        self.lists = [atoms[self.off[s]:self.off[s + 1]] for s in range(m)]
        self.contiguous = [int(v) for v in lines[3].split()]
        self.classes = [int(v) for v in lines[4].split()]
        self.start = [int(v) for v in lines[5].split()]
        r = [int(v) for v in lines[6].split()]
        self.recs = [tuple(r[3 * k:3 * k + 3]) for k in range(m)]

    @property
    def sizes(self):
        return [len(a) for a in self.lists]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("segments")
    src, exe = d / "seg_driver.cpp", d / "seg_driver"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-misleading-indentation", "-I" + CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(cmd, raw=False):
        out = subprocess.run([str(exe)], input=cmd + "\n", capture_output=True, text=True, check=True).stdout
        return out.splitlines() if raw else Part(out.splitlines())
    return run


def _labels(driver, labels, group=None):
    labels = np.asarray(labels, np.uint64)
    g = "-1" if group is None else "%d %s" % (len(group), " ".join(str(int(a)) for a in group))
    if group is None:
        return driver("labels %d -1 %s" % (len(labels), " ".join(str(int(v)) for v in labels)))
    return driver("labels %d %d %s %s" % (len(labels), len(group), " ".join(str(int(v)) for v in labels), " ".join(str(int(a)) for a in group)))


def _lists(driver, n_atoms, lists, offsets=None, null_off=False, null_atoms=False):
    off = offsets if offsets is not None else np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(int).tolist()
    flat = [int(a) for l in lists for a in l]
    return driver("lists %d %d %d %d %s %s" % (n_atoms, len(off) - 1, int(null_off), int(null_atoms), " ".join(str(o) for o in off), " ".join(str(a) for a in flat)))


def _restate(labels, group):
    """group_split_by_resid as a dict in insertion order"""
    out = {}
    for a in group:
        out.setdefault(int(labels[a]), []).append(int(a))
    return out


@pytest.fixture(scope="module")
def example():
    names = np.load(os.path.join(GOLD, "example_names.npz"))
    ex = np.load(os.path.join(GOLD, "example.npz"))

    def block(name):
        b = ex["blocks_" + name]
        return np.concatenate([np.arange(int(s), int(e) + 1) for s, e in b])
    return names["resid"], names["resname"], block


# ------------------------------------------------------------------ known answers of the reference
def test_protein_by_resid(driver, example):
    """groups.rs:2389-2415"""
    resid, _, block = example
    p = _labels(driver, resid, block("Protein"))
    assert p.status == OK and p.m == 29
    assert [int(resid[a[0]]) for a in p.lists] == list(range(1, 30))
    sizes = dict(zip(range(1, 30), p.sizes))
    assert (sizes[1], sizes[2], sizes[15], sizes[29]) == (1, 3, 2, 2)
    assert sum(p.sizes) == 61 and all(all(resid[a] == resid[l[0]] for a in l) for l in p.lists)


def test_membrane_by_resid(driver, example):
    """groups.rs:2418-2439"""
    resid, _, block = example
    p = _labels(driver, resid, block("Membrane"))
    assert p.status == OK and p.m == 512 and p.sizes == [12] * 512
    assert [int(resid[a[0]]) for a in p.lists] == list(range(30, 542))
    assert p.contiguous == [1] * 512 and p.classes == [0, 512, 0, 0]


def test_all_by_resname(driver, example):
    """groups.rs:2496-2519"""
    _, resname, _ = example
    _, first, inverse = np.unique(resname, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.uint64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    p = _labels(driver, rank[inverse])
    assert p.status == OK and p.m == 9
    got = [(resname[l[0]].decode().strip(), len(l)) for l in p.lists]
    assert got == [("GLY", 1), ("LYS", 12), ("VAL", 22), ("LEU", 2), ("ALA", 22), ("CYS", 2), ("POPC", 6144), ("W", 10399), ("ION", 240)]
    assert p.classes == [3, 1, 3, 2]           # <= 4: GLY LEU CYS; <= 16: LYS; one wave: VAL ALA ION; a workgroup: POPC W
    # residues of one name that are scattered over the protein are gather lists, a run of atoms is contiguous
    assert p.contiguous == [int(l[-1] - l[0] + 1 == len(l)) for l in p.lists] and 0 in p.contiguous and p.contiguous[7] == 1


# ------------------------------------------------------------------ what the specification says
def test_all_by_resid_equals_restatement(driver, example):
    resid, _, _ = example
    p = _labels(driver, resid)
    want = _restate(resid, range(len(resid)))
    assert p.status == OK and p.m == 11180 == len(want)
    assert p.lists == list(want.values())
    assert sum(p.classes) == 11180 and p.start == [0] + np.cumsum(p.classes).tolist()


def test_repeated_and_descending_labels(driver):
    # a label that comes back after another one joins its FIRST segment; the segments keep first-appearance order
    p = _labels(driver, [7, 7, 3, 7, 9, 3, 3, 1])
    assert p.lists == [[0, 1, 3], [2, 5, 6], [4], [7]] and p.contiguous == [0, 0, 1, 1]
    p = _labels(driver, [9, 9, 8, 5, 5, 5, 2])
    assert p.lists == [[0, 1], [2], [3, 4, 5], [6]] and p.contiguous == [1, 1, 1, 1]
    # a group: only its atoms, in index order; atoms outside belong to no segment
    p = _labels(driver, [4, 4, 4, 6, 6, 4, 4], group=[1, 2, 4, 5])
    assert p.lists == [[1, 2, 5], [4]]
    # labels beyond 32 bits
    p = _labels(driver, [2 ** 40, 5, 2 ** 40, 2 ** 63])
    assert p.lists == [[0, 2], [1], [3]]


def test_from_molecules(driver):
    fx = np.load(os.path.join(GOLD, "whole_fixture.npz"))
    bonds = fx["multi_bonds"]
    p = driver("mols 50 " + " ".join("%d %d" % (int(a), int(b)) for a, b in bonds))
    refs, orders = W.molecules(W.neighbours(50, bonds))
    inmol = set(a for o in orders for a in o)
    want = sorted([sorted(o) for o in orders] + [[a] for a in range(50) if a not in inmol])     # ordered by lowest atom
    assert p.status == OK and p.lists == want
    assert [l[0] for l in p.lists if len(l) > 1] == list(refs)
    assert sorted(a for l in p.lists for a in l) == list(range(50))                            # every atom exactly once
    # no bonds at all: every atom on its own
    p = driver("mols 5")
    assert p.lists == [[0], [1], [2], [3], [4]] and p.classes == [5, 0, 0, 0]
    # a molecule whose atoms interleave with another's
    p = driver("mols 6 0 4 1 3 3 5")
    assert p.lists == [[0, 4], [1, 3, 5], [2]] and p.contiguous == [0, 0, 1]


def test_errors(driver):
    assert _lists(driver, 10, [[1, 2]], null_off=True).status == INVALID_ARG
    assert _lists(driver, 10, [[1, 2]], null_atoms=True).status == INVALID_ARG
    assert _lists(driver, 10, []).status == EMPTY                                  # no segment
    assert _lists(driver, 10, [[1, 2], [], [3]]).status == EMPTY                   # an empty one
    assert _lists(driver, 10, [[1, 2], [3]], offsets=[0, 2, 1]).status == INVALID_ARG     # offsets that decrease
    assert _lists(driver, 10, [[1, 2, 2]]).status == INVALID_ARG                   # not strictly ascending
    assert _lists(driver, 10, [[0, 1], [5, 4]]).status == INVALID_ARG
    p = _lists(driver, 10, [[0, 1], [5, 10]])
    assert (p.status, p.bad) == (OUT_OF_RANGE, 10)
    p = _lists(driver, 10, [[0, 9], [3, 4, 5], [4, 5]])                            # overlap is allowed, and so are unassigned atoms
    assert p.status == OK and p.lists == [[0, 9], [3, 4, 5], [4, 5]] and p.contiguous == [0, 1, 1]
    p = _lists(driver, 10, [[7, 8]], offsets=[0, 2])
    assert p.status == OK and p.recs == [(7, 2 | 0x80000000, 0)]
    assert _labels(driver, [1, 2, 3], group=[]).status == EMPTY
    assert driver("labels 0 -1").status != OK


def test_class_boundaries(driver):
    sizes = [1, 4, 5, 16, 17, 4096, 4097, 3, 4, 20000, 16]
    assert [int(v) for v in driver("class " + " ".join(str(s) for s in sizes), raw=True)[0].split()] == [0, 0, 1, 1, 2, 2, 3, 0, 0, 3, 1]
    lists, a = [], 0
    for s in sizes:
        lists.append(list(range(a, a + s))); a += s
    p = _lists(driver, a, lists)
    assert p.status == OK and p.classes == [4, 3, 2, 2] and p.start == [0, 4, 7, 9, 11]
    # the records: classes one after the other, segments in order inside a class, contiguous ones carry their first atom
    assert [r[2] for r in p.recs] == [0, 1, 7, 8, 2, 3, 10, 4, 5, 6, 9]
    assert all(r[1] == (sizes[r[2]] | 0x80000000) and r[0] == lists[r[2]][0] for r in p.recs)
    # a gather list carries its offset into the flat atom list
    p = _lists(driver, 100, [[0, 1, 2], [10, 12, 14, 16, 18], [50]])
    assert p.recs == [(0, 3 | 0x80000000, 0), (50, 1 | 0x80000000, 2), (3, 5, 1)]


def test_python_mirror_and_abi():
    import groan_rs_amd as g
    lib = g._lib.load()
    assert g.Segments is g.segments.Segments
    for name in ("from_lists", "by_resid", "by_resname", "from_molecules", "centers", "get_com", "get_center", "estimate_com", "get_com_naive", "sizes", "atoms", "close"):
        assert hasattr(g.Segments, name), name
    assert lib.gr_segments_count(None) == 0
    assert lib.gr_segments_stat(None, 1, None) == g._lib.E_INVALID_ARG
    assert lib.gr_segments_center_batch(None, 0, 1, 0, 0, None, None) == g._lib.E_INVALID_ARG
    lib.gr_segments_destroy(None)


MIRROR = r"""
#include "groan_hip.hpp"
int main() {
    groan::System system(1000, 0, 4);
    groan::Segments a = groan::Segments::from_lists(system, {{0, 1, 2}, {5, 7}});
    std::vector<uint64_t> labels(1000, 1);
    groan::Segments b = groan::Segments::from_labels(system, labels);
    groan::Segments c = groan::Segments::from_labels(system, labels, "all");
    groan::Segments d = groan::Segments::from_molecules(system);
    try { groan::Segments bad = groan::Segments::from_lists(system, {{3, 2}}); } catch (const groan::Error &e) { if (e.kind != "DeviceError") return 1; }
    std::vector<int> status;
    std::vector<float> com = a.get_com(0, 4);
    std::vector<float> cen = b.get_center(0, 4, &status);
    std::vector<float> est = c.centers(0, 4, groan::CenterKind::Estimate, true, &status);
    std::vector<uint64_t> sz = d.sizes(), at = d.atoms(0);
    groan::Segments moved(std::move(a));
    return (int)(com.size() + cen.size() + est.size() + sz.size() + at.size() + moved.size() + moved.stat(GR_SEG_STAT_TEAM4));
}
"""


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "segments_snippet.cpp"
    src.write_text(MIRROR)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

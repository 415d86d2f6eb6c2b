"""Internals (gr_internals_*; groan_rs_amd.Internals): what can be checked without a device -- that the header's section is mirrored in
_lib.py (parameter counts), include/groan_hip.hpp and the Rust shim and says what the contract needs said, that the C++ mirror compiles,
that the f64 restatement the GPU tests compare with (tests/internals_ref.py) gives the reference's known answers for Vector3D::angle
and the dihedral's four pins, the bond helpers, and THE EMULATION behind the GPU tests' bounds.

THE BOUNDS (internals_ref.bounds), against the f64 restatement on the same f32 positions, with E = ulp_f32(largest |coordinate| among
the named atoms): distance 2E + 4 ulp(v); axis 2E/|d| + 4 ulp(1); angle 2E (1/|u| + 1/|v|) + 4 ulp(pi); dihedral 2E (1/rho1 + 1/rho4) +
4 ulp(pi) modulo 2 pi.  Derivation: each f32 displacement of a PBC-broken tuple is a difference of coordinates of magnitude up to the
box edge, so a component carries up to E/2 from the subtraction and as much again from the fused image shift: at most E per component
pair, 2E with both ends of a vector counted; an angle moves by (error across the vector) / (lever arm), the lever arms being |u|, |v|
or the distances rho of the end atoms from the central axis.  The 4 ulp term is the arithmetic behind the displacements (float_cmp's
default margin, which the reference's own tests use).  test_emulation_stays_inside_the_bounds runs the device's formulas in f32 numpy
on 20 000 wrapped chains per box; largest error / bound seen: orthorhombic 0.30 (distance), 0.28 (axis), 0.22 (angle), 0.29 (dihedral);
triclinic 0.51, 0.39, 0.35, 0.42."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

import internals_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_internals_accumulate_batch", "gr_internals_clear", "gr_internals_count", "gr_internals_create", "gr_internals_destroy", "gr_internals_frames",
         "gr_internals_merge", "gr_internals_read", "gr_internals_read_raw", "gr_internals_set_launch", "gr_internals_stat", "gr_internals_values_batch",
         "gr_internals_values_batch_device"]
KINDS = ("distance", "angle", "dihedral", "axis")
AXIS = (0.3, -0.2, 1.0)


def _header():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _section():
    return open(os.path.join(ROOT, "include", "groan_hip.h")).read().split("Internals: distance, angle and dihedral series")[1].split("gr_internals *gr_internals_create")[0]


def test_header_section_is_mirrored_in_lib_hpp_and_rust():
    from groan_rs_amd import _lib
    protos = {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
              for m in re.finditer(r"\b(gr_internals_[a-z_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S)}
    assert sorted(protos) == NAMES
    hpp = open(os.path.join(ROOT, "include", "groan_hip.hpp")).read()
    rs = re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "src", "groan_hip.rs")).read())
    for name, params in protos.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(params), (name, len(_lib.SIGNATURES[name][1]), len(params))
        assert re.search(r"\b%s\s*\(" % name, hpp), name
        m = re.search(r"pub\s+fn\s+%s\s*\((.*?)\)\s*(?:->[^;]*)?;" % name, rs, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if ":" in p]) == len(params), name
    assert _lib.SIGNATURES["gr_internals_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_internals_destroy"][0] is None
    assert _lib.SIGNATURES["gr_internals_count"][0] is C.c_uint64 and _lib.SIGNATURES["gr_internals_frames"][0] is C.c_uint64
    assert "class Internals" in hpp and "pub struct gr_internals" in rs


def test_kinds_flags_and_stat_keys_are_the_header_s():
    from groan_rs_amd import _lib
    h = _header()
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGR_(IC_[A-Z_]+)\s*=\s*(\d+)", h)}
    assert sorted(enums) == sorted(["IC_DISTANCE", "IC_ANGLE", "IC_DIHEDRAL", "IC_AXIS", "IC_STAT_LAUNCHES", "IC_STAT_LAST_RANGE_GROUPS", "IC_STAT_LAST_FRAME_GROUPS",
                                    "IC_STAT_LAST_CHECK_GROUPS", "IC_STAT_ARITY", "IC_STAT_UNIQUE_ATOMS", "IC_STAT_AHEAD"])
    for name, v in enums.items():
        assert getattr(_lib, name) == v, name
    assert re.search(r"#define\s+GR_IC_PBC\s+1u", h) and _lib.IC_PBC == 1
    assert re.search(r"#define\s+GR_IC_MAX_WS_BYTES\s+\(64u << 20\)", h) and _lib.IC_MAX_WS_BYTES == 64 << 20


def test_header_states_the_contract():
    s = _section()
    for words in ("gr_mag3(d(i->j))", "atan2f(|u x v|, u.v)", "b1 = d(i->j), b2 = d(j->k), b3 = d(k->l), n1 = b1 x b2, n2 = b2 x b3", "atan2f(|b2| (b1.n2), n1.n2)",
                  "(d(i->j).a) / |d(i->j)|", "0 when |d| = 0", "RADIANS", "gr_min_image_vec",
                  "l = (1,0,1) gives +pi/2", "l = (1,1,0) gives 0 (cis)", "l = (1,-1,0) gives pi (trans)", "l = (1,0,-1) gives -pi/2",
                  "ORDER OF THE SUMS", "if d > PI_F, subtract 2 PI_F; else if d < -PI_F, add 2 PI_F", "WITHIN pi OF THE ORIGIN", "NO LONGER THOSE OF ONE WALK",
                  "GR_IC_MAX_WS_BYTES", "ROW OF NaN"):
        assert words in s, words
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_internals.h")).read()
    assert re.search(r"ring\[GR_IC_AHEAD\]", src) and 2 <= R.source_ahead() <= 16
    assert '#include "gr_internals.h"' in open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_api.hip")).read()


def test_cpp_mirror_compiles_without_a_warning():
    """tests/cpp/internals_mirror.cpp calls every public method of groan::Internals"""
    src = os.path.join(ROOT, "tests", "cpp", "internals_mirror.cpp")
    hpp = open(os.path.join(ROOT, "include", "groan_hip.hpp")).read()
    cls = hpp.split("class Internals {")[1].split("  private:")[0]
    text = open(src).read()
    for name in ("values", "values_device", "accumulate", "clear", "read", "raw", "order_parameter", "merge", "set_launch", "stat", "raw_handle", "count", "frames"):
        assert re.search(r"\b%s\(" % name, cls) and re.search(r"\.%s\(" % name, text), name
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert hpp.split("class Internals {")[1].count("detail::batch_status") == 3       # a refused call throws, like the other batch objects


def test_internals_is_exported():
    import groan_rs_amd as G
    from groan_rs_amd import internals
    assert G.Internals is internals.Internals and G.angles_from_bonds is internals.angles_from_bonds and G.dihedrals_from_bonds is internals.dihedrals_from_bonds
    assert {"Internals", "angles_from_bonds", "dihedrals_from_bonds"} <= set(G.__all__)
    for method in ("values", "values_device", "accumulate", "clear", "read", "read_raw", "merge", "set_launch", "stat", "close", "order_parameter", "__enter__", "__exit__"):
        assert callable(getattr(G.Internals, method)), method
    assert isinstance(G.Internals.n_frames, property)
    assert sorted(internals.KINDS) == sorted(KINDS) and {k: v[1] for k, v in internals.KINDS.items()} == R.ARITY


def test_values_device_refuses_what_is_no_device_tensor():
    import pytest
    import torch
    import groan_rs_amd as G
    ic = G.Internals.__new__(G.Internals)
    ic.n_tuples, ic._f = 4, None
    for out in (torch.zeros((8, 4), dtype=torch.float32), torch.zeros((8, 4), dtype=torch.float64), torch.zeros((8, 3), dtype=torch.float32),
                torch.zeros((7, 4), dtype=torch.float32), torch.zeros((8, 8), dtype=torch.float32)[:, ::2], torch.zeros(32, dtype=torch.float32)):
        with pytest.raises(ValueError, match="float32 device tensor"):
            ic.values_device(out, 0, 8)
    with pytest.raises(ValueError, match="wants ld"):
        ic.values_device(4096, 0, 8)


def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "vector3d_angle.json")))


def test_restatement_gives_the_reference_s_angles_and_the_pins():
    """and so does the f32 emulation of the device's formulas, within 4 ulp_f32(pi)"""
    g = _golden()
    tol = 4 * float(R.ulp32(np.pi))
    assert len(g["cases"]) == 8
    for case in g["cases"]:
        pos = np.array([case["u"], [0, 0, 0], case["v"]], R.F)
        for v in (R.values64("angle", pos, [[0, 1, 2]])[0], float(R.values32("angle", pos, [[0, 1, 2]])[0])):
            assert abs(v - case["expected"]) <= tol, (case["name"], v)
    pins = g["dihedral_pins"]
    assert len(pins["l"]) == 4
    for l, want in zip(pins["l"], pins["expected"]):
        pos = np.array([pins["i"], pins["j"], pins["k"], l], R.F)
        for v in (R.values64("dihedral", pos, [[0, 1, 2, 3]])[0], float(R.values32("dihedral", pos, [[0, 1, 2, 3]])[0])):
            assert R.error("dihedral", v, want) <= tol, (l, v)
    # degenerate geometry: finite and in range
    pos = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], R.F)
    assert R.values32("angle", pos, [[0, 1, 2]])[0] == 0 and R.values32("axis", pos, [[0, 1]], axis=AXIS)[0] == 0
    assert abs(R.values32("dihedral", pos, [[1, 2, 3, 4]])[0]) <= np.pi


def test_minimum_image_of_the_restatement():
    """the exhaustive search against a brute-force search over 9 x 9 x 9 images, in the three cells of the GPU tests"""
    rng = np.random.default_rng(3)
    tric = np.load(os.path.join(ROOT, "tests", "golden", "tric_small.npz"))["triclinic_boxes9"][0]
    for box in (np.array([6.36432, 6.68132, 7.41583, 0, 0, 0, 0, 0, 0], R.F), tric, R.DODECAHEDRON):
        L = R.lattice(box)
        d = (rng.random((500, 3)) * 4 - 2) @ L
        got = R.min_image(d, box)
        sh = np.array([(a, b, c) for a in range(-4, 5) for b in range(-4, 5) for c in range(-4, 5)], np.float64) @ L
        brute = np.sqrt(((d[:, None, :] + sh[None]) ** 2).sum(-1)).min(1)
        assert np.abs(np.sqrt((got * got).sum(1)) - brute).max() <= 1e-12
        assert np.abs(R.min_image32(d.astype(R.F), box) - R.min_image(d.astype(R.F), box)).max() <= 1e-5


def test_generated_chains_meet_the_conditions_of_the_bounds():
    tric = np.load(os.path.join(ROOT, "tests", "golden", "tric_small.npz"))["triclinic_boxes9"][0]
    for box in (np.array([6.36432, 6.68132, 7.41583, 0, 0, 0, 0, 0, 0], R.F), tric, R.DODECAHEDRON):
        pw, pu = R.chains(500, box, 11)
        assert R.chain_ok(pw, box).all() and R.chain_ok(pu, None).all()
        # most chains are broken by the wrap, and the wrapped chain is the whole one
        shift = (pw - pu).reshape(500, 4, 3)
        broken = ((shift.max(1) - shift.min(1)).max(1) > 1.0).mean()
        assert broken > 0.5, broken
        for kind in KINDS:
            t = R.chain_tuples(kind, 500)
            # (the two copies were rounded to f32 apart: half an ulp of a coordinate per atom and component, the bounds' own measure)
            slack = R.bounds(kind, pw, t, box, AXIS) + R.bounds(kind, pu, t, None, AXIS)
            assert (R.error(kind, R.values64(kind, pw, t, box, AXIS), R.values64(kind, pu, t, None, AXIS)) <= slack).all()
        v, (r1, r4) = R.values64("dihedral", pw, R.chain_tuples("dihedral", 500), box, parts=True)
        assert min(r1.min(), r4.min()) >= 0.04
        assert R.bounds("dihedral", pw, R.chain_tuples("dihedral", 500), box).max() < 1e-3


def test_emulation_stays_inside_the_bounds():
    """the device's formulas in f32 numpy on 20 000 wrapped chains in an orthorhombic and a triclinic box, every tuple compared"""
    worst = {}
    for name, box in (("ortho", np.array([24.0, 23.0, 22.0, 0, 0, 0, 0, 0, 0], R.F)), ("tric", (R.DODECAHEDRON * R.F(3)).astype(R.F))):
        pw, pu = R.chains(20000, box, 5)
        for kind in KINDS:
            t = R.chain_tuples(kind, 20000)
            err = R.error(kind, R.values32(kind, pw, t, box, AXIS), R.values64(kind, pw, t, box, AXIS))
            bound = R.bounds(kind, pw, t, box, AXIS)
            assert bound.max() < 1e-3
            worst[name, kind] = float((err / bound).max())
            assert (err <= bound).all(), (name, kind, worst[name, kind])
    print("largest error / bound:", worst)


def test_statistics_restatement():
    rng = np.random.default_rng(9)
    rows = (rng.standard_normal((40, 7)) * 0.3 + 1.0).astype(R.F)
    rows[0] = np.nan; rows[5] = np.nan
    st = R.State("angle", 7).add(rows)
    assert st.n == 38 and R.same_bits(st.o, rows[1])
    mean, var = st.close()
    good = rows[~np.isnan(rows).all(1)].astype(np.float64)
    assert np.abs(mean - good.mean(0)).max() <= 1e-6 and np.abs(var - good.var(0)).max() <= 1e-6
    m2, v2 = st.two_pass(rows)
    assert np.abs(mean - m2).max() <= 1e-12 and np.abs(var - v2).max() <= 1e-12
    # cut into calls: the same bits
    cut = R.State("angle", 7).add(rows[:3]).add(rows[3:17]).add(rows[17:])
    assert R.same_bits(cut.s, st.s) and R.same_bits(cut.q, st.q) and R.same_bits(cut.o, st.o)
    # a torsion that alternates between +3.10 and -3.10
    tors = np.where(np.arange(30) % 2 == 0, 3.10, -3.10).astype(R.F)[:, None] + (rng.standard_normal((30, 1)) * 0.01).astype(R.F)
    d = R.State("dihedral", 1).add(tors)
    mean, var = d.close()
    assert var[0] < 0.01 and abs(mean[0]) > 3.1 and -np.pi < mean[0] <= np.pi
    plain = R.State("angle", 1).add(tors).close()
    assert plain[1][0] > 9.0                                                   # without the wrap: the variance of +-3.1


def test_bond_helpers():
    import groan_rs_amd as G
    chain = [[0, 1], [1, 2], [2, 3]]
    assert G.angles_from_bonds(chain).tolist() == [[0, 1, 2], [1, 2, 3]] and G.dihedrals_from_bonds(chain).tolist() == [[0, 1, 2, 3]]
    ring = [[k, (k + 1) % 6] for k in range(6)]
    a, d = G.angles_from_bonds(ring), G.dihedrals_from_bonds(ring)
    assert a.shape == (6, 3) and d.shape == (6, 4) and a.dtype == d.dtype == np.uint64
    assert all(i < k for i, j, k in a.tolist()) and all(j < k and i != l for i, j, k, l in d.tolist())
    assert sorted(j for i, j, k in a.tolist()) == list(range(6))
    # a branched atom: 1 bonded to 0, 2, 3 and 3 to 4 (listed twice and reversed: kept once)
    branched = [[0, 1], [2, 1], [1, 3], [3, 4], [1, 0]]
    assert G.angles_from_bonds(branched).tolist() == [[0, 1, 2], [0, 1, 3], [1, 3, 4], [2, 1, 3]]
    assert G.dihedrals_from_bonds(branched).tolist() == [[0, 1, 3, 4], [2, 1, 3, 4]]
    assert G.angles_from_bonds(np.zeros((0, 2), np.uint64)).shape == (0, 3) and G.dihedrals_from_bonds([[0, 1]]).shape == (0, 4)
    # a three-ring has no proper dihedral (i == l)
    assert G.dihedrals_from_bonds([[0, 1], [1, 2], [2, 0]]).shape == (0, 4) and G.angles_from_bonds([[0, 1], [1, 2], [2, 0]]).shape == (3, 3)

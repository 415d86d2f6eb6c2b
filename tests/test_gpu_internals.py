"""Internals over resident frames (gr_internals_*; groan_rs_amd.Internals) against the f64 restatement tests/internals_ref.py.

VALUES are held to internals_ref.bounds -- per tuple, E = ulp_f32(largest |coordinate| among the frame's named atoms): distance 2E +
4 ulp(v); axis 2E/|d| + 4 ulp(1); angle 2E (1/|u| + 1/|v|) + 4 ulp(pi); dihedral 2E (1/rho1 + 1/rho4) + 4 ulp(pi) modulo 2 pi
(tests/test_internals_host.py has the derivation and runs the device's formulas in f32 numpy against them).  EVERY tuple of every
frame is compared; the generator keeps bonds >= 0.09 nm and bond angles within 60 .. 150 degrees (rho >= 0.04 nm) and no displacement
component within 1e-3 nm of half a box edge; the largest bound stays below 1e-3.  The inputs: 300 four-atom chains, 9 in 10 laid
across a face of the cell and wrapped (so most tuples are broken), 8 frames whose boxes differ, in the orthorhombic box of the `aa`
fixture, tric_small's triclinic box and a rhombic dodecahedron; and the same chains whole, without boxes, without GR_IC_PBC.
THE STATE of accumulate (origin, sums, n) is compared bit for bit with the numpy restatement of the rows `values` returns.
Largest error / bound seen on the device (distance, angle, dihedral, axis; each test prints its own with -s): orthorhombic 0.28, 0.20,
0.25, 0.25; triclinic 0.51, 0.34, 0.36, 0.33; dodecahedron 0.48, 0.34, 0.31, 0.30; the hydrogen bonds' angles 0.58 of the angle bound."""
import json
import os

import numpy as np
import pytest

import internals_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("distance", "angle", "dihedral", "axis")
AXIS = (0.3, -0.2, 1.0)
NC, NF = 300, 8
ULP_PI4 = 4 * float(R.ulp32(np.pi))


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def cell_box(name, aa, tric_small):
    return {"ortho": aa["box9"], "tric": tric_small["triclinic_boxes9"][0], "dodeca": R.DODECAHEDRON}[name]


@pytest.fixture(scope="module", params=["ortho", "tric", "dodeca"])
def world(request, G, aa, tric_small):
    """slots 0 .. 7: wrapped chains with the frame's own box; slots 8 .. 15: the same chains whole, without a box"""
    boxes = R.frame_boxes(cell_box(request.param, aa, tric_small), NF)
    frames = [R.chains(NC, boxes[f], 100 + f) for f in range(NF)]
    s = G.System(4 * NC, n_slots=2 * NF)
    for f in range(NF):
        s.set_frame(frames[f][0], boxes[f], slot=f)
        s.set_frame(frames[f][1], None, slot=NF + f)
    yield request.param, s, boxes, frames
    s.close()


def make(G, s, kind, tuples, pbc=True):
    return G.Internals(s, kind, tuples, pbc=pbc, axis=AXIS if kind == "axis" else None)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---------------------------------------------------------------- the definitions
def test_reference_angles_and_dihedral_pins(G):
    g = json.load(open(os.path.join(GOLD, "vector3d_angle.json")))
    pins = g["dihedral_pins"]
    pos = np.array([p for c in g["cases"] for p in (c["u"], [0, 0, 0], c["v"])] + [p for l in pins["l"] for p in (pins["i"], pins["j"], pins["k"], l)], F)
    na = 3 * len(g["cases"])
    s = G.System(len(pos))
    s.set_frame(pos, None, slot=0)
    with make(G, s, "angle", np.arange(na).reshape(-1, 3), pbc=False) as ic:
        v, st = ic.values(0, 1)
        assert v.dtype == np.float32 and v.shape == (1, 8) and not st.any()
        want = np.array([c["expected"] for c in g["cases"]])
        assert (np.abs(v[0].astype(np.float64) - want) <= ULP_PI4).all(), v[0]
    with make(G, s, "dihedral", na + np.arange(16).reshape(-1, 4), pbc=False) as ic:
        v, st = ic.values(0, 1)
        assert (R.error("dihedral", v[0], np.array(pins["expected"])) <= ULP_PI4).all(), v[0]
        assert v[0][0] > 0 > v[0][3]                                                # the sign
    # degenerate geometry: finite and in range
    pos = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [1, 1, 1]], F)
    s2 = G.System(len(pos)); s2.set_frame(pos, None, slot=0)
    for kind, t in (("angle", [[0, 5, 1], [2, 3, 4]]), ("dihedral", [[1, 2, 3, 4], [0, 2, 1, 5]]), ("axis", [[0, 1]]), ("distance", [[0, 1]])):
        with make(G, s2, kind, t, pbc=False) as ic:
            v = ic.values(0, 1)[0]
            assert np.isfinite(v).all() and (np.abs(v) <= np.float32(np.pi) + 1e-6).all(), (kind, v)
    with make(G, s2, "axis", [[0, 1]], pbc=False) as ic:
        assert ic.values(0, 1)[0][0, 0] == 0                                        # |d| = 0
    s.close(); s2.close()


@pytest.mark.parametrize("kind", KINDS)
def test_values_against_the_restatement(G, world, kind):
    cell, s, boxes, frames = world
    t = R.chain_tuples(kind, NC)
    worst = 0.0
    for pbc, slot0 in ((True, 0), (False, NF)):
        with make(G, s, kind, t, pbc=pbc) as ic:
            assert ic.n_tuples == len(t) == len(ic) and ic.stat(G._lib.IC_STAT_ARITY) == R.ARITY[kind] and ic.stat(G._lib.IC_STAT_UNIQUE_ATOMS) == 4 * NC
            v, st = ic.values(slot0, NF)
            assert v.shape == (NF, len(t)) and v.dtype == np.float32 and st.dtype == np.int32 and not st.any()
            for f in range(NF):
                pos, box = (frames[f][0], boxes[f]) if pbc else (frames[f][1], None)
                bound = R.bounds(kind, pos, t, box, AXIS)
                err = R.error(kind, v[f], R.values64(kind, pos, t, box, AXIS))
                assert bound.max() < 1e-3
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (cell, kind, pbc, f, worst)
            if kind in ("angle", "dihedral"):
                assert (v >= -np.float32(np.pi)).all() and (v <= np.float32(np.pi)).all() and (kind == "dihedral" or (v >= 0).all())
    print("largest error / bound", cell, kind, round(worst, 3))


def test_hydrogen_bond_angles_and_distances(G, aa):
    """the (donor, hydrogen, acceptor) triples HBondAnalysis reports for the `aa` peptide: "angle" gives its angles x pi / 180 under
    the angle bound, "distance" (donor, acceptor) its distances within the project's 1e-5 nm"""
    import hbond_ref as H
    topo = np.load(os.path.join(GOLD, "aa_hbond_topology.npz"))
    don, hyd = H.protein_groups(topo["peptide_element"])
    frames, boxes = aa["traj_peptide"], aa["traj_boxes9"]
    nf = len(frames)
    s = G.System(frames.shape[1], n_slots=nf)
    for f in range(nf):
        s.set_frame(frames[f], boxes[f], slot=f)
    s.group_create_from_indices("NO", [int(i) for i in don]); s.group_create_from_indices("H", [int(i) for i in hyd])
    an = G.HBondAnalysis(s, [G.HBondChain("NO", "NO", "H")], [(0, 0)], 0.3, 150.0, topo["peptide_bonds"])
    res = an.batch(0, nf)
    assert (res[6] == 0).all() and len(res[0]) == 181
    worst = 0.0
    for f in range(nf):
        a, b = int(res[5][f]), int(res[5][f + 1])
        if a == b:
            continue
        tri = np.stack([res[0][a:b], res[1][a:b], res[2][a:b]], 1).astype(np.uint64)
        with make(G, s, "angle", tri) as ic:
            v = ic.values(f, 1)[0][0]
        bound = R.bounds("angle", frames[f], tri, boxes[f])
        err = np.abs(v.astype(np.float64) - res[4][a:b].astype(np.float64) * np.pi / 180)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (f, worst)
        assert (R.error("angle", v, R.values64("angle", frames[f], tri, boxes[f])) <= bound).all()
        with make(G, s, "distance", tri[:, [0, 2]]) as ic:
            d = ic.values(f, 1)[0][0]
        assert np.abs(d - res[3][a:b]).max() <= 1e-5
    print("hbond angles: largest error / bound", round(worst, 3))
    s.close()


# ---------------------------------------------------------------- failing frames
@pytest.fixture(scope="module")
def small(G, aa):
    """40 chains + 10 atoms no tuple names, 8 wrapped frames in slots 0 .. 7, clean; the tests copy and break it"""
    boxes = R.frame_boxes(aa["box9"], NF)
    rng = np.random.default_rng(4)
    frames = [np.concatenate([R.chains(40, boxes[f], 300 + f)[0], (rng.random((10, 3)) * 5).astype(F)]) for f in range(NF)]
    return boxes, frames


def load(G, frames, boxes, n_slots=None):
    s = G.System(len(frames[0]), n_slots=n_slots or len(frames))
    for f, (x, b) in enumerate(zip(frames, boxes)):
        s.set_frame(x, b, slot=f)
    return s


@pytest.mark.parametrize("kind", KINDS)
def test_failing_frames(G, small, kind):
    boxes, frames = small
    t = R.chain_tuples(kind, 40)
    clean = load(G, frames, boxes)
    with make(G, clean, kind, t) as ic:
        want, st = ic.values(0, NF)
        assert not st.any() and np.isfinite(want).all()
    broken, bx = [x.copy() for x in frames], list(boxes)
    broken[3][[17, 9], 0] = np.nan                  # named atoms: the frame fails with the lower index
    broken[5][165, :] = np.nan                      # an atom no tuple names: fails nothing
    bx[6] = None                                    # no box: fails with PBC only
    s = load(G, broken, bx)
    with make(G, s, kind, t) as ic:
        v, st = ic.values(0, NF, raise_on_error=False)
        assert st.tolist() == [0, 0, 0, R.E_NO_POSITION, 0, 0, R.E_NO_BOX, 0]
        assert np.isnan(v[3]).all() and np.isnan(v[6]).all()
        for f in (0, 1, 2, 4, 5, 7):
            assert bits(v[f]) == bits(want[f]), f
        with pytest.raises(G.AtomError) as e:
            ic.values(0, NF)
        assert e.value.variant == "InvalidPosition" and e.value.detail == 9 and e.value.status == R.E_NO_POSITION
        with pytest.raises(G.SimBoxError) as e:
            ic.values(6, 2)
        assert e.value.status == R.E_NO_BOX
        # accumulate: a failed frame is counted for no tuple
        st = ic.accumulate(0, NF, raise_on_error=False)
        assert st.tolist() == [0, 0, 0, R.E_NO_POSITION, 0, 0, R.E_NO_BOX, 0] and ic.n_frames == 6
        ref = R.State(kind, len(t)).add(v)
        o, sm, q, n = ic.read_raw()
        assert n == 6 and R.same_bits(o, ref.o) and R.same_bits(sm, ref.s) and R.same_bits(q, ref.q)
        # a batch in which only frame 0 fails takes its origin from frame 1
        ic.clear()
        assert ic.n_frames == 0
        st = ic.accumulate(3, 3, raise_on_error=False)
        assert st.tolist() == [R.E_NO_POSITION, 0, 0] and ic.n_frames == 2 and R.same_bits(ic.read_raw()[0], want[4])
    with make(G, s, kind, t, pbc=False) as ic:      # without PBC the frame without a box is good
        v, st = ic.values(0, NF, raise_on_error=False)
        assert st.tolist() == [0, 0, 0, R.E_NO_POSITION, 0, 0, 0, 0] and np.isnan(v[3]).all() and np.isfinite(np.delete(v, 3, 0)).all()
    clean.close(); s.close()


# ---------------------------------------------------------------- accumulate
@pytest.mark.parametrize("kind", KINDS)
def test_accumulate_is_the_restatement_of_the_rows(G, world, kind):
    cell, s, boxes, frames = world
    t = R.chain_tuples(kind, NC)
    with make(G, s, kind, t) as ic, make(G, s, kind, t) as three, make(G, s, kind, t) as single:
        rows = ic.values(0, NF)[0]
        assert not ic.accumulate(0, NF).any() and ic.n_frames == NF
        ref = R.State(kind, len(t)).add(rows)
        o, sm, q, n = ic.read_raw()
        assert n == NF and o.dtype == np.float32 and sm.dtype == q.dtype == np.float64
        assert R.same_bits(o, ref.o) and R.same_bits(sm, ref.s) and R.same_bits(q, ref.q)
        three.accumulate(0, 1); three.accumulate(1, 5); three.accumulate(6, 2)
        for f in range(NF):
            single.accumulate(f, 1)
        for other in (three, single):
            assert [bits(x) for x in other.read_raw()[:3]] == [bits(o), bits(sm), bits(q)] and other.n_frames == NF
        mean, var = ic.read()
        m2, v2 = ref.two_pass(rows)
        assert mean.dtype == var.dtype == np.float64 and np.abs(mean - m2).max() <= 1e-9 and np.abs(var - v2).max() <= 1e-9
        cm, cv = ref.close()
        assert np.abs(mean - cm).max() <= 1e-12 and np.abs(var - cv).max() <= 1e-12
        if kind == "axis":
            # (cosines drawn anew in every frame: |d| < 2, so v - o rounds by up to ulp_f32(1) / 2 = 6e-8 per term, v^2 by 2 |v| times
            #  that and S by 1.5 times that again; test_merge_of_two_halves holds a trajectory, where the subtraction is exact, to 1e-9)
            want = 1.5 * (rows.astype(np.float64) ** 2).mean(0) - 0.5
            assert np.abs(ic.order_parameter() - want).max() <= 1.5 * 2 * 6e-8
        else:
            with pytest.raises(ValueError):
                ic.order_parameter()
        # merge: an empty dst takes src's state as it is (two halves against one walk: test_merge_of_two_halves)
        with make(G, s, kind, t) as a, make(G, s, kind, t) as b, make(G, s, kind, t) as empty:
            a.accumulate(0, 3); b.accumulate(3, 5)
            a.merge(b)
            ma, va = a.read()
            assert a.n_frames == NF
            if kind != "dihedral":
                # (these chains are drawn anew in every frame: v - o is not exact in f32, the two origins round it differently by up
                #  to ulp_f32(pi) = 2.4e-7 per term, the variance by 2 max|d| times that: 1.5e-6; torsions drawn anew in every
                #  frame are not within pi of an origin, the header's condition for a dihedral's statistics)
                assert np.abs(ma - mean).max() <= 1e-6 and np.abs(va - var).max() <= 1e-5
            empty.merge(ic)
            assert [bits(x) for x in empty.read_raw()[:3]] == [bits(o), bits(sm), bits(q)] and empty.n_frames == NF
            b.clear(); a.merge(b)                   # an empty src changes nothing
            assert a.n_frames == NF and bits(a.read()[0]) == bits(ma)
            with pytest.raises(G.DeviceError) as e:
                a.merge(a)
            assert e.value.status == R.E_INVALID_ARG
            with make(G, s, kind, t[:-1]) as fewer, make(G, s, kind, t, pbc=False) as flagged:
                for other in (fewer, flagged):
                    with pytest.raises(G.GroupError) as e:
                        a.merge(other)
                    assert e.value.status == R.E_INCONSISTENT_GROUP
            with pytest.raises(G.DeviceError) as e:
                b.read()                            # n = 0
            assert e.value.status == R.E_INVALID_ARG


@pytest.mark.parametrize("kind", KINDS)
def test_merge_of_two_halves(G, kind):
    """merge moves src's sums to dst's origin in f64, so it agrees with one walk to 1e-9 wherever the f32 subtraction v - o is exact
    for both origins.  The input is what the statistics are for, a trajectory: 120 whole chains jiggling by 0.002 nm, and the tuples
    whose value in frame 0 is at least 0.3 in magnitude (a dihedral's at most 2.8), so that every later value lies within a factor
    of two of either origin and the subtraction is exact (Sterbenz); the test checks that it was"""
    rng = np.random.default_rng(21)
    base = R.chains(120, R.DODECAHEDRON, 77)[1]
    frames = [(base + (rng.standard_normal(base.shape) * 0.002 if f else 0)).astype(F) for f in range(NF)]
    t = R.chain_tuples(kind, 120)
    if kind != "distance":                      # (a bond's length moves by a few per cent: every bond stays in)
        v0 = np.abs(R.values64(kind, frames[0], t, None, AXIS))
        t = t[(v0 >= 0.3) & (v0 <= 2.8)]
    assert len(t) >= 40
    s = load(G, frames, [None] * NF)
    with make(G, s, kind, t, pbc=False) as walk, make(G, s, kind, t, pbc=False) as a, make(G, s, kind, t, pbc=False) as b:
        rows = walk.values(0, NF)[0].astype(np.float64)
        for o in (rows[0], rows[3]):
            assert ((rows / o >= 0.5) & (rows / o <= 2.0)).all()
        walk.accumulate(0, NF); a.accumulate(0, 3); b.accumulate(3, 5)
        a.merge(b)
        (mw, vw), (ma, va) = walk.read(), a.read()
        assert a.n_frames == NF == walk.n_frames and np.abs(ma - mw).max() <= 1e-9 and np.abs(va - vw).max() <= 1e-9
        if kind == "axis":                      # S = 1/2 <3 cos^2 - 1> of the rows
            assert np.abs(walk.order_parameter() - (1.5 * (rows ** 2).mean(0) - 0.5)).max() <= 1e-9
            assert np.abs(a.order_parameter() - (1.5 * (rows ** 2).mean(0) - 0.5)).max() <= 1e-9
    s.close()


def test_torsion_oscillating_across_pi(G):
    """a dihedral built to alternate between +3.10 and -3.10 rad: var < 0.01 and |mean| > 3.1"""
    nf = 10
    frames = []
    for f in range(nf):
        phi = 3.10 if f % 2 == 0 else -3.10
        # i = (0,1,0), j = 0, k = (1,0,0), l = k + (0, cos phi, sin phi): the pins' geometry turned by phi
        frames.append(np.array([[0, 1, 0], [0, 0, 0], [1, 0, 0], [1, np.cos(phi), np.sin(phi)]], F) * F(0.15) + F(2.0))
    s = load(G, frames, [None] * nf)
    with make(G, s, "dihedral", [[0, 1, 2, 3]], pbc=False) as ic:
        v = ic.values(0, nf)[0][:, 0]
        assert np.abs(np.abs(v) - 3.10).max() < 1e-4 and (np.sign(v) == np.where(np.arange(nf) % 2 == 0, 1, -1)).all()
        ic.accumulate(0, nf)
        mean, var = ic.read()
        assert var[0] < 0.01 and abs(mean[0]) > 3.1 and -np.pi < mean[0] <= np.pi
        ref = R.State("dihedral", 1).add(v[:, None])
        o, sm, q, n = ic.read_raw()
        assert R.same_bits(sm, ref.s) and R.same_bits(q, ref.q) and R.same_bits(o, ref.o)
    s.close()


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("kind", KINDS)
def test_values_bits_do_not_depend_on_the_launch(G, world, kind):
    cell, s, boxes, frames = world
    t = R.chain_tuples(kind, NC)
    T = len(t)
    with make(G, s, kind, t) as ic:
        want = bits(ic.values(0, NF)[0])
        assert bits(ic.values(0, NF)[0]) == want                                           # two runs
        for ranges in (1, 2, 7):
            for chunk in (1, 3, NF):
                ic.set_launch(ranges, chunk)
                assert bits(ic.values(0, NF)[0]) == want, (ranges, chunk)
                assert ic.stat(G._lib.IC_STAT_LAST_RANGE_GROUPS) == ranges and ic.stat(G._lib.IC_STAT_LAST_FRAME_GROUPS) == -(-NF // chunk)
        ic.set_launch(0, 0)
        assert bits(np.concatenate([ic.values(0, 3)[0], ic.values(3, 1)[0], ic.values(4, 4)[0]])) == want    # batch cuts
        # the device variant with ld > T, into device memory the library handed out (a distance matrix: the sentinel written
        # beforehand): the padding columns and the row behind the last keep it
        ld = T + 5
        dev, n1, n2, st = s.group_all_distances_batch_device("all", "all", 0, 1)
        assert not st.any() and n1 * n2 >= (NF + 1) * ld
        before = s.device_read(dev, 0, (NF + 1, ld))
        st = ic.values_device(dev, 0, NF, ld=ld)
        after = s.device_read(dev, 0, (NF + 1, ld))
        assert not st.any() and bits(after[:NF, :T]) == want and bits(after[:NF, T:]) == bits(before[:NF, T:]) and bits(after[NF]) == bits(before[NF])
        assert bits(before[:NF, :T]) != want
        with pytest.raises(G.DeviceError) as e:
            ic.values_device(dev, 0, NF, ld=T - 1)
        assert e.value.status == R.E_INVALID_ARG
        with pytest.raises(ValueError):
            ic.values_device(dev, 0, NF)
    # a fresh context
    s2 = G.System(4 * NC, n_slots=NF)
    for f in range(NF):
        s2.set_frame(frames[f][0], boxes[f], slot=f)
    with make(G, s2, kind, t) as ic:
        assert bits(ic.values(0, NF)[0]) == want
    s2.close()


# ---------------------------------------------------------------- errors
def test_creation_errors_and_refused_calls(G, small):
    boxes, frames = small
    s = load(G, frames, boxes)
    n = s.n_atoms

    def err(kind, tuples, **kw):
        with pytest.raises(G.GroanError) as e:
            G.Internals(s, kind, tuples, **kw)
        return type(e.value).__name__, e.value.status, e.value.detail

    assert err("distance", [[0, 1], [2, n]]) == ("AtomError", R.E_OUT_OF_RANGE, n)
    assert err("dihedral", [[0, 1, 2, 3], [4, 5, n + 7, 6]]) == ("AtomError", R.E_OUT_OF_RANGE, n + 7)
    assert err("angle", np.zeros((0, 3), np.uint64))[:2] == ("DeviceError", R.E_INVALID_ARG)          # T = 0
    lib = G._lib.load()
    assert err("angle", [[0, 1, 2], [3, 4, 3]])[:2] == ("DeviceError", R.E_INVALID_ARG)               # an atom twice in one tuple
    assert lib.gr_last_error_index(s._ctx) == 1                                                      # ... the tuple
    assert err("axis", [[0, 1]])[:2] == ("DeviceError", R.E_INVALID_ARG)                              # no axis
    assert err("axis", [[0, 1]], axis=(0, 0, 0))[:2] == ("DeviceError", R.E_INVALID_ARG)
    assert err("axis", [[0, 1]], axis=(0, np.nan, 1))[:2] == ("DeviceError", R.E_INVALID_ARG)
    assert err("axis", [[0, 1]], axis=(0, np.inf, 1))[:2] == ("DeviceError", R.E_INVALID_ARG)
    with pytest.raises(ValueError):
        G.Internals(s, "improper", [[0, 1, 2, 3]])
    with pytest.raises(ValueError):
        G.Internals(s, "angle", [[0, 1, 2]], axis=(0, 0, 1))
    import ctypes as C
    st = C.c_int(0)
    t = np.array([[0, 1]], np.uint64)
    assert not lib.gr_internals_create(s._ctx, 9, t.ctypes.data_as(C.c_void_p), 1, 0, None, C.byref(st)) and st.value == R.E_INVALID_ARG     # unknown kind
    # the caller's array may go; a scaled axis (by a power of two: the same f32 direction) is the same axis
    with G.Internals(s, "axis", [[0, 1], [4, 5]], axis=AXIS) as a, G.Internals(s, "axis", [[0, 1], [4, 5]], axis=tuple(8 * np.float32(x) for x in AXIS)) as b:
        assert bits(a.values(0, 2)[0]) == bits(b.values(0, 2)[0])
        a.accumulate(0, 2); b.accumulate(2, 2); a.merge(b)
        assert a.n_frames == 4
    # refused calls: slots out of range, a busy context, a closed object
    ic = G.Internals(s, "distance", [[0, 1]])
    with pytest.raises(G.DeviceError) as e:
        ic.values(NF - 1, 2)
    assert e.value.status == R.E_INVALID_ARG
    with pytest.raises(G.DeviceError):
        ic.accumulate(NF, 1)
    m = np.ones(n, F)
    ref, cur = G.System(n, masses=m, box=boxes[0], positions=frames[0]), G.System(n, masses=m, n_slots=2)
    cur.set_frame(frames[1], boxes[1], slot=0)
    plan = G.RMSDPlan(ref, cur, "all")
    with G.Internals(cur, "distance", [[0, 1]]) as busy, G.Internals(cur, "distance", [[0, 1]]) as other:
        busy.accumulate(0, 1)
        plan.begin(0, 1, fit=False)
        for call in (lambda: busy.values(0, 1), lambda: busy.accumulate(0, 1), lambda: busy.read(), lambda: busy.read_raw(), lambda: busy.clear(), lambda: busy.merge(other),
                     lambda: G.Internals(cur, "distance", [[0, 1]])):
            with pytest.raises(G.GroanError) as e:
                call()
            assert e.value.status == R.E_INVALID_ARG
        plan.end()
        assert busy.n_frames == 1 and not busy.accumulate(0, 1).any()
    plan.close(); ref.close(); cur.close()
    ic.close(); ic.close()
    for call in (lambda: ic.values(0, 1), lambda: ic.accumulate(0, 1), lambda: ic.read(), lambda: ic.read_raw(), lambda: ic.clear(), lambda: ic.stat(1), lambda: ic.set_launch(1, 1)):
        with pytest.raises(ValueError):
            call()
    s.close()

"""Region (gr_region_*; groan_rs_amd.Region): per-frame geometry selections over resident frames, against the oracle called once per
frame (oracle_lib.group_from_geometries).  A shape that follows an anchor is given to the oracle moved by the SAME float32 anchor array
that is passed to the call, added in numpy float32 arithmetic (one f32 add per component, as the library does).  Everything that is
compared is an integer -- counts, offsets, index lists -- and every comparison is np.array_equal; no atom and no frame is left out.

A frame whose anchor is not finite fails with GR_E_INVALID_ARG whether the region is naive or not (the rule is the anchors' own, not
one of the box checks that `naive` switches off); "the same frames with naive=True all succeed" is asserted for the frames that fail a
BOX check -- no box, strict mode on a triclinic cell, a body beyond the image walk."""
import os

import numpy as np
import pytest

import oracle_lib as O
from region_ref import E_GROUP_NOT_FOUND, E_INVALID_ARG, E_NO_BOX, E_NOT_ORTHOGONAL, E_UNSUPPORTED_BOX, build, check, expect, moved

pytestmark = pytest.mark.gpu
F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


# ------------------------------------------------------------------ 1. the reference's pinned counts, 2. anchored shapes
CASES = __import__("json").load(open(os.path.join(GOLD, "shape_cases.json")))["groups"]
EX_GROUPS = ("Protein", "Membrane", "W", "ION")


@pytest.fixture(scope="module")
def ex4(G, example):
    s = G.System(example["pos"].shape[0], n_slots=4)
    for f in range(4):
        s.set_frame(example["pos"], example["box9"], slot=f)
    for g in EX_GROUPS:
        s.group_create_from_ranges(g, [tuple(b) for b in example["blocks_" + g]])
    yield s
    s.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_L%d" % (c["source"], c["line"]))
def test_reference_pins(G, ex4, example, case):
    assert (case["source"], case["shapes"][0]["kind"], case["count"]) in (("Membrane", "cylinder", 206), ("W", "sphere", 1881), ("Protein", "rectangular", 25),
                                                                           ("W", "prism", 213))
    idx = O.container_expand(example["blocks_" + case["source"]])
    with G.Region(ex4, [build(G, sp) for sp in case["shapes"]]) as r:
        counts, st = r.select(case["source"], 0, 4)
        assert st.tolist() == [0] * 4 and counts.tolist() == [case["count"]] * 4          # the reference's pinned count, in every frame
        check(r, counts, expect([example["pos"]] * 4, [example["box9"]] * 4, idx, case["shapes"]))
        assert r.stat(G._lib.RG_STAT_LAST_TOTAL) == 4 * case["count"] and r.stat(G._lib.RG_STAT_LAST_PIECES) == 1 and r.stat(G._lib.RG_STAT_LAST_LAUNCHES) == 3


@pytest.fixture(scope="module")
def ex6(G, example):
    """frame 0 as it is; frames 1-5: group W moved by rng(7).uniform(-1, 1, 3) * box through the oracle's translate"""
    pos, box = example["pos"], example["box9"]
    W = O.container_expand(example["blocks_W"])
    rng = np.random.default_rng(7)
    frames = [pos]
    for f in range(1, 6):
        frames.append(O.translate(pos, W, (rng.uniform(-1, 1, 3) * box[:3]).astype(F), box))
    s = G.System(pos.shape[0], n_slots=6)
    for f in range(6):
        s.set_frame(frames[f], box, slot=f)
    for g in EX_GROUPS:
        s.group_create_from_ranges(g, [tuple(b) for b in example["blocks_" + g]])
    anchors, st = s.group_center_batch("Protein", G._lib.CENTER_PBC, 0, 0, 6)
    assert st.tolist() == [0] * 6 and anchors.dtype == F
    yield s, frames, box, W, anchors
    s.close()


CYL = {"kind": "cylinder", "position": [0.0, 0.0, -2.0], "radius": 2.0, "height": 4.0, "orientation": "Z"}
SPH = {"kind": "sphere", "position": [0.0, 0.0, 0.0], "radius": 2.5}


@pytest.mark.parametrize("specs", [[CYL], [CYL, SPH]], ids=["cylinder", "cylinder_and_sphere"])
def test_anchored_shapes(G, ex6, specs):
    """the README example: the waters inside a cylinder of radius 2, height 4 along z, centred on the protein's centre of every frame
    (the oracle counts 48, 411, 276, 407, 414, 46 for ITS centres; asserted here: the lists for the anchors that were actually used)"""
    s, frames, box, W, anchors = ex6
    with G.Region(s, [build(G, sp) for sp in specs]) as r:
        counts, st = r.select("W", 0, 6, anchors=anchors)
        assert st.tolist() == [0] * 6
        check(r, counts, expect(frames, [box] * 6, W, specs, anchors=anchors))
        assert (counts > 0).all() and len(set(counts.tolist())) > 1
        for f in (0, 3, 5):
            assert np.array_equal(r.frame(f), O.group_from_geometries(frames[f], W, box, moved(specs, anchors[f])))
        # the same anchors given to a sub-block of the frames
        sub, _ = r.select("W", 2, 3, anchors=anchors[2:5])
        check(r, sub, expect(frames[2:5], [box] * 3, W, specs, anchors=anchors[2:5]))


# ------------------------------------------------------------------ 3. ordinal, word and chunk edges
N_SYN = 12500
BOX_SYN = np.array([6.0, 6.4, 5.0, 0, 0, 0, 0, 0, 0], F)
EVERYTHING = {"kind": "sphere", "position": [3.0, 3.0, 2.5], "radius": 100.0}
NOTHING = {"kind": "sphere", "position": [3.0, 3.0, 2.5], "radius": 0.0}
HALF = {"kind": "rectangular", "position": [0.0, 0.0, 0.0], "size": [3.0, 6.4, 5.0]}               # periodic: half of the cell along x
HALF_NAIVE = {"kind": "rectangular", "position": [-1.2, -1.28, -1.0], "size": [4.2, 8.96, 7.0]}   # naive: half of where the atoms are (-0.2 L .. 1.2 L) along x
SYN_SPECS = {("everything", False): EVERYTHING, ("everything", True): EVERYTHING, ("nothing", False): NOTHING, ("nothing", True): NOTHING,
             ("half", False): HALF, ("half", True): HALF_NAIVE}


@pytest.fixture(scope="module")
def syn(G):
    rng = np.random.default_rng(20261001)
    frames = []
    for f in range(3):
        pos = (rng.uniform(-0.2, 1.2, (N_SYN, 3)) * BOX_SYN[:3]).astype(F)
        pos[rng.integers(0, N_SYN, 60)] = np.nan                              # Option<Vector3D>::None, other atoms in every frame
        pos[[5, 5 + 63, 5 + 64, 3 * 1023, 3 * 1024][f::3]] = np.nan         # ... and some at the edges of the groups below
        frames.append(pos)
    s = G.System(N_SYN, n_slots=3)
    for f in range(3):
        s.set_frame(frames[f], BOX_SYN, slot=f)
    regions = {key: G.Region(s, [build(G, spec)], naive=key[1]) for key, spec in SYN_SPECS.items()}
    yield s, frames, regions
    s.close()


def _form(form, n, rng):
    """the atoms of a source group of n atoms"""
    if form == "block": return np.arange(5, 5 + n)                            # one contiguous block not starting at 0
    if form == "list": return np.sort(rng.choice(N_SYN, n, replace=False))    # an index list
    if form == "third": return np.arange(2, 2 + 3 * n, 3)                     # every third atom
    cuts = sorted(set([0, n // 3, n // 2, n]))                                # several blocks with holes of 7 atoms between them
    return np.concatenate([np.arange(a, b) + 11 + 7 * k for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))])


def test_ordinal_word_and_chunk_edges(G, syn):
    s, frames, regions = syn
    C = regions[("half", False)].stat(G._lib.RG_STAT_CHUNK)
    assert C % 64 == 0 and 3 * (3 * C + 1) + 2 <= N_SYN
    sizes = [1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 1]
    rng = np.random.default_rng(20261002)
    seen_half = []
    for n in sizes + [4100]:                                                  # 4100: the dense scattered forms carry a mask (>= 4096 atoms)
        for form in ("block", "list", "third", "blocks"):
            if n == 4100 and form in ("block", "list"):
                continue
            idx = _form(form, n, rng).astype(np.uint64)
            assert idx.size == n and idx[-1] < N_SYN
            s.group_create_from_indices("src", idx)
            for (name, naive), r in regions.items():
                spec = SYN_SPECS[(name, naive)]
                counts, st = r.select("src", 0, 3)
                assert st.tolist() == [0, 0, 0], (n, form, name, naive)
                want = expect(frames, [BOX_SYN] * 3, idx, [spec], naive=naive)
                check(r, counts, want)
                has_pos = [int((~np.isnan(frames[f][idx.astype(np.int64), 0])).sum()) for f in range(3)]
                if name == "everything": assert counts.tolist() == has_pos, (n, form, naive)
                if name == "nothing": assert counts.tolist() == [0, 0, 0]
                if name == "half" and n >= 255: seen_half.append(float(counts.sum()) / (3 * n))
    assert 0.35 < min(seen_half) and max(seen_half) < 0.65                    # "about half": 0.5 expected, 255 atoms or more in every sample
    s.group_remove("src")


def test_all_atoms_and_empty_group_and_no_shapes(G, syn):
    s, frames, regions = syn
    r = regions[("half", False)]
    counts, st = r.select(None, 0, 3)                                         # NULL: all atoms
    check(r, counts, expect(frames, [BOX_SYN] * 3, np.arange(N_SYN, dtype=np.uint64), [HALF]))
    s.group_create_from_indices("void", [])
    counts, st = r.select("void", 0, 3)                                       # an empty group is not an error
    assert st.tolist() == [0, 0, 0] and counts.tolist() == [0, 0, 0]
    off, atoms = r.lists()
    assert off.tolist() == [0, 0, 0, 0] and atoms.size == 0
    s.group_remove("void")
    for naive in (False, True):                                               # no shape: every atom with a position
        with G.Region(s, [], naive=naive) as r0:
            counts, st = r0.select(None, 1, 2)
            check(r0, counts, expect(frames[1:], [BOX_SYN] * 2, np.arange(N_SYN, dtype=np.uint64), [], naive=naive))
            assert counts.tolist() == [int((~np.isnan(frames[f][:, 0])).sum()) for f in (1, 2)]


# ------------------------------------------------------------------ 4. non-orthogonal cells (the library's extension)
def tric_specs(frame0):
    """the five bodies about the centre of the fixture's atoms (a slab of 50 atoms, about 3.5 x 3 x 1 nm)"""
    c = np.round(frame0.mean(axis=0).astype(np.float64), 2)
    at = lambda dx, dy, dz: [float(c[0] + dx), float(c[1] + dy), float(c[2] + dz)]
    return [{"kind": "sphere", "position": at(0, 0, 0), "radius": 0.9},
            {"kind": "rectangular", "position": at(-1.0, -0.8, -0.3), "size": [1.6, 1.2, 0.5]},
            {"kind": "cylinder", "position": at(0, 0, -0.3), "radius": 0.9, "height": 0.5, "orientation": "Z"},
            {"kind": "cylinder", "position": at(-1.2, 0, 0), "radius": 0.35, "height": 2.0, "orientation": "X"},
            {"kind": "prism", "base1": at(-1.0, -0.8, -0.2), "base2": at(1.2, -0.5, -0.2), "base3": at(0.0, 0.9, -0.2), "height": 0.35}]


@pytest.mark.parametrize("name", ["triclinic", "octahedron", "dodecahedron"])
def test_triclinic_extension(G, tric_small, name):
    frames, boxes = tric_small[name + "_frames"], tric_small[name + "_boxes9"]
    nf, n = frames.shape[0], frames.shape[1]
    assert (nf, n) == (11, 50) and np.abs(boxes[:, 3:]).max() > 0
    s = G.System(n, n_slots=nf)
    for f in range(nf):
        s.set_frame(frames[f], boxes[f], slot=f)
    s.group_create_from_indices("Odd", list(range(1, n, 2)))
    TRIC_SPECS = tric_specs(frames[0])
    for spec in TRIC_SPECS:
        with G.Region(s, [build(G, spec)]) as r:
            for src, idx in ((None, np.arange(n, dtype=np.uint64)), ("Odd", np.arange(1, n, 2, dtype=np.uint64))):
                counts, st = r.select(src, 0, nf)
                assert st.tolist() == [0] * nf
                check(r, counts, expect(frames, boxes, idx, [spec]))
                assert 0 < int(counts.sum()) < nf * idx.size, (spec["kind"], src)     # every body takes some atoms and leaves some
    with G.Region(s, [build(G, TRIC_SPECS[0]), build(G, TRIC_SPECS[2])]) as r:      # two shapes: both must hold
        counts, st = r.select(None, 0, nf)
        check(r, counts, expect(frames, boxes, np.arange(n, dtype=np.uint64), [TRIC_SPECS[0], TRIC_SPECS[2]]))
        assert counts.sum() > 0
    # a body that reaches more lattice images than the selection enumerates: every frame is refused, on its own
    huge = {"kind": "cylinder", "position": [0.3, 0.2, 1.0], "radius": 40.0, "height": 40.0, "orientation": "Z"}
    with G.Region(s, [build(G, huge)]) as r:
        counts, st = r.select(None, 0, nf, raise_on_error=False)
        assert st.tolist() == [E_UNSUPPORTED_BOX] * nf and counts.tolist() == [0] * nf
        off, atoms = r.lists()
        assert off.tolist() == [0] * (nf + 1) and atoms.size == 0
        with pytest.raises(G.DeviceError) as e:
            r.select(None, 0, nf)
        assert e.value.status == E_UNSUPPORTED_BOX
    with G.Region(s, [build(G, huge)], naive=True) as r:                              # naive: no box, no walk
        counts, st = r.select(None, 0, nf)
        check(r, counts, expect(frames, boxes, np.arange(n, dtype=np.uint64), [huge], naive=True))
    s.close()


# ------------------------------------------------------------------ 5. per-frame failures
@pytest.fixture(scope="module")
def five(G):
    """300 atoms, 5 frames: 0, 1, 4 orthorhombic, 2 without a box, 3 triclinic"""
    n = 300
    rng = np.random.default_rng(20261003)
    ortho = np.array([4.0, 4.2, 3.8, 0, 0, 0, 0, 0, 0], F)
    tric = np.array([4.0, 4.2, 3.8, 0, 0, 0.7, 0, -0.9, 0.5], F)
    boxes = [ortho, ortho, None, tric, ortho]
    frames = [(rng.uniform(-0.1, 1.1, (n, 3)) * ortho[:3]).astype(F) for _ in range(5)]
    s = G.System(n, n_slots=5)
    for f in range(5):
        s.set_frame(frames[f], boxes[f], slot=f)
    s.group_create_from_ranges("most", [(3, 280)])
    yield s, frames, boxes, np.arange(3, 281, dtype=np.uint64)
    s.close()


FIVE_SPECS = [{"kind": "cylinder", "position": [0.0, 0.0, -1.0], "radius": 1.5, "height": 2.0, "orientation": "Z"},
              {"kind": "rectangular", "position": [-2.0, -2.0, -2.0], "size": [4.0, 4.0, 4.0]}]


def _failure(G, s, frames, boxes, idx, anchors, failed, status, error):
    """one call with the frames in `failed` failing with `status`: their status, count 0 and an empty list, the neighbours exact, and
    the call's own status the first failed frame's"""
    with G.Region(s, [build(G, sp) for sp in FIVE_SPECS]) as r:
        counts, st = r.select("most", 0, 5, anchors=anchors, raise_on_error=False)
        assert st.tolist() == [status[f] if f in failed else 0 for f in range(5)]
        clean = np.where(np.isfinite(anchors), anchors, F(0))
        want = expect(frames, boxes, idx, FIVE_SPECS, anchors=clean, failed=failed)
        check(r, counts, want)
        for f in failed:
            assert counts[f] == 0 and r.frame(f).size == 0
        assert want[0][[f for f in range(5) if f not in failed]].min() > 0
        with pytest.raises(error) as e:
            r.select("most", 0, 5, anchors=anchors)
        assert e.value.status == status[min(failed)]
        for f in failed:
            with pytest.raises(G.DeviceError) as e:                        # a failed frame is no group
                r.to_group(f, "Nope")
            assert e.value.status == E_INVALID_ARG and not s.group_exists("Nope")


def test_per_frame_failures(G, five):
    s, frames, boxes, idx = five
    rng = np.random.default_rng(20261004)
    anchors = (rng.uniform(0.5, 3.0, (5, 3))).astype(F)
    # one frame without a box among good ones
    _failure(G, s, frames, boxes, idx, anchors, {2}, {2: E_NO_BOX}, G.GroupError)
    # strict mode: the triclinic frame fails too; the first failed frame is still the one without a box
    s.set_strict_orthogonal(True)
    try:
        _failure(G, s, frames, boxes, idx, anchors, {2, 3}, {2: E_NO_BOX, 3: E_NOT_ORTHOGONAL}, G.GroupError)
        with G.Region(s, [build(G, sp) for sp in FIVE_SPECS]) as r:        # ... and alone it is the first
            counts, st = r.select("most", 3, 2, anchors=anchors[3:], raise_on_error=False)
            assert st.tolist() == [E_NOT_ORTHOGONAL, 0] and counts[0] == 0
            check(r, counts, expect(frames[3:], boxes[3:], idx, FIVE_SPECS, anchors=anchors[3:], failed={0}))
            with pytest.raises(G.GroupError) as e:
                r.select("most", 3, 2, anchors=anchors[3:])
            assert e.value.status == E_NOT_ORTHOGONAL
        # the same frames with naive=True all succeed: no box check of any kind
        with G.Region(s, [build(G, sp) for sp in FIVE_SPECS], naive=True) as r:
            counts, st = r.select("most", 0, 5, anchors=anchors)
            assert st.tolist() == [0] * 5
            check(r, counts, expect(frames, boxes, idx, FIVE_SPECS, naive=True, anchors=anchors))
            assert counts.min() > 0
    finally:
        s.set_strict_orthogonal(False)
    # a NaN / infinite anchor component (frames 1 and 4): the frame in front of the boxless one is now the first to fail
    bad = anchors.copy()
    bad[1, 2] = np.nan
    bad[4, 0] = np.inf
    _failure(G, s, frames, boxes, idx, bad, {1, 2, 4}, {1: E_INVALID_ARG, 2: E_NO_BOX, 4: E_INVALID_ARG}, G.DeviceError)
    with G.Region(s, [build(G, sp) for sp in FIVE_SPECS], naive=True) as r:    # the anchors' rule holds for a naive region too
        counts, st = r.select("most", 0, 5, anchors=bad, raise_on_error=False)
        assert st.tolist() == [0, E_INVALID_ARG, 0, 0, E_INVALID_ARG]
        check(r, counts, expect(frames, boxes, idx, FIVE_SPECS, naive=True, anchors=np.where(np.isfinite(bad), bad, F(0)), failed={1, 4}))


# ------------------------------------------------------------------ 6. segment and piece boundaries
def test_segment_boundary(G):
    """200 atoms, 1 030 resident frames in one call: two segments of the batch"""
    n, nf = 200, 1030
    rng = np.random.default_rng(20261005)
    base = (rng.random((n, 3)) * 3.0).astype(F)
    box = np.array([3.0, 3.0, 3.0, 0, 0, 0, 0, 0, 0], F)
    frames = [(base + F(0.013) * F(f % 97)).astype(F) for f in range(nf)]
    s = G.System(n, n_slots=nf)
    for f in range(nf):
        s.set_frame(frames[f], box, slot=f)
    s.group_create_from_ranges("g", [(1, 190)])
    idx = np.arange(1, 191, dtype=np.uint64)
    spec = {"kind": "cylinder", "position": [1.5, 1.5, 0.5], "radius": 1.0, "height": 1.5, "orientation": "Z"}
    with G.Region(s, [build(G, spec)]) as r:
        counts, st = r.select("g", 0, nf)
        want = expect(frames, [box] * nf, idx, [spec])
        assert not st.any()
        check(r, counts, want)
        assert r.stat(G._lib.RG_STAT_LAST_PIECES) == 2 and r.stat(G._lib.RG_STAT_LAST_LAUNCHES) == 6 and r.stat(G._lib.RG_STAT_LAST_TOTAL) == int(want[0].sum())
        assert len(set(want[0].tolist())) > 5 and want[0][1022:1027].min() > 0
        for f in range(1022, 1027):
            assert np.array_equal(r.frame(f), O.group_from_geometries(frames[f], idx, box, [spec])), f
        off, atoms = r.lists()
        # the pieces called on their own give the pieces of the list
        a, _ = r.select("g", 0, 1024)
        la = r.lists()[1]
        b, _ = r.select("g", 1024, 6)
        lb = r.lists()[1]
        assert np.array_equal(np.concatenate([a, b]), counts) and np.array_equal(np.concatenate([la, lb]), atoms)
    s.close()


def test_piece_boundaries(G, tric_small):
    """11 frames in pieces of 3 and of 1: the same bits as the default (one piece)"""
    frames, boxes = tric_small["octahedron_frames"], tric_small["octahedron_boxes9"]
    s = G.System(50, n_slots=11)
    for f in range(11):
        s.set_frame(frames[f], boxes[f], slot=f)
    rng = np.random.default_rng(20261006)
    anchors = rng.uniform(-0.5, 0.5, (11, 3)).astype(F)
    specs = [tric_specs(frames[0])[k] for k in (2, 0)]
    with G.Region(s, [build(G, sp) for sp in specs]) as r:
        c0, _ = r.select(None, 0, 11, anchors=anchors)
        o0, a0 = r.lists()
        assert r.stat(G._lib.RG_STAT_LAST_PIECES) == 1
        check(r, c0, expect(frames, boxes, np.arange(50, dtype=np.uint64), specs, anchors=anchors))
        assert c0.sum() > 0 and len(set(c0.tolist())) > 1
        for piece, pieces in ((3, 4), (1, 11), (0, 1)):
            r.set_piece_frames(piece)
            c, _ = r.select(None, 0, 11, anchors=anchors)
            o, a = r.lists()
            assert r.stat(G._lib.RG_STAT_LAST_PIECES) == pieces and r.stat(G._lib.RG_STAT_LAST_LAUNCHES) <= 3 * pieces
            assert np.array_equal(c, c0) and np.array_equal(o, o0) and np.array_equal(a, a0), piece
    s.close()


# ------------------------------------------------------------------ 7. state and history
def test_state_and_history(G, ex6):
    s, frames, box, W, anchors = ex6
    shapes = [build(G, CYL)]
    before = [s.get_positions(f) for f in range(6)]
    with G.Region(s, shapes) as r, G.Region(s, shapes) as fresh:
        c1, _ = r.select("W", 0, 6, anchors=anchors)
        o1, a1 = r.lists()
        c2, _ = r.select("W", 0, 6, anchors=anchors)                          # twice: the same bits
        o2, a2 = r.lists()
        assert np.array_equal(c1, c2) and np.array_equal(o1, o2) and np.array_equal(a1, a2)
        for f in range(6):                                                    # the frames are not modified
            assert np.array_equal(before[f].view(np.uint32), s.get_positions(f).view(np.uint32))
        # read_device + gr_device_read = read
        lib = G._lib.load()
        atoms_dev, off_dev, nf, total = r.lists_device()
        assert (nf, total) == (6, int(c1.sum()))
        narrow = np.zeros(total, np.uint32); off = np.zeros(nf + 1, np.uint64)
        assert lib.gr_device_read(s._ctx, atoms_dev, narrow.ctypes.data_as(G._lib.C.c_void_p), narrow.nbytes) == 0
        assert lib.gr_device_read(s._ctx, off_dev, off.ctypes.data_as(G._lib.C.c_void_p), off.nbytes) == 0
        assert np.array_equal(narrow.astype(np.uint64), a1) and np.array_equal(off, o1)
        # gr_region_read: the total alone, and a buffer that is too small
        n_total = G._lib.C.c_uint64(0)
        assert lib.gr_region_read(r._rg, None, None, 0, G._lib.C.byref(n_total)) == 0 and n_total.value == total
        small = np.zeros(total - 1, np.uint64)
        assert lib.gr_region_read(r._rg, None, small.ctypes.data_as(G._lib.C.c_void_p), total - 1, None) == E_INVALID_ARG
        # a failed call leaves an empty result, and the call after it gives what a fresh object gives
        with pytest.raises(G.GroupError) as e:
            r.select("nobody", 0, 6, anchors=anchors)
        assert e.value.variant == "NotFound" and e.value.status == E_GROUP_NOT_FOUND
        assert r.lists_device()[2:] == (0, 0) and r.lists()[0].tolist() == [0] and r.lists()[1].size == 0
        with pytest.raises(IndexError):
            r.frame(0)
        with pytest.raises(G.DeviceError) as e:
            r.to_group(0, "Pore")
        assert e.value.status == E_INVALID_ARG
        with pytest.raises(G.DeviceError):                                    # a refused argument: slots that do not exist
            r.select("W", 4, 3)
        c3, _ = r.select("W", 1, 4, anchors=anchors[1:5])
        cf, _ = fresh.select("W", 1, 4, anchors=anchors[1:5])
        assert np.array_equal(c3, cf) and all(np.array_equal(x, y) for x, y in zip(r.lists(), fresh.lists()))
        assert np.array_equal(c3, c1[1:5]) and np.array_equal(r.lists()[1], a1[int(o1[1]):int(o1[5])])
        # to_group: a per-frame selection as an ordinary group
        assert r.to_group(2, "Pore") is False
        members = np.array(list(s.group_container("Pore")), np.uint64)
        assert np.array_equal(members, r.frame(2)) and members.size == c3[2]
        cen, st = s.group_center_batch("Pore", G._lib.CENTER_PBC, 0, 3, 1)
        want = O.get_center(frames[3], members, box)
        assert st.tolist() == [0] and np.abs(cen[0] - want).max() <= 1e-5
        assert r.to_group(0, "Pore") is True                                  # replaced: AlreadyExistsWarning
        assert np.array_equal(np.array(list(s.group_container("Pore")), np.uint64), r.frame(0))
        with pytest.raises(G.GroupError) as e:
            r.to_group(0, "Po>re")
        assert e.value.variant == "InvalidName"
        with pytest.raises(G.DeviceError) as e:                               # beyond the last call's frames
            r.to_group(4, "Pore")
        assert e.value.status == E_INVALID_ARG
        s.group_remove("Pore")


def test_create_refusals(G, ex4):
    lib = G._lib.load()
    from groan_rs_amd.shapes import GrShape, pack
    st = G._lib.C.c_int(0)
    nine, _ = pack([G.Sphere([0, 0, 0], 1.0)] * 9)
    assert not lib.gr_region_create(ex4._ctx, nine, 9, 0, G._lib.C.byref(st)) and st.value == E_INVALID_ARG
    bad = (GrShape * 1)(); bad[0].kind = 7
    assert not lib.gr_region_create(ex4._ctx, bad, 1, 0, G._lib.C.byref(st)) and st.value == E_INVALID_ARG
    prism, _ = pack([G.TriangularPrism([3, 4, 2], [7, 5, 2], [4, 3, 2], 4.3)])
    assert not lib.gr_region_create(ex4._ctx, prism, 1, 1, G._lib.C.byref(st)) and st.value == E_INVALID_ARG
    r = lib.gr_region_create(ex4._ctx, prism, 1, 0, G._lib.C.byref(st))
    assert r and st.value == 0
    v = G._lib.C.c_uint64(0)
    assert lib.gr_region_stat(r, 99, G._lib.C.byref(v)) == E_INVALID_ARG
    lib.gr_region_destroy(r)

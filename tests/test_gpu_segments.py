"""Segments (gr_segments_*; groan_rs_amd.Segments): the centres of every segment of a partition over resident frames, against the
oracle called once per segment as a group.

The oracle runs in its f64-accumulation mode (set_accumulate_f64, as for the large-selection tests): there it is within 1e-6 nm of
exact arithmetic on every segment used here, while the reference's sequential f32 sums are themselves up to 1.14e-5 nm off on the
134-atom lipids.  Margin: 1e-5 nm per component, the project's parity margin.  A periodic centre that lies within 1e-4 nm of a cell
face may legitimately come out on either side of it: a component whose oracle ESTIMATE (for the PBC kind: the segment's unweighted
estimate, about which it unwraps) lies that close to 0 or to the box length is compared modulo the box vector, and the test asserts
that at most 16 segments per frame and kind need that rule.

Real system: tests/golden/aa_full.npz (2 frames, 32 817 atoms, orthorhombic), masses of aa_peptide.npz, split by residue number: 5 271
contiguous segments of 1, 3, 11, 12, 13, 19, 22 and 134 atoms.
Synthetic system: 9 500 atoms (37 tiles + 28 atoms), 6 slots, segments of 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4096 and
4097 atoms -- both sides of every team-class boundary -- in four layouts; every segment is a compact cloud that straddles the cell
faces; the 284 atoms outside every segment sit at 1e30 with a mass of 1e30 (an atom read by mistake wrecks a sum).
The pad atoms behind atom 9 499 (228 of them, up to the end of the last tile) are NOT poisoned by this test: the C ABI has no call
that writes them, so they hold what the library put there -- zero positions and NaN masses.  A read past the end is still seen: the
"to_end" layout ends its last segment on atom 9 499, where an overshoot meets a NaN mass in the weighted kinds and a (0, 0, 0) atom
that moves the mean in the unweighted ones.
  slot 0, 4  orthorhombic      1, 5  triclinic      2  no box      3  orthorhombic, NaN positions inside the 17- and the 4097-atom segment
  test_nan_position_in_the_narrow_teams overwrites slot 4 with NaN positions inside the 3- and the 15-atom segment and puts it back"""
import os

import numpy as np
import pytest

import oracle_lib as O
from segments_ref import (E_INVALID_ARG, E_NO_BOX, E_NO_MASS, E_NO_POSITION, ESTIMATE, KINDS, NAIVE, PBC, SEAM, TOL, _bits, _cell, _check_against, _max_error,  # noqa: F401
                          _oracle, _reference, _seam_flags)

pytestmark = pytest.mark.gpu
F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

N = 9500
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4096, 4097]
BOX = [6.0, 6.4, 5.0]
TRIC = [6.0, 6.4, 5.0, 0, 0, 1.0, 0, -1.5, 0.8]
BOXES = [BOX, TRIC, None, BOX, BOX, TRIC]
NAN_FRAME, NOBOX_FRAME = 3, 2
LAYOUTS = ["from3", "gather", "to_end", "overlap"]


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


# ------------------------------------------------------------------ the real system
@pytest.fixture(scope="module")
def aa(G):
    d = np.load(os.path.join(GOLD, "aa_full.npz"))
    masses = np.load(os.path.join(GOLD, "aa_peptide.npz"))["masses"]
    frames, boxes, resid = [f for f in d["frames"]], [b for b in d["boxes9"]], d["resid"]
    n = len(resid)
    s = G.System(n, masses=masses, n_slots=2)
    for f in range(2):
        s.set_frame(frames[f], boxes[f], slot=f)
    seg = G.Segments.by_resid(s, resid)
    lists = [seg.atoms(k) for k in range(len(seg))]
    ref = _reference(frames, boxes, masses, lists)
    yield s, seg, lists, ref, boxes
    s.close()


def test_real_system_partition(G, aa):
    s, seg, lists, _, _ = aa
    assert len(seg) == 5271 and sorted(set(seg.sizes.tolist())) == [1, 3, 11, 12, 13, 19, 22, 134]
    assert all(int(l[-1]) - int(l[0]) + 1 == len(l) for l in lists) and int(seg.sizes.sum()) == 32817
    sizes = seg.sizes
    want = [int((sizes <= 4).sum()), int(((sizes > 4) & (sizes <= 16)).sum()), int((sizes > 16).sum()), 0]
    assert [seg.stat(k) for k in (1, 2, 3, 4)] == want and all(want[:3])


@pytest.mark.parametrize("kind, weighted", KINDS)
def test_real_system_against_oracle(G, aa, kind, weighted):
    s, seg, lists, ref, boxes = aa
    got, st = seg.centers(0, 2, kind, weighted)
    assert st.tolist() == [0, 0]
    _check_against(got, st, ref, (kind, weighted), boxes)
    assert seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 3 and seg.stat(G._lib.SEG_STAT_LAST_LAUNCH_SETS) == 1


def test_real_system_against_group_calls(G, aa):
    """40 segments spread over all sizes, each as a group through gr_group_center_batch"""
    s, seg, lists, ref, boxes = aa
    sizes = seg.sizes
    # up to seven of every size (three sizes have a single residue), spread over the system: 7 + 7 + 7 + 1 + 1 + 7 + 1 + 7 + 2 more lipids
    pick = sorted(set(int(k) for n in sorted(set(sizes.tolist())) for k in np.nonzero(sizes == n)[0][np.linspace(0, int((sizes == n).sum()) - 1, 7).astype(int)]))
    pick = sorted(set(pick) | set(int(k) for k in np.nonzero(sizes == 134)[0][[1, 2]]))
    assert len(pick) == 40 and set(sizes[pick].tolist()) == set(sizes.tolist())
    for k in pick:
        s.group_create_from_ranges("seg%d" % k, [(int(lists[k][0]), int(lists[k][-1]))])
    for kind, w in KINDS:
        got, _ = seg.centers(0, 2, kind, w)
        flags = ref[(kind, w)][2]
        for k in pick:
            want, st = s.group_center_batch("seg%d" % k, kind, w, 0, 2)
            assert st.tolist() == [0, 0]
            for f in range(2):
                err = _max_error(got[f, k:k + 1], want[f:f + 1], flags[f, k:k + 1] if flags is not None else None, boxes[f])
                assert err.max() <= TOL, (kind, w, k, f, float(err.max()))
    for k in pick:
        s.group_remove("seg%d" % k)


# ------------------------------------------------------------------ the synthetic system
def _layout(name):
    rng = np.random.default_rng(20260601)
    if name == "gather":
        perm = rng.permutation(N)[:sum(SIZES)]
        cuts = np.cumsum([0] + SIZES)
        return [np.sort(perm[cuts[k]:cuts[k + 1]]).astype(np.uint64) for k in range(len(SIZES))]
    a = N - sum(SIZES) if name == "to_end" else 3
    lists = []
    for n in SIZES:
        lists.append(np.arange(a, a + n, dtype=np.uint64)); a += n
    if name == "overlap":            # a slice of the 4096-atom segment, and the 17-atom segment once more
        lists.append(lists[14][100:400].copy())
        lists.append(lists[7].copy())
    return lists


def _synthetic_frames(lists):
    rng = np.random.default_rng(20260602)
    frames = []
    for f, box in enumerate(BOXES):
        H = _cell(box if box is not None else BOX)
        Hi = np.linalg.inv(H)
        pos = np.full((N, 3), 1e30, np.float64)
        done = np.zeros(N, bool)
        for s, idx in enumerate(lists):
            idx = idx.astype(np.int64)
            new = idx[~done[idx]]                                  # (an overlapping segment lies inside a cloud that exists already)
            if new.size == 0:
                continue
            c = rng.random(3)
            c[rng.integers(0, 3)] = rng.choice([0.004, 0.996, 0.0, 0.5])      # the cloud straddles a face of the cell
            d = np.clip(rng.normal(0.0, 0.15, (new.size, 3)), -0.45, 0.45)
            u = c + d @ Hi
            u -= np.floor(u)
            pos[new] = u @ H
            done[new] = True
        frames.append(pos.astype(F))
    assert len(lists[7]) == 17 and len(lists[15]) == 4097
    frames[NAN_FRAME][int(lists[7][4])] = np.nan
    frames[NAN_FRAME][int(lists[15][4000])] = np.nan
    return frames


_WORLDS = {}


@pytest.fixture(scope="module")
def worlds(G):
    def get(name):
        if name not in _WORLDS:
            lists = _layout(name)
            frames = _synthetic_frames(lists)
            rng = np.random.default_rng(20260603)
            masses = (1.0 + 15.0 * rng.random(N)).astype(F)
            inside = np.zeros(N, bool)
            for l in lists:
                inside[l.astype(np.int64)] = True
            assert int((~inside).sum()) == N - sum(SIZES) == 284
            masses[~inside] = 1e30
            s = G.System(N, masses=masses, n_slots=6)
            for f in range(6):
                s.set_frame(frames[f], BOXES[f], slot=f)
            seg = G.Segments.from_lists(s, lists)
            _WORLDS[name] = (s, seg, lists, frames, masses, _reference(frames, BOXES, masses, lists))
        return _WORLDS[name]
    yield get
    for w in _WORLDS.values():
        w[0].close()
    _WORLDS.clear()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_synthetic_against_oracle(G, worlds, layout):
    s, seg, lists, frames, masses, ref = worlds(layout)
    assert len(seg) == len(lists) and seg.sizes.tolist() == [len(l) for l in lists]
    assert all(np.array_equal(seg.atoms(k), lists[k]) for k in range(len(lists)))
    if layout == "to_end":
        assert int(lists[-1][-1]) == N - 1
    if layout == "from3":
        assert all(int(l[0]) % 256 != 0 for l in lists) and sum(int(l[0]) // 256 != int(l[-1]) // 256 for l in lists) >= 6
    nan17, nan4097 = int(lists[7][4]), int(lists[15][4000])
    for kind, w in KINDS:
        got, st = seg.centers(0, 6, kind, w, raise_on_error=False)
        _check_against(got, st, ref, (kind, w), BOXES)
        # the frame with the two NaN atoms: exactly their segments are NaN, the status and index are the first one's in segment order
        bad = np.isnan(got[NAN_FRAME]).any(axis=1).nonzero()[0].tolist()
        assert bad == ([7, 15] if layout != "overlap" else [7, 15, 17]) and st[NAN_FRAME] == E_NO_POSITION
        assert ref[(kind, w)][1][NAN_FRAME][7] == (E_NO_POSITION, nan17) and ref[(kind, w)][1][NAN_FRAME][15] == (E_NO_POSITION, nan4097)
        with pytest.raises(G.GroupError) as e:
            seg.centers(NAN_FRAME, 1, kind, w)
        assert e.value.variant == "InvalidPosition" and e.value.detail == nan17
        assert st.tolist() == [0, 0, 0 if kind == NAIVE else E_NO_BOX, E_NO_POSITION, 0, 0]
        # the first failed FRAME of the call is what the call raises
        with pytest.raises(G.GroupError) as e:
            seg.centers(0, 6, kind, w)
        if kind == NAIVE:
            assert (e.value.variant, e.value.detail) == ("InvalidPosition", nan17)
        else:
            assert e.value.variant == "InvalidSimBox" and e.value.detail.variant == "DoesNotExist" and e.value.status == E_NO_BOX


def test_nan_mass(G, worlds):
    s, seg, lists, frames, masses, _ = worlds("from3")
    bad_mass = masses.copy()
    atom = int(lists[5][9])                            # inside the 15-atom segment, in front of the 17-atom one
    bad_mass[atom] = np.nan
    try:
        s.set_masses(bad_mass)
        ref = _reference(frames, BOXES, bad_mass, lists)
        for kind, w in KINDS:
            got, st = seg.centers(0, 6, kind, w, raise_on_error=False)
            _check_against(got, st, ref, (kind, w), BOXES)
            if w:
                assert st.tolist() == [E_NO_MASS, E_NO_MASS, E_NO_MASS if kind == NAIVE else E_NO_BOX, E_NO_MASS, E_NO_MASS, E_NO_MASS]
                assert np.isnan(got[0]).any(axis=1).nonzero()[0].tolist() == [5]
                assert np.isnan(got[NAN_FRAME]).any(axis=1).nonzero()[0].tolist() == [5, 7, 15]
                with pytest.raises(G.GroupError) as e:
                    seg.centers(NAN_FRAME, 1, kind, w)
                assert (e.value.variant, e.value.detail) == ("InvalidMass", atom)
            else:
                assert st.tolist() == [0, 0, 0 if kind == NAIVE else E_NO_BOX, E_NO_POSITION, 0, 0]
    finally:
        s.set_masses(masses)


@pytest.mark.parametrize("layout", ["from3", "gather"])
def test_nan_position_in_the_narrow_teams(G, worlds, layout):
    """NaN positions inside the 3-atom and the 15-atom segment: in the 4- and the 16-lane class several teams share a wave, so the
    failing team leaves out the second stage of a PBC centre while the teams next to it, in the same wave, run it"""
    s, seg, lists, frames, masses, _ = worlds(layout)
    assert len(lists[2]) == 3 and len(lists[5]) == 15
    nan3, nan15 = int(lists[2][1]), int(lists[5][14])
    slot = 4
    bad = frames[slot].copy()
    bad[nan3] = np.nan
    bad[nan15] = np.nan
    ref = _reference([bad], [BOXES[slot]], masses, lists)
    try:
        s.set_frame(bad, BOXES[slot], slot=slot)
        for kind, w in KINDS:
            got, st = seg.centers(slot, 1, kind, w, raise_on_error=False)
            _check_against(got, st, ref, (kind, w), [BOXES[slot]])
            assert np.isnan(got[0]).any(axis=1).nonzero()[0].tolist() == [2, 5] and st.tolist() == [E_NO_POSITION]
            assert ref[(kind, w)][1][0][2] == (E_NO_POSITION, nan3) and ref[(kind, w)][1][0][5] == (E_NO_POSITION, nan15)
            with pytest.raises(G.GroupError) as e:
                seg.centers(slot, 1, kind, w)
            assert e.value.variant == "InvalidPosition" and e.value.detail == nan3
    finally:
        s.set_frame(frames[slot], BOXES[slot], slot=slot)


# ------------------------------------------------------------------ bit-level properties
@pytest.mark.parametrize("layout", ["from3", "gather"])
def test_bitwise(G, worlds, layout):
    s, seg, lists, frames, masses, _ = worlds(layout)
    M = len(lists)
    assert [seg.stat(k) for k in (G._lib.SEG_STAT_TEAM4, G._lib.SEG_STAT_TEAM16, G._lib.SEG_STAT_WAVE, G._lib.SEG_STAT_WORKGROUP)] == [4, 3, 8, 1]
    rev = G.Segments.from_lists(s, lists[::-1])
    sub = G.Segments.from_lists(s, [lists[15], lists[2], lists[8], lists[5]])
    for kind, w in KINDS:
        a, st_a = seg.centers(0, 6, kind, w, raise_on_error=False)
        assert seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 4 and seg.stat(G._lib.SEG_STAT_LAST_LAUNCH_SETS) == 1
        # two runs
        b, st_b = seg.centers(0, 6, kind, w, raise_on_error=False)
        assert np.array_equal(_bits(a), _bits(b)) and st_a.tolist() == st_b.tolist()
        # six one-frame calls
        for f in range(6):
            one, st_1 = seg.centers(f, 1, kind, w, raise_on_error=False)
            assert np.array_equal(_bits(one[0]), _bits(a[f])) and st_1[0] == st_a[f], (kind, w, f)
        # the device form, read back
        dev, st_d = seg.centers_device(0, 6, kind, w, raise_on_error=False)
        assert np.array_equal(_bits(s.device_read(dev, 0, (6, M, 3))), _bits(a)) and st_d.tolist() == st_a.tolist()
        dev, st_d = seg.centers_device(4, 2, kind, w)
        assert np.array_equal(_bits(s.device_read(dev, 0, (2, M, 3))), _bits(a[4:6]))
        # the same segments among other neighbours: in reverse order, and four of them alone
        r, st_r = rev.centers(0, 6, kind, w, raise_on_error=False)
        assert np.array_equal(_bits(r[:, ::-1]), _bits(a)) and st_r.tolist() == st_a.tolist()
        q, _ = sub.centers(0, 6, kind, w, raise_on_error=False)
        assert np.array_equal(_bits(q), _bits(a[:, [15, 2, 8, 5]]))
    rev.close(); sub.close()


def test_overlapping_copy_has_the_same_bits(G, worlds):
    s, seg, lists, _, _, _ = worlds("overlap")
    assert np.array_equal(lists[17], lists[7])
    for kind, w in KINDS:
        a, _ = seg.centers(0, 6, kind, w, raise_on_error=False)
        assert np.array_equal(_bits(a[:, 17]), _bits(a[:, 7]))


def test_constructors_and_errors(G, worlds):
    s, seg, lists, _, _, _ = worlds("from3")
    lib = G._lib.load()
    # labels: a group, first-appearance order, atoms outside the group in no segment
    s.group_create_from_ranges("head", [(0, 99)])
    lab = np.arange(N, dtype=np.uint64) // 7
    lab[50:60] = 0
    by = G.Segments.by_resid(s, lab, group="head")
    assert len(by) == 15 and by.atoms(0).tolist() == list(range(7)) + list(range(50, 60)) and int(by.sizes.sum()) == 100
    names = np.array([b"SOL", b"NA", b"SOL", b"CL"])[np.arange(N) % 4]
    bn = G.Segments.by_resname(s, names)
    assert len(bn) == 3 and bn.atoms(0)[:3].tolist() == [0, 2, 4] and bn.atoms(1)[:2].tolist() == [1, 5] and bn.atoms(2)[0] == 3
    by.close(); bn.close()
    with pytest.raises(G.GroupError) as e:
        G.Segments.by_resid(s, lab, group="nobody")
    assert e.value.variant == "NotFound"
    s.group_create_from_indices("void", [])
    with pytest.raises(G.GroupError) as e:
        G.Segments.by_resid(s, lab, group="void")
    assert e.value.variant == "EmptyGroup"
    for name in ("head", "void"):
        s.group_remove(name)
    with pytest.raises(G.GroupError) as e:
        G.Segments.from_lists(s, [[1, 2], []])
    assert e.value.variant == "EmptyGroup"
    with pytest.raises(G.GroupError):
        G.Segments.from_lists(s, [])
    with pytest.raises(G.AtomError) as e:
        G.Segments.from_lists(s, [[1, 2], [5, N]])
    assert e.value.variant == "OutOfRange" and e.value.detail == N
    with pytest.raises(G.DeviceError) as e:
        G.Segments.from_lists(s, [[2, 1]])
    assert e.value.status == E_INVALID_ARG
    st = np.zeros(1, np.int32)
    assert not lib.gr_segments_create(s._ctx, None, None, 1, st.ctypes.data_as(G._lib.c_i32p)) and st[0] == E_INVALID_ARG
    # the calls' own refusals
    with pytest.raises(G.DeviceError):
        seg.centers(0, 6, 3, 0)
    with pytest.raises(G.DeviceError):
        seg.centers(4, 3, NAIVE, 0)
    with pytest.raises(G.DeviceError) as e:
        seg.centers_device(0, 1025, NAIVE, 0)
    assert e.value.status == E_INVALID_ARG
    with pytest.raises(IndexError):
        seg.atoms(len(seg))
    # strict mode: the triclinic frames fail their box check, the naive centre does not care
    s.set_strict_orthogonal(True)
    try:
        _, st = seg.centers(0, 2, PBC, 1, raise_on_error=False)
        assert st.tolist() == [0, 2]
        got, st = seg.centers(0, 2, NAIVE, 1, raise_on_error=False)
        assert st.tolist() == [0, 0] and not np.isnan(got).any()
    finally:
        s.set_strict_orthogonal(False)


def test_molecules(G):
    fx = np.load(os.path.join(GOLD, "whole_fixture.npz"))
    pos, box, bonds = fx["multi_pos"], fx["multi_box"], fx["multi_bonds"]
    s = G.System(50, masses=np.ones(50, F), n_slots=1)
    s.set_frame(pos, list(box), slot=0)
    none = G.Segments.from_molecules(s)
    assert len(none) == 50 and none.sizes.tolist() == [1] * 50
    s.add_bonds(bonds)
    seg = G.Segments.from_molecules(s)
    mols = [sorted(s.molecule_indices(r)) for r in s.get_mol_references()]
    inmol = set(a for m in mols for a in m)
    want = sorted(mols + [[a] for a in range(50) if a not in inmol])
    assert [seg.atoms(k).tolist() for k in range(len(seg))] == want
    s.clear_bonds()                                                    # a snapshot: the object keeps its molecules
    assert [seg.atoms(k).tolist() for k in range(len(seg))] == want and len(none) == 50
    got, st = seg.get_center(0, 1)
    O.set_accumulate_f64(True)
    try:
        ref = np.stack([O.get_center(pos, np.array(m), list(box)) for m in want])
        est = np.stack([O.estimate_center(pos, np.array(m), list(box)) for m in want])
    finally:
        O.set_accumulate_f64(False)
    assert st.tolist() == [0] and _max_error(got[0], ref, _seam_flags(est, list(box)), list(box)).max() <= TOL
    s.close()


def test_more_frames_than_one_piece(G):
    """1 030 frames of a 40-atom system: two pieces of the batch, the same bits as the pieces called on their own"""
    n, nf = 40, 1030
    rng = np.random.default_rng(20260604)
    s = G.System(n, masses=(1.0 + rng.random(n)).astype(F), n_slots=nf)
    base = (rng.random((n, 3)) * 0.4 + 1.0).astype(F)
    for f in range(nf):
        s.set_frame(base + F(0.001) * F(f % 97), [3.0, 3.0, 3.0] if f != 1027 else None, slot=f)
    seg = G.Segments.from_lists(s, [np.arange(0, 3), np.arange(3, 13), np.arange(1, 40, 2)])
    got, st = seg.centers(0, nf, PBC, 1, raise_on_error=False)
    assert seg.stat(G._lib.SEG_STAT_LAST_LAUNCH_SETS) == 2 and seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 6
    a, st_a = seg.centers(0, 1024, PBC, 1)
    b, st_b = seg.centers(1024, 6, PBC, 1, raise_on_error=False)
    assert np.array_equal(_bits(got), _bits(np.concatenate([a, b]))) and st.tolist() == st_a.tolist() + st_b.tolist()
    assert st[1027] == E_NO_BOX and int((st != 0).sum()) == 1 and np.isnan(got[1027]).all() and not np.isnan(np.delete(got, 1027, axis=0)).any()
    s.close()

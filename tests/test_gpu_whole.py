"""Bond topology and whole molecules / groups on resident frames (gr_add_bonds, gr_make_molecules_whole[_batch],
gr_make_group_whole[_batch]; groan_rs_amd.System) against the reference's known answers (src/system/modifying.rs:980-1220) and
the numpy-f32 restatement tests/whole_ref.py: bit for bit in orthorhombic cells, within 1e-5 nm of the oracle's triclinic wrap /
vector_to elsewhere (the full-size frames put atoms up to ~45 nm from the origin, where one f32 ulp is 3.8e-6 nm, and the two sides
contract the lattice shifts differently).  A frame that fails is left bit for bit untouched."""
import os

import numpy as np
import pytest

import oracle_lib as O
import whole_ref as W

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "whole_fixture.npz")
E_NO_BOX, E_NOT_ORTHOGONAL, E_NO_POSITION = 1, 2, 6


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _system(G, pos, box, bonds=None, n_slots=1):
    s = G.System(len(pos), n_slots=n_slots)
    for k in range(n_slots):
        s.set_frame(pos, box, slot=k)
    if bonds is not None and len(bonds):
        s.add_bonds(bonds)
    return s


def _ref_of(n, bonds):
    refs, orders = W.molecules(W.neighbours(n, bonds))
    return W.ref_of(n, refs, orders), refs, orders


# ------------------------------------------------------------------ known answers of the reference
def test_three_atom_cases(G):
    """modifying.rs:1009-1107"""
    pos = np.array([[6, 6, 2], [1, 4, 2], [4, 1, 2]], np.float32)
    s = _system(G, pos, [5, 5, 5], [(0, 1), (0, 2)])
    s.make_molecules_whole()
    assert s.get_positions().tolist() == [[1, 1, 2], [1, -1, 2], [-1, 1, 2]]
    s = _system(G, pos, [5, 5, 5], [(1, 2)])
    s.make_molecules_whole()
    assert s.get_positions().tolist() == [[6, 6, 2], [1, 4, 2], [-1, 6, 2]]
    s = _system(G, pos, [5, 5, 5])
    s.make_group_whole("all")
    assert np.allclose(s.get_positions(), [[1, 1, 2], [1, -1, 2], [-1, 1, 2]], atol=1e-6)
    s = _system(G, pos, [5, 5, 5])
    s.group_create_from_indices("Selected", [1, 2])
    s.make_group_whole("Selected")
    assert np.allclose(s.get_positions(), [[6, 6, 2], [1, -1, 2], [-1, 1, 2]], atol=1e-6)


def test_mol_references_and_orders(G, fx):
    s = _system(G, fx["multi_pos"], fx["multi_box"], fx["multi_bonds"])
    assert s.has_bonds() and s.get_mol_references() == [0, 5, 33]          # modifying.rs:980-992
    s.add_bond(10, 15)
    assert s.get_mol_references() == [0, 5, 33]
    with pytest.raises(G.AtomError) as e:
        s.add_bond(7, 7)
    assert e.value.variant == "InvalidBond" and e.value.detail == (7, 7)
    with pytest.raises(G.AtomError) as e:
        s.add_bonds([(1, 2), (3, 60), (60, 60)])
    assert e.value.variant == "OutOfRange" and e.value.detail == 60
    s.clear_bonds()
    assert not s.has_bonds() and s.get_mol_references() == []
    c = _system(G, fx["conect_pos"], fx["conect_box"], fx["conect_bonds"])
    nb = W.neighbours(50, fx["conect_bonds"])
    for start in (0, 28, 49):
        assert c.molecule_indices(start) == W.bfs(nb, start)
    with pytest.raises(G.AtomError) as e:
        c.molecule_indices(50)
    assert e.value.variant == "OutOfRange" and e.value.detail == 50


def _check_gro(pos, lines):
    for k in range(50):
        assert W.gro_xyz(pos[k]) == lines[2 + k][20:44], (k, W.gro_xyz(pos[k]), lines[2 + k])


def test_conect_whole_molecules_and_group(G, fx):
    """modifying.rs:1110-1158: conect.pdb translated by (3.5, 4.5, -3.0), made whole, written as gro"""
    s = _system(G, fx["conect_pos"], fx["conect_box"], fx["conect_bonds"])
    s.atoms_translate([3.5, 4.5, -3.0])
    moved = s.get_positions()
    s.make_molecules_whole()
    got = s.get_positions()
    _check_gro(got, fx["whole_molecules_lines"])
    ref_of, _, orders = _ref_of(50, fx["conect_bonds"])
    want, err = W.make_molecules_whole(moved, fx["conect_box"], ref_of, orders)
    assert err is None and np.array_equal(_bits(got), _bits(want))
    g = _system(G, fx["conect_pos"], fx["conect_box"])
    g.atoms_translate([3.5, 4.5, -3.0])
    moved = g.get_positions()
    g.make_group_whole("all")
    got = g.get_positions()
    _check_gro(got, fx["whole_group_lines"])
    g.set_frame(moved, fx["conect_box"])                 # the library's own estimate of the centre, on the frame before the call
    c, _ = g.group_center_batch("all", 1, 0, 0, 1)
    assert np.array_equal(_bits(got), _bits(W.make_group_whole(moved, np.arange(50), fx["conect_box"], c[0])))


def test_missing_box_and_missing_position(G, fx):
    """modifying.rs:1161-1220"""
    s = _system(G, fx["conect_pos"], fx["conect_box"], fx["conect_bonds"])
    s.reset_box()
    with pytest.raises(G.AtomError) as e:
        s.make_molecules_whole()
    assert e.value.variant == "InvalidSimBox" and e.value.detail.variant == "DoesNotExist"
    with pytest.raises(G.GroupError) as e:
        s.make_group_whole("all")
    assert e.value.variant == "InvalidSimBox" and e.value.detail.variant == "DoesNotExist"
    pos = fx["conect_pos"].copy(); pos[15] = np.nan
    s.set_frame(pos, fx["conect_box"])
    before = _bits(s.get_positions())
    with pytest.raises(G.AtomError) as e:
        s.make_molecules_whole()
    assert e.value.variant == "InvalidPosition" and e.value.detail == 15
    with pytest.raises(G.GroupError) as e:
        s.make_group_whole("all")
    assert e.value.variant == "InvalidPosition" and e.value.detail == 15
    assert np.array_equal(_bits(s.get_positions()), before)                # failed frames are left untouched


# ------------------------------------------------------------------ error order
def test_error_order(G, fx):
    ref_of, _, orders = _ref_of(50, fx["conect_bonds"])
    s = _system(G, fx["conect_pos"], fx["conect_box"], fx["conect_bonds"])
    pos = fx["conect_pos"].copy(); pos[[4, 5]] = np.nan                     # BFS from 0 visits atom 5 before atom 4
    s.set_frame(pos, fx["conect_box"])
    with pytest.raises(G.AtomError) as e:
        s.make_molecules_whole()
    assert e.value.detail == 5 and W.make_molecules_whole(pos, fx["conect_box"], ref_of, orders)[1] == 5
    # a NaN in the second molecule while the first is fine; then also one in the first
    mref, _, morders = _ref_of(50, fx["multi_bonds"])
    m = _system(G, fx["multi_pos"], fx["multi_box"], fx["multi_bonds"])
    pos = fx["multi_pos"].copy(); pos[40] = np.nan; pos[20] = np.nan
    m.set_frame(pos, fx["multi_box"])
    with pytest.raises(G.AtomError) as e:
        m.make_molecules_whole()
    assert e.value.detail == 20 == W.make_molecules_whole(pos, fx["multi_box"], mref, morders)[1]
    pos[20] = fx["multi_pos"][20]
    m.set_frame(pos, fx["multi_box"])
    with pytest.raises(G.AtomError) as e:
        m.make_molecules_whole()
    assert e.value.detail == 40
    # the isolated atom 49 without position is no error and stays without position
    pos = fx["conect_pos"].copy(); pos[49] = np.nan
    s.set_frame(pos, fx["conect_box"])
    s.make_molecules_whole()
    got = s.get_positions()
    want, err = W.make_molecules_whole(pos, fx["conect_box"], ref_of, orders)
    assert err is None and np.isnan(got[49]).all() and np.array_equal(_bits(got[:49]), _bits(want[:49]))


def test_no_bonds_moves_nothing_but_needs_a_box(G, fx):
    pos = fx["conect_pos"] + np.float32(7.0)
    s = _system(G, pos, fx["conect_box"])
    s.make_molecules_whole()
    assert np.array_equal(_bits(s.get_positions()), _bits(pos))
    s.reset_box()
    with pytest.raises(G.AtomError) as e:
        s.make_molecules_whole()
    assert e.value.variant == "InvalidSimBox"


# ------------------------------------------------------------------ batches and topology changes
def test_batch_statuses_and_untouched_failures(G, fx):
    box = fx["conect_box"]
    ref_of, _, orders = _ref_of(50, fx["conect_bonds"])
    rng = np.random.default_rng(11)
    s = G.System(50, n_slots=8)
    s.add_bonds(fx["conect_bonds"])
    frames, want_st = [], [0, E_NO_BOX, 0, E_NO_POSITION, 0, E_NO_BOX, E_NO_POSITION, 0]
    for f in range(8):
        p = (fx["conect_pos"] + rng.integers(-1, 2, (50, 3)).astype(np.float32) * box).astype(np.float32)
        if f == 3: p[20] = np.nan
        if f == 6: p[[4, 5]] = np.nan
        s.set_frame(p, None if want_st[f] == E_NO_BOX else box, slot=f)
        frames.append(s.get_positions(f))
    st = s.make_molecules_whole_batch(0, 8, raise_on_error=False)
    assert st.tolist() == want_st
    for f in range(8):
        got = s.get_positions(f)
        if want_st[f]:
            assert np.array_equal(_bits(got), _bits(frames[f])), f
        else:
            want, err = W.make_molecules_whole(frames[f], box, ref_of, orders)
            assert err is None and np.array_equal(_bits(got), _bits(want)), f
    with pytest.raises(G.AtomError) as e:                                   # the first failed frame: slot 1, no box
        s.make_molecules_whole_batch(0, 8)
    assert e.value.variant == "InvalidSimBox"
    with pytest.raises(G.AtomError) as e:                                   # from slot 2 on: slot 3, atom 20
        s.make_molecules_whole_batch(2, 6)
    assert e.value.variant == "InvalidPosition" and e.value.detail == 20
    # make_group_whole over the same slots: the errors of gr_group_center_batch(estimate)
    st = s.make_group_whole_batch("all", 0, 8, raise_on_error=False)
    _, cst = s.group_center_batch("all", 1, 0, 0, 8, raise_on_error=False)
    assert st.tolist() == cst.tolist() == want_st


def test_topology_change_between_calls(G):
    pos = np.array([[6, 6, 2], [1, 4, 2], [4, 1, 2], [9, 9, 9]], np.float32)
    box = np.full(3, 5.0, np.float32)
    s = _system(G, pos, box, [(1, 2)])
    s.make_molecules_whole()
    first = s.get_positions()
    r, _, o = _ref_of(4, [(1, 2)])
    assert np.array_equal(_bits(first), _bits(W.make_molecules_whole(pos, box, r, o)[0]))
    s.add_bond(0, 1)
    s.add_bond(2, 3)
    s.make_molecules_whole()
    r, _, o = _ref_of(4, [(1, 2), (0, 1), (2, 3)])
    assert np.array_equal(_bits(s.get_positions()), _bits(W.make_molecules_whole(first, box, r, o)[0]))
    s.clear_bonds()
    before = s.get_positions()
    s.make_molecules_whole()
    assert np.array_equal(_bits(s.get_positions()), _bits(before))


# ------------------------------------------------------------------ 1e6 atoms
N = 1_000_000
CHAIN0, CHAIN_N = 4998, 20000          # one chain whose reference lies many tiles and workgroups before most of its atoms
INTER0, INTER_N = CHAIN0 + CHAIN_N, 400  # two molecules on alternating indices
NF = 32


def _topology():
    bonds = []
    w0 = np.arange(0, CHAIN0, 3)
    bonds += [np.stack([w0, w0 + 1], 1), np.stack([w0, w0 + 2], 1)]
    c = np.arange(CHAIN0, CHAIN0 + CHAIN_N - 1)
    bonds.append(np.stack([c, c + 1], 1))
    for par in (0, 1):
        a = np.arange(INTER0 + par, INTER0 + INTER_N - 2, 2)
        bonds.append(np.stack([a, a + 2], 1))
    w1 = np.arange(INTER0 + INTER_N, N - 2, 3)
    bonds += [np.stack([w1, w1 + 1], 1), np.stack([w1, w1 + 2], 1)]
    bonds = np.concatenate(bonds).astype(np.uint64)
    ref = np.full(N, -1, np.int64)
    ref[:CHAIN0] = np.repeat(w0, 3)
    ref[CHAIN0:CHAIN0 + CHAIN_N] = CHAIN0
    ref[INTER0:INTER0 + INTER_N:2] = INTER0; ref[INTER0 + 1:INTER0 + INTER_N:2] = INTER0 + 1
    ref[INTER0 + INTER_N:INTER0 + INTER_N + 3 * len(w1)] = np.repeat(w1, 3)
    return bonds, ref


def _box9(kind):
    if kind == "ortho":
        return np.array([21.5, 22.0, 21.0, 0, 0, 0, 0, 0, 0], np.float32)
    if kind == "dodecahedron":
        return O.box_from_lengths_angles([22.0, 22.0, 22.0], [60.0, 60.0, 90.0])
    return O.box_from_lengths_angles([22.0, 21.5, 23.0], [75.0, 80.0, 70.0])


def _lattice(box9):
    a = np.array([box9[0], box9[3], box9[4]], np.float32)
    b = np.array([box9[5], box9[1], box9[6]], np.float32)
    c = np.array([box9[7], box9[8], box9[2]], np.float32)
    return np.stack([a, b, c])


def _frames(box9, ref, seed):
    """compact molecules about their references, every atom moved by a random lattice vector; references exactly on faces"""
    rng = np.random.default_rng(seed)
    M = _lattice(box9)
    frac = rng.random((N, 3), np.float32)
    refpos = (frac @ M).astype(np.float32)
    faces = np.array([[0, 0, 0], [box9[0], 1.0, 1.0], [-1e-7, 2.0, 2.0], [3.0, box9[1], -0.0], [np.float32(box9[0]) * 2, 0, box9[2]]], np.float32)
    for k, f in enumerate(faces):
        refpos[INTER0 + INTER_N + 3 * (k + 1)] = f                        # reference atoms of waters, exactly on faces
    refpos[CHAIN0] = faces[1]
    off = rng.normal(0.0, 0.06, (N, 3)).astype(np.float32)
    off[CHAIN0:CHAIN0 + CHAIN_N] = rng.uniform(-1.5, 1.5, (CHAIN_N, 3)).astype(np.float32)
    inmol = ref >= 0
    pos = refpos.copy()
    pos[inmol] = (refpos[ref[inmol]] + off[inmol]).astype(np.float32)
    for r in [INTER0 + INTER_N + 3 * (k + 1) for k in range(len(faces))] + [CHAIN0]:
        pos[r] = refpos[r]
    shifts = rng.integers(-1, 2, (N, 3)).astype(np.float32)
    shifts[rng.random(N) < 0.5] = 0
    return (pos + shifts @ M).astype(np.float32)


def _bonds_min_image(got, bonds, box9, tol=1e-5):
    i, j = bonds[:, 0].astype(np.int64), bonds[:, 1].astype(np.int64)
    d = (got[j] - got[i]).astype(np.float64)
    M = _lattice(box9).astype(np.float64)
    best = np.full(len(d), np.inf)
    for k in np.array(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1])).reshape(3, -1).T:
        best = np.minimum(best, np.linalg.norm(d + k @ M, axis=1))
    assert (np.linalg.norm(d, axis=1) <= best + tol).all()


@pytest.fixture(scope="module")
def big(G):
    bonds, ref = _topology()
    s = G.System(N, n_slots=NF)
    s.add_bonds(bonds)
    refs = s.get_mol_references()
    assert refs == sorted(set(ref[ref >= 0].tolist()))
    assert s.molecule_indices(INTER0 + 1)[:3] == [INTER0 + 1, INTER0 + 3, INTER0 + 5]
    yield s, bonds, ref
    s.close()


@pytest.mark.parametrize("kind", ["ortho", "dodecahedron", "triclinic"])
def test_full_size_molecules(big, kind):
    s, bonds, ref = big
    box9 = _box9(kind)
    inputs = []
    for f in range(NF):
        p = _frames(box9, ref, 1000 * f + len(kind))
        s.set_frame(p, box9, slot=f)
        inputs.append(p)
    st = s.make_molecules_whole_batch(0, NF)
    assert (st == 0).all()
    rng = np.random.default_rng(5)
    for f in range(NF):
        got = s.get_positions(f)
        if kind == "ortho":
            want, err = W.make_molecules_whole(inputs[f], box9[:3], ref)
            assert err is None and np.array_equal(_bits(got), _bits(want)), f
        elif f % 8 == 0 or f == NF - 1:
            sample = rng.choice(N, 20000, replace=False)
            sample = sample[ref[sample] >= 0]
            refw = {}
            for a in sample:
                r = int(ref[a])
                if r not in refw:
                    refw[r] = O.wrap(inputs[f][r], box9)
                want = refw[r] + O.vector_to(refw[r], inputs[f][a], box9)
                assert np.abs(got[a] - want).max() <= 1e-5, (f, a, got[a], want)
            lone = ref < 0
            assert np.array_equal(_bits(got[lone]), _bits(inputs[f][lone]))
        if f in (0, NF - 1):
            _bonds_min_image(got, bonds, box9)


def test_full_size_strict(G, big):
    s, _, ref = big
    box9 = _box9("dodecahedron")
    p = _frames(box9, ref, 77)
    for f in range(4):
        s.set_frame(p, box9, slot=f)
    s.set_strict_orthogonal(True)
    try:
        st = s.make_molecules_whole_batch(0, 4, raise_on_error=False)
        assert (st == E_NOT_ORTHOGONAL).all()
        with pytest.raises(G.AtomError) as e:
            s.make_molecules_whole(0)
        assert e.value.variant == "InvalidSimBox" and e.value.detail.variant == "NotOrthogonal"
    finally:
        s.set_strict_orthogonal(False)
    assert np.array_equal(_bits(s.get_positions(3)), _bits(p))


@pytest.mark.parametrize("form", ["block", "gather", "masked"])
def test_full_size_group(G, big, form):
    s, _, ref = big
    box9 = _box9("ortho")
    rng = np.random.default_rng(3)
    # (a scattered selection denser than an eighth of its span gets the bit mask, a sparser one walks its index list)
    idx = {"block": np.arange(100_003, 400_001), "gather": np.arange(5, 300_000, 11), "masked": np.arange(200_001, 600_000, 2)}[form]
    name = "whole_" + form
    s.group_create_from_indices(name, idx)
    # a compact blob about a point, every atom moved by a random lattice vector
    inputs = []
    for f in range(4):
        p = (rng.random((N, 3), np.float32) * box9[:3]).astype(np.float32)
        p[idx] = (np.float32([5.0, 6.0, 7.0]) + rng.normal(0, 1.5, (len(idx), 3))).astype(np.float32)
        p[idx] += (rng.integers(-1, 2, (len(idx), 3)) * box9[:3]).astype(np.float32)
        s.set_frame(p, box9, slot=f)
        inputs.append(p)
    c, cst = s.group_center_batch(name, 1, 0, 0, 4)
    st = s.make_group_whole_batch(name, 0, 4)
    assert (st == 0).all() and (cst == 0).all()
    for f in range(4):
        got = s.get_positions(f)
        want = W.make_group_whole(inputs[f], idx, box9[:3], c[f])
        assert np.array_equal(_bits(got), _bits(want)), f
        oc = O.estimate_center(inputs[f], idx, box9)
        for a in rng.choice(idx, 2000, replace=False):
            assert np.abs(got[a] - (oc + O.vector_to(oc, inputs[f][a], box9))).max() <= 1e-5

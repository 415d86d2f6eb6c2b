"""RMSDPanel / rmsd_matrix (gr_rmsd_panel_*, gr_rmsd_matrix*): the all-pairs RMSD matrix over packed frames, against two references.

1. The oracle: M[i, j] within 1e-5 nm of oracle_lib.calc_rmsd(frame j as reference, frame i as current), the project's bar for an RMSD.
2. The library's own one-reference path: column j within 1e-5 nm of gr_rmsd_batch with a plan on frame j.

Everything else is bit for bit: an entry depends on its two frames and on the number of atoms alone -- not on the frames' places in their
panels, on how they were appended, on the neighbours in the tile, on the run or on what the context did before."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from rmsd_matrix_ref import TOL, matrix_of, oracle_matrix, same_bits, system_with

pytestmark = pytest.mark.gpu
F = np.float32
OK, E_NO_BOX, E_NOT_ORTHOGONAL, E_NO_POSITION, E_INVALID_ARG = 0, 1, 2, 6, 10


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def aa_frames(aa):
    """the 21 peptide frames placed into the 32 817-atom system at the peptide's block"""
    a, b = (int(v) for v in aa["blocks_peptide"][0])
    assert b - a + 1 == aa["traj_peptide"].shape[1] == 363
    frames = []
    for f in range(21):
        x = aa["pos"].copy(); x[a:b + 1] = aa["traj_peptide"][f]
        frames.append(x)
    return frames, (a, b)


@pytest.fixture(scope="module")
def world(G, aa):
    """the aa system with its 21 frames resident (slots 21 .. 23 are spare), the full 21 x 21 matrix and the oracle's"""
    frames, (a, b) = aa_frames(aa)
    s = system_with(G, frames, aa["traj_boxes9"], aa["masses"], n_slots=24)
    s.group_create_from_ranges("Peptide", [(a, b)])
    idx = np.arange(a, b + 1)
    pep = [x[a:b + 1] for x in frames]
    want = oracle_matrix(pep, aa["traj_boxes9"], pep, aa["traj_boxes9"], aa["masses"][a:b + 1])
    full = matrix_of(G, s, "Peptide", list(range(21)))
    yield dict(s=s, frames=frames, boxes=aa["traj_boxes9"], masses=aa["masses"], idx=idx, want=want, full=full)
    s.close()


# ------------------------------------------------------------------ reference parity
def test_matrix_equals_the_oracle_and_the_one_reference_path(G, world):
    s, M = world["s"], world["full"]
    assert M.shape == (21, 21) and M.dtype == F and np.isfinite(M).all()
    err = np.abs(M - world["want"]).max()
    print("aa peptide 21 x 21: max |M - oracle| = %.3g nm" % err)
    assert err <= TOL
    worst = 0.0
    for j in range(21):
        plan = G.RMSDPlan(s, s, "Peptide", ref_slot=j)
        r, st = plan.rmsd(0, 21)
        plan.close()
        assert (st == OK).all()
        worst = max(worst, float(np.abs(M[:, j] - r).max()))
    print("aa peptide 21 x 21: max |column - gr_rmsd_batch| = %.3g nm" % worst)
    assert worst <= TOL


def test_short_trajectory_large_rmsds(G, short_traj):
    """11 x 261 atoms, RMSDs of 2.5 - 5.3 nm, seeded masses in 1 .. 32"""
    masses = np.random.default_rng(11).uniform(1.0, 32.0, 261).astype(F)
    frames, boxes = list(short_traj["frames"]), short_traj["boxes9"]
    s = system_with(G, frames, boxes, masses)
    M = matrix_of(G, s, "all", list(range(11)))
    want = oracle_matrix(frames, boxes, frames, boxes, masses)
    off = want[~np.eye(11, dtype=bool)]
    assert off.min() > 2.0 and off.max() < 6.0
    print("short_traj 11 x 11: max |M - oracle| = %.3g nm" % np.abs(M - want).max())
    assert np.abs(M - want).max() <= TOL and np.array_equal(M, M.T)
    s.close()


@pytest.mark.parametrize("cell", ["triclinic", "dodecahedron"])
def test_non_orthogonal_cells(G, tric_small, cell):
    """non-strict mode: the triclinic wrap of gr_math.h, as the one-reference path accepts it"""
    frames, boxes = list(tric_small[cell + "_frames"]), tric_small[cell + "_boxes9"]
    masses = np.random.default_rng(12).uniform(1.0, 32.0, 50).astype(F)
    s = system_with(G, frames, boxes, masses)
    M = matrix_of(G, s, "all", list(range(11)))
    want = oracle_matrix(frames, boxes, frames, boxes, masses)
    print("%s 11 x 11: max |M - oracle| = %.3g nm" % (cell, np.abs(M - want).max()))
    assert np.abs(M - want).max() <= TOL and np.array_equal(M, M.T)
    s.set_strict_orthogonal(True)
    p = G.RMSDPanel(s, "all", 11)
    st = p.append(0, 11, raise_on_error=False)
    assert (st == E_NOT_ORTHOGONAL).all() and np.array_equal(p.status, st)          # as gr_rmsd_batch in strict mode
    s.close()


# ------------------------------------------------------------------ two panels, determinism
def test_two_panels_equal_the_block_of_the_full_matrix(G, world):
    s = world["s"]
    rows, cols = G.RMSDPanel(s, "Peptide", 10), G.RMSDPanel(s, "Peptide", 11)
    rows.append(0, 10); cols.append(10, 11)
    assert len(rows) == 10 and len(cols) == 11 and rows.n_atoms == cols.n_atoms == 363
    assert same_bits(G.rmsd_matrix(rows, cols), world["full"][:10, 10:])
    assert same_bits(G.rmsd_matrix(cols, rows), world["full"][10:, :10])
    dev, nr, nc = G.rmsd_matrix(rows, cols, device=True)
    assert (nr, nc) == (10, 11) and same_bits(s.device_read(dev, 0, (10, 11)), world["full"][:10, 10:])
    rows.close(); cols.close()


def test_appending_in_pieces_running_twice_and_blocking_give_the_same_bits(G, world):
    s, full = world["s"], world["full"]
    assert np.array_equal(full, full.T)                              # cols == rows: exactly symmetric
    for pieces in (1, 5):
        assert same_bits(matrix_of(G, s, "Peptide", list(range(21)), pieces=pieces), full), pieces
    p = G.RMSDPanel(s, "Peptide", 21)
    p.append(0, 21)
    assert same_bits(G.rmsd_matrix(p), full) and same_bits(G.rmsd_matrix(p, p), full)
    dev, nr, nc = G.rmsd_matrix(p, device=True)
    assert (nr, nc) == (21, 21) and same_bits(s.device_read(dev, 0, (21, 21)), full)
    p.set_block_entries(21 * 16)                                     # the host form in column blocks of 16 (no mirror in there)
    assert same_bits(G.rmsd_matrix(p), full)
    p.set_block_entries(0)
    p.clear()
    assert len(p) == 0
    p.append(3, 4)
    assert same_bits(G.rmsd_matrix(p), full[3:7, 3:7])
    p.close()


def test_a_permutation_of_the_frames_permutes_the_matrix(G, world):
    s, full = world["s"], world["full"]
    perm = np.random.default_rng(5).permutation(21)
    M = matrix_of(G, s, "Peptide", [int(v) for v in perm])
    assert same_bits(M, full[np.ix_(perm, perm)])
    # ... and a frame copied into a spare slot is the same frame
    s.set_frame(world["frames"][9], world["boxes"][9], slot=22)
    assert same_bits(matrix_of(G, s, "Peptide", [22, 4, 9]), full[np.ix_([9, 4, 9], [9, 4, 9])])


# ------------------------------------------------------------------ failing frames
def test_failing_frames_in_the_middle(G, world):
    frames, boxes = [x.copy() for x in world["frames"]], list(world["boxes"])
    bad_atom = int(world["idx"][7])
    boxes[5] = None
    frames[12][bad_atom] = np.nan
    s = system_with(G, frames, boxes, world["masses"])
    s.group_create_from_ranges("Peptide", [(int(world["idx"][0]), int(world["idx"][-1]))])
    plan = G.RMSDPlan(s, s, "Peptide", ref_slot=0)
    r, want_st = plan.rmsd(0, 21, raise_on_error=False)
    want_ret = s._lib.gr_rmsd_batch(plan._plan, 0, 21, None, None, None)
    want_idx = int(s._lib.gr_last_error_index(s._ctx))
    assert want_st[5] == E_NO_BOX and want_st[12] == E_NO_POSITION and (np.delete(want_st, [5, 12]) == OK).all()
    p = G.RMSDPanel(s, "Peptide", 21)
    st = np.zeros(21, np.int32)
    ret = s._lib.gr_rmsd_panel_append_batch(p._p, 0, 21, st.ctypes.data_as(C.c_void_p))
    assert ret == want_ret == E_NO_BOX and int(s._lib.gr_last_error_index(s._ctx)) == want_idx
    assert np.array_equal(st, want_st) and np.array_equal(p.status, want_st) and len(p) == 21
    # the frame with the missing position on its own: the index is the atom's, as gr_rmsd_batch reports it
    assert s._lib.gr_rmsd_batch(plan._plan, 12, 1, None, None, None) == E_NO_POSITION
    want_idx = int(s._lib.gr_last_error_index(s._ctx))
    q = G.RMSDPanel(s, "Peptide", 1)
    with pytest.raises(G.RMSDError) as e:
        q.append(12, 1)
    assert e.value.variant == "InvalidPosition" and e.value.detail == want_idx == bad_atom and len(q) == 1
    M = G.rmsd_matrix(p)
    good = np.ones(21, bool); good[[5, 12]] = False
    assert np.isnan(M[~good, :]).all() and np.isnan(M[:, ~good]).all()
    assert same_bits(M[np.ix_(good, good)], world["full"][np.ix_(good, good)])
    assert np.isnan(G.rmsd_matrix(q, p)).all()
    plan.close(); s.close()


# ------------------------------------------------------------------ errors
def test_errors(G, world):
    s = world["s"]
    with pytest.raises(G.RMSDError) as e:
        G.RMSDPanel(s, "Nonexistent", 4)
    assert e.value.variant == "NonexistentGroup"
    s.group_create_from_indices("Nothing", [])
    with pytest.raises(G.RMSDError) as e:
        G.RMSDPanel(s, "Nothing", 4)
    assert e.value.variant == "EmptyGroup"
    p = G.RMSDPanel(s, "Peptide", 4)
    with pytest.raises(G.DeviceError) as e:                           # an empty panel
        G.rmsd_matrix(p)
    assert e.value.status == E_INVALID_ARG
    p.append(0, 3)
    before = G.rmsd_matrix(p)
    with pytest.raises(G.DeviceError) as e:                           # beyond the capacity: nothing changes
        p.append(3, 2)
    assert e.value.status == E_INVALID_ARG and len(p) == 3 and same_bits(G.rmsd_matrix(p), before)
    p.append(3, 1)
    assert len(p) == 4 and same_bits(G.rmsd_matrix(p), world["full"][:4, :4])
    s.group_create_from_ranges("Shorter", [(int(world["idx"][0]), int(world["idx"][-1]) - 1)])
    q = G.RMSDPanel(s, "Shorter", 2)
    q.append(0, 2)
    with pytest.raises(G.RMSDError) as e:                             # panels of different atom counts
        G.rmsd_matrix(p, q)
    assert e.value.variant == "InconsistentGroup" and e.value.detail[1:] == (362, 363)
    # the same atoms with other masses, in a context of their own
    other = world["masses"].copy(); other[int(world["idx"][3])] += F(1.0)
    t = system_with(G, world["frames"][:2], world["boxes"][:2], other)
    t.group_create_from_ranges("Peptide", [(int(world["idx"][0]), int(world["idx"][-1]))])
    u = G.RMSDPanel(t, "Peptide", 2)
    u.append(0, 2)
    with pytest.raises(G.DeviceError) as e:
        G.rmsd_matrix(p, u)
    assert e.value.status == E_INVALID_ARG
    # ... while equal masses from another context are fine
    t.set_masses(world["masses"])
    v = G.RMSDPanel(t, "Peptide", 2)
    v.append(0, 2)
    assert same_bits(G.rmsd_matrix(p, v), world["full"][:4, :2])
    with pytest.raises(G.DeviceError) as e:                           # the panel `u` no longer carries its context's masses
        u.append(0, 1)
    assert e.value.status == E_INVALID_ARG and len(u) == 2
    nomass = world["masses"].copy(); nomass[int(world["idx"][9])] = np.nan
    t.set_masses(nomass)
    with pytest.raises(G.RMSDError) as e:
        G.RMSDPanel(t, "Peptide", 2)
    assert e.value.variant == "InvalidMass" and e.value.detail == int(world["idx"][9])
    t.close()
    p.close(); q.close()


# ------------------------------------------------------------------ history
def test_history_of_the_context_does_not_matter(G, world):
    """a failing call and two other families of calls first: the same bits as the fresh context of `world`"""
    s = system_with(G, world["frames"], world["boxes"], world["masses"])
    s.group_create_from_ranges("Peptide", [(int(world["idx"][0]), int(world["idx"][-1]))])
    s.group_create_from_ranges("Near", [(400, 1400)])
    with pytest.raises(G.RMSDError):
        s.calc_rmsd(s, "Nonexistent", slot=1, ref_slot=0)
    s.group_get_com_batch("Near", 0, 21)
    s.group_pairs_within("Peptide", "Near", 0.5, slot=3)
    plan = G.RMSDPlan(s, s, "Peptide", ref_slot=2)
    plan.rmsd(0, 21)
    plan.close()
    assert same_bits(matrix_of(G, s, "Peptide", list(range(21))), world["full"])
    s.close()

"""atoms_center / atoms_center_mass of the whole system as ONE pass over HBM (gr_resident.h MODE 1, GR_TUNE_CENTER_RESIDENT; utility.rs:109-185):
the same bits as the two passes it replaces (centre estimate, then translate + wrap), the oracle as referee on a sample, and the frames it must
hand back -- an atom without position, a launch that never starts, a launch aborted half way."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def build(G, n, nf, box, seed, spread=0.9):
    rng = np.random.default_rng(seed)
    masses = rng.uniform(1.0, 16.0, n).astype(np.float32)
    s = G.System(n, masses=masses, n_slots=nf)
    L = np.array([box[0], box[1], box[2]], np.float32)
    frames = []
    for f in range(nf):
        # a blob that hangs over the cell's faces (so the wrap has work to do), a few atoms several cells away (the general wrap's turns)
        blob = rng.normal(0, spread, (n, 3)) + rng.uniform(0, 1, 3) * L
        far = rng.integers(0, n, 5)
        blob[far] += rng.integers(-3, 4, (5, 3)) * L
        pos = blob.astype(np.float32)
        s.set_frame(pos, box, slot=f); frames.append(pos)
    return s, frames, masses


def both_ways(G, s, frames, box, group, nf, dim, weighted, **tuning):
    """-> (positions after the resident form, positions after the two passes, statuses of both)"""
    res = {}
    for mode in (1, 0):
        for f in range(nf):
            s.set_frame(frames[f], box, slot=f)
        s.set_tuning(center_resident=mode, **tuning)
        st = s.atoms_center_batch(group, 0, nf, dim, weighted=weighted, raise_on_error=False)
        res[mode] = ([s.get_positions(f) for f in range(nf)], np.array(st))
    return res


@pytest.mark.parametrize("angles", [[90.0, 90.0, 90.0], [60.0, 60.0, 90.0], [75.0, 80.0, 70.0]])
@pytest.mark.parametrize("n,streams", [(20_011, 0), (150_000, 3)])
def test_same_bits_as_the_two_passes(G, angles, n, streams):
    box = O.box_from_lengths_angles([9.0, 8.5, 8.0], angles)
    nf = 21
    s, frames, m = build(G, n, nf, box, 5)
    s.group_create_from_ranges("most", [(7, n - 1 - n // 3)])
    for group, dim, weighted in (("all", G.Dimension.XYZ, True), ("all", G.Dimension.XYZ, False), ("most", G.Dimension.XZ, True), ("most", G.Dimension.Y, False)):
        before = s.stat("center_res_launches")
        res = both_ways(G, s, frames, box, group, nf, dim, weighted, resident=2, resident_streams=streams)
        assert s.stat("center_res_launches") == before + 1, "the resident form was not taken"
        assert (res[1][1] == 0).all() and (res[0][1] == 0).all()
        for f in range(nf):
            assert np.array_equal(res[1][0][f], res[0][0][f]), (group, int(dim), weighted, f, np.abs(res[1][0][f] - res[0][0][f]).max())
    # the oracle on one frame (the reference requires an orthogonal cell)
    if angles == [90.0, 90.0, 90.0]:
        want = O.atoms_center(frames[3], np.arange(n), "xyz", box, mass=m)
        s.set_tuning(center_resident=1, resident=2)
        for f in range(nf):
            s.set_frame(frames[f], box, slot=f)
        s.atoms_center_batch("all", 0, nf, G.Dimension.XYZ, weighted=True)
        assert np.abs(s.get_positions(3) - want).max() < 2e-5
    s.close()


def test_frames_it_hands_back(G):
    """an atom without position inside / outside the reference group, a frame without a box: the launch leaves those frames alone and the two
    passes report them exactly as they always did; every other frame of the batch is moved by the launch"""
    box = O.box_from_lengths_angles([9.0, 8.5, 8.0], [90.0, 90.0, 90.0])
    n, nf = 60_000, 20
    s, frames, m = build(G, n, nf, box, 9)
    s.group_create_from_ranges("half", [(0, n // 2)])
    frames[4] = frames[4].copy(); frames[4][100] = np.nan             # inside the group
    frames[11] = frames[11].copy(); frames[11][n - 5] = np.nan        # outside it
    res = {}
    for mode in (1, 0):
        for f in range(nf):
            s.set_frame(frames[f], box, slot=f)
        s.reset_box(slot=7)                                           # no box
        s.set_tuning(center_resident=mode, resident=2)
        before = s.stat("center_res_redone")
        st = s.atoms_center_batch("half", 0, nf, G.Dimension.XYZ, weighted=True, raise_on_error=False)
        res[mode] = ([s.get_positions(f) for f in range(nf)], np.array(st), s.stat("center_res_redone") - before)
    assert np.array_equal(res[1][1], res[0][1]), (res[1][1], res[0][1])
    assert res[1][1][4] != 0 and res[1][1][11] != 0 and res[1][1][7] != 0 and (np.delete(res[1][1], [4, 7, 11]) == 0).all()
    assert res[1][2] == 2 and res[0][2] == 0
    for f in range(nf):
        assert np.array_equal(res[1][0][f], res[0][0][f], equal_nan=True), f
    s.close()


def test_a_launch_that_never_starts_and_one_that_is_aborted(G):
    box = O.box_from_lengths_angles([9.0, 8.5, 8.0], [60.0, 60.0, 90.0])
    n, nf = 60_000, 40
    s, frames, m = build(G, n, nf, box, 13)
    want = both_ways(G, s, frames, box, "all", nf, G.Dimension.XYZ, True, resident=2)[0]
    # never started: every frame goes through the two passes
    for f in range(nf):
        s.set_frame(frames[f], box, slot=f)
    s.set_tuning(center_resident=1, resident=2, test_resident_no_start=1)
    misses = s.stat("res_handshake_misses")
    st = s.atoms_center_batch("all", 0, nf, G.Dimension.XYZ, weighted=True, raise_on_error=False)
    assert s.stat("res_handshake_misses") == misses + 1 and (np.array(st) == 0).all()
    for f in range(nf):
        assert np.array_equal(s.get_positions(f), want[0][f]), f
    # aborted at frame 17: frames before it are the launch's, the untouched ones are redone; a frame caught half-moved is reported, never silent
    for f in range(nf):
        s.set_frame(frames[f], box, slot=f)
    s.set_tuning(center_resident=1, resident=2, test_resident_abort_at=17, resident_streams=1)
    aborts = s.stat("res_aborts")
    for _ in range(8):      # (the backoff after the miss above makes the context sit out a few batches)
        st = np.array(s.atoms_center_batch("all", 0, nf, G.Dimension.XYZ, weighted=True, raise_on_error=False))
        if s.stat("res_aborts") > aborts:
            break
        for f in range(nf):
            s.set_frame(frames[f], box, slot=f)
        s.set_tuning(test_resident_abort_at=17)
    assert s.stat("res_aborts") == aborts + 1
    for f in range(nf):
        if st[f] == 0:
            assert np.array_equal(s.get_positions(f), want[0][f]), f
    assert (st == 0).sum() >= nf - 8
    s.close()


def test_the_switch_takes_zero_or_one(G):
    s = G.System(100)
    s.set_tuning(center_resident=0); s.set_tuning(center_resident=1)
    with pytest.raises(G.DeviceError):
        s.set_tuning(center_resident=2)
    s.close()


def run_counted(G, s, frames, box, group, nf, dim, weighted, mode, **tuning):
    """one atoms_center_batch over fresh copies of the frames -> (positions, statuses, error index of the call, resident launches, frames
    the launch handed back)"""
    for f in range(nf):
        s.set_frame(frames[f], box, slot=f)
    s.set_tuning(center_resident=mode, **tuning)
    launches, redone = s.stat("center_res_launches"), s.stat("center_res_redone")
    st = np.array(s.atoms_center_batch(group, 0, nf, dim, weighted=weighted, raise_on_error=False))
    idx = int(s._lib.gr_last_error_index(s._ctx))
    return ([s.get_positions(f) for f in range(nf)], st, idx, s.stat("center_res_launches") - launches, s.stat("center_res_redone") - redone)


def test_every_frame_handed_back_for_a_massless_atom(G):
    """a weighted centre whose (contiguous) reference group holds an atom without mass: the launch hands back EVERY frame and no frame failed
    a host check -- the two passes must then report the reference's MassError with the atom's index, not the launch's internal status"""
    box = O.box_from_lengths_angles([9.0, 8.5, 8.0], [90.0, 90.0, 90.0])
    n, nf, bad = 60_000, 12, 12_345
    s, frames, m = build(G, n, nf, box, 17)
    m = m.copy(); m[bad] = np.nan
    s.set_masses(m)
    s.group_create_from_ranges("half", [(0, n // 2)])
    res = {mode: run_counted(G, s, frames, box, "half", nf, G.Dimension.XYZ, True, mode, resident=2) for mode in (1, 0)}
    assert res[1][3] == 1 and res[1][4] == nf, "the resident launch did not run, or did not hand every frame back"
    assert res[0][3] == 0
    assert (res[1][1] == G._lib.E_NO_MASS).all(), res[1][1]
    assert np.array_equal(res[1][1], res[0][1]) and res[1][2] == res[0][2] == bad
    for f in range(nf):
        assert np.array_equal(res[1][0][f], frames[f]) and np.array_equal(res[0][0][f], frames[f]), f      # failed frames are untouched
    # the raising call names the atom, whichever path takes it
    for mode in (1, 0):
        for f in range(nf):
            s.set_frame(frames[f], box, slot=f)
        s.set_tuning(center_resident=mode, resident=2)
        launches = s.stat("center_res_launches")
        with pytest.raises(G.GroupError) as e:
            s.atoms_center_batch("half", 0, nf, G.Dimension.XYZ, weighted=True)
        assert e.value.variant == "InvalidMass" and e.value.detail == bad and s.stat("center_res_launches") == launches + mode
    # the same masses, unweighted: masses are not read, the launch moves every frame itself
    res = {mode: run_counted(G, s, frames, box, "half", nf, G.Dimension.XYZ, False, mode, resident=2) for mode in (1, 0)}
    assert res[1][3] == 1 and res[1][4] == 0
    assert (res[1][1] == 0).all() and (res[0][1] == 0).all(), (res[1][1], res[0][1])
    for f in range(nf):
        assert np.array_equal(res[1][0][f], res[0][0][f]), (f, np.abs(res[1][0][f] - res[0][0][f]).max())
        assert not np.array_equal(res[1][0][f], frames[f])
    s.close()


def test_every_frame_handed_back_for_atoms_without_position(G):
    """every frame holds one atom without position -- inside the reference group in some frames, outside it in others: every frame is handed
    back, and each must report GR_E_NO_POSITION with its own atom's index, as the two passes do"""
    box = O.box_from_lengths_angles([9.0, 8.5, 8.0], [90.0, 90.0, 90.0])
    n, nf = 60_000, 10
    s, frames, m = build(G, n, nf, box, 23)
    s.group_create_from_ranges("half", [(0, n // 2)])
    rng = np.random.default_rng(23)
    nan_at = [int(rng.integers(0, n // 2)) if f % 2 == 0 else int(rng.integers(n // 2 + 1, n)) for f in range(nf)]   # inside / outside
    for f in range(nf):
        frames[f] = frames[f].copy(); frames[f][nan_at[f]] = np.nan
    res = {mode: run_counted(G, s, frames, box, "half", nf, G.Dimension.XYZ, True, mode, resident=2) for mode in (1, 0)}
    assert res[1][3] == 1 and res[1][4] == nf, "the resident launch did not run, or did not hand every frame back"
    assert (res[1][1] == G._lib.E_NO_POSITION).all(), res[1][1]
    assert np.array_equal(res[1][1], res[0][1]) and res[1][2] == res[0][2] == nan_at[0]
    for f in range(nf):
        assert np.array_equal(res[1][0][f], res[0][0][f], equal_nan=True), f
    # each frame's own index: one frame per call, the launch forced on every one
    for f in range(nf):
        for mode in (1, 0):
            s.set_frame(frames[f], box, slot=f)
            s.set_tuning(center_resident=mode, resident=2)
            launches = s.stat("center_res_launches")
            with pytest.raises(G.GroupError) as e:
                s.atoms_center_batch("half", f, 1, G.Dimension.XYZ, weighted=True)
            assert e.value.variant == "InvalidPosition" and e.value.detail == nan_at[f], (f, mode, e.value.detail)
            assert s.stat("center_res_launches") == launches + mode
    s.close()


def test_a_launch_aborted_before_any_frame_finished(G):
    """frame 0's finalizer aborts the launch and no frame failed a host check -- in a batch of 20 frames and in a batch of that one frame,
    where nothing can have finished: the frames not finished go through the two passes, and no internal status (GR_ST_FALLBACK 100,
    GR_ST_ABORTED 102) reaches the caller"""
    box = O.box_from_lengths_angles([9.0, 8.5, 8.0], [60.0, 60.0, 90.0])
    n, nf = 60_000, 20
    s, frames, m = build(G, n, nf, box, 29)
    for nb in (nf, 1):
        want = run_counted(G, s, frames, box, "all", nb, G.Dimension.XYZ, True, 0)
        assert (want[1] == 0).all() and want[3] == 0
        aborts = s.stat("res_aborts")
        got = run_counted(G, s, frames, box, "all", nb, G.Dimension.XYZ, True, 1, resident=2, resident_streams=1, test_resident_abort_at=0)
        assert got[3] == 1 and s.stat("res_aborts") == aborts + 1, "the resident launch did not run, or was not aborted"
        assert not np.isin(got[1], [100, 102]).any(), (nb, got[1])
        assert np.isin(got[1], [0, G._lib.E_HIP]).all(), (nb, got[1])           # (a frame caught half-moved is reported, never silent)
        for f in range(nb):
            if got[1][f] == 0:
                assert np.array_equal(got[0][f], want[0][f]), (nb, f)
        assert (got[1] == 0).sum() >= nb - 8
    s.close()

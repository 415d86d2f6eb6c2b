"""The call path round the resident pass (gr_resident.h, gr_api.hip): no kernel zeroes anything before a launch (the handshake words
describe themselves, the finalizers start from fresh states when every frame passed the host's checks), one kernel behind the launch
hands states and control words to the host through mapped memory, and the host polls its sequence word instead of synchronising the
stream.  What has to hold: many launches back to back of changing shape, of both forms (RMSD-fit, atoms_center) and from two contexts
give the two-pass path's results; a segment with failed frames does not take the elided reset; a launch that never starts and a
launch that is aborted are redone and leave nothing behind that the next launch could trip over; the profiling events of a lean
segment are readable.  The pass is forced (GR_TUNE_RESIDENT = 2) for systems far smaller than the chip, as in test_gpu_resident.py."""
import numpy as np
import pytest

from groan_rs_amd import workload as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def _systems(G, n, nf, box, seed=W.SEED):
    masses = W.masses_cycle(n)
    cur = G.System(n, masses=masses, n_slots=nf + 1)
    cur.synth_reference(nf, box, 0.2 * min(box[0], box[1], box[2]), seed)
    cur.synth_frames(nf, 0, nf, 0, 0.04, seed)
    ref = G.System(n, masses=masses, box=box, positions=cur.get_positions(nf))
    frames = [cur.get_positions(f) for f in range(nf)]
    return cur, ref, frames


def _load(s, frames, box, nb):
    for f in range(nb):
        s.set_frame(frames[f], box, slot=f)


def test_sixty_segments_back_to_back(G):
    """60 segments of 1, 7, 64 and 200 frames in turn, RMSD-fit and atoms_center interleaved on one context, a second context's launches in
    between: every result is the two-pass path's (RMSD within 2e-6 nm, fitted coordinates within 2e-5 nm as in test_gpu_resident.py; the
    centred coordinates bit for bit as in test_gpu_center_resident.py), no abort, no missed handshake, every launch lean, no poll gave up."""
    n, counts = 20_000, (1, 7, 64, 200)
    box = W.box_from_lengths_angles([6.0, 6.0, 6.0], [60.0, 60.0, 90.0])
    obox = W.box_from_lengths_angles([6.0, 6.2, 5.8], [90.0, 90.0, 90.0])
    cur, ref, frames = _systems(G, n, max(counts), box)
    other, oref, oframes = _systems(G, 9_000, 7, obox, seed=W.SEED + 1)
    plan, oplan = G.RMSDPlan(ref, cur, "all"), G.RMSDPlan(oref, other, "all")
    check = {1: [0], 7: [0, 6], 64: [0, 31, 63], 200: [0, 77, 199]}
    want = {}
    cur.set_tuning(resident=0, center_resident=0)
    other.set_tuning(resident=0)
    for nb in counts:
        _load(cur, frames, box, nb)
        r, st = plan.rmsd_fit(0, nb)
        assert (st == 0).all()
        want[("fit", nb)] = (np.array(r), {f: cur.get_positions(f) for f in check[nb]})
        _load(cur, frames, box, nb)
        st = cur.atoms_center_batch("all", 0, nb, G.Dimension.XYZ, weighted=True)
        assert (np.array(st) == 0).all()
        want[("cen", nb)] = {f: cur.get_positions(f) for f in check[nb]}
    _load(other, oframes, obox, 7)
    owant, st = oplan.rmsd_fit(0, 7)
    owant = np.array(owant)
    cur.set_tuning(resident=2, center_resident=1)
    other.set_tuning(resident=2)
    segments = 0
    for k in range(60):
        nb = counts[k % 4]
        _load(cur, frames, box, nb)
        if (k // 4) % 2 == 0:
            r, st = plan.rmsd_fit(0, nb)
            assert (st == 0).all(), (k, st)
            assert np.abs(np.array(r) - want[("fit", nb)][0]).max() <= 2e-6, (k, nb)
            for f in check[nb]:
                assert np.abs(cur.get_positions(f) - want[("fit", nb)][1][f]).max() <= 2e-5, (k, nb, f)
        else:
            st = cur.atoms_center_batch("all", 0, nb, G.Dimension.XYZ, weighted=True)
            assert (np.array(st) == 0).all(), (k, st)
            for f in check[nb]:
                assert np.array_equal(cur.get_positions(f), want[("cen", nb)][f]), (k, nb, f)
        segments += 1
        if k % 5 == 2:
            _load(other, oframes, obox, 7)
            r, st = oplan.rmsd_fit(0, 7)
            assert (st == 0).all() and np.abs(np.array(r) - owant).max() <= 2e-6, k
    for s, n_seg in ((cur, segments), (other, 12)):
        assert s.stat("res_aborts") == 0 and s.stat("res_handshake_misses") == 0 and s.stat("res_redone_frames") == 0
        assert s.stat("res_launches") + s.stat("center_res_launches") == n_seg, (s.stat("res_launches"), s.stat("center_res_launches"), n_seg)
        assert s.stat("res_lean_segments") == n_seg
        assert s.stat("res_sync_fallbacks") == 0
    plan.close(); oplan.close(); ref.close(); oref.close(); cur.close(); other.close()


def test_failed_frames_do_not_take_the_elided_reset(G):
    """a frame without a box (fails the host's checks) and a frame with a NaN atom in one segment: statuses, error indices and the
    untouched coordinates are the two-pass path's, the other frames are fitted, and the launch is not counted as lean"""
    n, nf = 20_000, 9
    box = W.box_from_lengths_angles([6.0, 6.0, 6.0], [90.0, 90.0, 90.0])
    cur, ref, frames = _systems(G, n, nf, box)
    plan = G.RMSDPlan(ref, cur, "all")
    bad = frames[5].copy(); bad[4321] = np.nan
    res = {}
    for mode in (0, 2):
        cur.set_tuning(resident=mode)
        for f in range(nf):
            cur.set_frame(bad if f == 5 else frames[f], box, slot=f)
        cur.reset_box(slot=2)
        launches = cur.stat("res_launches")
        r, st = plan.rmsd_fit(0, nf, raise_on_error=False)
        res[mode] = (np.array(r), np.array(st), cur._err(0)[2], [cur.get_positions(f) for f in range(nf)])
        assert cur.stat("res_launches") - launches == (1 if mode == 2 else 0)
    assert cur.stat("res_lean_segments") == 0
    assert np.array_equal(res[0][1], res[2][1]) and res[2][1][2] == G._lib.E_NO_BOX and res[2][1][5] == G._lib.E_NO_POSITION, (res[0][1], res[2][1])
    assert res[0][2] == res[2][2]
    assert np.array_equal(res[2][3][2], frames[2]) and np.array_equal(np.nan_to_num(res[2][3][5], nan=-1.0), np.nan_to_num(bad, nan=-1.0))
    for f in range(nf):
        if f in (2, 5):
            continue
        assert abs(res[0][0][f] - res[2][0][f]) <= 2e-6, f
        assert np.abs(res[0][3][f] - res[2][3][f]).max() <= 2e-5, f
    # ... and the same segment with every frame in order right behind it is lean again
    _load(cur, frames, box, nf)
    r, st = plan.rmsd_fit(0, nf)
    assert (st == 0).all() and cur.stat("res_lean_segments") == 1
    plan.close(); ref.close(); cur.close()


@pytest.mark.parametrize("hook", ["no_start", "abort"])
def test_a_hooked_segment_and_the_ordinary_one_behind_it(G, hook):
    """the project's two bounded test hooks -- a launch that finds its verdict already "never started", a launch whose finalizer raises
    `abort` at frame 9 -- each followed at once by an ordinary segment on the same context: the hooked segment is redone correctly and the
    next launch of the pass runs to the end, although no kernel has cleared a handshake word, a progress word or a frame state in between"""
    n, nf = 20_000, 24
    box = W.box_from_lengths_angles([6.0, 6.0, 6.0], [60.0, 60.0, 90.0])
    cur, ref, frames = _systems(G, n, nf, box)
    plan = G.RMSDPlan(ref, cur, "all")
    cur.set_tuning(resident=0)
    _load(cur, frames, box, nf)
    want_r, st = plan.rmsd_fit(0, nf)
    want_r, want = np.array(want_r), [cur.get_positions(f) for f in range(nf)]
    # an ordinary launch first: the hooked one meets the words a launch leaves behind
    cur.set_tuning(resident=2)
    _load(cur, frames, box, nf)
    r, st = plan.rmsd_fit(0, nf)
    assert (st == 0).all() and cur.stat("res_launches") == 1
    if hook == "no_start":
        cur.set_tuning(resident=2, test_resident_no_start=1)
    else:
        cur.set_tuning(resident=2, test_resident_abort_at=9)
    _load(cur, frames, box, nf)
    r, st = plan.rmsd_fit(0, nf)
    assert (st == 0).all(), st
    assert np.abs(np.array(r) - want_r).max() <= 2e-6
    for f in range(nf):
        assert np.abs(cur.get_positions(f) - want[f]).max() <= 2e-5, f
    if hook == "no_start":
        assert cur.stat("res_handshake_misses") == 1 and cur.stat("res_aborts") == 0 and cur.stat("res_launches") == 1
    else:
        assert cur.stat("res_aborts") == 1 and cur.stat("res_handshake_misses") == 0 and cur.stat("res_launches") == 1
        assert 1 <= cur.stat("res_redone_frames") <= nf - 9
    # the next launch of the pass (after a miss the context sits out four segments first: those take the two passes)
    launches, tries = cur.stat("res_launches"), 0
    while cur.stat("res_launches") == launches and tries < 6:
        _load(cur, frames, box, nf)
        r, st = plan.rmsd_fit(0, nf)
        assert (st == 0).all(), (tries, st)
        assert np.abs(np.array(r) - want_r).max() <= 2e-6, tries
        tries += 1
    assert cur.stat("res_launches") == launches + 1 and tries == (5 if hook == "no_start" else 1), tries
    for f in range(nf):
        assert np.abs(cur.get_positions(f) - want[f]).max() <= 2e-5, f
    assert cur.stat("res_handshake_misses") == (1 if hook == "no_start" else 0) and cur.stat("res_aborts") == (0 if hook == "no_start" else 1)
    assert cur.stat("res_sync_fallbacks") == 0
    plan.close(); ref.close(); cur.close()


def test_profile_read_after_a_lean_segment(G):
    n, nf = 20_000, 12
    box = W.box_from_lengths_angles([6.0, 6.0, 6.0], [90.0, 90.0, 90.0])
    cur, ref, frames = _systems(G, n, nf, box)
    plan = G.RMSDPlan(ref, cur, "all")
    cur.set_tuning(resident=2)
    cur.profile_enable(True)
    _load(cur, frames, box, nf)
    r, st = plan.rmsd_fit(0, nf)
    prof = cur.profile_read()
    assert (st == 0).all() and cur.stat("res_lean_segments") == 1
    assert prof["k_fit_resident"][1] == 1 and prof["k_fit_resident"][0] > 0.0 and prof["k_fit_resident"][2] == nf, prof
    plan.close(); ref.close(); cur.close()

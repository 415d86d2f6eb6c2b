"""The kernel behind a resident launch (k_res_close, gr_resident.h): every frame's wave closes its state in device memory and counts
itself; the wave that completes the count copies the whole block of states and the control words to the host in one go and stores the
sequence word the host polls.  What has to hold: frame counts on both sides of every edge of that copy (an odd count, whose block does
not end on 16 bytes; one frame, whose only wave is also the last; a wave's worth of frames and its neighbours; the full block of
GR_MAX_BATCH frames) give the two-pass path's statuses and results; a short call behind a long one shows nothing of the long one's
states; frames that fail at the first and last position, a launch that never starts and a launch aborted in its last frames end as they
do on the two-pass path; two contexts taking turns never see one another's states.  The reference is always the two-pass path
(GR_TUNE_RESIDENT = 0) on fresh copies of the same frames; tolerances as in test_gpu_resident_call_path.py: rmsd 2e-6 nm, fitted
coordinates 2e-5 nm, centred coordinates bit for bit.  The pass is forced (GR_TUNE_RESIDENT = 2) for a system far smaller than the chip."""
import numpy as np
import pytest

from groan_rs_amd import workload as W

pytestmark = pytest.mark.gpu

N_ATOMS, N_FRAMES = 20_000, 1024      # N_FRAMES = GR_MAX_BATCH
BOX = W.box_from_lengths_angles([6.0, 6.0, 6.0], [60.0, 60.0, 90.0])


class _Bench:
    """one context with N_FRAMES synthetic frames kept on the host, its plan, and the two-pass results of every set of frames asked for"""

    def __init__(self, G, n=N_ATOMS, nf=N_FRAMES, box=BOX, seed=W.SEED):
        masses = W.masses_cycle(n)
        self.G, self.box, self.nf = G, box, nf
        self.cur = G.System(n, masses=masses, n_slots=nf + 1)
        self.cur.synth_reference(nf, box, 0.2 * min(box[0], box[1], box[2]), seed)
        self.cur.synth_frames(nf, 0, nf, 0, 0.04, seed)
        self.ref = G.System(n, masses=masses, box=box, positions=self.cur.get_positions(nf))
        self.frames = [self.cur.get_positions(f) for f in range(nf)]
        self.plan = G.RMSDPlan(self.ref, self.cur, "all")
        self._want = {}

    def load(self, idx):
        for slot, f in enumerate(idx):
            self.cur.set_frame(self.frames[f], self.box, slot=slot)

    @staticmethod
    def slots_checked(nb):
        return sorted({0, nb // 2, nb - 1})

    def want(self, kind, idx):
        """the two-pass path on fresh copies of frames `idx`: (rmsd of every frame | None, coordinates of the first, middle and last slot)"""
        key = (kind, tuple(idx))
        if key not in self._want:
            nb = len(idx)
            self.cur.set_tuning(resident=0, center_resident=0)
            self.load(idx)
            if kind == "fit":
                r, st = self.plan.rmsd_fit(0, nb)
                r = np.array(r)
            else:
                st, r = self.cur.atoms_center_batch("all", 0, nb, self.G.Dimension.XYZ, weighted=True), None
            assert (np.array(st) == 0).all()
            self._want[key] = (r, {s: self.cur.get_positions(s) for s in self.slots_checked(nb)})
            self.cur.set_tuning(resident=2, center_resident=1)
        return self._want[key]

    def run_and_check(self, kind, idx, tag=None):
        """the resident pass on fresh copies of frames `idx`, against want()"""
        nb, cur = len(idx), self.cur
        want_r, want_x = self.want(kind, idx)
        cur.set_tuning(resident=2, center_resident=1)
        self.load(idx)
        launches = cur.stat("res_launches") + cur.stat("center_res_launches")
        quiet = [cur.stat(k) for k in ("res_sync_fallbacks", "res_aborts", "res_handshake_misses")]
        if kind == "fit":
            r, st = self.plan.rmsd_fit(0, nb)
            assert (np.array(st) == 0).all(), (tag, nb, st)
            assert np.abs(np.array(r) - want_r).max() <= 2e-6, (tag, nb)
            for s in self.slots_checked(nb):
                assert np.abs(cur.get_positions(s) - want_x[s]).max() <= 2e-5, (tag, nb, s)
        else:
            st = cur.atoms_center_batch("all", 0, nb, self.G.Dimension.XYZ, weighted=True)
            assert (np.array(st) == 0).all(), (tag, nb, st)
            for s in self.slots_checked(nb):
                assert np.array_equal(cur.get_positions(s), want_x[s]), (tag, nb, s)
        assert cur.stat("res_launches") + cur.stat("center_res_launches") == launches + 1, (tag, nb)      # (the pass took the call)
        assert [cur.stat(k) for k in ("res_sync_fallbacks", "res_aborts", "res_handshake_misses")] == quiet, (tag, nb)

    def close(self):
        self.plan.close(); self.ref.close(); self.cur.close()


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.fixture(scope="module")
def bench(G):
    b = _Bench(G)
    yield b
    b.close()


def _frames_of(nb):
    """`nb` frames starting somewhere else for every count: a state left from another call is never the right answer"""
    off = (nb * 37) % N_FRAMES
    return [(off + k) % N_FRAMES for k in range(nb)]


@pytest.mark.parametrize("nb", [1, 2, 3, 63, 64, 65, 257, 1024])
def test_rmsd_fit_frame_counts(bench, nb):
    """every status and every rmsd of a call of `nb` frames, and the fitted coordinates of its first, middle and last frame"""
    bench.run_and_check("fit", _frames_of(nb))


@pytest.mark.parametrize("nb", [1, 3, 65, 257])
def test_atoms_center_frame_counts(bench, nb):
    bench.run_and_check("cen", _frames_of(nb))


def test_a_long_call_then_short_ones(bench):
    """257 frames, then 3, then 65 on the same context, each of frames of its own: the statuses and rmsds of the later calls are their
    own frames', not what the longer call left in the block of states"""
    for nb, first in ((257, 500), (3, 40), (65, 900)):
        bench.run_and_check("fit", [(first + k) % N_FRAMES for k in range(nb)], tag="long-short")


@pytest.mark.parametrize("no_box_at, nan_at", [(0, 64), (64, 0)])
def test_failing_frames_at_the_first_and_last_position(bench, no_box_at, nan_at):
    """a frame without a box and a frame with a NaN atom at the two ends of a 65-frame call: status, error index and the untouched
    coordinates equal the two-pass path's, and the call is not counted as lean"""
    nb, cur = 65, bench.cur
    idx = _frames_of(nb)
    gave_up = cur.stat("res_sync_fallbacks")
    bad = bench.frames[idx[nan_at]].copy(); bad[4321] = np.nan
    res = {}
    for mode in (0, 2):
        cur.set_tuning(resident=mode, center_resident=1)
        bench.load(idx)
        cur.set_frame(bad, bench.box, slot=nan_at)
        cur.reset_box(slot=no_box_at)
        launches, lean = cur.stat("res_launches"), cur.stat("res_lean_segments")
        r, st = bench.plan.rmsd_fit(0, nb, raise_on_error=False)
        res[mode] = (np.array(r), np.array(st), cur._err(0)[2], [cur.get_positions(f) for f in range(nb)])
        assert cur.stat("res_launches") - launches == (1 if mode == 2 else 0)
        assert cur.stat("res_lean_segments") == lean
    L = bench.G._lib
    assert np.array_equal(res[0][1], res[2][1]), (res[0][1], res[2][1])
    assert res[2][1][no_box_at] == L.E_NO_BOX and res[2][1][nan_at] == L.E_NO_POSITION
    assert (np.delete(res[2][1], [no_box_at, nan_at]) == 0).all()
    assert res[0][2] == res[2][2]
    assert np.array_equal(res[2][3][no_box_at], bench.frames[idx[no_box_at]])
    assert np.array_equal(np.nan_to_num(res[2][3][nan_at], nan=-1.0), np.nan_to_num(bad, nan=-1.0))
    for f in range(nb):
        if f in (no_box_at, nan_at):
            continue
        assert abs(res[0][0][f] - res[2][0][f]) <= 2e-6, f
        assert np.abs(res[0][3][f] - res[2][3][f]).max() <= 2e-5, f
    assert cur.stat("res_sync_fallbacks") == gave_up


@pytest.mark.parametrize("hook", ["no_start", "abort_at_62", "abort_at_63", "abort_at_64"])
def test_hooked_calls_of_65_frames(bench, hook):
    """the project's two test hooks -- a launch that finds its verdict "never started", a launch whose finalizer raises `abort` in one of
    the last three frames -- on a 65-frame call: the call is redone correctly, no poll gave up, and the next ordinary call of the pass
    (after a miss the context sits out four calls first, which take the two passes) is correct"""
    nb, cur = 65, bench.cur
    idx = _frames_of(nb)
    want_r, want_x = bench.want("fit", idx)
    cur.set_tuning(resident=2, center_resident=1)
    before = {k: cur.stat(k) for k in ("res_launches", "res_aborts", "res_handshake_misses", "res_redone_frames", "res_sync_fallbacks")}
    if hook == "no_start":
        cur.set_tuning(test_resident_no_start=1)
    else:
        cur.set_tuning(test_resident_abort_at=int(hook.rsplit("_", 1)[1]))
    bench.load(idx)
    r, st = bench.plan.rmsd_fit(0, nb)
    assert (np.array(st) == 0).all(), st
    assert np.abs(np.array(r) - want_r).max() <= 2e-6
    for s in bench.slots_checked(nb):
        assert np.abs(cur.get_positions(s) - want_x[s]).max() <= 2e-5, s
    assert cur.stat("res_launches") == before["res_launches"]
    if hook == "no_start":
        assert cur.stat("res_handshake_misses") == before["res_handshake_misses"] + 1 and cur.stat("res_aborts") == before["res_aborts"]
    else:
        assert cur.stat("res_aborts") == before["res_aborts"] + 1 and cur.stat("res_handshake_misses") == before["res_handshake_misses"]
        assert 1 <= cur.stat("res_redone_frames") - before["res_redone_frames"] <= nb - int(hook.rsplit("_", 1)[1])
    assert cur.stat("res_sync_fallbacks") == before["res_sync_fallbacks"]
    launches, tries = cur.stat("res_launches"), 0
    while cur.stat("res_launches") == launches and tries < 6:
        bench.load(idx)
        r, st = bench.plan.rmsd_fit(0, nb)
        assert (np.array(st) == 0).all(), (tries, st)
        assert np.abs(np.array(r) - want_r).max() <= 2e-6, tries
        tries += 1
    assert cur.stat("res_launches") == launches + 1 and tries == (5 if hook == "no_start" else 1), tries
    for s in bench.slots_checked(nb):
        assert np.abs(cur.get_positions(s) - want_x[s]).max() <= 2e-5, s
    assert cur.stat("res_sync_fallbacks") == before["res_sync_fallbacks"]


def test_two_contexts_taking_turns(G):
    """30 calls, two contexts of their own in turn, frame counts and frames changing from call to call: every result is the two-pass
    path's, no poll gave up and nothing was aborted on either context"""
    obox = W.box_from_lengths_angles([6.0, 6.2, 5.8], [90.0, 90.0, 90.0])
    one, other = _Bench(G, nf=140), _Bench(G, n=9_000, nf=70, box=obox, seed=W.SEED + 1)
    try:
        for k in range(30):
            b, nb = (one, (65, 3, 130)[(k // 2) % 3]) if k % 2 == 0 else (other, (7, 64, 1)[(k // 2) % 3])
            b.run_and_check("fit", [(11 * k + j) % b.nf for j in range(nb)], tag=k)
        for b in (one, other):
            assert b.cur.stat("res_sync_fallbacks") == 0 and b.cur.stat("res_aborts") == 0 and b.cur.stat("res_handshake_misses") == 0
            assert b.cur.stat("res_launches") == 15
    finally:
        one.close(); other.close()

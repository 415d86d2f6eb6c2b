"""The two device readers share one pair of staging banks (gr_api.hip: ingest_acquire / ingest_submit).  Here they alternate on ONE
context with no gr_sync in between, every read larger than the one that last used its bank (so both halves of the bank grow under
the copies and kernels still queued), one of them group-limited: what arrives in the slots must equal the host readers bit for bit,
boxes included, and a group-limited read must leave the atoms outside its group as the read before it left them.  gr_frame_get_box reads
the host's copy of a box; the copy on the device, which the unpack stream writes behind the kernels that still read the slot, is seen
through a call that needs it: the minimum-image distances inside the group equal those of a fresh context given the same frame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NF = 300, 8                # (above the 9 atoms an xtc frame stores uncompressed)
GROUP = (100, 199)            # 100 atoms in the middle of the system


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def test_xtc_and_trr_reads_alternate_on_growing_banks(G, tmp_path):
    rng = np.random.default_rng(20261018)
    xtc_path, trr_path = str(tmp_path / "mixed.xtc"), str(tmp_path / "mixed.trr")
    with G.XtcWriter(xtc_path) as wx, G.TrrWriter(trr_path) as wt:
        for f in range(NF):
            L = np.array([5.0 + 0.1 * f, 6.0 - 0.05 * f, 7.0 + 0.2 * f], np.float32)      # every frame its own box
            box9 = np.array([L[0], L[1], L[2], 0, 0, 0, 0, 0, 0], np.float32)
            x = (rng.uniform(-0.2, 1.2, (N, 3)) * L).astype(np.float32)
            if f == 1:
                x[5] = 0.0                                                              # trr: an atom without position, outside the group
            wx.write_frame(x, box9, step=10 * f, time=0.5 * f)
            wt.write_frame(x, box9, step=10 * f, time=0.5 * f)
    xf, tf = G.XtcFile(xtc_path), G.TrrFile(trr_path)
    assert xf.n_frames == tf.n_frames == NF and xf.n_atoms == tf.n_atoms == N

    def host(reader, frame):
        """-> (positions with NaN rows for missing positions, box9, step, time) as the host reader gives them"""
        if reader == "xtc":
            x, box9, step, time, _ = xf.read_frame(frame)
            return x.copy(), box9, step, time
        x, _, _, box9, step, time, _ = tf.read_frame(frame)
        x = x.copy()
        x[~x.any(axis=1)] = np.nan                                                     # (trr_io.rs:108-112: all-zero = no position)
        return x, box9, step, time

    s = G.System(N, n_slots=NF)
    s.group_create_from_ranges("middle", [GROUP])
    fresh = G.System(N, n_slots=1)
    fresh.group_create_from_ranges("middle", [GROUP])
    inside = np.zeros(N, bool); inside[GROUP[0]:GROUP[1] + 1] = True
    held = [None] * NF                                                                 # what every slot should hold
    # (reader, first frame, frames, group): each read is larger than the last one on its bank (the banks take the calls in turn)
    plan = [("xtc", 0, 1, None), ("trr", 1, 3, None), ("xtc", 4, 2, "middle"), ("trr", 1, 7, None), ("xtc", 0, 8, None)]
    for step_no, (reader, f0, nf, group) in enumerate(plan):
        if reader == "xtc":
            steps, times = xf.read_frames_device(s, f0, nf, group=group)
        else:
            steps, times = tf.read_frames_device(s, f0, nf)
        for k in range(nf):
            x, box9, step, time = host(reader, f0 + k)
            if group is None:
                held[k] = x
            else:
                assert held[k] is not None
                held[k] = np.where(inside[:, None], x, held[k])
            got = s.get_positions(k)
            ok = ~np.isnan(held[k][:, 0])                                              # (bit for bit; a missing position is NaN in x, y and z)
            assert np.array_equal(got[ok].view(np.uint32), held[k][ok].view(np.uint32)), (step_no, k)
            assert np.isnan(got[~ok]).all(), (step_no, k)
            assert np.array_equal(s.get_box(k), box9), (step_no, k)
            assert int(steps[k]) == step and times[k] == np.float32(time), (step_no, k)
            fresh.set_frame(held[k], box9, slot=0)                                      # (the box on the device: wrong, and distances across the cell differ)
            assert np.array_equal(s.group_all_distances("middle", "middle", slot=k), fresh.group_all_distances("middle", "middle", slot=0)), (step_no, k)
        if group is not None:
            # the atoms outside the group are still the trr frames of the read before -- the missing position among them
            for k in range(nf):
                before = host("trr", 1 + k)[0]
                got = s.get_positions(k)
                assert np.array_equal(got[~inside], before[~inside], equal_nan=True), k
            assert np.isnan(s.get_positions(0)[5]).all()
    s.close(); fresh.close(); xf.close(); tf.close()

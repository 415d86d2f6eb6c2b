"""A context's grow-only workspaces (gr_buf.h) across calls: a call that finds the block of an earlier, smaller call must replace it and
compute what it computes on a fresh context.  The pair-distance output (16 floats from gr_atoms_distance, then 40 x 50, then
200 x 300 distances) and the device xtc encoder's scratch and pinned banks (8 slots, then 24)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def test_pair_distance_output_grows_across_calls(G):
    n = 2000
    rng = np.random.default_rng(7)
    box9 = np.array([4.0, 5.0, 6.0, 0, 0, 0, 0, 0, 0], np.float32)
    x = (rng.uniform(-0.1, 1.1, (n, 3)) * box9[:3]).astype(np.float32)
    groups = {"a40": (10, 49), "b50": (1000, 1049), "a200": (300, 499), "b300": (1500, 1799)}

    def system():
        s = G.System(n, n_slots=1)
        s.set_frame(x, box9, slot=0)
        for name, r in groups.items():
            s.group_create_from_ranges(name, [r])
        return s

    calls = [lambda s: np.float32(s.atoms_distance(3, 1777)), lambda s: s.group_all_distances("a40", "b50"), lambda s: s.group_all_distances("a200", "b300")]
    fresh = []
    for call in calls:                                       # every call on a context of its own
        s = system(); fresh.append(call(s)); s.close()
    assert fresh[1].shape == (40, 50) and fresh[2].shape == (200, 300) and np.isfinite(fresh[2]).all() and fresh[0] > 0
    s = system()
    for k, call in enumerate(calls):                         # ... and in a row on one
        got = call(s)
        assert np.array_equal(np.asarray(got).view(np.uint32), np.asarray(fresh[k]).view(np.uint32)), k
    s.close()


def test_device_xtc_encoder_grows_across_calls(G, tmp_path):
    """8 slots, then 24 on the same context: the second call finds every scratch block too small, and -- the stream of these frames
    takes more than the 4 bytes per atom the pinned bank starts with -- grows the bank once more with its head kept"""
    n, nf = 25_000, 24
    rng = np.random.default_rng(11)
    box9 = np.array([30, 30, 30, 0, 0, 0, 0, 0, 0], np.float32)
    s = G.System(n, n_slots=nf)
    for f in range(nf):
        s.set_frame(rng.uniform(0, 30.0, (n, 3)).astype(np.float32), box9, slot=f)      # (a gas: no atom near its neighbour, ~5.6 bytes per atom)
    out = {}
    for device in (1, 0):
        s.set_tuning(xtc_device_encode=device)
        took = [s.stat("xtc_device_frames")]
        for count in (8, 24):
            path = tmp_path / ("grow_%d_%d.xtc" % (count, device))
            with G.XtcWriter(path) as w:
                w.write_slots(s, 0, count, steps=np.arange(count, dtype=np.int64) * 10, times=np.arange(count, dtype=np.float32) * 0.5, host_threads=2)
            took.append(s.stat("xtc_device_frames"))
            out[(count, device)] = open(path, "rb").read()
        assert np.diff(took).tolist() == ([8, 24] if device else [0, 0]), (device, took)
    s.close()
    for count in (8, 24):
        assert out[(count, 1)] == out[(count, 0)], count
        assert len(out[(count, 1)]) > count * (92 + 4 * n), count     # (the stream did outgrow the bank's first size: the keep-head path ran)

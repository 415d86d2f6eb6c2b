"""MSD (gr_msd_*) at the smallest shapes that can go wrong, every case against the numpy restatement tests/msd_ref.py: displacements bit
for bit, the curve under the derived bound of tests/test_gpu_msd.py, and itself bit for bit under another launch setting.
  group sizes   1, 15, 16, 17 (a tile of the matrix instruction), 63, 64, 65 (the wave and the pad of the panel), 257; the block starts
                at atom 2, not a multiple of 4
  frame counts  1, 2, AHEAD - 1, AHEAD, AHEAD + 1 (the ring of rows in flight), 63, 64, 65, 129 (the blocks of the Gram matrix), each in
                an object whose capacity is exactly that
  the segment   one append of 1025 frames of a 33-atom system, across the 1024-frame cut of a batched call
  max_lag       0, 1, 63, 64, 65, frames - 1 and beyond: each curve a prefix of the full one, bit for bit
  one atom      65 frames (two block rows, the second with one live frame), one of them failed, max_lag 3 and 64: the curve bit for bit in
                the order of the band's sums (tests/band_ref.py) -- the product's two-panel launch with its one panel
  clear         followed by re-use"""
import functools

import numpy as np
import pytest

import band_ref as B
import msd_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
NA, A0, NF = 300, 2, 129
SIZES = [1, 15, 16, 17, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@functools.lru_cache(maxsize=None)
def walk(n_atoms=NA, n_frames=NF, cell="tric"):
    return R.walk(n_atoms, n_frames, 20261024, cell)


def make_system(G, frames, boxes):
    s = G.System(len(frames[0]), n_slots=len(frames))
    for k, x in enumerate(frames):
        s.set_frame(x, [float(v) for v in boxes[k]], slot=k)
    return s


@pytest.fixture(scope="module")
def world(G):
    s = make_system(G, *walk()[:2])
    for S in SIZES:
        s.group_create_from_ranges("s%d" % S, [(A0, A0 + S - 1)])
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def ref(S):
    frames, boxes = walk()[:2]
    w = R.Walk(S)
    st, bad = w.append(frames, boxes, np.arange(A0, A0 + S))
    assert not st.any()
    return w


def within_bound(G, m, panel, ok, max_lag=None):
    S, n_pad = m.n_atoms, m.stat(G._lib.MSD_STAT_N_PAD)
    assert n_pad == (S + 63) // 64 * 64
    msd, pairs = m.msd(max_lag)
    want, wpairs, qsum = R.direct_msd(panel, ok, max_lag, dtype=np.longdouble)
    assert np.array_equal(pairs, wpairs) and msd[0] == 0.0
    have = pairs > 0
    assert np.array_equal(np.isnan(msd), ~have) and (np.abs(msd - want)[have] <= R.msd_bound(qsum, pairs, n_pad, S)[have]).all()
    return msd, pairs


def frame_counts():
    a = R.source_ahead()
    return [1, 2, a - 1, a, a + 1, 63, 64, 65, NF]


@pytest.mark.parametrize("S", SIZES)
def test_group_sizes_and_frame_counts(G, world, S):
    w = ref(S)
    for nf in frame_counts():
        with G.MSD(world, "s%d" % S, nf) as m, G.MSD(world, "s%d" % S, nf) as other:      # capacity: exactly full
            other.set_launch(2, 3)
            for x in (m, other):
                assert not x.append(0, nf).any() and x.n_frames == nf == x.capacity
            d = m.displacements(0, nf)
            assert R.same_bits(d, w.panel()[:nf]) and R.same_bits(other.displacements(0, nf), d)
            msd, pairs = within_bound(G, m, w.panel()[:nf], w.ok[:nf])
            omsd, opairs = other.msd()
            assert msd.tobytes() == omsd.tobytes() and pairs.tobytes() == opairs.tobytes() and m.from_origin().tobytes() == other.from_origin().tobytes()
            assert len(msd) == nf and m.stat(G._lib.MSD_STAT_BLOCK_EDGE) == 64
            with pytest.raises(G.DeviceError):
                m.append(0, 1)                                                             # full


def test_one_append_across_the_1024_frame_segment(G):
    frames, boxes = walk(33, 1025, "rescaled")[:2]
    s = make_system(G, frames, boxes)
    s.group_create_from_ranges("g", [(1, 31)])
    idx = np.arange(1, 32)
    w = R.Walk(31)
    w.append(frames, boxes, idx)
    with G.MSD(s, "g", 1025) as m, G.MSD(s, "g", 1025) as cut:
        assert not m.append(0, 1025).any()
        assert R.same_bits(m.displacements(0, 1025), w.panel())
        assert m.stat(G._lib.MSD_STAT_LAUNCHES) == 2                                       # two segments
        msd, pairs = within_bound(G, m, w.panel(), w.ok)
        assert len(msd) == 1025 and pairs[1024] == 1
        cut.append(0, 1023); cut.append(1023, 2)
        cmsd, cpairs = cut.msd()
        assert cmsd.tobytes() == msd.tobytes() and cut.displacements(1020, 5).tobytes() == m.displacements(1020, 5).tobytes()
        short, spairs = m.msd(64)
        assert short.tobytes() == msd[:65].tobytes() and spairs.tobytes() == pairs[:65].tobytes()
        assert m.stat(G._lib.MSD_STAT_LAST_BLOCKS) < cut.stat(G._lib.MSD_STAT_LAST_BLOCKS) == 17 * 18 // 2      # the band: not every block
    s.close()


@pytest.mark.parametrize("S", [17, 257])
def test_max_lag_gives_prefixes_of_the_full_curve(G, world, S):
    w = ref(S)
    with G.MSD(world, "s%d" % S, NF) as m:
        m.append(0, NF)
        full, fpairs = m.msd()
        assert len(full) == NF
        for lag in (0, 1, 63, 64, 65, NF - 1, NF + 5):
            msd, pairs = within_bound(G, m, w.panel(), w.ok, lag)
            n = min(lag, NF - 1) + 1                                                       # (a lag beyond the last frame is clamped)
            assert len(msd) == n and msd.tobytes() == full[:n].tobytes() and pairs.tobytes() == fpairs[:n].tobytes()
        assert m.msd(0)[0].tolist() == [0.0]


def test_a_failed_frame_at_each_side_of_a_block_edge(G):
    frames, boxes = walk(40, 70, "ortho")[:2]
    frames = [x.copy() for x in frames]
    frames[63][9] = np.nan; frames[64][9] = np.nan; frames[0][9] = np.nan
    s = make_system(G, frames, boxes)
    s.group_create_from_ranges("g", [(2, 38)])
    idx = np.arange(2, 39)
    w = R.Walk(37)
    st, bad = w.append(frames, boxes, idx)
    with G.MSD(s, "g", 70) as m:
        assert m.append(0, 70, raise_on_error=False).tolist() == st.tolist() and st[[0, 63, 64]].tolist() == [R.E_NO_POSITION] * 3
        assert R.same_bits(m.displacements(0, 70), w.panel())
        msd, pairs = within_bound(G, m, w.panel(), w.ok)
        assert pairs[0] == 67 and pairs[69] == 0 and np.isnan(msd[69]) and pairs[1] == 65
    s.close()


def test_clear_and_reuse(G, world):
    w = ref(65)
    with G.MSD(world, "s65", 40) as a, G.MSD(world, "s65", 40) as b:
        a.append(7, 33); a.msd(5)
        a.clear()
        assert a.n_frames == 0 and a.stat(G._lib.MSD_STAT_COUNTED) == 0 and a.stat(G._lib.MSD_STAT_LAGS) == 0
        a.append(0, 40); b.append(0, 40)                                                   # the full capacity again, a new origin
        assert R.same_bits(a.displacements(0, 40), w.panel()[:40])
        assert a.msd()[0].tobytes() == b.msd()[0].tobytes() and a.from_origin().tobytes() == b.from_origin().tobytes()


def test_one_atom_in_the_order_of_the_band(G):
    frames, boxes = walk(6, 65, "ortho")[:2]
    frames = [x.copy() for x in frames]
    frames[62][4] = np.nan
    s = make_system(G, frames, boxes)
    s.group_create_from_ranges("one", [(4, 4)])
    w = R.Walk(1)
    st, bad = w.append(frames, boxes, np.arange(4, 5))
    assert st.tolist() == [0] * 62 + [R.E_NO_POSITION, 0, 0]
    with G.MSD(s, "one", 65) as m:
        assert m.append(0, 65, raise_on_error=False).tolist() == st.tolist()
        assert m.stat(G._lib.MSD_STAT_N_PAD) == 64 and m.stat(G._lib.MSD_STAT_COUNTED) == 64
        d = m.displacements(0, 65)
        assert R.same_bits(d, w.panel()) and not d[62].any() and d[64].any()
        q = m.from_origin()                                                                 # one atom: the rows' squared norms themselves
        assert np.isnan(q[62]) and not np.isnan(np.delete(q, 62)).any()
        value = (q[:, None] + q[None, :]) - 2.0 * B.gram(d[:, 0, :])
        for lag in (3, 64):
            msd, pairs = within_bound(G, m, w.panel(), w.ok, lag)
            assert pairs[0] == 64 and pairs[1] == 62 and m.stat(G._lib.MSD_STAT_LAST_BLOCKS) == 3 == m.stat(G._lib.MSD_STAT_LAST_GRAM_GROUPS)
            want = B.band_sums(value, w.ok, lag, strict=True) / pairs.astype(np.float64)
            print("max_lag %d: largest difference from the restated order %.3g" % (lag, np.abs(msd - want).max()))
            assert R.same_bits(msd, want)
        assert pairs[64] == 1
    s.close()

"""Segments.gyration at its edges: the 1024-frame segment of the batch, the first error of a frame, and periodic invariance.

  batch boundary       40 atoms in 5 segments (1, 4, 5, 16 and 14 atoms), 1 026 slots, each frame a jittered copy: the rows of frames 1023,
                       1024 and 1025 of one 1 026-frame call are those of single-frame calls bit for bit, with and without axes; a
                       slot without box in the middle is GR_E_NO_BOX for that frame only, in the periodic kinds only
  first error          NaN positions in the 3-atom AND in the 4097-atom segment of one frame (two different team classes, two
                       launches): the frame's error is the lower segment's, as in `centers`
  periodic invariance  a whole segment moved by a box vector of a triclinic cell: the tensor moves by no more than the margin of
                       gyration_ref.py (taken at the larger coordinates of the moved copy)"""
import numpy as np
import pytest

import gyration_ref as R
from segments_ref import E_NO_BOX, E_NO_POSITION, ESTIMATE, NAIVE, PBC, _bits, _cell

pytestmark = pytest.mark.gpu
F = np.float32
TRIC = [6.0, 6.4, 5.0, 0, 0, 1.0, 0, -1.5, 0.8]


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def test_batch_boundary(G):
    n, nf, nobox = 40, 1026, 500
    rng = np.random.default_rng(20260703)
    s = G.System(n, masses=(1.0 + 15.0 * rng.random(n)).astype(F), n_slots=nf)
    base = (rng.random((n, 3)) * 0.6 + 2.7).astype(F)                  # a blob across the faces of the 3 nm cell
    base -= F(3.0) * (base >= F(3.0))
    for f in range(nf):
        s.set_frame(base + (F(0.01) * rng.random((n, 3))).astype(F), [3.0, 3.0, 3.0] if f != nobox else None, slot=f)
    cuts = np.cumsum([0, 1, 4, 5, 16, 14])
    seg = G.Segments.from_lists(s, [np.arange(cuts[k], cuts[k + 1]) for k in range(5)])
    assert [seg.stat(k) for k in (1, 2, 3, 4)] == [2, 3, 0, 0]
    for kind, w in ((PBC, 1), (NAIVE, 0)):
        for axes in (True, False):
            g = seg.gyration(0, nf, kind, w, axes=axes, raise_on_error=False)
            assert seg.stat(G._lib.SEG_STAT_LAST_PIECES) == 2 and seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 2 * (2 + int(axes))
            want = [0] * nf
            if kind != NAIVE:
                want[nobox] = E_NO_BOX
                assert np.isnan(g.moments[nobox]).all() and (not axes or np.isnan(g.raw_axes[nobox]).all())
            assert g.status.tolist() == want and not np.isnan(np.delete(g.moments, nobox, axis=0)).any()
            for f in (0, nobox, 1023, 1024, 1025):
                one = seg.gyration(f, 1, kind, w, axes=axes, raise_on_error=False)
                assert np.array_equal(_bits(one.moments[0]), _bits(g.moments[f])) and one.status[0] == g.status[f], (kind, axes, f)
                if axes:
                    assert np.array_equal(_bits(one.raw_axes[0]), _bits(g.raw_axes[f])), (kind, f)
            cen, st = seg.centers(1020, 6, kind, w)
            assert np.array_equal(_bits(g.center[1020:]), _bits(cen))
    # pieces that do not divide the segment of the batch: 1024 = 2 * 400 + 224, then the last two frames
    seg.set_piece_frames(400)
    h = seg.gyration(0, nf, PBC, 1, axes=True, raise_on_error=False)
    assert seg.stat(G._lib.SEG_STAT_LAST_PIECES) == 4
    seg.set_piece_frames(0)
    g = seg.gyration(0, nf, PBC, 1, axes=True, raise_on_error=False)
    assert np.array_equal(_bits(h.moments), _bits(g.moments)) and np.array_equal(_bits(h.raw_axes), _bits(g.raw_axes)) and h.status.tolist() == g.status.tolist()
    with pytest.raises(G.DeviceError):
        seg.gyration_device(0, 1025, PBC, 1)                          # more than a piece can ever hold
    s.close()


def test_first_error_is_the_lower_segment_s(G):
    n = 4200
    rng = np.random.default_rng(20260704)
    pos = (rng.normal(0.0, 0.1, (n, 3)) + 2.0).astype(F)
    lists = [np.arange(10, 13), np.arange(50, 50 + 4097), np.arange(20, 37)]
    nan3, nan4097 = 11, 50 + 4000
    s = G.System(n, masses=(1.0 + rng.random(n)).astype(F), n_slots=2)
    s.set_frame(pos, [4.0, 4.0, 4.0], slot=0)
    bad = pos.copy()
    bad[nan3] = np.nan
    bad[nan4097] = np.nan
    s.set_frame(bad, [4.0, 4.0, 4.0], slot=1)
    seg = G.Segments.from_lists(s, lists)
    rev = G.Segments.from_lists(s, lists[::-1])
    for kind, w in ((PBC, 1), (ESTIMATE, 0), (NAIVE, 1)):
        g = seg.gyration(0, 2, kind, w, axes=True, raise_on_error=False)
        cen, st = seg.centers(0, 2, kind, w, raise_on_error=False)
        assert g.status.tolist() == st.tolist() == [0, E_NO_POSITION] and np.array_equal(_bits(g.center), _bits(cen))
        assert np.isnan(g.moments[1]).all(axis=1).tolist() == [True, True, False] and np.isnan(g.raw_axes[1]).all(axis=1).tolist() == [True, True, False]
        assert np.array_equal(_bits(g.moments[1, 2]), _bits(g.moments[0, 2]))
        with pytest.raises(G.GroupError) as e:
            seg.gyration(0, 2, kind, w)
        assert (e.value.variant, e.value.detail) == ("InvalidPosition", nan3)
        with pytest.raises(G.GroupError) as e:                        # the other way round the workgroup's segment comes first
            rev.gyration(1, 1, kind, w)
        assert (e.value.variant, e.value.detail) == ("InvalidPosition", nan4097)
    s.close()


def test_periodic_invariance(G):
    H = _cell(TRIC)
    rng = np.random.default_rng(20260705)
    sizes = [2, 5, 17, 300, 4200]
    n = sum(sizes)
    cuts = np.cumsum([0] + sizes)
    lists = [np.arange(cuts[k], cuts[k + 1]) for k in range(len(sizes))]
    pos = np.zeros((n, 3))
    for l in lists:
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pos[l] = (np.array([0.3, 0.5, 0.5]) + 0.4 * rng.random(3)) @ H + (np.clip(rng.normal(0.0, 1.0, (len(l), 3)), -3, 3) * [0.15, 0.09, 0.045]) @ Q.T
    moves = [(0, 1, 0), (0, 0, -1), (1, 0, 1), (-1, 1, 0), (0, -1, 1)]
    moved = pos.copy()
    for l, mv in zip(lists, moves):
        moved[l] += np.array(mv, np.float64) @ H
    masses = (1.0 + 15.0 * rng.random(n)).astype(F)
    s = G.System(n, masses=masses, n_slots=2)
    s.set_frame(pos.astype(F), TRIC, slot=0)
    s.set_frame(moved.astype(F), TRIC, slot=1)
    seg = G.Segments.from_lists(s, lists)
    for kind, w in ((PBC, 1), (PBC, 0), (ESTIMATE, 1), (ESTIMATE, 0)):
        g = seg.gyration(0, 2, kind, w)
        assert g.status.tolist() == [0, 0]
        refs = [R.reference([pos, moved][f].astype(F), TRIC, masses, lists, g.center[f], kind, w) for f in range(2)]
        for f in range(2):
            R.check_moments("invariance kind %d weighted %d frame %d" % (kind, w, f), g.moments[f], *refs[f])
        margin = np.maximum(refs[0][1], refs[1][1])
        diff = np.abs(g.tensor[1].astype(np.float64) - g.tensor[0].astype(np.float64)).max(axis=(1, 2))
        print("invariance kind %d weighted %d: max |S' - S| / margin %.3g" % (kind, w, float((diff / margin).max())))
        assert (diff <= margin).all(), (kind, w, (diff / margin).tolist())
    s.close()

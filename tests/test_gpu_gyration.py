"""Segments.gyration (gr_segments_gyration_batch): centre, Rg, gyration tensor and principal axes of every segment over resident frames,
against the numpy f64 reference of gyration_ref.py (margins derived there).

Synthetic system: the one of test_gpu_segments.py -- 9 500 atoms, segments of 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4096
and 4097 atoms (both sides of every team-class boundary), layouts "gather" and "to_end", the 284 atoms outside every segment at 1e30
with a mass of 1e30 -- with ANISOTROPIC clouds: Gaussian with axis scales 1 : 0.6 : 0.3 (sigma 0.15 nm, cut at 3 sigma: extent <= 0.9 nm),
randomly rotated, straddling the cell faces, masses spread over 1 .. 16.
  slot 0  orthorhombic      1  triclinic      2  no box      3  orthorhombic, NaN positions inside the 17- and the 4097-atom segment
Real system: tests/golden/aa_full.npz by residue, 5 271 segments, 2 frames.
Closed forms: one atom, two atoms of masses 1 and 3, a planar ring of 12 atoms."""
import os

import numpy as np
import pytest

import gyration_ref as R
from segments_ref import E_INVALID_ARG, E_NO_BOX, E_NO_POSITION, ESTIMATE, KINDS, NAIVE, PBC, _bits, _cell

pytestmark = pytest.mark.gpu
F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

N = 9500
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4096, 4097]
BOX = [6.0, 6.4, 5.0]
TRIC = [6.0, 6.4, 5.0, 0, 0, 1.0, 0, -1.5, 0.8]
BOXES = [BOX, TRIC, None, BOX]
NOBOX_FRAME, NAN_FRAME, NF = 2, 3, 4
SCALES = np.array([0.15, 0.09, 0.045])


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def _layout(name):
    rng = np.random.default_rng(20260601)
    if name == "gather":
        perm = rng.permutation(N)[:sum(SIZES)]
        cuts = np.cumsum([0] + SIZES)
        return [np.sort(perm[cuts[k]:cuts[k + 1]]).astype(np.uint64) for k in range(len(SIZES))]
    a = N - sum(SIZES)
    lists = []
    for n in SIZES:
        lists.append(np.arange(a, a + n, dtype=np.uint64)); a += n
    return lists


def _frames(lists):
    rng = np.random.default_rng(20260702)
    frames = []
    for box in BOXES:
        H = _cell(box if box is not None else BOX)
        Hi = np.linalg.inv(H)
        pos = np.full((N, 3), 1e30, np.float64)
        for idx in lists:
            idx = idx.astype(np.int64)
            c = rng.random(3)
            c[rng.integers(0, 3)] = rng.choice([0.004, 0.996, 0.0, 0.5])      # the cloud straddles a face of the cell
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            d = (np.clip(rng.normal(0.0, 1.0, (idx.size, 3)), -3.0, 3.0) * SCALES) @ Q.T
            u = c + d @ Hi
            u -= np.floor(u)
            pos[idx] = u @ H
        frames.append(pos.astype(F))
    frames[NAN_FRAME][int(lists[7][4])] = np.nan
    frames[NAN_FRAME][int(lists[15][4000])] = np.nan
    return frames


_WORLDS = {}


@pytest.fixture(scope="module")
def worlds(G):
    def get(name):
        if name not in _WORLDS:
            lists = _layout(name)
            frames = _frames(lists)
            rng = np.random.default_rng(20260603)
            masses = (1.0 + 15.0 * rng.random(N)).astype(F)
            inside = np.zeros(N, bool)
            for l in lists:
                inside[l.astype(np.int64)] = True
            assert int((~inside).sum()) == N - sum(SIZES) == 284
            masses[~inside] = 1e30
            s = G.System(N, masses=masses, n_slots=NF)
            for f in range(NF):
                s.set_frame(frames[f], BOXES[f], slot=f)
            _WORLDS[name] = (s, G.Segments.from_lists(s, lists), lists, frames, masses)
        return _WORLDS[name]
    yield get
    for w in _WORLDS.values():
        w[0].close()
    _WORLDS.clear()


def _same(a, b):
    """two Gyration results: the same bits everywhere"""
    ok = np.array_equal(_bits(a.moments), _bits(b.moments)) and a.status.tolist() == b.status.tolist()
    if a.raw_axes is not None or b.raw_axes is not None:
        ok = ok and np.array_equal(_bits(a.raw_axes), _bits(b.raw_axes))
    return ok


# ------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("layout", ["gather", "to_end"])
@pytest.mark.parametrize("kind, weighted", KINDS)
def test_synthetic_against_reference(G, worlds, layout, kind, weighted):
    s, seg, lists, frames, masses = worlds(layout)
    if layout == "to_end":
        assert int(lists[-1][-1]) == N - 1
    g = seg.gyration(0, NF, kind, weighted, axes=True, raise_on_error=False)
    cen, st = seg.centers(0, NF, kind, weighted, raise_on_error=False)
    # the centre is centers' own, NaN rows and status are exactly centers'
    assert np.array_equal(_bits(g.center), _bits(cen)) and g.status.tolist() == st.tolist()
    assert st.tolist() == [0, 0, 0 if kind == NAIVE else E_NO_BOX, E_NO_POSITION]
    nan_rows = np.isnan(cen).any(axis=2)
    assert np.array_equal(np.isnan(g.moments).all(axis=2), nan_rows) and np.array_equal(np.isnan(g.moments).any(axis=2), nan_rows)
    assert nan_rows[NAN_FRAME].nonzero()[0].tolist() == [7, 15] and not nan_rows[0].any() and not nan_rows[1].any()
    assert g.tensor.shape == (NF, 16, 3, 3) and np.array_equal(_bits(g.tensor), _bits(np.swapaxes(g.tensor, 2, 3))) and g.rg.shape == (NF, 16)
    # from 63 atoms on the sample tensor of a 1 : 0.6 : 0.3 cloud keeps all three eigenvalues 0.2 lambda_1 apart (asserted on the
    # reference); below, the sample strays too far from 1 : 0.36 : 0.09 for that, and every axis that IS that far apart is compared
    enough = np.array(SIZES) >= 63
    for f in range(NF):
        if BOXES[f] is None and kind != NAIVE:
            assert np.isnan(g.moments[f]).all() and np.isnan(g.raw_axes[f]).all()
            continue
        what = "%s kind %d weighted %d frame %d" % (layout, kind, weighted, f)
        S_ref, margin = R.reference(frames[f], BOXES[f], masses, lists, cen[f], kind, weighted)
        R.check_moments(what, g.moments[f], S_ref, margin)
        # (a naive centre of a cloud that straddles a face measures the split cloud: no promise about its eigenvalue gaps)
        R.check_axes(what, g.moments[f], g.raw_axes[f], S_ref, enough if kind != NAIVE else None)
    # without axes: the same moments
    plain = seg.gyration(0, NF, kind, weighted, raise_on_error=False)
    assert plain.axes is None and plain.eigenvalues is None and np.array_equal(_bits(plain.moments), _bits(g.moments))
    # the first failed FRAME of the call is what the call raises
    with pytest.raises(G.GroupError) as e:
        seg.gyration(0, NF, kind, weighted)
    if kind == NAIVE:
        assert (e.value.variant, e.value.detail) == ("InvalidPosition", int(lists[7][4]))
    else:
        assert e.value.variant == "InvalidSimBox" and e.value.status == E_NO_BOX


@pytest.fixture(scope="module")
def aa(G):
    d = np.load(os.path.join(GOLD, "aa_full.npz"))
    masses = np.load(os.path.join(GOLD, "aa_peptide.npz"))["masses"]
    frames, boxes, resid = [f for f in d["frames"]], [b for b in d["boxes9"]], d["resid"]
    s = G.System(len(resid), masses=masses, n_slots=2)
    for f in range(2):
        s.set_frame(frames[f], boxes[f], slot=f)
    seg = G.Segments.by_resid(s, resid)
    yield s, seg, [seg.atoms(k) for k in range(len(seg))], frames, boxes, masses
    s.close()


@pytest.mark.parametrize("weighted", [1, 0])
def test_real_system_against_reference(G, aa, weighted):
    s, seg, lists, frames, boxes, masses = aa
    assert len(seg) == 5271
    g = seg.gyration(0, 2, PBC, weighted, axes=True)
    assert seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 4 and seg.stat(G._lib.SEG_STAT_LAST_PIECES) == 1
    cen, st = seg.centers(0, 2, PBC, weighted)
    # centers still reports its own launches after gyration calls
    assert seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 3 and seg.stat(G._lib.SEG_STAT_LAST_LAUNCH_SETS) == 1
    assert np.array_equal(_bits(g.center), _bits(cen)) and g.status.tolist() == st.tolist() == [0, 0] and not np.isnan(g.moments).any()
    for f in range(2):
        S_ref, margin = R.reference(frames[f], boxes[f], masses, lists, cen[f], PBC, weighted)
        R.check_moments("aa weighted %d frame %d" % (weighted, f), g.moments[f], S_ref, margin)
        R.check_axes("aa weighted %d frame %d" % (weighted, f), g.moments[f], g.raw_axes[f], S_ref)
    # the descriptors close on the host from the eigenvalues alone
    b, c, k2 = G.shape_descriptors(g.eigenvalues)
    assert b.shape == (2, 5271) and (k2 >= -1e-6).all() and (k2 <= 1.0 + 1e-6).all() and (c >= 0).all()
    I = seg.moments_of_inertia(g.eigenvalues, masses)
    assert I.shape == (2, 5271, 3) and (I[..., 0] <= I[..., 1]).all() and (I[..., 1] <= I[..., 2]).all()


def test_from_group_is_one_segment(G, aa):
    s, seg, lists, frames, boxes, masses = aa
    s.group_create_from_ranges("pep", [(0, 362)])
    try:
        one = G.Segments.from_group(s, "pep")
        assert len(one) == 1 and one.atoms(0).tolist() == list(range(363))
        g = one.gyration(0, 2)
        cen, _ = one.centers(0, 2, PBC, 1)
        assert g.rg.shape == (2, 1) and np.array_equal(_bits(g.center), _bits(cen))
        for f in range(2):
            S_ref, margin = R.reference(frames[f], boxes[f], masses, [np.arange(363)], cen[f], PBC, 1)
            R.check_moments("peptide frame %d" % f, g.moments[f], S_ref, margin)
        one.close()
    finally:
        s.group_remove("pep")


# ------------------------------------------------------------------ closed forms
def test_closed_forms(G):
    r = 0.37
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    normal = np.array([1.0, -2.0, 2.0]) / 3.0
    e1 = np.cross(normal, [0.0, 0.0, 1.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(normal, e1)
    t = 2.0 * np.pi * np.arange(12) / 12.0
    ring = np.array([2.0, 2.0, 2.0]) + 0.5 * (np.cos(t)[:, None] * e1 + 0.6 * np.sin(t)[:, None] * e2)
    a = np.array([3.9, 0.1, 1.0])                                     # the pair straddles a face of the cell
    pos = np.concatenate([[[1.0, 2.0, 3.0]], [a, a + r * u], ring]).astype(F)
    pos[2] -= F(4.0) * np.array([1, 0, 0], F) * (pos[2][0] >= 4.0)    # wrapped into the 4 nm cell
    masses = np.concatenate([[12.0], [1.0, 3.0], np.ones(12)]).astype(F)
    lists = [np.arange(0, 1), np.arange(1, 3), np.arange(3, 15)]
    s = G.System(15, masses=masses, n_slots=1)
    s.set_frame(pos, [4.0, 4.0, 4.0], slot=0)
    seg = G.Segments.from_lists(s, lists)
    for kind, w in [(PBC, 1), (ESTIMATE, 1), (NAIVE, 1)]:
        g = seg.gyration(0, 1, kind, w, axes=True)
        cen, _ = seg.centers(0, 1, kind, w)
        S_ref, margin = R.reference(pos, [4.0, 4.0, 4.0], masses, lists, cen[0], kind, w)
        R.check_moments("closed forms kind %d" % kind, g.moments[0], S_ref, margin)
        R.check_axes("closed forms kind %d" % kind, g.moments[0], g.raw_axes[0], S_ref)
        # one atom: all zeros and the identity
        assert (g.moments[0, 0, 3:] == 0).all() and (g.eigenvalues[0, 0] == 0).all() and np.array_equal(g.axes[0, 0], np.eye(3, dtype=F))
        # a ring: flat along its normal
        assert abs(g.eigenvalues[0, 2, 2]) <= margin[2] and abs(abs(float(g.axes[0, 2, 2] @ normal)) - 1.0) <= 1e-5
        assert abs(g.eigenvalues[0, 2, 0] - 0.125) <= margin[2] and abs(g.eigenvalues[0, 2, 1] - 0.045) <= margin[2]
        if kind == NAIVE:
            continue                                                  # (the naive centre sees the pair split by the cell)
        # two atoms of masses 1 and 3: lambda_1 = 3 r^2 / 16, the others 0, v_1 along the bond with positive components
        lam, v1 = g.eigenvalues[0, 1].astype(np.float64), g.axes[0, 1, 0].astype(np.float64)
        assert abs(lam[0] - 3.0 * r * r / 16.0) <= margin[1] and abs(lam[1]) <= margin[1] and abs(lam[2]) <= margin[1]
        assert np.abs(v1 - u).max() <= 1e-5 and v1[0] > 0 and v1[1] > 0
        assert abs(float(g.rg[0, 1]) ** 2 - 3.0 * r * r / 16.0) <= 3.0 * margin[1]
    s.close()


# ------------------------------------------------------------------ bit-level properties
@pytest.mark.parametrize("kind, weighted", [(PBC, 1), (ESTIMATE, 0), (NAIVE, 1)])
def test_bitwise(G, worlds, kind, weighted):
    s, seg, lists, frames, masses = worlds("gather")
    M = len(lists)
    P, L = G._lib.SEG_STAT_LAST_PIECES, G._lib.SEG_STAT_LAST_LAUNCHES
    a = seg.gyration(0, NF, kind, weighted, axes=True, raise_on_error=False)
    assert seg.stat(P) == 1 and seg.stat(L) == 5
    # two runs; a centers call in between
    assert _same(a, seg.gyration(0, NF, kind, weighted, axes=True, raise_on_error=False))
    cen, _ = seg.centers(0, NF, kind, weighted, raise_on_error=False)
    assert seg.stat(L) == 4
    assert _same(a, seg.gyration(0, NF, kind, weighted, axes=True, raise_on_error=False))
    # one call per frame
    for f in range(NF):
        one = seg.gyration(f, 1, kind, weighted, axes=True, raise_on_error=False)
        assert np.array_equal(_bits(one.moments[0]), _bits(a.moments[f])) and np.array_equal(_bits(one.raw_axes[0]), _bits(a.raw_axes[f])) and one.status[0] == a.status[f]
    # pieces of one and of two frames, and the default again
    for n, pieces in ((1, 4), (2, 2), (3, 2), (0, 1)):
        seg.set_piece_frames(n)
        assert _same(a, seg.gyration(0, NF, kind, weighted, axes=True, raise_on_error=False)), n
        assert seg.stat(P) == pieces and seg.stat(L) == 5 * pieces
        b = seg.gyration(0, NF, kind, weighted, raise_on_error=False)
        assert np.array_equal(_bits(b.moments), _bits(a.moments)) and seg.stat(P) == pieces and seg.stat(L) == 4 * pieces
    # the device form, read back
    mom, ax, st_d = seg.gyration_device(0, NF, kind, weighted, axes=True, raise_on_error=False)
    assert np.array_equal(_bits(s.device_read(mom, 0, (NF, M, 10))), _bits(a.moments)) and st_d.tolist() == a.status.tolist()
    assert np.array_equal(_bits(s.device_read(ax, 0, (NF, M, 12))), _bits(a.raw_axes))
    mom, ax, _ = seg.gyration_device(1, 1, kind, weighted)
    assert ax is None and np.array_equal(_bits(s.device_read(mom, 0, (1, M, 10))), _bits(a.moments[1:2]))
    # every other segment alone: the shared segments keep their rows
    sub = G.Segments.from_lists(s, lists[::2])
    q = sub.gyration(0, NF, kind, weighted, axes=True, raise_on_error=False)
    assert np.array_equal(_bits(q.moments), _bits(a.moments[:, ::2])) and np.array_equal(_bits(q.raw_axes), _bits(a.raw_axes[:, ::2]))
    sub.close()


def test_refusals(G, worlds):
    s, seg, lists, frames, masses = worlds("gather")
    lib = G._lib.load()
    good = seg.gyration(0, 2, PBC, 1, axes=True)

    def still_good():
        assert _same(good, seg.gyration(0, 2, PBC, 1, axes=True))
    with pytest.raises(G.DeviceError) as e:                           # an unknown kind
        seg.gyration(0, 2, 3, 1)
    assert e.value.status == E_INVALID_ARG
    still_good()
    assert lib.gr_segments_gyration_batch(seg._seg, 0, 2, PBC, 1, None, None, None) == E_INVALID_ARG      # moments NULL
    still_good()
    seg.set_piece_frames(2)
    try:
        with pytest.raises(G.DeviceError) as e:                       # the device form beyond one piece
            seg.gyration_device(0, 3, PBC, 1)
        assert e.value.status == E_INVALID_ARG
        seg.gyration_device(0, 2, PBC, 1)
    finally:
        seg.set_piece_frames(0)
    still_good()
    with pytest.raises(G.DeviceError):                                # a slot range out of bounds
        seg.gyration(3, 2, PBC, 1)
    with pytest.raises(G.DeviceError):
        seg.gyration_device(NF, 1, PBC, 1)
    still_good()

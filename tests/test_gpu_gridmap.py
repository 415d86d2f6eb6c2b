"""GridMap accumulated over resident frames (gr_gridmap_*; groan_rs_amd.GridMap) against the numpy restatement tests/gridmap_ref.py.

Every comparison is EXACT: counts and sums are integers and the tile index is a defined f32 expression.  The system has 1000 atoms
(one partial 256-atom tile: the pads must never be binned) in 6 slots:
  0  spread over and around the maps, with atoms exactly on half-way points between tiles, one ulp either side of the lower edge
     span0 - tile / 2 and of the upper edge, at +-inf, far outside and at coordinate 0
  1  every atom in ONE tile (maximum contention)
  2  like 3, with a NaN atom (index 6) inside most groups
  3  moderate coordinates (what the oracle's wrap loops can be run on)
  4  like 3, without a box
  5  like 3, in a triclinic box, with a few atoms far outside the cell
A second, 9000-atom system spreads one frame over several workgroups and has a group dense enough to be walked through its bit mask."""
import io

import numpy as np
import pytest

import gridmap_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
F = np.float32
N = 1000
BOX = [6.0, 6.4, 5.0]
TRIC = [6.0, 6.4, 5.0, 0, 0, 1.0, 0, -1.5, 0.8]
MAPS = {"4x3": ((0.0, 3.0), (0.0, 2.0), (1.0, 1.0)), "61x16": ((-2.0, 7.0), (3.0, 6.0), (0.15, 0.20)), "301x257": ((0.0, 6.0), (0.0, 6.4), (0.02, 0.025))}
SHAPES = {"4x3": (4, 3), "61x16": (61, 16), "301x257": (301, 257)}
GROUPS = {"block": np.arange(3, 771), "third": np.arange(0, N, 3), "two": np.concatenate([np.arange(10, 201), np.arange(600, 901)]), "all": np.arange(N)}
NAN_ATOM = 6
LDS, GLOBAL = 1, 2      # GR_GM_STAT_*_LAUNCHES


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def _frames():
    rng = np.random.default_rng(20260502)
    fr = [np.stack([rng.random(N) * 12 - 3, rng.random(N) * 10 - 1.5, rng.random(N) * 6 - 0.5], 1).astype(F) for _ in range(6)]
    f0 = fr[0]
    k = 3                                                   # special atoms sit at 3, 4, ... so that every group holds some
    for name in ("61x16", "301x257", "4x3"):
        sx, sy, td = MAPS[name]
        s0, t, hi = F(sx[0]), F(td[0]), F(sx[1])
        mids = [F(s0 + F(F(j + 0.5) * t)) for j in (0, 1, 7)]
        lo_edge, hi_edge = F(s0 - F(t / F(2))), F(hi + F(t / F(2)))
        for v in mids + [lo_edge, np.nextafter(lo_edge, F(np.inf)), np.nextafter(lo_edge, F(-np.inf)), hi_edge, np.nextafter(hi_edge, F(np.inf)), np.nextafter(hi_edge, F(-np.inf))]:
            f0[k, 0] = v; f0[k, 1] = F(sy[0]) + F(td[1]) * F(1.5); k += 3      # ... in x, and y itself on a half-way point
    for v in (np.inf, -np.inf, 1e9, -1e30, 0.0, -0.0):
        f0[k, 0] = v; k += 3
        f0[k, 1] = v; k += 3
    f0[k, 2] = np.inf; k += 3                                # a z that cannot be summed
    f0[k, 2] = 3e9; k += 3
    assert k < 300
    fr[1][:, 0] = 1.0; fr[1][:, 1] = 4.0                      # one tile of every map (4.0 lies in the y span of all three)
    fr[2][NAN_ATOM, 0] = np.nan
    fr[5][[12, 15, 18, 21], 0] = [1e9, -1e30, 250.0, -97.5]     # far outside the cell (the closed form of the wrap), in the triclinic frame
    fr[5][[24, 27], 1] = [-3e7, 123.25]
    return fr


@pytest.fixture(scope="module")
def world(G):
    fr = _frames()
    boxes = [BOX, BOX, BOX, BOX, None, TRIC]
    s = G.System(N, n_slots=12)
    for k in range(6):
        s.set_frame(fr[k], boxes[k], slot=k)
    s.group_create_from_ranges("block", [(3, 770)])
    s.group_create_from_indices("third", GROUPS["third"])
    s.group_create_from_ranges("two", [(10, 200), (600, 900)])
    ref_frames = [f.copy() for f in fr]
    ref_frames[2][NAN_ATOM] = np.nan
    yield s, ref_frames, boxes
    s.close()


def _wrap_fn(p, box):
    return O.wrap_atoms(p, np.arange(len(p)), box)


def _read(m):
    cnt, sq, mean = m._read(True)
    return cnt, sq, mean


def _same(m, ref):
    cnt, sq, mean = _read(m)
    assert np.array_equal(cnt, ref.count) and np.array_equal(sq, ref.sum_q)
    assert np.array_equal(mean.view(np.uint32), ref.mean().view(np.uint32))


def _path(m):
    return m.stat(LDS), m.stat(GLOBAL)


@pytest.mark.parametrize("mapname", ["4x3", "61x16", "301x257"])
@pytest.mark.parametrize("group", ["block", "third", "two", "all"])
def test_against_restatement(G, world, mapname, group):
    s, fr, boxes = world
    idx = GROUPS[group]
    offset = np.array([0.25, -1.0, 0.0, 2.5, 1e-3, -0.125], F)
    for value, gv, off in [(R.COUNT, "count", None), (R.Z, G.Dimension.Z, offset)]:
        m = G.GridMap(s, *MAPS[mapname])
        assert (m.n_tiles_x, m.n_tiles_y) == SHAPES[mapname]
        ref = R.Map(*MAPS[mapname])
        n_out, st = m.accumulate(group, 0, 6, value=gv, offset=off, raise_on_error=False)
        r_out, r_st, r_bad = ref.accumulate(fr, boxes, idx, value, off)
        assert st.tolist() == r_st.tolist() and n_out.tolist() == r_out.tolist()
        assert (st[2] == R.E_NO_POSITION) == (NAN_ATOM in idx) and st[4] == 0          # frame 4 needs no box without the wrap
        _same(m, ref)
        assert ref.count.sum() > 0 and int(ref.count.sum()) + int(r_out.sum()) == len(idx) * int((r_st == 0).sum())
        # the path taken: privatised in LDS below the budget, global atomics above it
        assert _path(m) == ((1, 0) if mapname != "301x257" else (0, 1))
        if NAN_ATOM in idx:
            with pytest.raises(G.GroupError) as e:
                m.accumulate(group, 2, 1, value=gv)
            assert e.value.variant == "InvalidPosition" and e.value.detail == NAN_ATOM
            _same(m, ref)                                                             # the failed frame added nothing
        # Y and X sums on one frame
        m.clear(); ref.clear()
        for dim, rv in ((G.Dimension.X, R.X), (G.Dimension.Y, R.Y)):
            a = m.accumulate(group, 0, 1, value=dim)
            b = ref.accumulate(fr[:1], boxes[:1], idx, rv)
            assert a[0].tolist() == b[0].tolist()
        _same(m, ref)
        m.close()


@pytest.mark.parametrize("mapname", ["4x3", "61x16", "301x257"])
def test_identities(G, world, mapname):
    s, fr, boxes = world
    offset = np.linspace(-1, 1, 6).astype(F)
    a = G.GridMap(s, *MAPS[mapname]); b = G.GridMap(s, *MAPS[mapname])
    oa = a.accumulate("all", 0, 6, value=G.Dimension.Z, offset=offset, raise_on_error=False)
    ob = b.accumulate("all", 0, 6, value=G.Dimension.Z, offset=offset, raise_on_error=False, force_global=True)   # GR_GM_FORCE_GLOBAL == default
    assert _path(b) == (0, 1)
    ra, rb = _read(a), _read(b)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(ra, rb)) and oa[0].tolist() == ob[0].tolist() and oa[1].tolist() == ob[1].tolist()
    b.clear()
    assert all(not x.view(np.uint8).any() for x in _read(b)[:2]) and np.isnan(_read(b)[2]).all()                   # clear, then read: zeros
    o1 = b.accumulate("all", 0, 3, value=G.Dimension.Z, offset=offset[:3], raise_on_error=False)                   # two calls of 3 == one call of 6
    o2 = b.accumulate("all", 3, 3, value=G.Dimension.Z, offset=offset[3:], raise_on_error=False)
    rb = _read(b)
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(ra, rb))
    assert np.concatenate([o1[0], o2[0]]).tolist() == oa[0].tolist() and np.concatenate([o1[1], o2[1]]).tolist() == oa[1].tolist()
    b.clear()
    b.accumulate("all", 0, 6, value=G.Dimension.Z, offset=offset, raise_on_error=False)                            # a second identical run == the first
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(ra, _read(b)))
    a.close(); b.close()


@pytest.mark.parametrize("mapname", ["61x16", "301x257"])
def test_contention_one_tile(G, world, mapname):
    s, fr, boxes = world
    m = G.GridMap(s, *MAPS[mapname])
    for _ in range(8):
        n_out, st = m.accumulate("all", 1, 1, value=G.Dimension.Z)
        assert n_out[0] == 0 and st[0] == 0
    cnt, sq, _ = _read(m)
    ix, iy = R.coord2index([1.0], MAPS[mapname][0][0], MAPS[mapname][2][0])[0], R.coord2index([4.0], MAPS[mapname][1][0], MAPS[mapname][2][1])[0]
    assert cnt[ix, iy] == 8000 and cnt.sum() == 8000
    assert sq[ix, iy] == 8 * int(R.quantise(fr[1][:, 2])[1].sum()) and np.count_nonzero(sq) == 1
    m.close()


@pytest.mark.parametrize("mapname", ["61x16", "301x257"])
def test_wrap(G, world, mapname):
    """GR_GM_WRAP == gr_group_wrap_batch on a copy of the frames + a plain accumulate; and == the restatement with the oracle's wrap"""
    s, fr, boxes = world
    for group in ("block", "third", "all"):
        idx = GROUPS[group]
        a = G.GridMap(s, *MAPS[mapname]); b = G.GridMap(s, *MAPS[mapname])
        before = [s.get_positions(k) for k in range(6)]
        n_out, st = a.accumulate(group, 0, 6, value=G.Dimension.Z, wrap=True, raise_on_error=False)
        assert all(np.array_equal(s.get_positions(k).view(np.uint32), before[k].view(np.uint32)) for k in range(6))     # the frames are not modified
        assert st[4] == R.E_NO_BOX and st[2] == R.E_NO_POSITION and n_out[2] == 0 and n_out[4] == 0
        assert st[[0, 1, 3, 5]].tolist() == [0, 0, 0, 0]                                                               # triclinic outside strict mode: the library's wrap
        for k in range(6):
            s.copy_frame(6 + k, k)
        wst = s.group_wrap_batch(group, 6, 6, raise_on_error=False)
        assert wst.tolist() == st.tolist()
        # identity on the frames the wrap accepted, one orthorhombic with every atom in one tile, one orthorhombic and one triclinic spread
        # out (frame 0 is left out: its atoms at +-inf wrap to NaN, which the copy then reports as an atom without position)
        a.clear()
        for k in (1, 3, 5):
            oa, _ = a.accumulate(group, k, 1, value=G.Dimension.Z, wrap=True)
            ob, _ = b.accumulate(group, 6 + k, 1, value=G.Dimension.Z)
            assert oa.tolist() == ob.tolist() == [int(n_out[k])]
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(_read(a), _read(b)))
        assert _read(a)[0].sum() > 0
        # against the restatement, where the oracle's wrap loops terminate: frames 3 and 1 (moderate coordinates, orthorhombic)
        a.clear()
        ref = R.Map(*MAPS[mapname])
        for k in (3, 1):
            o, _ = a.accumulate(group, k, 1, value=G.Dimension.Z, wrap=True)
            ro, rs, _ = ref.accumulate([fr[k]], [boxes[k]], idx, R.Z, None, wrap=True, wrap_fn=_wrap_fn)
            assert o.tolist() == ro.tolist() and rs[0] == 0
        _same(a, ref)
        a.close(); b.close()
    s.set_strict_orthogonal(True)
    try:
        a = G.GridMap(s, *MAPS[mapname])
        n_out, st = a.accumulate("all", 5, 1, wrap=True, raise_on_error=False)
        assert st[0] == R.E_NOT_ORTHOGONAL and n_out[0] == 0 and not _read(a)[0].any()
        n_out, st = a.accumulate("all", 5, 1)                                                                          # no wrap, no box check
        assert st[0] == 0
        a.close()
    finally:
        s.set_strict_orthogonal(False)


def test_failures_and_lifetime(G, world):
    s, fr, boxes = world
    with pytest.raises(G.GridMapError) as e:
        G.GridMap.from_box(s, (0.15, 0.20), slot=4)
    assert e.value.variant == "InvalidSimBox" and e.value.status == R.E_NO_BOX
    with pytest.raises(G.GridMapError) as e:
        G.GridMap.from_box(s, (0.15, 0.20), slot=5)                                      # a skewed cell has no tile plane: every mode
    assert e.value.status == R.E_NOT_ORTHOGONAL
    with pytest.raises(G.GridMapError) as e:
        G.GridMap(s, (2.0, -2.0), (3.0, 6.0), (0.15, 0.20))
    assert e.value.variant == "InvalidSpan"
    with pytest.raises(G.GridMapError) as e:
        G.GridMap(s, (-2.0, 7.0), (3.0, 6.0), (0.15, 0.0))
    assert e.value.variant == "InvalidGridTile"
    with pytest.raises(G.GridMapError) as e:
        G.GridMap(s, (0.0, 1000.0), (0.0, 1000.0), (0.01, 0.01))                         # 1e10 tiles
    assert e.value.status == R.E_INVALID_ARG
    m = G.GridMap.from_box(s, (0.15, 0.20), slot=0)
    assert (m.n_tiles_x, m.n_tiles_y) == (R.get_len((0.0, BOX[0]), 0.15)[1], R.get_len((0.0, BOX[1]), 0.20)[1])
    assert m.span_x == (F(0), F(BOX[0])) and m.span_y == (F(0), F(BOX[1]))
    with pytest.raises(G.GroupError) as e:
        m.accumulate("nothing", 0, 1)
    assert e.value.variant == "NotFound"
    s.group_create_from_indices("empty", [])
    with pytest.raises(G.GroupError) as e:
        m.accumulate("empty", 0, 1)
    assert e.value.variant == "EmptyGroup"
    assert not _read(m)[0].any()
    m.close()                                                                            # destroying the map leaves the context usable
    c, st = s.group_center_batch("all", 0, 0, 3, 1)
    assert st[0] == 0 and np.isfinite(c).all()
    m2 = G.GridMap(s, *MAPS["4x3"])
    assert m2.accumulate("all", 3, 1)[1][0] == 0
    m2.close()


def test_mirror_round_trip(G, world):
    s, fr, boxes = world
    m = G.GridMap(s, *MAPS["4x3"])
    ref = R.Map(*MAPS["4x3"])
    n_out, st = m.accumulate("all", 0, 2, value=G.Dimension.Z)
    r_out, _, _ = ref.accumulate(fr[:2], boxes[:2], GROUPS["all"], R.Z)
    assert n_out.tolist() == r_out.tolist() and n_out.dtype == np.uint64 and st.dtype == np.int32
    assert np.array_equal(m.counts, ref.count) and np.array_equal(m.sums_q, ref.sum_q)
    assert np.array_equal(m.sums, ref.sum_q.astype(np.float64) / 2.0 ** 20)
    mean = m.mean()
    assert mean.dtype == np.float32 and mean.shape == (4, 3) and np.array_equal(mean.view(np.uint32), ref.mean().view(np.uint32))
    out = io.StringIO(); m.write_map(out, m.counts)
    lines = out.getvalue().splitlines()
    assert len(lines) == 12 and lines[0] == "  0.000000   0.000000 %d" % ref.count[0, 0] and lines[5] == "  1.000000   2.000000 %d" % ref.count[1, 2]
    out = io.StringIO(); m.write_map(out, mean, column_major=True)
    lines = out.getvalue().splitlines()
    assert lines[1].startswith("  1.000000   0.000000 ") and np.float32(lines[1].split()[2]) == mean[1, 0]      # (the f32 the digits name: they are its shortest round-trip form)
    assert np.float32(lines[4].split()[2]) == mean[0, 1]                                 # shortest digits that round-trip
    assert m.is_inside(1.2, 0.4) and not m.is_inside(3.6, 0.0) and m.get_tile(1.2, 0.4) == (F(1.0), F(0.0))
    m.close()


def test_several_workgroups(G):
    """9000 atoms: the group's range is split over workgroups, with ragged ends; a block, a dense scattered group (walked over its span
    through its bit mask) and a sparse one (index list)"""
    n = 9000
    rng = np.random.default_rng(7)
    fr = [np.stack([rng.random(n) * 9 - 1.5, rng.random(n) * 9 - 1.5, rng.random(n) * 4], 1).astype(F) for _ in range(3)]
    s = G.System(n, n_slots=3)
    for k in range(3):
        s.set_frame(fr[k], [6.0, 6.4, 5.0], slot=k)
    groups = {"mid": np.arange(5, 8898), "odd": np.arange(1, n, 2), "seventh": np.arange(3, n, 7), "all": np.arange(n)}
    s.group_create_from_ranges("mid", [(5, 8897)])
    s.group_create_from_indices("odd", groups["odd"])
    s.group_create_from_indices("seventh", groups["seventh"])
    off = np.array([0.5, 0.0, -0.5], F)
    for group, idx in groups.items():
        for mapname in ("61x16", "301x257"):
            m = G.GridMap(s, *MAPS[mapname]); ref = R.Map(*MAPS[mapname])
            n_out, st = m.accumulate(group, 0, 3, value=G.Dimension.Z, offset=off)
            r_out, _, _ = ref.accumulate(fr, [None] * 3, idx, R.Z, off)
            assert n_out.tolist() == r_out.tolist()
            _same(m, ref)
            m.close()
    s.close()

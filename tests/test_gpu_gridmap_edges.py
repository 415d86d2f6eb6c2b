"""GridMap at the edges of k_gm_accumulate and k_gm_check (gr_gridmap.h): a workgroup that walks several frames, a workgroup that strides
through its range, the check's grid-stride loop, and both sides of the LDS budget.  Every comparison is EXACT, against the numpy
restatement tests/gridmap_ref.py (or, where the oracle's wrap loops cannot run, against the library's own wrap on a copy of the frames).

gr_gridmap_set_launch forces the grids onto a small system; what was launched is read back (GR_GM_STAT_LAST_*_GROUPS), not assumed.
The system has 8300 atoms (one partial 256-atom tile) in 12 slots and three groups that take the three forms of the walk:
  block    atoms 5 .. 8294: contiguous, starts off a multiple of 4, ragged end; 2073 units of 4 atoms
  odd      atoms 1, 3, 5, ...: 4150 atoms, dense, walked through its bit mask over its span; 2075 units
  seventh  atoms 3, 10, 17, ...: an index list of 1186 entries
Frames: spread over and around the maps; 1: every atom in one tile; 4: no box; 9: triclinic, a few atoms far outside the cell;
6: NaN x on the LAST atom of each group (the last step of every stride loop); 11: NaN on atom 101 (within the first 256 units of every
group) and on atom 4203 (beyond unit 512 of every group): the smaller one is reported."""
import ctypes as C

import numpy as np
import pytest

import gridmap_ref as R
from test_gpu_gridmap import BOX, G, MAPS, TRIC, _path, _read, _same, _wrap_fn     # noqa: F401 (G: the fixture)

pytestmark = pytest.mark.gpu
F = np.float32
N, NF = 8300, 12
GROUPS = {"block": np.arange(5, 8295), "odd": np.arange(1, N, 2), "seventh": np.arange(3, N, 7)}
SPAN_WALK = {"block": True, "odd": True, "seventh": False}          # ranges of 4-atom groups of the span / of list entries
UNITS = {g: R.units(GROUPS[g], SPAN_WALK[g]) for g in GROUPS}
ONE_TILE, NO_BOX, TRICLINIC, NAN_LAST, NAN_TWO = 1, 4, 9, 6, 11
NAN_LOW, NAN_HIGH = 101, 4203                                         # both belong to all three groups
OFFSET = np.array([0.25, -1.0, 0.0, 2.5, 1e-3, -0.125, 3.0, -2.75, 0.5, -0.5, 1.75, -4.0], F)
SETTINGS = [(0, 0), (1, 1), (2, 3), (3, 5), (1, 12), (2073, 1)]      # (range_groups, frame_groups)
M61 = MAPS["61x16"]
# the LDS budget of 65536 bytes: 12 bytes per tile with sums, 4 when only counting
BUDGET_MAPS = {"43x127": ((0.0, 5.25), (0.0, 7.875), (0.125, 0.0625)), "2x2731": ((0.0, 4.0), (0.0, 2730 * 2.0 ** -9), (4.0, 2.0 ** -9)),
               "128x128": ((0.0, 127 * 2.0 ** -5), (0.0, 127 * 2.0 ** -5), (2.0 ** -5, 2.0 ** -5)),
               "145x113": ((0.0, 144 * 2.0 ** -5), (0.0, 112 * 2.0 ** -5), (2.0 ** -5, 2.0 ** -5))}
BUDGET_SHAPES = {"43x127": (43, 127), "2x2731": (2, 2731), "128x128": (128, 128), "145x113": (145, 113)}
BUDGET_LDS = {"43x127": (True, True), "2x2731": (True, False), "128x128": (True, False), "145x113": (False, False)}     # (count, Z) on the LDS path


def test_the_groups_are_what_the_cases_need():
    assert UNITS == {"block": 2073, "odd": 2075, "seventh": 1186}
    assert len(GROUPS["odd"]) >= 4096 and len(GROUPS["odd"]) * 8 >= GROUPS["odd"][-1] - GROUPS["odd"][0] + 1       # dense: walked through its mask
    assert 1024 < len(GROUPS["seventh"]) < 4096                                                                  # an index list
    assert [int(GROUPS[g][-1]) for g in ("block", "odd", "seventh")] == [8294, 8299, 8298]                       # frame 6's atoms: no group holds another's
    assert not np.isin([8299, 8298], GROUPS["block"]).any() and not np.isin([8294, 8298], GROUPS["odd"]).any() and not np.isin([8294, 8299], GROUPS["seventh"]).any()
    for g, idx in GROUPS.items():
        assert NAN_LOW in idx and NAN_HIGH in idx
        lo, hi = ((NAN_LOW >> 2) - (int(idx[0]) >> 2), (NAN_HIGH >> 2) - (int(idx[0]) >> 2)) if SPAN_WALK[g] else (int(np.searchsorted(idx, NAN_LOW)), int(np.searchsorted(idx, NAN_HIGH)))
        assert lo < 256 and hi > 512, (g, lo, hi)
    for name, shape in BUDGET_SHAPES.items():
        sx, sy, td = BUDGET_MAPS[name]
        assert (R.get_len(sx, td[0]), R.get_len(sy, td[1])) == ((R.OK, shape[0]), (R.OK, shape[1]))
    assert [BUDGET_SHAPES[k][0] * BUDGET_SHAPES[k][1] for k in ("43x127", "2x2731", "128x128", "145x113")] == [5461, 5462, 16384, 16385]
    assert 5461 * 12 == 65532 and 5462 * 12 > 65536 and 16384 * 4 == 65536


def _walk(fy, nb):
    """frames (of a call of nb) each of the fy workgroups of a range walks, in order: for (f = blockIdx.y; f < nf; f += gridDim.y)"""
    return [list(range(y, nb, fy)) for y in range(fy)]


def test_where_the_failing_frames_fall_in_a_walk():
    """between the settings, frames 6 and 11 are a workgroup's middle and last frame; in a call over slots [6, 12) with 2 frame groups
    frame 6 is the FIRST frame of a workgroup.  From the loop's arithmetic."""
    def place(fy, nb, f):
        w = [w for w in _walk(fy, nb) if f in w][0]
        return "only" if len(w) == 1 else "first" if w[0] == f else "last" if w[-1] == f else "middle"
    assert [place(fy, NF, NAN_LAST) for fy in (1, 3, 5, 12)] == ["middle", "middle", "middle", "only"]
    assert [place(fy, NF, NAN_TWO) for fy in (1, 3, 5, 12)] == ["last", "last", "last", "only"]
    assert [place(fy, NF, NO_BOX) for fy in (1, 3)] == ["middle", "middle"]
    assert place(2, 6, NAN_LAST - 6) == "first" and place(2, 6, NAN_TWO - 6) == "last"
    # (1, 1) on `block`: 2073 units in one range, 9 steps of 256 lanes, the last one ragged; (2, ..) on an odd number of units: a shorter last range
    assert -(-2073 // 256) == 9 and 2073 % 256 != 0 and R.launch(2073, 256, 11712, NF, 2, 3)[3] * 2 == 2074
    assert R.launch(2073, 256, 11712, NF, 2073, 1)[3] == 1


def _draw():
    rng = np.random.default_rng(20260601)
    fr = [np.stack([rng.random(N) * 12 - 3, rng.random(N) * 10 - 1.5, rng.random(N) * 6 - 0.5], 1).astype(F) for _ in range(NF)]
    fr[ONE_TILE][:, 0] = 1.0; fr[ONE_TILE][:, 1] = 4.0                  # one tile of the 61 x 16 map
    fr[TRICLINIC][[13, 17, 21, 25], 0] = [1e9, -1e30, 250.0, -97.5]     # far outside the cell (the closed form of the wrap); 17, 21, 25: odd, 17: seventh
    fr[TRICLINIC][[29, 31], 1] = [-3e7, 123.25]
    # atoms in the first and in the last tile of every budget map, at both ends of `block` (frames 0 and 2)
    k = 8
    for name, (sx, sy, td) in BUDGET_MAPS.items():
        nx, ny = BUDGET_SHAPES[name]
        last = (R.index2coord(nx - 1, sx[0], td[0]), R.index2coord(ny - 1, sy[0], td[1]))
        for f in (0, 2):
            fr[f][[k, N - 10 - k]] = [sx[0], sy[0], 1.5]
            fr[f][[k + 1, N - 11 - k]] = [last[0], last[1], -0.75]
        k += 2
    for g in GROUPS.values():
        fr[NAN_LAST][g[-1], 0] = np.nan
    fr[NAN_TWO][[NAN_LOW, NAN_HIGH], 0] = np.nan
    return fr


def _system(G, frames, boxes, n_slots=None):
    s = G.System(N, n_slots=n_slots or len(frames))
    for k, f in enumerate(frames):
        s.set_frame(f, boxes[k], slot=k)
    s.group_create_from_ranges("block", [(5, 8294)])
    s.group_create_from_indices("odd", GROUPS["odd"])
    s.group_create_from_indices("seventh", GROUPS["seventh"])
    return s


@pytest.fixture(scope="module")
def world(G):
    fr = _draw()
    boxes = [BOX] * NF
    boxes[NO_BOX], boxes[TRICLINIC] = None, TRIC
    s = _system(G, fr, boxes, n_slots=2 * NF)          # slots 12 .. 23: room for the wrap test's copies
    yield s, fr, boxes
    s.close()


_REFS = {}


def _ref(fr, boxes, mapdef, group, value, frames=range(NF), offset=OFFSET, wrap=False):
    """the restatement over the given frames, computed once -> (Map, n_outside, status, first atom without position)"""
    key = (mapdef, group, value, tuple(frames), wrap)
    if key not in _REFS:
        ref = R.Map(*mapdef)
        frames = list(frames)
        off = None if value == R.COUNT else offset[frames]
        out = ref.accumulate([fr[k] for k in frames], [boxes[k] for k in frames], GROUPS[group], value, off, wrap=wrap, wrap_fn=_wrap_fn)
        ref.count.setflags(write=False); ref.sum_q.setflags(write=False)
        _REFS[key] = (ref,) + out
    return _REFS[key]


def _grid(G, m):
    L = G._lib
    return m.stat(L.GM_STAT_LAST_RANGE_GROUPS), m.stat(L.GM_STAT_LAST_FRAME_GROUPS), m.stat(L.GM_STAT_LAST_CHECK_GROUPS)


def _gv(G, value):
    return {R.COUNT: "count", R.X: G.Dimension.X, R.Y: G.Dimension.Y, R.Z: G.Dimension.Z}[value]


def _bytes_equal(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(_read(a), _read(b)))


# ------------------------------------------------------------------ 1. the frame walk and the range stride
@pytest.mark.parametrize("group", ["block", "odd", "seventh"])
def test_frame_walk_and_range_stride(G, world, group):
    s, fr, boxes = world
    idx, units, n_cus = GROUPS[group], UNITS[group], s.stat("n_cus")
    for value in (R.COUNT, R.Z):
        off = None if value == R.COUNT else OFFSET
        ref, r_out, r_st, r_bad = _ref(fr, boxes, M61, group, value)
        assert r_st[[NAN_LAST, NAN_TWO]].tolist() == [R.E_NO_POSITION] * 2 and np.count_nonzero(r_st) == 2
        assert r_bad[NAN_LAST] == idx[-1] and r_bad[NAN_TWO] == NAN_LOW and r_out[NAN_LAST] == 0 and r_out[NAN_TWO] == 0
        assert int(ref.count.sum()) + int(r_out.sum()) == len(idx) * 10
        for force_global in (False, True):
            lds_bytes = 0 if force_global else 61 * 16 * (4 if value == R.COUNT else 12)
            for rg, fg in SETTINGS:
                m = G.GridMap(s, *M61)
                assert _grid(G, m) == (0, 0, 0)                                        # nothing launched yet
                m.set_launch(rg, fg)
                n_out, st = m.accumulate(group, 0, NF, value=_gv(G, value), offset=off, raise_on_error=False, force_global=force_global)
                what = (group, value, force_global, rg, fg)
                assert st.tolist() == r_st.tolist() and n_out.tolist() == r_out.tolist(), what
                _same(m, ref)
                assert _path(m) == ((0, 1) if force_global else (1, 0))
                # the grid that was launched: the forced one, and the second statement of the launch function
                grid = _grid(G, m)
                assert grid == R.launch(units, n_cus, lds_bytes, NF, rg, fg)[:3], what
                if rg:
                    assert grid[:2] == (min(rg, units), min(fg, NF)), what
                else:
                    assert grid == (-(-units // 256), NF, -(-units // 256)), what         # every test before this file: one frame per workgroup
                # the raising form on frame 11 alone names the smaller atom, and adds nothing
                with pytest.raises(G.GroupError) as e:
                    m.accumulate(group, NAN_TWO, 1, value=_gv(G, value), offset=None if off is None else off[NAN_TWO:], force_global=force_global)
                assert e.value.variant == "InvalidPosition" and e.value.detail == NAN_LOW, what
                _same(m, ref)
                m.close()
            # slots [6, 12) with 2 frame groups: the failing frame 6 is the FIRST frame of a workgroup (and 11 the last of the other)
            part, p_out, p_st, _ = _ref(fr, boxes, M61, group, value, frames=range(6, NF))
            for rg in (1, 2):
                m = G.GridMap(s, *M61)
                m.set_launch(rg, 2)
                n_out, st = m.accumulate(group, 6, 6, value=_gv(G, value), offset=None if off is None else off[6:], raise_on_error=False, force_global=force_global)
                assert st.tolist() == p_st.tolist() == [R.E_NO_POSITION, 0, 0, 0, 0, R.E_NO_POSITION] and n_out.tolist() == p_out.tolist()
                assert _grid(G, m)[:2] == (rg, 2)
                _same(m, part)
                m.close()


# ------------------------------------------------------------------ 2. the check's grid-stride loop
@pytest.mark.parametrize("group", ["block", "odd", "seventh"])
def test_check_stride(G, world, group):
    """one or two workgroups of k_gm_check stride over the whole group: the atom without a position in the last step (frame 6), and the
    smaller of two in different steps (frame 11), are the ones the default grid reports; a clean frame stays clean"""
    s, fr, boxes = world
    default = -(-UNITS[group] // 256)
    assert default >= 5                                                                # 1 workgroup: 5 or 9 steps; 2: 3 or 5
    clean, c_out, c_st, _ = _ref(fr, boxes, M61, group, R.Z, frames=[0])
    for cg in (0, 1, 2):
        m = G.GridMap(s, *M61)
        m.set_launch(check_groups=cg)
        for f, atom in ((NAN_LAST, int(GROUPS[group][-1])), (NAN_TWO, NAN_LOW)):
            with pytest.raises(G.GroupError) as e:
                m.accumulate(group, f, 1, value=G.Dimension.Z)
            assert e.value.variant == "InvalidPosition" and e.value.detail == atom, (cg, f)
            assert _grid(G, m)[2] == (cg or default)
            n_out, st = m.accumulate(group, f, 1, value=G.Dimension.Z, raise_on_error=False)
            assert st.tolist() == [R.E_NO_POSITION] and n_out.tolist() == [0]
        assert not _read(m)[0].any() and not _read(m)[1].any()
        n_out, st = m.accumulate(group, 0, 1, value=G.Dimension.Z, offset=OFFSET[:1])
        assert st.tolist() == [0] == c_st.tolist() and n_out.tolist() == c_out.tolist()
        _same(m, clean)
        m.close()


# ------------------------------------------------------------------ 3. GR_GM_WRAP under the walk
@pytest.mark.parametrize("group", ["block", "odd", "seventh"])
def test_wrap_under_the_walk(G, world, group):
    """frames 0 .. 8 are orthorhombic with moderate coordinates (what the oracle's wrap loops can be run on, see test_gpu_gridmap.test_wrap):
    against the restatement with the oracle's wrap; frame 4 has no box and fails in the MIDDLE of a workgroup's walk, frame 6 has no
    position.  All 12 frames, the triclinic one included: GR_GM_WRAP == gr_group_wrap_batch on a copy + a plain accumulate."""
    s, fr, boxes = world
    before = [s.get_positions(k) for k in range(NF)]
    want_st = [0] * NF
    want_st[NO_BOX], want_st[NAN_LAST], want_st[NAN_TWO] = R.E_NO_BOX, R.E_NO_POSITION, R.E_NO_POSITION
    for k in range(NF):
        s.copy_frame(NF + k, k)
    wst = s.group_wrap_batch(group, NF, NF, raise_on_error=False)
    assert wst.tolist() == want_st
    for value in (R.X, R.Y, R.Z):
        ref, r_out, r_st, _ = _ref(fr, boxes, M61, group, value, frames=range(9), wrap=True)
        assert r_st.tolist() == want_st[:9] and ref.count.sum() > 0
        # the twin: a plain accumulate of the wrapped copies, without the frame that has no box (a plain accumulate needs none)
        b = G.GridMap(s, *M61)
        t1 = b.accumulate(group, NF, NO_BOX, value=_gv(G, value), offset=OFFSET[:NO_BOX], raise_on_error=False)
        t2 = b.accumulate(group, NF + NO_BOX + 1, NF - NO_BOX - 1, value=_gv(G, value), offset=OFFSET[NO_BOX + 1:], raise_on_error=False)
        twin_out = np.concatenate([t1[0], [0], t2[0]])
        for rg, fg in ((1, 1), (2, 3)):
            a = G.GridMap(s, *M61)
            a.set_launch(rg, fg)
            n_out, st = a.accumulate(group, 0, 9, value=_gv(G, value), offset=OFFSET[:9], wrap=True, raise_on_error=False)
            assert st.tolist() == want_st[:9] and n_out.tolist() == r_out.tolist(), (value, rg, fg)
            assert _grid(G, a)[:2] == (rg, fg)
            _same(a, ref)
            a.clear()
            n_out, st = a.accumulate(group, 0, NF, value=_gv(G, value), offset=OFFSET, wrap=True, raise_on_error=False)
            assert st.tolist() == want_st and n_out.tolist() == twin_out.tolist(), (value, rg, fg)
            assert n_out[TRICLINIC] > 0 and _bytes_equal(a, b)
            a.close()
        b.close()
    assert all(np.array_equal(s.get_positions(k).view(np.uint32), before[k].view(np.uint32)) for k in range(NF))     # the frames are not modified


# ------------------------------------------------------------------ 4. one tile, many frames, one workgroup
def test_contention_over_frames(G):
    fr = _draw()
    s = _system(G, [fr[ONE_TILE]], [BOX], n_slots=NF)
    for k in range(1, NF):
        s.copy_frame(k, 0)
    ix, iy = int(R.coord2index([1.0], M61[0][0], M61[2][0])[0]), int(R.coord2index([4.0], M61[1][0], M61[2][1])[0])
    for group, idx in GROUPS.items():
        a = G.GridMap(s, *M61); b = G.GridMap(s, *M61)
        a.set_launch(1, 1); b.set_launch(1, 1)
        for m, force_global in ((a, False), (b, True)):
            n_out, st = m.accumulate(group, 0, NF, value=G.Dimension.Z, offset=OFFSET, force_global=force_global)
            assert not n_out.any() and not st.any() and _grid(G, m)[:2] == (1, 1)
        assert _path(a) == (1, 0) and _path(b) == (0, 1)
        cnt, sq, _ = _read(a)
        want = sum(int(R.quantise((fr[ONE_TILE][idx, 2] - OFFSET[k]).astype(F))[1].sum()) for k in range(NF))
        assert cnt[ix, iy] == NF * len(idx) and cnt.sum() == NF * len(idx)
        assert sq[ix, iy] == want and np.count_nonzero(sq) == 1
        assert _bytes_equal(a, b)
        a.close(); b.close()
    s.close()


# ------------------------------------------------------------------ 5. both sides of the LDS budget
@pytest.mark.parametrize("mapname", ["43x127", "2x2731", "128x128", "145x113"])
def test_lds_budget_edges(G, world, mapname):
    s, fr, boxes = world
    L = G._lib
    mapdef, (nx, ny) = BUDGET_MAPS[mapname], BUDGET_SHAPES[mapname]
    for k, (value, bytes_per_tile) in enumerate(((R.COUNT, 4), (R.Z, 12))):
        on_lds = BUDGET_LDS[mapname][k]
        off = None if value == R.COUNT else OFFSET[:3]
        ref, r_out, r_st, _ = _ref(fr, boxes, mapdef, "block", value, frames=range(3))
        assert not r_st.any() and ref.count[0, 0] >= 4 and ref.count[nx - 1, ny - 1] >= 4 and r_out.sum() > 0          # the first and the last tile are hit
        twin = G.GridMap(s, *mapdef)
        assert (twin.n_tiles_x, twin.n_tiles_y) == (nx, ny)
        budget = twin.stat(L.GM_STAT_LDS_BUDGET)
        assert on_lds == (nx * ny * bytes_per_tile <= budget)
        if (mapname, value) == ("128x128", R.COUNT):
            assert nx * ny * bytes_per_tile == budget                                  # the launch asks for exactly the budget
        if (mapname, value) == ("43x127", R.Z):
            assert nx * ny * bytes_per_tile == budget - 4                              # lcnt lies behind 5461 u64 sums
        n_out, st = twin.accumulate("block", 0, 3, value=_gv(G, value), offset=off, force_global=True)
        assert _path(twin) == (0, 1) and not st.any() and n_out.tolist() == r_out.tolist()
        _same(twin, ref)
        for rg, fg in ((0, 0), (1, 1)) if on_lds else ((0, 0),):
            m = G.GridMap(s, *mapdef)
            m.set_launch(rg, fg)
            n_out, st = m.accumulate("block", 0, 3, value=_gv(G, value), offset=off)
            assert not st.any() and n_out.tolist() == r_out.tolist(), (mapname, value, rg, fg)
            assert _path(m) == ((1, 0) if on_lds else (0, 1)), (mapname, value)
            if rg:
                assert _grid(G, m)[:2] == (1, 1)                                       # the full-size LDS map holds 3 frames when it is flushed
            _same(m, ref)
            assert _bytes_equal(m, twin)
            m.close()
        twin.close()


# ------------------------------------------------------------------ 6. the default grid, no hook
def test_default_shape_walks_several_frames(G):
    """64 frames, a map of 65532 bytes of LDS (2 workgroups per CU): by itself the library launches fewer frame groups than frames"""
    base = _draw()
    rng = np.random.default_rng(64)
    shift = (rng.random((64, 3)) * 0.25 - 0.125).astype(F)
    fr = [(base[k % NF] + shift[k]).astype(F) for k in range(64)]
    boxes = [BOX] * 64
    s = _system(G, fr, boxes)
    mapdef = BUDGET_MAPS["43x127"]
    offset = np.linspace(-2, 2, 64).astype(F)
    m = G.GridMap(s, *mapdef); ref = R.Map(*mapdef)
    n_out, st = m.accumulate("block", 0, 64, value=G.Dimension.Z, offset=offset, raise_on_error=False)
    grid = _grid(G, m)
    print("test_default_shape_walks_several_frames: n_cus %d, (range, frame, check) groups = %r" % (s.stat("n_cus"), grid))
    assert grid == R.launch(UNITS["block"], s.stat("n_cus"), 5461 * 12, 64)[:3]
    assert grid[1] < 64 and _path(m) == (1, 0)
    r_out, r_st, _ = ref.accumulate(fr, boxes, GROUPS["block"], R.Z, offset)
    assert st.tolist() == r_st.tolist() and n_out.tolist() == r_out.tolist()
    assert np.nonzero(r_st)[0].tolist() == [k for k in range(64) if k % NF in (NAN_LAST, NAN_TWO)] and set(r_st.tolist()) == {0, R.E_NO_POSITION}
    _same(m, ref)
    m.close(); s.close()


# ------------------------------------------------------------------ 7. offsets that are not finite, values on either side of +-2^31
def test_offsets_and_value_limits(G, world):
    s, fr, boxes = world
    for group, idx in GROUPS.items():
        m = G.GridMap(s, *M61)
        off = np.array([np.nan, np.inf, -np.inf], F)
        n_out, st = m.accumulate(group, 0, 3, value=G.Dimension.Z, offset=off)
        r_out, r_st, _ = R.Map(*M61).accumulate(fr[:3], boxes[:3], idx, R.Z, off)
        assert st.tolist() == [0, 0, 0] == r_st.tolist() and n_out.tolist() == [len(idx)] * 3 == r_out.tolist()
        assert not _read(m)[0].any() and not _read(m)[1].any()
        m.close()
    # z - offset = the largest accepted value, 2^31, and their negatives, in one tile; every other atom outside the map in x
    n = 600
    big = np.nextafter(F(2.0 ** 31), F(0))
    pos = np.zeros((n, 3), F); pos[:, 0] = 100.0; pos[:, 1] = 4.0
    z0 = np.array([big, 2.0 ** 31, -big, -2.0 ** 31], F)
    z1 = np.array([2.0 ** 30, 2.0 ** 30 + 128, -(3 * 2.0 ** 30 - 256), -3 * 2.0 ** 30], F)       # the same four values of v after offset[1] = -(2^30 - 128)
    off = np.array([0.0, -(2.0 ** 30 - 128)], F)
    assert (z1 - off[1]).astype(F).tolist() == z0.tolist()
    frames = [pos.copy(), pos.copy()]
    atoms = [7, 300, 301, 599]                                                            # group order is atom order: spread over the waves
    for f, z in zip(frames, (z0, z1)):
        f[atoms, 0] = 1.0; f[atoms, 2] = z
    t = G.System(n, n_slots=2)
    for k in range(2):
        t.set_frame(frames[k], BOX, slot=k)
    thirds = np.unique(np.concatenate([np.arange(1, n, 3), [300, 599]]))                  # an index list; "all" is a block
    t.group_create_from_indices("thirds", thirds)
    ix, iy = int(R.coord2index([1.0], M61[0][0], M61[2][0])[0]), int(R.coord2index([4.0], M61[1][0], M61[2][1])[0])
    for group, idx in (("all", np.arange(n)), ("thirds", thirds)):
        assert np.isin(atoms, idx).all()
        for force_global in (False, True):
            for rg, fg in ((0, 0), (1, 1)):
                m = G.GridMap(t, *M61); ref = R.Map(*M61)
                m.set_launch(rg, fg)
                n_out, st = m.accumulate(group, 0, 1, value=G.Dimension.Z, force_global=force_global)
                r_out, r_st, _ = ref.accumulate(frames[:1], [BOX], idx, R.Z)
                assert st.tolist() == [0] == r_st.tolist() and n_out.tolist() == r_out.tolist() == [len(idx) - 2]      # +-2^31 count as outside
                _same(m, ref)
                cnt, sq, _ = _read(m)
                assert cnt[ix, iy] == 2 and cnt.sum() == 2 and not sq.any()                # +-(2^51 - 2^27) quanta cancel to exactly 0
                n_out, st = m.accumulate(group, 0, 2, value=G.Dimension.Z, offset=off, force_global=force_global)      # and with an offset, two frames in one walk
                r_out, r_st, _ = ref.accumulate(frames, [BOX, BOX], idx, R.Z, off)
                assert st.tolist() == [0, 0] == r_st.tolist() and n_out.tolist() == r_out.tolist() == [len(idx) - 2] * 2
                _same(m, ref)
                cnt, sq, _ = _read(m)
                assert cnt[ix, iy] == 6 and cnt.sum() == 6 and not sq.any()
                m.clear(); ref.clear()
                # one sign alone: the sum is there
                only = frames[0].copy(); only[atoms[2], 0] = 100.0
                t.set_frame(only, BOX, slot=0)
                m.accumulate(group, 0, 1, value=G.Dimension.Z, force_global=force_global)
                ref.accumulate([only], [BOX], idx, R.Z)
                _same(m, ref)
                assert _read(m)[1][ix, iy] == 2 ** 51 - 2 ** 27 and _read(m)[0][ix, iy] == 1
                t.set_frame(frames[0], BOX, slot=0)
                m.close()
    t.close()


# ------------------------------------------------------------------ 8. the hook itself
def test_set_launch_is_not_sticky(G, world):
    s, fr, boxes = world
    lib = G._lib.load()
    assert lib.gr_gridmap_set_launch(None, 1, 1, 1) == G._lib.E_INVALID_ARG
    fresh = G.GridMap(s, *M61); m = G.GridMap(s, *M61)
    m.set_launch(1, 1, 1)
    m.set_launch(0, 0, 0)
    for x in (fresh, m):
        x.accumulate("block", 0, NF, value=G.Dimension.Z, offset=OFFSET, raise_on_error=False)
    assert _grid(G, m) == _grid(G, fresh) == (9, NF, 9)
    assert _bytes_equal(m, fresh)
    m.set_launch(1, 1, 1)                                                                 # and set again, it holds: every key is its own
    m.clear()
    m.accumulate("block", 0, NF, value=G.Dimension.Z, offset=OFFSET, raise_on_error=False)
    assert _grid(G, m) == (1, 1, 1) and _bytes_equal(m, fresh)
    m.set_launch(frame_groups=5)
    m.clear()
    m.accumulate("block", 0, NF, value=G.Dimension.Z, offset=OFFSET, raise_on_error=False)
    assert _grid(G, m) == (9, 5, 9) and _bytes_equal(m, fresh)
    v = C.c_uint64(7)
    assert lib.gr_gridmap_stat(m._map, 7, C.byref(v)) == G._lib.E_INVALID_ARG              # keys 4 .. 6 are the new ones; 7 is none
    fresh.close(); m.close()

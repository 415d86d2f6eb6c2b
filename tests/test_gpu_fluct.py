"""Fluctuations over resident frames (gr_fluct_*; groan_rs_amd.Fluctuations) against the numpy restatement tests/fluct_ref.py.

The RAW state (origin, sums, sums of squares, n) is compared bit for bit: it is defined by a sequential walk over the counted frames.
The CLOSED results (mean, variance, RMSF) are held within 1e-5 nm -- the project's tolerance for centres and RMSDs --
against an independent two-pass f64 reference; the restatement's own error on these inputs is below 1e-6 (tests/test_fluct_host.py).
The system has 1000 atoms (one partial 256-atom tile: the pads must never enter a sum), 37 fitted frames in slots 0..36 within
|x| <= 16 nm, slot 20 without a box.  Groups: a block that is not 4-aligned, every third atom (index list), two ranges dense enough to
be walked through a bit mask, all atoms, one atom, four atoms aligned and not."""
import numpy as np
import pytest

import fluct_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
N, NF = 1000, 37
BOX = [40.0, 40.0, 40.0]
GROUPS = {"block": np.arange(3, 771), "third": np.arange(0, N, 3), "two": np.concatenate([np.arange(10, 301), np.arange(500, 901)]), "all": np.arange(N),
          "one": np.arange(517, 518), "four": np.arange(256, 260), "four_odd": np.arange(509, 513)}
RANGES = {"block": [(3, 770)], "two": [(10, 300), (500, 900)], "one": [(517, 517)], "four": [(256, 259)], "four_odd": [(509, 512)]}
FORM = {"block": 0, "third": 1, "two": 2, "all": 0, "one": 0, "four": 0, "four_odd": 0}
TOL = 1e-5
NAN_ATOM = 6                  # in block, third and all; not in two


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def make_groups(s):
    for name, ranges in RANGES.items():
        s.group_create_from_ranges(name, ranges)
    s.group_create_from_indices("third", GROUPS["third"])


def make_system(G, frames, n_slots=None, no_box=(), masses=None):
    s = G.System(len(frames[0]), n_slots=n_slots or len(frames), masses=masses)
    for k, x in enumerate(frames):
        s.set_frame(x, None if k in no_box else BOX, slot=k)
    if len(frames[0]) == N:
        make_groups(s)
    return s


@pytest.fixture(scope="module")
def frames():
    return R.fitted_frames(N, NF, 20261020)


@pytest.fixture(scope="module")
def world(G, frames):
    s = make_system(G, frames, n_slots=NF + 3, no_box=(20,))
    yield s
    s.close()


def ref_state(frames, group):
    st = R.State(len(GROUPS[group]))
    status, bad = st.accumulate(frames, GROUPS[group])
    return st, status, bad


def same_raw(fl, st):
    o, s, q, n = fl.raw()
    assert n == st.n == fl.n_frames
    assert R.same_bits(o, st.o) and R.same_bits(s, st.s) and R.same_bits(q, st.q)


def raw_bits(fl):
    o, s, q, n = fl.raw()
    return o.tobytes(), s.tobytes(), q.tobytes(), n, *(x.tobytes() for x in (fl.mean(), fl.variance(), fl.rmsf()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("nf", [1, 2, NF])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_raw_state_is_the_restatement_bit_for_bit(G, world, frames, group, nf):
    with G.Fluctuations(world, group) as fl:
        assert fl.n_atoms == len(GROUPS[group]) and fl.stat(G._lib.FL_STAT_FORM) == FORM[group] and fl.n_frames == 0
        status = fl.accumulate(0, nf)
        assert status.dtype == np.int32 and not status.any()                     # slot 20 has no box: counted all the same
        same_raw(fl, ref_state(frames[:nf], group)[0])
        assert fl.stat(G._lib.FL_STAT_LAUNCHES) == 1 and fl.stat(G._lib.FL_STAT_AHEAD) == R.source_ahead()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_closed_results_against_the_two_pass_reference(G, world, frames, group):
    with G.Fluctuations(world, group) as fl:
        fl.accumulate(0, NF)
        mean, var, rmsf = fl.mean(), fl.variance(), fl.rmsf()
    m2, v2, r2 = R.two_pass(frames, GROUPS[group])
    assert mean.dtype == var.dtype == rmsf.dtype == np.float64 and mean.shape == (len(GROUPS[group]), 3) and rmsf.shape == (len(GROUPS[group]),)
    assert np.abs(mean - m2).max() <= TOL and np.abs(var - v2).max() <= TOL and np.abs(rmsf - r2).max() <= TOL
    assert 0.01 < rmsf.mean() < 0.8                                              # (the frames do move)
    # the library's closing step is the restatement's
    cm, cv, cr = ref_state(frames, group)[0].close()
    assert np.abs(mean - cm).max() <= 1e-12 and np.abs(var - cv).max() <= 1e-12 and np.abs(rmsf - cr).max() <= 1e-12


def test_frames_jumping_across_the_box(G):
    fr = R.jumping_frames(N, 24, 77)
    s = make_system(G, fr)
    for group in ("block", "third", "two"):
        with G.Fluctuations(s, group) as fl:
            fl.accumulate(0, 24)
            same_raw(fl, ref_state(fr, group)[0])
            m2, v2, r2 = R.two_pass(fr, GROUPS[group])
            assert np.abs(fl.mean() - m2).max() <= TOL and np.abs(fl.rmsf() - r2).max() <= TOL
    s.close()


def test_rigid_copies_and_one_frame(G, world, frames):
    s = make_system(G, [frames[3]] * 5)
    for group in ("block", "third", "two", "all"):
        x = frames[3][GROUPS[group]].astype(np.float64)
        with G.Fluctuations(s, group) as fl:
            fl.accumulate(0, 5)
            assert fl.n_frames == 5 and np.array_equal(fl.mean(), x) and not fl.rmsf().any() and not fl.variance().any()
            o, sm, sq, n = fl.raw()
            assert not sm.any() and not sq.any()
        with G.Fluctuations(world, group) as fl:                                  # one frame: the mean is the frame
            fl.accumulate(3, 1)
            assert fl.n_frames == 1 and np.array_equal(fl.mean(), x) and not fl.rmsf().any()
    s.close()


@pytest.mark.parametrize("launch", [(0, 0), (1, 1), (3, 2), (5000, 0)])
def test_split_invariance(G, world, launch):
    for group in ("block", "third", "two", "four_odd"):
        a, b, c = (G.Fluctuations(world, group) for _ in range(3))
        for fl in (a, b, c):
            fl.set_launch(*launch)
        a.accumulate(0, NF)
        for k in range(NF):
            b.accumulate(k, 1)
        c.accumulate(0, 5); c.accumulate(5, 32)
        assert raw_bits(a) == raw_bits(b) == raw_bits(c)
        d = G.Fluctuations(world, group)                                          # ... and the default launch gives the same
        d.accumulate(0, NF)
        assert raw_bits(a) == raw_bits(d)
        if launch[0]:
            assert a.stat(G._lib.FL_STAT_LAST_RANGE_GROUPS) == launch[0]
        for fl in (a, b, c, d):
            fl.close()


@pytest.mark.parametrize("where", [0, 3, 7])
def test_failing_frames(G, frames, where):
    fr = [x.copy() for x in frames[:8]]
    fr[where][NAN_ATOM] = np.nan
    s = make_system(G, fr)
    before = [s.get_positions(k) for k in range(8)]
    for group in ("block", "third", "two", "all"):
        hit = NAN_ATOM in GROUPS[group]
        st, status, bad = ref_state(fr, group)
        fl = G.Fluctuations(s, group)
        got = fl.accumulate(0, 8, raise_on_error=False)
        assert got.tolist() == status.tolist() and (got[where] == R.E_NO_POSITION) == hit
        same_raw(fl, st)
        assert fl.n_frames == (7 if hit else 8)
        if hit:
            first = 1 if where == 0 else 0
            assert R.same_bits(fl.raw()[0], fr[first][GROUPS[group]])            # the origin: the first COUNTED frame
            keep = raw_bits(fl)
            with pytest.raises(G.GroupError) as e:
                fl.accumulate(where, 1)
            assert e.value.variant == "InvalidPosition" and e.value.detail == NAN_ATOM and e.value.status == R.E_NO_POSITION
            assert raw_bits(fl) == keep                                           # the failed frame added nothing
            with pytest.raises(G.GroupError) as e:                                # first error of a batch: the first failing frame's
                fl.accumulate(0, 8)
            assert e.value.detail == NAN_ATOM
        fl.close()
    assert all(np.array_equal(bits(s.get_positions(k)), bits(before[k])) for k in range(8))      # the frames are never modified
    s.close()


def test_every_frame_failing(G, frames):
    fr = [x.copy() for x in frames[:4]]
    for k, x in enumerate(fr):
        x[[NAN_ATOM + 3 * k, 300]] = np.nan
    s = make_system(G, fr + [frames[5]])
    with G.Fluctuations(s, "third") as fl:
        got = fl.accumulate(0, 4, raise_on_error=False)
        assert got.tolist() == [R.E_NO_POSITION] * 4 and fl.n_frames == 0
        assert all(np.isnan(x).all() for x in (fl.mean(), fl.variance(), fl.rmsf()))
        with pytest.raises(G.GroupError) as e:
            fl.accumulate(1, 3)
        assert e.value.detail == NAN_ATOM + 3                                     # the lowest atom of the first failing frame
        fl.accumulate(4, 1)
        keep = raw_bits(fl)
        assert fl.accumulate(0, 4, raise_on_error=False).tolist() == [R.E_NO_POSITION] * 4
        assert raw_bits(fl) == keep and fl.n_frames == 1                          # all frames failing: the state is unchanged
    s.close()


def test_nan_outside_the_group_changes_nothing(G, frames):
    """atoms without position next to the group: in the 4-atom groups its ends share, around a lone atom, between the entries of a list"""
    sparse = np.arange(3, N, 5)
    outside = {"block": [0, 1, 2, 771, 772], "one": [516, 518, 519, 513], "four": [255, 260, 252], "four_odd": [508, 513, 514, 515], "two": [9, 8, 301, 302, 499, 901],
               "sparse": [2, 4, 5, 6, 7, 997, 999, 256]}
    for group, out in outside.items():
        idx = sparse if group == "sparse" else GROUPS[group]
        assert not set(out) & set(idx.tolist())
        fr = [x.copy() for x in frames[:6]]
        for k, x in enumerate(fr):
            x[out[k % 2::2]] = np.nan                                             # some of them in every frame
        s = make_system(G, fr)
        s.group_create_from_indices("sparse", sparse)
        with G.Fluctuations(s, group) as fl:
            assert fl.stat(G._lib.FL_STAT_FORM) == (1 if group == "sparse" else FORM[group])
            assert not fl.accumulate(0, 6).any()
            st = R.State(len(idx)); st.accumulate(fr, idx)
            same_raw(fl, st)
            assert np.isfinite(fl.mean()).all() and np.isfinite(fl.rmsf()).all()
        s.close()


def test_a_frame_without_a_box_is_counted(G, world):
    assert not world.has_box(20)
    with G.Fluctuations(world, "all") as fl:
        assert fl.accumulate(20, 1).tolist() == [0] and fl.n_frames == 1


def test_store_mean(G, world, frames):
    rng = np.random.default_rng(9)
    other = (rng.random((N, 3)) * 8).astype(F)
    t = G.System(N, n_slots=2)
    t.set_frame(other, [7.0, 8.0, 9.0], slot=1)
    small = G.System(N - 1, n_slots=1)
    for group in ("block", "third", "two", "one"):
        idx = GROUPS[group]
        with G.Fluctuations(world, group) as fl:
            with pytest.raises(G.DeviceError) as e:                               # nothing counted: there is no mean
                fl.store_mean(t, 1)
            assert e.value.status == R.E_INVALID_ARG
            fl.accumulate(0, NF)
            with pytest.raises(G.DeviceError) as e:                               # a context with another number of atoms
                fl.store_mean(small, 0)
            assert e.value.status == R.E_INVALID_ARG
            mean = fl.mean().astype(F)
            for target, slot, was in ((t, 1, other), (world, NF + 1, None)):      # another context of the device, and the object's own
                if was is None:
                    world.copy_frame(slot, 0)
                    was = frames[0]
                box = target.get_box(slot).copy()
                fl.store_mean(target, slot)
                got = target.get_positions(slot)
                expect = was.copy(); expect[idx] = mean
                assert np.array_equal(bits(got), bits(expect))                    # the group's atoms: float32(mean); every other atom keeps its bits
                assert np.array_equal(bits(target.get_box(slot)), bits(box))
                target.set_frame(was, "keep", slot=slot)
    assert all(np.array_equal(bits(world.get_positions(k)), bits(frames[k])) for k in (0, 19, NF - 1))
    small.close(); t.close()


def _rotation(rng):
    q = rng.standard_normal(4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_round_trip_through_a_new_rmsd_plan(G):
    """fit -> mean -> store -> a new plan on the stored mean -> fit: the "fit to the average, iterate" loop converges"""
    rng = np.random.default_rng(31)
    nf, centre = 10, np.array([5.0, 5.0, 5.0])
    base = (rng.random((N, 3)) * 2 - 1) * 1.5
    fr = [(((base + 0.05 * rng.standard_normal((N, 3))) @ _rotation(rng).T) + centre + 0.3 * rng.standard_normal(3)).astype(F) for _ in range(nf)]
    s = G.System(N, n_slots=nf + 2, masses=np.ones(N, F))
    for k in range(nf):
        s.set_frame(fr[k], [10.0, 10.0, 10.0], slot=k)
    s.group_create_from_ranges("block", RANGES["block"])
    s.copy_frame(nf, 0); s.copy_frame(nf + 1, 0)
    idx = GROUPS["block"]
    plan = G.RMSDPlan(s, s, "block", ref_slot=nf)
    r1, st1 = plan.rmsd_fit(0, nf)
    assert not st1.any()
    fl = G.Fluctuations(s, "block")
    fl.accumulate(0, nf)
    mean1 = fl.mean()
    first = s.get_positions(0)[idx].astype(np.float64)
    fl.store_mean(s, nf + 1)
    plan2 = G.RMSDPlan(s, s, "block", ref_slot=nf + 1)
    r2, st2 = plan2.rmsd_fit(0, nf)
    assert not st2.any() and np.isfinite(r2).all()
    fl.clear(); fl.accumulate(0, nf)
    mean2 = fl.mean()
    rmsd = lambda a, b: float(np.sqrt(((a - b) ** 2).sum(1).mean()))
    assert np.isfinite(rmsd(mean2, mean1)) and rmsd(mean2, mean1) < rmsd(first, mean1)
    assert r2.mean() < r1.mean()                                                  # the frames lie closer to their average than to the first frame
    s.close()


def test_merge(G, world, frames):
    cut = 20
    w2 = make_system(G, frames[cut:])
    small = G.System(N, n_slots=1)
    small.group_create_from_ranges("block", [(3, 700)])
    for group in ("block", "third", "two"):
        a, b, empty = G.Fluctuations(world, group), G.Fluctuations(w2, group), G.Fluctuations(w2, group)
        a.accumulate(0, cut); b.accumulate(0, NF - cut)
        keep_a, keep_b = raw_bits(a), raw_bits(b)
        a.merge(empty)                                                            # an empty src changes nothing
        assert raw_bits(a) == keep_a
        empty.merge(b)                                                            # an empty dst takes src's origin and sums unchanged
        assert raw_bits(empty) == keep_b and raw_bits(b) == keep_b
        a.merge(b)
        assert a.n_frames == NF and raw_bits(b) == keep_b
        m2, v2, r2 = R.two_pass(frames, GROUPS[group])
        assert np.abs(a.mean() - m2).max() <= TOL and np.abs(a.variance() - v2).max() <= TOL and np.abs(a.rmsf() - r2).max() <= TOL
        ra, _, _ = ref_state(frames[:cut], group); rb, _, _ = ref_state(frames[cut:], group)
        ra.merge(rb)
        o, sm, sq, n = a.raw()
        assert R.same_bits(o, ra.o) and np.abs(sm - ra.s).max() <= 1e-9 and np.abs(sq - ra.q).max() <= 1e-9
        for fl in (a, b, empty):
            fl.close()
    a, c = G.Fluctuations(world, "block"), G.Fluctuations(small, "block")
    with pytest.raises(G.GroupError) as e:
        a.merge(c)
    assert e.value.variant == "InconsistentGroup" and e.value.detail[1:] == (768, 698) and e.value.status == R.E_INCONSISTENT_GROUP
    a.close(); c.close(); small.close(); w2.close()


def test_history_independence(G, frames):
    fresh, used = make_system(G, frames[:10], n_slots=20, masses=np.ones(N, F)), make_system(G, frames[:10], n_slots=20, masses=np.ones(N, F))
    for k in range(10):
        used.copy_frame(10 + k, k)
    used.group_center_batch("all", G._lib.CENTER_PBC, 1, 0, 10, raise_on_error=False)
    plan = G.RMSDPlan(used, used, "block", ref_slot=10)
    plan.rmsd_fit(11, 9, raise_on_error=False)
    gm = G.GridMap(used, (-16.0, 16.0), (-16.0, 16.0), (0.5, 0.5))
    gm.accumulate("third", 0, 10, value=G.Dimension.Z)
    for group in ("block", "third", "two", "all"):
        with G.Fluctuations(fresh, group) as a, G.Fluctuations(used, group) as b:
            a.accumulate(0, 10); b.accumulate(0, 10)
            assert raw_bits(a) == raw_bits(b)
    fresh.close(); used.close()


def test_clear(G, world, frames):
    for group in ("block", "third", "two"):
        with G.Fluctuations(world, group) as a, G.Fluctuations(world, group) as b:
            a.accumulate(7, 11)
            a.clear()
            assert a.n_frames == 0 and np.isnan(a.mean()).all()
            a.accumulate(2, 9); b.accumulate(2, 9)
            assert raw_bits(a) == raw_bits(b)
            same_raw(a, ref_state(frames[2:11], group)[0])


def test_errors_and_lifetime(G, world):
    with pytest.raises(G.GroupError) as e:
        G.Fluctuations(world, "nothing")
    assert e.value.variant == "NotFound"
    world.group_create_from_indices("empty", [])
    with pytest.raises(G.GroupError) as e:
        G.Fluctuations(world, "empty")
    assert e.value.variant == "EmptyGroup"
    fl = G.Fluctuations(world, "block")
    with pytest.raises(G.DeviceError):
        fl.accumulate(NF + 2, 5)                                                  # slots out of range: a hard error
    assert fl.n_frames == 0
    # the object keeps its snapshot: replacing the group afterwards changes nothing
    world.group_create_from_ranges("moving", [(100, 400)])
    mv = G.Fluctuations(world, "moving")
    try:
        world.group_create_from_ranges("moving", [(0, 10)])
    except G.GroanError:
        pass                                                                      # (the library reports that the group existed)
    mv.accumulate(0, 3)
    assert mv.n_atoms == 301 and np.isfinite(mv.mean()).all()
    mv.close(); fl.close()
    c, st = world.group_center_batch("all", 0, 0, 3, 1)                           # closing the objects leaves the context usable
    assert st[0] == 0 and np.isfinite(c).all()

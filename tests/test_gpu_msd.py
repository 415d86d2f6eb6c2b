"""MSD over resident frames (gr_msd_*; groan_rs_amd.MSD) against the numpy restatement tests/msd_ref.py.

The DISPLACEMENTS (the panel) are compared bit for bit: they are defined by a sequential walk over the appended frames.

The MSD VALUES are held against the restatement's direct evaluation sum (d_t - d_t')^2 (long double: its own error is 2^-11 of the
bound) under a DERIVED bound.  Per pair the device forms D2 = (q_t + q_t') - 2 G with K = 3 n_pad values per row, u = 2^-53:
  q_t   a sum of K exact products in some fixed order:            |dq_t| <= (K - 1) u q_t
  G     one chain of K exact products (four per instruction):     |dG| <= K u sum |x y| <= K u (q_t + q_t') / 2
  q_t + q_t' rounds once: u (q_t + q_t');  2 G is exact;  the subtraction rounds once: u |D2| <= 2 u (q_t + q_t')
so |D2 - exact| <= ((K - 1) + K + 1 + 2) u (q_t + q_t') = (2 K + 2) u (q_t + q_t'), stated as (2 K + 4) u (q_t + q_t') to cover the second-
order terms of the chains.  (The issue's sketch has 4 K; the derivation gives the smaller constant, which is the one used.)  A lag's P
pairs are added in at most P additions, each within u of a partial sum that is at most sum |D2| <= 2 sum (q_t + q_t'): msd_ref.msd_bound.
Measured worst share of the bound: 0.0016 (one pair, lag T - 1), 0.0047 (a whole lag) -- the products' errors are of random sign.

System: 300 atoms, 130 frames of a random walk per cell (three block rows of the Gram matrix).  Groups: a block that starts at atom 3,
every third atom (index list), two ranges dense enough for the bit mask."""
import functools

import numpy as np
import pytest

import msd_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
N, NF = 300, 130
GROUPS = {"block": np.arange(3, 203), "third": np.arange(0, N, 3), "two": np.concatenate([np.arange(10, 101), np.arange(150, 281)])}
RANGES = {"block": [(3, 202)], "two": [(10, 100), (150, 280)]}
SEED = 20261023


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@functools.lru_cache(maxsize=None)
def walk(cell, n_atoms=N, n_frames=NF, seed=SEED):
    return R.walk(n_atoms, n_frames, seed, cell)


def make_groups(s):
    for name, ranges in RANGES.items():
        s.group_create_from_ranges(name, ranges)
    s.group_create_from_indices("third", GROUPS["third"])


def make_system(G, frames, boxes, n_slots=None):
    s = G.System(len(frames[0]), n_slots=n_slots or len(frames))
    for k, x in enumerate(frames[:n_slots or len(frames)]):
        s.set_frame(x, None if boxes[k] is None else [float(v) for v in boxes[k]], slot=k)
    if len(frames[0]) == N:
        make_groups(s)
    return s


@pytest.fixture(scope="module")
def worlds(G):
    ws = {cell: make_system(G, *walk(cell)[:2]) for cell in R.CELLS}
    yield ws
    for s in ws.values():
        s.close()


@functools.lru_cache(maxsize=None)
def ref(cell, group, dims="xyz", nojump=True):
    frames, boxes = walk(cell)[:2]
    w = R.Walk(len(GROUPS[group]), dims=dims, nojump=nojump)
    st, bad = w.append(frames, boxes, GROUPS[group])
    assert not st.any()
    return w


def state_bits(m, max_lag=None):
    msd, pairs = m.msd(max_lag)
    return m.displacements(0, m.n_frames).tobytes(), m.from_origin().tobytes(), msd.tobytes(), pairs.tobytes()


def check_values(G, m, panel, ok, max_lag=None):
    """msd, pairs, msd[0] and from_origin of `m` against the direct evaluation of `panel`; -> the worst share of the bound"""
    S, n_pad = m.n_atoms, m.stat(G._lib.MSD_STAT_N_PAD)
    assert n_pad % 64 == 0 and 0 <= n_pad - S < 64
    msd, pairs = m.msd(max_lag)
    want, wpairs, qsum = R.direct_msd(panel, ok, max_lag, dtype=np.longdouble)
    assert msd.dtype == np.float64 and pairs.dtype == np.uint64 and np.array_equal(pairs, wpairs)
    if pairs[0]:
        assert msd[0] == 0.0 and not np.signbit(msd[0])
    assert np.array_equal(np.isnan(msd), pairs == 0)
    have = pairs > 0
    bound = R.msd_bound(qsum, pairs, n_pad, S)
    err = np.abs(msd[have] - want[have])
    assert (err <= bound[have]).all(), (err / np.maximum(bound[have], 1e-300)).max()
    share = float((err[1:] / bound[have][1:]).max()) if have.sum() > 1 else 0.0
    # from_origin: q_t / S with q_t a sum of K exact squares
    X = panel.reshape(len(panel), -1).astype(np.longdouble)
    q = np.asarray((X * X).sum(1), np.float64)
    fo = m.from_origin()
    okv = np.asarray(ok, bool)
    assert np.isnan(fo[~okv]).all() and (np.abs(fo[okv] - q[okv] / S) <= 3 * n_pad * 2.0 ** -53 * q[okv] / S).all()
    return share


@pytest.mark.parametrize("nojump", [True, False])
@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("cell", sorted(R.CELLS))
def test_displacements_are_the_restatement_bit_for_bit(G, worlds, cell, group, nojump):
    with G.MSD(worlds[cell], group, NF, nojump=nojump) as m:
        assert m.n_atoms == len(GROUPS[group]) and m.capacity == NF and m.n_frames == 0
        st = m.append(0, NF)
        assert st.dtype == np.int32 and not st.any() and m.n_frames == NF
        d = m.displacements(0, NF)
        assert d.dtype == F and d.shape == (NF, len(GROUPS[group]), 3)
        assert R.same_bits(d, ref(cell, group, "xyz", nojump).panel())
        assert R.same_bits(m.displacements(7, 3), d[7:10])
        assert m.stat(G._lib.MSD_STAT_COUNTED) == NF


@pytest.mark.parametrize("cell", sorted(R.CELLS))
def test_msd_values_within_the_derived_bound(G, worlds, cell):
    for group in sorted(GROUPS):
        w = ref(cell, group)
        with G.MSD(worlds[cell], group, NF) as m:
            m.append(0, NF)
            share = check_values(G, m, w.panel(), w.ok)
            msd, pairs = m.msd()
            assert len(msd) == NF and pairs.tolist() == list(range(NF, 0, -1))
            # one pair on its own: lag NF - 1 is the pair (0, NF - 1)
            X = w.panel().reshape(NF, -1).astype(np.longdouble)
            d2 = float(((X[-1] - X[0]) ** 2).sum())
            q = float((X[-1] ** 2).sum() + (X[0] ** 2).sum())
            one = abs(msd[-1] * m.n_atoms - d2) / ((6 * m.stat(G._lib.MSD_STAT_N_PAD) + 4) * 2.0 ** -53 * q)
            print("%s %s: worst share of the bound %.4f (a lag), %.4f (one pair)" % (cell, group, share, one))
            assert one <= 1.0
            # the random walk's law, loosely: the curve grows like 3 sigma^2 tau
            assert 0.5 < msd[10] / (3 * R.SIGMA ** 2 * 10) < 1.5


def test_dimension_masks(G, worlds):
    world = worlds["tric"]
    curves = {}
    for dims in ("xy", "z", "xyz", "x"):
        w = ref("tric", "third", dims)
        with G.MSD(world, "third", NF, dims=dims) as m:
            m.append(0, NF)
            assert R.same_bits(m.displacements(0, NF), w.panel())
            check_values(G, m, w.panel(), w.ok)
            curves[dims] = m.msd()[0]
            n_pad, S = m.stat(G._lib.MSD_STAT_N_PAD), m.n_atoms
    assert not ref("tric", "third", "xy").panel()[:, :, 2].any() and ref("tric", "third", "z").panel()[:, :, 2].any()
    # z + xy = xyz within the three curves' bounds
    total = sum(R.msd_bound(R.direct_msd(ref("tric", "third", d).panel(), [True] * NF)[2], np.arange(NF, 0, -1).astype(np.uint64), n_pad, S) for d in ("xy", "z", "xyz"))
    assert (np.abs(curves["xy"] + curves["z"] - curves["xyz"]) <= total).all()


@pytest.mark.parametrize("cell", ["rescaled", "tric"])
def test_cut_invariance(G, worlds, cell):
    """one call, calls of 1, 7 and 64 frames, and reloads of the slots: the same bits"""
    world = worlds[cell]
    frames, boxes = walk(cell)[:2]
    for group in sorted(GROUPS):
        one = G.MSD(world, group, NF); one.append(0, NF)
        keep = state_bits(one)
        for cut in (1, 7, 64):
            m = G.MSD(world, group, NF)
            for k in range(0, NF, cut):
                m.append(k, min(cut, NF - k))
            assert state_bits(m) == keep, cut
            m.close()
        one.close()
    small = make_system(G, frames, boxes, n_slots=48)                # a trajectory longer than the slots: block by block through the same slots
    for group in sorted(GROUPS):
        m = G.MSD(small, group, NF)
        for k in range(0, NF, 48):
            n = min(48, NF - k)
            for j in range(n):
                small.set_frame(frames[k + j], [float(v) for v in boxes[k + j]], slot=j)
            m.append(0, n)
        one = G.MSD(world, group, NF); one.append(0, NF)
        assert state_bits(m) == state_bits(one)
        m.close(); one.close()
    small.close()


@pytest.mark.parametrize("launch", [(1, 1), (3, 2), (5000, 5), (2, 0)])
def test_grid_independence(G, worlds, launch):
    world = worlds["tric"]
    for group in sorted(GROUPS):
        with G.MSD(world, group, NF) as a, G.MSD(world, group, NF) as b:
            b.set_launch(*launch)
            a.append(0, NF); b.append(0, 50); b.append(50, NF - 50)
            assert state_bits(a) == state_bits(b)
            assert state_bits(a, 70) == state_bits(b, 70)
            assert b.stat(G._lib.MSD_STAT_LAST_WALK_GROUPS) == launch[0]
            if launch[1]:
                assert b.stat(G._lib.MSD_STAT_LAST_GRAM_GROUPS) == launch[1] < a.stat(G._lib.MSD_STAT_LAST_GRAM_GROUPS)


def test_history_independence(G, worlds):
    frames, boxes = walk("ortho")[:2]
    used = make_system(G, frames, boxes, n_slots=NF)
    used.group_center_batch("all", G._lib.CENTER_PBC, 1, 0, 10, raise_on_error=False)
    fl = G.Fluctuations(used, "third"); fl.accumulate(0, 20)
    other = G.MSD(used, "two", 40, dims="z", nojump=False); other.append(5, 30); other.msd()
    for group in sorted(GROUPS):
        with G.MSD(worlds["ortho"], group, NF) as a, G.MSD(used, group, NF) as b:
            a.append(0, NF); b.append(0, NF)
            assert state_bits(a) == state_bits(b)
    used.close()


def _failing(G):
    frames, boxes = walk("ortho", N, 24, SEED + 1)[:2]
    frames, boxes = [x.copy() for x in frames], list(boxes)
    inside, outside = 60, 1                                           # atom 60 is in block, third and two; atom 1 in none of them
    assert all(inside in GROUPS[g] and outside not in GROUPS[g] for g in GROUPS)
    frames[3][inside] = np.nan; frames[5][outside] = np.nan; boxes[9] = None
    frames[12][[inside, inside + 30]] = np.nan; boxes[12] = None      # both: the host check's error comes first
    return frames, boxes, inside


def test_failed_frames(G):
    frames, boxes, inside = _failing(G)
    s = make_system(G, frames, boxes)
    for group in sorted(GROUPS):
        for nojump in (True, False):
            w = R.Walk(len(GROUPS[group]), nojump=nojump)
            st, bad = w.append(frames, boxes, GROUPS[group])
            m = G.MSD(s, group, 24, nojump=nojump)
            got = m.append(0, 24, raise_on_error=False)
            assert got.tolist() == st.tolist()
            assert got[3] == R.E_NO_POSITION and got[5] == 0 and got[9] == (R.E_NO_BOX if nojump else 0) and got[12] == (R.E_NO_BOX if nojump else R.E_NO_POSITION)
            assert m.n_frames == 24 and m.stat(G._lib.MSD_STAT_COUNTED) == sum(w.ok)
            d = m.displacements(0, 24)
            assert R.same_bits(d, w.panel()) and not d[3].any() and d[4].any()      # zero rows; the walk goes on across the gap
            check_values(G, m, w.panel(), w.ok)
            msd, pairs = m.msd()
            okv = np.array(w.ok)
            assert pairs.tolist() == [int((okv[:24 - t] & okv[t:]).sum()) for t in range(24)]
            # the first error of a mixed batch is the first failing frame's, as the other batch objects report it
            with pytest.raises(G.GroupError) as e:
                G.MSD(s, group, 24, nojump=nojump).append(0, 24)
            assert e.value.variant == "InvalidPosition" and e.value.detail == inside and e.value.status == R.E_NO_POSITION
            if nojump:
                with pytest.raises(G.SimBoxError) as e:
                    G.MSD(s, group, 24).append(9, 10)
                assert e.value.status == R.E_NO_BOX
                with pytest.raises(G.SimBoxError):
                    G.MSD(s, group, 24).append(12, 1)
            m.close()
    s.close()


def test_first_frames_failing_and_every_frame_failing(G):
    frames, boxes, inside = _failing(G)
    frames[0][inside] = np.nan; frames[1][inside + 30] = np.nan
    s = make_system(G, frames, boxes)
    w = R.Walk(len(GROUPS["two"]))
    st, bad = w.append(frames, boxes, GROUPS["two"])
    with G.MSD(s, "two", 30) as m:
        assert m.append(0, 2, raise_on_error=False).tolist() == [R.E_NO_POSITION] * 2 and m.n_frames == 2      # every frame of a call failing
        assert not m.displacements(0, 2).any() and np.isnan(m.from_origin()).all()
        msd, pairs = m.msd()
        assert pairs.tolist() == [0, 0] and np.isnan(msd).all()
        assert m.append(2, 22, raise_on_error=False).tolist() == st[2:].tolist()
        assert R.same_bits(m.displacements(0, 24), w.panel())         # the origin is the first COUNTED frame
        check_values(G, m, w.panel(), w.ok)
    s.close()


def test_errors_and_lifetime(G, worlds):
    world = worlds["ortho"]
    with pytest.raises(G.GroupError) as e:
        G.MSD(world, "nothing", 8)
    assert e.value.variant == "NotFound"
    world.group_create_from_indices("empty", [])
    with pytest.raises(G.GroupError) as e:
        G.MSD(world, "empty", 8)
    assert e.value.variant == "EmptyGroup"
    for bad in ({"dims": ""}, {"capacity": 0}, {"capacity": 2 ** 31}):                     # no component; no room; a panel beyond the cap
        kw = {"capacity": 8, "dims": "xyz"}; kw.update(bad)
        with pytest.raises(G.DeviceError) as e:
            G.MSD(world, "block", kw["capacity"], dims=kw["dims"])
        assert e.value.status == R.E_INVALID_ARG
    with pytest.raises(ValueError):
        G.MSD(world, "block", 8, dims="xw")
    m = G.MSD(world, "block", 10)
    lib = m._lib
    assert lib.gr_msd_read(m._f, None, None) == R.E_INVALID_ARG                            # read before compute
    assert lib.gr_msd_compute(m._f, 3) == R.E_INVALID_ARG                                  # nothing appended
    m.append(0, 7)
    keep = m.displacements(0, 7).tobytes(), m.from_origin().tobytes()
    with pytest.raises(G.DeviceError) as e:                                                # beyond the capacity: refused, nothing changed
        m.append(7, 4)
    assert e.value.status == R.E_INVALID_ARG and m.n_frames == 7
    assert (m.displacements(0, 7).tobytes(), m.from_origin().tobytes()) == keep
    with pytest.raises(G.DeviceError):
        m.append(NF - 1, 2)                                                                # slots out of range
    with pytest.raises(G.DeviceError):
        m.displacements(5, 3)                                                              # rows beyond the appended frames
    msd, pairs = m.msd(10 ** 6)                                                            # max_lag >= frames: clamped to frames - 1
    assert len(msd) == 7 and m.stat(G._lib.MSD_STAT_LAGS) == 7 and np.array_equal(msd, m.msd()[0]) and np.array_equal(msd[:3], m.msd(2)[0])
    m.append(7, 3)                                                                         # exactly full
    assert lib.gr_msd_read(m._f, None, None) == R.E_INVALID_ARG                            # an append behind the compute: the curve is stale
    assert m.n_frames == 10 == m.capacity and len(m.msd()[0]) == 10
    # the object keeps its snapshot: replacing the group afterwards changes nothing
    world.group_create_from_ranges("moving", [(100, 140)])
    mv = G.MSD(world, "moving", 4)
    try:
        world.group_create_from_ranges("moving", [(0, 10)])
    except G.GroanError:
        pass
    mv.append(0, 4)
    assert mv.n_atoms == 41 and np.isfinite(mv.msd()[0]).all()
    mv.close(); m.close()
    with pytest.raises(ValueError):
        m.n_frames                                                                         # closed
    # a system closes the objects that are still open before its context goes
    frames, boxes = walk("ortho")[:2]
    s = make_system(G, frames[:4], boxes[:4])
    late = G.MSD(s, "block", 4); late.append(0, 4)
    s.close()
    with pytest.raises(ValueError):
        late.append(0, 1)
    late.close()
    c, st = world.group_center_batch("all", 0, 0, 3, 1)                                    # closing the objects leaves the context usable
    assert st[0] == 0 and np.isfinite(c).all()

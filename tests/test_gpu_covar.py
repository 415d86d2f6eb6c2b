"""Covariance over resident frames (gr_covar_*; groan_rs_amd.Covariance) against the numpy restatement tests/covar_ref.py.

The RAW state: the origin bit for bit, n exactly, s and Q within the rounding bound of a sum of n exact terms taken in any order,
  |Q_dev - Q_ref| <= 2 n 2^-53 sum_f |d_i d_j|      |s_dev - s_ref| <= 2 n 2^-53 sum_f |d_i|
(every product of two widened f32 is exact in f64: device and restatement differ by the order of their additions only), and Q exactly
symmetric.  The CLOSED results equal the restatement's closing of the device's own raw state within 2 ulp and agree with an independent
two-pass f64 reference within 2^-22 sd_i sd_j (tests/test_covar_host.py says where that comes from; measured on the device at most
7.5e-8 sd_i sd_j = 0.31 of the bound, group "scattered").  Bits are compared wherever the
header promises them: across launch settings, contexts, runs, and across failed frames that leave the clean ones at their trip positions.
The system has 1000 atoms, 37 fitted frames in slots 0..36, slot 20 without a box."""
import numpy as np
import pytest

import covar_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
N, NF = 1000, 37
BOX = [40.0, 40.0, 40.0]
GROUPS = {"block": np.arange(8, 72), "masked": np.concatenate([np.arange(10, 40), np.arange(50, 90)]), "scattered": np.arange(0, N, 9), "odd": np.arange(3, 50),
          "straddle": np.arange(240, 275)}
RANGES = {"block": [(8, 71)], "masked": [(10, 39), (50, 89)], "odd": [(3, 49)], "straddle": [(240, 274)]}
REL = 2.0 ** -22
NAN_ATOM = 18                 # in block, masked, scattered and odd


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def make_groups(s):
    for name, ranges in RANGES.items():
        s.group_create_from_ranges(name, ranges)
    s.group_create_from_indices("scattered", GROUPS["scattered"])


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
def masses():
    return (1.0 + 15.0 * np.random.default_rng(4).random(N)).astype(F)


@pytest.fixture(scope="module")
def world(G, frames, masses):
    s = make_system(G, frames, n_slots=NF + 3, no_box=(20,), masses=masses)
    yield s
    s.close()


_REF = {}


def ref_state(frames, group, lo=0, hi=NF):
    """the restatement over frames[lo:hi] of the module's frames (computed once, never changed)"""
    key = (group, lo, hi)
    if key not in _REF:
        st = R.State(len(GROUPS[group]))
        st.accumulate(frames[lo:hi], GROUPS[group])
        _REF[key] = st
    return _REF[key]


def within_bounds(cv, st, extra=0.0):
    """the device's raw state against a restatement: o and n exactly, s and Q within the rounding bound (+ extra ulps of the absolute sums)"""
    o, s, Q, n = cv.raw()
    S = cv.n_atoms
    assert o.dtype == F and s.dtype == Q.dtype == np.float64 and o.shape == s.shape == (S, 3) and Q.shape == (3 * S, 3 * S)
    assert n == st.n == cv.n_frames
    assert R.same_bits(o.reshape(-1), st.o)
    dq, ds = np.abs(Q - st.Q), np.abs(s.reshape(-1) - st.s)
    assert (dq <= st.q_bound() + extra * R.U * st.abs_Q).all(), float((dq - st.q_bound()).max())
    assert (ds <= st.s_bound() + extra * R.U * st.abs_s).all(), float((ds - st.s_bound()).max())
    assert np.array_equal(Q, Q.T)


def raw_bits(cv):
    o, s, Q, n = cv.raw()
    return o.tobytes(), s.tobytes(), Q.tobytes(), n


def ulps(a, b):
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("nf", [1, 2, NF])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_raw_state_against_the_restatement(G, world, frames, group, nf):
    with G.Covariance(world, group) as cv:
        assert cv.n_atoms == len(GROUPS[group]) and cv.n_frames == 0
        status = cv.accumulate(0, nf)
        assert status.dtype == np.int32 and not status.any()                     # slot 20 has no box: counted all the same
        within_bounds(cv, ref_state(frames, group, 0, nf))
        assert cv.stat(G._lib.CV_STAT_LAUNCHES) == 1
        B = cv.stat(G._lib.CV_STAT_BLOCK_EDGE)
        nb = (3 * cv.n_atoms + 1 + B - 1) // B
        assert cv.stat(G._lib.CV_STAT_BLOCKS) == nb * (nb + 1) // 2 == cv.stat(G._lib.CV_STAT_LAST_PRODUCT_GROUPS)
        if nf == 1:                                                               # one frame: d = 0 everywhere
            o, s, Q, n = cv.raw()
            assert not s.any() and not Q.any() and R.same_bits(o, frames[0][GROUPS[group]])


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_closed_results(G, world, frames, masses, group):
    idx = GROUPS[group]
    with G.Covariance(world, group) as cv:
        assert np.isnan(cv.mean()).all() and np.isnan(cv.matrix()).all() and np.isnan(cv.dccm()).all()      # before the first counted frame
        cv.accumulate(0, NF)
        o, s, Q, n = cv.raw()
        mean, cov, covw, corr = cv.mean(), cv.matrix(), cv.matrix(mass_weighted=True), cv.dccm()
    assert mean.dtype == cov.dtype == corr.dtype == np.float64 and mean.shape == (len(idx), 3) and cov.shape == (3 * len(idx),) * 2 and corr.shape == (len(idx),) * 2
    # the library's closing step is the restatement's, applied to the device's own raw state
    cm, cc = R.close(o, s, Q, n)
    assert ulps(mean, cm).max() <= 2 and ulps(cov, cc).max() <= 2
    rm = np.sqrt(np.repeat(masses[idx].astype(np.float64), 3))
    assert ulps(covw, cov * np.outer(rm, rm)).max() <= 2
    # ... and the independent reference
    m2, c2, sd = R.two_pass(frames, idx)
    worst = (np.abs(cov - c2) / np.outer(sd, sd)).max()
    print("device vs two-pass: %.3g of sd_i sd_j (bound %.3g)" % (worst, REL))
    assert worst <= REL and np.abs(mean - m2).max() <= 1e-6
    assert np.array_equal(cov, cov.T) and 0.01 < np.sqrt(np.diagonal(cov)).mean() < 0.8        # (the frames do move)
    # the DCCM
    st = ref_state(frames, group)
    rc = R.dccm(R.close(st.o, st.s, st.Q, st.n)[1])
    assert np.abs(corr - rc).max() <= 1e-12
    assert np.abs(np.diagonal(corr) - 1.0).max() <= 1e-12 and np.array_equal(corr, corr.T) and np.abs(corr).max() <= 1.0 + 1e-12


@pytest.mark.parametrize("group", ["block", "masked", "scattered"])
def test_the_diagonal_is_fluctuations_variance(G, world, frames, group):
    with G.Covariance(world, group) as cv, G.Fluctuations(world, group) as fl:
        cv.accumulate(0, NF); fl.accumulate(0, NF)
        st = ref_state(frames, group)
        diff = np.abs(np.diagonal(cv.matrix()) - fl.variance().reshape(-1))
        assert (diff <= np.diagonal(st.q_bound()) / NF).all()
        assert np.abs(cv.mean() - fl.mean()).max() <= 1e-12


def test_dccm_of_an_atom_that_does_not_move(G, frames):
    fr = [x.copy() for x in frames[:12]]
    for x in fr:
        x[30] = fr[0][30]
    s = make_system(G, fr)
    with G.Covariance(s, "block") as cv:
        cv.accumulate(0, 12)
        corr = cv.dccm()
    k = 30 - 8
    moving = np.delete(np.arange(64), k)
    assert corr[k, k] == 1.0 and np.isnan(corr[k, moving]).all() and np.isnan(corr[moving, k]).all() and np.isfinite(corr[np.ix_(moving, moving)]).all()
    st = R.State(64); st.accumulate(fr, GROUPS["block"])
    rc = R.dccm(R.close(st.o, st.s, st.Q, st.n)[1])
    assert np.abs(corr - rc)[np.ix_(moving, moving)].max() <= 1e-12
    s.close()


def test_frames_jumping_across_the_box(G):
    fr = R.jumping_frames(N, 24, 77)
    s = make_system(G, fr)
    for group in ("block", "scattered", "masked"):
        with G.Covariance(s, group) as cv, G.Covariance(s, group) as two:
            cv.accumulate(0, 24)
            st = R.State(len(GROUPS[group])); st.accumulate(fr, GROUPS[group])
            within_bounds(cv, st)
            m2, c2, sd = R.two_pass(fr, GROUPS[group])
            assert (np.abs(cv.matrix() - c2) / np.outer(sd, sd)).max() <= REL
            # d with all 24 bits: here the sums do round, and two calls cut inside a trip differ from one -- within the bound
            two.accumulate(0, 7); two.accumulate(7, 17)
            within_bounds(two, st)
            diff = np.abs(two.raw()[2] - cv.raw()[2])
            print("one call vs two calls, %s: %d of %d entries differ, worst %.3g of the bound" % (group, (diff > 0).sum(), diff.size, (diff / st.q_bound().clip(1e-300)).max()))
            assert (diff <= st.q_bound()).all()
    s.close()


@pytest.mark.parametrize("where", [0, 3, 7])
def test_one_failing_frame(G, frames, where):
    """first (the origin then comes from the second frame), in the middle, last: statuses, the index, n; the clean frames have moved inside
    their trip, so the state is that of the clean frames alone within the bound (last: bit for bit, nothing has moved)"""
    fr = [x.copy() for x in frames[:8]]
    fr[where][NAN_ATOM] = np.nan
    clean = [x for k, x in enumerate(fr) if k != where]
    s, t = make_system(G, fr), make_system(G, clean)
    for group in ("block", "scattered", "masked", "straddle"):
        hit = NAN_ATOM in GROUPS[group]
        st = R.State(len(GROUPS[group]))
        status, bad = st.accumulate(fr, GROUPS[group])
        cv = G.Covariance(s, group)
        got = cv.accumulate(0, 8, raise_on_error=False)
        assert got.tolist() == status.tolist() and (got[where] == R.E_NO_POSITION) == hit
        assert cv.n_frames == (7 if hit else 8)
        within_bounds(cv, st)
        if hit:
            first = 1 if where == 0 else 0
            assert R.same_bits(cv.raw()[0], fr[first][GROUPS[group]])            # the origin: the first COUNTED frame
            keep = raw_bits(cv)
            with pytest.raises(G.GroupError) as e:
                cv.accumulate(where, 1)
            assert e.value.variant == "InvalidPosition" and e.value.detail == NAN_ATOM and e.value.status == R.E_NO_POSITION
            assert raw_bits(cv) == keep                                           # the failed frame added nothing
            with pytest.raises(G.GroupError) as e:                                # first error of a batch: the first failing frame's
                cv.accumulate(0, 8)
            assert e.value.detail == NAN_ATOM
            if where == 7:
                with G.Covariance(t, group) as alone:
                    alone.accumulate(0, 7)
                    assert raw_bits(alone) == keep
        cv.close()
    s.close(); t.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_failing_trip_leaves_the_bits_of_the_clean_frames(G, world, frames, where):
    """a whole trip of failing frames: the clean frames keep their places inside their trips, the zero columns are neutral, and the state
    is that of the clean frames alone BIT FOR BIT"""
    with G.Covariance(world, "block") as probe:
        T = probe.stat(G._lib.CV_STAT_TRIP_FRAMES)
    assert 2 * T + 5 <= NF
    lo = {"first": 0, "middle": T, "last": T}[where]
    n_all = 2 * T + 5 if where != "last" else 2 * T
    fr = [x.copy() for x in frames[:n_all]]
    for k in range(lo, lo + T):
        fr[k][[NAN_ATOM + 9 * (k % 3), 63]] = np.nan                              # (18, 27, 36 and 63 are atoms of all three groups)
    clean = [x for k, x in enumerate(fr) if not lo <= k < lo + T]
    s, t = make_system(G, fr), make_system(G, clean)
    for group in ("block", "scattered", "masked"):
        with G.Covariance(s, group) as cv, G.Covariance(t, group) as alone:
            got = cv.accumulate(0, n_all, raise_on_error=False)
            assert got.tolist() == [R.E_NO_POSITION if lo <= k < lo + T else 0 for k in range(n_all)]
            assert s._lib.gr_last_error_index(s._ctx) == NAN_ATOM + 9 * (lo % 3)     # the lowest atom of the first failing frame
            assert not alone.accumulate(0, n_all - T).any()
            assert cv.n_frames == alone.n_frames == n_all - T and raw_bits(cv) == raw_bits(alone)
            st = R.State(len(GROUPS[group])); st.accumulate(fr, GROUPS[group])
            within_bounds(cv, st)
            assert R.same_bits(cv.raw()[0], clean[0][GROUPS[group]])
    s.close(); t.close()


def test_every_frame_failing(G, frames):
    fr = [x.copy() for x in frames[:4]]
    for k, x in enumerate(fr):
        x[[NAN_ATOM + 9 * k, 300]] = np.nan
    s = make_system(G, fr + [frames[5], frames[6]])
    with G.Covariance(s, "scattered") as cv:
        got = cv.accumulate(0, 4, raise_on_error=False)
        assert got.tolist() == [R.E_NO_POSITION] * 4 and cv.n_frames == 0
        assert all(np.isnan(x).all() for x in (cv.mean(), cv.matrix(), cv.dccm()))
        o, sm, Q, n = cv.raw()
        assert n == 0 and not o.any() and not sm.any() and not Q.any()
        with pytest.raises(G.GroupError) as e:
            cv.accumulate(1, 3)
        assert e.value.detail == NAN_ATOM + 9                                     # the lowest atom of the first failing frame
        cv.accumulate(4, 2)
        keep = raw_bits(cv)
        assert cv.accumulate(0, 4, raise_on_error=False).tolist() == [R.E_NO_POSITION] * 4
        assert raw_bits(cv) == keep and cv.n_frames == 2                          # all frames failing: the state is unchanged
    s.close()


@pytest.fixture(scope="module")
def world6(G, frames):
    s = make_system(G, frames[:6])
    yield s
    s.close()


def test_nan_outside_the_group_changes_nothing(G, frames, world6):
    """atoms without position next to the group: the same bits as the same frames without the holes"""
    outside = {"block": [4, 5, 6, 7, 72, 73], "odd": [0, 1, 2, 50, 51], "straddle": [239, 238, 275, 276, 255 - 16], "masked": [9, 8, 40, 41, 49, 90], "scattered": [1, 2, 8, 10, 998, 257]}
    for group, out in outside.items():
        idx = GROUPS[group]
        assert not set(out) & set(idx.tolist())
        fr = [x.copy() for x in frames[:6]]
        for k, x in enumerate(fr):
            x[out[k % 2::2]] = np.nan                                             # some of them in every frame
        s = make_system(G, fr)
        with G.Covariance(s, group) as cv:
            assert not cv.accumulate(0, 6).any()
            with G.Covariance(world6, group) as same:
                same.accumulate(0, 6)
                assert raw_bits(cv) == raw_bits(same)
            assert np.isfinite(cv.matrix()).all() and np.isfinite(cv.mean()).all()
        s.close()


def test_a_frame_without_a_box_is_counted(G, world):
    assert not world.has_box(20)
    with G.Covariance(world, "odd") as cv:
        assert cv.accumulate(20, 1).tolist() == [0] and cv.n_frames == 1


def _calls(cv):
    cv.accumulate(0, 5); cv.accumulate(5, 32)
    return raw_bits(cv) + (cv.matrix().tobytes(), cv.dccm().tobytes())


def test_determinism_across_launch_settings_contexts_and_runs(G, world, frames, masses):
    """the same calls give the same bits: a product grid of 1 (one workgroup strides over every block), small odd grids, an over-large
    grid, the default; in a context that has run other families of calls and failed calls before; and in a second run"""
    used = make_system(G, frames, n_slots=NF + 12, masses=masses)
    for k in range(10):
        used.copy_frame(NF + k, k)
    used.group_center_batch("scattered", G._lib.CENTER_PBC, 1, 0, 10, raise_on_error=False)
    plan = G.RMSDPlan(used, used, "block", ref_slot=NF)
    plan.rmsd_fit(NF + 1, 9, raise_on_error=False)
    with G.Fluctuations(used, "masked") as fl:
        fl.accumulate(0, 10)
    with G.Covariance(used, "odd") as other:
        other.accumulate(3, 9)
        with pytest.raises(G.DeviceError):
            other.accumulate(NF + 10, 5)                                          # slots out of range: a hard error
    for group in ("block", "scattered", "masked"):
        want = None
        for system, launch in ((world, (0, 0)), (world, (1, 1)), (world, (3, 2)), (world, (100000, 0)), (used, (0, 0)), (used, (2, 1)), (world, (0, 0))):
            with G.Covariance(system, group) as cv:
                cv.set_launch(*launch)
                got = _calls(cv)
                if launch[0]:
                    assert cv.stat(G._lib.CV_STAT_LAST_PRODUCT_GROUPS) == min(launch[0], cv.stat(G._lib.CV_STAT_BLOCKS))
                if launch[1]:
                    assert cv.stat(G._lib.CV_STAT_LAST_CHECK_GROUPS) <= launch[1]
                assert cv.stat(G._lib.CV_STAT_LAUNCHES) == 2
            want = want or got
            assert got == want, (group, launch)
    used.close()


def test_one_call_equals_two_calls_within_the_bound(G, world, frames):
    for group in ("block", "scattered", "straddle"):
        st = ref_state(frames, group)
        with G.Covariance(world, group) as a, G.Covariance(world, group) as b, G.Covariance(world, group) as c:
            a.accumulate(0, NF); b.accumulate(0, 5); b.accumulate(5, 32)
            for k in range(NF):
                c.accumulate(k, 1)
            qa, qb, qc = a.raw()[2], b.raw()[2], c.raw()[2]
            for cv in (a, b, c):
                within_bounds(cv, st)
            assert (np.abs(qa - qb) <= st.q_bound()).all() and (np.abs(qa - qc) <= st.q_bound()).all()
            assert a.stat(G._lib.CV_STAT_LAUNCHES) == 1 and b.stat(G._lib.CV_STAT_LAUNCHES) == 2 and c.stat(G._lib.CV_STAT_LAUNCHES) == NF


def test_a_long_run_cut_by_the_segment_loop_and_by_the_caller(G):
    """1030 frames of a 40-atom system: one call (the segment loop cuts it at 1024) and two calls of 515"""
    na, ns = 40, 1030
    fr = R.fitted_frames(na, ns, 5)
    s = make_system(G, fr)
    s.group_create_from_ranges("all", [(0, na - 1)])
    st = R.State(na); st.accumulate(fr, np.arange(na))
    with G.Covariance(s, "all") as a, G.Covariance(s, "all") as b:
        assert not a.accumulate(0, ns).any()
        b.accumulate(0, 515); b.accumulate(515, 515)
        assert a.stat(G._lib.CV_STAT_LAUNCHES) == 2 == b.stat(G._lib.CV_STAT_LAUNCHES)
        within_bounds(a, st); within_bounds(b, st)
        assert (np.abs(a.raw()[2] - b.raw()[2]) <= st.q_bound()).all()
        m2, c2, sd = R.two_pass(fr, np.arange(na))
        assert (np.abs(a.matrix() - c2) / np.outer(sd, sd)).max() <= REL
    s.close()


def test_merge(G, world, frames):
    """two halves against one walk, across two contexts.  The host's merge adds five terms per entry: a few ulps of the absolute sums on
    top of the halves' own bounds (8 is generous by a factor two)"""
    cut = 20
    w2 = make_system(G, frames[cut:])
    small = G.System(N, n_slots=1)
    small.group_create_from_ranges("block", [(8, 70)])
    for group in ("block", "scattered", "masked"):
        a, b, empty, same_ctx = G.Covariance(world, group), G.Covariance(w2, group), G.Covariance(w2, group), G.Covariance(world, group)
        a.accumulate(0, cut); b.accumulate(0, NF - cut); same_ctx.accumulate(cut, NF - cut)
        keep_a, keep_b = raw_bits(a), raw_bits(b)
        assert raw_bits(same_ctx) == keep_b
        a.merge(empty)                                                            # an empty src changes nothing
        assert raw_bits(a) == keep_a
        empty.merge(b)                                                            # an empty dst takes src's origin and sums unchanged
        assert raw_bits(empty) == keep_b and raw_bits(b) == keep_b and empty.n_frames == NF - cut
        a.merge(b)
        assert a.n_frames == NF and raw_bits(b) == keep_b
        ra, rb = R.State(len(GROUPS[group])), R.State(len(GROUPS[group]))
        ra.accumulate(frames[:cut], GROUPS[group]); rb.accumulate(frames[cut:], GROUPS[group])
        ra.merge(rb)
        within_bounds(a, ra, extra=8.0)
        m2, c2, sd = R.two_pass(frames, GROUPS[group])
        assert (np.abs(a.matrix() - c2) / np.outer(sd, sd)).max() <= REL and np.abs(a.mean() - m2).max() <= 1e-6
        a.accumulate(0, 3)                                                        # a merged object goes on counting
        assert a.n_frames == NF + 3 and np.array_equal(a.raw()[2], a.raw()[2].T)
        for cv in (a, b, empty, same_ctx):
            cv.close()
    a, c = G.Covariance(world, "block"), G.Covariance(small, "block")
    with pytest.raises(G.GroupError) as e:
        a.merge(c)
    assert e.value.variant == "InconsistentGroup" and e.value.detail[1:] == (64, 63) and e.value.status == R.E_INCONSISTENT_GROUP
    with pytest.raises(G.DeviceError) as e:
        a.merge(a)
    assert e.value.status == R.E_INVALID_ARG
    a.close(); c.close(); small.close(); w2.close()


def test_clear(G, world, frames):
    for group in ("block", "scattered"):
        with G.Covariance(world, group) as a, G.Covariance(world, group) as b:
            a.accumulate(7, 11)
            a.clear()
            assert a.n_frames == 0 and np.isnan(a.mean()).all() and not a.raw()[2].any()
            a.accumulate(2, 9); b.accumulate(2, 9)
            assert raw_bits(a) == raw_bits(b)
            within_bounds(a, ref_state(frames, group, 2, 11))


def test_errors_and_lifetime(G, world):
    with pytest.raises(G.GroupError) as e:
        G.Covariance(world, "nothing")
    assert e.value.variant == "NotFound"
    world.group_create_from_indices("empty", [])
    with pytest.raises(G.GroupError) as e:
        G.Covariance(world, "empty")
    assert e.value.variant == "EmptyGroup"
    cv = G.Covariance(world, "block")
    with pytest.raises(G.DeviceError):
        cv.accumulate(NF + 2, 5)                                                  # slots out of range: a hard error
    assert cv.n_frames == 0
    with pytest.raises(ValueError):
        cv.stat(99)
    cv.close()
    # a group above the cap: the message names it
    cap = G._lib.CV_MAX_ATOMS
    big = G.System(cap + 1, n_slots=1)
    big.group_create_from_ranges("all", [(0, cap)])
    big.group_create_from_ranges("most", [(0, cap - 1)])
    with pytest.raises(G.DeviceError) as e:
        G.Covariance(big, "all")
    assert e.value.status == R.E_INVALID_ARG and str(cap) in e.value.detail and "GR_CV_MAX_ATOMS" in e.value.detail
    with G.Covariance(big, "most") as most:                                       # the cap itself is allowed
        assert most.n_atoms == cap
    big.close()
    # the object keeps its snapshot: replacing the group afterwards changes nothing
    world.group_create_from_ranges("moving", [(100, 140)])
    mv = G.Covariance(world, "moving")
    try:
        world.group_create_from_ranges("moving", [(0, 10)])
    except G.GroanError:
        pass                                                                      # (the library reports that the group existed)
    mv.accumulate(0, 3)
    assert mv.n_atoms == 41 and np.isfinite(mv.matrix()).all()
    mv.close()
    c, st = world.group_center_batch("block", 0, 0, 3, 1)                         # closing the objects leaves the context usable
    assert st[0] == 0 and np.isfinite(c).all()
    # use after System.close(): the system closes the object, which then refuses every call
    s = G.System(16, n_slots=1)
    s.set_frame(np.zeros((16, 3), F), BOX, slot=0)
    s.group_create_from_ranges("g", [(0, 15)])
    late = G.Covariance(s, "g")
    late.accumulate(0, 1)
    s.close()
    for call in (lambda: late.accumulate(0, 1), lambda: late.matrix(), lambda: late.raw(), lambda: late.n_frames, lambda: late.clear()):
        with pytest.raises(ValueError):
            call()
    late.close()

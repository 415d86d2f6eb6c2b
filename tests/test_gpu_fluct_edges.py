"""Fluctuations at the edges of its kernels (gr_fluct.h): the look-ahead of the frame walk (GR_FL_AHEAD frames in flight, read from the
source), the ranges a launch cuts the group into (gr_fluct_set_launch), groups that end on the last atom of the partial 256-atom tile or
begin next to a tile boundary, and the 1024-frame segment of a batched call.  Everything is compared bit for bit with the numpy
restatement tests/fluct_ref.py."""
import numpy as np
import pytest

import fluct_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
N = 1000
BOX = [40.0, 40.0, 40.0]
A = R.source_ahead()
NFR = max(2 * A + 1, A + 4)          # frames of the system
NAN_ATOM = 6
GROUPS = {"block": np.arange(3, 771), "third": np.arange(0, N, 3), "two": np.concatenate([np.arange(4, 301), np.arange(500, 901)]), "all": np.arange(N),
          "tail": np.arange(990, N), "long_tail": np.arange(3, N), "from255": np.arange(255, 301), "from256": np.arange(256, 301),
          "corners": np.array([1, 255, 256, 511, 512, 999])}
RANGES = {"block": [(3, 770)], "two": [(4, 300), (500, 900)], "tail": [(990, N - 1)], "long_tail": [(3, N - 1)], "from255": [(255, 300)], "from256": [(256, 300)]}
FORM = {"block": 0, "third": 1, "two": 2, "all": 0, "tail": 0, "long_tail": 0, "from255": 0, "from256": 0, "corners": 1}


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def make_system(G, frames):
    s = G.System(len(frames[0]), n_slots=len(frames))
    for k, x in enumerate(frames):
        s.set_frame(x, BOX, slot=k)
    if len(frames[0]) == N:
        for name, ranges in RANGES.items():
            s.group_create_from_ranges(name, ranges)
        s.group_create_from_indices("third", GROUPS["third"])
        s.group_create_from_indices("corners", GROUPS["corners"])
    return s


@pytest.fixture(scope="module")
def frames():
    return R.fitted_frames(N, NFR, 4242)


@pytest.fixture(scope="module")
def clean(G, frames):
    s = make_system(G, frames)
    yield s
    s.close()


@pytest.fixture(scope="module")
def holes(G, frames):
    """atom 6 has no position in frames 0, GR_FL_AHEAD - 1 and GR_FL_AHEAD"""
    fr = [x.copy() for x in frames]
    for k in (0, A - 1, A):
        fr[k][NAN_ATOM] = np.nan
    s = make_system(G, fr)
    yield s, fr
    s.close()


def same_raw(fl, st):
    o, s, q, n = fl.raw()
    assert n == st.n == fl.n_frames
    assert R.same_bits(o, st.o) and R.same_bits(s, st.s) and R.same_bits(q, st.q)


def raw_bits(fl):
    o, s, q, n = fl.raw()
    return o.tobytes(), s.tobytes(), q.tobytes(), n


def ref_state(frames, idx):
    st = R.State(len(idx))
    status, bad = st.accumulate(frames, idx)
    return st, status


@pytest.mark.parametrize("nf", [A - 1, A, A + 1, 2 * A + 1])
@pytest.mark.parametrize("group", ["block", "third", "two"])
def test_look_ahead(G, clean, holes, frames, group, nf):
    assert NAN_ATOM in GROUPS[group]
    with G.Fluctuations(clean, group) as fl:
        assert fl.stat(G._lib.FL_STAT_FORM) == FORM[group] and fl.stat(G._lib.FL_STAT_AHEAD) == A
        assert not fl.accumulate(0, nf).any()
        same_raw(fl, ref_state(frames[:nf], GROUPS[group])[0])
    s, fr = holes
    st, status = ref_state(fr[:nf], GROUPS[group])
    failing = [k for k in (0, A - 1, A) if k < nf]
    assert [k for k in range(nf) if status[k]] == failing
    with G.Fluctuations(s, group) as fl:
        got = fl.accumulate(0, nf, raise_on_error=False)
        assert got.tolist() == status.tolist() and fl.n_frames == nf - len(failing)
        same_raw(fl, st)
        assert R.same_bits(fl.raw()[0], fr[1][GROUPS[group]])                     # frame 0 failed: the origin is frame 1's
        with pytest.raises(G.GroupError) as e:
            fl.accumulate(0, nf)
        assert e.value.variant == "InvalidPosition" and e.value.detail == NAN_ATOM
    # a walk that starts on the failing frames, and one that ends on them
    for first, n in ((A - 1, 3), (1, A)):
        if first + n > NFR:
            continue
        st, status = ref_state(fr[first:first + n], GROUPS[group])
        with G.Fluctuations(s, group) as fl:
            assert fl.accumulate(first, n, raise_on_error=False).tolist() == status.tolist()
            same_raw(fl, st)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_range_edges(G, clean, frames, group):
    idx = GROUPS[group]
    nf = A + 2
    st, _ = ref_state(frames[:nf], idx)
    units = len(idx) if FORM[group] == 1 else ((idx[-1] >> 2) - (idx[0] >> 2) + 1)
    partial = max(2, (units + 2) // 3 - 1) if units > 3 else 2                    # ranges whose last one is cut short (or empty)
    for range_groups, check_groups in ((0, 0), (1, 0), (partial, 0), (units, 0), (units + 77, 0), (0, 1), (1, 1)):
        with G.Fluctuations(clean, group) as fl:
            assert fl.stat(G._lib.FL_STAT_FORM) == FORM[group]
            fl.set_launch(range_groups, check_groups)
            assert not fl.accumulate(0, nf).any()
            same_raw(fl, st)
            want = range_groups if range_groups else (units + 63) // 64
            assert fl.stat(G._lib.FL_STAT_LAST_RANGE_GROUPS) == want
            if check_groups:
                assert fl.stat(G._lib.FL_STAT_LAST_CHECK_GROUPS) == check_groups
            fl.set_launch(0, 0)                                                   # 0 restores the default; a second call goes on from the first
            assert not fl.accumulate(nf, 2).any()
            same_raw(fl, ref_state(frames[:nf + 2], idx)[0])


@pytest.mark.parametrize("group", ["tail", "long_tail", "from255", "from256", "corners", "all"])
def test_group_edges(G, clean, holes, frames, group):
    """groups that end on the last atom of the partial tile (the pads behind it never enter a sum, nor does a neighbour in the last
    4-atom group) or begin on either side of a tile boundary; with atom 6 -- outside most of them -- missing in some frames"""
    idx = GROUPS[group]
    nf = NFR
    with G.Fluctuations(clean, group) as fl:
        fl.accumulate(0, nf)
        same_raw(fl, ref_state(frames, idx)[0])
        m2, v2, r2 = R.two_pass(frames, idx)
        assert np.abs(fl.mean() - m2).max() <= 1e-5 and np.abs(fl.rmsf() - r2).max() <= 1e-5
    s, fr = holes
    st, status = ref_state(fr, idx)
    with G.Fluctuations(s, group) as fl:
        assert fl.accumulate(0, nf, raise_on_error=False).tolist() == status.tolist()
        assert bool(status.any()) == (NAN_ATOM in idx)
        same_raw(fl, st)


# ---------------------------------------------------------------------------------------------- the 1024-frame segment
NA, NS, CUT = 300, 1030, 1024
SEG_GROUPS = {"all": np.arange(NA), "fifth": np.arange(2, NA, 5)}


@pytest.fixture(scope="module")
def long_run(G):
    fr = R.fitted_frames(NA, NS, 1030, extent=10.0)
    s = make_system(G, fr)
    s.group_create_from_indices("fifth", SEG_GROUPS["fifth"])
    yield s, fr
    s.close()


@pytest.mark.parametrize("group", sorted(SEG_GROUPS))
def test_one_call_equals_two_calls_across_the_segment(G, long_run, group):
    s, fr = long_run
    idx = SEG_GROUPS[group]
    with G.Fluctuations(s, group) as one, G.Fluctuations(s, group) as two:
        assert not one.accumulate(0, NS).any()
        assert not two.accumulate(0, CUT).any() and not two.accumulate(CUT, NS - CUT).any()
        assert raw_bits(one) == raw_bits(two) and one.stat(G._lib.FL_STAT_LAUNCHES) == 2 == two.stat(G._lib.FL_STAT_LAUNCHES)
        same_raw(one, ref_state(fr, idx)[0])
        assert one.mean().tobytes() == two.mean().tobytes() and one.rmsf().tobytes() == two.rmsf().tobytes()


def test_failing_frames_on_both_sides_of_the_segment(G, long_run):
    s, fr = long_run
    early, late = 1000, 1026
    bad = {early: 17, late: 7}                                                   # both atoms are in "fifth" (2, 7, 12, 17, ...) and in "all"
    fr2 = list(fr)
    try:
        for k, atom in bad.items():
            fr2[k] = fr[k].copy(); fr2[k][atom] = np.nan
            s.set_frame(fr2[k], BOX, slot=k)
        for group, idx in SEG_GROUPS.items():
            st, status = ref_state(fr2, idx)
            assert [k for k in range(NS) if status[k]] == [early, late]
            with G.Fluctuations(s, group) as one, G.Fluctuations(s, group) as two:
                got = one.accumulate(0, NS, raise_on_error=False)
                g2 = np.concatenate([two.accumulate(0, CUT, raise_on_error=False), two.accumulate(CUT, NS - CUT, raise_on_error=False)])
                assert got.tolist() == g2.tolist() == status.tolist()
                assert raw_bits(one) == raw_bits(two) and one.n_frames == NS - 2
                same_raw(one, st)
                with pytest.raises(G.GroupError) as e:                            # the first error is the earlier frame's
                    one.accumulate(0, NS)
                assert e.value.variant == "InvalidPosition" and e.value.detail == bad[early]
                with pytest.raises(G.GroupError) as e:
                    one.accumulate(CUT, NS - CUT)
                assert e.value.detail == bad[late]
    finally:
        for k in bad:
            s.set_frame(fr[k], BOX, slot=k)

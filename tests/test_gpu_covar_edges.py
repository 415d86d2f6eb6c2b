"""Covariance (gr_covar_*) at the edges of its kernels' geometry, read from gr_covar_stat: B, the edge of a block of Q in dimensions, and
T, the frames per trip of the product.  The product has R = 3 S + 1 rows (the dimensions and the ones row): group sizes put R one below,
at and one above a multiple of 16 (a tile of the matrix instruction) and of B; S = 1; an S with at least three block rows, so that blocks
exist that do not touch the diagonal.  Frame counts T - 1, T, T + 1, 2 T + 1; a failing frame at each side of a trip boundary and of
the 1024-frame segment of a batched call.  Every case is compared with the numpy restatement tests/covar_ref.py under the rounding
bound of tests/test_gpu_covar.py, and with itself bit for bit under two launch settings."""
import numpy as np
import pytest

import covar_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
NA, A0 = 300, 2               # atoms of the system; the groups start at atom 2 (not a multiple of 4)
BOX = [40.0, 40.0, 40.0]


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.fixture(scope="module")
def geometry(G):
    s = G.System(8, n_slots=1)
    s.group_create_from_ranges("g", [(0, 7)])
    with G.Covariance(s, "g") as cv:
        B, T = cv.stat(G._lib.CV_STAT_BLOCK_EDGE), cv.stat(G._lib.CV_STAT_TRIP_FRAMES)
    s.close()
    assert B % 16 == 0 and B >= 16 and T % 4 == 0 and 4 <= T <= 64              # tiles of 16, four frames per matrix instruction
    return B, T


def sizes(B):
    """S -> why: R = 3 S + 1 one below / at / one above the first multiple of 16 and of B that 3 S can reach, S = 1, three block rows"""
    out = {1: "one atom"}
    for mult in (16, B):
        for delta in (-1, 0, 1):
            S = next(S for S in range(1, 4 * mult) if (3 * S + 1 - delta) % mult == 0 and 3 * S + 1 - delta > 0)
            out.setdefault(S, "R = %d k %+d" % (mult, delta))
    S3 = (2 * B) // 3 + 1                                                         # R = 3 S + 1 > 2 B
    out.setdefault(S3, "three block rows")
    return out


@pytest.fixture(scope="module")
def world(G, geometry):
    B, T = geometry
    nf = 2 * T + 1
    fr = R.fitted_frames(NA, nf, 20261021)
    s = G.System(NA, n_slots=nf)
    for k, x in enumerate(fr):
        s.set_frame(x, BOX, slot=k)
    for S in sizes(B):
        assert A0 + S <= NA
        s.group_create_from_ranges("s%d" % S, [(A0, A0 + S - 1)])
    yield s, fr
    s.close()


def within_bounds(cv, st):
    o, s, Q, n = cv.raw()
    assert n == st.n == cv.n_frames and R.same_bits(o.reshape(-1), st.o)
    assert (np.abs(Q - st.Q) <= st.q_bound()).all() and (np.abs(s.reshape(-1) - st.s) <= st.s_bound()).all()
    assert np.array_equal(Q, Q.T)
    return o.tobytes(), s.tobytes(), Q.tobytes(), n


def test_the_sizes_cover_the_edges(geometry):
    B, T = geometry
    got = sizes(B)
    rows = sorted(3 * S + 1 for S in got)
    for mult in (16, B):
        assert {r % mult for r in rows} >= {mult - 1, 0, 1}
    assert 1 in got and max(rows) > 2 * B and len(got) <= 8                       # (8: the cases of the test below)


# (the case list is built from the constants the library reports: B = 64 and T = 16 give S in 1, 5, 10, 16, 21, 42, 43, 64)
@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("nfk", ["T-1", "T", "T+1", "2T+1"])
def test_group_sizes_and_frame_counts(G, geometry, world, which, nfk):
    B, T = geometry
    s, fr = world
    all_sizes = sorted(sizes(B))
    if which >= len(all_sizes):
        return                                                                    # (fewer distinct sizes for this B)
    S = all_sizes[which]
    nf = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1}[nfk]
    idx = np.arange(A0, A0 + S)
    st = R.State(S); st.accumulate(fr[:nf], idx)
    nb = (3 * S + 1 + B - 1) // B
    bits = []
    for launch in ((0, 0), (2, 1)):
        with G.Covariance(s, "s%d" % S) as cv:
            cv.set_launch(*launch)
            assert not cv.accumulate(0, nf).any()
            bits.append(within_bounds(cv, st))
            assert cv.stat(G._lib.CV_STAT_BLOCKS) == nb * (nb + 1) // 2
            assert cv.stat(G._lib.CV_STAT_LAST_PRODUCT_GROUPS) == (min(2, nb * (nb + 1) // 2) if launch[0] else nb * (nb + 1) // 2)
    assert bits[0] == bits[1]


@pytest.mark.parametrize("side", [-1, 0])
def test_a_failing_frame_at_a_trip_boundary(G, geometry, side):
    B, T = geometry
    nf, S = 2 * T + 1, (2 * B) // 3 + 1
    fr = R.fitted_frames(NA, nf, 77)
    bad = T + side                                                                # the last frame of the first trip, the first of the second
    fr[bad][A0 + 3] = np.nan
    s = G.System(NA, n_slots=nf)
    for k, x in enumerate(fr):
        s.set_frame(x, BOX, slot=k)
    s.group_create_from_ranges("g", [(A0, A0 + S - 1)])
    st = R.State(S)
    status, _ = st.accumulate(fr, np.arange(A0, A0 + S))
    bits = []
    for launch in ((0, 0), (1, 1)):
        with G.Covariance(s, "g") as cv:
            cv.set_launch(*launch)
            got = cv.accumulate(0, nf, raise_on_error=False)
            assert got.tolist() == status.tolist() and got[bad] == R.E_NO_POSITION and got.sum() == R.E_NO_POSITION
            assert s._lib.gr_last_error_index(s._ctx) == A0 + 3
            bits.append(within_bounds(cv, st))
    assert bits[0] == bits[1]
    s.close()


@pytest.fixture(scope="module")
def long_run(G):
    na, ns = 40, 1030
    fr = R.fitted_frames(na, ns, 1030, extent=10.0)
    return na, ns, fr


@pytest.mark.parametrize("bad", [1023, 1024])
def test_a_failing_frame_at_the_segment_boundary(G, long_run, bad):
    na, ns, fr = long_run
    fr = list(fr)
    fr[bad] = fr[bad].copy(); fr[bad][7] = np.nan
    s = G.System(na, n_slots=ns)
    for k, x in enumerate(fr):
        s.set_frame(x, BOX, slot=k)
    s.group_create_from_ranges("g", [(1, na - 2)])
    idx = np.arange(1, na - 1)
    st = R.State(len(idx))
    status, _ = st.accumulate(fr, idx)
    bits = []
    for launch in ((0, 0), (3, 1)):
        with G.Covariance(s, "g") as cv:
            cv.set_launch(*launch)
            got = cv.accumulate(0, ns, raise_on_error=False)
            assert got.tolist() == status.tolist() and got[bad] == R.E_NO_POSITION and cv.n_frames == ns - 1
            assert cv.stat(G._lib.CV_STAT_LAUNCHES) == 2                         # the segment loop cuts at 1024
            bits.append(within_bounds(cv, st))
    assert bits[0] == bits[1]
    s.close()

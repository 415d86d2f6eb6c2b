"""VectorCorrelation (gr_vcorr_*) at the smallest shapes that can go wrong, every case against the numpy restatement tests/vcorr_ref.py:
the vectors and the per-vector curves bit for bit, the all-vector curves under the derived bound of tests/test_gpu_vcorr.py, and itself
bit for bit under another launch setting.
  vectors       1, 63, 64, 65 (the wave and the pad of the panels), 200 (four waves, a pad of 56)
  frame counts  1, 2, 63, 64, 65, 129, 130 (the blocks of the Gram matrix; the walk's ring of 4 frames with and without a tail), each in an
                object whose capacity is exactly that
  max_lag       0, 1, 63, 64, 65, frames - 1: each curve a prefix of the full one, bit for bit
  the segment   one append of 1030 frames of 5 vectors, across the 1024-frame cut of a batched call, against pieces of 7
  failed frames at time index 0, 63, 64 and the last: a named atom without position, an atom no pair names (fails nothing), with a
                minimum image a frame without a box; the pair counts are the host formula's, the rows zeros
  one kept panel a P1-only and a P2-only object (panel 0 of the product's launch is X1 or X2, the grid one panel high) of ONE vector, 65 frames
                (two block rows, the second with one live frame), one of them failed, max_lag 3 and 64: the curves bit for bit in the
                order of the band's sums (tests/band_ref.py), and the bits of the object that keeps both panels
  the product's prefetch depth (3 trips) divides every trip count (12 or 24 per 64 vectors): there is no tail to leave"""
import functools

import numpy as np
import pytest

import band_ref as B
import vcorr_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
NP, NF = 200, 130
SIZES = [1, 63, 64, 65, 200]
FRAMES = [1, 2, 63, 64, 65, 129, 130]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@functools.lru_cache(maxsize=None)
def world(n_pairs=NP, n_frames=NF, cell="tric"):
    return R.bonded_world(n_pairs, n_frames, 20261102, cell)


def make_system(G, frames, boxes):
    s = G.System(len(frames[0]), n_slots=len(frames))
    for k, x in enumerate(frames):
        s.set_frame(x, None if boxes[k] is None else [float(v) for v in boxes[k]], slot=k)
    return s


@pytest.fixture(scope="module")
def system(G):
    s = make_system(G, *world()[:2])
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def ref():
    frames, boxes, pairs, straddle = world()
    q = R.Panels(pairs)
    assert not q.append(frames)[0].any()
    return q.x1()


def within_bound(G, v, x1, ok, max_lag=None):
    V, n_pad = v.n_vectors, v.stat(G._lib.VCORR_STAT_N_PAD)
    assert n_pad == (V + 63) // 64 * 64
    c1, c2, pairs = v.correlate(max_lag)
    assert np.array_equal(pairs, R.pair_counts(ok, max_lag))
    den, have = pairs.astype(np.float64) * V, pairs > 0
    for rank, got, panel in ((1, c1, x1), (2, c2, R.rank2(x1))):
        S, A = R.direct(panel, ok, max_lag)
        want = R.close(np.asarray(S, np.float64), den, rank)
        bound = R.sum_bound(A, pairs, panel.shape[2] * n_pad)[have] / den[have] * (1.5 if rank == 2 else 1.0) + 4 * U * (np.abs(want[have]) + 1.0)
        assert np.array_equal(np.isnan(got), ~have) and (np.abs(got - want)[have] <= bound).all()
    return c1, c2, pairs


def bits(v, max_lag=None):
    return tuple(a.tobytes() for a in v.correlate(max_lag) + v.correlate_each(max_lag)) + (v.vectors(0, v.n_frames).tobytes(),)


@pytest.mark.parametrize("V", SIZES)
def test_vector_and_frame_counts(G, system, V):
    pairs = world()[2][:V]
    for nf in FRAMES:
        x1, ok = ref()[:nf, :V], [True] * nf
        with G.VectorCorrelation(system, pairs, nf) as v, G.VectorCorrelation(system, pairs, nf) as other:      # capacity: exactly full
            other.set_launch(1, 1, 1)
            for x in (v, other):
                assert not x.append(0, nf).any() and x.n_frames == nf == x.capacity
            assert R.same_bits(v.vectors(0, nf), x1)
            c1, c2, cnt = within_bound(G, v, x1, ok)
            e1, e2 = v.correlate_each()
            assert len(c1) == nf and e1.shape == (V, nf)
            assert R.same_bits(e1, R.each(x1, ok, 1)) and R.same_bits(e2, R.each(R.rank2(x1), ok, 2))
            assert bits(other) == bits(v)
            assert (other.stat(G._lib.VCORR_STAT_LAST_WALK_GROUPS), other.stat(G._lib.VCORR_STAT_LAST_GRAM_GROUPS), other.stat(G._lib.VCORR_STAT_LAST_EACH_GROUPS)) == (1, 1, 1)
            with pytest.raises(G.DeviceError):
                v.append(0, 1)                                                             # full


@pytest.mark.parametrize("launch", [(3, 2, 5), (5000, 0, 7), (0, 4, 0)])
def test_grid_independence(G, system, launch):
    pairs = world()[2]
    with G.VectorCorrelation(system, pairs, NF, pbc=True) as a, G.VectorCorrelation(system, pairs, NF, pbc=True) as b:
        b.set_launch(*launch)
        a.append(0, NF); b.append(0, 50); b.append(50, NF - 50)
        assert bits(a) == bits(b) and bits(a, 70) == bits(b, 70)
        if launch[0]:
            assert b.stat(G._lib.VCORR_STAT_LAST_WALK_GROUPS) == launch[0]
        if launch[1]:
            assert b.stat(G._lib.VCORR_STAT_LAST_GRAM_GROUPS) == launch[1] < a.stat(G._lib.VCORR_STAT_LAST_GRAM_GROUPS)
        if launch[2]:
            assert b.stat(G._lib.VCORR_STAT_LAST_EACH_GROUPS) == launch[2] < a.stat(G._lib.VCORR_STAT_LAST_EACH_GROUPS)


@pytest.mark.parametrize("V", [1, 65])
def test_max_lag_gives_prefixes_of_the_full_curves(G, system, V):
    pairs = world()[2][:V]
    x1, ok = ref()[:, :V], [True] * NF
    with G.VectorCorrelation(system, pairs, NF) as v:
        v.append(0, NF)
        c1, c2, cnt = v.correlate()
        e1, e2 = v.correlate_each()
        for lag in (0, 1, 63, 64, 65, NF - 1):
            s1, s2, scnt = within_bound(G, v, x1, ok, lag)
            n = lag + 1
            assert len(s1) == n == v.stat(G._lib.VCORR_STAT_LAGS)
            assert s1.tobytes() == c1[:n].tobytes() and s2.tobytes() == c2[:n].tobytes() and scnt.tobytes() == cnt[:n].tobytes()
            f1, f2 = v.correlate_each(lag)
            assert R.same_bits(f1, np.ascontiguousarray(e1[:, :n])) and R.same_bits(f2, np.ascontiguousarray(e2[:, :n]))
        assert len(v.correlate(10 ** 6)[0]) == NF                                          # a lag beyond the last frame is clamped


def test_one_append_across_the_1024_frame_segment(G):
    frames, boxes, pairs, straddle = world(5, 1030, "rescaled")
    s = make_system(G, frames, boxes)
    q = R.Panels(pairs)
    assert not q.append(frames)[0].any()
    with G.VectorCorrelation(s, pairs, 1030) as v, G.VectorCorrelation(s, pairs, 1030) as cut:
        assert not v.append(0, 1030).any()
        assert v.stat(G._lib.VCORR_STAT_LAUNCHES) == 2                                     # two segments
        for k in range(0, 1030, 7):
            cut.append(k, min(7, 1030 - k))
        assert R.same_bits(v.vectors(0, 1030), q.x1())
        assert bits(cut, 70) == bits(v, 70)
        c1, c2, cnt = within_bound(G, v, q.x1(), q.ok)
        assert len(c1) == 1030 and cnt[1029] == 1 and v.stat(G._lib.VCORR_STAT_LAST_BLOCKS) == 17 * 18 // 2
        e1, e2 = v.correlate_each()
        assert R.same_bits(e1, R.each(q.x1(), q.ok, 1)) and R.same_bits(e2, R.each(q.x2(), q.ok, 2))
        short = v.correlate(64)
        assert short[0].tobytes() == c1[:65].tobytes() and short[1].tobytes() == c2[:65].tobytes()
        assert v.stat(G._lib.VCORR_STAT_LAST_BLOCKS) == 17 + 16                               # the band: not every block
    s.close()


@pytest.mark.parametrize("kind", ["named", "unnamed", "nobox"])
def test_failed_frames_at_the_block_edges(G, kind):
    frames, boxes, pairs, straddle = world(40, NF, "ortho")
    frames, boxes = [x.copy() for x in frames], list(boxes)
    pairs = pairs[:33]                                                                      # atoms 66 .. 79 are named by no pair
    where = [0, 63, 64, NF - 1]
    for t in where:
        if kind == "named":
            frames[t][[21, 8]] = np.nan
        elif kind == "unnamed":
            frames[t][70] = np.nan
        else:
            boxes[t] = None
    pbc = kind == "nobox"
    s = make_system(G, frames, boxes)
    q = R.Panels(pairs, pbc=pbc)
    st, bad = q.append(frames, boxes)
    with G.VectorCorrelation(s, pairs, NF, pbc=pbc) as v:
        got = v.append(0, NF, raise_on_error=False)
        assert got.tolist() == st.tolist()
        failed = kind != "unnamed"
        assert [int(got[t]) for t in where] == [{"named": R.E_NO_POSITION, "unnamed": 0, "nobox": R.E_NO_BOX}[kind]] * 4
        assert v.n_frames == NF and v.stat(G._lib.VCORR_STAT_COUNTED) == NF - (4 if failed else 0)
        x = v.vectors(0, NF)
        if pbc:                                                                             # (with a minimum image the rows are compared through the run without one)
            with G.VectorCorrelation(s, pairs, NF) as raw:
                raw.append(0, NF)
                inside = ~straddle[:, :33]
                inside[where] = False
                assert R.same_bits(x[inside], raw.vectors(0, NF)[inside])
        else:
            assert R.same_bits(x, q.x1())
        assert all(bool(x[t].any()) != failed for t in where) and x[1].any()                # zero rows
        c1, c2, cnt = within_bound(G, v, x, q.ok)
        okv = np.array(q.ok)
        assert cnt.tolist() == [int((okv[:NF - t] & okv[t:]).sum()) for t in range(NF)]     # the host formula
        if failed:
            assert cnt[0] == NF - 4 and cnt[NF - 1] == 0 and np.isnan(c1[NF - 1]) and np.isnan(c2[NF - 1])
        e1, e2 = v.correlate_each()
        assert R.same_bits(e1, R.each(x, q.ok, 1)) and R.same_bits(e2, R.each(R.rank2(x), q.ok, 2))
        assert np.isnan(e1[:, NF - 1]).all() == failed
        # the first error of a mixed batch is the first failing frame's
        if kind == "named":
            with pytest.raises(G.AtomError) as e:
                G.VectorCorrelation(s, pairs, NF).append(0, NF)
            assert e.value.variant == "InvalidPosition" and e.value.detail == 8 and e.value.status == R.E_NO_POSITION
        elif kind == "nobox":
            with pytest.raises(G.SimBoxError) as e:
                G.VectorCorrelation(s, pairs, NF, pbc=True).append(60, 10)
            assert e.value.status == R.E_NO_BOX
    s.close()


def test_a_vector_of_length_zero(G):
    frames, boxes, pairs, straddle = world(12, 20, "ortho")
    frames = [x.copy() for x in frames]
    for t in (0, 5, 6, 19):
        frames[t][7] = frames[t][6]                                                         # pair 3 = (6, 7)
    s = make_system(G, frames, boxes)
    q = R.Panels(pairs)
    assert not q.append(frames)[0].any()
    with G.VectorCorrelation(s, pairs, 20) as v:
        assert not v.append(0, 20).any()                                                    # no frame fails
        x = v.vectors(0, 20)
        assert R.same_bits(x, q.x1()) and not x[[0, 5, 6, 19], 3].any() and x[1, 3].any() and np.isfinite(x).all()
        e1, e2 = v.correlate_each()
        assert R.same_bits(e1, R.each(q.x1(), q.ok, 1)) and R.same_bits(e2, R.each(q.x2(), q.ok, 2))
        # the vector adds nothing to the sums but counts in the mean: lag 0 of vector 3 is 16 / 20, and -0.5 + 1.5 * 16 / 20
        assert abs(e1[3, 0] - 0.8) <= 9 * R.EPS32 and abs(e2[3, 0] - 0.7) <= 35 * R.EPS32 and e1[3, 19] == 0.0 and e2[3, 19] == -0.5
        c1, c2, cnt = within_bound(G, v, x, q.ok)
        assert cnt[0] == 20 and abs(c1[0] - (12 * 20 - 4) / 240.0) <= 9 * R.EPS32
    s.close()


def test_clear_and_reuse(G, system):
    pairs = world()[2][:65]
    with G.VectorCorrelation(system, pairs, 40) as a, G.VectorCorrelation(system, pairs, 40) as b:
        a.append(7, 33); a.correlate(5); a.correlate_each(3)
        a.clear()
        assert a.n_frames == 0 and a.stat(G._lib.VCORR_STAT_COUNTED) == 0 and a.stat(G._lib.VCORR_STAT_LAGS) == 0
        a.append(0, 40); b.append(0, 40)                                                    # the full capacity again
        assert R.same_bits(a.vectors(0, 40), ref()[:40, :65]) and bits(a) == bits(b)


def test_refusals(G, system):
    from groan_rs_amd.system import _ptr
    pairs = world()[2][:10]
    n_atoms = 2 * NP
    for bad in ({"unit": False}, {"unit": False, "rank": 2}, {"rank": ()}, {"capacity": 0}, {"pairs": np.zeros((0, 2), np.uint64)}, {"pairs": [[3, 3]]}):
        kw = {"pairs": pairs, "capacity": 8, "rank": (1, 2), "unit": True}; kw.update(bad)
        with pytest.raises(G.DeviceError) as e:                                             # P2 without UNIT; no rank; no room; no pair; i == j
            G.VectorCorrelation(system, kw["pairs"], kw["capacity"], rank=kw["rank"], unit=kw["unit"])
        assert e.value.status == R.E_INVALID_ARG
    with pytest.raises(G.AtomError) as e:
        G.VectorCorrelation(system, [[0, 1], [2, n_atoms + 5]], 8)
    assert e.value.variant == "OutOfRange" and e.value.detail == n_atoms + 5 and e.value.status == R.E_OUT_OF_RANGE
    with pytest.raises(ValueError):
        G.VectorCorrelation(system, pairs, 8, rank=(1, 3))
    with pytest.raises(G.DeviceError) as e:                                                 # the panels beyond MSD's cap
        G.VectorCorrelation(system, pairs, 2 ** 31 - 1)
    assert e.value.status == R.E_INVALID_ARG
    G.VectorCorrelation(system, pairs, 8, rank=1, unit=False).close()                       # P1 of raw vectors is allowed
    v = G.VectorCorrelation(system, pairs, 10, rank=1)
    lib = v._lib
    assert lib.gr_vcorr_read(v._f, None, None, None) == R.E_INVALID_ARG                     # read before compute
    assert lib.gr_vcorr_compute(v._f, 3) == R.E_INVALID_ARG                                 # nothing appended
    v.append(0, 7)
    keep = (v.vectors(0, 7).tobytes(), v.correlate()[0].tobytes(), v.correlate_each()[0].tobytes())
    with pytest.raises(G.DeviceError) as e:                                                 # beyond the capacity: refused, nothing changed
        v.append(7, 4)
    assert e.value.status == R.E_INVALID_ARG and v.n_frames == 7 and v.stat(G._lib.VCORR_STAT_LAGS) == 7
    assert (v.vectors(0, 7).tobytes(), v.correlate()[0].tobytes(), v.correlate_each()[0].tobytes()) == keep
    with pytest.raises(G.DeviceError):
        v.append(NF - 1, 2)                                                                 # slots out of range
    with pytest.raises(G.DeviceError):
        v.vectors(5, 3)                                                                     # rows beyond the appended frames
    buf = np.zeros(7, np.float64)
    assert lib.gr_vcorr_read(v._f, None, _ptr(buf), None) == R.E_INVALID_ARG                # a rank that is not kept
    assert lib.gr_vcorr_read(v._f, _ptr(buf), None, None) == 0
    big = np.zeros((10, 7), np.float64)
    assert lib.gr_vcorr_compute_each(v._f, 6, None, _ptr(big)) == R.E_INVALID_ARG and lib.gr_vcorr_compute_each(v._f, 6, None, None) == R.E_INVALID_ARG
    v.append(7, 3)                                                                          # exactly full
    assert lib.gr_vcorr_read(v._f, _ptr(buf), None, None) == R.E_INVALID_ARG                # an append behind the compute: the curve is stale
    v.close()
    with pytest.raises(ValueError):
        v.n_frames                                                                          # closed
    with G.VectorCorrelation(system, pairs, 10, rank=2) as two:
        two.append(0, 3)
        with pytest.raises(G.DeviceError) as e:
            two.vectors(0, 3)                                                               # the vectors are the rank-1 panel
        assert e.value.status == R.E_INVALID_ARG


def test_an_output_above_the_cap_is_refused(G, system):
    """V x lags x 8 B of correlate_each above GR_VCORR_MAX_EACH_BYTES = 2^30: 2^21 vectors (pairs may repeat atoms) x 65 lags"""
    V = 2 ** 21
    rng = np.random.default_rng(3)
    i = rng.integers(0, 2 * NP, V)
    pairs = np.stack([i, (i + 1 + rng.integers(0, 2 * NP - 1, V)) % (2 * NP)], 1).astype(np.uint64)
    with G.VectorCorrelation(system, pairs, 65, rank=1, unit=False) as v:
        v.append(0, 65)
        assert V * 65 * 8 > G._lib.VCORR_MAX_EACH_BYTES >= V * 64 * 8
        with pytest.raises(G.DeviceError) as e:
            v.correlate_each()
        assert e.value.status == R.E_INVALID_ARG
        e1, e2 = v.correlate_each(3)                                                        # below the cap the same object answers
        q = R.Panels(pairs[:70], unit=False)
        q.append(world()[0][:65])
        assert e2 is None and e1.shape == (V, 4) and R.same_bits(np.ascontiguousarray(e1[:70]), R.each(q.x1(), q.ok, 1, 3))


@pytest.mark.parametrize("rank", [1, 2])
def test_one_kept_panel_of_one_vector_in_the_order_of_the_band(G, rank):
    frames, boxes, pairs, straddle = world(3, 65, "ortho")
    frames = [x.copy() for x in frames]
    pairs = pairs[1:2]                                                                      # the vector (2, 3)
    frames[62][3] = np.nan
    s = make_system(G, frames, boxes)
    q = R.Panels(pairs)
    st, bad = q.append(frames)
    assert st.tolist() == [0] * 62 + [R.E_NO_POSITION, 0, 0] and bad[62] == 3
    x1 = q.x1()
    panel = x1 if rank == 1 else R.rank2(x1)
    value = B.gram(panel[:, 0, :])
    with G.VectorCorrelation(s, pairs, 65, rank=rank) as v, G.VectorCorrelation(s, pairs, 65) as both:
        for x in (v, both):
            assert x.append(0, 65, raise_on_error=False).tolist() == st.tolist()
        assert v.stat(G._lib.VCORR_STAT_N_PAD) == 64 and v.stat(G._lib.VCORR_STAT_COUNTED) == 64
        assert R.same_bits(both.vectors(0, 65), x1) and not x1[62].any()
        for lag in (3, 64):
            out = v.correlate(lag)
            got, cnt = out[rank - 1], out[2]
            assert out[2 - rank] is None and np.array_equal(cnt, R.pair_counts(q.ok, lag)) and cnt[0] == 64 and cnt[1] == 62
            assert v.stat(G._lib.VCORR_STAT_LAST_BLOCKS) == 3 and v.stat(G._lib.VCORR_STAT_LAST_GRAM_GROUPS) == 3
            want = R.close(B.band_sums(value, q.ok, lag, strict=False), cnt.astype(np.float64), rank)
            print("rank %d, max_lag %d: largest difference from the restated order %.3g" % (rank, lag, np.abs(got - want).max()))
            assert R.same_bits(got, want)
            assert got.tobytes() == both.correlate(lag)[rank - 1].tobytes()
            assert R.same_bits(v.correlate_each(lag)[rank - 1], R.each(panel, q.ok, rank, lag))
        assert cnt[64] == 1
    s.close()

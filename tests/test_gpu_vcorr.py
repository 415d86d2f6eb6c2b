"""VectorCorrelation over resident frames (gr_vcorr_*; groan_rs_amd.VectorCorrelation) against the numpy restatement tests/vcorr_ref.py.

System: 150 bonded pairs (300 atoms), 130 frames (three block rows of the Gram matrix) per cell: orthorhombic, triclinic, rescaled from
frame to frame.  The even atoms walk at random (msd_ref.walk), every odd atom sits 0.1 nm from its partner in a direction that diffuses
on the sphere; both are wrapped into the cell, so some pairs straddle it in some frames.

BIT FOR BIT: without a minimum image `vectors()` is the restatement's panel rule, and `correlate_each` -- which reads both device
panels -- the restatement's chains over the restatement's panels.  With a minimum image a pair that does not straddle the cell gives
the bits of the run without one (k = 0 in every reduction: fmaf(-0, L, d) = d; the candidate search is not entered below half the
shortest lattice vector).

THE BOUND OF A STRADDLING PAIR against the f64 minimum image of the stored coordinates (vcorr_ref.unit_error, stored=False, of the kind
of DESIGN.md 3.16): the f32 subtraction x_j - x_i is formed at the size of the raw difference, at most 2 X with X the largest
|coordinate|, and up to four more single-rounded steps follow (three fused reductions, one candidate shift): per component
5 * ulp32(2 X) / 2, |delta d| <= sqrt(3) of it; normalising moves the unit vector by at most 2 |delta d| / b (b the shortest bond),
the rule's own roundings add 4 * 2^-24.  With X = 3.4 .. 4.0 nm (ulp32(2 X) = 2^-21), b = 0.1 nm: eps = 4.15e-5.  Measured worst
share: 0.059 (tric), 0.003 for the pairs inside the cell.

THE BOUND OF `correlate` against the long-double direct sum over the device's own panel, per lag with P pairs and A = the sum of the
|products| of its pairs, u = 2^-53 (as tests/test_gpu_msd.py derives for D2): an entry G(t, t') is ONE chain of K = 3 n_pad (6 n_pad)
exact products, |dG| <= K u sum |x y|; the P entries of a lag are added in at most P additions, each within u of a partial sum that is
at most A: |dS| <= (K + P) u A, stated as (K + 1 + P) u A for the second-order terms (vcorr_ref.sum_bound).  The closing divides by
P V (and multiplies by 1.5): two or three more roundings of the result, 4 u (|C| + 1).  Measured worst share: 0.027 (the products'
errors are of random sign)."""
import functools

import numpy as np
import pytest

import vcorr_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
NP, NF, BOND = 150, 130, 0.1
SEED = 20261101
CELLS = ("ortho", "rescaled", "tric")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@functools.lru_cache(maxsize=None)
def world(cell):
    return R.bonded_world(NP, NF, SEED, cell, BOND)


def make_system(G, frames, boxes=None, n_slots=None):
    n = n_slots or len(frames)
    s = G.System(len(frames[0]), n_slots=n)
    for k, x in enumerate(frames[:n]):
        s.set_frame(x, None if boxes is None or boxes[k] is None else [float(v) for v in boxes[k]], slot=k)
    return s


@pytest.fixture(scope="module")
def systems(G):
    ws = {cell: make_system(G, *world(cell)[:2]) for cell in CELLS}
    yield ws
    for s in ws.values():
        s.close()


@functools.lru_cache(maxsize=None)
def ref(cell, unit=True):
    frames, boxes, pairs, straddle = world(cell)
    q = R.Panels(pairs, unit=unit)
    st, bad = q.append(frames)
    assert not st.any()
    return q


@functools.lru_cache(maxsize=None)
def ref_each(cell, rank):
    q = ref(cell)
    return R.each(q.x1() if rank == 1 else q.x2(), q.ok, rank)


def state_bits(v, max_lag=None):
    c1, c2, pairs = v.correlate(max_lag)
    e1, e2 = v.correlate_each(max_lag)
    return tuple(None if a is None else a.tobytes() for a in (v.vectors(0, v.n_frames), c1, c2, pairs, e1, e2))


def check_correlate(G, v, x1, ok, max_lag=None):
    """c1, c2, pairs of `v` against the long-double direct sum over the panel x1 (and its rank-2 entries) -> the worst share of the bound"""
    V, n_pad = v.n_vectors, v.stat(G._lib.VCORR_STAT_N_PAD)
    assert n_pad % 64 == 0 and 0 <= n_pad - V < 64
    c1, c2, pairs = v.correlate(max_lag)
    want_pairs = R.pair_counts(ok, max_lag)
    assert pairs.dtype == np.uint64 and np.array_equal(pairs, want_pairs) and len(pairs) == v.stat(G._lib.VCORR_STAT_LAGS)
    den = pairs.astype(np.float64) * V
    have = pairs > 0
    share = 0.0
    for rank, got, panel in ((1, c1, x1), (2, c2, R.rank2(x1))):
        if got is None:
            continue
        S, A = R.direct(panel, ok, max_lag)
        want = R.close(np.asarray(S, np.float64), den, rank)
        assert got.dtype == np.float64 and np.array_equal(np.isnan(got), ~have)
        K = panel.shape[2] * n_pad
        bound = R.sum_bound(A, pairs, K)[have] / den[have] * (1.5 if rank == 2 else 1.0) + 4 * U * (np.abs(want[have]) + 1.0)
        err = np.abs(got[have] - want[have])
        assert (err <= bound).all(), (rank, (err / bound).max())
        share = max(share, float((err / bound).max()))
    return share


@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("cell", CELLS)
def test_vectors_and_chains_are_the_restatement_bit_for_bit(G, systems, cell, unit):
    q = ref(cell, unit)
    with G.VectorCorrelation(systems[cell], world(cell)[2], NF, rank=(1, 2) if unit else 1, unit=unit) as v:
        assert v.n_vectors == NP == len(v) and v.capacity == NF and v.n_frames == 0
        st = v.append(0, NF)
        assert st.dtype == np.int32 and not st.any() and v.n_frames == NF and v.stat(G._lib.VCORR_STAT_COUNTED) == NF
        x = v.vectors(0, NF)
        assert x.dtype == F and x.shape == (NF, NP, 3)
        assert R.same_bits(x, q.x1())
        assert R.same_bits(v.vectors(7, 3), x[7:10])
        e1, e2 = v.correlate_each()
        assert e1.dtype == np.float64 and e1.shape == (NP, NF)
        if unit:
            assert R.same_bits(e1, ref_each(cell, 1)) and R.same_bits(e2, ref_each(cell, 2))      # both panels hold the restatement's bits
            # lag 0 of unit vectors: |u|^2 = 1 within 8 * 2^-24 (each component within 4 * 2^-24 relative), its square within twice
            # that, the f32 rank-2 entries add 8 * 2^-24 times 1.5
            assert np.abs(e1[:, 0] - 1.0).max() <= 9 * R.EPS32 and np.abs(e2[:, 0] - 1.0).max() <= 35 * R.EPS32
        else:
            assert e2 is None and R.same_bits(e1, R.each(q.x1(), q.ok, 1))
            d = x.astype(np.float64)
            assert np.abs(np.sqrt((d * d).sum(2)) - BOND)[~world(cell)[3]].max() < 1e-6            # raw vectors: the bond where the pair does not straddle


@pytest.mark.parametrize("cell", CELLS)
def test_minimum_image(G, systems, cell):
    frames, boxes, pairs, straddle = world(cell)
    assert straddle.any() and straddle.mean() < 0.5 and straddle.any(1).sum() > NF // 2
    with G.VectorCorrelation(systems[cell], pairs, NF, pbc=True) as v, G.VectorCorrelation(systems[cell], pairs, NF) as raw:
        assert not v.append(0, NF).any() and not raw.append(0, NF).any()
        x, x0 = v.vectors(0, NF), raw.vectors(0, NF)
        assert R.same_bits(x[~straddle], x0[~straddle])
        want = np.stack([R.vectors64(frames[t], pairs, boxes[t]) for t in range(NF)])
        coord = max(float(np.abs(f).max()) for f in frames)
        d = np.stack([R.vectors64(frames[t], pairs, boxes[t], unit=False) for t in range(NF)])
        shortest = float(np.sqrt((d * d).sum(2)).min())
        assert abs(shortest - BOND) < 1e-6
        eps = R.unit_error(coord, shortest, steps=5.0, size=2.0 * coord, stored=False)
        err = np.abs(x.astype(np.float64) - want)
        print("%s: %d straddling vectors, largest |coordinate| %.2f, eps %.2e, worst share %.3f (straddling), %.3f (inside)"
              % (cell, int(straddle.sum()), coord, eps, err[straddle].max() / eps, err[~straddle].max() / eps))
        assert err.max() <= eps
        # without the minimum image a straddling vector points the other way round: the two runs do differ there
        assert np.abs(x[straddle] - x0[straddle]).max() > 0.5
        e1, e2 = v.correlate_each(20)
        assert R.same_bits(e1, R.each(x, [True] * NF, 1, 20)) and R.same_bits(e2, R.each(R.rank2(x), [True] * NF, 2, 20))


@pytest.mark.parametrize("cell", CELLS)
def test_correlate_within_the_derived_bound(G, systems, cell):
    q = ref(cell)
    with G.VectorCorrelation(systems[cell], world(cell)[2], NF) as v:
        v.append(0, NF)
        x = v.vectors(0, NF)
        share = check_correlate(G, v, x, q.ok)
        c1, c2, pairs = v.correlate()
        assert len(c1) == NF == len(c2) and pairs.tolist() == list(range(NF, 0, -1))
        assert abs(c1[0] - 1.0) <= 9 * R.EPS32 and abs(c2[0] - 1.0) <= 35 * R.EPS32
        # the mean over the vectors of the per-vector curves: another order of the same f64 sums
        e1, e2 = v.correlate_each()
        for rank, got, each, panel in ((1, c1, e1, x), (2, c2, e2, R.rank2(x))):
            S, A = R.direct(panel, q.ok)
            K = panel.shape[2] * v.stat(G._lib.VCORR_STAT_N_PAD)
            den = pairs.astype(np.float64) * NP
            bound = (R.sum_bound(A, pairs, K) + NF * NP * panel.shape[2] * U * np.asarray(A, np.float64)) / den * (1.5 if rank == 2 else 1.0) + 8 * U * (np.abs(got) + 1.0)
            assert (np.abs(each.mean(0) - got) <= bound).all()
            assert (bound <= 9 * R.EPS32).all()                                              # (far inside the f32 normalisation bound)
        # the curves decay: the vectors diffuse on the sphere
        assert c1[1] > c1[10] > c1[60] and c2[1] > c2[10] and c2[1] < c1[1]
        print("%s: correlate within %.4f of its bound at worst" % (cell, share))


def test_rank_selection_and_short_bands(G, systems):
    q = ref("tric")
    pairs = world("tric")[2]
    with G.VectorCorrelation(systems["tric"], pairs, NF) as both, G.VectorCorrelation(systems["tric"], pairs, NF, rank=1) as one, \
            G.VectorCorrelation(systems["tric"], pairs, NF, rank=(2,)) as two:
        for v in (both, one, two):
            v.append(0, NF)
        c1, c2, cnt = both.correlate()
        a1, a2, acnt = one.correlate()
        b1, b2, bcnt = two.correlate()
        assert a2 is None and b1 is None and a1.tobytes() == c1.tobytes() and b2.tobytes() == c2.tobytes() and cnt.tobytes() == acnt.tobytes() == bcnt.tobytes()
        assert one.correlate_each(5)[1] is None and two.correlate_each(5)[0] is None
        assert two.correlate_each(5)[1].tobytes() == both.correlate_each(5)[1].tobytes()
        for lag in (0, 1, 63, 64, 65, NF - 1, NF + 7):
            n = min(lag, NF - 1) + 1
            s1, s2, scnt = both.correlate(lag)
            assert len(s1) == n and s1.tobytes() == c1[:n].tobytes() and s2.tobytes() == c2[:n].tobytes() and scnt.tobytes() == cnt[:n].tobytes()
        check_correlate(G, two, q.x1(), q.ok, 70)


@pytest.mark.parametrize("theta,omega", [(0.6, 0.11), (np.pi / 2, 0.05)])
def test_rigid_rotor_on_the_device(G, theta, omega):
    V, T = 70, 100
    frames, pairs = R.rotor(V, T, theta, omega, 11)
    s = make_system(G, frames)
    with G.VectorCorrelation(s, pairs, T) as v:
        assert not v.append(0, T).any()
        c1, c2, cnt = v.correlate()
        w1, w2 = R.rotor_curves(theta, omega, T)
        b1, b2 = R.curve_bounds(R.unit_error(max(float(np.abs(x).max()) for x in frames), BOND))
        print("rotor theta %.2f: C1 within %.3f of its bound, C2 within %.3f" % (theta, np.abs(c1 - w1).max() / b1, np.abs(c2 - w2).max() / b2))
        assert np.abs(c1 - w1).max() <= b1 and np.abs(c2 - w2).max() <= b2
        e1, e2 = v.correlate_each()
        assert np.abs(e1 - w1).max() <= b1 and np.abs(e2 - w2).max() <= b2
    s.close()


def test_cut_invariance(G, systems):
    """one call, calls of 1, 7 and 64 frames, and a trajectory longer than the slots appended block by block: the same bits"""
    frames, boxes, pairs, straddle = world("rescaled")
    with G.VectorCorrelation(systems["rescaled"], pairs, NF, pbc=True) as one:
        one.append(0, NF)
        keep = state_bits(one, 70)
        for cut in (1, 7, 64):
            with G.VectorCorrelation(systems["rescaled"], pairs, NF, pbc=True) as v:
                for k in range(0, NF, cut):
                    v.append(k, min(cut, NF - k))
                assert state_bits(v, 70) == keep, cut
        small = make_system(G, frames, boxes, n_slots=48)
        with G.VectorCorrelation(small, pairs, NF, pbc=True) as v:
            for k in range(0, NF, 48):
                n = min(48, NF - k)
                for j in range(n):
                    small.set_frame(frames[k + j], [float(b) for b in boxes[k + j]], slot=j)
                v.append(0, n)
            assert state_bits(v, 70) == keep
        small.close()


def test_history_independence(G, systems):
    frames, boxes, pairs, straddle = world("ortho")
    used = make_system(G, frames, boxes)
    used.group_center_batch("all", G._lib.CENTER_PBC, 1, 0, 10, raise_on_error=False)
    m = G.MSD(used, "all", 40, dims="z"); m.append(5, 30); m.msd()
    ic = G.Internals(used, "distance", pairs[:50]); ic.values(0, 20)
    other = G.VectorCorrelation(used, pairs[10:90], 30, rank=2, pbc=True); other.append(3, 25); other.correlate(); other.correlate_each(4)
    for pbc in (False, True):
        with G.VectorCorrelation(systems["ortho"], pairs, NF, pbc=pbc) as a, G.VectorCorrelation(used, pairs, NF, pbc=pbc) as b:
            a.append(0, NF); b.append(0, NF)
            assert state_bits(a) == state_bits(b)
    used.close()

"""The hydrogen-bond analysis (gr_hbonds.h) where tests/test_gpu_hbonds.py does not go: donors with more hydrogens than the walk
keeps in registers, both sides of the NaN-angle rule, one batch whose frames have different grids and starts above slot 0, and
donor-acceptor distances exactly on max_distance in an orthorhombic cell.

The yardsticks are those of tests/test_gpu_hbonds.py (tests/hbond_ref.py through compare(): 2e-6 nm / 1e-3 deg round the two
thresholds); the last test has an integer model instead and allows nothing."""
import itertools

import numpy as np
import pytest

import hbond_ref as R
import oracle_lib as O
import test_gpu_hbonds as TH

pytestmark = pytest.mark.gpu
HREG = 4                                    # GR_HB_HREG: hydrogens of a donor the walk holds in registers


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def ortho9(box):
    return np.array(list(box) + [0.0] * 6, np.float32)


# ------------------------------------------------------------------ E: donors with up to seven hydrogens
MANY_H = {"ortho": (ortho9([3.0, 3.2, 3.4]), 23), "triclinic": (None, 29)}      # box, seed (settled on the CPU with hbond_ref alone)
MANY_DMAX, MANY_AMIN = 0.35, 110.0


def many_h_case(kind):
    b9, seed = MANY_H[kind]
    if b9 is None:
        b9 = O.box_from_lengths_angles([3.2, 3.4, 3.0], [70.0, 80.0, 65.0])
    return (b9,) + TH.seeded(seed, b9, n_don=200, n_other=400, max_h=7)


def many_h_conditions(want, hyds_of):
    """(bonds whose hydrogen is the 5th or a later one of its donor, bonds inside compare()'s forgiven bands, all bonds)"""
    late = band = total = 0
    for bonds in want.values():
        for d, h, a, dist, ang in bonds:
            total += 1
            late += hyds_of[d].index(h) >= HREG
            band += abs(float(dist) - MANY_DMAX) <= 2e-6 or abs(float(ang) - MANY_AMIN) <= 1e-3
    return late, band, total


@pytest.mark.parametrize("kind", ["ortho", "triclinic"])
def test_many_hydrogens_per_donor(G, kind):
    b9, pos, donors, others, hyds, bonds = many_h_case(kind)
    nb = R.bonded(bonds, pos.shape[0])
    hyds_of = {int(d): sorted(nb[int(d)]) for d in donors}
    assert sum(len(h) > HREG for h in hyds_of.values()) >= 40 and max(len(h) for h in hyds_of.values()) == 7
    s, an, pairs, rchains = TH.multi_chain(G, pos, b9, donors, others, hyds, bonds, MANY_DMAX, MANY_AMIN)
    want = R.analyze(pos, b9, rchains, pairs, MANY_DMAX, MANY_AMIN)
    late, band, total = many_h_conditions(want, hyds_of)
    assert late >= 50 and band * 100 <= total, (late, band, total)        # the case is not empty and not decided by the forgiven bands
    if kind == "ortho":
        assert all(n >= 3 for n in (b9[:3] // MANY_DMAX))
    res = an.batch(0, 1)
    assert (res[6] == 0).all()
    common = 0
    for p, key in enumerate(pairs):
        got = TH.frame_bonds(res, len(pairs), 0, p)
        common += TH.compare(got, want[key], MANY_DMAX, MANY_AMIN, dtol=1e-6 if kind == "ortho" else 2e-6)
        if key[0] != key[1]:
            continue
        # one segment: donors in the order of the chain, the run of a donor ascending by (acceptor, hydrogen)
        order = {d: k for k, (d, _) in enumerate(rchains[key[0]][1])}
        keys = [(order[d], a, h) for d, h, a, _, _ in got]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), key
    assert common >= total - band
    got_late = sum(hyds_of[int(d)].index(int(h)) >= HREG for d, h in zip(res[0], res[1]))
    assert got_late >= late - band
    s.close()


def test_sixth_hydrogen_without_position(G):
    b9, pos, donors, others, hyds, bonds = many_h_case("ortho")
    s, an, pairs, rchains = TH.multi_chain(G, pos, b9, donors, others, hyds, bonds, MANY_DMAX, MANY_AMIN)
    accs = set(rchains[0][0]) | set(rchains[1][0]) | set(rchains[2][0])
    cand = R.analyze(pos, b9, rchains, pairs, MANY_DMAX, -1.0)           # every acceptor in range becomes a bond
    with_acc = {b[0] for key in pairs for b in cand[key]}
    six = [(d, hs) for ch in rchains for d, hs in ch[1] if len(hs) >= 6 and hs[5] not in accs and hs[1] not in accs]   # (a hydrogen that is an acceptor too fails earlier, in the grid)
    d_in, h_in = next((d, hs[5]) for d, hs in six if d in with_acc)
    lib, nan = G._lib, np.float32(np.nan)
    p = pos.copy(); p[h_in] = nan
    s.set_frame(p, b9, slot=0)
    r, out, offs, st, tot = TH.raw_batch(G, an, 0, 1, 10 ** 6)
    assert r == lib.E_NO_POSITION and st[0] == lib.E_NO_POSITION and tot == 0 and int(offs[-1]) == 0
    assert int(an._lib.gr_last_error_index(s._ctx)) == h_in
    with pytest.raises(R.HBondRefError) as e:
        R.analyze(p, b9, rchains, pairs, MANY_DMAX, MANY_AMIN)
    assert e.value.payload == h_in
    # ... and with an earlier hydrogen of the same donor missing as well, the earlier one is named
    h_early = dict(six)[d_in][1]
    p[h_early] = nan
    s.set_frame(p, b9, slot=0)
    r, out, offs, st, tot = TH.raw_batch(G, an, 0, 1, 10 ** 6)
    assert r == lib.E_NO_POSITION and int(an._lib.gr_last_error_index(s._ctx)) == h_early
    s.close()
    # The same on a donor with no acceptor in range: no error, and the bonds of the frame as they were.  At 0.35 nm every donor
    # has an acceptor in range (its own hydrogens among them), so this half runs with max_distance below the D-H length (and any angle).
    short = 0.09
    s, an, pairs, rchains = TH.multi_chain(G, pos, b9, donors, others, hyds, bonds, short, 0.0)
    cand = R.analyze(pos, b9, rchains, pairs, short, -1.0)
    with_acc = {b[0] for key in pairs for b in cand[key]}
    assert with_acc
    d_out, h_out = next((d, hs[5]) for d, hs in six if d not in with_acc)
    r0, out0, offs0, st0, tot0 = TH.raw_batch(G, an, 0, 1, 10 ** 6)
    p = pos.copy(); p[h_out] = nan
    assert R.analyze(p, b9, rchains, pairs, short, 0.0).keys() == cand.keys()      # the restatement raises nothing either
    s.set_frame(p, b9, slot=0)
    r, out, offs, st, tot = TH.raw_batch(G, an, 0, 1, 10 ** 6)
    assert r == r0 == 0 and st[0] == 0 and tot == tot0 > 0 and np.array_equal(offs, offs0)
    for k in range(5):
        assert out[k][:tot].tobytes() == out0[k][:tot].tobytes(), k
    s.close()


# ------------------------------------------------------------------ F: the NaN angle, both sides
@pytest.mark.parametrize("min_angle, want", [(150.0, [(0, 1, 2, 180.0)]), (0.0, [(0, 1, 2, 180.0), (3, 4, 5, 0.0)])])
def test_nan_angle_both_sides(G, min_angle, want):
    """hbonds.rs:302-338: a hydrogen on its acceptor is nearer to it than the donor is: 180 degrees; a hydrogen on its donor is
    not: 0 degrees"""
    b9 = ortho9([3.0, 3.0, 3.0])
    pos = np.array([[1.0, 1.0, 1.0], [1.25, 1.0, 1.0], [1.25, 1.0, 1.0],            # donor, hydrogen ON the acceptor, acceptor
                    [2.0, 2.5, 2.0], [2.0, 2.5, 2.0], [2.0, 2.25, 2.0]], np.float32)  # donor, hydrogen ON the donor, acceptor
    bonds = np.array([[0, 1], [3, 4]])
    s = TH.system(G, [pos], [b9], {"A": [2, 5], "D": [0, 3], "H": [1, 4]})
    an = G.HBondAnalysis(s, [G.HBondChain("A", "D", "H")], [(0, 0)], 0.3, min_angle, bonds)
    res = an.batch(0, 1)
    assert (res[6] == 0).all()
    got = TH.frame_bonds(res, 1, 0, 0)
    assert [(d, h, a, ang) for d, h, a, _, ang in got] == want
    assert all(dist == np.float32(0.25) for _, _, _, dist, _ in got)
    chain = R.resolve_chain([2, 5], [0, 3], [1, 4], R.bonded(bonds, 6))
    ref = R.analyze(pos, b9, [chain], [(0, 0)], 0.3, min_angle)[(0, 0)]
    assert [(d, h, a, float(ang)) for d, h, a, _, ang in ref] == want
    s.close()


# ------------------------------------------------------------------ G: frames of different grids in one batch
def chain_groups(donors, others, hyds):
    """the groups of test_gpu_hbonds.multi_chain"""
    heavy = np.sort(np.concatenate([donors, others]))
    n = len(donors)
    d0, d1 = donors[: 3 * n // 5], donors[2 * n // 5:]
    return {"A0": np.union1d(heavy[::2], hyds[::7]), "D0": np.union1d(d0, others[:50]), "A1": np.union1d(heavy[1::2], d1), "D1": d1,
            "H": hyds, "E": [], "D2": d0[:40]}


def redraw(rng, box, donors, others, bonds, n_atoms, spread=(-0.2, 1.2)):
    """positions for the topology of seeded(), drawn anew in the lattice coordinates of `box`: hydrogens 0.1 nm from their donors"""
    L = np.array([[box[0], 0, 0], [box[5], box[1], 0], [box[7], box[8], box[2]]], np.float64)
    pos = np.zeros((n_atoms, 3))
    heavy = np.concatenate([donors, others])
    pos[heavy] = rng.uniform(*spread, (len(heavy), 3)) @ L
    v = rng.normal(size=(len(bonds), 3))
    pos[bonds[:, 1]] = pos[bonds[:, 0]] + 0.1 * v / np.linalg.norm(v, axis=1)[:, None]
    return pos.astype(np.float32)


def test_mixed_grids_in_one_batch(G):
    dmax, amin = 0.3, 130.0
    boxes = [ortho9([3.0, 3.2, 3.4]), ortho9([0.9, 1.5, 4.0]), ortho9([0.45, 0.8, 1.7]), O.box_from_lengths_angles([3.2, 3.4, 3.0], [70.0, 80.0, 65.0]),
             O.box_from_lengths_angles([3.5, 3.5, 3.5], [60.0, 60.0, 90.0]), ortho9([6.0, 0.5, 2.9]), ortho9([3.0, 3.2, 3.4])]
    pos0, donors, others, hyds, bonds = TH.seeded(31, boxes[0], n_don=150, n_other=200)
    n = pos0.shape[0]
    rng = np.random.default_rng(32)
    frames = [redraw(rng, b, donors, others, bonds, n) for b in boxes]
    decoy_boxes = [boxes[3], boxes[2], boxes[5], boxes[1], boxes[4]]
    decoys = [redraw(rng, b, donors, others, bonds, n) for b in decoy_boxes]
    groups = chain_groups(donors, others, hyds)
    s = TH.system(G, decoys[:3] + frames + decoys[3:], decoy_boxes[:3] + boxes + decoy_boxes[3:], groups)
    chains = [G.HBondChain("A0", "D0", "H"), G.HBondChain("A1", "D1", "H"), G.HBondChain("E", "D2", "H")]
    pairs = [(0, 0), (0, 1), (2, 1), (1, 1), (2, 2)]
    an = G.HBondAnalysis(s, chains, pairs, dmax, amin, bonds)
    nb = R.bonded(bonds, n)
    rchains = [R.resolve_chain(groups[a], groups[d], groups["H"], nb) for a, d in (("A0", "D0"), ("A1", "D1"), ("E", "D2"))]
    res = an.batch(3, 7)
    assert (res[6] == 0).all()
    counts = []
    for f in range(7):
        want = R.analyze(frames[f], boxes[f], rchains, pairs, dmax, amin)
        common = 0
        for p, key in enumerate(pairs):
            common += TH.compare(TH.frame_bonds(res, len(pairs), f, p), want[key], dmax, amin, dtol=1e-6 if not boxes[f][3:].any() else 2e-6)
        assert common > 20, f
        counts.append(common)
        one = an.batch(3 + f, 1)                                          # the slot alone: the same values in the same order
        assert (one[6] == 0).all()
        a, b = int(res[5][f * len(pairs)]), int(res[5][(f + 1) * len(pairs)])
        for k in range(5):
            assert one[k].tobytes() == res[k][a:b].tobytes(), (f, k)
        assert np.array_equal(one[5].astype(np.int64) + a, res[5][f * len(pairs): (f + 1) * len(pairs) + 1].astype(np.int64))
    for k, slot in enumerate((0, 1, 2, 10, 11)):                          # the decoys would have given other bonds
        one = an.batch(slot, 1)
        assert (one[6] == 0).all() and all(one[0].tobytes() != res[0][int(res[5][f * 5]): int(res[5][f * 5 + 5])].tobytes() for f in range(7))
    s.close()


# ------------------------------------------------------------------ H: distances exactly on max_distance
UNIT = 64                                   # coordinates are multiples of 1/64 nm
BOX_U = (128, 160, 192)                     # the box [2.0, 2.5, 3.0] in those units
CUT_U = 20                                  # max_distance 0.3125 nm


def _signed_permutations(v):
    out = set()
    for p in set(itertools.permutations(v)):
        for sg in itertools.product((1, -1), repeat=3):
            out.add(tuple(c * g for c, g in zip(p, sg)))
    return sorted(out)


def threshold_frames():
    """frames of four donor-acceptor pairs each (atoms: donor, hydrogen, acceptor per pair), integer coordinates in 1/64 nm.
    A pair lives on one of 2 x 2 sites in y and z: intervals of 16 units, 80 apart in y (box 160) and 96 apart in z (box 192), so
    atoms of different pairs are at least 64 units = 1 nm apart over the periodic faces whatever their x.  A pair that is to cross
    a face has one partner on 1 and the other on L - (|c| - 1) along an axis of its separation c: along x where the separation
    has an x component, else along y or z, which fixes where the sites of that frame begin.
    -> (list of int64 [12, 3], list of the separation of every pair, number of pairs across a face)"""
    seps = [(s, True) for s in _signed_permutations((12, 16, 0)) for _ in range(5)]          # on the threshold: kept
    seps += [(s, False) for v in ((12, 16, 1), (13, 16, 0), (12, 15, 0)) for s in _signed_permutations(v)]
    rng = np.random.default_rng(64)
    order = rng.permutation(len(seps))
    assert len(seps) % 4 == 0
    frames, frame_seps, crossing = [], [], 0
    for f0 in range(0, len(order), 4):
        mine = sorted((seps[k] for k in order[f0:f0 + 4]), key=lambda s: s[0][0] != 0)   # those without an x component first
        start = [0, int(rng.integers(0, BOX_U[1])), int(rng.integers(0, BOX_U[2]))]
        cross = [True, mine[1][0][0] != 0, mine[1][0][0] == 0 and mine[2][0][0] != 0, False]   # half of them, where the site allows it
        c0 = mine[0][0]
        if c0[0] == 0:                                                    # no x component: the first site of the frame lies on a face
            ax = 1 if c0[1] else 2
            start[ax] = -(c0[ax] - 1) if c0[ax] > 0 else -15
        xyz = np.zeros((12, 3), np.int64)
        for k, (c, _) in enumerate(mine):
            low = [0, start[1] + 80 * (k & 1), start[2] + 96 * (k >> 1)]
            d = [0, 0, 0]
            for ax in (1, 2):
                d[ax] = low[ax] if c[ax] >= 0 else low[ax] + 16
            d[0] = int(rng.integers(0, BOX_U[0]))
            if cross[k] and c[0] != 0:
                d[0] = BOX_U[0] - (c[0] - 1) if c[0] > 0 else 1
            d = np.array(d, np.int64); a = d + np.array(c, np.int64)
            h = d + np.array([4 if c[0] <= 0 else -4, 0, 0])
            box = np.array(BOX_U, np.int64)
            d, h, a = d % box, h % box, a % box                           # into the cell ...
            if (d - a != -np.array(c)).any():
                crossing += 1
            shift = int(rng.integers(0, 16))                              # ... and a few of them out again by a whole box
            if shift < 3:
                a[shift] += box[shift] * (1 if k & 1 else -1)
            elif shift == 3:
                d[1] += box[1]; h[1] += box[1]
            xyz[3 * k: 3 * k + 3] = d, h, a
        frames.append(xyz); frame_seps.append(mine)
    return frames, frame_seps, crossing


def _min_image_d2(u, v):
    """squared distance of the nearest images of two integer positions"""
    d2 = 0
    for ax in range(3):
        L = BOX_U[ax]
        c = (int(v[ax]) - int(u[ax]) + L // 2) % L - L // 2
        d2 += c * c
    return d2


def test_distance_exactly_on_the_threshold(G):
    frames, seps, crossing = threshold_frames()
    nf = len(frames)
    n_thr = sum(on for mine in seps for _, on in mine)
    assert n_thr >= 100 and abs(2 * crossing - 4 * nf) <= 0.2 * 4 * nf, (n_thr, crossing, nf)      # half of the pairs across a face
    # the integer model: which donor sees which acceptor, and that nothing else comes near
    want, outside_box = [], 0
    for f, xyz in enumerate(frames):
        outside_box += int(((xyz < 0) | (xyz >= np.array(BOX_U))).any(1).sum())
        for i in range(4):
            for j in range(4):
                if i == j:
                    continue
                assert all(_min_image_d2(xyz[3 * i + p], xyz[3 * j + q]) >= UNIT * UNIT for p in range(3) for q in range(3)), (f, i, j)
            c = seps[f][i][0]
            d2 = _min_image_d2(xyz[3 * i], xyz[3 * i + 2])
            assert d2 == sum(x * x for x in c)
            if d2 <= CUT_U * CUT_U:
                want.append((f, 3 * i, 3 * i + 1, 3 * i + 2, d2))
    assert outside_box >= 20
    assert sum(d2 == CUT_U * CUT_U for *_, d2 in want) == n_thr
    assert {d2 for *_, d2 in want} == {400, 369} and len(want) == n_thr + 24
    b9 = ortho9([2.0, 2.5, 3.0])
    pos = [(xyz.astype(np.float64) / UNIT).astype(np.float32) for xyz in frames]
    assert all((p.astype(np.float64) * UNIT == xyz).all() for p, xyz in zip(pos, frames))
    s = TH.system(G, pos, [b9] * nf, {"A": [2, 5, 8, 11], "D": [0, 3, 6, 9], "H": [1, 4, 7, 10]})
    an = G.HBondAnalysis(s, [G.HBondChain("A", "D", "H")], [(0, 0)], CUT_U / UNIT, 0.0, np.array([[0, 1], [3, 4], [6, 7], [9, 10]]))
    res = an.batch(0, nf)
    assert (res[6] == 0).all()
    got = [(f,) + b[:3] + (b[3],) for f in range(nf) for b in TH.frame_bonds(res, 1, f, 0)]
    assert [g[:4] for g in got] == [w[:4] for w in want]                  # the expected set exactly, in the order of the report
    for g, w in zip(got, want):
        assert np.float32(g[4]) == np.sqrt(np.float32(w[4] / (UNIT * UNIT))), (g, w)
        if w[4] == CUT_U * CUT_U:
            assert np.float32(g[4]) == np.float32(0.3125)
    s.close()

"""Hydrogen bonds on resident frames (gr_hbond_plan_create / gr_hbond_batch, groan_rs_amd.HBondAnalysis) against the reference's
pins and against the CPU restatement tests/hbond_ref.py (src/system/hbonds.rs:111-373).

Sets of (donor, hydrogen, acceptor) must be identical except for bonds within 2e-6 nm of max_distance or 1e-3 deg of min_angle
(the two sides may round them across the threshold); distances agree within 1e-6 nm (the same f32 expression), angles within
1e-3 deg, and the order of the bonds both sides report is the same."""
import ctypes as C
import os

import numpy as np
import pytest

import hbond_pins as P
import hbond_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.fixture(scope="module")
def full():
    return np.load(os.path.join(GOLD, "aa_full.npz"))


@pytest.fixture(scope="module")
def pep():
    return np.load(os.path.join(GOLD, "aa_peptide.npz"))


@pytest.fixture(scope="module")
def topo():
    return np.load(os.path.join(GOLD, "aa_hbond_topology.npz"))


def system(G, frames, boxes, groups):
    s = G.System(frames[0].shape[0], n_slots=len(frames), device=0)
    for f, (x, b) in enumerate(zip(frames, boxes)):
        s.set_frame(x, b, slot=f)
    for name, idx in groups.items():
        s.group_create_from_indices(name, [int(i) for i in idx])
    return s


def frame_bonds(res, n_pairs, f, p):
    """bonds of frame f, pair p of a batch result as a list of tuples"""
    a, b = int(res[5][f * n_pairs + p]), int(res[5][f * n_pairs + p + 1])
    return list(zip(res[0][a:b].tolist(), res[1][a:b].tolist(), res[2][a:b].tolist(), res[3][a:b].tolist(), res[4][a:b].tolist()))


def _keyed(bonds):
    """(donor, hydrogen, acceptor, k): the k-th occurrence -- a pair of two chains that share donors and acceptors meets a bond
    in both of its segments"""
    seen, out = {}, []
    for b in bonds:
        key = (int(b[0]), int(b[1]), int(b[2]))
        seen[key] = seen.get(key, -1) + 1
        out.append((key + (seen[key],), b))
    return out


def compare(got, want, dmax, amin, dtol=1e-6, atol=1e-3):
    gk, wk = _keyed(got), _keyed(want)
    g, w = dict(gk), dict(wk)
    for key in set(g) ^ set(w):                                       # only threshold bonds may differ
        b = g.get(key, w.get(key))
        assert abs(float(b[3]) - dmax) <= 2e-6 or abs(float(b[4]) - amin) <= 1e-3, (key, b)
    common = set(g) & set(w)
    assert [k for k, _ in gk if k in common] == [k for k, _ in wk if k in common]
    for k in common:
        assert abs(g[k][3] - float(w[k][3])) <= dtol and abs(g[k][4] - float(w[k][4])) <= atol, (k, g[k], w[k])
    return len(common)


# ---------------------------------------------------------------- the reference's systems
def test_water_frames_0_and_20(G, full):
    ow, hw, bonds = R.water_topology(full["atomname"])
    s = system(G, list(full["frames"]), list(full["boxes9"]), {"OW": ow, "HW": hw})
    an = G.HBondAnalysis(s, [G.HBondChain("OW", "OW", "HW")], [(0, 0)], 0.3, 150.0, bonds)
    res = an.batch(0, 2)
    assert (res[6] == 0).all()
    off = res[5].astype(np.int64)
    for k in range(2):
        frame = int(full["frame_index"][k])
        got = frame_bonds(res, 1, k, 0)
        assert len(got) == P.WATER_COUNTS[frame]
        assert R.close(got[0], P.WATER_FIRST_LAST[2 * frame]) and R.close(got[-1], P.WATER_FIRST_LAST[2 * frame + 1]), (got[0], got[-1])
        if frame == 20:
            hit = [b for b in got if b[:3] == (24613, 24614, 30592)]
            assert len(hit) == 1 and hit[0][4] == 180.0
        chain = R.resolve_chain(ow, ow, hw, R.bonded(bonds, full["frames"].shape[1]))
        compare(got, R.analyze(full["frames"][k], full["boxes9"][k], [chain], [(0, 0)], 0.3, 150.0)[(0, 0)], 0.3, 150.0)
    offs, st, total = an.count(0, 2)                                # count-only mode: NULL buffers
    assert np.array_equal(offs, res[5]) and total == off[-1] == 4675 + 4644 and (st == 0).all()
    m = an.analyze(s)                                               # FrameAnalyze form: the HBondMap of the current slot
    assert list(m) == [(0, 0)] and len(m[(0, 0)]) == 4675 and m[(0, 0)].dtype == G.HBOND_DTYPE
    s.close()


def _protein(G, pep, topo):
    don, hyd = R.protein_groups(topo["peptide_element"])
    s = system(G, list(pep["traj_peptide"]), list(pep["traj_boxes9"]), {"NO": don, "H": hyd})
    return s, G.HBondAnalysis(s, [G.HBondChain("NO", "NO", "H")], [(0, 0)], 0.3, 150.0, topo["peptide_bonds"])


def test_protein_trajectory_one_batch_and_frame_by_frame(G, pep, topo):
    s, an = _protein(G, pep, topo)
    nf = pep["traj_peptide"].shape[0]
    res = an.batch(0, nf)
    got = [b for f in range(nf) for b in frame_bonds(res, 1, f, 0)]
    assert len(got) == 181
    for g, w in zip(got, P.PROTEIN_TRAJ):
        assert R.close(g, w), (g, w)
    for f in range(nf):                                             # n_frames = 1: identical bits
        one = an.batch(f, 1)
        a, b = int(res[5][f]), int(res[5][f + 1])
        for k in range(5):
            assert one[k].tobytes() == res[k][a:b].tobytes(), (f, k)
    s.close()


def test_trajreader_hbonds_analyze(G, pep, topo):
    don, hyd = R.protein_groups(topo["peptide_element"])
    s = system(G, [pep["traj_peptide"][0]], [pep["traj_boxes9"][0]], {"NO": don, "H": hyd})
    frames = [(pep["traj_peptide"][f], pep["traj_boxes9"][f]) for f in range(pep["traj_peptide"].shape[0])]
    got = []
    for _, m in G.TrajReader(s, frames).hbonds_analyze([G.HBondChain("NO", "NO", "H")], [(0, 0)], 0.3, 150.0, topo["peptide_bonds"]):
        got += [tuple(r) for r in m[(0, 0)].tolist()]
    assert len(got) == 181 and all(R.close(g, w) for g, w in zip(got, P.PROTEIN_TRAJ))
    s.close()


def test_protein_water_gro(G, pep, topo, full):
    ow, hw, wb = R.water_topology(full["atomname"])
    don, hyd = R.protein_groups(topo["peptide_element"])
    bonds = np.concatenate([topo["peptide_bonds"].astype(np.int64), wb])
    s = system(G, [pep["pos"]], [pep["box9"]], {"NO": don, "OW": ow, "H": np.concatenate([hyd, hw])})
    an = G.HBondAnalysis(s, [G.HBondChain("NO", "NO", "H"), G.HBondChain("OW", "OW", "H")], [(0, 0), (0, 1)], 0.3, 150.0, bonds)
    m = an.analyze(s)
    assert list(m) == [(0, 0), (0, 1)]
    for key, want in (((0, 0), P.PROTEIN_PROTEIN_GRO), ((0, 1), P.PROTEIN_WATER_GRO)):
        got = [tuple(r) for r in m[key].tolist()]
        assert len(got) == len(want) and all(R.close(g, w) for g, w in zip(got, want)), (key, got)
    s.close()


# ---------------------------------------------------------------- seeded systems against the restatement
def seeded(seed, box, n_don=300, n_other=400, spread=(-0.2, 1.2), max_h=3):
    """donors with 1-max_h hydrogens at 0.1 nm, acceptor-only heavy atoms; some atoms outside the box.  Positions in lattice
    coordinates of `box` (gro box9).  Returns pos, donors, others, hydrogens, bonds"""
    rng = np.random.default_rng(seed)
    L = np.array([[box[0], 0, 0], [box[5], box[1], 0], [box[7], box[8], box[2]]], np.float64)
    pos, donors, hyds, bonds = [], [], [], []
    for _ in range(n_don):
        d = len(pos); donors.append(d)
        p = rng.uniform(*spread, 3) @ L
        pos.append(p)
        for _ in range(rng.integers(1, max_h + 1)):
            v = rng.normal(size=3); v *= 0.1 / np.linalg.norm(v)
            hyds.append(len(pos)); bonds.append((d, len(pos))); pos.append(p + v)
    pos[hyds[0]] = pos[donors[0]].copy()                             # a hydrogen sitting on its donor
    others = list(range(len(pos), len(pos) + n_other))
    pos += list(rng.uniform(*spread, (n_other, 3)) @ L)
    return np.asarray(pos, np.float32), np.array(donors), np.array(others), np.array(hyds), np.array(bonds)


def multi_chain(G, pos, box, donors, others, hyds, bonds, dmax, amin, strict=False):
    heavy = np.sort(np.concatenate([donors, others]))
    n = len(donors)
    d0, d1 = donors[: 3 * n // 5], donors[2 * n // 5:]                # overlapping donor groups
    groups = {"A0": np.union1d(heavy[::2], hyds[::7]),                # hydrogens as acceptors
              "D0": np.union1d(d0, others[:50]),                      # acceptor-only atoms among the donors: dropped
              "A1": np.union1d(heavy[1::2], d1), "D1": d1, "H": hyds, "E": [], "D2": d0[:40]}
    s = system(G, [pos], [box], groups)
    if strict:
        s.set_strict_orthogonal(True)
    chains = [G.HBondChain("A0", "D0", "H"), G.HBondChain("A1", "D1", "H"), G.HBondChain("E", "D2", "H")]
    pairs = [(0, 0), (0, 1), (2, 1), (1, 1), (2, 2)]
    an = G.HBondAnalysis(s, chains, pairs, dmax, amin, bonds)
    nb = R.bonded(bonds, pos.shape[0])
    rchains = [R.resolve_chain(groups[a], groups[d], groups["H"], nb) for a, d in (("A0", "D0"), ("A1", "D1"), ("E", "D2"))]
    return s, an, pairs, rchains


@pytest.mark.parametrize("dmax, amin", [(0.1, 150.0), (0.2, 130.0), (0.3, 160.0), (0.5, 160.0)])
@pytest.mark.parametrize("box", [[3.0, 3.2, 3.4], [0.9, 1.5, 4.0], [0.45, 0.8, 1.7]])   # >= 3, 2 and 1 cells per axis
def test_differential_seeded(G, dmax, amin, box):
    b9 = np.array(box + [0.0] * 6, np.float32)
    pos, donors, others, hyds, bonds = seeded(int(dmax * 10 + box[0] * 100), b9)
    s, an, pairs, rchains = multi_chain(G, pos, b9, donors, others, hyds, bonds, dmax, amin)
    res = an.batch(0, 1)
    assert (res[6] == 0).all()
    want = R.analyze(pos, b9, rchains, pairs, dmax, amin)
    n = 0
    for p, key in enumerate(pairs):
        n += compare(frame_bonds(res, len(pairs), 0, p), want[key], dmax, amin)
    assert n > 0
    s.close()


@pytest.mark.parametrize("lengths, angles", [([3.2, 3.4, 3.0], [70.0, 80.0, 65.0]), ([3.5, 3.5, 3.5], [60.0, 60.0, 90.0])])
def test_triclinic(G, lengths, angles):
    b9 = O.box_from_lengths_angles(lengths, angles)
    pos, donors, others, hyds, bonds = seeded(7, b9, n_don=400, n_other=600)
    dmax, amin = 0.35, 140.0
    s, an, pairs, rchains = multi_chain(G, pos, b9, donors, others, hyds, bonds, dmax, amin)
    res = an.batch(0, 1)
    assert (res[6] == 0).all()
    want = R.analyze(pos, b9, rchains, pairs, dmax, amin)
    L = np.array([[b9[0], 0, 0], [b9[5], b9[1], 0], [b9[7], b9[8], b9[2]]], np.float64)
    images = np.array([(i, j, k) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)], np.float64) @ L
    n = 0
    for p, key in enumerate(pairs):
        got = frame_bonds(res, len(pairs), 0, p)
        n += compare(got, want[key], dmax, amin, dtol=2e-6)
        for d, h, a, dist, ang in got:                              # distances against an fp64 image search
            v = pos[a].astype(np.float64) - pos[d].astype(np.float64)
            assert abs(np.sqrt(((v[None, :] + images) ** 2).sum(1).min()) - dist) <= 1e-5
    assert n > 20
    s.close()
    s, an, pairs, _ = multi_chain(G, pos, b9, donors, others, hyds, bonds, dmax, amin, strict=True)
    with pytest.raises(G.HBondError) as e:
        an.batch(0, 1)
    assert e.value.variant == "InvalidSimBox" and e.value.status == G._lib.E_NOT_ORTHOGONAL
    s.close()


# ---------------------------------------------------------------- errors
def test_plan_errors(G, pep, topo):
    don, hyd = R.protein_groups(topo["peptide_element"])
    s = system(G, [pep["traj_peptide"][0]], [pep["traj_boxes9"][0]], {"NO1": don[don < 150], "NO2": don[don >= 150], "H": hyd,
                                                                      "C": np.nonzero(topo["peptide_element"] == b"C")[0], "E": []})
    b = topo["peptide_bonds"]
    two = [G.HBondChain("NO1", "NO1", "H"), G.HBondChain("NO2", "NO2", "H")]

    def err(chains, pairs, dmax=3.0, bonds=b):
        with pytest.raises(G.HBondError) as e:
            G.HBondAnalysis(s, chains, pairs, dmax, 150.0, bonds)
        return e.value.variant, e.value.detail

    assert err(two, [(0, 1), (0, 2)]) == ("NonexistentChain", 2)
    assert err(two, [(0, 1), (0, 0), (0, 1)]) == ("PairSpecifiedMultipleTimes", (0, 1))
    assert err(two, [(1, 0), (0, 0), (0, 1)]) == ("PairSpecifiedMultipleTimes", (0, 1))
    assert err(two, [(0, 0), (1, 0), (0, 0)]) == ("PairSpecifiedMultipleTimes", (0, 0))
    assert err(two, [(0, 0)]) == ("UnusedChain", None)
    assert err(two + [G.HBondChain("E", "E", "H")], [(0, 1), (2, 2)]) == ("EmptyChain", 2)   # no acceptors, no donor with a hydrogen
    assert err(two + [G.HBondChain("E", "NO1", "E")], [(0, 1), (2, 2)]) == ("EmptyChain", 2)  # donors, but none bonded to a hydrogen of the chain
    assert err(two, [(0, 1)], dmax=0.0) == ("CellGridError", "InvalidCellSize")
    assert err([G.HBondChain("NO1", "nope", "H")], [(0, 0)])[0] == "SelectError"
    v, d = err(two, [(0, 1)], bonds=np.array([[0, 1], [2, 363]]))
    assert v == "AtomError" and d.variant == "OutOfRange" and d.detail == 363
    G.HBondAnalysis(s, [G.HBondChain("E", "NO1", "H")], [(0, 0)], 0.3, 150.0, b)         # acceptors empty, donors present: fine
    s.close()


def raw_batch(G, an, s0, n, cap, buffers=True, fill=7):
    out = [np.full(max(cap, 1), fill, np.uint32) for _ in range(3)] + [np.full(max(cap, 1), fill, np.float32) for _ in range(2)]
    offs = np.zeros(n * len(an.pairs) + 1, np.uint64); st = np.zeros(n, np.int32); tot = C.c_uint64(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    r = an._lib.gr_hbond_batch(an._plan, s0, n, cap, *[ptr(a) if buffers else None for a in out], ptr(offs), C.byref(tot), ptr(st))
    return r, out, offs, st, int(tot.value)


def test_frames_with_errors_in_a_batch(G):
    b9 = np.array([3.0, 3.2, 3.4] + [0.0] * 6, np.float32)
    pos, donors, others, hyds, bonds = seeded(11, b9)
    dmax, amin = 0.3, 130.0
    s, an, pairs, rchains = multi_chain(G, pos, b9, donors, others, hyds, bonds, dmax, amin)
    s.close()
    nb = R.bonded(bonds, pos.shape[0])
    acc0 = rchains[0][0]
    lone = [h for h in hyds if h not in set(acc0) | set(rchains[1][0])]   # hydrogens that are no acceptor
    cand = R.analyze(pos, b9, rchains, pairs, dmax, -1.0)            # every acceptor in range becomes a bond
    with_acc = {b[0] for key in pairs for b in cand[key]}
    accs = set(acc0) | set(rchains[1][0])
    d_in = next(d for d, hs in rchains[0][1] if d in with_acc and hs[0] in lone)
    h_in = dict(rchains[0][1])[d_in][0]
    d_out = next(d for ch in rchains for d, hs in ch[1] if d not in with_acc and not set(hs) & accs)
    h_out = sorted(nb[d_out])[0]
    nan = np.float32(np.nan)
    frames, boxes, want = [], [], []

    def add(p, b, status, index=None):
        frames.append(p); boxes.append(b); want.append((status, index))
    add(pos, b9, 0)
    add(pos, None, G._lib.E_NO_BOX)
    p = pos.copy(); p[acc0[5]] = nan; p[acc0[9]] = nan; add(p, b9, G._lib.E_NO_POSITION, acc0[5])
    add(pos + np.float32(0.01), b9, 0)
    p = pos.copy(); p[d_in] = nan; add(p, b9, G._lib.E_NO_POSITION, d_in if d_in not in acc0 else None)
    p = pos.copy(); p[h_in] = nan; add(p, b9, G._lib.E_NO_POSITION, h_in)
    p = pos.copy(); p[h_out] = nan; add(p, b9, 0)                 # a hydrogen without position on a donor with no acceptor in range
    add(pos - np.float32(0.02), b9, 0)
    groups = {"A0": np.union1d(np.sort(np.concatenate([donors, others]))[::2], hyds[::7])}
    heavy = np.sort(np.concatenate([donors, others])); n = len(donors); d0, d1 = donors[: 3 * n // 5], donors[2 * n // 5:]
    groups.update({"D0": np.union1d(d0, others[:50]), "A1": np.union1d(heavy[1::2], d1), "D1": d1, "H": hyds, "E": [], "D2": d0[:40]})
    s = system(G, frames, boxes, groups)
    chains = [G.HBondChain("A0", "D0", "H"), G.HBondChain("A1", "D1", "H"), G.HBondChain("E", "D2", "H")]
    an = G.HBondAnalysis(s, chains, pairs, dmax, amin, bonds)
    r, out, offs, st, tot = raw_batch(G, an, 0, len(frames), 10 ** 6)
    assert r == G._lib.E_NO_BOX and st.tolist() == [w[0] for w in want], st
    npairs = len(pairs)
    for f, (status, index) in enumerate(want):
        seg = offs[f * npairs: (f + 1) * npairs + 1].astype(np.int64)
        r1, out1, offs1, st1, tot1 = raw_batch(G, an, f, 1, 10 ** 6)
        assert r1 == status and st1[0] == status
        if status != 0:
            assert seg[0] == seg[-1] and tot1 == 0                   # a failed frame has empty segments
            if status == G._lib.E_NO_POSITION:
                try:
                    R.analyze(frames[f], b9, rchains, pairs, dmax, amin)
                    raise AssertionError("the restatement found no missing position")
                except R.HBondRefError as e:
                    assert int(an._lib.gr_last_error_index(s._ctx)) == e.payload
                    if index is not None:
                        assert e.payload == index
            continue
        a, b = int(seg[0]), int(seg[-1])
        assert tot1 == b - a
        for k in range(5):                                          # good frames: the bits of a single-frame call
            assert out1[k][:tot1].tobytes() == out[k][a:b].tobytes(), (f, k)
        want_f = R.analyze(frames[f], b9, rchains, pairs, dmax, amin)
        for p, key in enumerate(pairs):
            x, y = int(offs[f * npairs + p]), int(offs[f * npairs + p + 1])
            got = list(zip(out[0][x:y].tolist(), out[1][x:y].tolist(), out[2][x:y].tolist(), out[3][x:y].tolist(), out[4][x:y].tolist()))
            compare(got, want_f[key], dmax, amin)
    s.close()


def test_capacity(G):
    b9 = np.array([3.0, 3.2, 3.4] + [0.0] * 6, np.float32)
    pos, donors, others, hyds, bonds = seeded(5, b9)
    s, an, pairs, _ = multi_chain(G, pos, b9, donors, others, hyds, bonds, 0.35, 120.0)
    s.set_frame(pos + np.float32(0.05), b9, slot=0)
    r, out, offs, st, tot = raw_batch(G, an, 0, 1, 0, buffers=False)
    assert r == 0 and tot > 50 and int(offs[-1]) == tot
    r, out, offs2, st, tot2 = raw_batch(G, an, 0, 1, tot - 1)
    assert r == 0 and tot2 == tot and np.array_equal(offs2, offs)
    assert all((a == 7).all() for a in out)                          # nothing written
    r, out, offs3, st, tot3 = raw_batch(G, an, 0, 1, tot)
    assert r == 0 and tot3 == tot and np.array_equal(offs3, offs) and not (out[2][:tot] == 7).all()
    res = an.batch(0, 1)
    for k in range(5):
        assert res[k].tobytes() == out[k][:tot].tobytes()
    s.close()


# ---------------------------------------------------------------- scale
def water_box(n_mol, seed, density=33.4):
    """n_mol random waters: O uniform, O-H 0.1 nm, HOH 104.5 deg, random orientations; atoms O, H1, H2 per molecule"""
    rng = np.random.default_rng(seed)
    L = (n_mol / density) ** (1.0 / 3.0)
    o = rng.uniform(0, L, (n_mol, 3))
    u = rng.normal(size=(n_mol, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    w = rng.normal(size=(n_mol, 3)); w -= (w * u).sum(1)[:, None] * u; w /= np.linalg.norm(w, axis=1)[:, None]
    half = np.deg2rad(104.5) / 2
    h1 = o + 0.1 * (np.cos(half) * u + np.sin(half) * w)
    h2 = o + 0.1 * (np.cos(half) * u - np.sin(half) * w)
    pos = np.stack([o, h1, h2], 1).reshape(-1, 3).astype(np.float32)
    return pos, np.array([L, L, L] + [0.0] * 6, np.float32)


def test_scale_million_atoms(G):
    n_mol, nf = 333334, 8
    frames = []
    for f in range(nf):
        pos, b9 = water_box(n_mol, 100 + f)
        frames.append(pos)
    ow = np.arange(0, 3 * n_mol, 3); hw = np.sort(np.concatenate([ow + 1, ow + 2]))
    bonds = np.concatenate([np.stack([ow, ow + 1], 1), np.stack([ow, ow + 2], 1)])
    s = G.System(3 * n_mol, n_slots=nf, device=0)
    for f in range(nf):
        s.set_frame(frames[f], b9, slot=f)
    s.group_create_from_indices("OW", ow.tolist())
    s.group_create_from_indices("HW", hw.tolist())
    an = G.HBondAnalysis(s, [G.HBondChain("OW", "OW", "HW")], [(0, 0)], 0.3, 150.0, bonds)
    res = an.batch(0, nf)
    assert (res[6] == 0).all() and int(res[5][-1]) > nf * 1000
    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(ow, 500, replace=False))
    for f in (0, nf - 1):
        got = [b for b in frame_bonds(res, 1, f, 0) if b[0] in set(sample.tolist())]
        donors = [(int(d), [int(d) + 1, int(d) + 2]) for d in sample]
        want = R.analyze_single(frames[f], b9, ow.tolist(), donors, 0.3, 150.0)
        assert compare(got, want, 0.3, 150.0) > 20
    s.close()

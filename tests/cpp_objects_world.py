"""The world and the call script that tests/cpp/test_objects.cpp and tests/test_gpu_cpp_objects.py share, and the margins that let every
case of them be compared (tests/test_cpp_objects_world.py asserts those on the CPU).

The world: 100 three-atom water-like molecules (O, H, H with their two bonds), 96 of them a droplet in the middle of an orthorhombic
box, 4 outside the box beside it (so that a wrap moves something), in 10 slots.  Slot NAN_SLOT has one atom (NAN_ATOM, a hydrogen that
lies in the groups rng, lst, hyd and hydA) without position; slot NOBOX_SLOT has no box.  The constants below ARE the call script: the
C++ program has the same numbers in its calls.

No atom may sit on a decision point, else a result could legitimately differ between two correct implementations and a case would have
to be left out of a comparison.  `violations` finds the atoms that do, with the references alone: a criterion is evaluated by its
reference with the threshold moved to either side by the margin, and whatever changes sides lies within the margin of it.  `build`
redraws the thermal noise of the molecules found with three times the margins the tests assert, until nothing is found."""
import os

import numpy as np

import gridmap_ref
import hbond_ref
import oracle_lib as O
import region_ref
import segments_ref

F = np.float32
SEED = 20261020
N_MOL, N, NS = 100, 300, 10
NAN_SLOT, NOBOX_SLOT, NAN_ATOM = 4, 6, 23
MARGIN_NM, MARGIN_DEG = 1e-4, 0.1

OXY = np.arange(0, N, 3)
HYD = np.sort(np.concatenate([OXY + 1, OXY + 2]))
GROUPS = {"rng": np.arange(5, 161), "lst": np.arange(2, 288, 7), "hyd": HYD, "oxy": OXY,
          "oxyA": OXY[:50], "hydA": HYD[:100], "oxyB": OXY[50:], "hydB": HYD[100:]}
RANGES = {"rng": (5, 160)}                                  # made from a range; every other group from its index list
BONDS = np.concatenate([np.stack([OXY, OXY + 1], 1), np.stack([OXY, OXY + 2], 1)]).astype(np.uint64)
LABELS = ((np.arange(N) // 3) // 2).astype(np.uint64)      # a "residue" is two molecules

# -- hydrogen bonds: chains (acceptors, donors, hydrogens), pairs of chains
CHAINS = [("oxyA", "oxyA", "hydA"), ("oxyB", "oxyB", "hydB")]
HB_PAIRS = [(0, 0), (0, 1)]
HB_DIST, HB_ANGLE = 0.31, 135.0
HB_DIST_NONE = 0.15                                         # below every O-O distance: a plan that finds nothing
# -- grid maps
MAP1 = ((0.5, 2.5), (0.4, 2.8), (0.25, 0.3))
MAP2_TILE, MAP2_SLOT = (0.4, 0.5), 1
GM_OFFSET_Z = 0.7
GM_POINTS = np.array([[1.0, 1.0], [2.6, 2.9], [0.0, 1.0], [1.0, 9.0], [0.375, 0.25], [0.37, 1.0], [-1.0, -1.0]], F)   # (0.375, 0.25): the lower edge
# -- segments
SEG_LISTS = [np.arange(0, 9), np.arange(6, 11), np.array([23, 24, 25, 50]), np.arange(100, 140)]
# -- regions
SHAPES_A = [{"kind": "sphere", "position": [1.5, 1.6, 1.4], "radius": 0.55},
            {"kind": "cylinder", "position": [1.5, 1.6, 0.9], "radius": 0.5, "height": 1.0, "orientation": "z"}]
SHAPES_EMPTY = [{"kind": "sphere", "position": [0.3, 0.3, 0.3], "radius": 0.1}]
ANCHOR_ONE = np.array([[0.05, -0.03, 0.02]], F)
ANCHORS_3 = np.array([[0.1, 0.0, -0.05], [-0.07, 0.04, 0.0], [0.0, -0.11, 0.06]], F)
# -- contacts
CT_CUT, CT_NBINS, CT_CUT_NONE, CT_MAX_PAIRS = 0.25, 13, 0.05, 5

E_NO_BOX, E_NO_POSITION, E_GROUP_NOT_FOUND, E_INVALID_ARG = 1, 6, 8, 10


def _molecule(rng):
    """O at the origin, two H at 0.1 nm with 104.5 degrees between them, in a random orientation"""
    u = rng.standard_normal(3); u /= np.linalg.norm(u)
    v = np.cross(u, rng.standard_normal(3)); v /= np.linalg.norm(v)
    t = np.deg2rad(104.5)
    return np.stack([np.zeros(3), 0.1 * u, 0.1 * (np.cos(t) * u + np.sin(t) * v)])


def _noise(rng):
    return np.clip(0.012 * rng.standard_normal((3, 3)), -0.03, 0.03)


def boxes():
    return [None if f == NOBOX_SLOT else np.array([3.0 + 0.01 * f, 3.2 + 0.01 * f, 2.8 + 0.01 * f, 0, 0, 0, 0, 0, 0], F) for f in range(NS)]


def _lists_of_labels(labels, idx):
    out = {}
    for a in idx:
        out.setdefault(int(labels[a]), []).append(int(a))
    return [np.array(v) for v in out.values()]               # dicts keep the order of first appearance


def segment_lists():
    """the atom lists of the three Segments objects: from_lists, from_labels(LABELS, 'rng'), from_molecules"""
    return {"seg1": [np.asarray(a) for a in SEG_LISTS], "seg2": _lists_of_labels(LABELS, GROUPS["rng"]),
            "seg3": [np.arange(3 * m, 3 * m + 3) for m in range(N_MOL)]}


def resolved_chains():
    nb = hbond_ref.bonded(BONDS, N)
    return [hbond_ref.resolve_chain(GROUPS[a], GROUPS[d], GROUPS[h], nb) for a, d, h in CHAINS]


def hbonds_of(pos, box, dist, angle):
    """hbond_ref.analyze of one frame -> ({pair: bonds}, status)"""
    if box is None:
        return {p: [] for p in HB_PAIRS}, E_NO_BOX
    try:
        return hbond_ref.analyze(pos, box, resolved_chains(), HB_PAIRS, dist, angle), 0
    except hbond_ref.HBondRefError:
        return {p: [] for p in HB_PAIRS}, E_NO_POSITION


def map2_spans(bx):
    return (0.0, float(bx[MAP2_SLOT][0])), (0.0, float(bx[MAP2_SLOT][1]))


def region_calls():
    """(name, shapes, group, first slot, frames, anchors) of every Region::select call, in call order"""
    return [("a_all", SHAPES_A, "hyd", 0, NS, None), ("a_one", SHAPES_A, "rng", 2, 1, ANCHOR_ONE), ("a_anch", SHAPES_A, "hyd", 7, 3, ANCHORS_3),
            ("empty", SHAPES_EMPTY, None, 0, 3, None)]


def contact_calls():
    return [("rng", "hyd", CT_CUT), ("oxy", "oxy", CT_CUT_NONE)]


def violations(frames, bx, m_nm, m_deg, slots=range(NS)):
    """{(slot, atom)}: atoms within m_nm (m_deg for the hydrogen-bond angle) of a decision point of any call of the script"""
    bad = set()
    every = np.arange(N)
    for f in slots:
        pos, box = frames[f], bx[f]
        if box is not None:
            # the Contacts cut-offs and the hydrogen-bond distances: the pairs that change sides between cutoff -+ m
            for g1, g2, cut in contact_calls() + [("oxy", "oxy", HB_DIST), ("oxy", "oxy", HB_DIST_NONE)]:
                ok1, ok2 = [a for a in GROUPS[g1] if not np.isnan(pos[a, 0])], [a for a in GROUPS[g2] if not np.isnan(pos[a, 0])]
                lo, hi = O.pairs_within(pos, ok1, ok2, box, cut - m_nm), O.pairs_within(pos, ok1, ok2, box, cut + m_nm)
                for i, j in set(zip(hi[0].tolist(), hi[1].tolist())) - set(zip(lo[0].tolist(), lo[1].tolist())):
                    bad.add((f, i)); bad.add((f, j))
            # the hydrogen-bond angle
            p = np.where(np.isnan(pos), F(0), pos)               # (the frame without NAN_ATOM's position: its bonds are judged like all others)
            lo, hi = hbonds_of(p, box, HB_DIST, HB_ANGLE + m_deg)[0], hbonds_of(p, box, HB_DIST, HB_ANGLE - m_deg)[0]
            for key in HB_PAIRS:
                for b in set(x[:3] for x in hi[key]) - set(x[:3] for x in lo[key]):
                    bad.add((f, b[1]))
            # the shapes: every point of a surface moves by 2 m / sqrt(3) > m or more along its normal when the shape moves by 2 m along
            # the axis its normal leans to most, so an atom within m of a surface changes sides for one of the three axes
            for _, specs, group, first, n, anchors in region_calls():
                if not first <= f < first + n:
                    continue
                idx = every if group is None else GROUPS[group]
                sp = specs if anchors is None else region_ref.moved(specs, anchors[f - first])
                for axis in range(3):
                    d = np.zeros(3, F); d[axis] = 2 * m_nm
                    a, b = (O.group_from_geometries(pos, idx, box, region_ref.moved(sp, s * d)) for s in (1, -1))
                    bad.update((f, int(i)) for i in set(a.tolist()) ^ set(b.tolist()))
        # the tile edges: the index with the map's origin moved by -+ m
        for (sx, sy, td), idx, wrap in (((MAP1), every, False), ((*map2_spans(bx), MAP2_TILE), GROUPS["hyd"], True)):
            if wrap and box is None:
                continue
            p = pos[idx]
            keep = ~np.isnan(p[:, 0])
            if wrap:
                p = p.copy(); p[keep] = O.wrap_atoms(p[keep], np.arange(int(keep.sum())), box)
            for c, (s0, t) in enumerate(((sx[0], td[0]), (sy[0], td[1]))):
                moved = gridmap_ref.coord2index(p[:, c], s0 - m_nm, t) != gridmap_ref.coord2index(p[:, c], s0 + m_nm, t)
                bad.update((f, int(a)) for a in idx[moved & keep])
    return bad


def seam_flags(frames, bx, masses):
    """how many periodic centres of the script's segments lie within segments_ref.SEAM of a cell face (wanted: none)"""
    n = 0
    for lists in segment_lists().values():
        ref = segments_ref._reference(frames, bx, masses, lists)
        for key, (cen, errs, flags) in ref.items():
            if flags is not None:
                ok = np.array([[e is None for e in (errs[f] or [1] * len(lists))] for f in range(NS)])
                n += int((flags.any(axis=2) & ok).sum())
    return n


def build(seed=SEED):
    """-> dict(frames [NS] of float32 [N, 3], boxes [NS] of box9 or None, masses float32 [N])"""
    rng = np.random.default_rng(seed)
    site = np.array([[0.9 + 0.30 * ix, 0.96 + 0.32 * iy, 0.875 + 0.35 * iz] for ix in range(5) for iy in range(5) for iz in range(4)])
    site[96:] = [[-0.25, 0.5 + 0.5 * k, 1.0] for k in range(4)]               # four molecules outside the box
    base = np.stack([site[m] + rng.uniform(-0.03, 0.03, 3) + _molecule(rng) for m in range(N_MOL)])      # [N_MOL, 3, 3]
    noise = np.stack([[_noise(rng) for _ in range(N_MOL)] for _ in range(NS)])                           # [NS, N_MOL, 3, 3]
    masses = (np.tile([15.999, 1.008, 1.008], N_MOL) * (1.0 + 0.01 * rng.random(N))).astype(F)
    bx = boxes()

    def frames_of():
        fr = [(base + noise[f]).reshape(N, 3).astype(F) for f in range(NS)]
        fr[NAN_SLOT][NAN_ATOM] = np.nan
        return fr

    dirty = list(range(NS))
    for _ in range(200):
        fr = frames_of()
        bad = violations(fr, bx, 3 * MARGIN_NM, 3 * MARGIN_DEG, dirty)
        if not bad:
            break
        for f, m in sorted(set((f, a // 3) for f, a in bad)):
            noise[f, m] = _noise(rng)
        dirty = sorted(set(f for f, _ in bad))
    else:
        raise AssertionError("no world without an atom on a decision point")
    return {"frames": fr, "boxes": bx, "masses": masses}


def write(world, path):
    """the fixture files of the C++ program, raw little-endian"""
    np.stack(world["frames"]).astype("<f4").tofile(os.path.join(path, "frames.f32"))
    np.stack([np.full(9, np.nan, F) if b is None else b for b in world["boxes"]]).astype("<f4").tofile(os.path.join(path, "boxes.f32"))
    world["masses"].astype("<f4").tofile(os.path.join(path, "masses.f32"))
    BONDS.astype("<u8").tofile(os.path.join(path, "bonds.u64"))
    LABELS.astype("<u8").tofile(os.path.join(path, "labels.u64"))
    np.array([N, NS, NAN_SLOT, NOBOX_SLOT, NAN_ATOM], "<u8").tofile(os.path.join(path, "meta.u64"))
    for name, idx in GROUPS.items():
        if name not in RANGES:
            idx.astype("<u8").tofile(os.path.join(path, "group_%s.u64" % name))

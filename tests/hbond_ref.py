"""CPU restatement of the hydrogen-bond analysis (src/system/hbonds.rs:111-373) built from the oracle's primitives.

The pruning is an all-pairs cut-off search (oracle pairs_within: acceptor.distance(donor) <= max_distance, the donor itself
skipped), the angle is the reference's Vector3D::angle(..).to_degrees() in numpy float32 (left-to-right dot product and norms,
each operation rounded on its own) over the oracle's vector_to, with handle_nan (the oracle's distance).  Bonds come out by
segment, then donor (group order), then acceptor index, then hydrogen index -- the order the library reports.
"""
import numpy as np

import oracle_lib as O

DEG = np.float32(57.2957795130823208767981548141051703)


class HBondRefError(Exception):
    def __init__(self, variant, payload=None):
        super().__init__("%s(%r)" % (variant, payload))
        self.variant, self.payload = variant, payload


def bonded(bonds, n_atoms):
    """neighbour sets of a bond list (either order; a bond of an atom to itself is no bond)"""
    nb = [set() for _ in range(n_atoms)]
    for a, b in np.asarray(bonds, np.int64).reshape(-1, 2):
        if a != b:
            nb[a].add(int(b)); nb[b].add(int(a))
    return nb


def resolve_chain(acceptors, donors, hydrogens, nb):
    """HBondChainGroups::new: (acceptors, [(donor, [hydrogens in index order])]) or EmptyChain"""
    hs = set(int(h) for h in hydrogens)
    don = []
    for d in donors:
        h = sorted(x for x in nb[int(d)] if x in hs)
        if h:
            don.append((int(d), h))
    acc = [int(a) for a in acceptors]
    if not acc and not don:
        raise HBondRefError("EmptyChain")
    return acc, don


def check_pairs(pairs, n_chains):
    """HBondAnalysis::sanity_check_pairs"""
    seen, used = set(), set()
    for a, b in pairs:
        for ch in (a, b):
            if ch >= n_chains:
                raise HBondRefError("NonexistentChain", ch)
        if a != b:
            fresh = (a, b) not in seen and (b, a) not in seen
            seen.add((a, b)); seen.add((b, a))
        else:
            fresh = (a, b) not in seen
            seen.add((a, b))
        if not fresh:
            raise HBondRefError("PairSpecifiedMultipleTimes", (a, b))
        used.update((a, b))
    if len(used) != n_chains:
        raise HBondRefError("UnusedChain")


def angles(pos, box, d, hs, acc):
    """calc_angle for every (hydrogen in hs, acceptor in acc) of donor d: float32 [len(acc), len(hs)]"""
    n = len(acc) * len(hs)
    hd = np.zeros((n, 3), np.float32); ha = np.zeros((n, 3), np.float32)
    k = 0
    for a in acc:
        for h in hs:
            hd[k] = O.vector_to(pos[h], pos[d], box)
            ha[k] = O.vector_to(pos[h], pos[a], box)
            k += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = hd[:, 0] * ha[:, 0] + hd[:, 1] * ha[:, 1] + hd[:, 2] * ha[:, 2]
        lu = np.sqrt(hd[:, 0] * hd[:, 0] + hd[:, 1] * hd[:, 1] + hd[:, 2] * hd[:, 2])
        lv = np.sqrt(ha[:, 0] * ha[:, 0] + ha[:, 1] * ha[:, 1] + ha[:, 2] * ha[:, 2])
        ang = np.arccos(dot / (lu * lv)) * DEG
    k = 0
    for a in acc:
        for h in hs:
            if ang[k] != ang[k]:    # handle_nan
                ang[k] = 180.0 if O.distance(pos[h], pos[a], "xyz", box) < O.distance(pos[d], pos[a], "xyz", box) else 0.0
            k += 1
    return ang.astype(np.float32).reshape(len(acc), len(hs))


def analyze_single(pos, box, acc, donors, max_distance, min_angle):
    """-> list of (donor, hydrogen, acceptor, distance, angle); raises HBondRefError("NoPosition", index)"""
    out = []
    if not donors or not acc:
        for d, _ in donors:
            if np.isnan(pos[d][0]):
                raise HBondRefError("NoPosition", d)
        return out
    dlist = [d for d, _ in donors]
    ok = [d for d in dlist if not np.isnan(pos[d][0])]
    ii, jj, dd = O.pairs_within(pos, ok, acc, box, max_distance) if ok else (np.zeros(0), np.zeros(0), np.zeros(0))
    cand = {}
    for i, j, dist in zip(ii.tolist(), jj.tolist(), dd.tolist()):
        cand.setdefault(i, []).append((j, dist))
    for d, hs in donors:
        if np.isnan(pos[d][0]):
            raise HBondRefError("NoPosition", d)
        c = sorted(cand.get(d, []))
        if not c:
            continue
        for h in hs:
            if np.isnan(pos[h][0]):
                raise HBondRefError("NoPosition", h)
        ang = angles(pos, box, d, hs, [a for a, _ in c])
        for r, (a, dist) in enumerate(c):
            for q, h in enumerate(hs):
                if ang[r, q] >= np.float32(min_angle):
                    out.append((d, h, a, np.float32(dist), ang[r, q]))
    return out


def analyze(pos, box, chains, pairs, max_distance, min_angle):
    """HBondAnalysis::analyze for one frame.  chains = [(acceptors, donors)] as resolve_chain returns them.
    -> {(c1, c2): list of bonds}; raises HBondRefError("NoPosition", index) in the reference's order"""
    pos = np.asarray(pos, np.float32)
    for acc, _ in chains:                      # CellGrid::new_from_group for every chain first
        for a in acc:
            if np.isnan(pos[a][0]):
                raise HBondRefError("NoPosition", a)
    out = {}
    for a, b in pairs:
        if a == b:
            out[(a, b)] = analyze_single(pos, box, chains[a][0], chains[a][1], max_distance, min_angle)
        else:
            out[(a, b)] = (analyze_single(pos, box, chains[a][0], chains[b][1], max_distance, min_angle)
                           + analyze_single(pos, box, chains[b][0], chains[a][1], max_distance, min_angle))
    return out


# ---------------------------------------------------------------- the systems of the reference's tests
def water_topology(atomname):
    """OW / HW1 HW2 indices of aa_full.npz's names and the O-H bonds (every OW is followed by HW1 and HW2)"""
    names = np.asarray(atomname)
    ow = np.nonzero(names == b"OW")[0]
    assert (names[ow + 1] == b"HW1").all() and (names[ow + 2] == b"HW2").all()
    hw = np.sort(np.concatenate([ow + 1, ow + 2]))
    bonds = np.concatenate([np.stack([ow, ow + 1], 1), np.stack([ow, ow + 2], 1)])
    return ow, hw, bonds


def protein_groups(element):
    """'@protein and elsymbol N O' and the hydrogens of the peptide's element column"""
    el = np.asarray(element)
    return np.nonzero((el == b"N") | (el == b"O"))[0], np.nonzero(el == b"H")[0]


def close(got, want, tol=1e-3):
    """compare_hbonds: indices exact, distance and angle within tol"""
    return (int(got[0]), int(got[1]), int(got[2])) == tuple(want[:3]) and abs(float(got[3]) - want[3]) <= tol and abs(float(got[4]) - want[4]) <= tol

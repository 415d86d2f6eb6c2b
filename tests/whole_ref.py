"""numpy-f32 restatement of the reference's bond topology and make-whole calls (the yardstick of the make-whole tests).

Reference (paths relative to the groan_rs root):
  get_molecule_indices        src/system/iterating.rs:399-432   breadth-first, neighbours in ascending order (Atom::get_bonded is sorted)
  create_mol_references       src/system/modifying.rs:258-283   first unvisited atom with a bond, in index order
  make_molecules_whole        src/system/modifying.rs:338-392   ref_w = wrap(ref); atom = ref_w + ref_w.vector_to(atom)
  make_group_whole            src/system/modifying.rs:447-475   c = group_estimate_center; atom = c + c.vector_to(atom)
  wrap_coordinate             src/structures/vector3d.rs:398-417  `while w > L: w -= L; while w < 0: w += L`
  vector_to / floor_mod       src/structures/vector3d.rs:561-569, :28-30   floor_mod(x, y) = ((x % y) + y) % y
Every operation is one f32 operation, as in Rust (no contraction).  Orthorhombic boxes only: the library's triclinic extension is
checked against the oracle instead.  Unlike the reference, a frame that fails is returned unchanged (the library's batch rule)."""
from collections import deque

import numpy as np

F = np.float32


def neighbours(n, bonds):
    """sorted neighbour lists of n atoms from (i, j) pairs (either order, duplicates allowed)"""
    nb = [set() for _ in range(n)]
    for i, j in np.asarray(bonds, np.int64).reshape(-1, 2).tolist():
        nb[i].add(j); nb[j].add(i)
    return [sorted(s) for s in nb]


def bfs(nbrs, start):
    out, seen, q = [], {start}, deque([start])
    while q:
        a = q.popleft()
        out.append(a)
        for b in nbrs[a]:
            if b not in seen:
                seen.add(b); q.append(b)
    return out


def molecules(nbrs):
    """(references ascending, breadth-first order of each molecule)"""
    seen, refs, orders = set(), [], []
    for a in range(len(nbrs)):
        if a in seen or not nbrs[a]:
            continue
        o = bfs(nbrs, a)
        seen.update(o); refs.append(a); orders.append(o)
    return refs, orders


def ref_of(n, refs, orders):
    """per atom: the reference of its polyatomic molecule, -1 outside one"""
    r = np.full(n, -1, np.int64)
    for a, o in zip(refs, orders):
        r[o] = a
    return r


def wrap_coord(x, L):
    """the reference's loops, as masked repeated subtraction / addition (x, L: f32 arrays broadcastable)"""
    w = np.array(x, F, copy=True)
    L = np.broadcast_to(np.asarray(L, F), w.shape)
    while True:
        m = w > L
        if not m.any():
            break
        w[m] = (w[m] - L[m]).astype(F)
    while True:
        m = w < F(0)
        if not m.any():
            break
        w[m] = (w[m] + L[m]).astype(F)
    return w


def floor_mod(x, y):
    x = np.asarray(x, F); y = np.asarray(y, F)
    return np.fmod((np.fmod(x, y) + y).astype(F), y).astype(F)


def vector_to(a, p, box3):
    """a.vector_to(p) for rows of a and p, orthorhombic box (3,)"""
    L = np.asarray(box3, F)
    h = (L / F(2)).astype(F)
    d = ((np.asarray(p, F) - np.asarray(a, F)).astype(F) + h).astype(F)
    return (floor_mod(d, L) - h).astype(F)


def wrap(p, box3):
    return wrap_coord(p, np.asarray(box3, F))


def make_molecules_whole(pos, box3, ref_of, orders=None):
    """-> (new positions, None) or (pos unchanged, atom index of the NoPosition error).
    ref_of[i] = the reference atom of i's polyatomic molecule, -1 outside one; orders (list of breadth-first orders, by
    ascending reference) is needed only to name the failing atom."""
    pos = np.asarray(pos, F)
    ref_of = np.asarray(ref_of, np.int64)
    inmol = ref_of >= 0
    bad = inmol & np.isnan(pos[:, 0])
    if bad.any():
        first_ref = ref_of[bad].min()
        o = next(o for o in orders if o[0] == first_ref)
        return pos.copy(), next(a for a in o if np.isnan(pos[a, 0]))
    out = pos.copy()
    idx = np.nonzero(inmol)[0]
    ref_w = wrap(pos[ref_of[idx]], box3)
    out[idx] = (ref_w + vector_to(ref_w, pos[idx], box3)).astype(F)
    is_ref = idx == ref_of[idx]                  # the reference itself is only wrapped (the loop skips it: .skip(1))
    out[idx[is_ref]] = ref_w[is_ref]
    return out, None


def make_group_whole(pos, idx, box3, center):
    """every atom of idx becomes c + c.vector_to(atom); center = the (estimated) centre the caller supplies"""
    pos = np.asarray(pos, F); out = pos.copy()
    idx = np.asarray(idx, np.int64)
    c = np.broadcast_to(np.asarray(center, F), (len(idx), 3))
    out[idx] = (c + vector_to(c, pos[idx], box3)).astype(F)
    return out


def gro_xyz(p):
    """the coordinate fields of a gro atom line (write_gro: %8.3f each)"""
    return "%8.3f%8.3f%8.3f" % (float(p[0]), float(p[1]), float(p[2]))

"""The cell grid (gr_cellgrid.h: gr_cellgrid_make, gr_cg_cell_of) where random positions never go: atoms ON cell borders and box faces,
atoms whose wrapped coordinate is a rounded one, axes of 1 - 4 cells, the 1024-cell clamp, groups at the 256-lane block and a pair buffer
shorter than the result -- through its three consumers, System.group_pairs_within, Contacts and HBondAnalysis.

The yardstick is the oracle's brute force over all pairs (oracle_lib.pairs_within), which knows no grid: identical index lists in the same
order, d within 1e-6 nm (check of test_gpu_pairs_within.py; check_call / check_oracle of test_gpu_contacts.py for Contacts; hbond_ref for
the hydrogen bonds).  Nothing is sampled.  tests/cellgrid_ref.py (pinned to the C++ functions bit for bit by tests/test_cellgrid_host.py)
says where the borders are and how many cells a box has; the cell count is confirmed by Contacts' own statistic.  The boxes are slabs --
long along the axis under test, two cells along the others -- with enough atoms that Contacts and HBondAnalysis do not coarsen the grid.

NAMED are three pairs exactly at the cut-off that a cell only 1.00001 x cutoff thick puts two cells apart (gr_cellgrid.h)."""
import ctypes as C

import numpy as np
import pytest

import cellgrid_ref as R
import hbond_ref as HR
import oracle_lib as O
import test_gpu_hbonds as TH
from test_gpu_contacts import G, check_call, check_oracle, load     # noqa: F401 (G: the fixture)
from test_gpu_pairs_within import check

pytestmark = pytest.mark.gpu
F = np.float32
TURNS = (-1.0, 1.0, -2.0, 17.0)            # the images of an atom outside the cell; 17 is beyond the wrap's loop (GR_LOOP_TURNS): its cell
#                                            comes from the closed form, its distances (1e-6 nm from the oracle's) from the loop (GR_EXACT_TURNS)
NAMED = [(0.25, 41.25042, -9.000093, 32.000324), (0.25, 50.00051, -7.500078, 42.25043), (1.0, 282.00284, -51.000526, 230.0023)]


def up(v, n=1):
    v = F(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, F(np.inf) if n > 0 else F(-np.inf))
    return v


def box9(lengths):
    b = np.zeros(9, F); b[:3] = lengths
    return b


def slab(axis, L, cutoff, others=2):
    """L along `axis`, `others` cells along the two other axes"""
    lengths = [F((others + 0.5) * cutoff)] * 3
    lengths[axis] = F(L)
    assert R.grid(lengths, cutoff)[(axis + 1) % 3] == others
    return box9(lengths)


def partner(p, axis, side, cutoff, target, box):
    """a position whose distance from p in the oracle's float32 arithmetic is `target`: cutoff minus a little along the axis, the rest
    along the next axis, found by bisection over its floats"""
    q = np.array(p, F)
    q[axis] = F(p[axis] + F(side) * F(cutoff * 0.9999))
    o = (axis + 1) % 3
    lo, hi = F(0.0), F(0.2 * cutoff)
    dist = lambda dy: O.distance([q[0] + (o == 0) * dy, q[1] + (o == 1) * dy, q[2] + (o == 2) * dy], p, "xyz", box)
    for _ in range(8):                                                   # far from the origin the floats are coarse: come closer until below the target
        if dist(lo) < target: break
        q[axis] = up(q[axis], -side)
    assert dist(lo) < target <= dist(hi)
    lo_b, hi_b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while hi_b - lo_b > 1:
        mid = (lo_b + hi_b) // 2
        if dist(np.uint32(mid).view(F)) < target: lo_b = mid
        else: hi_b = mid
    q[o] = F(q[o] + np.uint32(hi_b).view(F))
    assert F(O.distance(q, p, "xyz", box)) == F(target), (p, q, target)
    return q


def around(p, axis, cutoff, box, images=True):
    """p, its neighbours one float to either side along the axis, its images TURNS box lengths away, partners at the cut-off, one float
    below and one float above it on either side, and partners well inside.  (The distance follows the reference's loop for 20 turns,
    GR_EXACT_TURNS: the farthest two of these atoms are 19 box lengths apart.)"""
    L = box[axis]
    out = [np.array(p, F)]
    for n in (-1, 1):
        q = np.array(p, F); q[axis] = up(p[axis], n); out.append(q)
    for t in TURNS if images else ():
        q = np.array(p, F); q[axis] = F(p[axis] + F(t) * L); out.append(q)
    for side in (-1, 1):
        for target in (F(cutoff), up(cutoff, -1), up(cutoff, 1)):
            out.append(partner(p, axis, side, cutoff, target, box))
        q = np.array(p, F); q[axis] = F(p[axis] + F(side * 0.5 * cutoff)); out.append(q)
    return out


def bystanders(rng, n, box):
    return (rng.uniform(-0.6, 1.6, (n, 3)) * box[:3]).astype(F)


def groups_of(s, n, n1):
    """"r" = the first n1 atoms (the special ones) as a range; "i" = an index list of every other special atom and the bystanders
    without every seventh -> their indices.  Both hold border atoms, and "i" selects them through its list"""
    s.group_create_from_ranges("r", [(0, n1 - 1)])
    ii = np.array(list(range(1, n1, 2)) + [k for k in range(n1, n) if k % 7 != 3])
    s.group_create_from_indices("i", ii.tolist())
    return np.arange(n1), ii


def assemble(special, box, cutoff, seed):
    cells = int(np.prod(R.grid(box[:3], cutoff)))
    assert cells <= 1 << 16
    special = np.array(special, F)
    n1 = special.shape[0]
    n = n1 + max(40, (cells // 2 + 8) * 7 // 6 + 8)
    return np.concatenate([special, bystanders(np.random.default_rng(seed), n - n1, box)]), n1, cells


def run_consumers(G, special, box, cutoff, seed, consumers=("pairs", "contacts")):
    """the special atoms first, bystanders up to where Contacts keeps the cut-off's grid.  Every consumer gets the special atoms on BOTH
    sides: as a range against the index list, the other way round, either group against itself and every atom against every atom
    -> the number of pairs among all atoms"""
    pos, n1, cells = assemble(special, box, cutoff, seed)
    n = pos.shape[0]
    s = load(G, [pos], [box])
    ir, ii = groups_of(s, n, n1)
    ia = np.arange(n)
    assert 2 * ii.size >= cells
    total = O.pairs_within(pos, ia, ia, box, cutoff)[0].size
    if "pairs" in consumers:
        check(G, s, pos, "r", ir, "r", ir, box, cutoff)
        check(G, s, pos, "r", ir, "i", ii, box, cutoff)
        check(G, s, pos, "i", ii, "r", ir, box, cutoff)
        check(G, s, pos, "i", ii, "i", ii, box, cutoff)
        assert check(G, s, pos, "all", ia, "all", ia, box, cutoff) == total
    if "contacts" in consumers:
        for g1, i1, g2, i2 in (("all", ia, "all", ia), ("r", ir, "i", ii), ("i", ii, "r", ir), ("i", ii, "i", ii)):
            with G.Contacts(s, g1, g2, cutoff) as ct:
                n_pairs, st = ct.pairs(0, 1)
                assert (st == 0).all() and ct.stat(G._lib.CT_STAT_LAST_CELLS) == cells       # the cut-off's own grid, not a coarser one
                check_oracle(ct.lists(), [pos], [box], i1, i2, cutoff)
                check_call(ct, s, g1, g2, cutoff, 0, 1, i1)
    s.close()
    return total


def on_axis(axis, v, other=1.0):
    p = np.full(3, other, F); p[axis] = F(v)
    return p


# ------------------------------------------------------------------ a. pairs across a cell border
@pytest.mark.parametrize("consumer", ["pairs", "contacts"])
@pytest.mark.parametrize("row,axis", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 2)], ids=["L41_x", "L50_x", "L282_x", "L41_y", "L50_z"])
def test_named_pairs_at_the_cutoff(G, row, axis, consumer):
    """the pair, exactly at the cut-off with one atom outside the cell: found by group_pairs_within and by Contacts (each on its own, so
    that neither hides the other), from either side; the first atom is in the range group, the second in the index list too"""
    cutoff, L, xi, xj = NAMED[row]
    box = slab(axis, L, cutoff)
    a, b = on_axis(axis, xi), on_axis(axis, xj)
    assert F(O.distance(b, a, "xyz", box)) == F(cutoff)
    special = around(a, axis, cutoff, box) + around(b, axis, cutoff, box)
    oi, oj, _ = O.pairs_within(np.array(special, F), [0], [len(special) // 2], box, cutoff)
    assert oi.size == 1 and (len(special) // 2) % 2 == 1                 # the oracle reports it, and its second atom is in "i"
    assert run_consumers(G, special, box, cutoff, 10 + row, consumers=(consumer,)) > 50


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("cutoff,k", [(0.25, 165), (0.6, 70)])
def test_pairs_across_borders_of_the_thinnest_cells(G, axis, cutoff, k):
    """a box on the step of floor(L / cs): k cells as thin as the grid makes them.  Atoms on the lowest float of a low, a middle and a
    high cell of the axis (and the highest float below it), with partners at the cut-off on either side"""
    L = R.step_length(cutoff, k)
    box = slab(axis, L, cutoff)
    assert R.grid(box[:3], cutoff)[axis] == k
    special = []
    for m in (1, k // 2, k - 1):
        w = R.border(L, cutoff, m)
        special += around(on_axis(axis, w), axis, cutoff, box)
        special += around(on_axis(axis, up(w, -1) - L), axis, cutoff, box)[:7]      # from outside the cell
    assert run_consumers(G, special, box, cutoff, 20 + axis) > 100


def test_a_corner_of_three_borders(G):
    """an atom on a cell border along x, y and z at once, partners across each border and across all three"""
    cutoff, ks = 0.3, (40, 3, 3)
    lengths = [R.step_length(cutoff, k) for k in ks]
    box = box9(lengths)
    assert R.grid(lengths, cutoff) == ks
    corner = np.array([R.border(lengths[0], cutoff, 17), R.border(lengths[1], cutoff, 1), R.border(lengths[2], cutoff, 2)], F)
    special = []
    for axis in range(3):
        special += around(corner, axis, cutoff, box)
    for sg in ((-1, -1, -1), (1, 1, 1), (-1, 1, -1)):
        for r in (0.55, 0.577, 0.58):                                    # the diagonal: inside, about on and outside the cut-off
            special.append((corner + F(r * cutoff) * np.array(sg, F)).astype(F))
    below = np.array([up(c, -1) for c in corner], F)
    special += [below, (below - box[:3]).astype(F), (below + F(17.0) * box[:3]).astype(F)]
    assert run_consumers(G, special, box, cutoff, 31) > 100


def test_hydrogen_bond_across_a_border_at_max_distance(G):
    """the first named pair as donor and acceptor, the hydrogen on the line between them: a bond at exactly max_distance"""
    dmax, L, xi, xj = NAMED[0]
    box = slab(0, L, dmax)
    cells = int(np.prod(R.grid(box[:3], dmax)))
    donor, acc = on_axis(0, xi), on_axis(0, xj)
    hyd = on_axis(0, F(xi) - F(0.1))                                     # towards the acceptor's image at x_j - L
    n_by = cells // 2 + 20
    pos = np.concatenate([[donor, hyd, acc], bystanders(np.random.default_rng(41), n_by, box)]).astype(F)
    n = pos.shape[0]
    accs = [2] + list(range(3, n))
    assert 2 * len(accs) >= cells                                        # hb_grid keeps the cut-off's grid
    bonds = np.array([[0, 1]])
    s = TH.system(G, [pos], [box], {"A": accs, "D": [0], "H": [1]})
    an = G.HBondAnalysis(s, [G.HBondChain("A", "D", "H")], [(0, 0)], dmax, 150.0, bonds)
    res = an.batch(0, 1)
    assert (res[6] == 0).all()
    got = TH.frame_bonds(res, 1, 0, 0)
    chain = HR.resolve_chain(accs, [0], [1], HR.bonded(bonds, n))
    want = HR.analyze(pos, box, [chain], [(0, 0)], dmax, 150.0)[(0, 0)]
    TH.compare(got, want, dmax, 150.0)
    key = [(d, h, a) for d, h, a, _, _ in got]
    assert (0, 1, 2) in key and (0, 1, 2) in [(d, h, a) for d, h, a, _, _ in want]       # compare() forgives a bond at the threshold: this one it may not
    dist = [b[3] for b in got if b[:3] == (0, 1, 2)][0]
    assert F(dist) == F(dmax)
    s.close()


# ------------------------------------------------------------------ b. atoms on the faces of the box
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("L", [7.25, 41.25042])
def test_atoms_on_box_faces(G, axis, L):
    cutoff = 0.3
    box = slab(axis, L, cutoff, others=3)
    L = box[axis]
    tiny = F(-1e-9)
    assert F(tiny + L) == L                                              # the closed upper end: the wrap leaves this atom ON L
    faces = [F(0.0), F(-0.0), L, up(L, -1), np.nextafter(F(0.0), F(-1.0)), tiny, F(1e-42), F(-2.0) * L, F(2.0) * L, up(L, 1)]
    special = []
    for v in faces:
        special += around(on_axis(axis, v, other=0.2), axis, cutoff, box, images=False)
    assert run_consumers(G, special, box, cutoff, 50 + axis) > 500


# ------------------------------------------------------------------ c. axes of one to four cells
def test_every_combination_of_1_to_4_cells(G):
    """64 boxes of 1 - 4 cells per axis, every edge on a step of floor(L / cs): one float below it (a cell fewer), on it, one float above.
    With 2 cells the walk visits a cell and its upper neighbour, with 1 the cell alone: no pair twice, none missing.  In at least 16 of
    the boxes the cut-off is above half the shortest edge.  Atoms on the corners of the box, one float inside it, and 1 and 17 box
    diagonals away"""
    cutoff = 0.4
    steps = {k: R.step_length(cutoff, k) for k in (1, 2, 3, 4, 5)}
    steps[1] = F(cutoff * 1.3)                                           # (one cell has no step below it)
    seen, above_half = set(), 0
    for kx in range(1, 5):
        for ky in range(1, 5):
            for kz in range(1, 5):
                want, lengths = [], []
                for a, k in enumerate((kx, ky, kz)):
                    v = (kx + 2 * ky + 3 * kz + a) % 3                   # 0: one float below the step to k + 1; 1: on the step to k; 2: one float above it
                    lengths.append(up(steps[k + 1], -1) if v == 0 else up(steps[k], v - 1))
                    want.append(k)
                above_half += cutoff > min(lengths) / 2
                box = box9(lengths)
                assert R.grid(lengths, cutoff) == tuple(want), (lengths, want)
                rng = np.random.default_rng(100 * kx + 10 * ky + kz)
                pos = bystanders(rng, 40, box)
                pos[:6] = [[0, 0, 0], box[:3], [up(l, -1) for l in lengths], [-l for l in lengths], [l / F(2) for l in lengths], [F(17) * l for l in lengths]]
                s = load(G, [pos], [box])
                ir, ii = groups_of(s, 40, 16)
                i, j, d = s.group_pairs_within("all", "all", cutoff)
                assert len(set(zip(i.tolist(), j.tolist()))) == i.size           # no pair twice
                assert check(G, s, pos, "all", np.arange(40), "all", np.arange(40), box, cutoff) > 0
                check(G, s, pos, "r", ir, "i", ii, box, cutoff)
                with G.Contacts(s, "all", "all", cutoff) as ct:
                    got = check_call(ct, s, "all", "all", cutoff, 0, 1, np.arange(40))
                    assert ct.stat(G._lib.CT_STAT_LAST_CELLS) == kx * ky * kz
                    check_oracle(got, [pos], [box], np.arange(40), np.arange(40), cutoff)
                s.close()
                seen.add((kx, ky, kz))
    assert len(seen) == 64 and above_half >= 16


# ------------------------------------------------------------------ d. the clamp at 1024 cells per axis
def test_the_1024_cell_clamp(G):
    cutoff = 0.3
    box = box9([400.0, 0.7, 0.7])
    assert R.grid(box[:3], cutoff) == (1024, 2, 2) and int(400.0 / cutoff) == 1333
    special = []
    for v in (0.0, 0.1, 200.0, R.border(400.0, cutoff, 512), R.border(400.0, cutoff, 1023), 399.9, up(400.0, -1), -0.05, 400.05):
        special += around(on_axis(0, v, other=0.3), 0, cutoff, box)
    assert run_consumers(G, special, box, cutoff, 61) > 500


# ------------------------------------------------------------------ e. groups at the 256-lane block
def test_group_sizes_at_the_block(G):
    cutoff, n = 0.4, 600
    box = box9([3.0, 2.6, 2.2])
    pos = bystanders(np.random.default_rng(71), n, box)
    s = load(G, [pos], [box])
    sizes = (1, 255, 256, 257)
    idx_b = {m: np.arange(50, 50 + 2 * m, 2) for m in sizes}            # every other atom: an index list that shares atoms with the ranges
    for m in sizes:
        s.group_create_from_ranges("a%d" % m, [(0, m - 1)])
        s.group_create_from_indices("b%d" % m, idx_b[m].tolist())
    for m1 in sizes:
        a, ia = "a%d" % m1, np.arange(m1)
        for m2 in sizes:
            b, ib = "b%d" % m2, idx_b[m2]
            check(G, s, pos, a, ia, b, ib, box, cutoff)
            check(G, s, pos, b, ib, a, ia, box, cutoff)
        same = check(G, s, pos, a, ia, a, ia, box, cutoff)               # the same group on both sides
        assert (same == 0) == (m1 == 1)
        check(G, s, pos, "b%d" % m1, idx_b[m1], "b%d" % m1, idx_b[m1], box, cutoff)
        with G.Contacts(s, a, "b257", cutoff) as ct:
            got = check_call(ct, s, a, "b257", cutoff, 0, 1, ia)
            check_oracle(got, [pos], [box], ia, idx_b[257], cutoff)
    i, j, d = s.group_pairs_within("a1", "a1", cutoff)                   # one atom against itself
    assert i.size == 0
    assert check(G, s, pos, "a257", np.arange(257), "b257", idx_b[257], box, 1e-4) == 0       # no pair at all
    s.close()


# ------------------------------------------------------------------ f. a pair buffer shorter than the result
def test_max_pairs_below_the_total(G):
    cutoff, n = 0.45, 300
    box = box9([2.4, 2.0, 1.7])
    pos = bystanders(np.random.default_rng(81), n, box)
    s = load(G, [pos], [box])
    s.group_create_from_ranges("a", [(0, 119)]); s.group_create_from_indices("b", list(range(100, n, 2)) + [1, 5])
    fi, fj, fd = s.group_pairs_within("a", "b", cutoff)
    total = fi.size
    assert total > 200
    full = set(zip(fi.tolist(), fj.tolist(), fd.view(np.uint32).tolist()))
    ends = np.flatnonzero(np.diff(fi)) + 1                               # where the segment of one group-1 atom ends
    boundary = int(ends[len(ends) // 2])
    SENT = 0xDEADBEEF
    for cap in (0, 1, boundary, total - 1):
        room = total + 16
        bi = np.full(room, SENT, np.uint32); bj = np.full(room, SENT, np.uint32); bd = np.full(room, SENT, np.uint32).view(F)
        cnt = C.c_uint64(0)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        st = s._lib.gr_group_pairs_within(s._ctx, 0, b"a", b"b", C.c_float(cutoff), cap, ptr(bi), ptr(bj), ptr(bd), C.byref(cnt))
        assert st == 0 and int(cnt.value) == total                       # the full total, whatever fits
        for buf in (bi, bj, bd.view(np.uint32)):
            assert (buf[cap:] == SENT).all()                             # nothing at or beyond max_pairs
        rows = set(zip(bi[:cap].tolist(), bj[:cap].tolist(), bd[:cap].view(np.uint32).tolist()))
        assert len(rows) == cap and rows <= full                         # every written row is a pair of the full result
        whole = int(ends[ends <= cap].max()) if (ends <= cap).any() else 0     # the atoms whose segment fits below max_pairs
        assert np.array_equal(bi[:whole], fi[:whole]) and np.array_equal(bj[:whole], fj[:whole])
        assert np.array_equal(bd[:whole].view(np.uint32), fd[:whole].view(np.uint32))
    s.close()

"""make_molecules_whole / make_group_whole (gr_whole.h) at the edges of their layout and in mixed batches: system sizes round the
4-atom groups and the 256-atom tiles, references read from other tiles, non-orthogonal cells for make_group_whole, batches that
start above slot 0 with another box in every slot, and failed frames in every chunk of a multi-chunk batch.

The yardsticks are those of tests/test_gpu_whole.py: bit for bit against tests/whole_ref.py in orthorhombic cells, within 1e-5 nm
of the oracle's wrap / vector_to elsewhere; atoms a call must not move are compared bit for bit with what was uploaded."""
import itertools

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_whole as TW
import whole_ref as W

pytestmark = pytest.mark.gpu
E_NO_POSITION = 6
TOL = 1e-5                                  # nm: the tolerance of test_full_size_molecules / test_full_size_group


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


_bits = TW._bits
_lattice = TW._lattice


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ortho(box9):
    return not np.asarray(box9)[3:].any()


# ------------------------------------------------------------------ topology and frames of the sweep
def edge_topology(n):
    """-> (bonds [m, 2], ref [n]: the reference of the atom's molecule or -1, kinds: what the topology holds)
       chain        n >= 65: reference atom 1, then atoms 33 and 62 and three atoms of every later tile -- from 264 atoms on its
                    reference is read from other tiles (GR_TOPO_FARREF: the gathered reference, k_whole_far)
       alternating  n >= 265: atoms 250 .. 261, even and odd indices two molecules: both cross the 255 / 256 edge
       lone         atoms 20, 57, 94, ... (i % 37 == 20) and, from 300 atoms on, atom 262: in no molecule
       triatomic    every other atom, three consecutive free indices each, water-like bonds (a, b) (a, c); the last molecule
                    takes what is left (2 to 4 atoms), so it ends on atom n - 1"""
    taken = np.zeros(n, bool)
    ref = np.full(n, -1, np.int64)
    bonds, kinds = [], set()
    if n >= 65:
        chain = [1, 33, 62]
        for t in range(1, (n + 255) // 256):
            chain += [a for a in (256 * t + 7, 256 * t + 129, 256 * t + 254) if a < n - 4]
        bonds += list(zip(chain[:-1], chain[1:]))
        ref[chain] = 1; taken[chain] = True
        kinds.add("chain")
        if chain[-1] >= 256: kinds.add("far")
    if n >= 265:
        for par in (0, 1):
            a = np.arange(250 + par, 262, 2)
            bonds += list(zip(a[:-1], a[1:]))
            ref[a] = 250 + par; taken[a] = True
        kinds.add("alternating")
    lone = [i for i in range(20, n - 4, 37) if not taken[i]] + ([262] if n >= 300 else [])
    taken[lone] = True
    if lone: kinds.add("lone")
    free = np.nonzero(~taken)[0]
    assert len(free) >= 2
    cut = list(range(0, len(free), 3))
    if len(free) - cut[-1] == 1:
        cut.pop()                                   # ... the last molecule has four atoms
    for k, c in enumerate(cut):
        mol = free[c:cut[k + 1]] if k + 1 < len(cut) else free[c:]
        bonds += [(mol[0], b) for b in mol[1:]]
        ref[mol] = mol[0]
    assert ref[n - 1] >= 0
    return np.array(bonds, np.uint64), ref, kinds, np.array(lone, np.int64)


def edge_frames(box9, ref, lone, seed, nan_lone=True):
    """as test_gpu_whole._frames: compact molecules about their references, every atom moved by a random lattice vector with
    probability 1/2, some references exactly on faces; every other lone atom has no position"""
    n = len(ref)
    rng = np.random.default_rng(seed)
    M = _lattice(box9)
    refpos = (rng.random((n, 3), np.float32) @ M).astype(np.float32)
    faces = np.array([[0, 0, 0], [box9[0], 1.0, 1.0], [-1e-7, 2.0, 2.0], [3.0, box9[1], -0.0], [np.float32(box9[0]) * 2, 0, box9[2]]], np.float32)
    refs = np.unique(ref[ref >= 0])
    for k, r in enumerate(refs[:: max(1, len(refs) // 5)][:5]):
        refpos[r] = faces[k]
    off = rng.normal(0.0, 0.06, (n, 3)).astype(np.float32)
    far = ref == 1                                                       # the chain: a wide molecule
    off[far] = rng.uniform(-1.5, 1.5, (int(far.sum()), 3)).astype(np.float32)
    inmol = ref >= 0
    pos = refpos.copy()
    pos[inmol] = (refpos[ref[inmol]] + off[inmol]).astype(np.float32)
    pos[refs] = refpos[refs]
    shifts = rng.integers(-1, 2, (n, 3)).astype(np.float32)
    shifts[rng.random(n) < 0.5] = 0
    pos = (pos + shifts @ M).astype(np.float32)
    if nan_lone:
        pos[lone[::2]] = np.nan
    return pos


def check_molecules(got, inp, box9, ref, tag):
    """one frame after make_molecules_whole against its reference, every atom"""
    lone = ref < 0
    assert _same(got[lone], inp[lone]), tag                              # atoms outside molecules, those without position included
    if _ortho(box9):
        want, err = W.make_molecules_whole(inp, box9[:3], ref)
        assert err is None
        bad = np.nonzero((_bits(got) != _bits(want)).any(1))[0]
        assert bad.size == 0, (tag, bad[:5], got[bad[:5]], want[bad[:5]])
        return
    refw = {}
    for a in np.nonzero(~lone)[0]:
        r = int(ref[a])
        if r not in refw:
            refw[r] = O.wrap(inp[r], box9)
        want = refw[r] + O.vector_to(refw[r], inp[a], box9)
        assert np.abs(got[a] - want).max() <= TOL, (tag, a, r, got[a], want)


# ------------------------------------------------------------------ A: the sizes round the 4-atom groups and the 256-atom tiles
@pytest.mark.parametrize("kind", ["ortho", "dodecahedron", "triclinic"])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 258, 511, 513, 1025])
def test_tile_boundary_sweep(G, n, kind):
    bonds, ref, kinds, lone = edge_topology(n)
    assert kinds == {k for k, least in (("lone", 25), ("chain", 65), ("alternating", 265), ("far", 268)) if n >= least}, (n, kinds)
    refs, orders = W.molecules(W.neighbours(n, bonds))
    assert np.array_equal(W.ref_of(n, refs, orders), ref)                # the topology is what it says it is
    if n in (257, 513, 1025):                                            # a water-like molecule across the last tile edge
        edge = (n - 1) // 256 * 256
        assert any(ref[a] >= 0 and ref[a] < edge and ref[a] != 1 for a in range(edge, min(edge + 2, n)))
    box9 = TW._box9(kind)
    s = G.System(n, n_slots=5)
    s.add_bonds(bonds)
    assert s.get_mol_references() == refs
    inputs = [edge_frames(box9, ref, lone, 100 * n + 10 * k + len(kind)) for k in range(5)]
    for k in range(5):
        s.set_frame(inputs[k], box9, slot=k)
    st = s.make_molecules_whole_batch(1, 3)
    assert (st == 0).all()
    for k in (0, 4):
        assert _same(s.get_positions(k), inputs[k]), k
    for k in (1, 2, 3):
        check_molecules(s.get_positions(k), inputs[k], box9, ref, (n, kind, k))
    s.close()


# ------------------------------------------------------------------ B: make_group_whole, its three forms
def blob_frame(rng, n, idx, box9, centre_frac, outliers=0):
    """a compact blob (sigma = 0.1 of the shortest box height) of the atoms idx about a point, every atom of it moved by a random
    lattice vector; the other atoms anywhere in and round the cell.  `outliers` atoms of the blob lie anywhere in the cell about
    that point instead: in a skewed cell some of them have their nearest image outside the brick the first reduction maps into,
    which only the search of gr_tric_refine finds (too few of them to move the circular mean)"""
    M = _lattice(box9).astype(np.float64)
    heights = 1.0 / np.linalg.norm(np.linalg.inv(M), axis=0)
    p = rng.uniform(-0.5, 1.5, (n, 3)) @ M
    p[idx] = np.asarray(centre_frac) @ M + rng.normal(0.0, 0.1 * heights.min(), (len(idx), 3))
    if outliers:
        far = rng.choice(len(idx), outliers, replace=False)
        p[idx[far]] = (np.asarray(centre_frac) + rng.uniform(-0.5, 0.5, (outliers, 3))) @ M
    p[idx] += rng.integers(-1, 2, (len(idx), 3)) @ M
    return p.astype(np.float32)


def check_group_free(got, inp, idx, box9, tag):
    """independent of the library: got - input is a lattice vector, and no image of the atom lies nearer to the oracle's
    estimated centre than the one the call chose"""
    M = _lattice(box9).astype(np.float64)
    others = np.setdiff1d(np.arange(len(inp)), idx)
    assert _same(got[others], inp[others]), tag
    g, p = got[idx].astype(np.float64), inp[idx].astype(np.float64)
    k = np.linalg.solve(M.T, (g - p).T).T
    assert np.linalg.norm((g - p) - np.rint(k) @ M, axis=1).max() <= TOL, tag
    c = O.estimate_center(inp, idx, box9).astype(np.float64)
    best = np.full(len(idx), np.inf)
    for t in itertools.product(range(-2, 3), repeat=3):
        best = np.minimum(best, np.linalg.norm(p + np.array(t, np.float64) @ M - c, axis=1))
    d = np.linalg.norm(g - c, axis=1)
    worst = int(np.argmax(d - best))
    assert d[worst] <= best[worst] + TOL, (tag, idx[worst], got[idx[worst]], c, d[worst], best[worst])


CELLS = {"dodecahedron": ([22.0, 22.0, 22.0], [60.0, 60.0, 90.0]), "triclinic": ([22.0, 21.5, 23.0], [75.0, 80.0, 70.0]),
         "skewed_negative": ([6.5, 7.5, 6.0], [100.0, 95.0, 110.0])}
# gr_api.hip group_build / make_sel and gr_whole.h group_whole_batch: one block is `contiguous` (form 0); a scattered selection is
# `masked` (form 2) when it has >= 4096 atoms and at least an eighth of its span, else it keeps to its index list (form 1).
# In 6 000 atoms every second atom of a span is at most 3 000 atoms and would take the list: three atoms of every four of
# 16 .. 5 987 (4 479 atoms) is the dense scattered selection that gets the mask here.
SELECTIONS = {"block": np.arange(3, 4098), "gather": np.arange(5, 6000, 11),
              "masked": np.array([a for a in range(16, 5988) if a % 4 != 1])}


@pytest.mark.parametrize("form", ["block", "gather", "masked"])
@pytest.mark.parametrize("cell", list(CELLS))
def test_group_whole_in_non_orthogonal_cells(G, cell, form):
    n, idx = 6000, SELECTIONS[form]
    assert form != "masked" or (len(idx) >= 4096 and 8 * len(idx) >= idx[-1] - idx[0] + 1 and (np.diff(idx) > 1).any())
    box9 = O.box_from_lengths_angles(*CELLS[cell])
    rng = np.random.default_rng(len(cell) * 10 + len(form))
    inputs = [blob_frame(rng, n, idx, box9, cf, outliers=32) for cf in ([0.3, 0.6, 0.45], [0.02, 0.97, 0.5])]   # (the second blob lies across faces)
    s = G.System(n, n_slots=2)
    for k in range(2):
        s.set_frame(inputs[k], box9, slot=k)
    s.group_create_from_indices("sel", idx)
    st = s.make_group_whole_batch("sel", 0, 2)
    assert (st == 0).all()
    for k in range(2):
        check_group_free(s.get_positions(k), inputs[k], idx, box9, (cell, form, k))
    s.close()


@pytest.mark.parametrize("n", [5, 64, 257])
def test_group_whole_small_orthorhombic(G, n):
    """the same three kinds of selection in systems of a few atoms, bit for bit (below 4096 atoms the dense scattered one keeps
    to its index list: form 1, as the sparse one)"""
    box9 = TW._box9("ortho")
    sels = {"block": np.arange(1, n - 1), "gather": np.arange(0, n, 11 if n > 11 else 4), "dense": np.arange(n % 2, n, 2)}
    rng = np.random.default_rng(n)
    s = G.System(n, n_slots=1)
    for name, idx in sels.items():
        s.group_create_from_indices(name, idx)
        inp = blob_frame(rng, n, idx, box9, [0.9, 0.1, 0.5])
        s.set_frame(inp, box9)
        c, _ = s.group_center_batch(name, 1, 0, 0, 1)                     # the library's own estimate, on the frame before the call
        s.make_group_whole(name)
        got = s.get_positions()
        assert _same(got, W.make_group_whole(inp, idx, box9[:3], c[0])), (n, name)
        oc = O.estimate_center(inp, idx, box9)
        for a in idx:
            assert np.abs(got[a] - (oc + O.vector_to(oc, inp[a], box9))).max() <= TOL, (n, name, a)
    s.close()


# ------------------------------------------------------------------ C: first slot above 0, another box in every slot
def _slot_boxes():
    o = [np.array(b + [0.0] * 6, np.float32) for b in ([21.5, 22.0, 21.0], [18.0, 19.5, 20.5], [24.0, 17.0, 19.0], [16.5, 23.0, 18.5])]
    dod, tri = TW._box9("dodecahedron"), TW._box9("triclinic")
    tri2 = O.box_from_lengths_angles([19.0, 20.0, 18.0], [80.0, 70.0, 75.0])
    #       0     1     2     3    4    5 (frame of 2)  6 (frame of 3)  7 (frame of 4)
    return [o[0], o[1], o[2], dod, tri, o[3], tri2, o[0]]


def test_first_slot_above_zero_mixed_boxes_molecules(G):
    n = 300
    bonds, ref, _, lone = edge_topology(n)
    boxes = _slot_boxes()
    inputs = [edge_frames(boxes[k], ref, lone, 40 + k) for k in range(5)]
    inputs += [inputs[2], inputs[3], inputs[4]]

    def fresh():
        s = G.System(n, n_slots=8)
        s.add_bonds(bonds)
        for k in range(8):
            s.set_frame(inputs[k], boxes[k], slot=k)
        return s
    mol = ref >= 0
    for k in range(2, 7):                                                 # read under a neighbour's box, a frame comes out differently
        for other in (boxes[k - 1], boxes[k + 1]):
            if _ortho(boxes[k]) and _ortho(other):
                a, b = W.make_molecules_whole(inputs[k], boxes[k][:3], ref)[0], W.make_molecules_whole(inputs[k], other[:3], ref)[0]
                assert (np.abs(a - b)[mol].max(1) > 1e-3).sum() > n // 4
            else:
                assert np.abs(_lattice(boxes[k]) - _lattice(other)).max() > 1.0
    s = fresh()
    st = s.make_molecules_whole_batch(2, 5)
    assert (st == 0).all()
    batch = [s.get_positions(k) for k in range(8)]
    s.close()
    for k in (0, 1, 7):
        assert _same(batch[k], inputs[k]), k
    for k in range(2, 7):
        check_molecules(batch[k], inputs[k], boxes[k], ref, ("batch", k))
    assert not _same(batch[2], batch[5]) and not _same(batch[3], batch[6])
    s = fresh()
    for k in range(2, 7):
        s.make_molecules_whole(k)
        assert _same(s.get_positions(k), batch[k]), k                     # the single-slot call: the same bits
    s.close()


@pytest.mark.parametrize("form", ["block", "gather"])
def test_first_slot_above_zero_mixed_boxes_group(G, form):
    n = 300
    idx = {"block": np.arange(3, 290), "gather": np.arange(1, 300, 3)}[form]
    boxes = _slot_boxes()
    rng = np.random.default_rng(17 + len(form))
    inputs = [blob_frame(rng, n, idx, boxes[k], [0.05 + 0.1 * k, 0.5, 0.93]) for k in range(5)]
    inputs += [inputs[2], inputs[3], inputs[4]]

    def fresh():
        s = G.System(n, n_slots=8)
        for k in range(8):
            s.set_frame(inputs[k], boxes[k], slot=k)
        s.group_create_from_indices("sel", idx)
        return s
    s = fresh()
    c, cst = s.group_center_batch("sel", 1, 0, 2, 5)
    st = s.make_group_whole_batch("sel", 2, 5)
    assert (st == 0).all() and (cst == 0).all()
    batch = [s.get_positions(k) for k in range(8)]
    s.close()
    for k in (0, 1, 7):
        assert _same(batch[k], inputs[k]), k
    for k in range(2, 7):
        if _ortho(boxes[k]):
            assert _same(batch[k], W.make_group_whole(inputs[k], idx, boxes[k][:3], c[k - 2])), k
            for other in (boxes[k - 1], boxes[k + 1]):                    # under a neighbour's box or centre: other coordinates
                if _ortho(other):
                    assert not _same(batch[k], W.make_group_whole(inputs[k], idx, other[:3], c[k - 2]))
            for j in (k - 3, k - 1):
                if 0 <= j < 5 and j != k - 2:
                    assert not _same(batch[k], W.make_group_whole(inputs[k], idx, boxes[k][:3], c[j]))
        check_group_free(batch[k], inputs[k], idx, boxes[k], (form, k))
    assert not _same(batch[2], batch[5]) and not _same(batch[3], batch[6])
    s = fresh()
    for k in range(2, 7):
        s.make_group_whole("sel", k)
        assert _same(s.get_positions(k), batch[k]), k
    s.close()


# ------------------------------------------------------------------ D: failed frames beyond the first chunk, at 1e6 atoms
WHOLE_CHUNK_BYTES = 96 << 20                # GR_WHOLE_CHUNK_BYTES (gr_whole.h)


def test_failed_frames_in_every_chunk(G):
    N = TW.N
    bonds, ref = TW._topology()
    n_pad = (N + 255) & ~255
    chunk = WHOLE_CHUNK_BYTES // (3 * 4 * n_pad)                          # frames of one chunk (molecules_whole_batch)
    nf = 2 * chunk + chunk // 2                                           # three chunks, the last one partial
    assert chunk == 8 and nf == 20
    box9, tric9 = TW._box9("ortho"), TW._box9("triclinic")
    f_first, f_mid, f_tric, f_last = 2, chunk + 4, chunk + 2, nf - 1
    chain = list(range(TW.CHAIN0, TW.CHAIN0 + TW.CHAIN_N))
    odd = list(range(TW.INTER0 + 1, TW.INTER0 + TW.INTER_N, 2))
    water = TW.INTER0 + TW.INTER_N + 3 * 200_000
    assert ref[water] == water and ref[water + 3 * 5000 + 1] == water + 3 * 5000
    # (frame: the atoms without position, the breadth-first order of the molecule the reference stops in)
    fails = {f_first: ([chain[12000], chain[700], water + 1], chain),                # the inter-tile chain; a later molecule as well
             f_mid: ([odd[150], odd[31], odd[90]], odd),                             # the odd alternating-index molecule
             f_last: ([water + 3 * 5000 + 1, water], [water, water + 1, water + 2])}  # a water's reference atom; a later water's hydrogen
    base = TW._frames(box9, ref, 4242)
    tric_in = TW._frames(tric9, ref, 4243)
    rng = np.random.default_rng(9)
    s = G.System(N, n_slots=nf)
    s.add_bonds(bonds)
    want_st, want_idx, kept = [], {}, {}
    for f in range(nf):
        if f == f_tric:
            p = tric_in
        else:                                                             # the base frame, translated
            p = (base + rng.uniform(-30.0, 30.0, 3).astype(np.float32) * np.float32(f > 0)).astype(np.float32)
        if f in fails:
            p[fails[f][0]] = np.nan
            out, err = W.make_molecules_whole(p, box9[:3], ref, [fails[f][1]])
            assert err == fails[f][0][1] and out is not p
            want_idx[f] = err
        want_st.append(E_NO_POSITION if f in fails else 0)
        s.set_frame(p, tric9 if f == f_tric else box9, slot=f)
        if f in fails or f == f_tric:
            kept[f] = p
        else:
            kept[f] = W.make_molecules_whole(p, box9[:3], ref)[0]
    st = s.make_molecules_whole_batch(0, nf, raise_on_error=False)
    assert st.tolist() == want_st
    for f in range(nf):
        got = s.get_positions(f)
        if f in fails:
            assert _same(got, kept[f]), f                                 # failed frames: untouched
            with pytest.raises(G.AtomError) as e:
                s.make_molecules_whole(f)
            assert e.value.variant == "InvalidPosition" and e.value.detail == want_idx[f], f
            assert int(s._lib.gr_last_error_index(s._ctx)) == want_idx[f]
        elif f == f_tric:
            sample = np.random.default_rng(5).choice(N, 20000, replace=False)
            sample = np.concatenate([sample[ref[sample] >= 0], [TW.CHAIN0, TW.CHAIN0 + 1, TW.CHAIN0 + TW.CHAIN_N - 1]])
            refw = {}
            for a in sample:
                r = int(ref[a])
                if r not in refw:
                    refw[r] = O.wrap(kept[f][r], tric9)
                want = refw[r] + O.vector_to(refw[r], kept[f][a], tric9)
                assert np.abs(got[a] - want).max() <= TOL, (f, a, got[a], want)
            lone = ref < 0
            assert _same(got[lone], kept[f][lone])
        else:
            bad = np.nonzero((_bits(got) != _bits(kept[f])).any(1))[0]
            assert bad.size == 0, (f, bad[:5], got[bad[:5]], kept[f][bad[:5]])
    with pytest.raises(G.AtomError) as e:                                 # the first failed frame of a batch names its atom
        s.make_molecules_whole_batch(1, nf - 1)
    assert e.value.variant == "InvalidPosition" and e.value.detail == want_idx[f_first]
    s.close()

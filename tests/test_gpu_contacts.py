"""Contacts (gr_contacts_*; groan_rs_amd.Contacts): the cut-off pair search over a block of resident frames, against two references.

1. The per-slot call on the same context, System.group_pairs_within slot by slot: i, j AND d bit-identical (np.array_equal on the f32
   arrays), in orthorhombic and in non-orthogonal boxes -- both kernels make the same call, gr_distance<4, true>(x_j, x_i, 7, box).
2. The oracle's brute force over all pairs (oracle_lib.pairs_within) per frame: indices identical and d within 1e-6 nm in orthorhombic
   boxes (the tolerance of tests/test_gpu_pairs_within.py); in non-orthogonal boxes the rule of test_pairs_within_in_non_orthogonal_boxes
   (only pairs within 2e-6 nm of the cut-off may differ, d within 2e-6).

counts and hist are checked against numpy on the call's own lists: bincount of i, and the f32 binning rule applied to d, exact."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, E_NO_BOX, E_NOT_ORTHOGONAL, E_ZERO_BOX, E_NO_POSITION, E_GROUP_NOT_FOUND, E_INVALID_ARG = 0, 1, 2, 3, 6, 8, 10


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


# ------------------------------------------------------------------ helpers
def per_slot(s, g1, g2, cutoff, slots):
    """the first reference: (offsets, i, j, d) of the per-slot call over `slots`"""
    parts = [s.group_pairs_within(g1, g2, cutoff, slot=f) for f in slots]
    off = np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.uint64)
    return off, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def slot_status(s, g1, g2, cutoff, slot):
    """(status, error index) of the per-slot call, without raising"""
    n = C.c_uint64(0)
    st = s._lib.gr_group_pairs_within(s._ctx, slot, g1.encode(), g2.encode(), C.c_float(cutoff), 0, None, None, None, C.byref(n))
    return st, int(s._lib.gr_last_error_index(s._ctx))


def same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)
               for x, y in zip(a, b))


def numpy_hist(d, cutoff, nbins):
    """the rule of GR_PD_HIST in f32: s = f32(nbins) / f32(cutoff), bin = u32(d * s), counted iff d * s < nbins"""
    s = F(nbins) / F(cutoff)
    v = (d.astype(F) * s).astype(F)
    keep = v < F(nbins)
    return np.bincount(v[keep].astype(np.uint32), minlength=nbins).astype(np.uint64)


def check_call(ct, s, g1, g2, cutoff, first, n, idx1, nbins=7):
    """pairs over slots first .. first + n - 1 == the per-slot call, bit for bit; counts and hist == numpy on the lists -> the lists"""
    n_pairs, st = ct.pairs(first, n)
    got = ct.lists()
    want = per_slot(s, g1, g2, cutoff, range(first, first + n))
    assert (st == OK).all()
    assert same_bits(got, want), (cutoff, got[0].tolist(), want[0].tolist())
    assert np.array_equal(n_pairs, np.diff(want[0])) and ct.total == int(want[0][-1])
    off, i, j, d = got
    per_atom, np2, st2 = ct.counts(first, n)
    hist, st3 = ct.hist(first, n, nbins)
    assert (st2 == OK).all() and (st3 == OK).all() and np.array_equal(np2, n_pairs)
    lookup = np.full(int(idx1.max()) + 1 if idx1.size else 1, -1, np.int64); lookup[idx1] = np.arange(idx1.size)
    for f in range(n):
        a, b = int(off[f]), int(off[f + 1])
        assert np.array_equal(per_atom[f], np.bincount(lookup[i[a:b]], minlength=idx1.size).astype(np.uint32))
        assert np.array_equal(hist[f], numpy_hist(d[a:b], cutoff, nbins))
    assert same_bits(ct.lists(), got)                         # counts and hist leave the lists alone
    return got


def check_oracle(got, frames, boxes, idx1, idx2, cutoff, stride=1):
    """the second reference, frame by frame.  The oracle is a brute force over n1 x n2 distances on the host (0.7 - 8 s per frame at the
    sizes of the random systems), and the pairs of a query do not depend on the other queries: with stride > 1 it is asked for every
    stride-th atom of group 1 (starting at the frame's number) against ALL of group 2, and the rows of those queries in the call's list
    must be its answer -- same indices, same order, d within 1e-6.  Every row of every list is still pinned bit for bit by check_call"""
    off, i, j, d = got
    for f, pos in enumerate(frames):
        a, b = int(off[f]), int(off[f + 1])
        sel = idx1[f % stride::stride] if stride > 1 else idx1
        rows = np.isin(i[a:b], sel) if stride > 1 else np.ones(b - a, bool)
        oi, oj, od = O.pairs_within(pos, sel, idx2, boxes[f], cutoff)
        assert int(rows.sum()) == oi.size, (f, cutoff, int(rows.sum()), oi.size)
        assert np.array_equal(i[a:b][rows], oi.astype(np.uint32)) and np.array_equal(j[a:b][rows], oj.astype(np.uint32))
        assert oi.size == 0 or np.abs(d[a:b][rows] - od).max() <= 1e-6


def check_oracle_near_cutoff(got, frames, boxes, idx1, idx2, cutoff):
    """the second reference in non-orthogonal boxes (test_pairs_within_in_non_orthogonal_boxes): only pairs within 2e-6 nm of the cut-off
    may differ, d within 2e-6 -> the fewest pairs the oracle found in a frame"""
    off, i, j, d = got
    fewest = None
    for f, pos in enumerate(frames):
        a, b = int(off[f]), int(off[f + 1])
        oi, oj, od = O.pairs_within(pos, idx1, idx2, boxes[f], cutoff)
        have = {(int(x), int(y)): float(v) for x, y, v in zip(i[a:b], j[a:b], d[a:b])}
        want = {(int(x), int(y)): float(v) for x, y, v in zip(oi, oj, od)}
        assert len(have) == b - a                             # no pair twice
        for key in set(have) ^ set(want):
            v = have.get(key, want.get(key))
            assert abs(v - cutoff) <= 2e-6, (f, key, v)
        common = set(have) & set(want)
        assert not common or max(abs(have[k] - want[k]) for k in common) <= 2e-6
        fewest = len(want) if fewest is None else min(fewest, len(want))
    return fewest


def jittered(pos, box, n, seed):
    """the frame, then n - 1 seeded jitters with box lengths of their own: every frame of a piece has its own grid"""
    rng = np.random.default_rng(seed)
    frames, boxes = [pos.astype(F)], [np.asarray(box, F).copy()]
    for _ in range(n - 1):
        scale = F(rng.uniform(0.93, 1.08))
        b = np.asarray(box, F).copy(); b[:3] = (b[:3] * scale).astype(F)
        frames.append((pos * scale + rng.normal(0.0, 0.02, pos.shape)).astype(F)); boxes.append(b)
    return frames, boxes


def load(G, frames, boxes):
    s = G.System(frames[0].shape[0], n_slots=len(frames))
    for f, (p, b) in enumerate(zip(frames, boxes)):
        s.set_frame(p, b, slot=f)
    return s


# ------------------------------------------------------------------ real systems
EX_GROUPS = ("Protein", "Membrane", "W", "ION")


@pytest.fixture(scope="module")
def ex(G, example):
    frames, boxes = jittered(example["pos"], example["box9"], 4, 7)
    s = load(G, frames, boxes)
    idx = {}
    for g in EX_GROUPS:
        s.group_create_from_ranges(g, [tuple(b) for b in example["blocks_" + g]])
        idx[g] = O.container_expand(example["blocks_" + g])
    yield s, frames, boxes, idx
    s.close()


@pytest.mark.parametrize("g1,g2,cutoff", [("Protein", "Membrane", 0.6), ("Protein", "Protein", 0.5), ("ION", "W", 0.8)])
def test_example_groups(G, ex, g1, g2, cutoff):
    s, frames, boxes, idx = ex
    with G.Contacts(s, g1, g2, cutoff) as ct:
        assert (ct.n1, ct.n2) == (idx[g1].size, idx[g2].size)
        got = check_call(ct, s, g1, g2, cutoff, 0, 4, idx[g1])
        check_oracle(got, frames, boxes, idx[g1], idx[g2], cutoff)
        off, i, j, d = got
        assert off[1] > 30 and (i != j).all()
        if g1 == g2:                                          # self pairs skipped, both orders present
            a = int(off[1])
            pairs = set(zip(i[:a].tolist(), j[:a].tolist()))
            assert all((y, x) in pairs for x, y in pairs)


def test_aa_protein_against_all(G):
    z = np.load(os.path.join(GOLD, "aa_full.npz"))
    frames, boxes = [z["frames"][0], z["frames"][1]], [z["boxes9"][0], z["boxes9"][1]]
    s = load(G, frames, boxes)
    s.group_create_from_ranges("protein", [(0, 362)])
    n = frames[0].shape[0]
    with G.Contacts(s, "protein", "all", 0.6) as ct:
        got = check_call(ct, s, "protein", "all", 0.6, 0, 2, np.arange(363))
        check_oracle(got, frames, boxes, np.arange(363), np.arange(n), 0.6)
        assert got[0][-1] > 10000
    s.close()


# ------------------------------------------------------------------ grid shapes
@pytest.mark.parametrize("seed", range(5))
def test_random_systems_every_grid_shape(G, seed):
    """the systems of test_gpu_pairs_within.test_random_systems_every_grid_shape, three frames with boxes of their own in one call"""
    rng = np.random.default_rng(50 + seed)
    n = int(rng.integers(3000, 9000))
    L = rng.uniform(2.0, 9.0, 3)
    if seed == 0: L[:] = [1.3, 6.0, 2.1]                                   # a slab: 1 and 2 cells along some axes
    box = np.zeros(9, F); box[:3] = L
    frames, boxes = [], []
    for f in range(3):
        b = box.copy(); b[:3] = (box[:3] * F(1.0 + 0.04 * f)).astype(F)
        frames.append((rng.uniform(-0.6, 1.6, (n, 3)) * b[:3]).astype(F)); boxes.append(b)
    s = load(G, frames, boxes)
    a = np.unique(rng.integers(0, n, n // 3)); b = np.unique(rng.integers(0, n, n // 2)); c = np.arange(100, n - 49)
    s.group_create_from_indices("A", a); s.group_create_from_indices("B", b)
    s.group_create_from_ranges("C", [(100, n - 50)])
    for cutoff in (0.35, 0.7, float(L.min() / 2.0), float(L.min() / 3.0) * 1.0001, 1.2):
        for g1, i1, g2, i2 in (("A", a, "B", b), ("C", c, "A", a)):
            with G.Contacts(s, g1, g2, cutoff) as ct:
                got = check_call(ct, s, g1, g2, cutoff, 0, 3, i1)
                check_oracle(got, frames, boxes, i1, i2, cutoff, stride=16)
    with G.Contacts(s, "all", "all", 0.3) as ct:
        got = check_call(ct, s, "all", "all", 0.3, 0, 3, np.arange(n))
        check_oracle(got, frames, boxes, np.arange(n), np.arange(n), 0.3, stride=64)
    s.close()


# ------------------------------------------------------------------ tile overflow
def test_more_candidates_than_one_tile(G):
    """group 2 holds 2 TILE + 37 atoms inside a 0.2 nm ball (one cell's candidates span three tiles) plus 2000 spread atoms; half of group 1
    sits in the ball.  The second frame moves the ball; the third call is a frame where almost every cell is empty"""
    rng = np.random.default_rng(3)
    probe = G.System(4, n_slots=1); probe.set_frame(np.zeros((4, 3), F), [3, 3, 3]); probe.group_create_from_ranges("a", [(0, 3)])
    with G.Contacts(probe, "a", "a", 0.3) as ct:
        tile = ct.stat(G._lib.CT_STAT_TILE)
    probe.close()
    assert tile >= 64
    nb = 2 * tile + 37
    n = nb + 2000 + 300
    box = np.array([6.0, 5.0, 7.0, 0, 0, 0, 0, 0, 0], F)

    def ball(m, centre):
        v = rng.normal(size=(m, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
        return centre + v * (0.2 * rng.uniform(0, 1, (m, 1)) ** (1 / 3))

    frames = []
    for centre in (np.array([2.0, 2.0, 2.0]), np.array([5.9, 0.05, 6.95])):          # (the second ball straddles the periodic corner)
        pos = np.empty((n, 3))
        pos[:nb] = ball(nb, centre)
        pos[nb:nb + 2000] = rng.uniform(0, 1, (2000, 3)) * box[:3]
        pos[nb + 2000:nb + 2150] = ball(150, centre)
        pos[nb + 2150:] = rng.uniform(0, 1, (150, 3)) * box[:3]
        frames.append(pos.astype(F))
    sparse = np.full((n, 3), 0.1, F) + rng.uniform(0, 0.05, (n, 3)).astype(F)        # everything in one corner of a large cell
    sparse[::7] = (rng.uniform(0, 1, (sparse[::7].shape[0], 3)) * 30.0).astype(F)
    frames.append(sparse)
    boxes = [box, box, np.array([30.0, 30.0, 30.0, 0, 0, 0, 0, 0, 0], F)]
    s = load(G, frames, boxes)
    s.group_create_from_ranges("two", [(0, nb + 1999)]); s.group_create_from_ranges("one", [(nb + 2000, n - 1)])
    i1, i2 = np.arange(nb + 2000, n), np.arange(0, nb + 2000)
    with G.Contacts(s, "one", "two", 0.3) as ct:
        got = check_call(ct, s, "one", "two", 0.3, 0, 2, i1, nbins=64)
        check_oracle(got, frames[:2], boxes[:2], i1, i2, 0.3)
        per_atom, _, _ = ct.counts(0, 2)
        assert per_atom.max() > 2 * tile                     # one query's hits come from three tiles
        got = check_call(ct, s, "one", "two", 0.3, 2, 1, i1)
        check_oracle(got, frames[2:], boxes[2:], i1, i2, 0.3)
    s.close()


# ------------------------------------------------------------------ exact edges
def test_exact_edges(G):
    """d == cutoff exactly: in the list, outside the histogram; coincident atoms: d == 0, bin 0; an atom of both groups never pairs itself"""
    pos = np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0], [3.0, 3.0, 3.0], [3.0, 3.0, 3.0], [5.0, 5.0, 1.0]], F)
    s = G.System(5, n_slots=1); s.set_frame(pos, [8.0, 8.0, 8.0])
    s.group_create_from_ranges("all5", [(0, 4)])
    with G.Contacts(s, "all5", "all5", 0.5) as ct:
        n_pairs, _ = ct.pairs(0, 1)
        off, i, j, d = ct.lists()
        assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (1, 0), (2, 3), (3, 2)] and int(n_pairs[0]) == 4
        assert d.tolist() == [0.5, 0.5, 0.0, 0.0]
        assert same_bits((off, i, j, d), per_slot(s, "all5", "all5", 0.5, [0]))
        hist, _ = ct.hist(0, 1, 4)
        assert hist[0].tolist() == [2, 0, 0, 0]               # the two pairs at 0.5 fall outside [0, cutoff)
        per_atom, n2, _ = ct.counts(0, 1)
        assert per_atom[0].tolist() == [1, 1, 1, 1, 0] and int(n2[0]) == 4
    s.close()


# ------------------------------------------------------------------ non-orthogonal boxes
@pytest.mark.parametrize("lengths,angles,cutoff", [([7.0, 6.5, 6.0], [75.0, 80.0, 70.0], 0.45), ([6.0, 6.0, 6.0], [60.0, 60.0, 90.0], 0.6),
                                                   ([6.0, 6.0, 6.0], [70.53, 109.47, 70.53], 1.3), ([6.5, 7.5, 6.0], [100.0, 95.0, 110.0], 2.4),
                                                   ([8.0, 7.0, 3.0], [60.0, 70.0, 80.0], 0.9)])
def test_non_orthogonal_boxes(G, lengths, angles, cutoff):
    """the boxes and cut-offs of test_pairs_within_in_non_orthogonal_boxes, 3000 atoms, 2 frames.  Against the per-slot call everything is
    bit-identical: the walk makes k_cg_pairs' call, gr_distance<4, true>(x_j, x_i, 7, box), whose triclinic path is explicit fmaf and
    single operations plus sums that the compiler contracts per expression, alike in both kernels.  Against the oracle the rule of that
    test: only pairs within 2e-6 nm of the cut-off may differ, d within 2e-6"""
    from groan_rs_amd import workload as W
    box = W.box_from_lengths_angles(lengths, angles)
    Lm = np.array([[box[0], 0, 0], [box[5], box[1], 0], [box[7], box[8], box[2]]], np.float64)
    rng = np.random.default_rng(int(cutoff * 100))
    n = 3000
    frames = [(rng.uniform(-0.4, 1.4, (n, 3)) @ Lm).astype(F) for _ in range(2)]
    boxes = [box, box]
    s = load(G, frames, boxes)
    i1 = np.arange(0, 800); i2 = np.unique(np.concatenate([np.arange(500, n, 2), np.arange(1500, 1600)]))
    s.group_create_from_ranges("A", [(0, 799)]); s.group_create_from_indices("B", i2.tolist())
    with G.Contacts(s, "A", "B", cutoff) as ct:
        off, i, j, d = check_call(ct, s, "A", "B", cutoff, 0, 2, i1)
    assert check_oracle_near_cutoff((off, i, j, d), frames, boxes, i1, i2, cutoff) > 300
    s.close()


# ------------------------------------------------------------------ statuses
def test_statuses_of_a_mixed_batch(G, example):
    pos, box = example["pos"][:2000].copy(), example["box9"]
    bad2 = pos.copy(); bad2[700, 0] = np.nan; bad2[20, 0] = np.nan
    bad1 = pos.copy(); bad1[20, 0] = np.nan
    good2 = (pos + F(0.01)).astype(F)
    frames = [pos, pos, pos, bad2, bad1, good2]
    s = G.System(2000, n_slots=6)
    for f, p in enumerate(frames):
        s.set_frame(p, box, slot=f)
    s.reset_box(slot=1)
    s.set_box(np.zeros(9, F), slot=2)
    s.group_create_from_ranges("A", [(0, 99)]); s.group_create_from_ranges("B", [(50, 1999)])
    want_st = [slot_status(s, "A", "B", 0.5, f) for f in range(6)]
    assert [w[0] for w in want_st] == [OK, E_NO_BOX, E_ZERO_BOX, E_NO_POSITION, E_NO_POSITION, OK]
    assert want_st[3][1] == 700 and want_st[4][1] == 20       # the grid (group 2) is built first
    with G.Contacts(s, "A", "B", 0.5) as ct:
        n_pairs = np.zeros(6, np.uint64); st = np.zeros(6, np.int32); total = C.c_uint64(0)
        ret = ct._lib.gr_contacts_pairs_batch(ct._ct, 0, 6, 2 ** 64 - 1, n_pairs.ctypes.data_as(C.c_void_p), C.byref(total), st.ctypes.data_as(C.c_void_p))
        assert st.tolist() == [w[0] for w in want_st]
        assert ret == E_NO_BOX and s._lib.gr_last_error(s._ctx) == b"simulation box does not exist"     # the first error is the return value
        off, i, j, d = ct.lists()
        assert n_pairs[1:5].tolist() == [0, 0, 0, 0] and off[1] == off[5] and n_pairs[0] > 100 and n_pairs[5] > 100
        # every frame on its own: status and index as the per-slot call raises them
        for f in range(6):
            one = np.zeros(1, np.int32)
            r = ct._lib.gr_contacts_pairs_batch(ct._ct, f, 1, 2 ** 64 - 1, None, None, one.ctypes.data_as(C.c_void_p))
            assert (r, int(one[0])) == (want_st[f][0], want_st[f][0])
            if r == E_NO_POSITION:
                assert int(s._lib.gr_last_error_index(s._ctx)) == want_st[f][1]
        with pytest.raises(G.GroupError) as e:
            ct.pairs(3, 2)
        assert e.value.variant == "InvalidPosition" and e.value.detail == 700
        # failed frames: zero rows
        per_atom, np2, st2 = ct.counts(0, 6, raise_on_error=False)
        hist, st3 = ct.hist(0, 6, 16, raise_on_error=False)
        assert st2.tolist() == st.tolist() == st3.tolist()
        for f in (1, 2, 3, 4):
            assert not per_atom[f].any() and not hist[f].any() and np2[f] == 0
        assert hist[0].sum() > 0 and per_atom[5].sum() == n_pairs[5]
        # the good frames are what they are without the bad ones
        mixed = ct._lib.gr_contacts_pairs_batch(ct._ct, 0, 6, 2 ** 64 - 1, None, None, None)
        assert mixed == E_NO_BOX
        off, i, j, d = ct.lists()
        a, b = int(off[5]), int(off[6])
        want0, want5 = per_slot(s, "A", "B", 0.5, [0]), per_slot(s, "A", "B", 0.5, [5])
        assert same_bits((i[:int(off[1])], j[:int(off[1])], d[:int(off[1])]), want0[1:]) and same_bits((i[a:b], j[a:b], d[a:b]), want5[1:])
        ct.pairs(0, 1)
        assert same_bits(ct.lists(), want0)
    s.close()


def test_strict_mode_empty_groups_and_create_errors(G, example):
    pos, box = example["pos"][:2000].copy(), example["box9"]
    nan = pos.copy(); nan[::3, 0] = np.nan
    s = G.System(2000, n_slots=2)
    s.set_frame(pos, np.array([13.0, 13.0, 11.0, 0, 0, 1.0, 0, 0, 0], F), slot=0)
    s.set_frame(nan, box, slot=1)
    s.group_create_from_ranges("A", [(0, 99)]); s.group_create_from_ranges("B", [(50, 1999)]); s.group_create_from_indices("E", [])
    with G.Contacts(s, "A", "B", 0.5) as ct:
        s.set_strict_orthogonal(True)                         # the reference's gate (cellgrid.rs:423)
        n_pairs, st = ct.pairs(0, 1, raise_on_error=False)
        assert st.tolist() == [E_NOT_ORTHOGONAL] == [slot_status(s, "A", "B", 0.5, 0)[0]] and n_pairs[0] == 0
        with pytest.raises(G.GroupError) as e:
            ct.pairs(0, 1)
        assert e.value.variant == "InvalidSimBox" and e.value.detail.variant == "NotOrthogonal"
        s.set_strict_orthogonal(False)
        n_pairs, st = ct.pairs(0, 1)
        assert st[0] == OK and same_bits(ct.lists(), per_slot(s, "A", "B", 0.5, [0]))
    # an empty group on either side: OK and 0 pairs, even where positions are missing
    for g1, g2 in (("E", "B"), ("A", "E"), ("E", "E")):
        assert slot_status(s, g1, g2, 0.5, 1)[0] == OK
        with G.Contacts(s, g1, g2, 0.5) as ct:
            n_pairs, st = ct.pairs(0, 2)
            assert st.tolist() == [OK, OK] and n_pairs.tolist() == [0, 0] and ct.total == 0
            off, i, j, d = ct.lists()
            assert off.tolist() == [0, 0, 0] and i.size == 0
            per_atom, np2, st2 = ct.counts(0, 2)
            hist, st3 = ct.hist(0, 2, 5)
            assert per_atom.shape == (2, ct.n1) and not per_atom.any() and not hist.any() and (st2 == OK).all() and (st3 == OK).all()
    with pytest.raises(G.GroupError) as e:
        G.Contacts(s, "nope", "alsonope", 0.5)
    assert e.value.variant == "NotFound" and e.value.detail == "nope"                 # group1 is looked up first
    with pytest.raises(G.GroupError) as e:
        G.Contacts(s, "A", "nope", 0.5)
    assert e.value.variant == "NotFound"
    for cutoff in (0.0, -1.0, float("nan")):
        with pytest.raises(G.GroanError) as e:
            G.Contacts(s, "A", "B", cutoff)
        assert e.value.status == E_INVALID_ARG and s._lib.gr_last_error(s._ctx) == b"cell size (cut-off) must be positive"
    s.close()


# ------------------------------------------------------------------ pieces and segments
@pytest.fixture(scope="module")
def seven(G, example):
    frames, boxes = jittered(example["pos"][:5000], example["box9"], 7, 11)
    s = load(G, frames, boxes)
    s.group_create_from_ranges("A", [(0, 1499)]); s.group_create_from_indices("B", np.arange(1000, 5000, 2))
    yield s
    s.close()


def test_piece_sizes_give_the_same_bits(G, seven):
    s = seven
    with G.Contacts(s, "A", "B", 0.7) as ct:
        ct.pairs(0, 7)
        base = ct.lists()
        assert ct.stat(G._lib.CT_STAT_LAST_PIECES) == 1 and same_bits(base, per_slot(s, "A", "B", 0.7, range(7)))
        c0, h0 = ct.counts(0, 7)[0], ct.hist(0, 7, 33)[0]
        for piece, pieces in ((1, 7), (2, 4), (3, 3), (0, 1)):
            ct.set_piece_frames(piece)
            ct.pairs(0, 7)
            assert ct.stat(G._lib.CT_STAT_LAST_PIECES) == pieces and same_bits(ct.lists(), base)
            assert np.array_equal(ct.counts(0, 7)[0], c0) and np.array_equal(ct.hist(0, 7, 33)[0], h0)


def test_across_the_1024_frame_segment(G):
    rng = np.random.default_rng(5)
    n, nf = 96, 1030
    s = G.System(n, n_slots=nf)
    for f in range(nf):
        L = F(2.0 + 0.001 * (f % 37))
        s.set_frame((rng.uniform(-0.2, 1.2, (n, 3)) * L).astype(F), [L, L, L], slot=f)
    s.group_create_from_ranges("A", [(0, 59)]); s.group_create_from_ranges("B", [(30, 95)])
    with G.Contacts(s, "A", "B", 0.45) as ct:
        n_pairs, st = ct.pairs(0, nf)
        off, i, j, d = ct.lists()
        assert (st == OK).all() and off.size == nf + 1 and (np.diff(off.astype(np.int64)) >= 0).all() and np.array_equal(np.diff(off), n_pairs)
        assert n_pairs.min() > 0
        a, b = int(off[1022]), int(off[1026])
        want = per_slot(s, "A", "B", 0.45, range(1022, 1026))
        assert same_bits((off[1022:1027] - off[1022], i[a:b], j[a:b], d[a:b]), want)
        per_atom, np2, _ = ct.counts(0, nf)
        assert np.array_equal(np2, n_pairs) and np.array_equal(per_atom.sum(1).astype(np.uint64), n_pairs)
    s.close()


def test_launches_per_piece_do_not_depend_on_the_frames(G):
    rng = np.random.default_rng(9)
    n = 400
    s = G.System(n, n_slots=64)
    for f in range(64):
        s.set_frame((rng.uniform(0, 1, (n, 3)) * 3.0).astype(F), [3.0, 3.0, 3.0], slot=f)
    s.group_create_from_ranges("A", [(0, 199)]); s.group_create_from_ranges("B", [(100, 399)])
    with G.Contacts(s, "A", "B", 0.5) as ct:
        per_piece = {}
        for nf in (2, 64):
            for name, call in (("pairs", lambda: ct.pairs(0, nf)), ("counts", lambda: ct.counts(0, nf)), ("hist", lambda: ct.hist(0, nf, 10))):
                call()
                assert ct.stat(G._lib.CT_STAT_LAST_PIECES) == 1
                per_piece.setdefault(name, []).append(ct.stat(G._lib.CT_STAT_LAST_LAUNCHES))
        assert all(v[0] == v[1] and v[0] > 0 for v in per_piece.values()), per_piece
        ct.set_piece_frames(16)
        ct.pairs(0, 64)
        assert ct.stat(G._lib.CT_STAT_LAST_PIECES) == 4 and ct.stat(G._lib.CT_STAT_LAST_LAUNCHES) == 4 * per_piece["pairs"][0]
    s.close()


# ------------------------------------------------------------------ max_pairs
def test_max_pairs_counts_only(G, seven):
    s = seven
    want = per_slot(s, "A", "B", 0.7, range(3))
    total = int(want[0][-1])
    with G.Contacts(s, "A", "B", 0.7) as ct:
        for piece in (0, 1):                                  # (with pieces of one frame the first pieces fit and are dropped later)
            ct.set_piece_frames(piece)
            n_pairs, st = ct.pairs(0, 3, max_pairs=total - 1)
            assert (st == OK).all() and np.array_equal(n_pairs, np.diff(want[0])) and ct.total == total
            assert np.array_equal(ct.offsets(), want[0])
            buf = np.zeros(total, np.uint32); dbuf = np.zeros(total, F); tot = C.c_uint64(0)
            args = [x.ctypes.data_as(C.c_void_p) for x in (buf, buf.copy(), dbuf)]
            assert ct._lib.gr_contacts_read(ct._ct, None, *args, total, C.byref(tot)) == E_INVALID_ARG and tot.value == total
            assert ct._lib.gr_contacts_read(ct._ct, None, None, None, None, 0, C.byref(tot)) == OK and tot.value == total       # NULL lists: totals only
            with pytest.raises(G.GroanError):
                ct.lists()
            ct.pairs(0, 3, max_pairs=total)                   # the next call with room writes the lists
            assert same_bits(ct.lists(), want)
            assert ct._lib.gr_contacts_read(ct._ct, None, *args, total - 1, None) == E_INVALID_ARG                             # cap < total


# ------------------------------------------------------------------ state and history
def test_history_does_not_change_the_bits(G, seven):
    s = seven
    want = per_slot(s, "A", "B", 0.7, range(2, 5))
    with G.Contacts(s, "A", "B", 0.7) as ct, G.Contacts(s, "B", "A", 0.4) as other:
        ct.pairs(2, 3); first = ct.lists()
        assert same_bits(first, want)
        ct.pairs(2, 3); assert same_bits(ct.lists(), first)                           # the same call twice
        other.pairs(0, 7); other_first = other.lists()
        ct.pairs(0, 7); ct.pairs(2, 3); assert same_bits(ct.lists(), first)           # after a larger call (workspace grown)
        with pytest.raises(G.GroanError):
            ct.pairs(5, 10)                                                           # a refused call: slots out of range
        assert ct.lists()[0].tolist() == [0] and ct.total == 0                        # ... leaves an empty result of 0 frames
        ct.pairs(2, 3); assert same_bits(ct.lists(), first)
        ct.hist(0, 7, 100); ct.counts(0, 7)
        s.group_center_batch("A", G._lib.CENTER_PBC, 0, 0, 7)
        with G.Region(s, [G.Sphere([2.0, 2.0, 2.0], 1.5)]) as rg:
            rg.select("B", 0, 7)
        ct.pairs(2, 3); assert same_bits(ct.lists(), first)
        other.pairs(0, 7); assert same_bits(other.lists(), other_first)               # two objects on one context
        assert same_bits(other_first, per_slot(s, "B", "A", 0.4, range(7)))
        # the snapshot: replacing the group after create changes nothing
        s.group_create_from_ranges("A", [(0, 10)])
        ct.pairs(2, 3); assert same_bits(ct.lists(), first)
        s.group_create_from_ranges("A", [(0, 1499)])


# ------------------------------------------------------------------ hist
def test_hist_bins(G, seven):
    s = seven
    with G.Contacts(s, "A", "B", 0.7) as ct:
        ct.pairs(0, 2)
        off, i, j, d = ct.lists()
        for nbins in (1, 7, 4096):
            hist, st = ct.hist(0, 2, nbins)
            assert hist.shape == (2, nbins) and hist.dtype == np.uint64
            for f in range(2):
                assert np.array_equal(hist[f], numpy_hist(d[int(off[f]):int(off[f + 1])], 0.7, nbins))
        out = np.zeros(4097, np.uint64)
        for bad in (0, 4097):
            assert ct._lib.gr_contacts_hist_batch(ct._ct, 0, 1, bad, out.ctypes.data_as(C.c_void_p), None) == E_INVALID_ARG
            with pytest.raises(ValueError):
                ct.hist(0, 1, bad)

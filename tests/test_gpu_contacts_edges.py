"""Contacts at the edges of k_ct_walk (gr_contacts.h): candidate counts at and around the LDS tile, candidate and query counts at and around
a team's round, every run length against every row length, and one workgroup that serves many runs and frames.

Every case is checked twice, as in test_gpu_contacts.py, whose helpers these are: pairs / counts / hist bit for bit against
System.group_pairs_within per slot (check_call), and every query of every frame against the oracle's brute force (check_oracle with
stride 1: the same indices in the same order, d within 1e-6 nm; in non-orthogonal cells check_oracle_near_cutoff).  The systems hold tens to
hundreds of atoms, so nothing is sampled.  Positions are drawn well outside the cell (or moved by whole box vectors), so wrapping matters.

What a case hits is known by construction and confirmed by the object's own statistics (gr_contacts_stat): the cells and runs of the last
call and its query cells per run are read back, not recomputed."""
import numpy as np
import pytest

from test_gpu_contacts import G, OK, check_call, check_oracle, check_oracle_near_cutoff, load, numpy_hist, per_slot, same_bits, slot_status     # noqa: F401 (G: the fixture)

pytestmark = pytest.mark.gpu
F = np.float32
CUTOFF = 0.5
ONE_CELL, CELLS_27 = [0.9, 0.9, 0.9], [1.6, 1.6, 1.6]       # floor(L / cutoff) = 1 and 3 cells per axis; with 3 every row is `whole`: M = n2 in every run


@pytest.fixture(scope="module")
def tile(G):
    probe = G.System(4, n_slots=1); probe.set_frame(np.zeros((4, 3), F), [3, 3, 3]); probe.group_create_from_ranges("a", [(0, 3)])
    with G.Contacts(probe, "a", "a", 0.3) as ct:
        t = ct.stat(G._lib.CT_STAT_TILE)
    probe.close()
    assert t >= 64 and t % 32 == 0
    return t


def box9(lengths):
    b = np.zeros(9, F); b[:3] = lengths
    return b


def cell_rows(box):
    """rows = the box vectors"""
    return np.array([[box[0], 0, 0], [box[5], box[1], 0], [box[7], box[8], box[2]]], np.float64)


def spread(rng, n, box):
    """uniform over more than the cell: fractional coordinates in (-0.6, 1.6)"""
    return rng.uniform(-0.6, 1.6, (n, 3)) @ cell_rows(box)


def ball(rng, n, centre, box, radius=0.2):
    """inside a ball, every atom then moved by whole box vectors of its own"""
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    return np.asarray(centre) + v * (radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) + rng.integers(-1, 2, (n, 3)) @ cell_rows(box)


def stats(G, ct):
    L = G._lib
    return {k: ct.stat(getattr(L, "CT_STAT_LAST_" + k)) for k in ("RUNS", "CELLS", "RUN_CELLS_MIN", "RUN_CELLS_MAX", "WALK_GROUPS", "LAUNCHES", "PIECES")}


def two_ranges(G, pos, box, n1):
    """one frame; "q" = the first n1 atoms, "c" = the others -> (system, idx1, idx2)"""
    s = load(G, [pos.astype(F)], [box])
    n = pos.shape[0]
    s.group_create_from_ranges("q", [(0, n1 - 1)]); s.group_create_from_ranges("c", [(n1, n - 1)])
    return s, np.arange(n1), np.arange(n1, n)


# ------------------------------------------------------------------ 1. the tile
def tile_sizes(t):
    return [t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 2 * t + 17]


@pytest.mark.parametrize("lengths,cells", [(ONE_CELL, 1), (CELLS_27, 27)], ids=["1_cell", "27_cells"])
def test_tile_boundaries(G, tile, lengths, cells):
    """M = n2 candidates in every run: one cell, or 3 x 3 x 3 cells whose rows are all `whole` (27 runs of one query cell; the tile boundary
    then falls inside one of the 9 ranges or between two).  M == TILE: one tile, no final sort; TILE + 1: a last tile of one candidate;
    2 TILE: two full tiles.  Spread: about an eighth of the candidates hit in the larger cell (most in the smaller); dense: both groups in
    one 0.2 nm ball across a cell corner, so every query hits every candidate and the final per-query sort sees n = M"""
    box, n1 = box9(lengths), 37
    for k, n2 in enumerate(tile_sizes(tile)):
        for dense in (False, True):
            rng = np.random.default_rng(100 * cells + 2 * k + dense)
            pos = ball(rng, n1 + n2, np.asarray(lengths) / 3.0 + 0.01, box) if dense else spread(rng, n1 + n2, box)
            s, i1, i2 = two_ranges(G, pos, box, n1)
            with G.Contacts(s, "q", "c", CUTOFF) as ct:
                got = check_call(ct, s, "q", "c", CUTOFF, 0, 1, i1)
                st = stats(G, ct)
                assert (st["CELLS"], st["RUNS"], st["RUN_CELLS_MIN"], st["RUN_CELLS_MAX"]) == (cells, cells, 1, 1), (n2, st)
                check_oracle(got, [pos.astype(F)], [box], i1, i2, CUTOFF)
                per_atom, n_pairs, _ = ct.counts(0, 1)
                if dense:
                    assert per_atom.min() == per_atom.max() == n2
                else:
                    assert 0 < int(n_pairs[0]) < n1 * n2
            s.close()


@pytest.mark.parametrize("lengths,cells", [(ONE_CELL, 1), (CELLS_27, 27)], ids=["1_cell", "27_cells"])
def test_tile_boundaries_same_group(G, tile, lengths, cells):
    """one table: a query is its own candidate, in whichever tile holds it, and must be skipped there"""
    box = box9(lengths)
    for k, n in enumerate((tile, tile + 1, 2 * tile + 1)):
        rng = np.random.default_rng(300 + 10 * cells + k)
        pos = ball(rng, n, np.asarray(lengths) / 3.0 + 0.01, box)
        s = load(G, [pos.astype(F)], [box])
        s.group_create_from_ranges("g", [(0, n - 1)])
        with G.Contacts(s, "g", "g", CUTOFF) as ct:
            off, i, j, d = got = check_call(ct, s, "g", "g", CUTOFF, 0, 1, np.arange(n))
            assert stats(G, ct)["CELLS"] == cells
            check_oracle(got, [pos.astype(F)], [box], np.arange(n), np.arange(n), CUTOFF)
            per_atom, _, _ = ct.counts(0, 1)
            assert per_atom.min() == per_atom.max() == n - 1 and i.size == n * (n - 1) and (i != j).all()
            key = i.astype(np.uint64) * n + j                # both orders of every pair, each once: all of the n (n - 1) ordered pairs
            assert np.unique(key).size == key.size and np.array_equal(np.sort(key), np.sort(j.astype(np.uint64) * n + i))
        s.close()


def test_tile_boundaries_triclinic(G, tile):
    from groan_rs_amd import workload as W
    box = W.box_from_lengths_angles([1.7, 1.7, 1.7], [75.0, 80.0, 70.0])
    n1, n2 = 37, 2 * tile + 1
    rng = np.random.default_rng(77)
    pos = ball(rng, n1 + n2, cell_rows(box).sum(0) / 3.0 + 0.01, box)
    s, i1, i2 = two_ranges(G, pos, box, n1)
    with G.Contacts(s, "q", "c", CUTOFF) as ct:
        got = check_call(ct, s, "q", "c", CUTOFF, 0, 1, i1)
        assert check_oracle_near_cutoff(got, [pos.astype(F)], [box], i1, i2, CUTOFF) >= n1 * n2 - 4
        per_atom, _, _ = ct.counts(0, 1)
        assert per_atom.max() == n2
    s.close()


# ------------------------------------------------------------------ 2. teams and rounds
N2_TEAM = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65)       # a team tests 16 candidates per lane step, 32 per round
N1_TEAM = (1, 2, 3, 4, 5, 9)                                # four teams per workgroup: the invalid teams of the last step must add nothing to the ballots
N_TEAM = 120
FAR = 0.75 / np.sqrt(3.0)                                   # 0.75 nm along the cell's diagonal, the one direction in which a 0.9 nm cell has room: 0.6 nm or more by the nearest image


def team_frames():
    """three arrangements of one system in the one-cell box.  all-hit: everything in one 0.2 nm ball; gapped: the even atoms of 0 .. 65 in
    the ball and the odd ones 0.75 nm away (a team's ballot words alternate); none: all of 0 .. 65 away.  The queries, taken from the
    tail, are in the ball"""
    rng = np.random.default_rng(21)
    box = box9(ONE_CELL)
    centre = np.array([0.3, 0.35, 0.3])
    base = ball(rng, N_TEAM, centre, box)
    away = ball(rng, N_TEAM, centre + FAR, box, radius=0.01)
    gapped, none = base.copy(), base.copy()
    gapped[1:66:2] = away[1:66:2]
    none[:66] = away[:66]
    return [x.astype(F) for x in (base, gapped, none)], [box] * 3


def test_team_and_round_edges(G):
    frames, boxes = team_frames()
    s = load(G, frames, boxes)
    for n2 in N2_TEAM:
        s.group_create_from_ranges("c%d" % n2, [(0, n2 - 1)])
    for n1 in N1_TEAM:
        s.group_create_from_ranges("q%d" % n1, [(N_TEAM - n1, N_TEAM - 1)])
    for n1 in N1_TEAM:
        i1 = np.arange(N_TEAM - n1, N_TEAM)
        for n2 in N2_TEAM:
            i2 = np.arange(n2)
            g1, g2 = "q%d" % n1, "c%d" % n2
            with G.Contacts(s, g1, g2, CUTOFF) as ct:
                for f, hits in enumerate((n2, (n2 + 1) // 2, 0)):
                    got = check_call(ct, s, g1, g2, CUTOFF, f, 1, i1, nbins=5)
                    check_oracle(got, frames[f:f + 1], boxes[f:f + 1], i1, i2, CUTOFF)
                    per_atom, n_pairs, _ = ct.counts(f, 1)
                    assert (per_atom == hits).all() and int(n_pairs[0]) == n1 * hits, (n1, n2, f, per_atom.tolist())
                    if f == 1:
                        assert (got[2] % 2 == 0).all()       # the even ordinals, and only they
                    if f == 2:
                        hist, _ = ct.hist(f, 1, 5)
                        assert ct.total == 0 and got[1].size == 0 and got[0].tolist() == [0, 0] and not hist.any()
                st = stats(G, ct)
                assert (st["CELLS"], st["RUNS"]) == (1, 1)
    s.close()


# ------------------------------------------------------------------ 3. run lengths against row lengths
PER_CELL = (8.0, 6.5, 5.5, 4.5, 3.9, 3.4, 3.0, 2.5)         # candidates per cell at which ct_run_cells should give 1 .. 8 query cells per run: observed below, not assumed
ROWS = range(3, 14)
N1_ROWS = 60


def row_cases(G, box, sizes, near_cutoff=False):
    """one frame spread over `box`; "q" = the first 60 atoms, for every n2 of `sizes` the candidates are the n2 atoms behind them -> the
    stats of each call"""
    n1, out = N1_ROWS, []
    rng = np.random.default_rng(int(1000 * float(box[0])) + max(sizes))
    pos = spread(rng, n1 + max(sizes), box).astype(F)
    s = load(G, [pos], [box])
    s.group_create_from_ranges("q", [(0, n1 - 1)])
    i1 = np.arange(n1)
    for n2 in sizes:
        s.group_create_from_ranges("c", [(n1, n1 + n2 - 1)])
        i2 = np.arange(n1, n1 + n2)
        with G.Contacts(s, "q", "c", CUTOFF) as ct:
            got = check_call(ct, s, "q", "c", CUTOFF, 0, 1, i1)
            st = stats(G, ct)
            if near_cutoff:
                assert check_oracle_near_cutoff(got, [pos], [box], i1, i2, CUTOFF) > n1
            else:
                check_oracle(got, [pos], [box], i1, i2, CUTOFF)
                assert int(got[0][-1]) > n1
        assert st["RUN_CELLS_MIN"] == st["RUN_CELLS_MAX"], st
        out.append(st)
    s.close()
    return out


def test_run_lengths_against_row_lengths(G):
    """a grid of nc0 x 3 x 3 cells, nc0 = 3 .. 13, and runs of rx = 1 .. min(8, nc0) query cells: nc0 - rx is 0, 1, 2, 3 and more, so a row has
    only `whole` runs (run + 2 neighbours cover the row: one range), none (three parts, two of them the periodic wrap), or both (a
    clipped last run).  rx and the cell count are the call's own (gr_contacts_stat), and the sweep must have met every rx with every
    difference that rows of 3 .. 13 cells allow"""
    seen = set()
    for nc0 in ROWS:
        box = box9([nc0 * 0.51, 1.53, 1.53])
        for st in row_cases(G, box, [int(round(p * 9 * nc0)) for p in PER_CELL]):
            rx = st["RUN_CELLS_MAX"]
            assert st["CELLS"] == 9 * nc0 and 1 <= rx <= min(8, nc0) and st["RUNS"] == 9 * ((nc0 + rx - 1) // rx), (nc0, st)
            seen.add((rx, min(nc0 - rx, 4)))
    want = set((rx, min(nc0 - rx, 4)) for rx in range(1, 9) for nc0 in ROWS if nc0 >= rx)
    assert seen >= want, sorted(want - seen)


@pytest.mark.parametrize("nc,p", [(7, 8.0), (10, 4.5), (13, 2.5)])
def test_run_lengths_with_the_long_rows_along_y(G, nc, p):
    """x and y exchanged: rows of 3 cells, nc rows per layer -- the neighbour rows wrap along y"""
    st, = row_cases(G, box9([1.53, nc * 0.51, 1.53]), [int(round(p * 9 * nc))])
    assert st["CELLS"] == 9 * nc and st["RUN_CELLS_MAX"] <= 3 and st["RUNS"] == 3 * nc * ((3 + st["RUN_CELLS_MAX"] - 1) // st["RUN_CELLS_MAX"]), st


@pytest.mark.parametrize("nc0,p", [(5, 6.5), (9, 3.4)])
def test_run_lengths_in_a_triclinic_cell(G, nc0, p):
    """the same grid counts in a skewed cell (heights 0.514 nc0, 1.58 and 1.6 nm between the faces)"""
    box = np.array([nc0 * 0.51 * 1.03, 1.6, 1.6, 0, 0, 0.3, 0, 0.2, 0.25], F)
    st, = row_cases(G, box, [int(round(p * 9 * nc0))], near_cutoff=True)
    assert st["CELLS"] == 9 * nc0 and 1 < st["RUN_CELLS_MAX"] < nc0, st


# ------------------------------------------------------------------ 4. one workgroup, many runs, several frames
E_NO_BOX, E_NO_POSITION = 1, 6


def strided_world(G, tile):
    """six slots with three different cells.  A = atoms 0 .. 199, B = the odd atoms from 150 on (the odd atoms of 150 .. 199 are in both).
    Slot 1 holds 2 TILE + 5 atoms of B and 20 of A in one 0.2 nm ball: a run of more than two tiles; slot 3 has an atom of A without
    position, slot 4 no box.  B needs room for the ball: 700 atoms and two more per atom of the ball"""
    nball = 2 * tile + 5
    n = 700 + 2 * nball
    a, b = np.arange(200), np.arange(151, n, 2)
    lengths = [[2.1, 2.1, 2.1], [2.6, 2.6, 2.6], [3.3, 2.2, 1.7]] * 2
    rng = np.random.default_rng(44)
    frames, boxes = [], []
    for f, L in enumerate(lengths):
        box = box9(L)
        pos = spread(rng, n, box)
        if f == 1:
            centre = np.array([1.05, 1.57, 0.5])
            pos[b[-nball:]] = ball(rng, nball, centre, box)
            pos[:20] = ball(rng, 20, centre, box)
        if f == 3:
            pos[7] = np.nan
        frames.append(pos.astype(F)); boxes.append(box)
    s = load(G, frames, boxes)
    s.reset_box(slot=4)
    s.group_create_from_ranges("A", [(0, 199)]); s.group_create_from_indices("B", b)
    return s, frames, boxes, a, b, nball


def test_one_workgroup_serves_many_runs_and_frames(G, tile):
    """gr_contacts_set_walk_groups caps the walk's grid, so a workgroup takes several runs in turn and crosses from frame to frame: the HIST
    walk flushes its bins when its frame changes and once more behind the loop, the WRITE walk skips the runs of a frame with a missing
    position, and a run of three tiles is met in the middle of the loop.  Whatever the cap, the pieces and the bins: the default call's
    bits, which are the per-slot call's and the oracle's"""
    s, frames, boxes, a, b, nball = strided_world(G, tile)
    L = G._lib
    want_st = [slot_status(s, "A", "B", CUTOFF, f)[0] for f in range(6)]
    assert want_st == [OK, OK, OK, E_NO_POSITION, E_NO_BOX, OK]
    good = [f for f in range(6) if want_st[f] == OK]
    want = {f: per_slot(s, "A", "B", CUTOFF, [f]) for f in good}
    BINS = (1, 7, 4096)

    def call(ct):
        n_pairs, st = ct.pairs(0, 6, raise_on_error=False)
        lists, launches = ct.lists(), [ct.stat(L.CT_STAT_LAST_LAUNCHES)]
        groups = [ct.stat(L.CT_STAT_LAST_WALK_GROUPS)]
        per_atom, np2, st2 = ct.counts(0, 6, raise_on_error=False)
        launches.append(ct.stat(L.CT_STAT_LAST_LAUNCHES)); groups.append(ct.stat(L.CT_STAT_LAST_WALK_GROUPS))
        hists = []
        for nbins in BINS:
            h, st3 = ct.hist(0, 6, nbins, raise_on_error=False)
            assert st3.tolist() == want_st
            hists.append(h)
            launches.append(ct.stat(L.CT_STAT_LAST_LAUNCHES)); groups.append(ct.stat(L.CT_STAT_LAST_WALK_GROUPS))
        assert st.tolist() == want_st == st2.tolist() and np.array_equal(n_pairs, np2)
        assert ct.stat(L.CT_STAT_LAST_RUNS) == runs_all
        return (n_pairs, per_atom) + lists + tuple(hists), launches, groups

    with G.Contacts(s, "A", "B", CUTOFF) as ct:
        ct.pairs(0, 6, raise_on_error=False)
        runs_all = ct.stat(L.CT_STAT_LAST_RUNS)
        assert runs_all > 100 and ct.stat(L.CT_STAT_LAST_PIECES) == 1
        base, base_launches, base_groups = call(ct)
        assert base_groups == [min(runs_all, 8192)] * 5
        n_pairs, per_atom, off, i, j, d = base[:6]
        # the default call: failed frames are empty, good frames are the per-slot call's bits and the oracle's pairs
        for f in range(6):
            x, y = int(off[f]), int(off[f + 1])
            if f not in good:
                assert x == y and n_pairs[f] == 0 and not per_atom[f].any() and not any(h[f].any() for h in base[6:])
                continue
            assert same_bits((i[x:y], j[x:y], d[x:y]), want[f][1:]), f
            check_oracle((np.array([0, y - x]), i[x:y], j[x:y], d[x:y]), [frames[f]], [boxes[f]], a, b, CUTOFF)
            assert np.array_equal(per_atom[f], np.bincount(i[x:y], minlength=200)[:200].astype(np.uint32))
            for nbins, h in zip(BINS, base[6:]):
                assert np.array_equal(h[f], numpy_hist(d[x:y], CUTOFF, nbins)), (f, nbins)
        assert per_atom[1][:20].min() >= nball               # the ball: one query's pairs come from three tiles
        for piece in (0, 2):
            ct.set_piece_frames(piece)
            ct.set_walk_groups(0)
            _, piece_launches, piece_groups = call(ct)        # (the largest grid of a piece, which a cap can only lower)
            assert ct.stat(L.CT_STAT_LAST_PIECES) == (3 if piece else 1)
            for cap in (1, 2, 7, runs_all - 1, runs_all, 0):
                ct.set_walk_groups(cap)
                got, launches, groups = call(ct)
                assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(got, base)) and same_bits(got[2:6], base[2:6]), (piece, cap)
                assert launches == piece_launches, (piece, cap, launches, piece_launches)
                assert groups == [min(cap, g) if cap else g for g in piece_groups], (piece, cap, groups)
                if piece == 0:
                    assert groups == [cap if cap else min(runs_all, 8192)] * 5
    s.close()

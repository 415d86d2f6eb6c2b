"""Batched calls across the 1024-frame segment of the library (GR_MAX_BATCH): ONE call over slots [0, 1030) against the same work as TWO
calls, [0, 1024) and [1024, 1030), on an identical twin system.  Results, per-frame statuses and the positions left in every slot must be
equal bit for bit; with failing frames on either side of the boundary the raised error is the first failing frame's, and failed frames
are left untouched.  (RMSD-fit has its own files; a hydrogen-bond batch refuses more than 1024 frames.)

group_translate_batch and group_wrap_batch find an atom without position while they move the others: k_translate_wrap skips that atom,
names it and moves the rest (test_gpu_translate_rows.py pins that; the reference's loop has likewise moved the atoms in front of it).
For these two a frame that fails on such an atom is therefore NOT untouched: the check there is that the atom itself and every atom
outside the moved group are left alone, and that one call and two calls leave the same bits.  A frame that fails its host checks
(no box) is untouched for every call."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

N, NS, CUT = 300, 1030, 1024
BOX = np.array([6.0, 7.0, 8.0, 0, 0, 0, 0, 0, 0], np.float32)
BAD = 30                                                      # the atom that loses its position: in A, in B and in a molecule
BONDS = [(28, 29), (29, 30), (30, 31), (100, 101), (101, 150), (200, 250)]
MOVES_AROUND_NAN = {"group_translate_batch": "B", "group_wrap_batch": None}     # call -> the group it moves (None: all); see the module's docstring


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.fixture(scope="module")
def data():
    """masses, frames (drawn as test_gpu_batch_calls.make does), the index group's atoms, one offset per frame"""
    rng = np.random.default_rng(1030)
    masses = rng.uniform(1.0, 16.0, N).astype(np.float32)
    L = BOX[:3]
    frames = []
    for f in range(NS):
        blob = rng.normal(0, 0.6, (N, 3)) + rng.uniform(0, 1, 3) * L
        frames.append(O.wrap_atoms(blob.astype(np.float32), np.arange(N), BOX))
    idx_b = np.unique(np.append(rng.integers(0, N, 40), BAD))
    return masses, frames, idx_b, rng.uniform(-1, 1, NS).astype(np.float32)


def build(G, data, no_box=(), nan_at=()):
    masses, frames, idx_b, _ = data
    s = G.System(N, masses=masses, n_slots=NS)
    sent = []
    for f in range(NS):
        pos = frames[f]
        if f in nan_at:
            pos = pos.copy(); pos[BAD] = np.nan
        s.set_frame(pos, BOX, slot=f); sent.append(pos)
    for f in no_box:
        s.reset_box(slot=f)
    s.group_create_from_ranges("A", [(10, 60)])
    s.group_create_from_indices("B", idx_b)
    s.add_bonds(BONDS)
    return s, G.GridMap(s, (0.0, 6.0), (0.0, 7.0), (0.5, 0.5)), sent


def calls(G, data):
    """name -> (call(system, gridmap, first, n, raise_on_error) -> (list of result arrays, status[n]), checks the box?, moves atoms: 0 never / 1 may / 2 must)"""
    offs = data[3]

    def matrices(s, gm, a, n, r):
        dev, n1, n2, st = s.group_all_distances_batch_device("A", "B", a, n, raise_on_error=r)
        return [s.device_read(dev, 0, (n, n1, n2))], st

    def gridmap(s, gm, a, n, r):
        n_out, st = gm.accumulate("B", a, n, value=G.Dimension.Z, offset=offs[a:a + n], raise_on_error=r)
        return [n_out], st

    def only_status(fn):
        return lambda s, gm, a, n, r: ([], fn(s, a, n, r))

    return {
        "group_get_com_batch": (lambda s, gm, a, n, r: _pair(s.group_get_com_batch("B", a, n, raise_on_error=r)), True, 0),
        "group_estimate_com_batch": (lambda s, gm, a, n, r: _pair(s.group_estimate_com_batch("A", a, n, raise_on_error=r)), True, 0),
        "group_all_distances_reduce max": (lambda s, gm, a, n, r: _pair(s.group_all_distances_reduce("A", "B", "max", first_slot=a, n_frames=n, raise_on_error=r)), True, 0),
        "group_all_distances_reduce count_below per row": (lambda s, gm, a, n, r: _pair(s.group_all_distances_reduce("A", "B", "count_below", per_row=True, param=1.5, first_slot=a, n_frames=n,
                                                                                                                      raise_on_error=r)), True, 0),
        "group_all_distances_batch_device": (matrices, True, 0),
        "GridMap.accumulate": (gridmap, False, 0),
        "atoms_center_batch": (only_status(lambda s, a, n, r: s.atoms_center_batch("B", a, n, G.Dimension.XYZ, weighted=True, raise_on_error=r)), True, 2),
        "atoms_center_batch contiguous": (only_status(lambda s, a, n, r: s.atoms_center_batch("A", a, n, G.Dimension.XZ, raise_on_error=r)), True, 2),
        "group_translate_batch": (only_status(lambda s, a, n, r: s.group_translate_batch("B", [3.3, -9.1, 0.4], a, n, raise_on_error=r)), True, 2),
        "group_wrap_batch": (only_status(lambda s, a, n, r: s.group_wrap_batch(None, a, n, raise_on_error=r)), True, 1),
        "make_group_whole_batch": (only_status(lambda s, a, n, r: s.make_group_whole_batch("B", a, n, raise_on_error=r)), True, 1),
        "make_molecules_whole_batch": (only_status(lambda s, a, n, r: s.make_molecules_whole_batch(a, n, raise_on_error=r)), True, 1),
    }


def _pair(res):
    return [res[0]], res[1]


def positions(s):
    return np.stack([s.get_positions(f) for f in range(NS)])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def twins_agree(G, data, no_box=(), nan_at=()):
    one, gm1, sent = build(G, data, no_box, nan_at)
    two, gm2, _ = build(G, data, no_box, nan_at)
    table = calls(G, data)
    E = G._lib
    kept = np.stack(sent)                                                 # what the slots held before the call at hand
    for name, (call, checks_box, moves) in table.items():
        r1, st1 = call(one, gm1, 0, NS, False)
        ra, sta = call(two, gm2, 0, CUT, False)
        rb, stb = call(two, gm2, CUT, NS - CUT, False)
        assert np.array_equal(st1, np.concatenate([sta, stb])), (name, np.flatnonzero(st1 != np.concatenate([sta, stb])))
        want = np.zeros(NS, np.int32)
        want[list(nan_at)] = E.E_NO_POSITION
        if checks_box:
            want[list(no_box)] = E.E_NO_BOX
        assert np.array_equal(st1, want), (name, np.flatnonzero(st1 != want), st1[st1 != want])
        for x1, xa, xb in zip(r1, ra, rb):
            assert same(x1, np.concatenate([xa, xb])), name
        if moves:
            p1, p2 = positions(one), positions(two)
            assert same(p1, p2), (name, np.flatnonzero((p1 != p2).any(axis=(1, 2))))
            for f in np.flatnonzero(want):                                # failed frames are left untouched
                if name in MOVES_AROUND_NAN and f in nan_at:
                    still = np.ones(N, bool)
                    if MOVES_AROUND_NAN[name] == "B":
                        still[data[2]] = False
                    else:
                        still[:] = False
                    still[BAD] = True
                    assert same(p1[f][still], kept[f][still]), (name, f)
                else:
                    assert same(p1[f], kept[f]), (name, f)
            assert moves == 1 or not same(p1[0], kept[0]), name
            kept = p1
    assert same(gm1.counts, gm2.counts) and same(gm1.sums_q, gm2.sums_q) and gm1.counts.sum() > 0
    # the raising form of the one call: the first failing frame's error (the calls above have shown that the frames that fail stay the same)
    failing = sorted(set(nan_at) | set(no_box))
    for name, (call, checks_box, moves) in table.items() if failing else ():
        first = [f for f in failing if checks_box or f in nan_at]
        with pytest.raises((G.GroupError, G.AtomError)) as e:
            call(one, gm1, 0, NS, True)
        if first[0] in no_box:
            assert e.value.variant == "InvalidSimBox" and e.value.status == E.E_NO_BOX, (name, e.value)
        else:
            assert e.value.variant == "InvalidPosition" and e.value.detail == BAD, (name, e.value)
    one.close(); two.close()


def test_one_call_equals_two_calls_across_the_segment(G, data):
    twins_agree(G, data)


def test_failing_frames_on_both_sides_of_the_boundary(G, data):
    """slot 1023 (the last frame of the first segment) has no box, slot 1024 (the first of the second) an atom without position"""
    twins_agree(G, data, no_box=(1023,), nan_at=(1024,))


def test_the_only_failing_frame_lies_in_the_second_segment(G, data):
    twins_agree(G, data, nan_at=(1026,))

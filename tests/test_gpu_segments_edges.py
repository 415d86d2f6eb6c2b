"""Segments at the edges its feature tests (test_gpu_segments.py) do not reach, against the same oracle (once per segment as a group,
summing in f64) with the same margins: TOL = 1e-5 nm, SEAM = 1e-4 nm, at most 16 segments per frame compared modulo a box vector
(asserted from the oracle when a world is made, before any call of the library).  "Bits" means another call of the library on the same
data, compared bit for bit.

1. Class counts: 65 / 17 / 5 / 3 segments in the 4-lane, 16-lane, wave and 256-lane class (a workgroup holds 64 / 16 / 4 / 1 teams), and
   sub-partitions with 63, 64, 65 / 15, 16, 17 / 3, 4, 5 / 1, 2, 3 of them: a class that fills its workgroups exactly, and one team more.
2. The 256-lane class (four loads of 256 atoms per trip): last trips in which some loads and some waves have nothing.
3. The first error inside a team: bad atoms in several lanes, waves and trips of one segment; a NaN mass and a NaN position together.
4. The first error of a frame: the 64-bit key (ordinal, mass bit, atom) with ordinals, classes and atoms in conflicting orders, and
   with ordinals above 65 535.
The atoms outside every segment sit at 1e30 with a mass of 1e30, as in the feature file: an atom read by mistake wrecks a sum."""
import numpy as np
import pytest

import oracle_lib as O
from segments_ref import E_NO_MASS, E_NO_POSITION, ESTIMATE, KINDS, NAIVE, PBC, TOL, _bits, _cell, _check_against, _max_error, _reference

pytestmark = pytest.mark.gpu
F = np.float32
BOX = [6.0, 6.4, 5.0]
TRIC = [6.0, 6.4, 5.0, 0, 0, 1.0, 0, -1.5, 0.8]
VARIANT = {E_NO_POSITION: "InvalidPosition", E_NO_MASS: "InvalidMass"}
WORST = {}                                                 # (kind, weighted) -> largest error against the oracle seen by this file, nm


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


# ------------------------------------------------------------------ worlds
SMALL = [1, 2, 3, 4] * 16 + [1]                            # 65 segments of the 4-lane class
MID = list(range(5, 17)) + [16, 16, 5, 9, 13]              # 17 of the 16-lane class
WAVE = [17, 257, 1023, 1025, 4096]                         # 5 of the wave class
BLOCKS2 = [4097, 4096 + 255, 4096 + 256 + 1, 5120, 5121, 8192 + 255]          # the 256-lane class: test 2
BLOCK = [BLOCKS2[2], BLOCKS2[4], BLOCKS2[5]]               # 3 of them in the world of test 1
SIZES1 = SMALL + MID + WAVE + BLOCK
K_MID, K_WAVE, K_BLOCK = len(SMALL), len(SMALL) + len(MID), len(SMALL) + len(MID) + len(WAVE)
N1, N2 = 30000, 31600


def make_lists(sizes, n_atoms, layout, seed):
    if layout == "gather":
        perm = np.random.default_rng(seed).permutation(n_atoms)[:sum(sizes)]
        cuts = np.cumsum([0] + list(sizes))
        return [np.sort(perm[cuts[k]:cuts[k + 1]]).astype(np.uint64) for k in range(len(sizes))]
    lists, a = [], 3                                       # contiguous, one behind the other from atom 3
    for n in sizes:
        lists.append(np.arange(a, a + n, dtype=np.uint64)); a += n
    assert a <= n_atoms
    return lists


def make_frames(lists, n_atoms, boxes, seed):
    """every segment a compact cloud that straddles a face of the cell (test_gpu_segments._synthetic_frames)"""
    rng = np.random.default_rng(seed)
    frames = []
    for box in boxes:
        H = _cell(box)
        Hi = np.linalg.inv(H)
        pos = np.full((n_atoms, 3), 1e30, np.float64)
        for idx in lists:
            idx = idx.astype(np.int64)
            c = rng.random(3)
            c[rng.integers(0, 3)] = rng.choice([0.004, 0.996, 0.0, 0.5])
            d = np.clip(rng.normal(0.0, 0.15, (idx.size, 3)), -0.45, 0.45)
            u = c + d @ Hi
            u -= np.floor(u)
            pos[idx] = u @ H
        frames.append(pos.astype(F))
    return frames


def make_masses(lists, n_atoms, seed):
    masses = (1.0 + 15.0 * np.random.default_rng(seed).random(n_atoms)).astype(F)
    inside = np.zeros(n_atoms, bool)
    for l in lists:
        inside[l.astype(np.int64)] = True
    masses[~inside] = 1e30
    return masses


def seam_ok(ref, n_frames):
    """at most 16 segments of a frame have their oracle estimate within SEAM of a face: _check_against's cap can hold"""
    for (kind, w), (cen, errs, flags) in ref.items():
        if flags is None: continue
        for f in range(n_frames):
            ok = np.array([e is None for e in errs[f]])
            assert int(flags[f][ok].any(axis=1).sum()) <= 16, (kind, w, f)
    return True


def world_data(which, layout):
    """(lists, frames, masses, boxes, reference) of world 1 (all classes, 3 frames) or 2 (the 256-lane class, 2 frames): host only"""
    sizes, n, boxes = (SIZES1, N1, [BOX, TRIC, BOX]) if which == 1 else (BLOCKS2, N2, [BOX, TRIC])
    lists = make_lists(sizes, n, layout, 20261110 + which)
    frames = make_frames(lists, n, boxes, 20261120 + which)
    masses = make_masses(lists, n, 20261130 + which)
    ref = _reference(frames, boxes, masses, lists)
    assert seam_ok(ref, len(boxes))
    return lists, frames, masses, boxes, ref


_WORLDS = {}


@pytest.fixture(scope="module")
def worlds(G):
    def get(which, layout):
        if (which, layout) not in _WORLDS:
            lists, frames, masses, boxes, ref = world_data(which, layout)
            s = G.System(len(masses), masses=masses, n_slots=len(boxes))
            for f in range(len(boxes)):
                s.set_frame(frames[f], boxes[f], slot=f)
            _WORLDS[(which, layout)] = (s, G.Segments.from_lists(s, lists), lists, frames, masses, boxes, ref)
        return _WORLDS[(which, layout)]
    yield get
    for w in _WORLDS.values():
        w[0].close()
    _WORLDS.clear()
    for key in sorted(WORST):
        print("segments edges kind %d weighted %d: largest |error| against the oracle %.3g nm" % (key[0], key[1], WORST[key]))


def checked(got, st, ref, key, boxes):
    """_check_against, and the largest error kept for the report"""
    _check_against(got, st, ref, key, boxes)
    cen, errs, flags = ref[key]
    for f in range(cen.shape[0]):
        ok = np.array([e is None for e in errs[f]])
        if ok.any():
            err = _max_error(got[f][ok], cen[f][ok], flags[f][ok] if flags is not None else None, boxes[f])
            WORST[key] = max(WORST.get(key, 0.0), float(err.max()))


def class_stats(G, seg):
    return [seg.stat(k) for k in (G._lib.SEG_STAT_TEAM4, G._lib.SEG_STAT_TEAM16, G._lib.SEG_STAT_WAVE, G._lib.SEG_STAT_WORKGROUP)]


# ------------------------------------------------------------------ 1. class-count edges
@pytest.mark.parametrize("layout", ["contiguous", "gather"])
def test_class_count_edges(G, worlds, layout):
    s, seg, lists, frames, masses, boxes, ref = worlds(1, layout)
    assert seg.sizes.tolist() == SIZES1 and class_stats(G, seg) == [65, 17, 5, 3]
    assert (layout == "gather") == any(int(l[-1]) - int(l[0]) + 1 != len(l) for l in lists if len(l) > 1)
    full = {}
    for kind, w in KINDS:
        got, st = seg.centers(0, 3, kind, w)
        assert st.tolist() == [0, 0, 0] and seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 4
        checked(got, st, ref, (kind, w), boxes)
        full[(kind, w)] = got
    # one team less than the workgroups hold, exactly what they hold, one team more: the same bits for the segments that are there
    for k in range(3):
        pick = list(range(0, 63 + k)) + list(range(K_MID, K_MID + 15 + k)) + list(range(K_WAVE, K_WAVE + 3 + k)) + list(range(K_BLOCK, K_BLOCK + 1 + k))
        with G.Segments.from_lists(s, [lists[p] for p in pick]) as sub:
            assert class_stats(G, sub) == [63 + k, 15 + k, 3 + k, 1 + k]
            for kind, w in KINDS:
                got, st = sub.centers(0, 3, kind, w)
                assert np.array_equal(_bits(got), _bits(full[(kind, w)][:, pick])), (k, kind, w)
    # ... and a class on its own
    for a, b, want in ((0, 64, [64, 0, 0, 0]), (K_MID, K_MID + 16, [0, 16, 0, 0]), (K_WAVE, K_WAVE + 4, [0, 0, 4, 0]), (K_BLOCK, K_BLOCK + 3, [0, 0, 0, 3])):
        with G.Segments.from_lists(s, lists[a:b]) as sub:
            assert class_stats(G, sub) == want
            got, _ = sub.centers(0, 3, PBC, 1)
            assert sub.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 1 and np.array_equal(_bits(got), _bits(full[(PBC, 1)][:, a:b]))


# ------------------------------------------------------------------ 2. the 256-lane class
@pytest.mark.parametrize("layout", ["contiguous", "gather"])
def test_workgroup_class_sizes(G, worlds, layout):
    s, seg, lists, frames, masses, boxes, ref = worlds(2, layout)
    assert seg.sizes.tolist() == [4097, 4351, 4353, 5120, 5121, 8447] and class_stats(G, seg) == [0, 0, 0, 6]
    rev = G.Segments.from_lists(s, lists[::-1])
    ones = [G.Segments.from_lists(s, [l]) for l in lists]
    for kind, w in KINDS:
        got, st = seg.centers(0, 2, kind, w)
        assert st.tolist() == [0, 0] and seg.stat(G._lib.SEG_STAT_LAST_LAUNCHES) == 1
        checked(got, st, ref, (kind, w), boxes)
        r, _ = rev.centers(0, 2, kind, w)
        assert np.array_equal(_bits(r[:, ::-1]), _bits(got)), (kind, w)
        for k, one in enumerate(ones):
            q, _ = one.centers(0, 2, kind, w)
            assert np.array_equal(_bits(q[:, 0]), _bits(got[:, k])), (kind, w, k)
    rev.close()
    for one in ones:
        one.close()


# ------------------------------------------------------------------ 3. the first error inside a team
def inject(G, world, seg, lists, nan_pos, nan_mass, groups=(), slot=0):
    """slot `slot` with NaN positions at the atoms nan_pos and NaN masses at nan_mass: every kind against the oracle (values, NaN rows,
    the frame's status), the raised error's variant and detail against the oracle's (status, index) of the first failed segment, and the
    segments `groups` against gr_group_center_batch on the same atoms.  -> {(kind, weighted): [(status, index) or None per segment]}"""
    s, _, _, frames, masses, boxes, _ = world
    bad = frames[slot].copy()
    bad[list(nan_pos)] = np.nan
    bm = masses.copy()
    bm[list(nan_mass)] = np.nan
    ref = _reference([bad], [boxes[slot]], bm, lists)
    out = {}
    try:
        s.set_frame(bad, boxes[slot], slot=slot)
        if len(nan_mass): s.set_masses(bm)
        for k in groups:
            s.group_create_from_indices("edge%d" % k, lists[k])
        for kind, w in KINDS:
            got, st = seg.centers(slot, 1, kind, w, raise_on_error=False)
            checked(got, st, ref, (kind, w), [boxes[slot]])
            errs = ref[(kind, w)][1][0]
            out[(kind, w)] = errs
            failed = [e for e in errs if e is not None]
            if failed:
                with pytest.raises(G.GroupError) as e:
                    seg.centers(slot, 1, kind, w)
                assert (e.value.status, e.value.detail, e.value.variant) == (failed[0][0], failed[0][1], VARIANT[failed[0][0]]), (kind, w, failed[0])
            else:
                assert st.tolist() == [0]
            for k in groups:
                cen, gst = s.group_center_batch("edge%d" % k, kind, w, slot, 1, raise_on_error=False)
                if errs[k] is not None:
                    assert gst[0] == errs[k][0] and np.isnan(cen[0]).all() and np.isnan(got[0, k]).all()
                    with pytest.raises(G.GroupError) as e:
                        s.group_center_batch("edge%d" % k, kind, w, slot, 1)
                    assert (e.value.status, e.value.detail) == errs[k], (kind, w, k)
                else:
                    flags = ref[(kind, w)][2]
                    err = _max_error(got[0, k:k + 1], cen[0:1], flags[0, k:k + 1] if flags is not None else None, boxes[slot])
                    assert gst[0] == 0 and err.max() <= TOL, (kind, w, k, float(err.max()))
    finally:
        s.set_frame(frames[slot], boxes[slot], slot=slot)
        if len(nan_mass): s.set_masses(masses)
        for k in groups:
            if s.group_exists("edge%d" % k): s.group_remove("edge%d" % k)
    return out


def only(errs, k, want):
    """segment k is the only one that failed, with (status, index) = want"""
    assert [j for j, e in enumerate(errs) if e is not None] == [k] and errs[k] == want, (k, want, errs[k])


def pos_and_mass(res, k, at_pos, at_mass):
    """a NaN position at at_pos and a NaN mass at at_mass < at_pos, different atoms of segment k: the weighted naive centre and the
    weighted estimate meet the mass first (they walk atom by atom); the weighted PBC centre runs the unweighted estimate over all atoms
    before it reads a mass, so it reports the position; the unweighted kinds never read a mass"""
    assert at_mass < at_pos
    for (kind, w), errs in res.items():
        only(errs, k, (E_NO_MASS, at_mass) if w and kind != PBC else (E_NO_POSITION, at_pos))


def one_atom_both(res, k, atom):
    """the same atom without position and without mass: position first for the naive centre, mass first for the estimate"""
    for (kind, w), errs in res.items():
        only(errs, k, (E_NO_MASS, atom) if w and kind == ESTIMATE else (E_NO_POSITION, atom))


def test_first_error_in_the_block_class(G, worlds):
    world = worlds(1, "contiguous")
    s, seg, lists = world[:3]
    k = K_BLOCK + 1
    a0 = int(lists[k][0])
    assert len(lists[k]) == 5121 and int(lists[k][-1]) - a0 + 1 == 5121
    # thread t of the workgroup walks offsets t, t + 256, ...: offset o is wave (o % 256) / 64's
    for o, wave in ((10, 0), (100, 1), (160, 2), (250, 3)):
        assert (o % 256) // 64 == wave
        res = inject(G, world, seg, lists, [a0 + o], [], groups=[k] if wave == 3 else [])
        for errs in res.values(): only(errs, k, (E_NO_POSITION, a0 + o))
    # two bad atoms: the lower one is wave 1's, the higher one wave 0's
    assert (100 % 256) // 64 == 1 and (300 % 256) // 64 == 0
    res = inject(G, world, seg, lists, [a0 + 100, a0 + 300], [], groups=[k, k - 1])
    for errs in res.values(): only(errs, k, (E_NO_POSITION, a0 + 100))
    # ... and the other way round, and in the last trip (offset 5120 is thread 0's, alone in its trip)
    res = inject(G, world, seg, lists, [a0 + 40, a0 + 256 + 70], [])
    for errs in res.values(): only(errs, k, (E_NO_POSITION, a0 + 40))
    res = inject(G, world, seg, lists, [a0 + 5120, a0 + 4096 + 200], [])
    for errs in res.values(): only(errs, k, (E_NO_POSITION, a0 + 4096 + 200))
    pos_and_mass(inject(G, world, seg, lists, [a0 + 256 + 3], [a0 + 7], groups=[k]), k, a0 + 259, a0 + 7)
    # the mass in another wave than the position; and the mass BEHIND the position: every kind reports the position
    pos_and_mass(inject(G, world, seg, lists, [a0 + 256 + 3], [a0 + 200], []), k, a0 + 259, a0 + 200)
    res = inject(G, world, seg, lists, [a0 + 70], [a0 + 256 + 130], [])
    for errs in res.values(): only(errs, k, (E_NO_POSITION, a0 + 70))
    one_atom_both(inject(G, world, seg, lists, [a0 + 130], [a0 + 130], groups=[k]), k, a0 + 130)


@pytest.mark.parametrize("layout", ["contiguous", "gather"])
def test_first_error_in_the_wave_class(G, worlds, layout):
    world = worlds(1, layout)
    s, seg, lists = world[:3]
    k = K_WAVE + 3
    at = lambda o: int(lists[k][o])
    assert len(lists[k]) == 1025
    # lane l walks offsets l, l + 64, l + 128, l + 192, then l + 256, ...: the lower atom sits in a later lane and an earlier trip
    assert (64 * 4 + 1) % 64 == 1 and 70 % 64 == 6
    res = inject(G, world, seg, lists, [at(64 * 4 + 1), at(70)], [], groups=[k, k + 1])
    for errs in res.values(): only(errs, k, (E_NO_POSITION, at(70)))
    res = inject(G, world, seg, lists, [at(1024), at(1023)], [])                # the last trip: lane 0's first load, lane 63's fourth
    for errs in res.values(): only(errs, k, (E_NO_POSITION, at(1023)))
    pos_and_mass(inject(G, world, seg, lists, [at(64 * 4 + 1)], [at(70)], groups=[k]), k, at(257), at(70))
    one_atom_both(inject(G, world, seg, lists, [at(321)], [at(321)], []), k, at(321))


@pytest.mark.parametrize("layout", ["contiguous", "gather"])
@pytest.mark.parametrize("cls", ["team16", "team4"])
def test_first_error_in_the_narrow_classes(G, worlds, layout, cls):
    """a team's lanes hold one atom each; the teams next to the failing one, in the same wave, are unharmed (every one is compared)"""
    world = worlds(1, layout)
    s, seg, lists = world[:3]
    k, first, n, lanes = (K_MID + 12, K_MID, 16, (0, 5, 15, 11, 2, 12, 3)) if cls == "team16" else (3 + 4 * 9, 0, 4, (0, 2, 3, 2, 1, 3, 1))
    at = lambda o: int(lists[k][o])
    assert len(lists[k]) == n and 0 < (k - first) % (256 // n)                      # not the first team of its workgroup
    for o in lanes[:3]:                                                            # one bad atom, in the first, a middle and the last lane
        res = inject(G, world, seg, lists, [at(o)], [], groups=[k] if o == lanes[2] else [])
        for errs in res.values(): only(errs, k, (E_NO_POSITION, at(o)))
    hi, lo = lanes[3], lanes[4]                                                    # two bad atoms in two lanes of the team
    res = inject(G, world, seg, lists, [at(hi), at(lo)], [], groups=[k, k + 1])
    for errs in res.values(): only(errs, k, (E_NO_POSITION, at(lo)))
    pos_and_mass(inject(G, world, seg, lists, [at(lanes[5])], [at(lanes[6])], groups=[k]), k, at(lanes[5]), at(lanes[6]))
    one_atom_both(inject(G, world, seg, lists, [at(lanes[4])], [at(lanes[4])], []), k, at(lanes[4]))


# ------------------------------------------------------------------ 4. the first error of a frame
def test_first_error_of_a_frame(G, worlds):
    world = worlds(1, "contiguous")
    s, _, lists1 = world[:3]
    # ordinal 0: a 256-lane segment (launched last, the highest atoms); 2: a 16-lane one; 3: a wave; every other one: four lanes
    lists = [lists1[K_BLOCK + 1], lists1[0], lists1[K_MID], lists1[K_WAVE + 3]] + lists1[1:40]
    sizes = [len(l) for l in lists]
    assert sizes[0] == 5121 and 4 < sizes[2] <= 16 and sizes[3] == 1025 and sizes[40] <= 4 and len(lists) == 43
    blk, low = int(lists[0][777]), int(lists[40][0])
    assert blk > low and int(lists[2][1]) < int(lists[3][5])
    with G.Segments.from_lists(s, lists) as seg:
        assert class_stats(G, seg) == [40, 1, 1, 1]
        # ordinal 0 and ordinal 40 fail: the frame reports ordinal 0's atom, the higher one, from the class that is launched last
        res = inject(G, world, seg, lists, [blk, low], [])
        for errs in res.values():
            assert [j for j, e in enumerate(errs) if e is not None] == [0, 40] and errs[0] == (E_NO_POSITION, blk) and errs[40] == (E_NO_POSITION, low)
        # ordinal 2 on its position, ordinal 3 on a mass: ordinal 2's; the pair swapped: the mass error of ordinal 2, the LOWER ordinal with the HIGHER mass bit
        p2, m3 = int(lists[2][1]), int(lists[3][5])
        res = inject(G, world, seg, lists, [p2], [m3])
        for (kind, w), errs in res.items():
            assert [j for j, e in enumerate(errs) if e is not None] == ([2, 3] if w else [2]) and errs[2] == (E_NO_POSITION, p2)
            if w: assert errs[3] == (E_NO_MASS, m3)
        m2, p3 = int(lists[2][1]), int(lists[3][5])
        res = inject(G, world, seg, lists, [p3], [m2])
        for (kind, w), errs in res.items():
            assert [j for j, e in enumerate(errs) if e is not None] == ([2, 3] if w else [3]) and errs[3] == (E_NO_POSITION, p3)
            if w: assert errs[2] == (E_NO_MASS, m2)
        # ... and with the atoms the other way round too: ordinal 1 (atoms 3 ..) on a mass, ordinal 0 (the highest atoms) on a position
        res = inject(G, world, seg, lists, [blk], [int(lists[1][0])])
        for (kind, w), errs in res.items():
            assert errs[0] == (E_NO_POSITION, blk) and (errs[1] == (E_NO_MASS, int(lists[1][0]))) == bool(w)


N_ONE = 70000


def one_atom_world():
    """70 000 one-atom segments in one orthorhombic frame; segment k holds atom perm[k]; the atoms keep 0.05 L from every face, half of
    them in a neighbouring cell (a one-atom centre is the atom, wrapped by the periodic kinds: no centre lies near a face)"""
    rng = np.random.default_rng(20261140)
    perm = rng.permutation(N_ONE).astype(np.uint64)
    if perm[66000] < perm[69999]: perm[[66000, 69999]] = perm[[69999, 66000]]  # the lower ordinal holds the higher atom
    u = rng.uniform(0.05, 0.95, (N_ONE, 3)) + rng.integers(-1, 2, (N_ONE, 3))
    pos = (u * np.array(BOX)).astype(F)
    masses = (1.0 + 15.0 * rng.random(N_ONE)).astype(F)
    # the oracle on 3 000 of them (a call costs 30 us: all of them, six kinds, would take 13 s): both ends, both sides of ordinal 65 536
    sample = np.unique(np.concatenate([np.arange(0, N_ONE, 35), np.arange(65236, 66036), np.arange(N_ONE - 450, N_ONE)]))
    return perm, pos, masses, sample


def test_ordinals_above_65535(G):
    perm, pos, masses, sample = one_atom_world()
    L = np.array(BOX, np.float64)
    wrapped = pos.astype(np.float64)[perm.astype(np.int64)]
    wrapped -= np.floor(wrapped / L) * L
    assert (np.minimum(wrapped, L - wrapped) > 0.04 * L).all() and sample.size >= 3000 and (sample > 65535).sum() > 500
    s = G.System(N_ONE, masses=masses, n_slots=1)
    s.set_frame(pos, BOX, slot=0)
    seg = G.Segments.from_lists(s, perm.reshape(-1, 1))
    assert len(seg) == N_ONE and class_stats(G, seg) == [N_ONE, 0, 0, 0]
    ref = _reference([pos], [BOX], masses, [perm[k:k + 1] for k in sample])
    assert seam_ok(ref, 1)
    for kind, w in KINDS:
        got, st = seg.centers(0, 1, kind, w)
        assert st.tolist() == [0]
        checked(got[:, sample], st, ref, (kind, w), [BOX])
        # every one of them: the atom itself, or the atom wrapped into the cell
        if kind == NAIVE and not w: assert np.array_equal(_bits(got[0]), _bits(pos[perm.astype(np.int64)]))
        want = pos.astype(np.float64)[perm.astype(np.int64)] if kind == NAIVE else wrapped
        err = np.abs(got[0].astype(np.float64) - want).max()
        print("segments 70 000 one-atom segments kind %d weighted %d: max |centre - atom| %.3g nm" % (kind, w, err))
        assert err <= TOL, (kind, w, float(err))
    try:
        # (66 000 = 65 536 + 464: an ordinal cut to 16 bits would come in front of ordinal 3 000)
        for ordinals, first in (([69999], 69999), ([69999, 66000], 66000), ([69999, 66000, 3000], 3000)):
            bad = pos.copy()
            bad[perm[ordinals].astype(np.int64)] = np.nan
            s.set_frame(bad, BOX, slot=0)
            for kind, w in KINDS:
                got, st = seg.centers(0, 1, kind, w, raise_on_error=False)
                assert st.tolist() == [E_NO_POSITION] and np.isnan(got[0]).any(axis=1).nonzero()[0].tolist() == sorted(ordinals)
                with pytest.raises(G.GroupError) as e:
                    seg.centers(0, 1, kind, w)
                assert (e.value.variant, e.value.detail) == ("InvalidPosition", int(perm[first])), (kind, w, ordinals)
            lone = [perm[k:k + 1] for k in sorted(ordinals)]                       # the oracle agrees: (status, index) of these segments
            with O.acc64():
                for l in lone:
                    with pytest.raises(O.OracleError) as e:
                        O.get_center(bad, l, BOX, masses)
                    assert (e.value.status, int(e.value.index)) == (E_NO_POSITION, int(l[0]))
        # a NaN mass at a low ordinal beside them: the weighted kinds report it, its ordinal is the first
        bm = masses.copy()
        bm[int(perm[70])] = np.nan
        s.set_masses(bm)
        for kind, w in KINDS:
            with pytest.raises(G.GroupError) as e:
                seg.centers(0, 1, kind, w)
            assert (e.value.variant, e.value.detail) == (("InvalidMass", int(perm[70])) if w else ("InvalidPosition", int(perm[3000]))), (kind, w)
    finally:
        s.close()

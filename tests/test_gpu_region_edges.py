"""Region at the edges its feature tests (test_gpu_region.py) do not reach, against the same oracle (oracle_lib.group_from_geometries,
once per frame) and with the same rule: everything compared is an integer, every comparison is np.array_equal, no atom and no frame is
left out.

1. k_rg_scan beyond wave 0.  One workgroup turns a frame's chunk counts into prefixes: a lane-serial stretch of per = ceil(chunks / 256)
   chunks, a shuffle scan over 64 lanes, the four waves through LDS.  A group of at most 64 chunks (65 536 ordinals) keeps all of it in
   wave 0 with per = 1; the groups here are the smallest at which the second and third step run at all, in a 525 400-atom system whose
   chunk counts are 1024 over long stretches, 0 over others, 1 once, and something between everywhere else -- so a prefix that is off
   by one chunk, one lane or one wave moves the list.
2. Pieces x batch segments x anchors x failed frames, on 1 030 frames: a failed frame in a later piece (its mask rows are the piece
   before's), a piece in which every frame fails, a batch segment in which every frame fails, the anchors of the second segment.
3. A list that has to move to a bigger block while it already holds entries, and one object reused with a smaller and a larger group."""
import numpy as np
import pytest

import oracle_lib as O
from region_ref import E_INVALID_ARG, E_NO_BOX, build, check, expect, moved

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


# ------------------------------------------------------------------ 1. the scan across waves and stretches
C_ = 1024                                                  # GR_RG_CHUNK, asserted against RG_STAT_CHUNK below
N_BIG = 525400
BOX_BIG = np.array([12.0, 12.8, 10.0, 0, 0, 0, 0, 0, 0], F)
START = 5                                                  # every source group starts at atom 5
BLOCK_SIZES = [64 * C_, 64 * C_ + 1, 129 * C_, 256 * C_, 256 * C_ + 1, 384 * C_ + 1, 512 * C_, 512 * C_ + 1, 513 * C_ + 5]
GATHER_SIZES = [64 * C_ + 1, 256 * C_ + 1]                 # every second atom: walked through the gather list
# chunks of the contiguous groups (chunk k = atoms 5 + 1024 k .. 5 + 1024 k + 1023), the same in every frame
INSIDE = [(12, 16), (66, 134), (330, 398)]                 # wholly inside both regions: count 1024; the long ones cross chunk 128 and chunk 384
OUTSIDE = [(6, 10), (150, 220), (420, 490)]                # wholly outside both: count 0
LONE = (180, 500)                                          # one atom inside in the middle of an outside stretch: chunk 180, ordinal 500 of it
NAN_CHUNKS = (64, 256, 512)                                # no position at the first and at the last ordinal of these chunks
HALF_BIG = {"kind": "rectangular", "position": [0.0, 0.0, 0.0], "size": [6.0, 12.8, 10.0]}      # half of the cell along x, periodic and naive


def big_frames():
    """three frames of N_BIG atoms: uniform over (-0.2 L, 1.2 L) except for the stretches above"""
    rng = np.random.default_rng(20261101)
    L = BOX_BIG[:3].astype(np.float64)
    frames = []
    for f in range(3):
        pos = rng.uniform(-0.2, 1.2, (N_BIG, 3)) * L

        def fill(c0, c1, x_lo, x_hi):
            a, b = START + C_ * c0, START + C_ * c1
            pos[a:b] = rng.uniform([x_lo, 0.05, 0.05], [x_hi, 0.95, 0.95], (b - a, 3)) * L
        for c0, c1 in INSIDE: fill(c0, c1, 0.05, 0.45)
        for c0, c1 in OUTSIDE: fill(c0, c1, 0.55, 0.95)
        pos[START + C_ * LONE[0] + LONE[1]] = np.array([0.25, 0.5, 0.5]) * L
        pos = pos.astype(F)
        pos[rng.integers(0, N_BIG, 200)] = np.nan                             # atoms without a position, others in every frame
        for c0, c1 in INSIDE:                                                  # (... but none inside the full stretches)
            a, b = START + C_ * c0, START + C_ * c1
            bad = np.isnan(pos[a:b, 0])
            pos[a:b][bad] = (np.array([0.25, 0.5, 0.5]) * L).astype(F)
        for k in NAN_CHUNKS:
            pos[START + C_ * k] = np.nan
            pos[START + C_ * k + C_ - 1] = np.nan
        frames.append(pos)
    return frames


def big_group(form, n):
    return (START + np.arange(n, dtype=np.uint64) * np.uint64(2 if form == "gather" else 1)).astype(np.uint64)


def chunk_counts(listed, form, n):
    """the oracle's list of one frame -> atoms inside per chunk of the source group"""
    ordinal = (listed.astype(np.int64) - START) // (2 if form == "gather" else 1)
    return np.bincount(ordinal // C_, minlength=(n + C_ - 1) // C_)


def check_distinctive(frames, form, n, naive, boxes):
    """the property the frames were built for, from the oracle alone: full chunks, empty chunks, a lone atom, the rest between"""
    idx = big_group(form, n)
    chunks = (n + C_ - 1) // C_
    for f in (0, 2) if not naive else (0, 1, 2):
        cnt = chunk_counts(O.group_from_geometries(frames[f], idx, boxes[f], [HALF_BIG], naive=naive), form, n)
        assert cnt.size == chunks
        size = np.minimum(C_, n - C_ * np.arange(chunks))                      # ordinals of every chunk (the last one may be short)
        special = np.zeros(chunks, bool)
        step = 2 if form == "gather" else 1                                    # a gather chunk spans two chunks of atoms
        for c0, c1 in INSIDE:
            a, b = (c0 + step - 1) // step, min(c1 // step, n // C_)
            if a < b:
                assert (cnt[a:b] == C_).all(), (form, n, f, c0)
                special[a:b] = True
        lone = C_ * LONE[0] + LONE[1]                                          # (atom - START) of the lone atom; ordinal lone / step where it is in the group
        lone_chunk = lone // step // C_ if lone % step == 0 and lone // step < n else -1
        for c0, c1 in OUTSIDE:
            a, b = (c0 + step - 1) // step, min(c1 // step, chunks)
            if a < b:
                want = np.zeros(b - a, np.int64)
                if a <= lone_chunk < b: want[lone_chunk - a] = 1
                assert (cnt[a:b] == want).all(), (form, n, f, c0, cnt[a:b].tolist())
                special[a:b] = True
        rest = ~special & (size == C_)
        assert rest.any() and (cnt[rest] > 0).all() and (cnt[rest] < C_).all(), (form, n, f)
        assert (cnt == C_).any() and (cnt == 0).any() and len(set(cnt.tolist())) > min(chunks, 40) // 2
        if form == "block":
            for k in NAN_CHUNKS:
                if k < chunks and C_ * (k + 1) <= n: assert 0 < cnt[k] <= C_ - 2


@pytest.fixture(scope="module")
def big(G):
    frames = big_frames()
    boxes = [BOX_BIG, None, BOX_BIG]
    s = G.System(N_BIG, n_slots=3)
    for f in range(3):
        s.set_frame(frames[f], boxes[f], slot=f)
    regions = {naive: G.Region(s, [build(G, HALF_BIG)], naive=naive) for naive in (False, True)}
    yield s, frames, boxes, regions
    s.close()


def test_big_layout():
    """the sizes mean what they say, and the largest group reaches every stretch"""
    n = BLOCK_SIZES[-1]
    assert START + n <= N_BIG and START + 2 * (GATHER_SIZES[-1] - 1) < N_BIG
    assert (n + C_ - 1) // C_ == 514 and max(c1 for _, c1 in INSIDE + OUTSIDE) <= 513 and sum(c1 - c0 >= 64 for c0, c1 in INSIDE) == 2
    per = lambda m: ((m + C_ - 1) // C_ + 255) // 256
    assert [per(m) for m in BLOCK_SIZES] == [1, 1, 1, 1, 2, 2, 2, 3, 3] and [per(m) for m in GATHER_SIZES] == [1, 2]
    # 256 C + 1: lane 128 holds one chunk; 384 C + 1: wave 3 (lane 192) holds one chunk; 513 C + 5: lane 171 holds one chunk of three
    assert 257 - 2 * 128 == 1 and 385 - 2 * 192 == 1 and 514 - 3 * 171 == 1


@pytest.mark.parametrize("form, n", [("block", n) for n in BLOCK_SIZES] + [("gather", n) for n in GATHER_SIZES],
                         ids=lambda v: v if isinstance(v, str) else "%dC%+d" % ((v + 512) // C_, v - (v + 512) // C_ * C_))
def test_scan_across_waves_and_stretches(G, big, form, n):
    s, frames, boxes, regions = big
    assert regions[False].stat(G._lib.RG_STAT_CHUNK) == C_ == 1024
    idx = big_group(form, n)
    assert idx.size == n and int(idx[-1]) < N_BIG
    if form == "block": s.group_create_from_ranges("src", [(START, START + n - 1)])
    else: s.group_create_from_indices("src", idx)
    try:
        for naive in (False, True):
            check_distinctive(frames, form, n, naive, boxes)
            r = regions[naive]
            counts, st = r.select("src", 0, 3, raise_on_error=False)
            failed = set() if naive else {1}                                   # slot 1 has no box: a periodic region refuses it, a naive one does not care
            assert st.tolist() == [0, 0 if naive else E_NO_BOX, 0]
            want = expect(frames, boxes, idx, [HALF_BIG], naive=naive, failed=failed)
            check(r, counts, want)
            assert r.stat(G._lib.RG_STAT_LAST_TOTAL) == int(want[0].sum()) and want[0][0] > 0 and want[0][2] > 0
            if not naive:
                assert counts[1] == 0 and r.frame(1).size == 0
                with pytest.raises(G.GroupError) as e:
                    r.select("src", 0, 3)
                assert e.value.status == E_NO_BOX
            print("region scan %s n %d naive %d: %d chunks, per %d, inside %s" % (form, n, naive, (n + C_ - 1) // C_, ((n + C_ - 1) // C_ + 255) // 256, counts.tolist()))
    finally:
        s.group_remove("src")


# ------------------------------------------------------------------ 2. pieces x batch segments x anchors x failures
N_SMALL, NF = 200, 1030
BOX_SMALL = np.array([3.0, 3.0, 3.0, 0, 0, 0, 0, 0, 0], F)
SPECS2 = [{"kind": "cylinder", "position": [0.0, 0.0, -0.75], "radius": 1.0, "height": 1.5, "orientation": "Z"},
          {"kind": "sphere", "position": [0.0, 0.0, 0.0], "radius": 1.2}]
# no box: 0, 299, 300, 1023, 1024, 1029, and 600 .. 608.  (Pieces of 7 start at multiples of 7: the piece 602 .. 608 fails as a whole,
# and 600, 601 end the piece in front of it.)
NO_BOX = sorted({0, 299, 300, 1023, 1024, 1029} | set(range(600, 609)))
BAD_ANCHOR = 1025


def small_world():
    rng = np.random.default_rng(20261102)
    base = (rng.random((N_SMALL, 3)) * 3.0).astype(F)
    frames = [(base + F(0.013) * F(f % 97)).astype(F) for f in range(NF)]
    anchors = (1.5 + rng.uniform(-0.3, 0.3, (NF, 3))).astype(F)
    boxes = [None if f in NO_BOX else BOX_SMALL for f in range(NF)]
    bad = anchors.copy()
    bad[BAD_ANCHOR, 1] = np.inf
    return frames, boxes, anchors, bad


def n_pieces(piece, live_segments=((0, 1024), (1024, 6))):
    """pieces of a call: every batch segment that has a frame to work is cut on its own"""
    return sum((nb + piece - 1) // piece if piece else 1 for _, nb in live_segments)


@pytest.fixture(scope="module")
def small(G):
    frames, boxes, anchors, bad = small_world()
    s = G.System(N_SMALL, n_slots=NF)
    for f in range(NF):
        s.set_frame(frames[f], boxes[f], slot=f)
    s.group_create_from_ranges("g", [(1, 190)])
    idx = np.arange(1, 191, dtype=np.uint64)
    failed = set(NO_BOX) | {BAD_ANCHOR}
    want = expect(frames, boxes, idx, SPECS2, anchors=anchors, failed=failed)
    good = np.array([f not in failed for f in range(NF)])
    assert want[0][good].min() > 0 and len(set(want[0].tolist())) > 5          # every good frame lists something: an empty one is a failed one
    status = [E_INVALID_ARG if f == BAD_ANCHOR else E_NO_BOX if f in NO_BOX else 0 for f in range(NF)]
    with G.Region(s, [build(G, sp) for sp in SPECS2]) as r:
        yield s, r, frames, boxes, anchors, bad, idx, failed, want, status
    s.close()


def test_pieces_segments_anchors_and_failures(G, small):
    s, r, frames, boxes, anchors, bad, idx, failed, want, status = small
    assert any(all(f in failed for f in range(p0, p0 + 7)) for p0 in range(0, 1024, 7))       # with pieces of 7 one piece fails as a whole
    r.set_piece_frames(0)
    c0, st0 = r.select("g", 0, NF, anchors=bad, raise_on_error=False)
    o0, a0 = r.lists()
    assert st0.tolist() == status
    check(r, c0, want)
    assert r.stat(G._lib.RG_STAT_LAST_PIECES) == 2 and r.stat(G._lib.RG_STAT_LAST_TOTAL) == int(want[0].sum())
    for piece in (0, 300, 7, 1, 6):
        r.set_piece_frames(piece)
        c, st = r.select("g", 0, NF, anchors=bad, raise_on_error=False)
        assert st.tolist() == status, piece
        check(r, c, want)
        o, a = r.lists()
        assert np.array_equal(c, c0) and np.array_equal(o, o0) and np.array_equal(a, a0), piece
        pieces, launches = r.stat(G._lib.RG_STAT_LAST_PIECES), r.stat(G._lib.RG_STAT_LAST_LAUNCHES)
        print("region pieces of %d: %d pieces, %d launches, %d listed" % (piece, pieces, launches, r.stat(G._lib.RG_STAT_LAST_TOTAL)))
        assert pieces == n_pieces(piece) and 2 * pieces <= launches <= 3 * pieces
        if piece in (7, 1):
            assert launches < 3 * pieces                                       # the piece without a good frame lists nothing and emits nothing
        if piece == 6:
            # frames 1024 .. 1029 are one piece whose first frame failed: its mask rows are what the piece 1018 .. 1023 left there
            assert n_pieces(6) == 171 + 1
            for f in sorted(failed):
                assert c[f] == 0 and int(o[f + 1]) == int(o[f]) and r.frame(f).size == 0
            for f in (1022, 1026, 1027, 1028):
                assert np.array_equal(r.frame(f), O.group_from_geometries(frames[f], idx, boxes[f], moved(SPECS2, anchors[f]))) and c[f] > 0
    with pytest.raises(G.GroupError) as e:                                     # the call's own status: its first failed frame's
        r.select("g", 0, NF, anchors=bad)
    assert e.value.status == E_NO_BOX
    with pytest.raises(G.DeviceError) as e:
        r.select("g", 1025, 5, anchors=bad[1025:])
    assert e.value.status == E_INVALID_ARG
    r.set_piece_frames(0)


def test_second_segment_alone(G, small):
    """frames 1024 .. 1029 with their own anchors, and 0 .. 1023: together the 1 030-frame call (the anchor of frame seg_b0 + f)"""
    s, r, frames, boxes, anchors, bad, idx, failed, want, status = small
    assert len(set(map(tuple, anchors[1024:].tolist())) & set(map(tuple, anchors[:6].tolist()))) == 0
    for piece in (0, 4):
        r.set_piece_frames(piece)
        cb, stb = r.select("g", 1024, 6, anchors=bad[1024:], raise_on_error=False)
        ob, ab = r.lists()
        check(r, cb, expect(frames[1024:], boxes[1024:], idx, SPECS2, anchors=anchors[1024:], failed={f - 1024 for f in failed if f >= 1024}))
        ca, sta = r.select("g", 0, 1024, anchors=bad[:1024], raise_on_error=False)
        oa, aa = r.lists()
        assert np.array_equal(np.concatenate([ca, cb]), want[0]) and np.array_equal(np.concatenate([aa, ab]), want[2])
        assert np.array_equal(np.concatenate([oa, ob[1:] + oa[-1]]), want[1]) and sta.tolist() + stb.tolist() == status
        assert cb[2:5].min() > 0
    r.set_piece_frames(0)


def test_a_segment_in_which_every_frame_fails(G, small):
    s, r, frames, boxes, anchors, bad, idx, failed, want, status = small
    try:
        for f in (1026, 1027, 1028):
            s.set_frame(frames[f], None, slot=f)
        gone = failed | set(range(1024, NF))
        want2 = expect(frames, boxes, idx, SPECS2, anchors=anchors, failed=gone)
        assert np.array_equal(want2[2], want[2][:int(want[1][1024])])
        for piece in (0, 7):
            r.set_piece_frames(piece)
            c, st = r.select("g", 0, NF, anchors=bad, raise_on_error=False)
            assert st.tolist() == status[:1024] + [E_NO_BOX, E_INVALID_ARG] + [E_NO_BOX] * 4
            check(r, c, want2)
            assert c[1024:].tolist() == [0] * 6 and all(r.frame(f).size == 0 for f in range(1024, NF))
            assert r.stat(G._lib.RG_STAT_LAST_PIECES) == n_pieces(piece, ((0, 1024),)) and r.stat(G._lib.RG_STAT_LAST_LAUNCHES) <= 3 * r.stat(G._lib.RG_STAT_LAST_PIECES)
        # ... and that segment on its own: nothing is launched at all
        c, st = r.select("g", 1024, 6, anchors=bad[1024:], raise_on_error=False)
        assert c.tolist() == [0] * 6 and r.lists()[0].tolist() == [0] * 7 and r.lists()[1].size == 0 and r.stat(G._lib.RG_STAT_LAST_PIECES) == 0
    finally:
        for f in (1026, 1027, 1028):
            s.set_frame(frames[f], BOX_SMALL, slot=f)
        r.set_piece_frames(0)
    c, st = r.select("g", 0, NF, anchors=bad, raise_on_error=False)            # put back: the first test's result again
    check(r, c, want)


# ------------------------------------------------------------------ 3. a list that grows while it holds entries
N_GROW = 3000
BALL = {"kind": "sphere", "position": [0.0, 0.0, 0.0], "radius": 10.0}        # naive; the anchor carries it along x
BALL_X = [100.0, 100.0, 100.0, 14.85, 10.0, 100.0, 14.2, 13.8, 13.3, 12.8, 12.0, 11.0]


def grow_world():
    rng = np.random.default_rng(20261103)
    frames = [(rng.random((N_GROW, 3)) * 5.0).astype(F) for _ in range(12)]
    anchors = np.array([[x, 2.5, 2.5] for x in BALL_X], F)
    anchors[:, 1:] += rng.uniform(-0.1, 0.1, (12, 2)).astype(F)
    return frames, anchors


def test_list_grows_while_it_holds_entries(G):
    frames, anchors = grow_world()
    box = np.array([5.0, 5.0, 5.0, 0, 0, 0, 0, 0, 0], F)
    groups = {"mid": np.arange(3, 2001, dtype=np.uint64), "few": np.arange(10, 201, dtype=np.uint64), "all": np.arange(N_GROW, dtype=np.uint64)}
    want = {k: expect(frames, [box] * 12, idx, [BALL], naive=True, anchors=anchors) for k, idx in groups.items()}
    cnt = want["mid"][0].astype(np.int64)
    assert cnt[:3].tolist() == [0, 0, 0] and 0 < cnt[3] <= 20 and cnt[4] >= 0.95 * groups["mid"].size and cnt[5] == 0
    assert (np.diff(cnt[6:]) > 0).all() and cnt[6] > cnt[3]
    # a block that held the list after frame 4 with room for no more than twice as much is too small twice more before the end
    tot = np.cumsum(cnt)
    assert tot[4] > 40 * tot[3] and tot[9] > 2 * tot[4] - tot[3] and tot[11] > 1.5 * tot[9]
    s = G.System(N_GROW, n_slots=12)
    for f in range(12):
        s.set_frame(frames[f], box, slot=f)
    s.group_create_from_ranges("mid", [(3, 2000)])
    s.group_create_from_ranges("few", [(10, 200)])
    with G.Region(s, [build(G, BALL)], naive=True) as r:                       # a new object: its list block holds one entry
        r.set_piece_frames(1)
        c1, st = r.select("mid", 0, 12, anchors=anchors)
        assert not st.any() and r.stat(G._lib.RG_STAT_LAST_PIECES) == 12
        assert r.stat(G._lib.RG_STAT_LAST_LAUNCHES) == 2 * 12 + int((cnt > 0).sum())      # a piece that lists nothing emits nothing
        check(r, c1, want["mid"])
        o1, a1 = r.lists()
        r.set_piece_frames(0)
        c0, _ = r.select("mid", 0, 12, anchors=anchors)
        o0, a0 = r.lists()
        assert r.stat(G._lib.RG_STAT_LAST_PIECES) == 1
        assert np.array_equal(c0, c1) and np.array_equal(o0, o1) and np.array_equal(a0, a1)
        print("region growing list: counts %s" % cnt.tolist())
        # the same object with a smaller and a larger group in turn: the words of a mask row change under the workspace that exists
        for piece in (1, 5, 0):
            r.set_piece_frames(piece)
            for name in ("few", "all", "mid", "few"):
                c, st = r.select(None if name == "all" else name, 0, 12, anchors=anchors)
                assert not st.any()
                check(r, c, want[name])
    with G.Region(s, [build(G, BALL)], naive=True) as r:                       # ... and a new object that starts with the small one
        r.set_piece_frames(1)
        for name in ("few", "all"):
            c, _ = r.select(None if name == "all" else name, 0, 12, anchors=anchors)
            check(r, c, want[name])
    s.close()

"""Internals at the edges of its kernel (gr_internals.h): the wave of 64 tuples (T = 1, 63, 64, 65, 257), tuples whose atoms straddle a
256-atom tile (254, 255, 256, 257) or name the last atom of the system, the look-ahead of the frame walk (GR_IC_AHEAD, read from the
source: frame counts AHEAD - 1, AHEAD, AHEAD + 1 and frame chunks that do not divide them), and 1 025 frames in one call, across the
1 024-frame segment of a batched call.

Values are held to internals_ref.bounds against the f64 restatement (tests/test_gpu_internals.py, tests/test_internals_host.py), every
tuple of every frame; the state of accumulate is compared bit for bit with the restatement of the rows.
THE 300-ATOM SYSTEM: atoms 0, 1, 258, 259 belong to no chain; chains (four atoms each) start at 2, 6 .. 254 and at 260, 264 .. 296, so
that one chain is atoms 254 .. 257 and the last one ends on atom 299."""
import numpy as np
import pytest

import internals_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
KINDS = ("distance", "angle", "dihedral", "axis")
AXIS = (0.3, -0.2, 1.0)
AHEAD = R.source_ahead()
STARTS = np.concatenate([2 + 4 * np.arange(64), 260 + 4 * np.arange(10)]).astype(np.uint64)
N, NF = 300, AHEAD + 4
REL = {"distance": [(1, 2), (0, 1), (2, 3)], "axis": [(1, 2), (0, 1), (2, 3)], "angle": [(0, 1, 2), (1, 2, 3)], "dihedral": [(0, 1, 2, 3)]}


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def tuples(kind, T):
    """T tuples of the 74 chains, chain by chain: the chain 254 .. 257 first (its first tuple straddles the tiles), the chain that ends
    on atom 299 second, then the others, and round again"""
    order = [63, 73] + list(range(63)) + list(range(64, 73))
    every = np.array([[int(STARTS[c]) + k for k in r] for c in order for r in REL[kind]], np.uint64)
    return every[np.arange(T) % len(every)]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def world(G, tric_small):
    boxes = R.frame_boxes(tric_small["triclinic_boxes9"][0], NF)
    rng = np.random.default_rng(8)
    frames = []
    for f in range(NF):
        x = (rng.random((N, 3)) * 2).astype(F)
        x[(STARTS[:, None] + np.arange(4, dtype=np.uint64)[None, :]).ravel()] = R.chains(len(STARTS), boxes[f], 500 + f)[0]
        frames.append(x)
    s = G.System(N, n_slots=NF)
    for f in range(NF):
        s.set_frame(frames[f], boxes[f], slot=f)
    yield s, boxes, frames
    s.close()


def check(kind, t, v, frames, boxes):
    for f in range(len(v)):
        bound = R.bounds(kind, frames[f], t, boxes[f], AXIS)
        assert bound.max() < 1e-3
        assert (R.error(kind, v[f], R.values64(kind, frames[f], t, boxes[f], AXIS)) <= bound).all(), (kind, f)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", KINDS)
def test_tuple_counts_around_the_wave(G, world, kind, T):
    s, boxes, frames = world
    t = tuples(kind, T)
    assert t[0].min() < 256 <= t[0].max() and (T == 1 or (t == N - 1).any())
    with G.Internals(s, kind, t, axis=AXIS if kind == "axis" else None) as ic:
        v, st = ic.values(0, NF)
        assert v.shape == (NF, T) and not st.any()
        check(kind, t, v, frames, boxes)
        assert ic.stat(G._lib.IC_STAT_LAST_RANGE_GROUPS) == -(-T // 64)
        for ranges in (2, 5):                                           # ranges that cut a wave's tuples apart and leave waves idle
            ic.set_launch(ranges, 0)
            assert bits(ic.values(0, NF)[0]) == bits(v)
        ic.accumulate(0, NF)
        ref = R.State(kind, T).add(v)
        o, sm, q, n = ic.read_raw()
        assert n == NF and R.same_bits(o, ref.o) and R.same_bits(sm, ref.s) and R.same_bits(q, ref.q)


@pytest.mark.parametrize("nf", [1, AHEAD - 1, AHEAD, AHEAD + 1, 2 * AHEAD - 1, NF])
@pytest.mark.parametrize("kind", KINDS)
def test_frame_counts_around_the_look_ahead(G, world, kind, nf):
    s, boxes, frames = world
    t = tuples(kind, 65)
    with G.Internals(s, kind, t, axis=AXIS if kind == "axis" else None) as ic:
        assert ic.stat(G._lib.IC_STAT_AHEAD) == AHEAD
        full = ic.values(0, NF)[0]
        for first in (0, NF - nf):
            v, st = ic.values(first, nf)
            assert not st.any() and bits(v) == bits(full[first:first + nf])
            for chunk in (2, 3, AHEAD + 1):                             # at least one of them does not divide nf
                ic.set_launch(0, chunk)
                assert bits(ic.values(first, nf)[0]) == bits(v), (first, chunk)
                assert ic.stat(G._lib.IC_STAT_LAST_FRAME_GROUPS) == -(-nf // min(chunk, nf))
            ic.set_launch(0, 0)
        check(kind, t, full[:nf], frames, boxes)
        ic.accumulate(0, nf)
        ref = R.State(kind, len(t)).add(full[:nf])
        o, sm, q, n = ic.read_raw()
        assert n == nf and R.same_bits(o, ref.o) and R.same_bits(sm, ref.s) and R.same_bits(q, ref.q)
        # a failed frame at the end of the ring's first turn and at the start of the next
    broken = [x.copy() for x in frames]
    for f in (AHEAD - 1, AHEAD):
        if f < nf:
            broken[f][int(t[0][0]), 0] = np.nan
    s2 = G.System(N, n_slots=nf)
    for f in range(nf):
        s2.set_frame(broken[f], boxes[f], slot=f)
    with G.Internals(s2, kind, t, axis=AXIS if kind == "axis" else None) as ic:
        v, st = ic.values(0, nf, raise_on_error=False)
        bad = [f for f in (AHEAD - 1, AHEAD) if f < nf]
        assert [f for f in range(nf) if st[f]] == bad and all(st[f] == R.E_NO_POSITION for f in bad)
        for f in range(nf):
            assert np.isnan(v[f]).all() if f in bad else bits(v[f]) == bits(full[f]), f
        ic.accumulate(0, nf, raise_on_error=False)
        ref = R.State(kind, len(t)).add(v)
        o, sm, q, n = ic.read_raw()
        assert n == nf - len(bad) == ref.n and (n == 0 or (R.same_bits(o, ref.o) and R.same_bits(sm, ref.s) and R.same_bits(q, ref.q)))
    s2.close()


# ---------------------------------------------------------------- 1 025 frames of a 33-atom system
LONG = 1025


@pytest.fixture(scope="module")
def long_world(G, aa):
    box = aa["box9"]
    pos = R.chains(8 * LONG, box, 900)[0].reshape(LONG, 32, 3)
    frames = np.concatenate([pos, np.full((LONG, 1, 3), 1.5, F)], axis=1)
    s = G.System(33, n_slots=LONG)
    for f in range(LONG):
        s.set_frame(frames[f], box, slot=f)
    yield s, box, frames
    s.close()


def test_workspace_pieces(G, long_world):
    """T_pad x 1024 x 4 B above GR_IC_MAX_WS_BYTES: the host variant walks a segment in pieces of fewer frames, and no bit depends on it"""
    s, box, frames = long_world
    base = R.chain_tuples("angle", 8)
    T = G._lib.IC_MAX_WS_BYTES // (4 * 1024) + 1000
    t = base[np.arange(T) % len(base)]
    with G.Internals(s, "angle", base) as small, G.Internals(s, "angle", t) as big:
        want = small.values(0, LONG)[0]
        got, st = big.values(0, LONG)
        assert not st.any() and big.stat(G._lib.IC_STAT_LAUNCHES) > small.stat(G._lib.IC_STAT_LAUNCHES) == 2
        for k in range(len(base)):
            assert (got[:, k::len(base)].view(np.uint32) == want[:, k:k + 1].view(np.uint32)).all(), k


@pytest.mark.parametrize("kind", KINDS)
def test_1025_frames_in_one_call(G, long_world, kind):
    s, box, frames = long_world
    t = R.chain_tuples(kind, 8)
    with G.Internals(s, kind, t, axis=AXIS if kind == "axis" else None) as ic, G.Internals(s, kind, t, axis=AXIS if kind == "axis" else None) as cut:
        v, st = ic.values(0, LONG)
        assert v.shape == (LONG, len(t)) and not st.any()
        # every frame at once: frame f's atoms are 33 f .. 33 f + 32 of the stacked positions, E is each frame's own
        stacked = frames.reshape(-1, 3)
        tt = (t[None, :, :] + (33 * np.arange(LONG, dtype=np.uint64))[:, None, None]).reshape(-1, t.shape[1])
        E = np.repeat(R.ulp32(np.abs(frames[:, :32]).max(axis=(1, 2))), len(t))
        bound = R.bounds(kind, stacked, tt, box, AXIS, E=E)
        err = R.error(kind, v.ravel(), R.values64(kind, stacked, tt, box, AXIS))
        assert bound.max() < 1e-3 and (err <= bound).all(), float((err / bound).max())
        assert bits(v[1020:]) == bits(ic.values(1020, 5)[0]) and bits(v[:3]) == bits(ic.values(0, 3)[0])
        assert not ic.accumulate(0, LONG).any() and ic.n_frames == LONG
        cut.accumulate(0, 1000); cut.accumulate(1000, 25)
        ref = R.State(kind, len(t)).add(v)
        for obj in (ic, cut):
            o, sm, q, n = obj.read_raw()
            assert n == LONG and R.same_bits(o, ref.o) and R.same_bits(sm, ref.s) and R.same_bits(q, ref.q)

#!/usr/bin/env python3
"""Contacts on resident frames: time per frame of the batched calls, next to the per-slot loop they replace and to one read of the positions.

Two rows:
  aa      tests/golden/aa_full.npz (32 817 atoms, its two frames in turn): protein (atoms 0-362) x water (SOL) at 0.6 nm, --frames frames
          per call (64) in every mode
  water   --atoms atoms (1e6) uniform in an orthorhombic cell at water density (100 atoms / nm^3; every frame drawn from its own seed
          on the device), all x all at 0.35 nm: `count` and `hist` with --frames frames per call, `pairs` with --pair-frames (4; the
          lists are ~0.2 GB per frame)
Alternating in one process, --steps timed calls (after --warmup of each) of
  count / hist / pairs     Contacts.counts / .hist (--bins bins) / .pairs over the frames; the lists stay on the device
  loop_count / loop_pairs  the path that exists without the object: one gr_group_pairs_within call per slot over the same slots, count only
                           (NULL buffers) for count and hist, with preallocated host buffers for pairs
  all_atoms                the yardstick (water row): group_center_batch("all", naive) of the same frames -- the memory system's pace
                           for one read of the positions by existing code
and, from their medians: us per frame of each and the ratios loop / batched.  The counts of the two paths are compared before anything
is timed.  No threshold is set.  Prints one JSON line; --out also writes it (profiles/contacts_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def water(G, n, nf):
    L = float((n / 100.0) ** (1.0 / 3.0))
    s = G.System(n, n_slots=nf, device=0)
    for f in range(nf):
        s.synth_uniform(f, [L, L, L], 20261019 + f)
    s.group_create_from_ranges("one", [(0, n - 1)])
    return s, "one", "one", 0.35


def aa(G, nf):
    d = np.load(os.path.join(ROOT, "tests", "golden", "aa_full.npz"))
    sol = np.nonzero(d["resname"] == b"SOL")[0]
    s = G.System(len(d["resid"]), n_slots=nf, device=0)
    for f in range(nf):
        s.set_frame(d["frames"][f % 2], d["boxes9"][f % 2], slot=f)
    s.group_create_from_ranges("one", [(0, 362)])
    s.group_create_from_indices("two", sol)
    return s, "one", "two", 0.6


def measure(G, s, g1, g2, cutoff, nf, nf_pairs, bins, steps, warmup, yardstick):
    lib = G._lib.load()
    ct = G.Contacts(s, g1, g2, cutoff)
    n = C.c_uint64(0)
    loop_counts = np.zeros(nf, np.uint64)
    a, b = g1.encode(), g2.encode()

    def loop_count():
        for f in range(nf):
            st = lib.gr_group_pairs_within(s._ctx, f, a, b, C.c_float(cutoff), 0, None, None, None, C.byref(n))
            assert st == 0
            loop_counts[f] = n.value

    loop_count()
    cap = int(loop_counts[:nf_pairs].max())
    bi, bj, bd = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)

    def loop_pairs():
        for f in range(nf_pairs):
            st = lib.gr_group_pairs_within(s._ctx, f, a, b, C.c_float(cutoff), cap, vp(bi), vp(bj), vp(bd), C.byref(n))
            assert st == 0

    got = {}

    def count(): got["count"] = ct.counts(0, nf)[1]
    def hist(): got["hist"] = ct.hist(0, nf, bins)[0]
    def pairs(): got["pairs"] = ct.pairs(0, nf_pairs)[0]

    calls = {"count": count, "hist": hist, "pairs": pairs, "loop_count": loop_count, "loop_pairs": loop_pairs}
    if yardstick:
        calls["all_atoms"] = lambda: s.group_center_batch("all", G._lib.CENTER_NAIVE, 0, 0, nf)
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    assert np.array_equal(got["count"], loop_counts) and np.array_equal(got["pairs"], loop_counts[:nf_pairs]), "the batch and the per-slot loop disagree"
    assert (got["hist"].sum(1) <= loop_counts).all()
    stats = {"pairs_pieces": ct.stat(G._lib.CT_STAT_LAST_PIECES), "pairs_launches": ct.stat(G._lib.CT_STAT_LAST_LAUNCHES)}
    res = {k: [] for k in calls}
    for _ in range(steps):                        # alternate them, one timed call each per round
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            res[k].append(time.perf_counter() - t0)
    frames = {k: (nf_pairs if k in ("pairs", "loop_pairs") else nf) for k in calls}
    med = {k: float(np.median(v)) / frames[k] * 1e6 for k, v in res.items()}
    out = {"atoms": s.n_atoms, "n1": ct.n1, "n2": ct.n2, "cutoff": cutoff, "frames_per_call": nf, "frames_per_pairs_call": nf_pairs, "bins": bins,
           "pairs_per_frame_mean": float(loop_counts.mean()), "tile": ct.stat(G._lib.CT_STAT_TILE)}
    out.update(stats)
    for k in calls:
        out[k + "_us_per_frame"] = med[k]
        out[k + "_us_per_frame_min"] = float(min(res[k])) / frames[k] * 1e6
    out["loop_over_count"] = med["loop_count"] / med["count"]
    out["loop_over_hist"] = med["loop_count"] / med["hist"]
    out["loop_over_pairs"] = med["loop_pairs"] / med["pairs"]
    if yardstick:
        out["count_over_all_atoms"] = med["count"] / med["all_atoms"]
    ct.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--pair-frames", type=int, default=4)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default="aa,water", help="comma-separated: aa, water")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/contacts_bench.py", "calls": a.steps, "warmup": a.warmup}
    rows = a.rows.split(",")
    if "aa" in rows:
        s, g1, g2, cutoff = aa(G, a.frames)
        out["aa"] = measure(G, s, g1, g2, cutoff, a.frames, a.frames, a.bins, a.steps, a.warmup, False)
        s.close()
    if "water" in rows:
        s, g1, g2, cutoff = water(G, a.atoms, a.frames)
        out["water"] = measure(G, s, g1, g2, cutoff, a.frames, min(a.pair_frames, a.frames), a.bins, a.steps, a.warmup, True)
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

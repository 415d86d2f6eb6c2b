#!/usr/bin/env python3
"""Region.select on resident frames: time per frame, next to the per-slot loop it replaces and to one read of the positions.

Two systems, --frames resident frames each (64 by default):
  water   --atoms atoms (1e6) uniform in an orthorhombic 22 nm cell; the selection runs over all of them, the anchor group is
          the first 3 000 atoms
  aa      tests/golden/aa_full.npz (32 817 atoms, its two frames in turn); the selection runs over its 15 273 water atoms (SOL),
          the anchor group is everything in front of them (lipids and peptide)
The shape is a cylinder along z, a quarter of the cell's x length in radius, whose base centre is stored as (0, 0, -h/2) and anchored
at the anchor group's centre of every frame (gr_group_center_batch, once, outside the timing).  Its height h is a quarter of the cell
in the water box, and the cell's whole z length in `aa`: the water above, below and inside a pore through the membrane.
Alternating in one process, --steps timed calls (after --warmup of each) of
  region        Region.select over all frames (three launches and one read-back of the counts per piece); the lists stay on the device
  per_slot      the path that exists without it: one gr_sel_filter_geometry call per slot, with that frame's cylinder (made outside
                the timing) and preallocated output blocks -- a launch, a synchronisation and the host's walk of the mask per frame
  all_atoms     the yardstick: group_center_batch("all", naive) of the same frames -- the memory system's pace for one read of the
                positions by existing code
and, from their medians: us per frame of each and the two ratios per_slot / region and region / all_atoms.  No threshold is set.
Prints one JSON line; --out also writes it (profiles/region_bench.json)."""
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
    rng = np.random.default_rng(20261010)
    box = [22.0, 22.0, 22.0]
    s = G.System(n, n_slots=nf, device=0)
    s.set_frame((rng.random((n, 3)) * 22.0).astype(np.float32), box, slot=0)
    for f in range(1, nf):
        s.copy_frame(f, 0)
    s.group_create_from_ranges("anchor", [(0, 2999)])
    s.group_create_from_ranges("water", [(0, n - 1)])
    return s, 5.5, 5.5


def aa(G, nf):
    d = np.load(os.path.join(ROOT, "tests", "golden", "aa_full.npz"))
    sol = np.nonzero(d["resname"] == b"SOL")[0]
    s = G.System(len(d["resid"]), n_slots=nf, device=0)
    for f in range(nf):
        s.set_frame(d["frames"][f % 2], d["boxes9"][f % 2], slot=f)
    s.group_create_from_ranges("anchor", [(0, int(sol[0]) - 1)])
    s.group_create_from_indices("water", sol)
    return s, 0.25 * float(d["boxes9"][0][0]), float(d["boxes9"][0][2])


def measure(G, s, radius, height, nf, steps, warmup):
    lib = G._lib.load()
    anchors, st = s.group_center_batch("anchor", G._lib.CENTER_PBC, 0, 0, nf)
    assert not st.any()
    region = G.Region(s, [G.Cylinder([0.0, 0.0, -0.5 * height], radius, height, G.Dimension.Z)])
    # the per-slot loop: the frame's own cylinder, the group's blocks and the output blocks made once
    offset = np.array([0.0, 0.0, -0.5 * height], np.float32)
    shapes = [G.shapes.pack([G.Cylinder(offset + anchors[f], radius, height, G.Dimension.Z)]) for f in range(nf)]
    blocks = np.asarray(s.group_container("water").blocks, np.uint64).reshape(-1, 2)
    b0, b1 = np.ascontiguousarray(blocks[:, 0]), np.ascontiguousarray(blocks[:, 1])
    n_water = s.group_get_n_atoms("water")
    o0, o1 = np.zeros(n_water, np.uint64), np.zeros(n_water, np.uint64)
    nb, na = C.c_size_t(0), C.c_uint64(0)
    picked = np.zeros(nf, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def per_slot():
        for f in range(nf):
            st = lib.gr_sel_filter_geometry(s._ctx, f, vp(b0), vp(b1), b0.size, shapes[f][0], 1, 0, vp(o0), vp(o1), n_water, C.byref(nb), C.byref(na))
            assert st == 0
            picked[f] = na.value

    counts = [None]

    def batched():
        counts[0], _ = region.select("water", 0, nf, anchors=anchors)

    calls = {"region": batched, "per_slot": per_slot, "all_atoms": lambda: s.group_center_batch("all", G._lib.CENTER_NAIVE, 0, 0, nf)}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    assert np.array_equal(counts[0], picked), "the batch and the per-slot loop disagree"
    res = {k: [] for k in calls}
    for _ in range(steps):                        # alternate the three, one timed call each per round
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            res[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) / nf * 1e6 for k, v in res.items()}
    out = {"atoms": s.n_atoms, "selection_atoms": n_water, "frames_per_call": nf, "cylinder_radius_height": [radius, height],
           "inside_per_frame_mean": float(counts[0].mean()), "pieces_per_call": region.stat(G._lib.RG_STAT_LAST_PIECES),
           "launches_per_call": region.stat(G._lib.RG_STAT_LAST_LAUNCHES),
           "region_us_per_frame": med["region"], "region_us_per_frame_min": float(min(res["region"])) / nf * 1e6,
           "per_slot_us_per_frame": med["per_slot"], "all_atoms_us_per_frame": med["all_atoms"],
           "per_slot_over_region": med["per_slot"] / med["region"], "region_over_all_atoms": med["region"] / med["all_atoms"]}
    region.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/region_bench.py", "calls": a.steps, "warmup": a.warmup}
    for name, make in (("water", lambda: water(G, a.atoms, a.frames)), ("aa", lambda: aa(G, a.frames))):
        s, radius, height = make()
        out[name] = measure(G, s, radius, height, a.frames, a.steps, a.warmup)
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

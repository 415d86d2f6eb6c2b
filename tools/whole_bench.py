#!/usr/bin/env python3
"""make_molecules_whole / make_group_whole on resident frames: time per 1e6-atom frame.

The 1e6-atom water box of tools/hbond_bench.py (333 334 waters, O-H bonds) with every atom wrapped into the cell on its own --
the molecules on the faces are broken, as a trajectory stores them -- in --frames slots (256 by default), in an orthorhombic cell
and in a rhombic-dodecahedral cell of the same volume.  Per cell, alternating in one process, --steps timed calls (after --warmup)
of each of
  make_molecules_whole_batch(0, frames)
  make_group_whole_batch("all", 0, frames)
  group_wrap_batch("all", 0, frames)          the yardstick: one read and one write of every atom
and their medians in us per frame.  Each call rewrites the frames in place; once whole they stay whole, so every timed call does
the same work.  The check / placement split and the HBM bytes come from separate rocprofv3 runs of this script
(--kernel-trace --stats; --pmc FETCH_SIZE, --pmc WRITE_SIZE).  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hbond_bench import water_box  # noqa: E402


def cell(kind, L):
    if kind == "ortho":
        return np.array([L, L, L, 0, 0, 0, 0, 0, 0], np.float32)
    d = L / 0.5 ** (1.0 / 6.0)                    # rhombic dodecahedron (xy-square) of volume L^3: d^3 / sqrt(2)
    return np.array([d, d, d * np.sqrt(0.5), 0, 0, 0, 0, d / 2, d / 2], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8, help="distinct frames (seeds) copied round the slots")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", default="ortho,dodecahedron")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    n_mol, nf = 333334, a.frames
    ow = np.arange(0, 3 * n_mol, 3)
    bonds = np.concatenate([np.stack([ow, ow + 1], 1), np.stack([ow, ow + 2], 1)])
    out = {"tool": "tools/whole_bench.py", "atoms": 3 * n_mol, "frames_per_call": nf, "calls": a.steps}
    s = G.System(3 * n_mol, n_slots=nf, device=0)
    s.add_bonds(bonds)
    for kind in a.cells.split(","):
        base = []
        for k in range(a.distinct):
            pos, b9 = water_box(n_mol, 1000 + k)
            box = cell(kind, float(b9[0]))
            lat = np.array([[box[0], 0, 0], [0, box[1], 0], [box[7], box[8], box[2]]], np.float64)
            frac = pos.astype(np.float64) @ np.linalg.inv(lat)
            base.append(((frac - np.floor(frac)) @ lat).astype(np.float32))       # every atom into the cell on its own
        for f in range(nf):
            s.set_frame(base[f % a.distinct], box, slot=f)
        calls = {"make_molecules_whole_batch": lambda: s.make_molecules_whole_batch(0, nf),
                 "make_group_whole_batch_all": lambda: s.make_group_whole_batch("all", 0, nf),
                 "group_wrap_batch_all": lambda: s.group_wrap_batch("all", 0, nf)}
        for fn in calls.values():
            for _ in range(a.warmup):
                fn()
        res = {k: [] for k in calls}
        for _ in range(a.steps):                  # alternate the three calls, one timed call each per round
            for k, fn in calls.items():
                t0 = time.perf_counter()
                st = fn()
                res[k].append(time.perf_counter() - t0)
                assert (np.asarray(st) == 0).all(), k
        r = {k: {"us_per_frame_median": float(np.median(v)) / nf * 1e6, "us_per_frame_min": float(min(v)) / nf * 1e6} for k, v in res.items()}
        r["box9"] = [float(v) for v in box]
        r["ratio_molecules_to_wrap"] = r["make_molecules_whole_batch"]["us_per_frame_median"] / r["group_wrap_batch_all"]["us_per_frame_median"]
        out[kind] = r
    s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

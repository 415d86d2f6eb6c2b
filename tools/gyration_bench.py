#!/usr/bin/env python3
"""Segments.gyration on resident frames: time per frame, next to `centers` of the same object and to the host loop it replaces.

Three systems, --frames resident frames each (64 by default):
  aa        tests/golden/aa_full.npz (32 817 atoms, its two frames in turn), masses of aa_peptide.npz; its 5 271 residues
  water     --atoms atoms (1e6) as compact 3-atom molecules, uniform in an orthorhombic 22 nm cell; one segment per molecule
  peptide   the `aa` system again, ONE segment holding its 363-atom peptide (Segments.from_group: the gmx gyrate curve)
Alternating in one process, medians of --steps timed calls (7; after --warmup of each), PBC and mass-weighted, of
  moments   gr_segments_gyration_batch_device without axes, the piece forced to all frames of the call (set_piece_frames): the call ends
            behind its own synchronise
  axes      the same with the principal axes
  centers   gr_segments_center_batch_device of the same object and frames
and, timed once over 8 frames, the loop users run today: gr_frame_download of a frame plus the numpy f64 arithmetic of
tests/gyration_ref.py (minimum image about the centre, two passes) for every segment.  Reported: us per frame of each, moments / centers,
axes / centers and host_loop / axes.  No ratio is fixed in advance.  Prints one JSON line; --out also writes it
(profiles/gyration_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PBC = 2
LOOP_FRAMES = 8


def water(G, n, nf):
    n -= n % 3
    rng = np.random.default_rng(20260605)
    centre = rng.random((n // 3, 1, 3)) * 22.0
    pos = (centre + rng.normal(0.0, 0.05, (n // 3, 3, 3))).reshape(n, 3)
    pos -= np.floor(pos / 22.0) * 22.0
    masses = np.tile(np.array([15.999, 1.008, 1.008], np.float32), n // 3)
    s = G.System(n, masses=masses, n_slots=nf, device=0)
    s.set_frame(pos.astype(np.float32), [22.0, 22.0, 22.0], slot=0)
    for f in range(1, nf):
        s.copy_frame(f, 0)
    return s, G.Segments.by_resid(s, np.arange(n, dtype=np.uint64) // 3), masses, [[22.0, 22.0, 22.0]] * nf


def aa(G, nf, peptide):
    d = np.load(os.path.join(ROOT, "tests", "golden", "aa_full.npz"))
    masses = np.load(os.path.join(ROOT, "tests", "golden", "aa_peptide.npz"))["masses"]
    s = G.System(len(masses), masses=masses, n_slots=nf, device=0)
    for f in range(nf):
        s.set_frame(d["frames"][f % 2], d["boxes9"][f % 2], slot=f)
    if peptide:
        s.group_create_from_ranges("peptide", [(0, 362)])
        return s, G.Segments.from_group(s, "peptide"), masses, [d["boxes9"][f % 2] for f in range(nf)]
    return s, G.Segments.by_resid(s, d["resid"]), masses, [d["boxes9"][f % 2] for f in range(nf)]


def measure(s, seg, masses, boxes, nf, steps, warmup):
    import gyration_ref as R
    seg.set_piece_frames(nf)                      # the device form takes one piece: all frames of the call in one block (water: 1.9 GB)
    calls = {"moments": lambda: seg.gyration_device(0, nf, PBC, 1), "axes": lambda: seg.gyration_device(0, nf, PBC, 1, axes=True),
             "centers": lambda: seg.centers_device(0, nf, PBC, 1)}
    launches = {}
    for k, fn in calls.items():
        for _ in range(warmup):
            fn()
        launches[k] = seg.stat(5)
    res = {k: [] for k in calls}
    for _ in range(steps):                        # alternate the three, one timed call each per round
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            res[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in res.items()}
    # the loop it replaces
    lists = R.flatten([seg.atoms(k) for k in range(len(seg))])      # (made once, outside the clock)
    cen, _ = seg.centers(0, LOOP_FRAMES, PBC, 1)
    loop = []
    for f in range(LOOP_FRAMES):
        t0 = time.perf_counter()
        pos = s.get_positions(f)
        S, _ = R.reference(pos, boxes[f], masses, lists, cen[f], PBC, 1)
        np.linalg.eigh(S)
        loop.append(time.perf_counter() - t0)
    out = {"segments": len(seg), "atoms": s.n_atoms, "frames_per_call": nf, "team_classes": [seg.stat(k) for k in (1, 2, 3, 4)], "launches_per_call": launches}
    for k in calls:
        out[k + "_us_per_frame"] = med[k] / nf * 1e6
        out[k + "_us_per_frame_min"] = float(min(res[k])) / nf * 1e6
    out["host_loop_us_per_frame"] = float(np.median(loop)) * 1e6
    out["moments_over_centers"] = med["moments"] / med["centers"]
    out["axes_over_centers"] = med["axes"] / med["centers"]
    out["host_loop_over_axes"] = out["host_loop_us_per_frame"] / out["axes_us_per_frame"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/gyration_bench.py", "calls": a.steps, "warmup": a.warmup, "kind": "pbc", "weighted": 1, "host_loop_frames": LOOP_FRAMES}
    for name, make in (("aa", lambda: aa(G, a.frames, False)), ("water", lambda: water(G, a.atoms, a.frames)), ("peptide", lambda: aa(G, a.frames, True))):
        s, seg, masses, boxes = make()
        out[name] = measure(s, seg, masses, boxes, a.frames, a.steps, a.warmup)
        s.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

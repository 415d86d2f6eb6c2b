#!/usr/bin/env python3
"""Segments.centers on resident frames: time per frame, next to the paths that exist without it.

Two systems, --frames resident frames each (64 by default):
  water   --atoms atoms (1e6) as compact 3-atom molecules, uniform in an orthorhombic 22 nm cell; one segment per molecule
  aa      tests/golden/aa_full.npz (32 817 atoms, its two frames in turn), masses of aa_peptide.npz; its 5 271 residues
Alternating in one process, --steps timed calls (after --warmup of each) per centre kind (naive, estimate, pbc; mass-weighted) of
  segments      gr_segments_center_batch_device over all frames: the call ends behind its own synchronise
  all_atoms     the yardstick: group_center_batch("all", same kind) of the same frames -- a read-only pass over the same atoms by
                existing code
  per_group     gr_group_center_batch of ONE segment as a group over the same frames, for 64 of the segments in turn: the path
                users have today; reported per call
and, from their medians: us per frame of `segments`, its ratio to `all_atoms`, and the ratio of the per-group loop extended to every
segment (calls x M / 64) to `segments`.  No threshold is set.  Prints one JSON line; --out also writes it
(profiles/segments_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = {"naive": 0, "estimate": 1, "pbc": 2}


def water(G, n, nf):
    n -= n % 3
    rng = np.random.default_rng(20260605)
    box = [22.0, 22.0, 22.0]
    centre = rng.random((n // 3, 1, 3)) * 22.0
    pos = (centre + rng.normal(0.0, 0.05, (n // 3, 3, 3))).reshape(n, 3)
    pos -= np.floor(pos / 22.0) * 22.0
    s = G.System(n, masses=np.tile(np.array([15.999, 1.008, 1.008], np.float32), n // 3), n_slots=nf, device=0)
    s.set_frame(pos.astype(np.float32), box, slot=0)
    for f in range(1, nf):
        s.copy_frame(f, 0)
    seg = G.Segments.by_resid(s, np.arange(n, dtype=np.uint64) // 3)
    return s, seg


def aa(G, nf):
    d = np.load(os.path.join(ROOT, "tests", "golden", "aa_full.npz"))
    masses = np.load(os.path.join(ROOT, "tests", "golden", "aa_peptide.npz"))["masses"]
    s = G.System(len(masses), masses=masses, n_slots=nf, device=0)
    for f in range(nf):
        s.set_frame(d["frames"][f % 2], d["boxes9"][f % 2], slot=f)
    return s, G.Segments.by_resid(s, d["resid"])


def measure(s, seg, nf, steps, warmup):
    m = len(seg)
    pick = np.linspace(0, m - 1, 64).astype(int)
    names = []
    for k in pick:
        a = seg.atoms(int(k))
        names.append("bench_seg%d" % k)
        s.group_create_from_indices(names[-1], a)
    out = {"segments": m, "atoms": s.n_atoms, "frames_per_call": nf,
           "team_classes": [seg.stat(k) for k in (1, 2, 3, 4)]}
    for kname, kind in KINDS.items():
        def loop():
            for g in names:
                s.group_center_batch(g, kind, 1, 0, nf)
        calls = {"segments": lambda: seg.centers_device(0, nf, kind, 1), "all_atoms": lambda: s.group_center_batch("all", kind, 1, 0, nf), "per_group": loop}
        for fn in calls.values():
            for _ in range(warmup):
                fn()
        res = {k: [] for k in calls}
        for _ in range(steps):                    # alternate the three, one timed call each per round
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                res[k].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in res.items()}
        r = {"segments_us_per_frame": med["segments"] / nf * 1e6, "segments_us_per_frame_min": float(min(res["segments"])) / nf * 1e6,
             "all_atoms_us_per_frame": med["all_atoms"] / nf * 1e6,
             "per_group_us_per_call": med["per_group"] / len(names) * 1e6,
             "launches_per_call": seg.stat(5)}
        r["segments_over_all_atoms"] = r["segments_us_per_frame"] / r["all_atoms_us_per_frame"]
        r["per_group_loop_over_segments"] = (med["per_group"] / len(names) * m) / med["segments"]
        out[kname] = r
    for g in names:
        s.group_remove(g)
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
    out = {"tool": "tools/segments_bench.py", "calls": a.steps, "warmup": a.warmup, "weighted": 1}
    for name, make in (("water", lambda: water(G, a.atoms, a.frames)), ("aa", lambda: aa(G, a.frames))):
        s, seg = make()
        out[name] = measure(s, seg, a.frames, a.steps, a.warmup)
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

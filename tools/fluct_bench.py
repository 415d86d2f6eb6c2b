#!/usr/bin/env python3
"""Fluctuations: time of accumulating resident frames into the mean structure / RMSF sums, next to two yardsticks taken in the same run.

Two cases, each at 64 and at 1 024 frames per call:
  peptide    tests/golden/aa_peptide.npz: the 363-atom peptide in its 32 817-atom system; the 21 trajectory frames in turn, each with its
             own seeded Gaussian noise of 0.01 nm on the peptide
  million    all atoms of a --atoms system (1e6): one synthetic reference and noisy, rigidly moved copies generated on the device
             (System.synth_reference / synth_frames, as bench.py does)
Per case and frame count, --steps timed calls (after --warmup of each), alternating, medians:
  accumulate  Fluctuations.accumulate of all frames in one call (after clear)              -> us per frame
  center      System.group_center_batch("all", naive) over the same frames: the project's usual yardstick (one read of the system's atoms)
  loop        the loop this replaces: gr_frame_download of a frame + a numpy accumulation of the group (origin, sum, sum of squares in
              f64), for --loop-frames frames (8); `loop_us_per_frame` is its median per frame.  It is run for that subset only: the time
              of the full loop would be that x frames.
Before anything is timed the object's mean and RMSF over the loop's frames are compared with the loop's own (`max_abs_diff_nm`).  No
threshold is set.  Prints one JSON line; --out also writes it (profiles/fluct_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def peptide(G, nf):
    d = np.load(os.path.join(ROOT, "tests", "golden", "aa_peptide.npz"))
    a, b = (int(v) for v in d["blocks_peptide"][0])
    s = G.System(d["pos"].shape[0], masses=d["masses"], n_slots=nf, device=0)
    rng = np.random.default_rng(20261020)
    x = d["pos"].copy()
    for f in range(nf):
        x[a:b + 1] = d["traj_peptide"][f % 21] + rng.normal(0.0, 0.01, (b - a + 1, 3)).astype(np.float32)
        s.set_frame(x, d["traj_boxes9"][f % 21], slot=f)
    s.group_create_from_ranges("Group", [(a, b)])
    return s, 0, np.arange(a, b + 1)


def million(G, n, nf):
    masses = np.array([1.008, 12.011, 14.007, 15.999], np.float32)[np.arange(n) % 4]
    s = G.System(n, masses=masses, n_slots=nf + 1, device=0)
    s.synth_reference(0, [10.0, 10.0, 10.0], 2.0, 20261020)
    s.synth_frames(0, 1, nf, 0, 0.05, 20261020)
    s.group_create_from_ranges("Group", [(0, n - 1)])
    return s, 1, np.arange(n)


def measure(G, s, first, idx, nf, steps, warmup, loop_frames):
    fl = G.Fluctuations(s, "Group")
    loop_state = {}

    def accumulate():
        fl.clear(); fl.accumulate(first, nf)
        s.sync()

    def center():
        s.group_center_batch("all", G._lib.CENTER_NAIVE, 0, first, nf)

    def loop():
        o = None
        for k in range(loop_frames):
            p = s.get_positions(first + k)[idx]
            if o is None:
                o, sm, sq = p.copy(), np.zeros(p.shape, np.float64), np.zeros(p.shape, np.float64)
            d = (p - o).astype(np.float64)
            sm += d; sq += d * d
        loop_state["v"] = (o, sm, sq)

    calls = {"accumulate": accumulate, "center": center, "loop": loop}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    # the object against the loop, over the loop's frames
    loop()
    o, sm, sq = loop_state["v"]
    n = float(loop_frames)
    mean = o.astype(np.float64) + sm / n
    rmsf = np.sqrt((np.maximum(sq - sm * sm / n, 0.0) / n).sum(1))
    fl.clear(); fl.accumulate(first, loop_frames)
    diff = max(float(np.abs(fl.mean() - mean).max()), float(np.abs(fl.rmsf() - rmsf).max()))
    res = {k: [] for k in calls}
    for _ in range(steps):                        # alternate them, one timed call each per round, behind an untimed call of the same kind (the
        for k, fn in calls.items():               # device idles while the loop's numpy runs: a call timed right behind it pays for the clocks coming back)
            fn()
            t0 = time.perf_counter()
            fn()
            res[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {"group_atoms": fl.n_atoms, "system_atoms": s.n_atoms, "frames": nf, "form": fl.stat(G._lib.FL_STAT_FORM),
           "range_groups": fl.stat(G._lib.FL_STAT_LAST_RANGE_GROUPS), "max_abs_diff_nm": diff, "rmsf_mean_nm": float(fl.rmsf().mean()),
           "accumulate_us_per_frame": med["accumulate"] / nf * 1e6, "accumulate_us_per_frame_min": min(res["accumulate"]) / nf * 1e6,
           "center_us_per_frame": med["center"] / nf * 1e6, "center_us_per_frame_min": min(res["center"]) / nf * 1e6,
           "loop_frames": loop_frames, "loop_us_per_frame": med["loop"] / loop_frames * 1e6, "loop_is_scaled_from_subset": True,
           "accumulate_over_center": med["accumulate"] / med["center"], "loop_over_accumulate": (med["loop"] / loop_frames) / (med["accumulate"] / nf)}
    fl.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1000000)
    ap.add_argument("--frames", default="64,1024", help="comma-separated frames per call")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=8)
    ap.add_argument("--rows", default="peptide,million", help="comma-separated: peptide, million")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    counts = [int(v) for v in a.frames.split(",")]
    out = {"tool": "tools/fluct_bench.py", "calls": a.steps, "warmup": a.warmup,
           "note": "us per frame = median wall time of one call (host clock, the call ends synchronised) / frames; loop_us_per_frame = median time of "
                   "gr_frame_download + numpy accumulation per frame, measured for loop_frames frames"}
    for row in a.rows.split(","):
        s, first, idx = peptide(G, max(counts)) if row == "peptide" else million(G, a.atoms, max(counts))
        out[row] = {str(nf): measure(G, s, first, idx, nf, a.steps, a.warmup, min(a.loop_frames, nf)) for nf in counts}
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Covariance: time of accumulating resident frames into the positional covariance sums, next to yardsticks taken in the same run.

Two cases, --frames (1 024) frames per call:
  peptide    tests/golden/aa_peptide.npz: the 363-atom peptide in its 32 817-atom system; the 21 trajectory frames in turn, each with its
             own seeded Gaussian noise of 0.01 nm on the peptide
  cap        all atoms of a GR_CV_MAX_ATOMS (4 096) atom system: one synthetic reference and noisy, rigidly moved copies generated on the
             device (System.synth_reference / synth_frames, as bench.py does)
Per case, --steps timed calls (after --warmup of each), alternating, medians:
  accumulate  Covariance.accumulate of all frames in one call (the sums go on growing: no clear between the calls)   -> us per frame, and
              f64 TFLOP/s counted on the blocks of Q that are computed: blocks x B x B x K_pad x 2 per call.  The time is the whole
              call's (position check, pack, product, the host's sync), not the product kernel's alone.
  fluct       Fluctuations.accumulate of the same frames (after clear): the diagonal alone
  loop        the loop this replaces: gr_frame_download of a frame, d = x - origin, and one numpy Q += X.T @ X of the group over
              --loop-frames frames (8); `loop_us_per_frame` is its median per frame.  It is run for that subset only.
Before anything is timed the object's covariance over the loop's frames is compared with the loop's own (`max_rel_diff`, relative to
sd_i sd_j).  No threshold is set.  Prints one JSON line; --out also writes it (profiles/covar_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RMSD_PANEL_TFLOPS = 43.0      # RMSDPanel's product kernel on the same instruction (profiles/rmsd_matrix_bench.json)


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


def cap(G, nf):
    n = G._lib.CV_MAX_ATOMS
    masses = np.array([1.008, 12.011, 14.007, 15.999], np.float32)[np.arange(n) % 4]
    s = G.System(n, masses=masses, n_slots=nf + 1, device=0)
    s.synth_reference(0, [10.0, 10.0, 10.0], 2.0, 20261020)
    s.synth_frames(0, 1, nf, 0, 0.05, 20261020)
    s.group_create_from_ranges("Group", [(0, n - 1)])
    return s, 1, np.arange(n)


def measure(G, s, first, idx, nf, steps, warmup, loop_frames):
    cv, fl = G.Covariance(s, "Group"), G.Fluctuations(s, "Group")
    loop_state = {}

    def accumulate():
        cv.accumulate(first, nf)
        s.sync()

    def fluct():
        fl.clear(); fl.accumulate(first, nf)
        s.sync()

    def loop():
        rows = []
        o = None
        for k in range(loop_frames):
            p = s.get_positions(first + k)[idx].reshape(-1)
            if o is None:
                o = p.copy()
            rows.append((p - o).astype(np.float64))
        X = np.stack(rows)
        loop_state["v"] = (X.sum(0), X.T @ X)

    calls = {"accumulate": accumulate, "fluct": fluct, "loop": loop}
    # the object against the loop, over the loop's frames
    loop()
    sm, Q = loop_state["v"]
    n = float(loop_frames)
    cov = (Q - np.outer(sm, sm) / n) / n
    cv.accumulate(first, loop_frames)
    sd = np.sqrt(np.maximum(np.diagonal(cov), 1e-300))
    diff = float((np.abs(cv.matrix() - cov) / np.outer(sd, sd)).max())
    del cov, Q
    cv.clear()
    for k, fn in calls.items():
        for _ in range(warmup if k != "loop" else 0):
            fn()
    res = {k: [] for k in calls}
    for _ in range(steps):                        # alternate them, one timed call each per round, the device calls behind an untimed call of the same kind
        for k, fn in calls.items():               # (the device idles while the loop's numpy runs: a call timed right behind it pays for the clocks coming back)
            if k != "loop":
                fn()
            t0 = time.perf_counter()
            fn()
            res[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in res.items()}
    B, T, blocks = (cv.stat(k) for k in (G._lib.CV_STAT_BLOCK_EDGE, G._lib.CV_STAT_TRIP_FRAMES, G._lib.CV_STAT_BLOCKS))
    kpad = sum(-(-min(1024, nf - k) // T) * T for k in range(0, nf, 1024))
    flop = 2.0 * blocks * B * B * kpad
    out = {"group_atoms": cv.n_atoms, "system_atoms": s.n_atoms, "frames": nf, "block_edge": B, "trip_frames": T, "blocks": blocks,
           "product_groups": cv.stat(G._lib.CV_STAT_LAST_PRODUCT_GROUPS), "max_rel_diff": diff, "counted_frames": cv.n_frames,
           "accumulate_us_per_frame": med["accumulate"] / nf * 1e6, "accumulate_us_per_frame_min": min(res["accumulate"]) / nf * 1e6,
           "flop_per_call": flop, "f64_tflops": flop / med["accumulate"] / 1e12, "f64_tflops_best": flop / min(res["accumulate"]) / 1e12,
           "rmsd_panel_tflops": RMSD_PANEL_TFLOPS,
           "fluct_us_per_frame": med["fluct"] / nf * 1e6, "accumulate_over_fluct": med["accumulate"] / med["fluct"],
           "loop_frames": loop_frames, "loop_us_per_frame": med["loop"] / loop_frames * 1e6, "loop_is_scaled_from_subset": True,
           "loop_over_accumulate": (med["loop"] / loop_frames) / (med["accumulate"] / nf)}
    cv.close(); fl.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024, help="frames per call")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=8)
    ap.add_argument("--rows", default="peptide,cap", help="comma-separated: peptide, cap")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/covar_bench.py", "calls": a.steps, "warmup": a.warmup,
           "note": "us per frame = median wall time of one call (host clock, the call ends synchronised) / frames; f64_tflops = flop of the computed "
                   "blocks / that time; loop_us_per_frame = median time of gr_frame_download + numpy X.T @ X per frame, measured for loop_frames frames"}
    for row in a.rows.split(","):
        s, first, idx = peptide(G, a.frames) if row == "peptide" else cap(G, a.frames)
        out[row] = measure(G, s, first, idx, a.frames, a.steps, a.warmup, min(a.loop_frames, a.frames))
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""MSD: time of appending resident frames to the displacement panel and of closing the band of lags, next to yardsticks of the same run.

APPEND, --frames (1 024) frames per call, after clear():
  peptide    tests/golden/aa_peptide.npz: the 363-atom peptide in its 32 817-atom system, the 21 trajectory frames in turn with seeded noise
  water      all atoms of a 1e5-atom synthetic system (System.synth_reference / synth_frames, as bench.py does)
  beside it  Fluctuations.accumulate over the same frames (after clear)                                   -> us per frame, both
COMPUTE, a 1e4-atom synthetic group, 1 024 and 4 096 frames: MSD.msd() for the full band and for max_lag = 64  -> ms per call, and f64
  TFLOP/s counted on the blocks computed: blocks x 64 x 64 x 3 n_pad x 2.  The time is the whole call's (product, closing, the sums of the
  lags, the pair counts on the host, the sync), not the product kernel's alone.
THE LOOP IT REPLACES: gr_frame_download of a frame and a numpy minimum-image unwrap against the previous one (--loop-frames frames, per
  frame), then the direct sum (d_t - d_t')^2 of one pair (--loop-pairs pairs, per pair); scaled to T frames and to the band's pairs
  (`loop_is_scaled_from_subset`).  The object's curve over the loop's frames is compared with the loop's own (`max_rel_diff`).
--steps timed calls after --warmup, alternating, medians on the host's clock.  No threshold is set.  Prints one JSON line; --out also
writes it (profiles/msd_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COVAR_TFLOPS, RMSD_PANEL_TFLOPS = 49.0, 43.0      # the project's own figures on the same instruction (profiles/covar_bench.json, rmsd_matrix_bench.json)


def peptide(G, nf):
    d = np.load(os.path.join(ROOT, "tests", "golden", "aa_peptide.npz"))
    a, b = (int(v) for v in d["blocks_peptide"][0])
    s = G.System(d["pos"].shape[0], masses=d["masses"], n_slots=nf, device=0)
    rng = np.random.default_rng(20261025)
    x = d["pos"].copy()
    for f in range(nf):
        x[a:b + 1] = d["traj_peptide"][f % 21] + rng.normal(0.0, 0.01, (b - a + 1, 3)).astype(np.float32)
        s.set_frame(x, d["traj_boxes9"][f % 21], slot=f)
    s.group_create_from_ranges("Group", [(a, b)])
    return s, 0, np.arange(a, b + 1)


def synthetic(G, n, nf):
    s = G.System(n, masses=np.ones(n, np.float32), n_slots=nf + 1, device=0)
    s.synth_reference(0, [10.0, 10.0, 10.0], 2.0, 20261025)
    s.synth_frames(0, 1, nf, 0, 0.05, 20261025)
    s.group_create_from_ranges("Group", [(0, n - 1)])
    assert s.has_box(1) and s.has_box(nf)
    return s, 1, np.arange(n)


def median_times(calls, steps, warmup):
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    res = {k: [] for k in calls}
    for _ in range(steps):                        # alternating, each timed call behind an untimed one of its kind
        for k, fn in calls.items():
            fn()
            t0 = time.perf_counter()
            fn()
            res[k].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in res.items()}, {k: float(min(v)) for k, v in res.items()}


def the_loop(s, first, idx, loop_frames, loop_pairs):
    """-> (seconds per frame of download + unwrap, seconds per pair of the direct sum, the loop's MSD curve over its frames)"""
    t0 = time.perf_counter()
    u, prev, rows = None, None, []
    for k in range(loop_frames):
        p = s.get_positions(first + k)[idx]
        if u is None:
            u = p.astype(np.float64)
        else:
            box = s.get_box(first + k)[:3]
            d = p - prev
            d -= box * np.rint(d / box)
            u = u + d
        prev = p
        rows.append(u.copy())
    per_frame = (time.perf_counter() - t0) / loop_frames
    X = np.stack(rows) - rows[0]
    t0 = time.perf_counter()
    for k in range(loop_pairs):
        a, b = k % loop_frames, (3 * k + 1) % loop_frames
        float(((X[a] - X[b]) ** 2).sum())
    per_pair = (time.perf_counter() - t0) / loop_pairs
    curve = np.array([np.mean([((X[t + tau] - X[t]) ** 2).sum() for t in range(loop_frames - tau)]) / len(idx) for tau in range(loop_frames)])
    return per_frame, per_pair, curve


def append_case(G, s, first, idx, nf, steps, warmup, loop_frames, loop_pairs):
    m, fl = G.MSD(s, "Group", nf), G.Fluctuations(s, "Group")

    def append():
        m.clear(); m.append(first, nf)
        s.sync()

    def fluct():
        fl.clear(); fl.accumulate(first, nf)
        s.sync()

    per_frame, per_pair, curve = the_loop(s, first, idx, loop_frames, loop_pairs)
    m.append(first, loop_frames)
    mine = m.msd()[0]
    diff = float(np.abs(mine[1:] - curve[1:]).max() / curve[1:].max())
    med, best = median_times({"append": append, "fluct": fluct}, steps, warmup)
    out = {"group_atoms": m.n_atoms, "system_atoms": s.n_atoms, "frames": nf, "n_pad": m.stat(G._lib.MSD_STAT_N_PAD), "walk_groups": m.stat(G._lib.MSD_STAT_LAST_WALK_GROUPS),
           "append_us_per_frame": med["append"] / nf * 1e6, "append_us_per_frame_min": best["append"] / nf * 1e6,
           "fluct_us_per_frame": med["fluct"] / nf * 1e6, "append_over_fluct": med["append"] / med["fluct"],
           "loop_frames": loop_frames, "loop_download_unwrap_us_per_frame": per_frame * 1e6, "loop_direct_us_per_pair": per_pair * 1e6, "max_rel_diff": diff,
           "loop_over_append": per_frame / (med["append"] / nf), "loop_is_scaled_from_subset": True}
    m.close(); fl.close()
    return out


def compute_case(G, s, first, idx, nf, steps, warmup, loop_frames, loop_pairs):
    m = G.MSD(s, "Group", nf)
    m.append(first, nf)
    s.sync()
    per_frame, per_pair, _ = the_loop(s, first, idx, loop_frames, loop_pairs)
    out = {"group_atoms": m.n_atoms, "frames": nf, "n_pad": m.stat(G._lib.MSD_STAT_N_PAD), "block_edge": m.stat(G._lib.MSD_STAT_BLOCK_EDGE),
           "covar_tflops": COVAR_TFLOPS, "rmsd_panel_tflops": RMSD_PANEL_TFLOPS, "loop_is_scaled_from_subset": True}
    K, B = 3 * out["n_pad"], out["block_edge"]
    for name, lag in (("full", None), ("lag64", 64)):
        med, best = median_times({"msd": lambda: m.msd(lag)}, steps, warmup)
        blocks = m.stat(G._lib.MSD_STAT_LAST_BLOCKS)
        flop = 2.0 * blocks * B * B * K
        lags = nf if lag is None else lag + 1
        pairs = sum(nf - t for t in range(lags))
        loop_s = nf * per_frame + pairs * per_pair
        out[name] = {"lags": lags, "blocks": blocks, "gram_groups": m.stat(G._lib.MSD_STAT_LAST_GRAM_GROUPS), "compute_ms": med["msd"] * 1e3, "compute_ms_min": best["msd"] * 1e3,
                     "flop_per_call": flop, "f64_tflops": flop / med["msd"] / 1e12, "f64_tflops_best": flop / best["msd"] / 1e12,
                     "pairs": pairs, "loop_s_scaled": loop_s, "loop_over_compute": loop_s / med["msd"]}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024, help="frames per append call")
    ap.add_argument("--compute-frames", default="1024,4096")
    ap.add_argument("--compute-atoms", type=int, default=10000)
    ap.add_argument("--water-atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=8)
    ap.add_argument("--loop-pairs", type=int, default=64)
    ap.add_argument("--rows", default="peptide,water,compute", help="comma-separated: peptide, water, compute")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/msd_bench.py", "calls": a.steps, "warmup": a.warmup,
           "note": "us per frame = median wall time of one call (host clock, the call ends synchronised) / frames; compute_ms = median wall time of gr_msd_compute + "
                   "gr_msd_read; f64_tflops = flop of the computed blocks / that time; the loop = gr_frame_download + numpy unwrap per frame and a direct numpy sum per "
                   "pair, measured for loop_frames frames and loop_pairs pairs and scaled"}
    loop_frames = min(a.loop_frames, a.frames)
    for row in a.rows.split(","):
        if row == "compute":
            for nf in (int(v) for v in a.compute_frames.split(",")):
                s, first, idx = synthetic(G, a.compute_atoms, nf)
                out["compute_%d" % nf] = compute_case(G, s, first, idx, nf, a.steps, a.warmup, loop_frames, a.loop_pairs)
                s.close()
            continue
        s, first, idx = peptide(G, a.frames) if row == "peptide" else synthetic(G, a.water_atoms, a.frames)
        out[row] = append_case(G, s, first, idx, a.frames, a.steps, a.warmup, loop_frames, a.loop_pairs)
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""VectorCorrelation: time of appending resident frames to the vector panels, of closing the band of lags over all vectors and of the
per-vector curves, next to yardsticks of the same run.

APPEND, --frames (1 024) frames per call, after clear(), pbc and both ranks:
  peptide    tests/golden/aa_peptide.npz: 300 neighbour pairs inside the 363-atom peptide of the 32 817-atom system (the N-H-sized case)
  water      every O-H bond of a 1e5-atom synthetic water group: atoms 3 m, 3 m + 1, 3 m + 2 -> 66 666 vectors
  beside it  MSD.append of a block of as many atoms over the same frames (after clear): the same kind of walk with one load stream
             fewer (3 loads and 3 stores per atom and frame against 6 loads and 9 stores per vector)     -> us per frame, both, the ratio
  THE LOOP IT REPLACES: gr_frame_download of a frame and a numpy gather, minimum image and normalise (--loop-frames frames, per frame)
CORRELATE, 1e4 vectors of a 2e4-atom synthetic system over --compute-frames (4 096) frames, full band and max_lag = 64: both ranks in
  one object, rank 1 alone, and MSD.msd() of a 1e4-atom group in the same session (the rank-1 product is the size of MSD's, the rank-2
  product twice as large)  -> ms per call, and f64 TFLOP/s counted on the blocks computed: blocks x 64 x 64 x K x 2 with K = 3, 6 or
  9 n_pad.  The time is the whole call's (product, the sums of the lags, the pair counts on the host, the sync, the read).
CORRELATE_EACH, 300 vectors x --compute-frames frames, full band: both ranks -> ms per call, and the pair terms per second.
--steps timed calls after --warmup, alternating, each behind an untimed one of its kind, medians on the host's clock.  No threshold is
set.  Prints one JSON line; --out also writes it (profiles/vcorr_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from msd_bench import median_times, peptide, synthetic      # noqa: E402  (the same systems as the MSD figures)


def the_loop(s, first, pairs, loop_frames):
    """seconds per frame of download + gather + minimum image (orthorhombic) + normalise in numpy"""
    t0 = time.perf_counter()
    rows = []
    for k in range(loop_frames):
        p = s.get_positions(first + k)
        box = s.get_box(first + k)[:3]
        d = p[pairs[:, 1]] - p[pairs[:, 0]]
        d -= box * np.rint(d / box)
        rows.append(d / np.sqrt((d * d).sum(1))[:, None])
    return (time.perf_counter() - t0) / loop_frames, np.stack(rows)


def append_case(G, s, first, pairs, nf, steps, warmup, loop_frames):
    V = len(pairs)
    s.group_create_from_ranges("AsMany", [(int(pairs.min()), int(pairs.min()) + V - 1)])
    v, m = G.VectorCorrelation(s, pairs, nf, pbc=True), G.MSD(s, "AsMany", nf)

    def append():
        v.clear(); v.append(first, nf)
        s.sync()

    def msd():
        m.clear(); m.append(first, nf)
        s.sync()

    per_frame, rows = the_loop(s, first, pairs, loop_frames)
    v.append(first, loop_frames)
    diff = float(np.abs(v.vectors(0, loop_frames) - rows).max())
    med, best = median_times({"append": append, "msd": msd}, steps, warmup)
    n_pad = v.stat(G._lib.VCORR_STAT_N_PAD)
    # bytes a walk moves per frame: vcorr 6 loads + 9 stores of 4 B per (padded) vector, MSD 3 loads + 3 stores per (padded) atom
    out = {"vectors": V, "system_atoms": s.n_atoms, "frames": nf, "n_pad": n_pad, "walk_groups": v.stat(G._lib.VCORR_STAT_LAST_WALK_GROUPS),
           "append_us_per_frame": med["append"] / nf * 1e6, "append_us_per_frame_min": best["append"] / nf * 1e6,
           "msd_atoms": m.n_atoms, "msd_append_us_per_frame": med["msd"] / nf * 1e6, "append_over_msd_append": med["append"] / med["msd"],
           "bytes_per_frame": 15 * 4 * n_pad, "msd_bytes_per_frame": 6 * 4 * m.stat(G._lib.MSD_STAT_N_PAD), "bytes_ratio": 15.0 / 6.0,
           "loop_frames": loop_frames, "loop_download_gather_us_per_frame": per_frame * 1e6, "max_abs_diff_to_loop": diff,
           "loop_over_append": per_frame / (med["append"] / nf)}
    v.close(); m.close()
    return out


def correlate_case(G, n_vectors, nf, steps, warmup):
    s, first, idx = synthetic(G, 2 * n_vectors, nf)
    s.group_create_from_ranges("Half", [(0, n_vectors - 1)])
    pairs = np.stack([np.arange(0, 2 * n_vectors, 2), np.arange(1, 2 * n_vectors, 2)], 1)
    both, one, m = G.VectorCorrelation(s, pairs, nf, pbc=True), G.VectorCorrelation(s, pairs, nf, rank=1, pbc=True), G.MSD(s, "Half", nf)
    for o in (both, one, m):
        o.append(first, nf)
    s.sync()
    n_pad, B = both.stat(G._lib.VCORR_STAT_N_PAD), 64
    out = {"vectors": n_vectors, "frames": nf, "n_pad": n_pad, "msd_atoms": m.n_atoms, "msd_n_pad": m.stat(G._lib.MSD_STAT_N_PAD)}
    for name, lag in (("full", None), ("lag64", 64)):
        med, best = median_times({"both": lambda: both.correlate(lag), "rank1": lambda: one.correlate(lag), "msd": lambda: m.msd(lag)}, steps, warmup)
        blocks = both.stat(G._lib.VCORR_STAT_LAST_BLOCKS)
        assert blocks == one.stat(G._lib.VCORR_STAT_LAST_BLOCKS) == m.stat(G._lib.MSD_STAT_LAST_BLOCKS)
        flop = 2.0 * blocks * B * B * n_pad
        row = {"lags": nf if lag is None else lag + 1, "blocks": blocks, "gram_groups": both.stat(G._lib.VCORR_STAT_LAST_GRAM_GROUPS)}
        for key, comps in (("both", 9), ("rank1", 3), ("msd", 3)):
            row[key + "_ms"] = med[key] * 1e3
            row[key + "_ms_min"] = best[key] * 1e3
            row[key + "_f64_tflops"] = comps * flop / med[key] / 1e12
        row["rank1_over_msd"] = med["rank1"] / med["msd"]
        row["both_over_msd"] = med["both"] / med["msd"]
        out[name] = row
    for o in (both, one, m):
        o.close()
    s.close()
    return out


def each_case(G, n_vectors, nf, steps, warmup):
    s, first, idx = synthetic(G, 2 * n_vectors, nf)
    pairs = np.stack([np.arange(0, 2 * n_vectors, 2), np.arange(1, 2 * n_vectors, 2)], 1)
    v = G.VectorCorrelation(s, pairs, nf, pbc=True)
    v.append(first, nf)
    s.sync()
    med, best = median_times({"each": lambda: v.correlate_each()}, steps, warmup)
    terms = n_vectors * (nf * (nf + 1) // 2) * 9.0              # pair terms of both ranks: one f64 fma each
    out = {"vectors": n_vectors, "frames": nf, "lags": nf, "each_groups": v.stat(G._lib.VCORR_STAT_LAST_EACH_GROUPS), "each_ms": med["each"] * 1e3, "each_ms_min": best["each"] * 1e3,
           "terms": terms, "gterms_per_s": terms / med["each"] / 1e9, "output_mib": 2 * n_vectors * nf * 8 / 2.0 ** 20}
    v.close(); s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024, help="frames per append call")
    ap.add_argument("--compute-frames", type=int, default=4096)
    ap.add_argument("--compute-vectors", type=int, default=10000)
    ap.add_argument("--each-vectors", type=int, default=300)
    ap.add_argument("--water-atoms", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=8)
    ap.add_argument("--rows", default="peptide,water,correlate,each", help="comma-separated: peptide, water, correlate, each")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/vcorr_bench.py", "calls": a.steps, "warmup": a.warmup,
           "note": "us per frame = median wall time of one call (host clock, the call ends synchronised) / frames; *_ms = median wall time of the whole call "
                   "(gr_vcorr_compute + gr_vcorr_read, gr_msd_compute + gr_msd_read, gr_vcorr_compute_each); f64_tflops = flop of the computed blocks / that time; "
                   "the loop = gr_frame_download + numpy gather, minimum image and normalise per frame, measured for loop_frames frames"}
    loop_frames = min(a.loop_frames, a.frames)
    for row in a.rows.split(","):
        if row == "correlate":
            out["correlate"] = correlate_case(G, a.compute_vectors, a.compute_frames, a.steps, a.warmup)
        elif row == "each":
            out["each"] = each_case(G, a.each_vectors, a.compute_frames, a.steps, a.warmup)
        elif row == "peptide":
            s, first, idx = peptide(G, a.frames)
            out[row] = append_case(G, s, first, np.stack([idx[:300], idx[1:301]], 1), a.frames, a.steps, a.warmup, loop_frames)
            s.close()
        else:
            s, first, idx = synthetic(G, a.water_atoms, a.frames)
            o = np.arange(0, a.water_atoms - 2, 3)
            out[row] = append_case(G, s, first, np.concatenate([np.stack([o, o + 1], 1), np.stack([o, o + 2], 1)]), a.frames, a.steps, a.warmup, loop_frames)
            s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

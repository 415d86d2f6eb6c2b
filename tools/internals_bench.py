#!/usr/bin/env python3
"""Internals: time of the series (values) and of the running statistics (accumulate) of atom tuples over resident frames, next to
yardsticks of the same run.

  phipsi     tests/golden/aa_peptide.npz + aa_hbond_topology.npz: every proper dihedral of the 363-atom peptide's bonds
             (dihedrals_from_bonds) in its 32 817-atom system, --frames (1 024) frames: the 21 trajectory frames in turn with seeded noise
  water      every O-H bond of a synthetic --water-atoms (1e6) system (atoms 3m, 3m + 1, 3m + 2 taken as O, H, H; System.synth_reference /
             synth_frames, as bench.py does) as "axis" against z, --water-frames (64) frames
  per case   values (host array), values_device (a torch tensor on the device: no copy out), accumulate (after clear)
  beside it  group_center_batch("all", naive) over the same frames: it streams every atom of every frame once, the memory system's pace
  the loop it replaces: gr_frame_download of a frame and the same formula in numpy (--loop-frames frames, per frame; scaled to the
             case's frames: `loop_is_scaled_from_subset`); the largest difference between the loop's values and the object's is reported
--steps timed calls after --warmup, alternating, medians on the host's clock.  No threshold is set.  Prints one JSON line; --out also
writes it (profiles/internals_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def phipsi(G, nf):
    d = np.load(os.path.join(ROOT, "tests", "golden", "aa_peptide.npz"))
    bonds = np.load(os.path.join(ROOT, "tests", "golden", "aa_hbond_topology.npz"))["peptide_bonds"]
    a, b = (int(v) for v in d["blocks_peptide"][0])
    s = G.System(d["pos"].shape[0], masses=d["masses"], n_slots=nf, device=0)
    rng = np.random.default_rng(20261021)
    x = d["pos"].copy()
    for f in range(nf):
        x[a:b + 1] = d["traj_peptide"][f % 21] + rng.normal(0.0, 0.01, (b - a + 1, 3)).astype(np.float32)
        s.set_frame(x, d["traj_boxes9"][f % 21], slot=f)
    return s, 0, "dihedral", G.dihedrals_from_bonds(bonds) + np.uint64(a), None


def water(G, n, nf):
    n -= n % 3
    s = G.System(n, masses=np.ones(n, np.float32), n_slots=nf + 1, device=0)
    s.synth_reference(0, [22.0, 22.0, 22.0], 2.0, 20261021)
    s.synth_frames(0, 1, nf, 0, 0.05, 20261021)
    o = 3 * np.arange(n // 3, dtype=np.uint64)
    t = np.stack([np.repeat(o, 2), (o[:, None] + np.array([1, 2], np.uint64)[None, :]).ravel()], 1)
    return s, 1, "axis", t, (0.0, 0.0, 1.0)


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


def numpy_values(kind, x, t, box, axis):
    def disp(a, b):
        d = x[t[:, b]] - x[t[:, a]]
        return d - box * np.rint(d / box)
    if kind == "axis":
        d = disp(0, 1)
        return (d @ np.asarray(axis, np.float32)) / np.sqrt((d * d).sum(1))
    b1, b2, b3 = disp(0, 1), disp(1, 2), disp(2, 3)
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return np.arctan2(np.sqrt((b2 * b2).sum(1)) * (b1 * n2).sum(1), (n1 * n2).sum(1))


def case(G, s, first, kind, t, axis, nf, steps, warmup, loop_frames):
    import torch
    ic = G.Internals(s, kind, t, axis=axis)
    out_dev = torch.empty((nf, len(t)), dtype=torch.float32, device="cuda:0")
    ti = t.astype(np.int64)

    def accumulate():
        ic.clear(); ic.accumulate(first, nf)
        s.sync()

    t0 = time.perf_counter()
    loop = []
    for k in range(loop_frames):                  # the loop it replaces (orthorhombic boxes: the diagonal is the whole box)
        loop.append(numpy_values(kind, s.get_positions(first + k), ti, s.get_box(first + k)[:3], axis))
    per_frame = (time.perf_counter() - t0) / loop_frames
    mine = ic.values(first, loop_frames)[0]
    diff = np.abs(np.stack(loop) - mine)
    if kind == "dihedral":
        diff = np.minimum(diff, np.abs(2 * np.pi - diff))
    calls = {"values": lambda: ic.values(first, nf), "values_device": lambda: (ic.values_device(out_dev, first, nf), s.sync()), "accumulate": accumulate,
             "center_all_naive": lambda: s.group_center_batch("all", G._lib.CENTER_NAIVE, 0, first, nf)}
    med, best = median_times(calls, steps, warmup)
    assert np.array_equal(out_dev[:loop_frames].cpu().numpy().view(np.uint32), mine.view(np.uint32))
    arity = t.shape[1]
    res = {"kind": kind, "tuples": len(t), "system_atoms": s.n_atoms, "frames": nf, "range_groups": ic.stat(G._lib.IC_STAT_LAST_RANGE_GROUPS),
           "gather_bytes_per_frame": 12 * arity * len(t), "frame_bytes": 12 * s.n_atoms, "loop_frames": loop_frames, "loop_is_scaled_from_subset": True,
           "loop_download_numpy_us_per_frame": per_frame * 1e6, "max_abs_diff_to_loop": float(diff.max())}
    for k in calls:
        res[k + "_us_per_frame"] = med[k] / nf * 1e6
        res[k + "_us_per_frame_min"] = best[k] / nf * 1e6
    res["values_device_over_center"] = med["values_device"] / med["center_all_naive"]
    res["accumulate_over_center"] = med["accumulate"] / med["center_all_naive"]
    res["loop_over_values"] = per_frame / (med["values"] / nf)
    res["loop_over_accumulate"] = per_frame / (med["accumulate"] / nf)
    ic.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024, help="frames of the phi/psi-sized case")
    ap.add_argument("--water-atoms", type=int, default=1000000)
    ap.add_argument("--water-frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-frames", type=int, default=8)
    ap.add_argument("--rows", default="phipsi,water", help="comma-separated: phipsi, water")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/internals_bench.py", "calls": a.steps, "warmup": a.warmup,
           "note": "us per frame = median wall time of one call (host clock, the call ends synchronised) / frames; values ends with the copy into a pageable host "
                   "array, values_device leaves the rows in a torch tensor; center_all_naive = group_center_batch('all', naive) over the same frames; the loop = "
                   "gr_frame_download + the formula in numpy per frame, measured for loop_frames frames"}
    for row in a.rows.split(","):
        if row == "phipsi":
            s, first, kind, t, axis = phipsi(G, a.frames)
            nf = a.frames
        else:
            s, first, kind, t, axis = water(G, a.water_atoms, a.water_frames)
            nf = a.water_frames
        out[row] = case(G, s, first, kind, t, axis, nf, a.steps, a.warmup, min(a.loop_frames, nf))
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

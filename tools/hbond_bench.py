#!/usr/bin/env python3
"""Hydrogen bonds on resident frames (gr_hbond_batch): time per frame of the two workloads of the feature.

  aa    the aa_membrane_peptide water (OW donors with HW1 / HW2, OW acceptors) at 0.3 nm / 150 deg: frames 0 and 20 of
        tests/golden/aa_full.npz jittered (sigma 0.005 nm, seeded) into 256 distinct slots, 256 frames per call
  box   a seeded 1e6-atom water box (33.4 O / nm^3, O-H 0.1 nm, HOH 104.5 deg, random orientations), 64 distinct frames
        (independent seeds), 64 frames per call, 0.3 nm / 150 deg

For each: us per frame and frames/s (median of --steps timed calls after --warmup), candidates per frame (donor-acceptor
pairs within max_distance: the same plan with min_angle = -1 counts every candidate once per hydrogen) and bonds per frame.
The split between grid build and walk comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/hbond_bench.py`
run (k_hb_assign + scan + k_hb_scatter vs k_hb_walk).  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def water_box(n_mol, seed, density=33.4):
    rng = np.random.default_rng(seed)
    L = (n_mol / density) ** (1.0 / 3.0)
    o = rng.uniform(0, L, (n_mol, 3))
    u = rng.normal(size=(n_mol, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    w = rng.normal(size=(n_mol, 3)); w -= (w * u).sum(1)[:, None] * u; w /= np.linalg.norm(w, axis=1)[:, None]
    half = np.deg2rad(104.5) / 2
    h1 = o + 0.1 * (np.cos(half) * u + np.sin(half) * w)
    h2 = o + 0.1 * (np.cos(half) * u - np.sin(half) * w)
    return np.stack([o, h1, h2], 1).reshape(-1, 3).astype(np.float32), np.array([L, L, L] + [0.0] * 6, np.float32)


def run(G, s, ow, hw, bonds, nf, steps, warmup, dmax=0.3, amin=150.0):
    s.group_create_from_indices("OW", ow.tolist())
    s.group_create_from_indices("HW", hw.tolist())
    an = G.HBondAnalysis(s, [G.HBondChain("OW", "OW", "HW")], [(0, 0)], dmax, amin, bonds)
    for _ in range(warmup):
        res = an.batch(0, nf)
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = an.batch(0, nf)
        times.append(time.perf_counter() - t0)
    assert (res[6] == 0).all()
    cand = G.HBondAnalysis(s, [G.HBondChain("OW", "OW", "HW")], [(0, 0)], dmax, -1.0, bonds)
    _, _, n_cand_h = cand.count(0, nf)
    t = float(np.median(times))
    return {"frames_per_call": nf, "calls": steps, "s_per_call_median": t, "s_per_call_min": float(min(times)),
            "us_per_frame": t / nf * 1e6, "frames_per_s": nf / t, "bonds_per_frame": int(res[5][-1]) / nf,
            "candidates_per_frame": n_cand_h / 2 / nf, "atoms": int(s.n_atoms), "donors": int(ow.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("aa", "box", "all"), default="all")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--box-frames", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hbond_ref as R
    out = {"tool": "tools/hbond_bench.py", "max_distance": 0.3, "min_angle": 150.0}
    if a.workload in ("aa", "all"):
        d = np.load(os.path.join(ROOT, "tests", "golden", "aa_full.npz"))
        ow, hw, bonds = R.water_topology(d["atomname"])
        nf = 256
        s = G.System(d["frames"].shape[1], n_slots=nf, device=0)
        rng = np.random.default_rng(20261016)
        for f in range(nf):
            s.set_frame(d["frames"][f % 2] + rng.normal(0, 0.005, d["frames"].shape[1:]).astype(np.float32), d["boxes9"][f % 2], slot=f)
        out["aa_water"] = run(G, s, ow, hw, bonds, nf, a.steps, a.warmup)
        s.close()
    if a.workload in ("box", "all"):
        n_mol, nf = 333334, a.box_frames
        ow = np.arange(0, 3 * n_mol, 3); hw = np.sort(np.concatenate([ow + 1, ow + 2]))
        bonds = np.concatenate([np.stack([ow, ow + 1], 1), np.stack([ow, ow + 2], 1)])
        s = G.System(3 * n_mol, n_slots=nf, device=0)
        for f in range(nf):
            pos, b9 = water_box(n_mol, 1000 + f)
            s.set_frame(pos, b9, slot=f)
        out["water_box_1e6"] = run(G, s, ow, hw, bonds, nf, a.steps, a.warmup)
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

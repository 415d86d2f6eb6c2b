#!/usr/bin/env python3
"""RMSDPanel / rmsd_matrix: time of packing frames and of the all-pairs matrix, next to the loop it replaces.

Two rows, --frames frames each (1 024):
  peptide    tests/golden/aa_peptide.npz: the 363-atom peptide in its 32 817-atom system; the 21 trajectory frames in turn, each with its
             own seeded Gaussian noise of 0.01 nm on the peptide (so no two frames are equal)
  synthetic  a group of --atoms atoms (1e4) that is its whole system: one synthetic reference and --frames noisy, rigidly moved copies,
             generated on the device (System.synth_reference / synth_frames, as bench.py does)
Per row, --steps timed calls (after --warmup of each), medians:
  append     RMSDPanel.append of all frames in one call (after clear)                       -> us per frame
  matrix     rmsd_matrix(panel, device=True): the product kernel and its closing, no copy     -> ms, pairs/s, f64 FLOP/s of the product
             (2 * 18 * N per pair, counted for all F^2 pairs of the result; the kernel computes one triangle of them and mirrors it,
             `flops_computed` counts only the blocks it runs)
  matrix_host rmsd_matrix(panel): the same plus the copy to the host
  loop       the path that exists without the object, on the same build: gr_rmsd_plan_create on frame j + gr_rmsd_batch over all frames,
             for --refs reference frames (8) spread over the trajectory; `loop_ms_scaled` = median per reference frame x frames.  It is
             run for that subset only and scaled -- the full loop would take `loop_ms_scaled`.
Before anything is timed, the matrix's columns of those reference frames are compared with the loop's results (`max_abs_diff_nm`).
No threshold is set.  Prints one JSON line; --out also writes it (profiles/rmsd_matrix_bench.json)."""
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
    return s, 0


def synthetic(G, n, nf):
    masses = np.array([1.008, 12.011, 14.007, 15.999], np.float32)[np.arange(n) % 4]
    s = G.System(n, masses=masses, n_slots=nf + 1, device=0)
    s.synth_reference(0, [10.0, 10.0, 10.0], 2.0, 20261020)
    s.synth_frames(0, 1, nf, 0, 0.05, 20261020)
    s.group_create_from_ranges("Group", [(0, n - 1)])
    return s, 1


def measure(G, s, first, nf, steps, warmup, n_refs):
    panel = G.RMSDPanel(s, "Group", nf)
    n = panel.n_atoms
    refs = sorted({int(v) for v in np.linspace(0, nf - 1, n_refs)})
    loop_cols = {}

    def append():
        panel.clear(); panel.append(first, nf)

    def matrix(): G.rmsd_matrix(panel, device=True)
    def matrix_host(): return G.rmsd_matrix(panel)

    def loop():
        for j in refs:
            plan = G.RMSDPlan(s, s, "Group", ref_slot=first + j)
            loop_cols[j] = plan.rmsd(first, nf)[0]
            plan.close()

    calls = {"append": append, "matrix": matrix, "matrix_host": matrix_host, "loop": loop}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    M = matrix_host()
    diff = max(float(np.abs(M[:, j] - loop_cols[j]).max()) for j in refs)
    res = {k: [] for k in calls}
    for _ in range(steps):                        # alternate them, one timed call each per round
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            res[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in res.items()}
    pairs = float(nf) * nf
    blocks = sum(1 for bi in range((nf + 7) // 8) for bj in range((nf + 15) // 16) if 8 * bi <= 16 * bj + 15)
    out = {"group_atoms": n, "system_atoms": s.n_atoms, "frames": nf, "symmetric": bool(np.array_equal(M, M.T)), "max_abs_diff_nm": diff,
           "rmsd_mean_nm": float(M.mean()), "rmsd_max_nm": float(M.max()),
           "append_us_per_frame": med["append"] / nf * 1e6, "append_us_per_frame_min": min(res["append"]) / nf * 1e6,
           "matrix_ms": med["matrix"] * 1e3, "matrix_ms_min": min(res["matrix"]) * 1e3, "matrix_host_ms": med["matrix_host"] * 1e3,
           "pairs_per_s": pairs / med["matrix"], "product_f64_flops": 2.0 * 18.0 * n * pairs / med["matrix"],
           "flops_computed": 2.0 * 48.0 * 48.0 * ((n + 15) // 16 * 16) * blocks / med["matrix"],
           "loop_reference_frames": len(refs), "loop_ms_per_reference_frame": med["loop"] / len(refs) * 1e3,
           "loop_ms_scaled": med["loop"] / len(refs) * nf * 1e3, "loop_is_scaled_from_subset": True,
           "loop_over_matrix": med["loop"] / len(refs) * nf / (med["matrix"] + med["append"])}
    panel.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--refs", type=int, default=8)
    ap.add_argument("--rows", default="peptide,synthetic", help="comma-separated: peptide, synthetic")
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    out = {"tool": "tools/rmsd_matrix_bench.py", "calls": a.steps, "warmup": a.warmup,
           "note": "loop_ms_scaled = (median time of plan_create + rmsd_batch over all frames, per reference frame, measured for loop_reference_frames of them) x frames; "
                   "loop_over_matrix compares it with append + matrix"}
    rows = a.rows.split(",")
    if "peptide" in rows:
        s, first = peptide(G, a.frames)
        out["peptide"] = measure(G, s, first, a.frames, a.steps, a.warmup, a.refs)
        s.close()
    if "synthetic" in rows:
        s, first = synthetic(G, a.atoms, a.frames)
        out["synthetic"] = measure(G, s, first, a.frames, a.steps, a.warmup, a.refs)
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""GridMap.accumulate on resident frames: time per 1e6-atom frame.

1e6 atoms uniform in an orthorhombic 10 x 10 x 10 nm cell (gr_synth_uniform, one seed per slot) in --frames slots (256 by default),
group "all".  Alternating in one process, --steps timed calls (after --warmup) of each of
  lds_count / lds_z            a from_box map of 0.15 x 0.20 nm tiles (68 x 51: privatised in LDS), COUNT and Z
  forced_count / forced_z      the same map with GR_GM_FORCE_GLOBAL
  global_count / global_z      a from_box map of 0.02 x 0.02 nm tiles (501 x 501: global atomics by itself)
  center_naive                 the yardstick: group_center_batch(GR_CENTER_NAIVE) of the same group and frames, a read-only pass over
                               the same bytes
and then, with every slot rewritten so that all atoms sit in ONE tile (the worst case for the atomics),
  onetile_global_count / _z    the 501 x 501 map
  onetile_lds_count / _z       the 68 x 51 map
and their medians in us per frame, with the ratios to the yardstick.  The path each map took is read from the map's own counters and
asserted.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=1000000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import groan_rs_amd as G
    from groan_rs_amd import _lib
    n, nf = a.atoms, a.frames
    box = [10.0, 10.0, 10.0]
    s = G.System(n, n_slots=nf, device=0)
    for f in range(nf):
        s.synth_uniform(f, box, 1000 + f)
    small = G.GridMap.from_box(s, (0.15, 0.20))
    forced = G.GridMap.from_box(s, (0.15, 0.20))
    large = G.GridMap.from_box(s, (0.02, 0.02))
    Z = G.Dimension.Z
    out = {"tool": "tools/gridmap_bench.py", "atoms": n, "frames_per_call": nf, "calls": a.steps, "box": box,
           "lds_map": [small.n_tiles_x, small.n_tiles_y], "global_map": [large.n_tiles_x, large.n_tiles_y],
           "lds_budget_bytes": small.stat(_lib.GM_STAT_LDS_BUDGET)}

    def acc(m, value, force=False):
        def fn():
            return m.accumulate("all", 0, nf, value=value, force_global=force)[1]
        return fn

    def run(calls):
        for fn in calls.values():
            for _ in range(a.warmup):
                fn()
        res = {k: [] for k in calls}
        for _ in range(a.steps):                  # alternate the calls, one timed call each per round
            for k, fn in calls.items():
                t0 = time.perf_counter()
                st = fn()
                res[k].append(time.perf_counter() - t0)
                assert (np.asarray(st) == 0).all(), k
        return {k: {"us_per_frame_median": float(np.median(v)) / nf * 1e6, "us_per_frame_min": float(min(v)) / nf * 1e6} for k, v in res.items()}

    r = run({"lds_count": acc(small, "count"), "lds_z": acc(small, Z), "forced_count": acc(forced, "count", True), "forced_z": acc(forced, Z, True),
             "global_count": acc(large, "count"), "global_z": acc(large, Z),
             "center_naive": lambda: s.group_center_batch("all", _lib.CENTER_NAIVE, 0, 0, nf)[1]})
    assert small.stat(_lib.GM_STAT_GLOBAL_LAUNCHES) == 0 and forced.stat(_lib.GM_STAT_LDS_LAUNCHES) == 0 and large.stat(_lib.GM_STAT_LDS_LAUNCHES) == 0
    total = int(small.counts.sum())
    assert total + 0 <= 2 * (a.steps + a.warmup) * nf * n and total > 0
    # the worst case: every atom of every frame in one tile
    one = np.empty((n, 3), np.float32)
    one[:, 0] = 5.0; one[:, 1] = 5.0; one[:, 2] = np.linspace(0.0, 10.0, n, dtype=np.float32)
    s.set_frame(one, box, slot=0)
    for f in range(1, nf):
        s.copy_frame(f, 0)
    small.clear(); large.clear()
    r.update(run({"onetile_global_count": acc(large, "count"), "onetile_global_z": acc(large, Z), "onetile_lds_count": acc(small, "count"), "onetile_lds_z": acc(small, Z)}))
    cnt = large.counts
    assert int(cnt.max()) == int(cnt.sum()) == 2 * (a.steps + a.warmup) * nf * n
    base = r["center_naive"]["us_per_frame_median"]
    out["us_per_frame"] = r
    out["ratio_to_center_naive"] = {k: v["us_per_frame_median"] / base for k, v in r.items() if k != "center_naive"}
    out["lds_over_forced_global"] = {"count": r["lds_count"]["us_per_frame_median"] / r["forced_count"]["us_per_frame_median"],
                                     "z": r["lds_z"]["us_per_frame_median"] / r["forced_z"]["us_per_frame_median"]}
    s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

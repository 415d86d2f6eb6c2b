#!/usr/bin/env python3
"""bench.py -- frames/s of the RMSD-fit hot path on synthetic 1e6-atom frames resident in HBM.

Workload (BASELINE.json metric): 1e6 atoms in a rhombic-dodecahedral (triclinic) box
(lengths d,d,d, angles 60,60,90, d = 24.18 nm); reference = blob of radius 0.2 x (shortest box height) about
the box centre; frame f = R_f (x0 - c) + c + t_f + noise(0.05 nm), wrapped into the cell (so the blob is
broken across the periodic boundaries); masses {1.008,12.011,14.007,15.999}[i mod 4]; group = all atoms.
One "step" = gr_rmsd_fit_batch over `--frames-per-step` frames (RMSD + in-place fit of every atom).
Every frame of warmup + timed steps is a DISTINCT, freshly generated PBC-broken frame in its own HBM-resident buffer:
frames-per-step is sized so that (steps + warmup) x frames-per-step fits the pool (768 frames per step = 230 GB for the
driver's --steps 20 --warmup 5), and `config.reused_frames` (0 unless the caller forces more work than 288 GB hold) says so.

  python bench.py                      # 1 GPU
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N   # one rank per GPU

Multi-GPU: frames are independent units, sharded round-robin (global frame g -> rank g % N, exactly the
reference's thread sharding, src/system/parallel.rs:424-448); no data-path collective; one final gather of the
per-frame RMSDs over RCCL (torch.distributed, backend nccl) inside the timed region.  Scaling is weak: each rank
processes `--frames-per-step` frames per step.

Prints ONE JSON line on rank 0.  `roofline` is for the dominant kernel, measured with HIP events on the
library's own stream during the timed region (gr_profile_*).  A plain run does only that: set-up, warm-up, the timed steps,
--dump-outputs if asked, the line.  `--full` adds the measurements that take runs of their own: `cpu_baseline` times the CPU
oracle's restatement of the reference path (oracle/, kind "port") on a bounded sample of the same frames, rank 0 at N=1 only --
in a fresh CHILD process that never touches the GPU (`bench.py --cpu-baseline-child`), so nothing on the CPU side can take the
GPU number down with it; nproc, CPU model and both thread counts (all visible cores, and 16 = one GPU's share of the node) are
reported as BASELINE.md section 3 promises; and `roofline.copy_floor_live`, the arithmetic-free probe of the same launch shape.

--dump-outputs DIR writes what the last timed step returned, for comparing two builds on the same (seeded) inputs:
rmsd.npy (float32, the step's per-frame RMSDs, global frame order), status.npy (rank 0's per-frame status codes as float32) and
fitted_positions.npy (float32, frames x atoms x 3: the fitted coordinates of a fixed seeded sample of rank 0's frames of the
step, every atom while 4 frames fit in 48 MB, else a fixed seeded sample of atoms as well).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)
SEED = 20260424


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--warmup-seconds", type=float, default=1.5, help="the warm-up lasts at least this long: after the --warmup steps "
                    "their slots are fitted again (results discarded) until the device has run this long")
    ap.add_argument("--box-per-frame", action="store_true", help="a slightly different box in every frame (a constant-pressure trajectory): "
                    "the kernels read the box per frame instead of once per launch; NOT the headline configuration")
    ap.add_argument("--atoms", type=int, default=1_000_000)
    ap.add_argument("--frames-per-step", type=int, default=0, help="0 = the largest multiple of 256 (<= 1024) for which every frame "
                    "of warmup + timed steps is a distinct buffer inside --max-pool-gb")
    ap.add_argument("--max-pool-gb", type=float, default=240.0, help="HBM for the frame pool (288 GB per MI355X)")
    ap.add_argument("--cpu-frames-per-thread", type=int, default=32, help="frames of the CPU sample per thread (32 x 16 threads = 512 frames: ~6 s of CPU work per figure)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the CPU baseline's main figure (0 = all host cores visible "
                    "to this process); a second figure at 16 threads (one GPU's share of the node) is always reported")
    ap.add_argument("--cpu-max-frames", type=int, default=512, help="upper bound on the CPU sample (frames; 12 MB each in /dev/shm)")
    ap.add_argument("--full", action="store_true", help="also the measurements beside the headline that take runs of their own: the CPU "
                    "baseline and the live copy-floor probe (a plain run does only the headline)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="under --full: no CPU baseline")
    ap.add_argument("--no-live-floor", action="store_true", help="under --full: do not run the arithmetic-free copy probe (tools/bin/copy_matrix3) beside the "
                    "result; implied under a profiler (ROCPROF* / ROCP_* variables or an LD_PRELOAD are inherited by the child)")
    ap.add_argument("--tune", action="append", default=[], metavar="KEY=VALUE", help="gr_ctx_set_tuning (sub_batch, chunks, fit_wgs, fuse, "
                    "two_pass): launch-geometry sweeps; the defaults are the measured optimum")
    ap.add_argument("--gather", choices=["torch", "abi"], default="torch", help="final gather of the per-frame RMSDs at N > 1: torch.distributed "
                    "all_gather (backend nccl = RCCL; the launch contract's own channel) or the library's C-ABI communicator (gr_comm_*: "
                    "ncclCommInitRank + ncclAllGather; the unique id travels through torch.distributed)")
    ap.add_argument("--dump-rmsd", default=None, metavar="PATH", help="rank 0 writes the per-frame RMSDs of the timed steps, in GLOBAL frame "
                    "order (after the gather at N > 1), as a .npy file: what tests/test_gpu_multirank.py compares between rank counts")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="rank 0 writes what the last timed step returned as DIR/<name>.npy "
                    "(rmsd, status, fitted_positions: see the module docstring), at most 64 MB in all")
    ap.add_argument("--cpu-baseline-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--with-torch", action="store_true", help="import torch first even at N=1 (coexistence check)")
    args = ap.parse_args()
    if args.cpu_baseline_child:
        return cpu_baseline_child(args.cpu_baseline_child)

    # --gpus N means N ranks.  Under a launcher (WORLD_SIZE set) the two must agree; without one, `python bench.py --gpus N` starts the
    # N ranks itself -- fresh child processes of python -m torch.distributed.run, started BEFORE this process makes any GPU call -- and
    # only relays rank 0's line and the launcher's return code.
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args.gpus)
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE=%s: the rank count is the launcher's; run\n  python -m torch.distributed.run --nnodes=1 "
              "--nproc-per-node %d --master-addr 127.0.0.1 --master-port P bench.py --gpus %d ...\nor plain `python bench.py --gpus %d` "
              "(which starts the ranks itself)" % (args.gpus, os.environ.get("WORLD_SIZE"), args.gpus, args.gpus, args.gpus), file=sys.stderr)
        return 2

    # stdout carries exactly ONE JSON line: everything else any library prints there (RCCL prints a version banner on
    # init) is sent to stderr by pointing fd 1 at fd 2 until the result is written to the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    torch = None
    backend = os.environ.get("GROAN_DIST_BACKEND", "nccl")   # "gloo": CPU rehearsal of the multi-rank path (ranks may share a GPU)
    tdev = None
    if world > 1 or args.with_torch:
        # torch first: its bundled HIP runtime (SONAME libamdhip64.so.7) is then the one libgroan_hip.so binds to
        import torch
        for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29517"), ("RANK", "0"), ("WORLD_SIZE", "1")):
            os.environ.setdefault(k, v)   # plain `python bench.py --with-torch` (no launcher)
        ndev = max(torch.cuda.device_count(), 1)
        local_rank = local_rank % ndev
        if world > 1 or args.with_torch:
            import torch.distributed as dist
            if backend == "nccl":
                torch.cuda.set_device(local_rank)
                tdev = torch.device("cuda", local_rank)
                dist.init_process_group(backend="nccl", device_id=tdev)
            else:
                tdev = torch.device("cpu")
                dist.init_process_group(backend=backend)

    import numpy as np
    import groan_rs_amd as G

    from groan_rs_amd import workload as WL
    abi_comm = None
    if dist is not None and world > 1 and args.gather == "abi":
        ids = [G.Comm.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0)
        abi_comm = G.Comm(local_rank, rank, world, ids[0])

    G._lib.load()
    n = args.atoms
    K, W = args.steps, args.warmup
    frame_bytes = ((n + 255) // 256 * 256) * 12
    max_frames = int(args.max_pool_gb * 1e9 // frame_bytes)
    B = args.frames_per_step
    if B <= 0:
        # every frame of the run distinct: B <= max_frames / (K + W), in whole 256-frame launch groups where possible
        B = min(1024, max(1, max_frames // max(K + W, 1)))
        B = B // 256 * 256 if B >= 256 else (B // 64 * 64 if B >= 64 else B)
        B = max(B, 1)
    want = (K + W) * B
    pool = max(B, min(want, max_frames // B * B))
    reused = max(0, want - pool)      # frames of the run that are a second visit to a buffer (already fitted): 0 by construction
    # rhombic dodecahedron, SimBox::from_lengths_angles([d,d,d],[60,60,90]) (simbox.rs:96-123, :300-314)
    box = WL.c4_box(24.18)
    radius = WL.blob_radius(box)
    masses = WL.masses_cycle(n)

    trace_on = bool(os.environ.get("GROAN_BENCH_TRACE"))

    def trace(what):                          # GROAN_BENCH_TRACE=1: progress lines on stderr (where does a run under a profiler stop?)
        if trace_on:
            print("[bench %.3f] rank %d: %s" % (time.time() % 1000.0, rank, what), file=sys.stderr, flush=True)

    dev = local_rank
    trace("creating the system: %d atoms, %d slots" % (n, pool + 1))
    cur = G.System(n, masses=masses, n_slots=pool + 1, device=dev)      # slot `pool` holds the reference blob
    if args.tune:
        cur.set_tuning(**{kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.tune})
    cur.synth_reference(pool, box, radius, SEED)
    ref = G.System(n, masses=masses, n_slots=1, device=dev)
    ref.set_frame(cur.get_positions(pool), box)
    plan = G.RMSDPlan(ref, cur, "all")
    # local frame j of this rank is global frame j*world + rank
    t_gen = time.time()
    trace("synthesising %d frames" % pool)
    cur.synth_frames(pool, 0, pool, rank, 0.05, SEED, frame_index_stride=world)
    if args.box_per_frame:
        for f in range(pool):
            cur.set_box(WL.c4_box(24.18 * (1.0 + 2.0e-4 * ((f * 7) % 11 - 5))), slot=f)
    cur.sync()
    trace("frames ready")
    t_gen = time.time() - t_gen

    def barrier():
        cur.sync()
        if dist is not None:
            dist.barrier()
        if torch is not None and torch.cuda.is_available():
            torch.cuda.synchronize()

    rmsd_all = np.zeros((K, B), np.float32)
    step_ms = []
    step_slot = lambda s: ((s * B) % pool)
    # ---- warmup (untimed); profiling already on so the first use of the profiling events is not timed
    cur.profile_enable(True)
    t_warm = time.perf_counter()
    for s in range(W):
        trace("warmup step %d" % s)
        r, st = plan.rmsd_fit(step_slot(s), B)
        assert (st == 0).all(), st
    # W launches of a few milliseconds do not bring the device to its steady clocks (round 3: the driver's first four timed steps
    # were 2-11 % slow): the warm-up goes on, on the WARM-UP steps' own slots (already fitted, never timed; results discarded),
    # until --warmup-seconds of wall time have passed since it began.  The timed steps still see only fresh frames.
    warm_extra = 0
    while W > 0 and time.perf_counter() - t_warm < args.warmup_seconds:
        r, st = plan.rmsd_fit(step_slot(warm_extra % W), B)
        assert (st == 0).all(), st
        warm_extra += 1
    t_warm = time.perf_counter() - t_warm
    fallbacks = 0
    barrier()
    cur.profile_enable(True)
    cur.timer_start()
    t0 = time.perf_counter()
    t_prev = t0
    for s in range(K):
        trace("step %d" % s)
        r, st = plan.rmsd_fit(step_slot(W + s), B)       # synchronous: returns with the step's results on the host
        rmsd_all[s] = r
        fallbacks += plan.last_fallbacks()
        t_now = time.perf_counter(); step_ms.append(round(1e3 * (t_now - t_prev), 4)); t_prev = t_now
    gathered = None
    if dist is not None:
        # final gather of the per-frame RMSDs (K*B floats per rank) over RCCL, restored to global frame order
        if abi_comm is not None:
            gathered = abi_comm.gather_per_frame(rmsd_all.reshape(-1), K * B * world)
        else:
            gathered = G.gather_per_frame(rmsd_all.reshape(-1), K * B * world, dist=dist, device=tdev)
    gpu_ms = cur.timer_stop()
    trace("timed steps done")
    barrier()
    t1 = time.perf_counter()
    prof = cur.profile_read()
    cur.profile_enable(False)
    elapsed = t1 - t0
    per_rank_fps = [K * B / elapsed]
    if dist is not None:
        mine = torch.tensor([elapsed], dtype=torch.float64, device=tdev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)                     # per-rank times: a straggler shows in per_rank_frames_per_s
        per_rank_fps = [K * B / float(t.item()) for t in every]
        elapsed = max(float(t.item()) for t in every)    # MAX over ranks
    assert np.isfinite(rmsd_all).all()
    if gathered is not None:
        # every rank's frames arrived, in global frame order: frame g sits at g, and this rank's own are where they belong
        assert gathered.shape[0] == world * K * B, (gathered.shape, world, K, B)
        assert np.array_equal(gathered[rank::world], rmsd_all.reshape(-1)) and np.isfinite(gathered).all()
    total_frames = K * B * world
    value = total_frames / elapsed
    if rank == 0 and args.dump_outputs:
        # before anything else touches the frame slots (the CPU baseline regenerates and refits the first ones)
        dump_outputs(args.dump_outputs, rmsd_all[-1] if gathered is None else gathered[(K - 1) * B * world:], st, cur, step_slot(W + K - 1), B, n)

    # ---- roofline of the dominant kernel (HIP events on the library's stream, timed region)
    # `achieved` counts the bytes the kernel HAS TO MOVE through HBM per launch, every array once:
    #   k_sums_pk 28 B/atom/frame (cur 12 + ref 12 + mass 4), k_fit_pk 24 B/atom/frame (12 read + 12 written);
    #   k_fit_resident -- the whole RMSD-fit of a frame in ONE pass, reference rows and masses held in registers for the whole launch --
    #   24 B/atom/frame (12 read + 12 written) + 16 B/atom ONCE per launch.  That is what the PMC counters measure (`traffic`).
    # SURVEY 8d prices the RMSD-fit at 40 B/atom/frame (it counts the reference and the masses once per FRAME): that figure is kept
    # as `survey_8d_equivalent_GBs` -- a throughput in the contract's unit, NOT a bandwidth: it is never divided by the HBM peak.
    fpl = {k: (prof[k][2] / max(prof[k][1], 1) if k in prof else 0.0) for k in ("k_sums_pk", "k_fit_pk", "k_fit_resident")}
    alg_bytes = {"k_sums_pk": 28.0 * n * fpl["k_sums_pk"], "k_fit_pk": 24.0 * n * fpl["k_fit_pk"], "k_fit_resident": 24.0 * n * fpl["k_fit_resident"] + 16.0 * n}
    dom = max(("k_sums_pk", "k_fit_pk", "k_fit_resident"), key=lambda k: prof[k][0] if k in prof else -1.0)
    ms_total, launches, frames = prof[dom]
    avg_ms = ms_total / max(launches, 1)
    bytes_per_launch = alg_bytes[dom]
    achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    # HBM bytes per launch from the committed rocprofv3 PMC passes of this same command (separate --pmc runs,
    # FETCH_SIZE x2 gfx950 correction + WRITE_SIZE; profiles/*_pmc_summary.json) -- only when the launch shape matches
    traffic, traffic_src = None, None
    try:
        import glob
        for pf in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")), reverse=True):
            pj = json.load(open(pf))
            if pj.get("n_atoms") == n and pj.get("frames_per_launch") == frames / max(launches, 1):
                key = [k for k in pj["traffic"] if k.startswith(dom)]
                if key:
                    traffic = pj["traffic"][key[0]]["hbm_bytes_per_launch"]; traffic_src = os.path.basename(pf)
                    break
    except Exception:
        pass
    # the arithmetic-free floor of the same traffic at the same launch shape (tools/ceiling_bench.hip, committed per round)
    copy_floor_us, copy_floor_src = None, None
    try:
        import glob
        for pf in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_ceiling.json")), reverse=True):
            cj = json.load(open(pf))
            if cj.get("n_atoms") != n:
                continue
            want_k = "resident copy" if dom == "k_fit_resident" else ("copy+pw" if dom == "k_fit_pk" else "read+pw")
            cand = [r["us_per_frame"] for r in cj["results"] if r["kernel"].startswith(want_k) and "us_per_frame" in r]
            if cand:
                copy_floor_us, copy_floor_src = min(cand), os.path.basename(pf)
                break
    except Exception:
        pass
    # ... and the arithmetic-free PROBE of the same shape measured NOW, on this box, by a child process beside the (idle) frame pool:
    # the walk of the resident pass's address stream (tools/copy_matrix3.hip --quick, warmed up, as many frames per launch as this
    # run's launches; built by __graft_entry__.build()): free-running (4.3-4.65 us per 1e6-atom frame from box to box) and with its row
    # requests swept in address order by the metronome (3.7: round 5's finding, profiles/r05_copy_matrix.md).  Never fatal.
    copy_floor_live = None
    # only a profiler that is actually wrapped round this process (rocprofv3 preloads its tool library and names it in these variables)
    profiled = "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k in os.environ for k in ("ROCP_TOOL_LIBRARIES", "ROCPROF_OUTPUT_PATH", "ROCPROFILER_LIBRARY_CTOR"))
    if rank == 0 and dom == "k_fit_resident" and args.full and not args.no_live_floor and not profiled:
        try:
            exe = os.path.join(ROOT, "tools", "bin", "copy_matrix3")
            if os.path.isfile(exe):
                # the child sees exactly this rank's device: index `dev` of the list this process was given (itself possibly a restriction)
                vis = [v for v in os.environ.get("HIP_VISIBLE_DEVICES", "").split(",") if v != ""]
                child_dev = vis[dev] if dev < len(vis) else str(dev)
                cp = subprocess.run([exe, "--quick", str(n), str(int(frames / max(launches, 1)))], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120,
                                    env=dict(os.environ, HIP_VISIBLE_DEVICES=child_dev))
                line = [ln for ln in cp.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
                if cp.returncode == 0 and line:
                    copy_floor_live = json.loads(line[-1])
        except Exception:
            copy_floor_live = None
    us_per_frame_dom = 1e3 * ms_total / max(frames, 1)
    moved = traffic if traffic is not None else bytes_per_launch
    roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
                "hbm_moved_GBs": round(moved / (avg_ms * 1e-3) / 1e9, 1) if avg_ms > 0 else 0.0,
                "frac_hbm_moved": round(moved / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if avg_ms > 0 else 0.0,
                "hbm_moved_source": "PMC (%s)" % traffic_src if traffic is not None else "bytes that have to move (no PMC pass of this launch shape is committed)",
                "copy_floor_us_per_frame": copy_floor_us, "copy_floor_source": copy_floor_src,
                "frac_of_copy_floor": round(copy_floor_us / us_per_frame_dom, 4) if copy_floor_us and us_per_frame_dom > 0 else None,
                "copy_floor_live": copy_floor_live,
                "frac_of_copy_floor_live": (round(copy_floor_live["persistent_copy_us_per_frame_metronome"] / us_per_frame_dom, 4)
                                            if copy_floor_live and us_per_frame_dom > 0 else None),
                "copy_floor_live_note": "the walk of the pass's address stream without arithmetic, measured now on this box (tools/copy_matrix3.hip --quick): free-running, "
                                        "and with its requests in address order at the shortest metronome period it keeps; the fraction is the latter over the kernel's time",
                "us_per_frame": round(us_per_frame_dom, 4),
                "avg_launch_ms": round(avg_ms, 4), "launches": launches, "frames_per_launch": frames / max(launches, 1),
                "algorithmic_bytes_per_launch": bytes_per_launch,
                "algorithmic_bytes_note": "every array the launch has to move through HBM, once" + (": 24 B/atom/frame + 16 B/atom per launch (reference rows and masses stay in registers)" if dom == "k_fit_resident" else "")}
    kernels = {k: {"ms_total": round(v[0], 3), "launches": v[1], "us_per_frame": round(1e3 * v[0] / max(v[2], 1), 3)} for k, v in prof.items()}
    # whole step in the contract's unit: SURVEY 8d's 40 B/atom/frame whichever pass runs (a throughput, not a bandwidth)
    resident = prof.get("k_fit_resident", (0.0, 0, 0))[1] > 0
    path_gbs = 40.0 * n * (K * B) / (gpu_ms * 1e-3) / 1e9
    roofline["survey_8d_equivalent_GBs"] = round(40.0 * n * (frames / max(launches, 1)) / (avg_ms * 1e-3) / 1e9, 1) if dom == "k_fit_resident" and avg_ms > 0 else None

    out = {
        "metric": "frames/sec RMSD-fit, 1e6 atoms triclinic, 1/2/4/8 GPUs; HBM GB/s vs peak",
        "value": round(value, 1), "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": round(1e3 * elapsed / K, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32 (fp64 accumulators)", "data": "synthetic",
        "config": {"workload": "synthetic %d-atom rhombic-dodecahedral (triclinic) frames resident in HBM, Kabsch RMSD-fit of all atoms "
                               "(BASELINE configs[3] shard per GPU)" % n,
                   "n_atoms": n, "box_per_frame": bool(args.box_per_frame), "frames_per_step": B, "frames_per_gpu": K * B, "selection": "all atoms", "box9": [float(x) for x in box],
                   "pool_frames": pool, "reused_frames": reused, "parallelism": "frames round-robin over %d GPU(s), final RCCL gather (%s)" % (world, "gr_comm_gather_per_frame" if abi_comm is not None else "torch.distributed all_gather"),
                   "fallback_frames": fallbacks, "synth_seconds": round(t_gen, 2), "warmup_seconds": round(t_warm, 3), "warmup_extra_steps_on_warmup_slots": warm_extra, "step_ms": step_ms,
                   "per_rank_frames_per_s": [round(v, 1) for v in per_rank_fps]},
        "roofline": roofline,
        "kernels": kernels,
        "path": {"survey_8d_equivalent_GBs": round(path_gbs, 1), "survey_8d_bytes_per_frame": 40.0 * n, "gpu_ms_timed_region": round(gpu_ms, 3),
                 "timed_region_note": "the timed region is %.2f s of GPU work (%d steps); per-step times in config.step_ms" % (gpu_ms * 1e-3, K),
                 "hbm_bytes_per_frame_moved": (24.0 * n if resident else 36.0 * n),
                 "hbm_moved_GBs": round((24.0 if resident else 36.0) * n * (K * B) / (gpu_ms * 1e-3) / 1e9, 1),
                 "frac_hbm_moved": round((24.0 if resident else 36.0) * n * (K * B) / (gpu_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                 "pass": "resident (one pass over HBM: 24 B/atom/frame move)" if resident else "two-pass (sums, fit: 36 B/atom/frame move + 16 B/atom/frame from L2 / Infinity Cache)"},
    }

    # ---- CPU baseline: the oracle's restatement of the reference path on a bounded sample of the SAME frames (rank 0, N=1 only),
    # timed in a child process that never touches the GPU; a failure there is reported, never fatal for the GPU number
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        tmpdir = None
        try:
            t_main = args.cpu_threads or usable_cores()
            nf = min(max(t_main, 16) * args.cpu_frames_per_thread, args.cpu_max_frames, pool)
            # fresh frames: regenerate the first nf frames (the timed region fitted them in place), copy them out, then run
            # the GPU on them for the parity figures
            cur.synth_frames(pool, 0, nf, rank, 0.05, SEED, frame_index_stride=world)
            tmpdir = tempfile.mkdtemp(prefix="groan_cpu_baseline_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
            sample = np.lib.format.open_memmap(os.path.join(tmpdir, "frames.npy"), mode="w+", dtype=np.float32, shape=(nf, n, 3))
            for f in range(nf):
                sample[f] = cur.get_positions(f)
            sample.flush(); del sample
            np.save(os.path.join(tmpdir, "ref.npy"), ref.get_positions(0))
            np.save(os.path.join(tmpdir, "masses.npy"), masses)
            np.save(os.path.join(tmpdir, "box.npy"), box)
            gpu_r, gpu_st = plan.rmsd_fit(0, nf)
            np.save(os.path.join(tmpdir, "gpu_rmsd.npy"), gpu_r)
            np.save(os.path.join(tmpdir, "gpu_fit0.npy"), cur.get_positions(0))
            with open(os.path.join(tmpdir, "job.json"), "w") as fh:
                json.dump({"threads_main": t_main, "frames_per_thread": args.cpu_frames_per_thread, "gpu_value": value}, fh)
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", tmpdir],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            line = [ln for ln in child.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
            if child.returncode != 0 or not line:
                raise RuntimeError("child rc=%d: %s" % (child.returncode, child.stderr.decode(errors="replace")[-400:]))
            out["cpu_baseline"] = json.loads(line[-1])
        except Exception as e:
            out["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
        finally:
            if tmpdir:
                import shutil
                shutil.rmtree(tmpdir, ignore_errors=True)
    # what the resident pass did on every rank (ranks that share a device take turns on it or fall back to the two passes: gr_resident.h)
    res_stats = {}
    for k in ("res_launches", "res_handshake_misses", "res_aborts", "res_redone_frames", "res_last_streams", "res_metro_period_ns", "res_last_turn_ns", "res_late_permille", "res_sclk_mhz"):
        try:
            res_stats[k] = cur.stat(k)
        except Exception:                         # (an older build of the library under GR_LIB_PATH: A/B runs)
            res_stats[k] = None
    every_stats = [res_stats]
    if dist is not None:
        try:                                      # (diagnostics only: never allowed to take the benchmark line down)
            gathered_stats = [None] * world
            dist.all_gather_object(gathered_stats, res_stats)
            every_stats = gathered_stats
        except Exception as e:
            every_stats = [res_stats, {"all_gather_object": repr(e)}]
    out["config"]["per_rank_resident"] = every_stats
    if rank == 0:
        if args.dump_rmsd:
            np.save(args.dump_rmsd, gathered if gathered is not None else rmsd_all.reshape(-1))
        if gathered is not None:
            out["config"]["gathered_frames"] = int(gathered.shape[0])      # == n_gpus * steps * frames_per_step (asserted above)
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    plan.close(); ref.close(); cur.close()
    if dist is not None:
        dist.destroy_process_group()


def dump_outputs(out_dir, rmsd, status, cur, first_slot, n_frames, n_atoms):
    """What the last timed step returned (see the module docstring).  The sample of frames and atoms depends on the arguments
    only, so two builds run with the same arguments write the same frames and atoms."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "rmsd.npy"), np.asarray(rmsd, np.float32))
    np.save(os.path.join(out_dir, "status.npy"), np.asarray(status, np.float32))
    rng = np.random.default_rng(SEED)
    k = min(n_frames, 4)
    frames = np.sort(rng.choice(n_frames, k, replace=False))
    m = min(n_atoms, (48 << 20) // (12 * k))
    atoms = np.sort(rng.choice(n_atoms, m, replace=False)) if m < n_atoms else slice(None)
    np.save(os.path.join(out_dir, "fitted_positions.npy"), np.stack([cur.get_positions(first_slot + int(f))[atoms] for f in frames]))


def launch_ranks(n_ranks):
    """`python bench.py --gpus N` without a launcher: start the N ranks as the driver would (one process per GPU, rendezvous on
    127.0.0.1) and relay rank 0's JSON line.  This process has made no GPU call and makes none: the ranks are children, not an exec."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    child = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    lines = [ln for ln in child.stdout.decode(errors="replace").splitlines() if ln.startswith("{") and '"metric"' in ln]
    for ln in lines[-1:]:
        sys.stdout.write(ln + "\n")
    sys.stdout.flush()
    if child.returncode != 0:
        return child.returncode
    return 0 if len(lines) == 1 else 3


def usable_cores():
    """host cores this process can actually run on: the affinity mask, capped by the cgroup CPU quota (a GPU box hands each
    GPU's job a share of the node: 256 hardware threads may be visible while the quota is 16 cores' worth of time)"""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(-(-int(quota) // int(period)))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and p > 0:
                n = max(1, min(n, -(-q // p)))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline_child(tmpdir):
    """The CPU leg (kind "port": oracle/groan_oracle.c, the restatement of the reference path pinned by its known answers).
    Runs in its own process, loads no GPU library.  Sample frames come from the parent through files in `tmpdir`."""
    import numpy as np
    import oracle_lib as O
    job = json.load(open(os.path.join(tmpdir, "job.json")))
    # BASELINE.md section 3 asks for -O3 -march=native: built HERE, on the host that runs it (the shipped liboracle.so is a
    # portable build, so that a test process can never die of an illegal instruction on a different CPU)
    build = "portable -O3 (oracle/liboracle.so)"
    try:
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "native"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
        O.use_library(os.path.join(ROOT, "oracle", "liboracle_native.so"))
        build = "-O3 -march=native, built on this host (oracle/liboracle_native.so)"
    except Exception:
        pass
    frames = np.load(os.path.join(tmpdir, "frames.npy"), mmap_mode="r")
    ref_pos, masses, box = (np.load(os.path.join(tmpdir, k + ".npy")) for k in ("ref", "masses", "box"))
    gpu_r, gpu_fit0 = np.load(os.path.join(tmpdir, "gpu_rmsd.npy")), np.load(os.path.join(tmpdir, "gpu_fit0.npy"))
    nf_all, fpt = frames.shape[0], int(job["frames_per_thread"])
    visible = len(os.sched_getaffinity(0))
    model = ""
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip(); break
    except OSError:
        pass
    cargo = subprocess.run("cargo --version", shell=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()

    def run(threads, layout, cap=None):
        nf = min(nf_all, max(threads * fpt, 1), cap or nf_all)
        buf = np.array(frames[:nf])                     # private copy: fitted in place
        sec, r = O.baseline_rmsd_fit(buf, ref_pos, masses, box, threads, layout)
        return nf / sec, nf, r, buf

    t_main = int(job["threads_main"])
    fps_main, nf_main, r_f, _ = run(t_main, 0)          # reference-faithful 232-byte AoS records, frames round-robin over threads
    fps_soa, _, _, _ = run(t_main, 1)
    fps_16, nf_16, _, _ = run(16, 0) if t_main != 16 else (fps_main, nf_main, None, None)
    fps_1, _, _, _ = run(1, 0, cap=8)                   # (one thread: 8 frames, ~1.3 s)
    # parity at full size: the reference's sequential f32 sums lose ~1e-2 nm over 1e6 terms, so the GPU (fp64 sums) is compared
    # with the same CPU restatement summing in double; the literal f32 figure is reported beside it
    O.set_accumulate_f64(True)
    chk = np.array(frames[:2])
    _, r_64 = O.baseline_rmsd_fit(chk, ref_pos, masses, box, 2, 1)
    O.set_accumulate_f64(False)
    # the headline CPU figure is the BETTER of the two thread counts (a container may expose 256 hardware threads and schedule
    # 16 cores' worth of them: oversubscribed threads then make "all cores" the slower configuration); both are reported
    best_fps, best_t, best_nf = (fps_main, t_main, nf_main) if fps_main >= fps_16 else (fps_16, 16, nf_16)
    out = {
        "value": round(best_fps, 2), "unit": "frames/s", "cores": best_t, "kind": "port",
        "sample": "%d of the benchmark's own frames (%d per thread), reference-faithful 232-byte AoS layout, f32, frames round-robin over %d threads "
                  "(src/system/parallel.rs:424-448), decode excluded" % (best_nf, fpt, best_t),
        "value_all_cores": round(fps_main, 2), "threads_all_cores": t_main,
        "nproc": os.cpu_count(), "cores_visible": visible, "cores_usable_cgroup_quota": usable_cores(), "cpu_model": model, "build": build,
        "value_16_threads": round(fps_16, 2), "sample_16_threads": "%d frames" % nf_16,
        "soa_value": round(fps_soa, 2), "single_thread_value": None if fps_1 is None else round(fps_1, 3),
        "gpu_vs_cpu": round(float(job["gpu_value"]) / best_fps, 1),
        "rust_toolchain_on_this_host": cargo or "absent (cargo --version fails): the reference itself cannot be built here",
        "process": "child process without any GPU library",
        "parity_max_abs_rmsd_diff_vs_cpu_f64sums": float(np.abs(gpu_r[:2] - r_64).max()),
        "parity_max_abs_fit_diff_vs_cpu_f64sums_frame0": float(np.abs(gpu_fit0 - chk[0]).max()),
        "reference_f32_sum_error_rmsd": float(np.abs(r_f[:2] - r_64).max()),
    }
    sys.stdout.write(json.dumps(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

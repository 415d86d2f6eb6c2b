#!/usr/bin/env python3
"""One steady-state step of bench.py out of a `rocprofv3 --hip-trace --kernel-trace --output-format csv` run: what the device and the host
do between two resident launches (profiles/resident_call_path.md).  Usage: call_path_trace.py DIR_WITH_THE_TWO_CSVS [STEPS=20]

A step = from the end of one k_fit_resident to the end of the next; the last STEPS steps of the run are the timed ones.  Printed per
step, median over the steps, in us: every kernel in the window with its duration and the idle gap in front of it, every HIP API call
of the host thread in the window with count and time inside, and the host time between the return of the call's last wait
(hipStreamSynchronize, or the last API call before the gap in which the host polls) and the next launch."""
import csv, glob, os, sys
from collections import OrderedDict
from statistics import median

d = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
kfile = glob.glob(os.path.join(d, "*kernel_trace.csv"))[0]
afile = glob.glob(os.path.join(d, "*hip_api_trace.csv"))[0]
kern = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].split("<")[0].replace("void ", "")) for r in csv.DictReader(open(kfile))))
api = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"]) for r in csv.DictReader(open(afile)) if r["Domain"].startswith("HIP_RUNTIME_API")))
fits = [k for k in kern if k[2].startswith("k_fit_resident")]
fits = fits[-(steps + 1):]
dev_rows, api_rows, host_gap, step_us, fit_us, dev_idle = OrderedDict(), OrderedDict(), [], [], [], []
for prev, cur in zip(fits[:-1], fits[1:]):
    w0, w1 = prev[1], cur[1]
    step_us.append((w1 - w0) / 1e3); fit_us.append((cur[1] - cur[0]) / 1e3)
    t, seen, idle = w0, {}, 0.0
    for s, e, name in kern:
        if s < w0 or e > w1: continue
        k = seen.get(name, 0); seen[name] = k + 1
        key = name if k == 0 else "%s #%d" % (name, k + 1)
        dev_rows.setdefault(key, []).append(((s - t) / 1e3, (e - s) / 1e3))
        idle += (s - t) / 1e3; t = e
    dev_idle.append(idle)
    per = {}
    calls = [a for a in api if a[0] >= w0 and a[0] < w1]
    for s, e, name in calls:
        n, tot = per.get(name, (0, 0.0)); per[name] = (n + 1, tot + (e - s) / 1e3)
    for name, v in per.items(): api_rows.setdefault(name, []).append(v)
    # the host's way from "results are here" to the next launch: the largest hole between two API calls of the window is the wait
    # (a blocking call shows as a long call instead), what follows it up to hipLaunchKernel of the resident kernel is host work
    launches = [a for a in calls if a[2] == "hipLaunchKernel"]
    if launches:
        syncs = [a for a in calls if a[2] == "hipStreamSynchronize" and a[1] < launches[-1][0]]
        if syncs: host_gap.append((launches[-1][0] - syncs[-1][1]) / 1e3)
print("steps %d | step %.1f us | k_fit_resident %.1f us | rest of the step %.1f us | device idle inside the step %.1f us" %
      (len(step_us), median(step_us), median(fit_us), median(step_us) - median(fit_us), median(dev_idle)))
print("\ndevice (in order of appearance): kernel | idle before it | duration | in steps")
for name, v in dev_rows.items(): print("| %s | %.1f | %.1f | %d |" % (name, median(x[0] for x in v), median(x[1] for x in v), len(v)))
print("\nhost: HIP API | calls per step | us inside per step | in steps")
for name, v in sorted(api_rows.items(), key=lambda kv: -median(x[1] for x in kv[1])): print("| %s | %.0f | %.1f | %d |" % (name, median(x[0] for x in v), median(x[1] for x in v), len(v)))
if host_gap: print("\nhost, return of the last hipStreamSynchronize before the resident launch -> that hipLaunchKernel: %.1f us" % median(host_gap))

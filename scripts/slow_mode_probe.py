#!/usr/bin/env python3
"""What a slow pass of the headline command is (profiles/r10a_slow_mode.txt).

  python scripts/slow_mode_probe.py [--runs N] [--rows K] [--timeout S] [--json FILE]
      N fresh child processes, one after another, each under its own time limit; the first non-zero exit status ends the loop.
      A child repeats what `bench.py --gpus 1 --steps 20 --warmup 2` does -- the same scenario, a torch stream set on the handle, 2 warm-up
      steps, reset, 20 untimed steps, reset, 20 timed steps -- with the library's timeline on (er_tsdf_set_timeline) for all three phases,
      and prints one JSON line: the wall time of each phase and the timeline rows.  The parent prints per phase the rate, its class
      (slow below 150 k frames/s), and what the rows say: the medians of k_integrate, of the pre-pass chain and of its parts, the share
      of k_integrate's time during which a pre-pass chain of another batch was running, and how far the host ran ahead of the voxel
      stream; then the first K rows of the timed phase.
  python scripts/slow_mode_probe.py --child          one such process (also the program to put behind `rocprofv3 --kernel-trace ... --`)
  python scripts/slow_mode_probe.py --report FILE    the same tables from the JSON lines of children run by hand
  python scripts/slow_mode_probe.py --trace CSV      a rocprofv3 kernel trace of a child: per hardware-queue id the kernels that ran on it, and
                                                     the same overlap share from the kernels' own timestamps, over the last 60 batches
The environment is passed on as it is: GPU_MAX_HW_QUEUES (4 unless set; never above 32 here) and ER_HIP_LIB choose the case."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, W, I = 20, 2, 50
SLOW_BELOW = 150e3


def child():
    import torch
    from elasticreconstruction_amd import synth
    from elasticreconstruction_amd.tsdf import TSDFVolume
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    S = 150
    sc = synth.make_scenario(K * S, interval=I, warp=True, frame_offset=0, total_frames=K * S, revolutions=1.0, device=dev)
    depth, w = sc["depth"], synth.warp_arrays(sc)
    px = depth.shape[1]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_stream(stream)

    def steps(vol, k):
        for s in range(k):
            lo, hi = s * S, (s + 1) * S
            gi = w["grid_index"][lo:hi]
            g0, g1 = int(gi.min()), int(gi.max()) + 1
            vol.IntegrateFrames(None, sc["traj"][lo:hi], dict(ctr=w["ctr"][g0:g1], resolution=w["resolution"], length=w["length"], grid_index=gi - g0,
                                                              seg=w["seg"][lo:hi], madj=w["madj"][lo:hi]), device_ptr=depth.data_ptr() + lo * px * 2)

    vol = TSDFVolume(max_units=640, device=0)
    vol.set_stream(stream.cuda_stream)
    vol.set_timeline(True)
    out = {"queues": os.environ.get("GPU_MAX_HW_QUEUES", ""), "lib": os.path.basename(os.environ.get("ER_HIP_LIB", "in-tree")), "phases": []}
    for name, k, reset in (("warm-up", W, False), ("untimed", K, True), ("timed", K, True)):
        if reset:
            vol.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps(vol, k)
        if name == "untimed":
            vol.synchronize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["phases"].append({"name": name, "frames": k * S, "seconds": dt, "rows": vol.get_timeline()})
    vol.set_timeline(False)
    assert vol.unit_count() > 0
    vol.close()
    print(json.dumps(out))


def union_overlap(lo, hi, spans):
    """Length of [lo, hi] covered by the union of spans."""
    cov, at = 0.0, lo
    for a, b in sorted(spans):
        a, b = max(a, at), min(b, hi)
        if b > a:
            cov += b - a
            at = b
    return cov


def med(x):
    x = sorted(x)
    return x[len(x) // 2] if x else float("nan")


def summarise(ph):
    r = ph["rows"]
    fps = ph["frames"] / ph["seconds"]
    integ = [(x["v_begin"], x["v_end"]) for x in r]
    chain = [(x["x_consts"], x["x_plan"]) for x in r]
    busy = sum(b - a for a, b in integ)
    beside = sum(union_overlap(a, b, [c for j, c in enumerate(chain) if j != i]) for i, (a, b) in enumerate(integ))
    us = lambda f: 1e3 * med([f(x) for x in r])
    return ("%-8s %4d frames %8.2f ms %8.0f frames/s %-4s | k_integrate %5.0f us  period %5.0f us  chain %5.0f (scatter+fix %4.0f, k_prepare %4.0f) us"
            "  beside a chain %.2f  host ahead of V %6.0f us  wait for constants %4.0f us"
            % (ph["name"], ph["frames"], 1e3 * ph["seconds"], fps, "SLOW" if fps < SLOW_BELOW else "fast", us(lambda x: x["v_end"] - x["v_begin"]),
               1e3 * med([b["v_begin"] - a["v_begin"] for a, b in zip(r, r[1:])]), us(lambda x: x["x_plan"] - x["x_consts"]),
               us(lambda x: x["x_fix"] - x["x_consts"]), us(lambda x: x["x_prepare"] - x["x_fix"]), beside / busy if busy else 0.0,
               us(lambda x: x["v_begin"] - x["host_out"]), us(lambda x: x["host_consts"] - x["host_in"])))


def rows_table(rows, k):
    cols = ("host_in", "host_out", "x_wait", "x_consts", "x_fix", "x_prepare", "x_plan", "v_begin", "v_end")
    t0 = rows[0]["host_in"]
    print("  batch slot X " + " ".join("%9s" % c for c in cols) + "   (us since the first row's entry)")
    for x in rows[:k]:
        print("  %5d %4d %1d " % (x["batch"], x["slot"], x["stream"]) + " ".join("%9.0f" % (1e3 * (x[c] - t0)) for c in cols))


def trace(path):
    ks = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(anonymous namespace)::")[-1].replace("void ", "").split("(")[0].split("<")[0].split("::")[-1]
        ks.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r.get("Queue_Id", "?")))
    ks.sort()
    ints = [k for k in ks if k[2] == "k_integrate"][-3 * K:]
    lo = ints[0][0]
    win = [k for k in ks if k[0] >= lo - 1000000]
    byq = {}
    for s, e, name, q in win:
        byq.setdefault(q, {}).setdefault(name, 0)
        byq[q][name] += 1
    for q in sorted(byq):
        print("  hardware queue %-3s %s" % (q, ", ".join("%s x %d" % kv for kv in sorted(byq[q].items()))))
    pre = [(s, e) for s, e, name, q in win if name in ("k_reproject_scatter", "k_reproject_fix", "k_prepare", "k_plan")]
    busy = sum(e - s for s, e, _, _ in ints)
    print("  last %d k_integrate: median %.0f us, period %.0f us, share of their time beside a pre-pass kernel %.2f"
          % (len(ints), med([e - s for s, e, _, _ in ints]) / 1e3, med([b[0] - a[0] for a, b in zip(ints, ints[1:])]) / 1e3,
             sum(union_overlap(s, e, pre) for s, e, _, _ in ints) / busy))


def report(run, d, k):
    print("run %d  GPU_MAX_HW_QUEUES=%s  lib=%s" % (run, d["queues"] or "(unset)", d["lib"]))
    for ph in d["phases"]:
        print("  " + summarise(ph))
    rows_table(d["phases"][-1]["rows"], k)
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--report", help="print the tables of the JSON lines in this file (children run by hand, under a profiler for instance)")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--rows", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--json", help="append every child's JSON line to this file")
    a = ap.parse_args()
    if a.child:
        return child()
    if a.trace:
        return trace(a.trace)
    if a.report:
        for run, line in enumerate(l for l in open(a.report) if l.startswith("{")):
            report(run, json.loads(line), a.rows)
        return
    if int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) > 32:
        raise SystemExit("GPU_MAX_HW_QUEUES above 32")
    for run in range(a.runs):
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child"], stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise SystemExit("run %d: exit status %d -- stopping" % (run, p.returncode))
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        if a.json:
            open(a.json, "a").write(line + "\n")
        report(run, json.loads(line), a.rows)


if __name__ == "__main__":
    main()

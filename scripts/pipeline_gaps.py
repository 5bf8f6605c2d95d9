"""Where the batch pipeline of path A waits, from a rocprofv3 kernel-trace CSV of bench.py (scripts/gpu_timeline.sh):
python scripts/pipeline_gaps.py <kernel_trace.csv> [skip_batches]
Per pre-pass queue: the idle time between a k_plan and the next kernel of the queue, the wait between the warp's scatter chain and
k_prepare (where the wait for the pipeline slot stands when the scatter runs ahead) and the length of a chain from its first kernel to
its k_plan; on the voxel queue: the idle time between k_integrate launches and the period.  Medians and means over the steady state
(the first skip_batches k_integrate launches, default 70, are warm-up)."""
import csv
import statistics
import sys


def short(name):
    if "(anonymous namespace)::" in name:
        name = name.split("(anonymous namespace)::", 1)[1]
    return name.replace("void ", "").split("(")[0].split("<")[0].split("::")[-1]


def stat(xs):
    if not xs:
        return "n=0"
    xs = sorted(xs)
    return "n=%4d  median %7.1f  mean %7.1f  p10 %7.1f  p90 %7.1f us" % (len(xs), statistics.median(xs), statistics.fmean(xs), xs[len(xs) // 10], xs[(9 * len(xs)) // 10])


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 70
    ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Queue_Id", "?")) for r in rows)
    ks = [k for k in ks if k[2].startswith("k_")]
    ints = [k for k in ks if k[2] == "k_integrate"]
    skip = min(skip, len(ints) // 3)
    t0 = ints[skip][0]
    ks = [k for k in ks if k[0] >= t0]
    ints = ints[skip:]
    print("k_integrate: %d launches after the warm-up" % len(ints))
    print("  duration                     %s" % stat([(e - s) / 1e3 for s, e, _, _ in ints]))
    print("  idle before the next launch  %s" % stat([(b[0] - a[1]) / 1e3 for a, b in zip(ints, ints[1:]) if b[0] - a[1] < 5e6]))
    print("  period (start to start)      %s" % stat([(b[0] - a[0]) / 1e3 for a, b in zip(ints, ints[1:]) if b[0] - a[0] < 5e6]))
    for name in ("k_reproject_scatter", "k_prepare", "k_reset", "k_reproject_fix", "k_plan"):
        print("%-22s duration %s" % (name, stat([(e - s) / 1e3 for s, e, n, _ in ks if n == name])))
    pre = {"k_reset", "k_reproject_scatter", "k_reproject_fix", "k_prepare", "k_plan"}
    for q in sorted({k[3] for k in ks if k[2] in pre}):
        mine = [k for k in ks if k[3] == q and k[2] in pre]
        if not any(k[2] == "k_plan" for k in mine):
            continue
        idle, slot, chain, first = [], [], [], None
        for a, b in zip(mine, mine[1:]):
            if first is None:
                first = a[0]
            if a[2] == "k_plan":
                chain.append((a[1] - first) / 1e3)
                first = None
                if b[0] - a[1] < 5e6:
                    idle.append((b[0] - a[1]) / 1e3)
            if a[2] == "k_reproject_fix" and b[0] - a[1] < 5e6:
                slot.append((b[0] - a[1]) / 1e3)
        print("pre-pass queue %s" % q)
        print("  k_plan -> next kernel        %s" % stat(idle))
        print("  k_reproject_fix -> next      %s" % stat(slot))
        print("  chain, first kernel -> k_plan %s" % stat(chain))


if __name__ == "__main__":
    main()

"""A rocprofv3 kernel-trace CSV cut down to what scripts/timeline.py and scripts/pipeline_gaps.py read -- the k_* kernels, short names,
queue, start and end -- and to the last `batches` k_integrate launches:  python scripts/trim_trace.py <in.csv> <out.csv> [batches]"""
import csv
import sys


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    keep = ["Kernel_Name", "Queue_Id", "Start_Timestamp", "End_Timestamp"]
    out = []
    for r in rows:
        n = r["Kernel_Name"].replace("void ", "").split("(anonymous namespace)::")[-1].split("(")[0].split("<")[0].split("::")[-1]
        if n.startswith("k_"):
            out.append({"Kernel_Name": n, "Queue_Id": r.get("Queue_Id", "?"), "Start_Timestamp": r["Start_Timestamp"], "End_Timestamp": r["End_Timestamp"]})
    out.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(sys.argv) > 3:
        ints = [i for i, r in enumerate(out) if r["Kernel_Name"] == "k_integrate"]
        if len(ints) > int(sys.argv[3]):
            out = out[ints[-int(sys.argv[3])]:]
    w = csv.DictWriter(open(sys.argv[2], "w", newline=""), keep)
    w.writeheader()
    w.writerows(out)


if __name__ == "__main__":
    main()

"""Mean timeline of one soccer step from a rocprofv3 --kernel-trace CSV.

    python tools/kernel_timeline.py <dir with *kernel_trace.csv> [envs] [steps]

Launches of one kernel are told apart by hardware queue and grid (the live row builder has one
workgroup per env; the tail finisher's second tier has more workgroups than its first). A step
runs from one live k_soccer_rows start to the next; the last `steps` whole steps are averaged.
Prints, per launch, its mean start and end (ms from the step's start) and duration, and the step
period.
"""
import csv
import glob
import os
import sys

NAMES = ("k_soccer_rows", "k_pgs_groups", "k_soccer_bank_finish", "k_soccer_finish", "k_soccer_settle")


def main(d, envs=4096, steps=50):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = []
    for r in csv.DictReader(open(f)):
        name = next((n for n in NAMES if n + "<" in r["Kernel_Name"] or r["Kernel_Name"].endswith(n)), None)
        if not name:
            continue
        gk = "Grid_Size_X" if "Grid_Size_X" in r else "Grid_Size"
        wk = "Workgroup_Size_X" if "Workgroup_Size_X" in r else "Workgroup_Size"
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r.get("Queue_Id", "?"),
                     int(r[gk]) // max(1, int(r[wk]))))
    rows.sort()
    anchors = [i for i, x in enumerate(rows) if x[2] == "k_soccer_rows" and x[4] == envs]
    anchors = anchors[-(steps + 1):]
    acc, n = {}, len(anchors) - 1
    for a, b in zip(anchors, anchors[1:]):
        t0 = rows[a][0]
        for s, e, name, q, grid in rows[a:b]:
            k = (name, q, grid)
            v = acc.setdefault(k, [0, 0.0, 0.0, 0.0])
            v[0] += 1
            v[1] += (s - t0) / 1e6
            v[2] += (e - t0) / 1e6
            v[3] += (e - s) / 1e6
    print(f"{os.path.basename(f)}: {n} steps, step period {(rows[anchors[-1]][0] - rows[anchors[0]][0]) / 1e6 / n:.4f} ms")
    print(f"{'kernel':22s} {'queue':>5s} {'blocks':>6s} {'calls':>5s} {'start':>8s} {'end':>8s} {'dur ms':>8s}")
    for k, v in sorted(acc.items(), key=lambda kv: kv[1][1] / kv[1][0]):
        c = v[0]
        print(f"{k[0]:22s} {k[1]:>5s} {k[2]:6d} {c:5d} {v[1] / c:8.4f} {v[2] / c:8.4f} {v[3] / c:8.4f}")


if __name__ == "__main__":
    main(sys.argv[1], *(int(x) for x in sys.argv[2:4]))

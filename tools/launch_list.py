#!/usr/bin/env python3
"""launch_list.py [--collapse] DIR [DIR ...] — the kernel launches of one profiled run as text, for a diff of two builds (profiles/api_split.md).

DIR holds what `rocprofv3 --kernel-trace --output-format csv -d DIR -- <driver>` wrote (one *_kernel_trace.csv per process).  Prints, per
process in the order the processes started and per queue in the order the queues were first used, every dispatch in dispatch order as
`kernel name | grid | workgroup | LDS bytes`; process and queue ids are replaced by their rank, so that two runs of the same driver with two
builds of the library give the same text exactly when they launch the same kernels in the same order with the same geometry.
--collapse: for a driver that repeats its step for a time and not for a count (bench.py's timed regions): a block of up to 64 launches that
repeats the block in front of it is dropped, so the text holds every distinct step once, in order, whatever the number of steps was."""
import csv
import glob
import os
import sys


def runs(d):
    out = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows = list(csv.DictReader(open(path)))
        if rows:
            rows.sort(key=lambda r: int(r["Dispatch_Id"]))
            out.append((int(rows[0]["Start_Timestamp"]), rows))
    return [rows for _, rows in sorted(out, key=lambda t: t[0])]


def collapsed(lines):
    out = []
    for line in lines:
        out.append(line)
        again = True
        while again:
            again = False
            for p in range(1, min(64, len(out) // 2) + 1):
                if out[-p:] == out[-2 * p:-p]:
                    del out[-p:]
                    again = True
                    break
    return out


def main():
    total = 0
    collapse = "--collapse" in sys.argv
    for d in (a for a in sys.argv[1:] if a != "--collapse"):
        for p, rows in enumerate(runs(d)):
            lane = "Stream_Id" if "Stream_Id" in rows[0] and len({r["Stream_Id"] for r in rows}) > 1 else "Queue_Id"
            queues = {}
            for r in rows:
                queues.setdefault(r[lane], []).append(r)
            for q, (_, rs) in enumerate(queues.items()):
                lines = []
                for r in rs:
                    grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
                    wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
                    lines.append(f"{r['Kernel_Name']} | {grid} | {wg} | {r['LDS_Block_Size']}")
                if collapse:
                    lines = collapsed(lines)
                print(f"# {os.path.basename(os.path.normpath(d))} process {p} {lane.lower()} {q}: {len(lines)} launches" + (" once repeats are dropped" if collapse else ""))
                print("\n".join(lines))
                total += len(rs)
    print("# launches read" if collapse else f"# total {total} launches")


if __name__ == "__main__":
    main()

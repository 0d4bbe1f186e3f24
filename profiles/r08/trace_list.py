"""Ordered kernel names per queue from a rocprofv3 kernel trace: trace_list.py DIR REGIME -> lines 'REGIME qN name' on stdout.
Queues are numbered in the order of their first dispatch; within a queue the order is that of the dispatch ids."""
import csv
import glob
import os
import re
import sys

d, regime = sys.argv[1], sys.argv[2]
files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
assert len(files) == 1, files
rows = list(csv.DictReader(open(files[0], newline="")))
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
queues = {}
per_queue = {}
for r in rows:
    q = queues.setdefault(r["Queue_Id"], len(queues))
    name = re.sub(r"\s+", " ", r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]).strip() or r["Kernel_Name"]
    name = re.sub(r"^(void|int) ", "", name)
    per_queue.setdefault(q, []).append(name[:160])
for q in sorted(per_queue):
    for name in per_queue[q]:
        print(f"{regime} q{q} {name}")
print(f"{regime} total {len(rows)} kernels on {len(per_queue)} queue(s)")

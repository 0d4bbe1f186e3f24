"""The launches of a rocprofv3 kernel trace in a form short enough to keep: trace_list.py DIR REGIME -> on stdout, per queue,
'REGIME qN: COUNT kernels, sha256 DIGEST' where DIGEST is over the kernel names of the queue in dispatch order (one per line), then
per kernel name 'REGIME COUNT x name'.  Queues are numbered in the order of their first dispatch.  Two traces with the same lines
made the same launches in the same order on every queue; where they differ the counts say which kernel."""
import collections
import csv
import glob
import hashlib
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
    digest = hashlib.sha256("\n".join(per_queue[q]).encode()).hexdigest()
    print(f"{regime} q{q}: {len(per_queue[q])} kernels, sha256 {digest}")
counts = collections.Counter(n for names in per_queue.values() for n in names)
for name in sorted(counts):
    print(f"{regime} {counts[name]} x {name}")
print(f"{regime} total {len(rows)} kernels on {len(per_queue)} queue(s)")

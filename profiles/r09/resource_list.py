"""hipcc ... --cuda-device-only -Rpass-analysis=kernel-resource-usage -c FILE -o /dev/null 2>&1 | resource_list.py
-> one line per kernel, by name: registers, scratch, occupancy, LDS."""
import re
import sys

cur, out = None, {}
for line in sys.stdin:
    m = re.search(r"remark: +(.*?) \[-Rpass-analysis", line)
    if not m:
        continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        cur = re.search(r"\d+([a-z0-9_]+_kernel)", t).group(1)
        out[cur] = []
    elif cur:
        out[cur].append(t)
for k in sorted(out):
    print(k, "|", "; ".join(out[k]))

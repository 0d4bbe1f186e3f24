#!/usr/bin/env python3
"""Set-up and teardown cost of a subband stream: wall time of create + apv_stream_init + close, per cycle, over 20 cycles of the
evaluated stream tests/test_gpu_stream_lifecycle.py uses (block 32, hop 16, 4 x 4, ranks (1, 2), 64-tap responses: fast-convolution
K1; evaluation at 5 validation microphones through 9-tap responses).  One JSON line: median, fastest and slowest cycle in ms; the
first cycle (it loads the code objects and builds the FFT tables) is reported apart.  `--root DIR` measures another checkout's
package (its library built), for a comparison in one visit to one GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--cycles", type=int, default=20)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

from ap_vast_unofficial_amd._capi import Engine  # noqa: E402

N, H, L, M, P, PV, MV = 32, 16, 4, 4, 64, 9, 5
rng = np.random.default_rng(1)
rirA, rirB = rng.standard_normal((2, P, L, M)) * 1e-3
rvA, rvB = rng.standard_normal((2, PV, L, MV))


def cycle():
    t0 = time.perf_counter()
    eng = Engine(N // 2 + 1, L, M, ranks=(1, 2), compute_dtype="f64", block_size=N, hop_size=H, n_zones=3,
                 evaluation=(rvA, rvB, [1, 2]))
    eng.stream_init(rirA, rirB, 0, 1, 2)
    eng.close()
    return (time.perf_counter() - t0) * 1e3


first = cycle()
ms = sorted(cycle() for _ in range(args.cycles))
print(json.dumps({"root": os.path.abspath(args.root), "cycles": args.cycles, "first_ms": round(first, 3),
                  "median_ms": round(float(np.median(ms)), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}))

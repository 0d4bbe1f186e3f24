#!/usr/bin/env python3
"""Time of one fused order-16 launch (Engine.update_dev, float64, K = 32 768) at control-point counts that are no multiple of the
32-row chunk of stage 0 -- the ragged-M loop of correlate16 -- next to M = 32, by HIP events around 100 launches after 20 of warm-up.
Run it in a tree of the parent and in a tree of the change, each in a process of its own, and compare the lines.

    python tools/probes/ragged_m_timing.py [--M 24 40 32] [--ranks 8] [--dtype f64] [--lam] [--json FILE]

--ranks takes a rank list, so the same probe times a long list (--ranks 1 2 ... 16) against a single rank.
--lam gives the launch a buffer for the eigenvalues (the float64 kernel then refines all sixteen eigenvector columns)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ap_vast_unofficial_amd import Engine  # noqa: E402
import bench  # noqa: E402

K, L = 32 * 1024, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[24, 40, 32])
    ap.add_argument("--ranks", type=int, nargs="+", default=[8])
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--lam", action="store_true", help="launch with an eigenvalue buffer")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    rows = []
    for M in args.M:
        XB, XD, d = bench.synth(K, 1234, L, M)
        eng = Engine(K, L, M, ranks=tuple(args.ranks), compute_dtype=args.dtype, out_c128=False)
        bufs = [eng.to_device(a) for a in (XB, XD, d)]
        dw, ds = eng.alloc(K * len(args.ranks) * L * 8), eng.alloc(K * 4)
        dl = eng.alloc(K * L * np.dtype(eng.lam_dtype).itemsize) if args.lam else None
        for _ in range(20):
            eng.update_dev(bufs[0], bufs[1], bufs[2], dw, dl, ds)
        eng.sync()
        eng.timer_start()
        for _ in range(100):
            eng.update_dev(bufs[0], bufs[1], bufs[2], dw, dl, ds)
        ms = eng.timer_stop() / 100
        bad = int((ds.download((K,), np.int32) != 0).sum())
        rows.append(dict(M=M, ranks=list(args.ranks), lam=args.lam, dtype=args.dtype, ms_per_launch=ms, status_nonzero=bad))
        print(f"M = {M:3d}  ranks {tuple(args.ranks)}{' lam' if args.lam else ''}  {args.dtype}: {ms:.4f} ms per launch = {K / ms * 1e3:.3e} updates/s, "
              f"status != 0 in {bad} bins")
        for b in bufs + [dw, ds] + ([dl] if dl else []):
            b.free()
        eng.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Subband mode above 64 loudspeakers (csrc/kernels_gevd128.hip): one JSON line.

  kernel  Engine.update_dev alone: K = 2048 bins, L = M = 128, ranks (1, 8), float64; ms per launch and updates/s
  class   apvast(mode="subband", dtype="f64") at N = 2048, H = 1024, 48 kHz, M = 128 per zone, P = 256 taps, V = 8, both
          zones, L = 128 and L = 96: ms per process_input_buffers call and ms per hop of process_signal (64 hops)

A hop of 1024 samples at 48 kHz lasts 21.3 ms: the real-time budget of both class figures.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ap_vast_unofficial_amd import Engine  # noqa: E402
from ap_vast_unofficial_amd.apvast import apvast  # noqa: E402


def kernel(L=128, M=128, K=2048, ranks=(1, 8), launches=5):
    rng = np.random.default_rng(1234)

    def cn(*s):
        return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)

    eng = Engine(K, L, M, ranks=ranks, compute_dtype="f64", out_c128=False)
    dXB, dXD, dd = eng.to_device(cn(K, M, L)), eng.to_device(cn(K, M, L)), eng.to_device(cn(K, M))
    dw, ds = eng.alloc(K * len(ranks) * L * 8), eng.alloc(K * 4)
    for _ in range(2):
        eng.update_dev(dXB, dXD, dd, dw, None, ds)
    eng.sync()
    eng.timer_start()
    for _ in range(launches):
        eng.update_dev(dXB, dXD, dd, dw, None, ds)
    ms = eng.timer_stop() / launches
    st = ds.download((K,), np.int32)
    eng.close()
    return {"L": L, "M": M, "K": K, "ranks": list(ranks), "ms_per_launch": round(ms, 3),
            "updates_per_s": round(K / ms * 1e3, 1), "status_nonzero": int((st != 0).sum())}


def stream(L, M=128, N=2048, H=1024, P=256, V=8, hops=64, calls=16):
    rng = np.random.default_rng(7)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    rirA = rng.standard_normal((P, L, M)) * env * 1e-3
    rirB = rng.standard_normal((P, L, M)) * env * 1e-3
    mk = lambda: apvast(N, rirA, rirB, 16, 20, 0, 1, V, 1.0, 4 * N, hop_size=H, sampling_rate=48000, perceptual=False,
                        seed=0, dtype="f64")
    x = rng.standard_normal((2, (hops + calls + 2) * H))
    ap = mk()
    for h in range(2):                           # warm-up: first launches, clocks
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
    t0 = time.perf_counter()
    for h in range(2, 2 + calls):
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
    per_call = (time.perf_counter() - t0) / calls * 1e3
    ap.close()
    ap = mk()
    out = ap.alloc_signal_output(hops * H)
    ap.process_signal(x[0, :4 * H], x[1, :4 * H])           # sets up the whole-signal path's buffers
    t0 = time.perf_counter()
    ap.process_signal(x[0, :hops * H], x[1, :hops * H], out=out)
    per_hop = (time.perf_counter() - t0) / hops * 1e3
    ap.close()
    return {"L": L, "M": M, "N": N, "H": H, "P": P, "V": V, "fs": 48000,
            "ms_per_process_input_buffers": round(per_call, 3), "ms_per_hop_process_signal": round(per_hop, 3),
            "hop_ms_realtime": round(H / 48.0, 3)}


def main():
    res = {"workload": "subband orders above 64 (kernels_gevd128.hip)", "kernel": kernel()}
    for L in (128, 96):
        res[f"class_L{L}"] = stream(L)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the subband stream's statistics window (apvast(..., statistics_hops=T), csrc/kernels_statwin.hip).

Per-hop wall time of process_input_buffers (median) at cfg3's shape (16 x 32, N 2048, H 1024, 800 taps, f64) for
T in {1, 2, 4, 8, 16} and at one shape with more loudspeakers than control points (128 x 32, N 2048) for T in {1, 4}; for T > 1
also the statistics launch's own time from HIP events around it (a second object with APV_STAT_WINDOW_TIMING set, which runs the
hop's launches uncaptured), the bytes it moves by the traffic model -- one slot written, T read:
(T + 1) Z K (2 L^2 + L) 16 B -- and the fraction of the HBM roof that makes.  A hop of audio at 48 kHz lasts H / 48 ms.
`--forgetting BETA` adds, per shape, a leg with statistics_forgetting=BETA (one slot read and written: the model's T = 1).

Every (shape, T) is one child process under its own time limit; the first that fails or overruns ends the run.  One JSON line
per leg.  `--leg SHAPE T` runs one leg in this process (also the way to time T = 1 on another checkout: the keyword is left out
there); with `--forgetting BETA` (and T = 1) that leg is the forgetting one.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ROOF_GBS = 8000.0        # MI355X HBM3E peak
SHAPES = {"cfg3": dict(L=16, M=32, N=2048, H=1024, P=800, Ts=(1, 2, 4, 8, 16)),
          "wide": dict(L=128, M=32, N=2048, H=1024, P=800, Ts=(1, 4))}


def rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / 120.0)[:, None, None]
    return rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3


def hop_times(obj, H, warm, n):
    x = np.random.default_rng(3).standard_normal((2, (warm + n) * H))
    ts = []
    for h in range(warm + n):
        t0 = time.perf_counter()
        obj.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        ts.append(time.perf_counter() - t0)
    return np.array(ts[warm:]) * 1e3


def leg(shape, T, hops, beta=None):
    from ap_vast_unofficial_amd.apvast import apvast
    s = SHAPES[shape]
    L, M, N, H, P = s["L"], s["M"], s["N"], s["H"], s["P"]
    a0, b0 = rirs(P, L, M, 99)
    kw = {} if T == 1 else dict(statistics_hops=T)          # T = 1 without the keyword: runs on a checkout that lacks it
    if beta is not None:
        kw = dict(statistics_forgetting=beta)
    mk = lambda: apvast(N, a0, b0, 100, 20, 0, 0, 1, 1.0, 4 * N, hop_size=H, perceptual=False, dtype="f64", seed=0, **kw)
    warm = max(8, 2 * T)
    obj = mk()
    ts = hop_times(obj, H, warm, hops)
    obj.close()
    res = dict(shape=shape, L=L, M=M, N=N, H=H, rir_len=P, dtype="f64", statistics_hops=T, hops=hops,
               hop_ms_median=float(np.median(ts)), hop_ms_p90=float(np.percentile(ts, 90)), audio_hop_ms=H / 48.0)
    if beta is not None:
        res["statistics_forgetting"] = beta
    if T > 1 or beta is not None:
        os.environ["APV_STAT_WINDOW_TIMING"] = "1"
        obj = mk()
        hop_times(obj, H, warm, hops)
        ms_sum, count = obj._eng.get_state("stat_window_kernel_ms", (2,), np.float64)
        obj.close()
        del os.environ["APV_STAT_WINDOW_TIMING"]
        K = N // 2 + 1
        model = (T + 1) * 2 * K * (2 * L * L + L) * 16
        k_ms = ms_sum / count                               # (the fill phase's shorter sums are in the mean: warm + hops >> T)
        res.update(stat_kernel_ms=float(k_ms), model_bytes=int(model), model_gbs=float(model / (k_ms * 1e-3) / 1e9),
                   hbm_roof_fraction=float(model / (k_ms * 1e-3) / 1e9 / HBM_ROOF_GBS))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs=2, metavar=("SHAPE", "T"))
    ap.add_argument("--forgetting", type=float, default=None, metavar="BETA")
    ap.add_argument("--hops", type=int, default=100)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        if args.forgetting is not None and int(args.leg[1]) != 1:
            ap.error("--forgetting goes with T = 1: a window and forgetting exclude each other")
        leg(args.leg[0], int(args.leg[1]), args.hops, args.forgetting)
        return 0
    for shape, s in SHAPES.items():
        legs = [(T, []) for T in s["Ts"]]
        if args.forgetting is not None:
            legs.append((1, ["--forgetting", str(args.forgetting)]))
        for T, extra in legs:
            # one child per leg, under its own time limit; nothing more is started after a leg that fails or overruns
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", shape,
                                str(T), "--hops", str(args.hops if shape == "cfg3" else max(args.hops // 4, 10))] + extra)
            if r.returncode != 0:
                print(json.dumps(dict(shape=shape, statistics_hops=T, forgetting=bool(extra), failed=r.returncode)), flush=True)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

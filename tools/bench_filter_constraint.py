#!/usr/bin/env python3
"""Cost of the subband stream's filter-length constraint (apvast(..., constrain_filter_length=True), csrc/kernels_constrain.hip).

Per-hop wall time of process_input_buffers (median) at cfg3's shape (16 x 32, N 2048, H 1024, 800 taps, f64, V = 16, both zone
programs: Z V L = 512 channels) without the keyword and with it (J = 256), and the projection launch's own time from HIP events
around it (a second object with APV_FILTER_CONSTRAINT_TIMING set, which runs the hop's launches uncaptured), the bytes it moves
by the traffic model of DESIGN.md section 4.15 -- every filter element read once and written once, the taps written once:
Z V L (2 K 16 + J 8) B in float64 -- and the fraction of the HBM roof that makes.  A hop of audio at 48 kHz lasts H / 48 ms.

Each leg is one child process under its own time limit; the first that fails or overruns ends the run.  One JSON line per leg.
`--leg off|on` runs one leg in this process (`off` leaves the keyword out: it runs on a checkout that lacks it).
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
CFG3 = dict(L=16, M=32, N=2048, H=1024, P=800, V=16, J=256)


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


def leg(on, hops):
    from ap_vast_unofficial_amd.apvast import apvast
    s = CFG3
    L, M, N, H, P, V, J = s["L"], s["M"], s["N"], s["H"], s["P"], s["V"], s["J"]
    a0, b0 = rirs(P, L, M, 99)
    kw = dict(constrain_filter_length=True) if on else {}
    mk = lambda: apvast(N, a0, b0, J, 20, 0, 0, V, 1.0, 4 * N, hop_size=H, perceptual=False, dtype="f64", seed=0, **kw)
    obj = mk()
    ts = hop_times(obj, H, 8, hops)
    obj.close()
    res = dict(shape="cfg3", L=L, M=M, N=N, H=H, rir_len=P, V=V, dtype="f64", constrain_filter_length=on, filter_length=J, hops=hops,
               hop_ms_median=float(np.median(ts)), hop_ms_p10=float(np.percentile(ts, 10)), hop_ms_p90=float(np.percentile(ts, 90)),
               audio_hop_ms=H / 48.0)
    if on:
        os.environ["APV_FILTER_CONSTRAINT_TIMING"] = "1"
        obj = mk()
        hop_times(obj, H, 8, hops)
        ms_sum, count = obj._eng.get_state("filter_constraint_kernel_ms", (2,), np.float64)
        obj.close()
        del os.environ["APV_FILTER_CONSTRAINT_TIMING"]
        K = N // 2 + 1
        model = 2 * V * L * (2 * K * 16 + J * 8)
        k_ms = ms_sum / count
        res.update(channels=2 * V * L, constraint_kernel_ms=float(k_ms), model_bytes=int(model),
                   model_gbs=float(model / (k_ms * 1e-3) / 1e9), hbm_roof_fraction=float(model / (k_ms * 1e-3) / 1e9 / HBM_ROOF_GBS))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("off", "on"))
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg == "on", args.hops)
        return 0
    for name in ("off", "on", "off", "on"):
        # one child per leg, under its own time limit; nothing more is started after a leg that fails or overruns
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
                            "--hops", str(args.hops)])
        if r.returncode != 0:
            print(json.dumps(dict(leg=name, failed=r.returncode)), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

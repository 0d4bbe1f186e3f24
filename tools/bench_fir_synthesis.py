#!/usr/bin/env python3
"""Cost of the constrained subband stream's FIR synthesis (apvast(..., synthesis="fir"), csrc/kernels_firsynth.hip).

Per-hop wall time of process_input_buffers (median) at cfg3's shape (16 x 32, N 2048, H 1024, 800 taps, f64, V = 16, J = 256, both
zone programs: Z V = 32 groups of H x L results) of the constrained stream with the WOLA synthesis and with the FIR synthesis, and
the synthesis launch's own time from HIP events around it (a second object with APV_FIR_SYNTHESIS_TIMING set, which runs the hop's
launches uncaptured), against the flop model of DESIGN.md section 4.16 -- two GEMMs of H x J by J x L per group, 2 Z V L H J
multiply-adds -- as a share of the float64 MFMA peak and of the hop.  A hop of audio at 48 kHz lasts H / 48 ms.

Each leg is one child process under its own time limit; the first that fails or overruns ends the run.  One JSON line per leg.
`--leg wola|fir` runs one leg in this process (`wola` leaves the keyword out: it runs on a checkout that lacks it).
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

F64_MFMA_PEAK_TFLOPS = 78.6      # MI355X, float64 matrix, data sheet
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


def leg(fir, hops):
    from ap_vast_unofficial_amd.apvast import apvast
    s = CFG3
    L, M, N, H, P, V, J = s["L"], s["M"], s["N"], s["H"], s["P"], s["V"], s["J"]
    a0, b0 = rirs(P, L, M, 99)
    kw = dict(synthesis="fir") if fir else {}
    mk = lambda: apvast(N, a0, b0, J, 20, 0, 0, V, 1.0, 4 * N, hop_size=H, perceptual=False, dtype="f64", seed=0,
                        constrain_filter_length=True, **kw)
    obj = mk()
    ts = hop_times(obj, H, 8, hops)
    obj.close()
    res = dict(shape="cfg3", L=L, M=M, N=N, H=H, rir_len=P, V=V, dtype="f64", filter_length=J, synthesis="fir" if fir else "wola",
               hops=hops, hop_ms_median=float(np.median(ts)), hop_ms_p10=float(np.percentile(ts, 10)),
               hop_ms_p90=float(np.percentile(ts, 90)), audio_hop_ms=H / 48.0)
    if fir:
        os.environ["APV_FIR_SYNTHESIS_TIMING"] = "1"
        obj = mk()
        hop_times(obj, H, 8, hops)
        ms_sum, count = obj._eng.get_state("fir_synthesis_kernel_ms", (2,), np.float64)
        obj.close()
        del os.environ["APV_FIR_SYNTHESIS_TIMING"]
        flop = 2 * 2 * (2 * V) * L * H * J           # two GEMMs, 2 flop per multiply-add, Z = 2 zone programs
        k_ms = ms_sum / count
        res.update(groups=2 * V, synthesis_kernel_ms=float(k_ms), model_gflop=flop / 1e9,
                   model_tflops=float(flop / (k_ms * 1e-3) / 1e12),
                   f64_mfma_peak_fraction=float(flop / (k_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS),
                   hop_fraction=float(k_ms / np.median(ts)))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("wola", "fir"))
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg == "fir", args.hops)
        return 0
    for name in ("wola", "fir", "wola", "fir"):
        # one child per leg, under its own time limit; nothing more is started after a leg that fails or overruns
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
                            "--hops", str(args.hops)])
        if r.returncode != 0:
            print(json.dumps(dict(leg=name, failed=r.returncode)), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

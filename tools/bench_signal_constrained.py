#!/usr/bin/env python3
"""process_signal of the subband stream at cfg3's shape (16 x 32, N 2048, H 1024, 800-tap responses, f64, V = 16, J = 256, both
zone programs): ms per hop of the default stream, of the constrained stream (constrain_filter_length=True, WOLA synthesis) and of
the constrained stream with synthesis="fir", and the schedule each call took (apvast.signal_schedule: hops through chunk launches,
hops hop by hop; "unknown" on a checkout that lacks the attribute, where a constrained stream runs hop by hop).

The chunked schedule (DESIGN.md sections 4.5 and 4.17) launches one projection and, for "fir", one synthesis per chunk of sixteen
hops; their own times come from a kernel trace of one leg (`--leg fir` under a profiler), not from this tool's wall clock.

Each leg is one child process under its own time limit; the first that fails or overruns ends the run.  One JSON line per leg.
`--leg default|wola|fir` runs one leg in this process.
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

CFG3 = dict(L=16, M=32, N=2048, H=1024, P=800, V=16, J=256)
LEGS = ("default", "wola", "fir")


def rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / 120.0)[:, None, None]
    return rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3


def leg(name, hops, repeats):
    from ap_vast_unofficial_amd.apvast import apvast
    s = CFG3
    L, M, N, H, P, V, J = s["L"], s["M"], s["N"], s["H"], s["P"], s["V"], s["J"]
    a0, b0 = rirs(P, L, M, 99)
    kw = {} if name == "default" else dict(constrain_filter_length=True)
    if name == "fir":
        kw["synthesis"] = "fir"
    obj = apvast(N, a0, b0, J, 20, 0, 0, V, 1.0, 4 * N, hop_size=H, perceptual=False, dtype="f64", seed=0, **kw)
    x = np.random.default_rng(3).standard_normal((2, hops * H))
    out = obj.alloc_signal_output(hops * H)
    obj.process_signal(x[0, :32 * H], x[1, :32 * H])          # warm-up: buffers, streams, graphs, clocks
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        obj.process_signal(x[0], x[1], out=out)
        ms.append((time.perf_counter() - t0) * 1e3 / hops)
    sched = getattr(obj, "signal_schedule", None)
    obj.close()
    print(json.dumps(dict(shape="cfg3", L=L, M=M, N=N, H=H, rir_len=P, V=V, dtype="f64", filter_length=J, stream=name, hops=hops,
                          hop_ms_median=float(np.median(ms)), hop_ms_min=float(min(ms)), hop_ms_max=float(max(ms)), repeats=repeats,
                          signal_schedule=list(sched) if sched is not None else "unknown", audio_hop_ms=H / 48.0)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--hops", type=int, default=160)
    ap.add_argument("--repeats", type=int, default=5, help="timed process_signal calls per leg")
    ap.add_argument("--timeout", type=int, default=180, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.hops, args.repeats)
        return 0
    for name in LEGS:
        # one child per leg, under its own time limit; nothing more is started after a leg that fails or overruns
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
                            "--hops", str(args.hops), "--repeats", str(args.repeats)])
        if r.returncode != 0:
            print(json.dumps(dict(leg=name, failed=r.returncode)), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

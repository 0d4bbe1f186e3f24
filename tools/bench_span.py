#!/usr/bin/env python3
"""Cost of the per-bin span of the subband stream (apvast(..., mu_profile=, rank_profile=, contrast_floor_db=), csrc/gevd_span.h).

At cfg3's shape (16 x 32, N 2048, H 1024, 800 taps, f64, one rank: the order-16 kernel, which carries the span as a branch) and at
64 x 72 with the same block (the order-64 kernel, whose span instantiation spills: profiles/span_profile.md) two legs, each
without the keywords and with all three (a mu profile rising tenfold over the bins, a cap of 1, a floor of 3 dB):

  hop      per-hop wall time of process_input_buffers (median, p90)
  signal   process_signal over `--hops` hops: wall time per hop and the schedule it took (apvast.signal_schedule)

A hop of audio at 48 kHz lasts H / 48 ms.  Every leg is one child process under its own time limit; the first that fails or
overruns ends the run.  One JSON line per leg.  `--leg SHAPE KIND SPAN` (cfg3 | order64, hop | signal, 0 | 1) runs one leg in this
process; SPAN = 0 leaves the keywords out, so that leg also runs on a checkout that lacks them.
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

N, H, P = 2048, 1024, 800
SHAPES = {"cfg3": (16, 32), "order64": (64, 72)}


def rirs(seed, L, M):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / 120.0)[:, None, None]
    return rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3


def make(span, L, M):
    from ap_vast_unofficial_amd.apvast import apvast
    a0, b0 = rirs(99, L, M)
    K = N // 2 + 1
    kw = dict(mu_profile=np.geomspace(1.0, 10.0, K), rank_profile=np.ones(K, dtype=np.int32), contrast_floor_db=3.0) if span else {}
    return apvast(N, a0, b0, 100, 20, 0, 0, 1, 1.0, 4 * N, hop_size=H, perceptual=False, dtype="f64", seed=0, **kw)


def leg(shape, kind, span, hops):
    L, M = SHAPES[shape]
    obj = make(span, L, M)
    res = dict(shape=shape, leg=kind, span=bool(span), L=L, M=M, N=N, H=H, rir_len=P, dtype="f64", hops=hops, audio_hop_ms=H / 48.0)
    if kind == "hop":
        warm = 8
        x = np.random.default_rng(3).standard_normal((2, (warm + hops) * H))
        ts = []
        for h in range(warm + hops):
            t0 = time.perf_counter()
            obj.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts[warm:]) * 1e3
        res.update(hop_ms_median=float(np.median(ts)), hop_ms_p90=float(np.percentile(ts, 90)))
    else:
        x = np.random.default_rng(3).standard_normal((2, hops * H))
        out = obj.alloc_signal_output(hops * H)
        ts = []
        for _ in range(4):                                    # the first call allocates the chunk buffers
            t0 = time.perf_counter()
            obj.process_signal(x[0], x[1], out=out)
            ts.append(time.perf_counter() - t0)
        res.update(signal_ms_per_hop=float(np.median(ts[1:]) * 1e3 / hops), schedule=list(obj.signal_schedule))
    if span:
        res["span_rank_max"] = int(obj.span_rank_A.max())
    obj.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs=3, metavar=("SHAPE", "KIND", "SPAN"))
    ap.add_argument("--hops", type=int, default=96)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        if args.leg[0] not in SHAPES or args.leg[1] not in ("hop", "signal") or args.leg[2] not in ("0", "1"):
            ap.error("--leg cfg3|order64 hop|signal 0|1")
        leg(args.leg[0], args.leg[1], int(args.leg[2]), args.hops)
        return 0
    for shape in SHAPES:
        for kind in ("hop", "signal"):
            for span in (0, 1):
                # one child per leg, under its own time limit; nothing more is started after a leg that fails or overruns
                r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", shape,
                                    kind, str(span), "--hops", str(args.hops if shape == "cfg3" else max(args.hops // 2, 16))])
                if r.returncode != 0:
                    print(json.dumps(dict(shape=shape, leg=kind, span=bool(span), failed=r.returncode)), flush=True)
                    return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

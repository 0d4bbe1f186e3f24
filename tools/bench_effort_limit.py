#!/usr/bin/env python3
"""Cost of the per-bin array-effort limit of the subband stream (apvast(..., effort_limit_db=), csrc/kernels_effort.hip).

At cfg3's shape (16 x 32, N 2048, H 1024, 800 taps, f64, one rank: the order-16 kernel and the batched chunk launch) and at
64 x 72 with the same block (the order-64 kernel, hop by hop on the back streams) two legs, each without the keyword and with a
limit of -12 dB in every bin:

  hop      per-hop wall time of process_input_buffers (median, p90)
  signal   process_signal over `--hops` hops: wall time per hop and the schedule it took (apvast.signal_schedule)

A hop of audio at 48 kHz lasts H / 48 ms.  Every leg is one child process under its own time limit; the first that fails or
overruns ends the run.  One JSON line per leg.  `--leg SHAPE KIND LIMIT` (cfg3 | order64, hop | signal, 0 | 1) runs one leg in this
process; LIMIT = 0 leaves the keyword out, so that leg also runs on a checkout that lacks it.

`--parent DIR` names a built checkout of the parent commit: every leg without the keyword then runs `--repeat` times from DIR and
from this tree in turn (parent, change, parent, change, ...), which gives the parent's own run-to-run spread in the session --
the bar for "the stream without the keyword is unchanged".

The stage's own kernel time comes from a profiler, not from here: `rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python
tools/bench_effort_limit.py --leg cfg3 signal 1` and the line of `limit_effort_kernel` in the statistics."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, H, P = 2048, 1024, 800
SHAPES = {"cfg3": (16, 32), "order64": (64, 72)}
LIMIT_DB = -12.0


def rirs(seed, L, M):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / 120.0)[:, None, None]
    return rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3


def make(limit, L, M):
    from ap_vast_unofficial_amd.apvast import apvast
    a0, b0 = rirs(99, L, M)
    kw = dict(effort_limit_db=LIMIT_DB) if limit else {}
    return apvast(N, a0, b0, 100, 20, 0, 0, 1, 1.0, 4 * N, hop_size=H, perceptual=False, dtype="f64", seed=0, **kw)


def leg(shape, kind, limit, hops, root):
    sys.path.insert(0, root)
    L, M = SHAPES[shape]
    obj = make(limit, L, M)
    res = dict(shape=shape, leg=kind, limit=bool(limit), tree=os.path.relpath(root, ROOT), L=L, M=M, N=N, H=H, rir_len=P, dtype="f64",
               hops=hops, audio_hop_ms=H / 48.0)
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
    if limit:
        g = obj.effort_gain_A
        res.update(bins_scaled=float((g != 1.0).mean()), effort_db_max=float(10 * np.log10(obj.effort_A.max())))
    obj.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs=3, metavar=("SHAPE", "KIND", "LIMIT"))
    ap.add_argument("--root", default=ROOT, help="the checkout whose package a --leg imports")
    ap.add_argument("--parent", help="a built checkout of the parent commit: alternate it against this tree on the legs without the keyword")
    ap.add_argument("--repeat", type=int, default=3, help="runs per tree of an alternated leg")
    ap.add_argument("--hops", type=int, default=96)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        if args.leg[0] not in SHAPES or args.leg[1] not in ("hop", "signal") or args.leg[2] not in ("0", "1"):
            ap.error("--leg cfg3|order64 hop|signal 0|1")
        leg(args.leg[0], args.leg[1], int(args.leg[2]), args.hops, os.path.abspath(args.root))
        return 0
    for shape in SHAPES:
        for kind in ("hop", "signal"):
            for limit in (0, 1):
                trees = [ROOT]
                if not limit and args.parent:
                    trees = [os.path.abspath(args.parent), ROOT] * args.repeat
                for tree in trees:
                    # one child per leg, under its own time limit; nothing more is started after a leg that fails or overruns
                    r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg",
                                        shape, kind, str(limit), "--root", tree, "--hops",
                                        str(args.hops if shape == "cfg3" else max(args.hops // 2, 16))])
                    if r.returncode != 0:
                        print(json.dumps(dict(shape=shape, leg=kind, limit=bool(limit), failed=r.returncode)), flush=True)
                        return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

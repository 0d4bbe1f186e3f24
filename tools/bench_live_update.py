#!/usr/bin/env python3
"""Cost of reassigning responses and mu between hops (class apvast, rir_* / target_rir_* / mu setters).

For cfg3 (N 2048, H 1024, P 800, 16 x 32; f64 and mixed) and broadband at the reference's test shape with n = J L = 800: median
wall time of a plain hop, of a hop that applies an RIR update (rir_A and rir_B replaced: one upload, one correction launch) and
of a hop that applies a mu update.  One JSON line per shape.  A hop of audio at 48 kHz lasts H / 48 ms (21.3 ms at H = 1024).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / 120.0)[:, None, None]
    return rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3


def measure(obj, H, n_plain, n_updates, sets, drain):
    x = np.random.default_rng(3).standard_normal((2, H))
    hop = lambda: obj.process_input_buffers(x[0], x[1])
    for _ in range(4):
        hop()

    def timed(before):
        ts = []
        for i in range(n_updates):
            before(i)
            t0 = time.perf_counter()
            hop()
            ts.append(time.perf_counter() - t0)
            # let every tail drain so that the next sample is an update hop again, not a hop that only adds a tail
            for _ in range(drain):
                hop()
        return float(np.median(ts)) * 1e3

    plain = []
    for _ in range(n_plain):
        t0 = time.perf_counter()
        hop()
        plain.append(time.perf_counter() - t0)

    def rir_update(i):
        obj.rir_A, obj.rir_B = sets[i % 2]

    def mu_update(i):
        obj.mu = 1.0 + 0.5 * (i % 2 + 1)

    return dict(plain_hop_ms=float(np.median(plain)) * 1e3, rir_update_hop_ms=timed(rir_update), mu_update_hop_ms=timed(mu_update),
                updates=n_updates)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=24)
    ap.add_argument("--plain", type=int, default=100)
    args = ap.parse_args()
    from ap_vast_unofficial_amd.apvast import apvast
    # cfg3
    N, H, L, M, P = 2048, 1024, 16, 32, 800
    sets = [rirs(P, L, M, 5), rirs(P, L, M, 6)]
    for dtype in ("f64", "mixed"):
        a0, b0 = rirs(P, L, M, 99)
        obj = apvast(N, a0, b0, 100, 20, 0, 0, 1, 1.0, 4 * N, hop_size=H, perceptual=False, dtype=dtype, seed=0)
        r = measure(obj, H, args.plain, args.updates, sets, -(-(P - 1) // H))
        print(json.dumps(dict(workload=f"cfg3 subband N={N} H={H} L={L} M={M} rir_len={P}", dtype=dtype, audio_hop_ms=H / 48.0, **r)))
        obj.close()
    # broadband at the reference's test parameters (make_python_test.m): N 256, H 128, J 100, 8 loudspeakers -> n = 800
    N, H, L, M, P, J = 256, 128, 8, 8, 800, 100
    sets = [rirs(P, L, M, 5), rirs(P, L, M, 6)]
    a0, b0 = rirs(P, L, M, 99)
    obj = apvast(N, a0, b0, J, 16, 0, 0, 8, 1.0, 1024, hop_size=H, perceptual=False, mode="broadband", seed=0)
    r = measure(obj, H, args.plain // 4, args.updates, sets, -(-(P - 1) // H))
    print(json.dumps(dict(workload=f"broadband N={N} H={H} J={J} L={L} M={M} rir_len={P} n={J * L}", dtype="f64",
                          audio_hop_ms=H / 48.0, **r)))
    obj.close()


if __name__ == "__main__":
    main()

"""Broadband mode at the size of the reference's MATLAB demo (main.m:34-42): N = 1020, H = 510, J = 400, L = 10 (n = J L =
4000), 8 kHz, MATLAB dialect, ranks [1, 2000, 4000], synthetic responses with 8 microphones.  Prints one JSON line with

  * ms per hop through process_input_buffers and through process_signal,
  * the stage split and the sweeps of the complete solve (APV_BB_TIMING=1, in a child process: the switch is read once),
  * the device memory in use after the hops,
  * the CPU oracle's time for one hop,
  * ||R||_2 device times of both norm kernels at a range of orders (four matrices, as a hop has them).

    python tools/bench_broadband_main_m.py [--hops K] [--warmup W] [--skip-oracle]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, J, L, M, S, P, DELAY = 1020, 400, 10, 8, 1020, 500, 50
RANKS = [1, 2000, 4000]
NORM_ORDERS = [1024, 1536, 2048, 2560, 3072, 4000, 4096]


def synth_rirs(seed=31):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


def make():
    from ap_vast_unofficial_amd.apvast import apvast
    rA, rB = synth_rirs()
    ap = apvast(N, rA, rB, J, DELAY, 0, 0, RANKS, 1.0, S, sampling_rate=8000, perceptual=False, mode="broadband",
                dialect="matlab")
    rng = np.random.default_rng(21)
    st = ap.get_state()
    ap.set_state({"response": 1e-3 * rng.standard_normal(st["response"].shape),
                  "target_response": 1e-3 * rng.standard_normal(st["target_response"].shape)})
    return ap


def signal(hops):
    return np.random.default_rng(8).standard_normal((2, hops * N // 2))


def device_used_bytes():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def timing_child(hops):
    """Runs with APV_BB_TIMING=1: stage lines of a few hops, then the norm kernels' device times."""
    from ap_vast_unofficial_amd import _capi
    ap = make()
    H = ap.hop_size
    x = signal(hops)
    for h in range(hops):
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
    ap.close()
    eng = _capi.Engine(1, 4, 4)
    rng = np.random.default_rng(3)
    for n in NORM_ORDERS:
        G = rng.standard_normal((n, n)) / np.sqrt(n)
        R = G @ G.T
        mats = np.stack([R] * 4)
        for method in ("one_wg", "grid"):
            for _ in range(3):            # the first call of a shape loads code and sets up the pool
                eng.norm2(mats, method)
    eng.close()


def parse_timing(err):
    stages = [tuple(float(v) for v in m) for m in re.findall(
        r"\[apv bb\] fir ([\d.]+)\s+wola ([\d.]+)\s+stats ([\d.]+)\s+gevd ([\d.]+)\s+out ([\d.]+) ms", err)]
    sweeps = [(int(k), float(f), float(sw), float(so)) for f, k, sw, so in re.findall(
        r"\[apv gevd_large\] n=4000 batch=\d+: factor\+whiten ([\d.]+) ms, (\d+) sweeps ([\d.]+) ms, sort\+filter ([\d.]+) ms", err)]
    norms = {}
    for n, method, ms in re.findall(r"\[apv norm2\] n=(\d+) count=4 method=(\d): ([\d.]+) ms", err):
        norms.setdefault(f"{n}/{'one_wg' if method == '1' else 'grid'}", []).append(float(ms))
    # the last of the three calls of each shape
    norms = {k: v[-1] for k, v in norms.items()}
    return stages, sweeps, norms


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--hops", type=int, default=4)
    ap_.add_argument("--warmup", type=int, default=1)
    ap_.add_argument("--skip-oracle", action="store_true")
    ap_.add_argument("--timing-child", action="store_true", help=argparse.SUPPRESS)
    a = ap_.parse_args()
    if a.timing_child:
        timing_child(3)
        return
    out = {"shape": dict(N=N, H=N // 2, J=J, L=L, M=M, S=S, n=J * L, ranks=RANKS, fs=8000, dialect="matlab")}
    # the stage split, sweeps and norm times first, in a child process of their own
    env = dict(os.environ, APV_BB_TIMING="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--timing-child"], env=env, capture_output=True, text=True,
                       timeout=1800)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"timing child failed with {r.returncode}")
    stages, sweeps, norms = parse_timing(r.stderr)
    out["stages_ms_per_hop"] = [dict(zip(("fir", "wola", "stats", "gevd", "out"), s)) for s in stages]
    out["complete_solve"] = [dict(sweeps=s[0], factor_whiten_ms=s[1], sweeps_ms=s[2], sort_filter_ms=s[3]) for s in sweeps]
    out["norm2_ms_4_matrices"] = norms

    import torch
    torch.cuda.init()
    base = device_used_bytes()
    ap = make()
    H = ap.hop_size
    x = signal(a.warmup + a.hops)
    for h in range(a.warmup):
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
    t0 = time.perf_counter()
    for h in range(a.warmup, a.warmup + a.hops):
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
    out["ms_per_hop_process_input_buffers"] = 1e3 * (time.perf_counter() - t0) / a.hops
    out["device_bytes_per_hop_path"] = device_used_bytes() - base
    ap.close()
    b = make()
    b.process_signal(x[0, :a.warmup * H], x[1, :a.warmup * H])
    t0 = time.perf_counter()
    b.process_signal(x[0, a.warmup * H:], x[1, a.warmup * H:])
    out["ms_per_hop_process_signal"] = 1e3 * (time.perf_counter() - t0) / a.hops
    out["device_bytes_process_signal"] = device_used_bytes() - base
    b.close()
    out["audio_ms_per_hop"] = 1e3 * H / 8000.0
    if not a.skip_oracle:
        from oracle.broadband_matlab import MatlabBroadbandOracle
        rA, rB = synth_rirs()
        orc = MatlabBroadbandOracle(N, rA, rB, J, DELAY, 0, 0, RANKS, 1.0, S, sampling_rate=8000)
        t0 = time.perf_counter()
        orc.process_input_buffers(x[0, :H], x[1, :H])
        out["oracle_ms_per_hop_cpu"] = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

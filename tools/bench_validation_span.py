#!/usr/bin/env python3
"""Cost and effect of the rank choice by validation contrast (apvast(..., validation_floor_db=), csrc/kernels_valspan.hip).

The scene is that of tools/bench_stream_evaluation.py: cfg3's shape (16 x 32, N 2048, H 1024, 800-tap responses, float64, both zone
programs), validation responses = the control responses plus 10 % noise (Pv 800, Mv 32), V = 16, `evaluation_ranks=[16]`.

  hop FLOOR     per-hop wall time of process_input_buffers (median of `--hops` hops after 8 warm-up hops) with the evaluation
                keywords, without the floor (FLOOR = none) and with it (a dB value; `median` = the median of the stage's own
                contrast curves, taken from a run with -inf); the time-domain contrast and NMSE of the evaluation stage over the
                same hops, and the ranks the stage chose
  kernel        the launch alone between two HIP events (apv_validation_span's h_ms) at K 1025, L 16, Mv 32, nV 16, complex128,
                one program: median of `--reps` calls, the bytes it must move (two banks, one filter set) and the share of the
                HBM roof that is

Every leg is one fresh child process under its own time limit; the first that fails or overruns ends the run.  One JSON line per
leg.  Without `--leg` the tool runs hop none / hop 0 twice in turn, hop median, and the kernel leg, and writes
sections 1 to 3 of profiles/validation_span.md (a section 4 that is there is kept)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_ROOF_GBS = 8000.0            # MI355X, data sheet
V = 16


def make(floor_db):
    from bench_stream_evaluation import CFG3 as s, rirs, validation
    from ap_vast_unofficial_amd.apvast import apvast
    a0, b0 = rirs(s["P"], s["L"], s["M"], 99)
    va, vb = validation(a0, b0)
    kw = {} if floor_db is None else dict(validation_floor_db=floor_db)
    return apvast(s["N"], a0, b0, s["J"], 20, 0, 0, V, 1.0, 4 * s["N"], hop_size=s["H"], perceptual=False, dtype="f64", seed=0,
                  validation_rir_A=va, validation_rir_B=vb, evaluation_ranks=[V], **kw), s["H"]


def run_hops(obj, H, hops, warm=8):
    x = np.random.default_rng(3).standard_normal((2, (warm + hops) * H))
    ts = []
    for h in range(warm + hops):
        if h == warm:
            obj.reset_evaluation()
        t0 = time.perf_counter()
        obj.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        ts.append(time.perf_counter() - t0)
    return np.array(ts[warm:]) * 1e3


def leg_hop(floor, hops):
    from ap_vast_unofficial_amd.evaluation import metrics
    floor_db = None if floor == "none" else floor
    if floor == "median":
        probe, H = make(-np.inf)
        run_hops(probe, H, 8, warm=0)
        c = np.concatenate([(getattr(probe, "validation_bright_" + z) / getattr(probe, "validation_dark_" + z)).ravel() for z in "AB"])
        floor_db = float(10 * np.log10(np.median(c)))
        probe.close()
    elif floor_db is not None:
        floor_db = float(floor_db)
    obj, H = make(floor_db)
    ts = run_hops(obj, H, hops)
    m = metrics(obj.evaluation_totals())
    res = dict(leg="hop", floor=floor, floor_db=floor_db, hops=hops, hop_ms_median=float(np.median(ts)),
               hop_ms_p10=float(np.percentile(ts, 10)), hop_ms_p90=float(np.percentile(ts, 90)), audio_hop_ms=H / 48.0,
               contrast_db=m["contrast_db"][:, 0].tolist(), nmse=m["nmse"][:, 0].tolist())
    if floor_db is not None:
        ranks = np.concatenate([obj.validation_rank_A, obj.validation_rank_B])
        res.update(rank_mean=float(ranks.mean()), rank_full_share=float((ranks == V).mean()))
    obj.close()
    print(json.dumps(res), flush=True)


def leg_kernel(reps):
    from ap_vast_unofficial_amd import Engine
    K, L, Mv, nV = 1025, 16, 32, 16
    rng = np.random.default_rng(0)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    W, GB, GD = cn(K, nV, L), cn(K, Mv, L), cn(K, Mv, L)
    eng = Engine(4, 4, 4, ranks=(1,), compute_dtype="f64")
    out = {}
    for name, phi in (("median_floor", 1.0), ("no_floor", 0.0)):
        ts = [eng.validation_span_kernel(W, GB, GD, np.full(K, phi), timed=True)[-1] for _ in range(reps)]
        out[name + "_us"] = float(np.median(ts[2:]) * 1e3)
    eng.close()
    nbytes = 16 * (2 * K * Mv * L + K * nV * L) + 20 * K * nV
    us = out["no_floor_us"]
    print(json.dumps(dict(leg="kernel", K=K, L=L, Mv=Mv, nV=nV, reps=reps, bytes=nbytes, **out,
                          gbs=nbytes / us * 1e-3, hbm_share=nbytes / us * 1e-3 / HBM_ROOF_GBS)), flush=True)


def child(leg, timeout, hops, reps):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--leg", *leg, "--hops", str(hops),
           "--reps", str(reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    if r.returncode != 0:
        print(json.dumps(dict(leg=leg, failed=r.returncode)), flush=True)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", nargs="+", metavar="LEG", help="hop none|median|<dB>, or kernel")
    ap.add_argument("--hops", type=int, default=100)
    ap.add_argument("--reps", type=int, default=22)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_span.md"))
    args = ap.parse_args()
    if args.leg:
        if args.leg[0] == "kernel":
            leg_kernel(args.reps)
        elif args.leg[0] == "hop" and len(args.leg) == 2:
            leg_hop(args.leg[1], args.hops)
        else:
            ap.error("--leg hop none|median|<dB> | --leg kernel")
        return 0
    res = []
    for leg in (["hop", "none"], ["hop", "0"], ["hop", "none"], ["hop", "0"], ["hop", "median"], ["kernel"]):
        r = child(leg, args.timeout, args.hops, args.reps)
        if r is None:                                          # nothing more is started after a leg that fails or overruns
            return 1
        res.append(r)
    off, on, med, ker = [res[0], res[2]], [res[1], res[3]], res[4], res[5]
    f = lambda v: ", ".join(f"{x:.4f}" for x in v)
    g = lambda v: " / ".join(f"{x:.2f}" for x in v)
    t_off, t_on = np.mean([r["hop_ms_median"] for r in off]), np.mean([r["hop_ms_median"] for r in on])
    lines = [
        "# The rank choice by validation contrast: what it costs and what it does",
        "",
        f"MI355X (gfx950); `tools/bench_validation_span.py`, cfg3 (16 x 32, N 2048, H 1024, 800-tap responses, float64, both zone",
        f"programs), validation responses = the control responses plus 10 % noise (Pv 800, Mv 32), V = 16, `evaluation_ranks=[16]`.",
        f"Every leg a fresh process; medians of {off[0]['hops']} hops after 8 warm-up hops; a hop of audio lasts {off[0]['audio_hop_ms']:.2f} ms.",
        "No time was fixed in advance.",
        "",
        "## 1. The hop with the evaluation keywords, without and with the floor (two runs each, in turn)",
        "",
        "| leg | ms per hop, medians of the runs | mean |",
        "|---|---|---|",
        f"| without `validation_floor_db` | {f([r['hop_ms_median'] for r in off])} | {t_off:.4f} |",
        f"| with a floor of 0 dB | {f([r['hop_ms_median'] for r in on])} | {t_on:.4f} |",
        "",
        f"Difference of the means: {t_on - t_off:+.4f} ms per hop ({100 * (t_on / t_off - 1):+.1f} %).",
        "",
        "## 2. The launch alone (HIP events around it, one zone program, complex128)",
        "",
        f"K {ker['K']}, L {ker['L']}, Mv {ker['Mv']}, nV {ker['nV']}: {ker['no_floor_us']:.1f} us without a floor (no copies), "
        f"{ker['median_floor_us']:.1f} us with a floor of 1 (linear)",
        f"on random filters; {ker['bytes'] / 1e6:.1f} MB of banks, filters and outputs, {ker['gbs']:.0f} GB/s, "
        f"{100 * ker['hbm_share']:.1f} % of the {HBM_ROOF_GBS / 1000:.0f} TB/s HBM roof.  The call",
        "uploads its operands just before the launch, so part of them is served from the caches.",
        "",
        "## 3. What the floor does to the time-domain evaluation (program A / program B, the top filter's outputs)",
        "",
        "| floor | contrast, dB | NMSE | mean chosen rank | bins at rank 16 |",
        "|---|---|---|---|---|",
        f"| none | {g(off[0]['contrast_db'])} | {g(off[0]['nmse'])} | 16 | 100 % |",
        f"| 0 dB | {g(on[0]['contrast_db'])} | {g(on[0]['nmse'])} | {on[0]['rank_mean']:.2f} | {100 * on[0]['rank_full_share']:.0f} % |",
        f"| the median of the stage's own curves, {med['floor_db']:.2f} dB | {g(med['contrast_db'])} | {g(med['nmse'])} | "
        f"{med['rank_mean']:.2f} | {100 * med['rank_full_share']:.0f} % |",
        "",
        "Not gated.  The stage predicts the contrast of a stationary filter per bin; the evaluation stage measures the time-domain",
        "energies of filters that change every hop, over all bins at once.",
    ]
    # section 4 (the stream without the keyword and the headline, parent against change) is measured with a checkout of the
    # parent and written by hand: it is kept
    kept = ""
    if os.path.exists(args.out):
        old = open(args.out).read()
        if "\n## 4." in old:
            kept = old[old.index("\n## 4."):]
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n" + kept)
    return 0


if __name__ == "__main__":
    sys.exit(main())

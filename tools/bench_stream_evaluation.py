#!/usr/bin/env python3
"""Cost and first results of the subband stream's evaluation stage (apvast(..., validation_rir_A=, validation_rir_B=),
csrc/kernels_streameval.hip).

At cfg3's shape (16 x 32, N 2048, H 1024, 800 taps, f64, both zone programs) with Pv = 800 validation taps and Mv = 32 validation
microphones:

  * per-hop wall time of process_input_buffers (median) with and without the keywords, for the WOLA stream and the constrained FIR
    stream (J = 256), at V = 1 and at V = 16 with evaluation_ranks=[V] -- every leg a fresh child process, the two legs of a pair
    alternating (off, on, off, on);
  * the pressure launch alone (apv_eval_pressure on device buffers of the stream's sizes, timed with HIP events) against the flop
    model 2 sets H L Pv Mv at the float64 matrix peak, and its share of the hop;
  * contrast_db and nmse (evaluation.metrics on the accumulated totals) of the WOLA, constrained-WOLA and FIR streams on the same
    signal: recorded, not gated.  The validation responses are the control responses with 10 % independent noise added.

`--spectra` runs the leg of the per-bin spectra instead (apvast(..., evaluation_spectra=True), csrc/kernels_evalspec.hip): ms per
hop of process_input_buffers with the evaluation stage alone and with the spectra, WOLA stream, V = 1 and V = 16, same protocol;
and contrast and NMSE per third-octave band from the accumulated spectra (recorded, not gated).  It replaces the section "Per-bin
spectra" of the file and leaves the rest as it is.

`--detectability` runs the leg of the detectability stage (apvast(..., evaluation_detectability=True), csrc/kernels_evaldetect.hip)
beside the spectra leg of the same run: ms per hop with the spectra alone and with the detectabilities, same protocol, and the mean
detectability and audible share of hops (evaluation.detectability_metrics; recorded, not gated).  It writes
profiles/evaluation_detectability.md.

Writes profiles/stream_evaluation.md (and one JSON line per leg on stdout).  A leg that fails or overruns its time limit ends the
run.  `--bench-parent A,B,C --bench-this A,B,C` adds the ms_per_step of bench.py on the parent commit and on this one to the file.
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
CFG3 = dict(L=16, M=32, N=2048, H=1024, P=800, J=256)
PV, MV = 800, 32


def rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / 120.0)[:, None, None]
    return rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3


def validation(a0, b0):
    rng = np.random.default_rng(7)
    return tuple(r + 0.1 * np.sqrt(np.mean(r ** 2, axis=(1, 2), keepdims=True)) * rng.standard_normal(r.shape) for r in (a0, b0))


def make(synth, V, evaluate, spectra=False, detect=False):
    from ap_vast_unofficial_amd.apvast import apvast
    s = CFG3
    a0, b0 = rirs(s["P"], s["L"], s["M"], 99)
    kw = {}
    if synth in ("cwola", "fir"):
        kw.update(constrain_filter_length=True)
    if synth == "fir":
        kw.update(synthesis="fir")
    if evaluate:
        va, vb = validation(a0, b0)
        kw.update(validation_rir_A=va, validation_rir_B=vb, evaluation_ranks=[V])
    if spectra:
        kw.update(evaluation_spectra=True)
    if detect:
        kw.update(evaluation_detectability=True)
    return apvast(s["N"], a0, b0, s["J"], 20, 0, 0, V, 1.0, 4 * s["N"], hop_size=s["H"], perceptual=False, dtype="f64", seed=0, **kw)


def leg_hop(synth, V, evaluate, hops, spectra=False, detect=False):
    H = CFG3["H"]
    obj = make(synth, V, evaluate, spectra, detect)
    warm = 8
    x = np.random.default_rng(3).standard_normal((2, (warm + hops) * H))
    ts = []
    for h in range(warm + hops):
        t0 = time.perf_counter()
        obj.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts[warm:]) * 1e3
    res = dict(leg="hop", synthesis=synth, V=V, evaluation=bool(evaluate), spectra=bool(spectra), hops=hops, hop_ms_median=float(np.median(ts)),
               hop_ms_p10=float(np.percentile(ts, 10)), hop_ms_p90=float(np.percentile(ts, 90)), audio_hop_ms=H / 48.0)
    if evaluate:
        m = __import__("ap_vast_unofficial_amd.evaluation", fromlist=["metrics"]).metrics(obj.evaluation_totals())
        res.update(nmse=m["nmse"][:, 0].tolist(), contrast_db=m["contrast_db"][:, 0].tolist())
    if spectra:
        from ap_vast_unofficial_amd.evaluation import spectral_metrics, third_octave_bands
        centres, bands = third_octave_bands(48000, CFG3["N"], f_min=100.0, f_max=16000.0)
        m = spectral_metrics(obj.evaluation_spectra(), bands)
        res.update(band_hz=centres.tolist(), band_contrast_db=m["contrast_db"][:, 0].tolist(), band_nmse=m["nmse"][:, 0].tolist())
    if detect:
        from ap_vast_unofficial_amd.evaluation import detectability_metrics
        m = detectability_metrics(obj.evaluation_detectability())
        res.update(detectability=True, **{k: v[:, 0].tolist() for k, v in m.items()})
    obj.close()
    print(json.dumps(res), flush=True)


def leg_kernel(reps):
    """the pressure launch alone at the stream's sizes: 2 programs x (bright, dark of one rank + target) = 6 sets"""
    import ctypes
    from ap_vast_unofficial_amd._capi import Engine
    s = CFG3
    L, H, G = s["L"], s["H"], 6
    eng = Engine(9, 4, 4)
    rng = np.random.default_rng(1)
    dy = eng.to_device(rng.standard_normal((G, PV - 1 + H, L)))
    dr = eng.to_device(rng.standard_normal((PV, L, MV)))
    dp = eng.alloc(G * H * MV * 8)
    ms = ctypes.c_float()
    times = []
    for i in range(reps + 3):
        eng._chk(eng.lib.apv_timer_start(eng.h))
        eng._chk(eng.lib.apv_eval_pressure(eng.h, dy.ptr, dr.ptr, G, L, PV, H, MV, dp.ptr))
        eng._chk(eng.lib.apv_timer_stop(eng.h, ctypes.byref(ms)))
        if i >= 3:
            times.append(ms.value)
    flop = 2.0 * G * H * L * PV * MV
    k_ms = float(np.median(times))
    print(json.dumps(dict(leg="kernel", sets=G, H=H, L=L, Pv=PV, Mv=MV, kernel_ms=k_ms, model_gflop=flop / 1e9,
                          model_ms_at_peak=flop / (F64_MFMA_PEAK_TFLOPS * 1e12) * 1e3,
                          f64_mfma_peak_fraction=flop / (k_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS)), flush=True)
    for b in (dy, dr, dp):
        b.free()
    eng.close()


def child(args, timeout):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args,
                       stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    if r.returncode != 0:
        print(json.dumps(dict(args=args, failed=r.returncode)), flush=True)
        return None
    return json.loads(r.stdout.strip().splitlines()[-1])


def spectra_section(args):
    """the --spectra leg: evaluation alone against evaluation + spectra, alternating, fresh processes; the section's lines"""
    rows = []
    for V in (1, 16):
        for rep in range(2):
            for sp in (0, 1):
                r = child(["--leg", "hop", "--synthesis", "wola", "--V", str(V), "--evaluation", "1", "--with-spectra", str(sp),
                           "--hops", str(args.hops)], args.timeout)
                if r is None:
                    return None
                rows.append(r)
    lines = [SPECTRA_HEAD, "",
             "`tools/bench_stream_evaluation.py --spectra`: the WOLA stream above with the evaluation stage, without and with",
             f"`evaluation_spectra=True` (three more launches per hop); {args.hops} timed hops per leg after 8 warm-up hops, every leg a",
             "fresh process, without / with alternating.  ms per hop of `process_input_buffers` (median; p10 .. p90):", "",
             "| V | spectra | run 1 | run 2 |", "|---|---|---|---|"]
    for V in (1, 16):
        for sp in (False, True):
            q = [r for r in rows if r["V"] == V and r["spectra"] == sp]
            cells = " | ".join(f"{r['hop_ms_median']:.3f} ({r['hop_ms_p10']:.3f} .. {r['hop_ms_p90']:.3f})" for r in q)
            lines.append(f"| {V} | {'on' if sp else 'off'} | {cells} |")
    for V in (1, 16):
        off = np.median([r["hop_ms_median"] for r in rows if r["V"] == V and not r["spectra"]])
        on = np.median([r["hop_ms_median"] for r in rows if r["V"] == V and r["spectra"]])
        lines.append("")
        lines.append(f"V = {V}: {on - off:+.3f} ms per hop for the spectra (median of the runs with, less median of the runs without).")
    q = [r for r in rows if r["V"] == 16 and r["spectra"]][0]
    lines += ["", "Contrast and NMSE per third-octave band (`evaluation.third_octave_bands(48000, 2048, 100, 16000)` into",
              "`evaluation.spectral_metrics`), V = 16, rank 16, totals over all hops of the leg; recorded, not gated.  Per zone",
              "program [A, B].", "", "| band (Hz) | contrast_db | nmse |", "|---|---|---|"]
    for i, fc in enumerate(q["band_hz"]):
        lines.append(f"| {fc:.0f} | {', '.join('%.2f' % z[i] for z in q['band_contrast_db'])} | "
                     f"{', '.join('%.4f' % z[i] for z in q['band_nmse'])} |")
    return lines


SPECTRA_HEAD = "## Per-bin spectra"


def detectability_file(args):
    """the --detectability leg: evaluation + spectra against evaluation + spectra + detectabilities, alternating, fresh processes;
    the lines of profiles/evaluation_detectability.md"""
    rows = []
    for V in (1, 16):
        for rep in range(2):
            for dt in (0, 1):
                r = child(["--leg", "hop", "--synthesis", "wola", "--V", str(V), "--evaluation", "1", "--with-spectra", "1",
                           "--with-detectability", str(dt), "--hops", str(args.hops)], args.timeout)
                if r is None:
                    return None
                rows.append(r)
    on_of = lambda r: bool(r.get("detectability"))
    lines = ["# Detectability stage of the subband stream: cost and first results", "",
             "Written by `tools/bench_stream_evaluation.py --detectability` on an MI355X.  cfg3's shape (16 loudspeakers x 32 control",
             f"microphones, N 2048, H 1024, 800-tap responses, float64, both zone programs), Pv = {PV}, Mv = {MV},",
             "`evaluation_ranks=[V]`, `evaluation_spectra=True`, without and with `evaluation_detectability=True` (three more launches per",
             f"hop); {args.hops} timed hops per leg after 8 warm-up hops, every leg a fresh process, without / with alternating.  A hop of",
             "audio at 48 kHz lasts 21.33 ms.", "",
             "## ms per hop of `process_input_buffers` (median; p10 .. p90)", "",
             "| V | detectability | run 1 | run 2 |", "|---|---|---|---|"]
    for V in (1, 16):
        for dt in (False, True):
            q = [r for r in rows if r["V"] == V and on_of(r) == dt]
            cells = " | ".join(f"{r['hop_ms_median']:.3f} ({r['hop_ms_p10']:.3f} .. {r['hop_ms_p90']:.3f})" for r in q)
            lines.append(f"| {V} | {'on' if dt else 'off'} | {cells} |")
    for V in (1, 16):
        off = np.median([r["hop_ms_median"] for r in rows if r["V"] == V and not on_of(r)])
        on = np.median([r["hop_ms_median"] for r in rows if r["V"] == V and on_of(r)])
        lines.append("")
        lines.append(f"V = {V}: {on - off:+.3f} ms per hop for the detectabilities (median of the runs with, less median of the runs without).")
    lines += ["", "## Mean detectability and audible share of hops (recorded, not gated)", "",
              "`evaluation.detectability_metrics` on the totals over all hops of the leg (warm-up included), white-noise inputs at full",
              "scale; D = 1 is just audible.  Per zone program [A, B].", "",
              "| V | error_mean | error_audible_share | leak_mean | leak_audible_share |", "|---|---|---|---|---|"]
    for V in (1, 16):
        q = [r for r in rows if r["V"] == V and on_of(r)][0]
        f = lambda k: ", ".join("%.4g" % v for v in q[k])
        lines.append(f"| {V} | {f('error_mean')} | {f('error_audible_share')} | {f('leak_mean')} | {f('leak_audible_share')} |")
    if args.bench_parent or args.bench_this:
        f = lambda s: [float(v) for v in s.split(",") if v]
        p, t = f(args.bench_parent), f(args.bench_this)
        lines += ["", "## bench.py --gpus 1 --steps 200 --warmup 20, parent commit and this one, alternating", "",
                  f"* parent: ms_per_step {', '.join('%.4f' % v for v in p)} (range {min(p):.4f} .. {max(p):.4f})",
                  f"* this commit: ms_per_step {', '.join('%.4f' % v for v in t)} (range {min(t):.4f} .. {max(t):.4f})",
                  "", "The default stream launches nothing new: the stage is behind `ed_on`, which only the keyword sets."]
    return lines


def replace_section(text, head, lines):
    """`text` with the section that starts at the line `head` (up to the next '## ' line or the end) replaced by `lines`"""
    old = text.split("\n")
    out, skip = [], False
    for ln in old:
        if ln == head:
            skip = True
            continue
        if skip and ln.startswith("## "):
            skip = False
        if not skip:
            out.append(ln)
    while out and out[-1] == "":
        out.pop()
    return "\n".join(out + [""] + lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("hop", "kernel"))
    ap.add_argument("--synthesis", default="wola")
    ap.add_argument("--V", type=int, default=16)
    ap.add_argument("--evaluation", type=int, default=0)
    ap.add_argument("--hops", type=int, default=100)
    ap.add_argument("--with-spectra", type=int, default=0, help="a hop leg with evaluation_spectra=True")
    ap.add_argument("--with-detectability", type=int, default=0, help="a hop leg with evaluation_detectability=True")
    ap.add_argument("--detectability", action="store_true",
                    help="run the detectability leg and write profiles/evaluation_detectability.md")
    ap.add_argument("--spectra", action="store_true", help="run the per-bin spectra leg and replace its section of the file")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per leg")
    ap.add_argument("--bench-parent", default="", help="ms_per_step of bench.py on the parent commit, comma separated")
    ap.add_argument("--bench-this", default="", help="... and on this commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_evaluation.md"))
    args = ap.parse_args()
    if args.leg == "hop":
        leg_hop(args.synthesis, args.V, args.evaluation, args.hops, bool(args.with_spectra), bool(args.with_detectability))
        return 0
    if args.leg == "kernel":
        leg_kernel(20)
        return 0
    if args.detectability:
        lines = detectability_file(args)
        if lines is None:
            return 1
        out = os.path.join(os.path.dirname(args.out), "evaluation_detectability.md")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return 0
    if args.spectra:
        lines = spectra_section(args)
        if lines is None:
            return 1
        text = open(args.out).read() if os.path.exists(args.out) else ""
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(replace_section(text, SPECTRA_HEAD, lines))
        return 0
    rows, metrics = [], []
    for synth in ("wola", "fir"):
        for V in (1, 16):
            for rep in range(2):
                for ev in (0, 1):
                    r = child(["--leg", "hop", "--synthesis", synth, "--V", str(V), "--evaluation", str(ev), "--hops", str(args.hops)],
                              args.timeout)
                    if r is None:
                        return 1
                    rows.append(r)
    r = child(["--leg", "hop", "--synthesis", "cwola", "--V", "16", "--evaluation", "1", "--hops", str(args.hops)], args.timeout)
    if r is None:
        return 1
    metrics = [q for q in rows if q["evaluation"] and q["V"] == 16 and q["synthesis"] == "wola"][:1] + [r] + \
              [q for q in rows if q["evaluation"] and q["V"] == 16 and q["synthesis"] == "fir"][:1]
    k = child(["--leg", "kernel"], args.timeout)
    if k is None:
        return 1
    lines = ["# Evaluation stage of the subband stream: cost and first results", "",
             "Written by `tools/bench_stream_evaluation.py` on an MI355X.  cfg3's shape (16 loudspeakers x 32 control microphones,",
             f"N 2048, H 1024, 800-tap responses, float64, both zone programs), Pv = {PV}, Mv = {MV}, `evaluation_ranks=[V]`;",
             f"{args.hops} timed hops per leg after 8 warm-up hops, every leg a fresh process, off / on alternating.  A hop of audio at",
             "48 kHz lasts 21.33 ms.", "",
             "## ms per hop of `process_input_buffers` (median; p10 .. p90)", "",
             "| synthesis | V | evaluation | run 1 | run 2 |", "|---|---|---|---|---|"]
    for synth in ("wola", "fir"):
        for V in (1, 16):
            for ev in (False, True):
                q = [r for r in rows if r["synthesis"] == synth and r["V"] == V and r["evaluation"] == ev]
                cells = " | ".join(f"{r['hop_ms_median']:.3f} ({r['hop_ms_p10']:.3f} .. {r['hop_ms_p90']:.3f})" for r in q)
                lines.append(f"| {synth} | {V} | {'on' if ev else 'off'} | {cells} |")
    lines += ["", "## The pressure launch against the model", "",
              f"`apv_eval_pressure` alone on device buffers of the stream's sizes ({k['sets']} pressure sets: two programs x bright, dark,",
              "target), HIP events around the launch, median of 20:", "",
              f"* launch: {k['kernel_ms']:.4f} ms; model 2 sets H L Pv Mv = {k['model_gflop']:.2f} Gflop = {k['model_ms_at_peak']:.4f} ms at the",
              f"  float64 matrix peak ({F64_MFMA_PEAK_TFLOPS} Tflop/s): {100 * k['f64_mfma_peak_fraction']:.1f} % of the peak",
              ]
    on = [r["hop_ms_median"] for r in rows if r["evaluation"] and r["synthesis"] == "wola" and r["V"] == 16]
    if on:
        lines.append(f"* share of the evaluated WOLA hop at V = 16: {100 * k['kernel_ms'] / np.median(on):.1f} %")
    lines += ["", "## contrast_db and nmse on the same signal (recorded, not gated)", "",
              "V = 16, rank 16 evaluated, totals over all hops of the leg (warm-up included); validation responses = control responses",
              "+ 10 % independent noise per tap.  Per zone program [A, B].", "",
              "| stream | contrast_db | nmse |", "|---|---|---|"]
    for name, q in zip(("WOLA", "constrained WOLA (J = 256)", "FIR (J = 256)"), metrics):
        lines.append(f"| {name} | {', '.join('%.2f' % v for v in q['contrast_db'])} | {', '.join('%.4f' % v for v in q['nmse'])} |")
    if args.bench_parent or args.bench_this:
        f = lambda s: [float(v) for v in s.split(",") if v]
        p, t = f(args.bench_parent), f(args.bench_this)
        lines += ["", "## bench.py --gpus 1 --steps 200 --warmup 20, parent commit and this one, alternating", "",
                  f"* parent: ms_per_step {', '.join('%.4f' % v for v in p)} (range {min(p):.4f} .. {max(p):.4f})",
                  f"* this commit: ms_per_step {', '.join('%.4f' % v for v in t)} (range {min(t):.4f} .. {max(t):.4f})",
                  "", "The default stream launches nothing new: the evaluation stage is behind `ev_on`, which only the keywords set."]
    # the section of the --spectra leg, if the file has one, stays
    kept = []
    if os.path.exists(args.out):
        for ln in open(args.out).read().split("\n"):
            if ln == SPECTRA_HEAD or (kept and not ln.startswith("## ")):
                kept.append(ln)
            elif kept:
                break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines + ([""] + kept if kept else [])).rstrip("\n") + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

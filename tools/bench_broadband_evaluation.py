#!/usr/bin/env python3
"""Cost and first results of the broadband stream's evaluation stage (apvast.enable_evaluation, csrc/kernels_bbeval.hip).

At the two shapes of tools/bench_broadband.py -- cfg1 (bundled 8 x 8 responses, N 256, H 128, J 32, V 8) and the reference's test
parameters (N 1600, H 800, J 100, V 50) -- with the control responses plus 10 % independent noise as validation responses and the
largest rank evaluated:

  * ms per hop of process_input_buffers (median) and of process_signal (one call, after a call that sized the buffers), with the
    stage off and on -- every leg a fresh child process, two runs per leg, alternating (off, on, off, on);
  * the time of ONE per-hop evaluation on device buffers of the stream's sizes -- apv_eval_pressure + apv_eval_energies, HIP
    events around a loop of them -- next to the time per hop the stage adds to process_signal, where one launch of each covers a
    group of hops;
  * NMSE and contrast (evaluation.metrics on the totals) of the signal the whole-signal leg ran: recorded, not gated.

Writes profiles/broadband_evaluation.md (and one JSON line per leg on stdout).  A leg that fails or overruns its time limit ends
the run.

--spectra: the per-bin spectra on top of the stage (apvast.enable_evaluation_spectra, csrc/kernels_bbevalspec.hip) instead: the same
two timings with the stage on against the stage on plus the spectra (on, spectra, on, spectra), at the reference's test
parameters one more pair with all 50 ranks evaluated -- a hop's spectra are 20.7 MB there, so a group of 16 runs as sub-launches
of three hops -- and contrast and NMSE per third-octave band at 48 kHz (recorded, not gated).  Replaces the section "Per-bin
spectra" of the same file.

--detectability: the perceptual detectability on top of the spectra (apvast.enable_evaluation_detectability, the hop-batched
launches of csrc/kernels_evaldetect.hip): the same two timings with stage + spectra against stage + spectra + detectability
(spectra, detectability, spectra, detectability), and the mean detectability per hop and the audible share of hops of error and
leak (evaluation.detectability_metrics; recorded, not gated).  Replaces the section "Detectability" at the end of the same
file."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "cfg1": dict(N=256, J=32, delay=16, ref=0, V=8, S=512, H=128, hops=64, signal_hops=128,
                 label="cfg1: 8 x 8, N 256, H 128, J 32 (n = 256), S 512, V 8"),
    "reftest": dict(N=1600, J=100, delay=20, ref=6, V=50, S=1000, H=800, hops=12, signal_hops=32,
                    label="make_python_test.m: 8 x 8, N 1600, H 800, J 100 (n = 800), S 1000, V 50"),
}


def responses():
    g = np.load(os.path.join(ROOT, "tests", "golden", "rirs_cfg1.npz"))
    return g["rirA"], g["rirB"]


def validation(a0, b0):
    rng = np.random.default_rng(7)
    return tuple(r + 0.1 * np.sqrt(np.mean(r ** 2, axis=(1, 2), keepdims=True)) * rng.standard_normal(r.shape) for r in (a0, b0))


def make(shape, stage, all_ranks=False):
    """stage 0: off; 1: the evaluation stage; 2: the stage and its per-bin spectra; 3: those and the detectability"""
    from ap_vast_unofficial_amd.apvast import apvast
    s = SHAPES[shape]
    a0, b0 = responses()
    ap = apvast(s["N"], a0, b0, s["J"], s["delay"], s["ref"], s["ref"], s["V"], 1.0, s["S"], hop_size=s["H"], perceptual=False,
                mode="broadband", seed=0)
    if stage:
        va, vb = validation(a0, b0)
        ap.enable_evaluation(va, vb, None if all_ranks else [s["V"]])
    if stage >= 2:
        ap.enable_evaluation_spectra()
    if stage == 3:
        ap.enable_evaluation_detectability()
    return ap


def leg_stream(shape, stage, all_ranks=False):
    s = SHAPES[shape]
    H, hops, nsig = s["H"], s["hops"], s["signal_hops"]
    ap = make(shape, stage, all_ranks)
    x = np.random.default_rng(7).standard_normal((2, (hops + 2) * H))
    times = []
    for h in range(hops + 2):
        t0 = time.perf_counter()
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        times.append(time.perf_counter() - t0)
    xs = np.random.default_rng(8).standard_normal((2, nsig * H))
    out = ap.alloc_signal_output(nsig * H)
    ap.process_signal(xs[0], xs[1], out=out)                 # sizes the group buffers
    if stage:
        ap.reset_evaluation()
    t0 = time.perf_counter()
    ap.process_signal(xs[0], xs[1], out=out)
    sig = (time.perf_counter() - t0) / nsig
    r = {"shape": shape, "stage": int(stage), "all_ranks": bool(all_ranks), "ms_per_hop": float(np.median(times[2:])) * 1e3, "ms_per_hop_process_signal": sig * 1e3,
         "hops": hops, "signal_hops": nsig}
    if stage:
        from ap_vast_unofficial_amd.evaluation import metrics
        m = metrics(ap.evaluation_totals())
        r.update(nmse=m["nmse"][:, -1].tolist(), contrast_db=m["contrast_db"][:, -1].tolist(), Pv=int(ap._eval_dims()[2]),
                 Mv=int(ap._eval_dims()[3]), E=int(ap._eval_dims()[1]))
    if stage == 3:
        from ap_vast_unofficial_amd.evaluation import detectability_metrics
        d = detectability_metrics(ap.evaluation_detectability())
        r.update(detect_hops=int(ap.evaluation_detectability()["hops"]), n_channels=int(ap.detectability_model.n_channels),
                 **{k: v[:, -1].tolist() for k, v in d.items()})
    if stage == 2:
        from ap_vast_unofficial_amd.evaluation import spectral_metrics, third_octave_bands
        centres, bands = third_octave_bands(48000, s["N"], f_min=100.0, f_max=16000.0)
        b = spectral_metrics(ap.evaluation_spectra(), bands)
        r.update(band_hz=centres.tolist(), band_contrast_db=b["contrast_db"][:, -1].tolist(), band_nmse=b["nmse"][:, -1].tolist())
    ap.close()
    return r


def leg_kernels(shape, reps=200):
    """one per-hop evaluation on device buffers: the stream's 2 (2 E + 1) = 6 pressure sets of H samples, then their energies"""
    from ap_vast_unofficial_amd import _capi
    s = SHAPES[shape]
    a0, _ = responses()
    Pv, L, Mv = a0.shape
    H, Z, E = s["H"], 2, 1
    sets = Z * (2 * E + 1)
    eng = _capi.Engine(9, L, 4)
    rng = np.random.default_rng(5)
    dy = eng.to_device(rng.standard_normal((sets, Pv - 1 + H, L)))
    dr = eng.to_device(np.ascontiguousarray(a0, dtype=np.float64))
    dp, drec, dtot = eng.alloc(sets * H * Mv * 8), eng.to_device(np.zeros(Z * (3 * E + 1) * Mv)), eng.to_device(np.zeros(Z * (3 * E + 1) * Mv))
    out = {}
    for what in ("pressure", "energies", "both"):
        def once():
            if what != "energies":
                eng._chk(eng.lib.apv_eval_pressure(eng.h, dy.ptr, dr.ptr, sets, L, Pv, H, Mv, dp.ptr))
            if what != "pressure":
                eng._chk(eng.lib.apv_eval_energies(eng.h, dp.ptr, Z, E, H, Mv, 1, drec.ptr, dtot.ptr))
        for _ in range(10):
            once()
        eng.sync()
        eng.timer_start()
        for _ in range(reps):
            once()
        out[what] = eng.timer_stop() / reps
    eng.close()
    return {"shape": shape, "kernels_ms": out, "Pv": int(Pv), "Mv": int(Mv), "sets": sets, "reps": reps}


def child(args, limit):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"leg {args} failed with status {p.returncode}")
    line = [q for q in p.stdout.splitlines() if q.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def rng_of(v):
    return f"{min(v):.3f} .. {max(v):.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["stream", "kernels"])
    ap.add_argument("--shape", choices=list(SHAPES))
    ap.add_argument("--stage", type=int, default=0,
                    help="0: off, 1: the evaluation stage, 2: the stage and its per-bin spectra, 3: those and the detectability")
    ap.add_argument("--all-ranks", action="store_true", help="evaluate every rank instead of the largest")
    ap.add_argument("--spectra", action="store_true", help="the legs of the per-bin spectra (see the module docstring)")
    ap.add_argument("--detectability", action="store_true", help="the legs of the detectability (see the module docstring)")
    ap.add_argument("--shapes", default="cfg1,reftest")
    ap.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "broadband_evaluation.md"))
    a = ap.parse_args()
    if a.leg == "stream":
        print(json.dumps(leg_stream(a.shape, a.stage, a.all_ranks)))
        return
    if a.leg == "kernels":
        print(json.dumps(leg_kernels(a.shape)))
        return
    if a.spectra:
        return main_spectra(a)
    if a.detectability:
        return main_detectability(a)
    lines = ["# Broadband stream: evaluation stage (`apvast.enable_evaluation`)", "",
             "Written by `tools/bench_broadband_evaluation.py`; every leg a fresh process, two runs per leg, alternating (off, on, off, on).",
             "Validation responses: the control responses plus 10 % independent noise; the largest rank evaluated (E = 1, both zone",
             "programs: 6 pressure sets).  Times in ms per hop; `process_signal` is one call over the given number of hops into a",
             "page-locked result array, after a call that sized the buffers.", ""]
    for shape in a.shapes.split(","):
        s = SHAPES[shape]
        runs = {0: [], 1: []}
        for _ in range(2):
            for stage in (0, 1):
                runs[stage].append(child(["--leg", "stream", "--shape", shape, "--stage", str(stage)], a.limit))
        k = child(["--leg", "kernels", "--shape", shape], a.limit)
        off, on = runs[0], runs[1]
        hop = [[r["ms_per_hop"] for r in q] for q in (off, on)]
        sig = [[r["ms_per_hop_process_signal"] for r in q] for q in (off, on)]
        added_hop = np.mean(hop[1]) - np.mean(hop[0])
        added_sig = np.mean(sig[1]) - np.mean(sig[0])
        km = k["kernels_ms"]
        lines += [f"## {s['label']}", "",
                  f"Pv = {on[0]['Pv']} validation taps, Mv = {on[0]['Mv']} validation microphones; {s['hops']} per-hop calls (median), "
                  f"`process_signal` over {s['signal_hops']} hops.", "",
                  "| | stage off (two runs) | stage on (two runs) | added, mean |", "|---|---|---|---|",
                  f"| `process_input_buffers` | {rng_of(hop[0])} | {rng_of(hop[1])} | {added_hop:+.3f} |",
                  f"| `process_signal` | {rng_of(sig[0])} | {rng_of(sig[1])} | {added_sig:+.3f} |", "",
                  f"One per-hop evaluation on device buffers of these sizes, HIP events around {k['reps']} of them: pressure launch "
                  f"{km['pressure']:.4f} ms, energies and totals {km['energies']:.4f} ms, both {km['both']:.4f} ms -- against "
                  f"{added_sig:+.4f} ms per hop that the stage adds to `process_signal`, where three launches cover a group of 16 hops.", "",
                  f"NMSE per zone program (A, B) at rank {s['V']}: {', '.join(f'{v:.4f}' for v in on[0]['nmse'])}; contrast "
                  f"{', '.join(f'{v:.2f}' for v in on[0]['contrast_db'])} dB (recorded, not gated).", ""]
    path = a.out
    tail = ""
    if os.path.exists(path):
        old = open(path).read()
        mark = "\n## Notes"
        if mark in old:
            tail = old[old.index(mark):]
    with open(path, "w") as f:
        f.write("\n".join(lines) + tail)
    print("wrote", path)


SPECTRA_MARK = "\n# Per-bin spectra"


def main_spectra(a):
    lines = [SPECTRA_MARK.strip("\n") + " (`apvast.enable_evaluation_spectra`)", "",
             "Written by `tools/bench_broadband_evaluation.py --spectra`; every leg a fresh process, two runs per leg, alternating (stage,",
             "stage + spectra, stage, stage + spectra).  Same validation responses and calls as above.  Times in ms per hop.", ""]
    for shape in a.shapes.split(","):
        s = SHAPES[shape]
        runs = {1: [], 2: []}
        for _ in range(2):
            for stage in (1, 2):
                runs[stage].append(child(["--leg", "stream", "--shape", shape, "--stage", str(stage)], a.limit))
        on, sp = runs[1], runs[2]
        hop = [[r["ms_per_hop"] for r in q] for q in (on, sp)]
        sig = [[r["ms_per_hop_process_signal"] for r in q] for q in (on, sp)]
        lines += [f"## {s['label']}", "",
                  f"The largest rank evaluated (6 pressure sets x {sp[0]['Mv']} microphones = {6 * sp[0]['Mv']} transforms of N = {s['N']} per hop); "
                  f"{s['hops']} per-hop calls (median), `process_signal` over {s['signal_hops']} hops.", "",
                  "| | stage on (two runs) | stage + spectra (two runs) | added, mean |", "|---|---|---|---|",
                  f"| `process_input_buffers` | {rng_of(hop[0])} | {rng_of(hop[1])} | {np.mean(hop[1]) - np.mean(hop[0]):+.3f} |",
                  f"| `process_signal` | {rng_of(sig[0])} | {rng_of(sig[1])} | {np.mean(sig[1]) - np.mean(sig[0]):+.3f} |", ""]
        if shape == "reftest":
            full = [child(["--leg", "stream", "--shape", shape, "--stage", str(stage), "--all-ranks"], a.limit) for stage in (1, 2)]
            ch = 2 * (2 * full[1]["E"] + 1) * full[1]["Mv"]
            mb = ch * (s["N"] // 2 + 1) * 16 / 1e6
            lines += [f"All {full[1]['E']} ranks evaluated ({ch} transforms and {mb:.1f} MB of spectra per hop: sub-launches of "
                      f"{max(int(64 * 2 ** 20 / (mb * 1e6)), 1)} hops under the 64 MB budget), one run each, stage / stage + spectra: "
                      f"`process_input_buffers` {full[0]['ms_per_hop']:.3f} / {full[1]['ms_per_hop']:.3f}, `process_signal` "
                      f"{full[0]['ms_per_hop_process_signal']:.3f} / {full[1]['ms_per_hop_process_signal']:.3f}.", ""]
        r = sp[0]
        lines += [f"Contrast and NMSE per third-octave band (`evaluation.third_octave_bands(48000, {s['N']}, 100, 16000)` into "
                  f"`evaluation.spectral_metrics`), rank {s['V']}, totals over the {s['signal_hops']} hops of the `process_signal` leg; "
                  "recorded, not gated.  Per zone program [A, B].", "", "| band (Hz) | contrast_db | nmse |", "|---|---|---|"]
        for i, fc in enumerate(r["band_hz"]):
            lines.append(f"| {fc:.0f} | " + ", ".join(f"{z[i]:.2f}" for z in r["band_contrast_db"]) + " | "
                         + ", ".join(f"{z[i]:.4f}" for z in r["band_nmse"]) + " |")
        lines += ["", f"Broadband, from the energies of the same leg: contrast {', '.join(f'{v:.2f}' for v in r['contrast_db'])} dB, NMSE "
                  f"{', '.join(f'{v:.4f}' for v in r['nmse'])}.", ""]
    old = open(a.out).read() if os.path.exists(a.out) else ""
    notes = after = ""
    if DETECT_MARK in old:                                   # the section behind this one stays
        after = "\n" + old[old.index(DETECT_MARK):]
        old = old[:old.index(DETECT_MARK)]
    if SPECTRA_MARK in old:
        block = old[old.index(SPECTRA_MARK):]
        old = old[:old.index(SPECTRA_MARK)]
        mark = "\n## Notes on the spectra"
        if mark in block:
            notes = block[block.index(mark):]
    with open(a.out, "w") as f:
        f.write(old.rstrip("\n") + "\n\n" + "\n".join(lines) + notes.rstrip("\n") + "\n" + after)
    print("wrote", a.out)


DETECT_MARK = "\n# Detectability"


def main_detectability(a):
    lines = [DETECT_MARK.strip("\n") + " (`apvast.enable_evaluation_detectability`)", "",
             "Written by `tools/bench_broadband_evaluation.py --detectability`; every leg a fresh process, two runs per leg, alternating",
             "(stage + spectra, stage + spectra + detectability, and again).  Same validation responses and calls as above; the model's",
             "tables are `PerceptualTables(N, 48000, 94)`.  Times in ms per hop.", ""]
    for shape in a.shapes.split(","):
        s = SHAPES[shape]
        runs = {2: [], 3: []}
        for _ in range(2):
            for stage in (2, 3):
                runs[stage].append(child(["--leg", "stream", "--shape", shape, "--stage", str(stage)], a.limit))
        sp, de = runs[2], runs[3]
        hop = [[r["ms_per_hop"] for r in q] for q in (sp, de)]
        sig = [[r["ms_per_hop_process_signal"] for r in q] for q in (sp, de)]
        r = de[0]
        fmt = lambda v, f: ", ".join(format(x, f) for x in v)
        lines += [f"## {s['label']}", "",
                  f"The largest rank evaluated (2 programs x {r['Mv']} microphones = {2 * r['Mv']} curves of K = {s['N'] // 2 + 1} bins and "
                  f"{r['n_channels']} channels per hop, {4 * r['Mv']} weighted sums); {s['hops']} per-hop calls (median), `process_signal` "
                  f"over {s['signal_hops']} hops.", "",
                  "| | stage + spectra (two runs) | + detectability (two runs) | added, mean |", "|---|---|---|---|",
                  f"| `process_input_buffers` | {rng_of(hop[0])} | {rng_of(hop[1])} | {np.mean(hop[1]) - np.mean(hop[0]):+.3f} |",
                  f"| `process_signal` | {rng_of(sig[0])} | {rng_of(sig[1])} | {np.mean(sig[1]) - np.mean(sig[0]):+.3f} |", "",
                  f"Detectability at rank {s['V']} over the {r['detect_hops']} hops of the `process_signal` leg, per zone program [A, B], mean "
                  f"over the microphones (D = 1: just audible; recorded, not gated): `error_mean` {fmt(r['error_mean'], '.4g')}, `leak_mean` "
                  f"{fmt(r['leak_mean'], '.4g')}; audible share of hops: error {fmt(r['error_audible_share'], '.3f')}, leak "
                  f"{fmt(r['leak_audible_share'], '.3f')}.", ""]
    old = open(a.out).read() if os.path.exists(a.out) else ""
    notes = ""
    if DETECT_MARK in old:
        block = old[old.index(DETECT_MARK):]
        old = old[:old.index(DETECT_MARK)]
        mark = "\n## Notes on the detectability"
        if mark in block:
            notes = block[block.index(mark):]
    with open(a.out, "w") as f:
        f.write(old.rstrip("\n") + "\n\n" + "\n".join(lines) + notes)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

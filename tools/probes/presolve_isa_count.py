#!/usr/bin/env python3
"""Static instruction counts of the float32 pre-solve (tridiag_presolve16) in the product instantiation of the order-16 float64
kernel, gevd16m_kernel_f64<true, float2, false>.  Compiles kernels_gevd16m.hip to gfx950 assembly with hipcc (no GPU needed)
and splits the common path of the function into the regions of DESIGN 4.1:

  Householder reduction       from the first v_sqrt_f32 / v_rsq_f32 after the last f64 MFMA in front of the Sturm loop
                              (the scalar chain of reflector 0) to the wide step
  wide multisection step      from the first of the last 15 v_rcp_f32 in front of the Sturm loop (the recurrence of the
                              wave-wide first step, straight-line code) to the head of the loop: the recurrence, the sixteen
                              votes and v_writelane_b32, the interval update (the scheduler moves a few instructions of the
                              reduction's end in here and the step's point out: the split is good to about five)
  quad steps                  the body of the one loop that holds the 15 v_rcp_f32 of the recurrence, times its 6 steps
  inverse iteration, gate, QX from the loop's end to the last v_mfma_f32

and prints VGPRs, spills, scratch, LDS and, per region, the VALU count (every v_* but the MFMAs), s_nop, other SALU, ds_bpermute
and MFMA counts, and the commonest VALU mnemonics of the reduction.

    python tools/probes/presolve_isa_count.py [--asm FILE.s] [--top N]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "kernels_gevd16m.hip")
KERNEL = "gevd16m_kernel_f64ILb1E15HIP_vector_typeIfLj2EELb0EE"      # <true, float2, false>
STEPS = 6                                                               # kTpQuadSteps


def compile_asm(path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I/opt/rocm/include", "-S", "--cuda-device-only",
                    SRC, "-o", path], check=True, stderr=subprocess.DEVNULL)


def function_lines(text):
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and KERNEL in l.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for l in lines[end:end + 80]:
        m = re.match(r";\s*(NumVgprs|ScratchSize|LDSByteSize|Occupancy):\s*(\d+)", l)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    return lines[start + 1:end], meta


def mnemonic(line):
    s = line.strip()
    if not s or s.startswith((";", ".", "/")) or re.match(r"[\w.$]+:", s):
        return None
    return s.split()[0]


def classify(ms):
    c = collections.Counter()
    for m in ms:
        if m.startswith("v_mfma"):
            c["mfma"] += 1
        elif m.startswith("v_"):
            c["valu"] += 1
        elif m == "s_nop":
            c["s_nop"] += 1
        elif m.startswith("s_") and not m.startswith(("s_waitcnt", "s_cbranch", "s_branch", "s_barrier")):
            c["salu"] += 1
        elif m.startswith("ds_bpermute"):
            c["ds_bpermute"] += 1
        elif m.startswith("ds_"):
            c["ds_other"] += 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="count an assembly file made earlier instead of compiling")
    ap.add_argument("--top", type=int, default=14)
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            compile_asm(os.path.join(td, "k.s"))
            text = open(os.path.join(td, "k.s")).read()
    body, meta = function_lines(text)
    spills = sum(1 for l in body if "Folded Spill" in l or "Spill" in l and "scratch_store" in l)
    reloads = sum(1 for l in body if "Reload" in l)
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l.strip())] if m}
    # the Sturm loop: a backward branch whose body holds the recurrence's 15 v_rcp_f32 and no MFMA
    loop = None
    for i, l in enumerate(body):
        m = re.match(r"\s*s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), len(body)) < i:
            seg = [mnemonic(x) for x in body[labels[m.group(1)]:i + 1]]
            seg = [x for x in seg if x]
            if sum(x == "v_rcp_f32_e32" or x.startswith("v_rcp_f32") for x in seg) >= 15 and not any(x.startswith("v_mfma") for x in seg):
                loop = (labels[m.group(1)], i + 1)
                break
    if loop is None:
        sys.exit("Sturm loop not found")
    last_f64 = max(i for i in range(loop[0]) if body[i].strip().startswith("v_mfma_f64"))
    red0 = next(i for i in range(last_f64, loop[0]) if body[i].strip().startswith(("v_sqrt_f32", "v_rsq_f32")))
    last_f32 = max(i for i, l in enumerate(body) if l.strip().startswith("v_mfma_f32"))
    rcps = [i for i in range(red0, loop[0]) if body[i].strip().startswith("v_rcp_f32")]
    wide0 = rcps[-15]
    regions = [("Householder reduction", body[red0:wide0], 1), ("wide multisection step", body[wide0:loop[0]], 1),
               (f"quad steps, loop body x {STEPS}", body[loop[0]:loop[1]], STEPS),
               ("inverse iteration, gate, Q X", body[loop[1]:last_f32 + 1], 1)]
    print(f"gevd16m_kernel_f64<true, float2, false>: {meta.get('NumVgprs')} VGPRs, {spills} spill stores / {reloads} reloads, "
          f"{meta.get('ScratchSize')} B scratch, {meta.get('LDSByteSize')} B LDS")
    print("\n| region (static, common path) | VALU | s_nop | SALU | ds_bpermute | other ds | MFMA |\n|---|---|---|---|---|---|---|")
    total = 0
    for name, seg, mult in regions:
        c = classify([x for x in map(mnemonic, seg) if x])
        total += c["valu"] * mult
        f = (lambda v: f"{v} x {mult}") if mult > 1 else str
        print(f"| {name} | {f(c['valu'])} | {f(c['s_nop'])} | {f(c['salu'])} | {c['ds_bpermute']} | {c['ds_other']} | {c['mfma']} |")
    print(f"| together | {total} | | | | | |")
    top = collections.Counter(re.sub(r"_e(32|64)$", "", x) for x in map(mnemonic, regions[0][1]) if x and x.startswith("v_"))
    print("\nreduction, VALU by mnemonic: " + ", ".join(f"{k} {v}" for k, v in top.most_common(args.top)))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Static instruction counts of the whole product instantiation of the order-16 float64 kernel, gevd16m_kernel_f64<true, float2,
false>: every path of the function, the rare ones (double sweeps, second refinement step, failed pivot) included, so the figures
are larger than what a wave issues.  Compiles kernels_gevd16m.hip to gfx950 assembly with hipcc (no GPU needed) and prints one
table row in the form of DESIGN 4.1:

  VALU          every v_* but the MFMAs            SALU        every s_* but waits, nops, branches and barriers
  branches      s_branch and s_cbranch_*           LDS         every ds_* (ds_bpermute included)
  waits/nops    s_waitcnt* and s_nop               MFMA        v_mfma_*
  ds_bpermute   the crossbar trips among the LDS instructions (ds_bpermute_b32; a __shfl_xor of a double is two)

with the register count, spill stores and reloads, scratch and LDS bytes from the function's own footer.  Instructions are
classed by the prefix of their mnemonic only.  (The regions of the float32 pre-solve: presolve_isa_count.py.)

Below the table: the slab loops of stage 0 (every loop of the function that holds both global loads and MFMAs), one line each with
its global loads, its full waits `s_waitcnt vmcnt(0)` and the loads issued before the first wait of any kind.  A loop that selects
or masks (v_cndmask, s_and_saveexec) is a ragged-M loop, (M & 31) != 0; it should read like the full loops: 16 loads (X_B and d) or
8 (X_D) ahead of the first wait and one full wait.  With every load under its own predicate it reads 24 loads, 24 full waits.

    python tools/probes/gevd16m_isa_count.py [--asm FILE.s] [--kernel MANGLED_SUBSTRING] [--label NAME] [--top N]
"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "kernels_gevd16m.hip")
KERNEL = "gevd16m_kernel_f64ILb1E15HIP_vector_typeIfLj2EELb0EE"      # <true, float2, false>


def compile_asm(path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I/opt/rocm/include", "-S", "--cuda-device-only",
                    SRC, "-o", path], check=True, stderr=subprocess.DEVNULL)


def function_lines(text, kernel):
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and kernel in l.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for l in lines[end:end + 80]:
        m = re.match(r";\s*(NumVgprs|NumSgprs|ScratchSize|LDSByteSize|Occupancy):\s*(\d+)", l)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    return lines[start + 1:end], meta


def mnemonic(line):
    s = line.strip()
    if not s or s.startswith((";", ".", "/")) or re.match(r"[\w.$]+:", s):
        return None
    return s.split()[0]


def slab_loops(body):
    """(header label, ragged, loads, full waits, loads before the first wait) of every loop with global loads and MFMAs.  The
    compiler marks a loop's blocks in the label comments: `=>This Inner Loop Header` and `in Loop: Header=BBn_m`."""
    blocks, cur = [], None                       # (label, header it belongs to or None, lines)
    for l in body:
        m = re.match(r"\.L(BB\d+_\d+):(.*)", l)
        if m:
            h = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            cur = (m.group(1), m.group(1) if "Loop Header" in m.group(2) else h.group(1) if h else None, [])
            blocks.append(cur)
        elif cur is not None:
            cur[2].append(l)
    out = []
    for head in [b[0] for b in blocks if b[1] == b[0]]:
        members = [b for b in blocks if b[1] == head]
        members.sort(key=lambda b: b[0] != head)                  # execution starts at the header block
        ms = [m for b in members for m in ((mnemonic(l), l) for l in b[2]) if m[0]]
        loads = [i for i, (m, _) in enumerate(ms) if m.startswith("global_load")]
        if not loads or not any(m.startswith("v_mfma") for m, _ in ms):
            continue
        waits = [i for i, (m, _) in enumerate(ms) if m == "s_waitcnt" or m.startswith("s_waitcnt_")]
        full = sum(1 for m, l in ms if m == "s_waitcnt" and re.search(r"vmcnt\(0\)", l))
        first = min([i for i in waits if i > loads[0]], default=len(ms))
        ragged = any(m.startswith(("v_cndmask", "s_and_saveexec")) for m, _ in ms)
        out.append((head, ragged, len(loads), full, sum(1 for i in loads if i < first)))
    return out


def classify(ms):
    c = collections.Counter()
    for m in ms:
        if m.startswith("v_mfma"):
            c["mfma"] += 1
        elif m.startswith("v_"):
            c["valu"] += 1
        elif m.startswith(("s_waitcnt", "s_nop")):
            c["wait"] += 1
        elif m.startswith(("s_cbranch", "s_branch")):
            c["branch"] += 1
        elif m.startswith("s_barrier"):
            c["barrier"] += 1
        elif m.startswith("s_"):
            c["salu"] += 1
        elif m.startswith("ds_"):
            c["lds"] += 1
            if m.startswith("ds_bpermute"):
                c["bpermute"] += 1
        else:
            c["other"] += 1                     # global / scratch / buffer memory
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="count an assembly file made earlier instead of compiling")
    ap.add_argument("--kernel", default=KERNEL, help="substring of the mangled name of the function to count")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--top", type=int, default=0, help="also list the N commonest VALU mnemonics")
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            compile_asm(os.path.join(td, "k.s"))
            text = open(os.path.join(td, "k.s")).read()
    body, meta = function_lines(text, args.kernel)
    spills = sum(1 for l in body if "Folded Spill" in l or "Spill" in l and "scratch_store" in l)
    reloads = sum(1 for l in body if "Reload" in l)
    ms = [m for m in map(mnemonic, body) if m]
    c = classify(ms)
    print("| build | VALU | SALU | branches | LDS | ds_bpermute | waits/nops | MFMA | memory | VGPRs | spill st / reloads | scratch | LDS bytes |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    print(f"| {args.label} | {c['valu']} | {c['salu']} | {c['branch']} | {c['lds']} | {c['bpermute']} | {c['wait']} | {c['mfma']} | {c['other']} | "
          f"{meta.get('NumVgprs')} | {spills} / {reloads} | {meta.get('ScratchSize')} B | {meta.get('LDSByteSize')} |")
    print()
    for head, ragged, loads, full, ahead in slab_loops(body):
        print(f"slab loop {head} ({'ragged M' if ragged else 'full chunks'}): {loads} global loads, {full} full vmcnt(0) waits, "
              f"{ahead} loads before the first wait")
    if args.top:
        top = collections.Counter(re.sub(r"_e(32|64)$", "", m) for m in ms if m.startswith("v_") and not m.startswith("v_mfma"))
        print("\nVALU by mnemonic: " + ", ".join(f"{k} {v}" for k, v in top.most_common(args.top)))


if __name__ == "__main__":
    main()

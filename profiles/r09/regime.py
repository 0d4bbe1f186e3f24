"""One regime of the broadband stream, for a kernel trace or for a bit-for-bit comparison.
Run from the root of the tree under test: python3 <path>/regime.py NAME [OUT.npz]
With OUT.npz every returned sample and get_state() (plus the last hop's attributes) are written there."""
import os
import sys

import numpy as np

root = os.getcwd()
sys.path[:0] = [root]

import ap_vast_unofficial_amd  # noqa: E402
import ap_vast_unofficial_amd.apvast as mod  # noqa: E402
from ap_vast_unofficial_amd.apvast import apvast  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(ap_vast_unofficial_amd.__file__))) == root, ap_vast_unofficial_amd.__file__

rirs = np.load(os.path.join(root, "tests", "golden", "rirs_cfg1.npz"))
rA, rB = rirs["rirA"], rirs["rirB"]


def cfg1(**kw):
    return apvast(256, rA, rB, 32, 16, 0, 0, 8, 1.0, 512, hop_size=128, perceptual=False, mode="broadband", seed=0, **kw), 128


def matlab():
    a, b = rA[:, :4, :6], rB[:, :4, :6]
    o = apvast(256, a, b, 16, 8, 1, 2, [1, 3, 8, 20], 1.0, 384, sampling_rate=16000, perceptual=True, mode="broadband",
               dialect="matlab", fullscale_db_spl=100.0)
    rng = np.random.default_rng(21)
    st = o.get_state()
    o.set_state({"response": 1e-3 * rng.standard_normal(st["response"].shape),
                 "target_response": 1e-3 * rng.standard_normal(st["target_response"].shape)})
    return o, 128


def reftest():
    return apvast(1600, rA, rB, 100, 20, 6, 6, 50, 1.0, 1000, perceptual=False, mode="broadband", seed=0), 800


# name -> (constructor, [(call, hops), ...]); "live" reassigns the responses between its two signals
REGIMES = {
    "hop_loop": (cfg1, [("hops", 6)]),
    "signal_pageable": (cfg1, [("signal", 35)]),
    "signal_pinned": (cfg1, [("pinned", 35)]),
    "zone_A": (lambda: cfg1(run_B=False), [("signal", 17), ("hops", 2)]),
    "zone_B": (lambda: cfg1(run_A=False), [("signal", 17), ("hops", 2)]),
    "matlab_perceptual": (matlab, [("signal", 9), ("hops", 2)]),
    "python_relative": (cfg1, [("signal", 17), ("hops", 2)]),
    "max_sweeps_30": (lambda: cfg1(max_sweeps=30), [("signal", 17), ("hops", 2)]),
    "live": (cfg1, [("signal", 4), ("set_rirs", 0), ("signal", 4)]),
    "reftest": (reftest, [("signal", 16)]),
}

name = sys.argv[1]
out_path = sys.argv[2] if len(sys.argv) > 2 else None
make, calls = REGIMES[name]
if name == "python_relative":
    mod.EXPERIMENTAL_REGULARIZATION = False
ap, H = make()
total = sum(n for _, n in calls)
x = np.random.default_rng(7).standard_normal((2, total * H))
saved, at = {}, 0


def keep(tag, res):
    for q in range(4):
        if res[q] is not None:
            saved[f"{tag}_out{q}"] = np.stack([np.asarray(v) for v in res[q]])


for i, (call, n) in enumerate(calls):
    xa, xb = x[0, at * H:(at + n) * H], x[1, at * H:(at + n) * H]
    if call == "signal":
        keep(f"c{i}", ap.process_signal(xa, xb))
    elif call == "pinned":
        keep(f"c{i}", ap.process_signal(xa, xb, out=ap.alloc_signal_output(n * H)))
    elif call == "hops":
        for h in range(n):
            keep(f"c{i}h{h}", ap.process_input_buffers(xa[h * H:(h + 1) * H], xb[h * H:(h + 1) * H]))
    elif call == "set_rirs":
        ap.rir_A = 0.5 * rA + 0.25 * rB
        ap.rir_B = rB[::-1].copy() * 0.1 + rB
    at += n
if out_path:
    for k, v in ap.get_state().items():
        saved["state_" + k] = np.asarray(v)
    for k in ("R_A_to_A", "R_A_to_B", "R_B_to_B", "R_B_to_A", "r_A", "r_B", "lambda_A", "lambda_B", "w_A", "w_B", "U_A", "U_B",
              "input_spectrum_A", "input_spectrum_B"):
        v = getattr(ap, k)
        if v is not None:
            saved["attr_" + k] = np.asarray(v)
    np.savez(out_path, **saved)
ap.close()
print(name, "ok", len(saved), "arrays", ap_vast_unofficial_amd.__file__)

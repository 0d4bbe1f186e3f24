"""Writes tests/golden/g10_per_hop_entry_points.npz: what the per-hop entry points of the FIR synthesis and of the filter-length
constraint return on one small case each, (J, H) = (6, 30) with (V, L) = (2, 70), inputs included.

    python tools/make_golden_signal_constrained.py [out.npz]          (needs the GPU)

Run on the commit BEFORE the two kernels took the hop into their grids (csrc/kernels_firsynth.hip, csrc/kernels_constrain.hip):
tests/test_gpu_signal_constrained.py holds the later builds to these bits.  This project's own outputs, float64.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, L, J, H, N = 2, 70, 6, 30, 32


def main():
    from ap_vast_unofficial_amd._capi import Engine
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "g10_per_hop_entry_points.npz")
    rng = np.random.default_rng(610)
    eng = Engine(9, 4, 4, compute_dtype="f64")
    x = rng.standard_normal(J - 1 + H)
    gp, gc = rng.standard_normal((V, J, L)), rng.standard_normal((V, J, L))
    y = eng.fir_synthesis(x, gp, gc, H)
    w = rng.standard_normal((N // 2 + 1, V, L)) + 1j * rng.standard_normal((N // 2 + 1, V, L))
    w2, taps = eng.constrain_filters(w, N, J)
    eng.close()
    np.savez_compressed(out, fir_x=x, fir_taps_prev=gp, fir_taps_cur=gc, fir_H=H, fir_out=y, cf_w=w, cf_N=N, cf_J=J, cf_w_out=w2,
                        cf_taps_out=taps)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

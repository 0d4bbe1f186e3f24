"""One regime of the subband stream, 20 hops at the shapes of tests/test_gpu_signal_constrained.py, for a kernel trace.
Run from the root of the tree under test: python3 <path>/regime.py NAME"""
import os
import sys

root = os.getcwd()
sys.path[:0] = [root, os.path.join(root, "tests")]

import ap_vast_unofficial_amd  # noqa: E402
from test_gpu_signal_constrained import H, make, signal  # noqa: E402
from test_gpu_stream import _hop_loop  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(ap_vast_unofficial_amd.__file__))) == root, ap_vast_unofficial_amd.__file__

CONS = dict(constrain_filter_length=True)
FIR = dict(constrain_filter_length=True, synthesis="fir")
REGIMES = {
    "perhop_nograph": (dict(), False, (0, 0)),
    "pipeline_P20": (dict(P=20), True, (0, 20)),
    "chunked_L4": (dict(), True, (20, 0)),
    "chunked_L16": (dict(L=16, M=20), True, (20, 0)),
    "wola_L4": (dict(**CONS), True, (20, 0)),
    "wola_L16": (dict(L=16, M=20, **CONS), True, (20, 0)),
    "fir_L4": (dict(**FIR), True, (20, 0)),
    "fir_L16": (dict(L=16, M=20, **FIR), True, (20, 0)),
    "forgetting": (dict(statistics_forgetting=0.9), True, (0, 20)),
}

name = sys.argv[1]
kw, whole, expected = REGIMES[name]
if name == "perhop_nograph":
    assert os.environ.get("APV_NO_GRAPH"), "per-hop regime runs with graphs off"
ap = make(**kw)
x = signal(20)
if whole:
    ap.process_signal(x[0], x[1])
else:
    _hop_loop(ap, x, 0, 20)
assert ap.signal_schedule == expected, (name, ap.signal_schedule)
ap.close()
print(name, "ok", ap_vast_unofficial_amd.__file__)

"""process_signal of a constrained subband stream (constrain_filter_length=True, synthesis "wola" or "fir") through the chunked
schedule: one projection launch and, for "fir", one synthesis launch per chunk of sixteen hops (csrc/stream.hip,
process_signal_chunked_t; csrc/kernels_constrain.hip and csrc/kernels_firsynth.hip with the hop in grid.z).

The contract is the hop loop's bits: every comparison is np.array_equal, no tolerance.  The state "signal_schedule"
(apvast.signal_schedule) says which schedule a call took, which is what lets a test see the feature at all.

Streams are those of tests/test_gpu_stream.py::test_process_signal_equals_hop_loop -- 70-tap responses, so K1 takes one
fast-convolution segment and the chunked driver runs; N = 128, H = 64, filter_length 16, modeling_delay 5, two eigenvectors -- with
the two keywords.  (L, M) = (4, 8) runs the joint diagonalisations hop by hop on the back streams, (16, 20) as one launch per chunk."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_stream import _hop_loop, synth_rirs  # noqa: E402

N, H, J, DELAY = 128, 64, 16, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_per_hop_entry_points.npz")


def make(L=4, M=8, P=70, n=N, h=H, j=J, delay=DELAY, dtype="f64", seed=3, perceptual=False, **kw):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 11)
    return apvast(n, rirA, rirB, j, delay, 1, 2, 2, 1.0, 4 * n, hop_size=h, seed=seed, dtype=dtype, perceptual=perceptual,
                  sampling_rate=16000, **kw)


def signal(n_hops, h=H, seed=8):
    return np.random.default_rng(seed).standard_normal((2, n_hops * h))


def same_signal(got, ref):
    for q in range(4):
        if ref[q] is None:
            assert got[q] is None
            continue
        for v in range(len(ref[q])):
            assert got[q][v].shape == ref[q][v].shape
            assert np.array_equal(got[q][v], ref[q][v]), (q, v)


ATTRS = ("w_A", "w_B", "w_time_A", "w_time_B", "lambda_A", "lambda_B")


def same_state(b, c):
    sb, sc = b.get_state(), c.get_state()
    assert sb.keys() == sc.keys()
    for k in sb:
        assert np.array_equal(sb[k], sc[k]), k
    for name in ATTRS:
        x, y = getattr(b, name), getattr(c, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert np.array_equal(x, y), name


# 1 ---------------------------------------------------------------------------------------------------------------
SCHEDULES = [
    ("wola-hop-by-hop-regime", dict(constrain_filter_length=True), 41, (41, 0)),
    ("wola-batched-regime", dict(L=16, M=20, constrain_filter_length=True), 41, (41, 0)),
    ("fir-hop-by-hop-regime", dict(constrain_filter_length=True, synthesis="fir"), 41, (41, 0)),
    ("fir-batched-regime", dict(L=16, M=20, constrain_filter_length=True, synthesis="fir"), 41, (41, 0)),
    ("unconstrained", dict(), 41, (41, 0)),
    ("fir-forgetting", dict(constrain_filter_length=True, synthesis="fir", statistics_forgetting=0.9), 5, (0, 5)),
    ("fir-20-tap-responses", dict(P=20, constrain_filter_length=True, synthesis="fir"), 5, (0, 5)),
]


@pytest.mark.parametrize("name,kw,n_hops,expected", SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_schedule_taken(name, kw, n_hops, expected):
    ap = make(**kw)
    x = signal(n_hops + 2)
    assert ap.signal_schedule == (0, 0)                      # before any whole-signal call
    _hop_loop(ap, x, 0, 2)
    assert ap.signal_schedule == (0, 0)                      # after per-hop calls only
    ap.process_signal(x[0, 2 * H:], x[1, 2 * H:])
    assert ap.signal_schedule == expected
    assert "signal_schedule" not in ap.get_state()
    ap.close()


# 2 ---------------------------------------------------------------------------------------------------------------
def against_the_hop_loop(mk):
    """per-hop calls, 41 hops (three chunks, the last partial), per-hop calls, 4 hops, a per-hop call: samples, states and
    attributes are those of the hop loop"""
    a, b, c = mk(), mk(), mk()
    n_hops = 2 + 41 + 2 + 4 + 1
    x = signal(n_hops)
    ref = _hop_loop(a, x, 0, n_hops)
    parts = [_hop_loop(b, x, 0, 2)]
    pos, cpos = 2, 0
    for n in (41, 0, 4):
        if n == 0:
            parts.append(_hop_loop(b, x, pos, pos + 2))
            pos += 2
            continue
        parts.append(list(b.process_signal(x[0, pos * H:(pos + n) * H], x[1, pos * H:(pos + n) * H])))
        pos += n
        assert b.signal_schedule == (n, 0)
        _hop_loop(c, x, cpos, pos)                           # the third object: the hop loop up to here
        cpos = pos
        same_state(b, c)
    parts.append(_hop_loop(b, x, pos, pos + 1))
    got = [[np.concatenate([p[q][v] for p in parts]) for v in range(len(ref[q]))] for q in range(4)]
    same_signal(got, ref)
    for o in (a, b, c):
        o.close()


@pytest.mark.parametrize("L,M", [(4, 8), (16, 20)])
@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
@pytest.mark.parametrize("synthesis", ["wola", "fir"])
def test_bit_for_bit_against_the_hop_loop(synthesis, dtype, L, M):
    against_the_hop_loop(lambda: make(L=L, M=M, dtype=dtype, constrain_filter_length=True, synthesis=synthesis))


@pytest.mark.parametrize("perceptual", [False, True], ids=["plain", "perceptual"])
def test_bit_for_bit_unconstrained_one_launch_per_chunk(perceptual):
    """the same against an unconstrained stream whose joint diagonalisations are one launch per chunk: that launch without a
    projection behind it and, with the perceptual weighting on, the weighting of every hop of a chunk on the front stream"""
    against_the_hop_loop(lambda: make(L=16, M=20, dtype="f64", perceptual=perceptual))


# 3 ---------------------------------------------------------------------------------------------------------------
EDGES = [
    (128, 64, 1, 0, {}),                         # no history
    (128, 64, 128, 5, dict(run_B=False)),        # J - 1 > H and > N - H: the history spans two hops
    (128, 32, 100, 5, dict(run_A=False)),        # J - 1 > 3 H
    (60, 20, 45, 5, {}),                         # hop other than N / 2, mixed-radix N
]


@pytest.mark.parametrize("n,h,j,delay,kw", EDGES, ids=["J1", "J128", "J100-H32", "N60-H20-J45"])
def test_edges_of_taps_and_hop(n, h, j, delay, kw):
    mk = lambda: make(n=n, h=h, j=j, delay=delay, constrain_filter_length=True, synthesis="fir", **kw)
    a, b = mk(), mk()
    hops = 19
    x = signal(hops, h)
    ref = _hop_loop(a, x, 0, hops)
    got = list(b.process_signal(x[0], x[1]))
    assert b.signal_schedule == (hops, 0)
    same_signal(got, ref)
    same_state(b, a)
    a.close()
    b.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "mixed"])
def test_resume(dtype):
    mk = lambda **kw: make(dtype=dtype, constrain_filter_length=True, synthesis="fir", **kw)
    a, b, c = mk(), mk(), mk(seed=1)
    x = signal(40)
    ref = _hop_loop(a, x, 0, 40)
    b.process_signal(x[0, :20 * H], x[1, :20 * H])
    c.set_state(b.get_state())
    tail = [[r[20 * H:] for r in ref[q]] for q in range(4)]
    for o in (b, c):
        same_signal(list(o.process_signal(x[0, 20 * H:], x[1, 20 * H:])), tail)
        assert o.signal_schedule == (20, 0)
    for o in (a, b, c):
        o.close()


# 5 ---------------------------------------------------------------------------------------------------------------
def test_into_the_callers_array():
    mk = lambda: make(constrain_filter_length=True, synthesis="fir")
    a, b = mk(), mk()
    x = signal(20)
    ref = list(a.process_signal(x[0], x[1]))
    out = b.alloc_signal_output(20 * H)
    got = list(b.process_signal(x[0], x[1], out=out))
    assert b.signal_schedule == (20, 0)
    same_signal(got, ref)
    assert np.shares_memory(got[0][0], out)
    a.close()
    b.close()


# 6 ---------------------------------------------------------------------------------------------------------------
def test_per_hop_entry_points_keep_their_bits():
    """Engine.fir_synthesis and Engine.constrain_filters at (J, H) = (6, 30), (V, L) = (2, 70) against what the build without the
    hop index in the two kernels' grids returned for the same arrays on the same GPU (tools/make_golden_signal_constrained.py
    recorded inputs and outputs): this project's own earlier output, bit for bit."""
    from ap_vast_unofficial_amd._capi import Engine
    g = np.load(GOLDEN)
    eng = Engine(9, 4, 4, compute_dtype="f64")
    y = eng.fir_synthesis(g["fir_x"], g["fir_taps_prev"], g["fir_taps_cur"], int(g["fir_H"]))
    assert y.dtype == g["fir_out"].dtype and np.array_equal(y, g["fir_out"])
    w, taps = eng.constrain_filters(g["cf_w"], int(g["cf_N"]), int(g["cf_J"]))
    assert w.dtype == g["cf_w_out"].dtype and np.array_equal(w, g["cf_w_out"])
    assert taps.dtype == g["cf_taps_out"].dtype and np.array_equal(taps, g["cf_taps_out"])
    eng.close()

"""FIR synthesis of the constrained subband stream (apvast(..., synthesis="fir"), apv_stream_set_synthesis, apv_fir_synthesis,
csrc/kernels_firsynth.hip): the kernel against the float64 NumPy definition (tests/fir_synthesis_oracle.py), the stream against
that definition evaluated on its own taps and on the taps of the constrained stream oracles (tests/constraint_oracle.py).

Tolerance, derived.  A J-term dot product summed in any order errs by at most about J u sum |g| |x|; the blend of the two sums adds
a handful of roundings; the NumPy side carries the same bound in float64.  Every output sample is therefore held to

    |got - ref| <= 2 (J + 6) u S,    S = sum |g_prev| |x| + sum |g_cur| |x|  (elementwise, fir_reference returns it)

with u = 2^-53 for float64 filters and samples and 2^-24 for float32, `ref` computed from the taps and inputs as the device holds
them.  Against the stream oracles the taps themselves differ by the solver's error: those tests hold to the table TOL of
tests/test_gpu_stream.py as it stands, relative to the largest reference value of the run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from constraint_oracle import ConstrainedForgettingOracle, ConstrainedSubbandOracle  # noqa: E402, F401
from fir_synthesis_oracle import FirStreamReference, fir_reference  # noqa: E402
from test_gpu_filter_constraint import DELAY, REF_A, REF_B, make_pair, signal  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import TOL, check_outputs, synth_rirs  # noqa: E402

U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}

# the issue's stream shape: N = 32, H = 16, L = 4, M = 6, 24-tap responses, V = 2, J = 8, six hops
N, H, L, M, P, V, J, HOPS = 32, 16, 4, 6, 24, 2, 8, 6


def bound(j, dtype):
    return 2 * (j + 6) * U[dtype]


def make_fir_pair(dtype="f64", **kw):
    return make_pair(dtype, synthesis="fir", **kw)


# 1 ---------------------------------------------------------------------------------------------------------------
# the issue's (J, H), then one hop of 272 samples: from 256 samples on a workgroup takes four sample tiles, the last one partial here
JH = [(1, 16), (5, 16), (6, 30), (40, 16), (32, 16), (64, 64), (7, 272)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("j,h", JH)
def test_kernel_against_numpy(j, h, dtype):
    from ap_vast_unofficial_amd._capi import Engine
    rng = np.random.default_rng(100 * j + h)
    eng = Engine(9, 4, 4, compute_dtype=dtype)
    worst = 0.0
    for nv, nl in ((1, 3), (4, 16), (2, 70)):
        gp = rng.standard_normal((nv, j, nl)).astype(eng.lam_dtype)
        gc = rng.standard_normal((nv, j, nl)).astype(eng.lam_dtype)
        x = rng.standard_normal(j - 1 + h).astype(eng.s_dtype)
        got = eng.fir_synthesis(x, gp, gc, h)
        assert got.shape == (nv, h, nl) and got.dtype == eng.s_dtype
        ref, S = fir_reference(x, gp, gc, h)
        worst = max(worst, (np.abs(got - ref) / S).max() / bound(j, dtype))
        assert np.all(np.abs(got - ref) <= bound(j, dtype) * S), (nv, nl, (np.abs(got - ref) / S).max() / bound(j, dtype))
        # equal taps: the linear convolution
        same = eng.fir_synthesis(x, gc, gc, h).astype(np.float64)
        xd, gd = x.astype(np.float64), gc.astype(np.float64)
        conv = np.stack([np.stack([np.convolve(xd, gd[v, :, l])[j - 1:j - 1 + h] for l in range(nl)], axis=1) for v in range(nv)])
        _, S2 = fir_reference(x, gc, gc, h)
        worst = max(worst, (np.abs(same - conv) / S2).max() / bound(j, dtype))
        assert np.all(np.abs(same - conv) <= bound(j, dtype) * S2)
        # delta taps (a different delay per rank and loudspeaker): the shifted input, exactly
        delta = np.zeros((nv, j, nl), dtype=eng.lam_dtype)
        at = (np.arange(nv)[:, None] * 3 + np.arange(nl)[None, :]) % j
        for v in range(nv):
            delta[v, at[v], np.arange(nl)] = 1.0
        shifted = eng.fir_synthesis(x, delta, delta, h)
        for v in range(nv):
            for l in range(nl):
                assert np.array_equal(shifted[v, :, l], x[j - 1 - at[v, l]:j - 1 - at[v, l] + h]), (v, l)
    print(f"J={j} H={h} {dtype}: largest error / bound {worst:.3f}")
    eng.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_kernel_writes_nothing_beyond_its_output(dtype):
    """canary values in front of and behind d_out, and behind the inputs' ends nothing to read: L = 70, H = 30, J = 6 are all off
    the tile sizes"""
    from ap_vast_unofficial_amd._capi import Engine
    eng = Engine(9, 4, 4, compute_dtype=dtype)
    rng = np.random.default_rng(5)
    nv, j, nl, h, pad = 2, 6, 70, 30, 256
    sd, isz = eng.s_dtype, np.dtype(eng.s_dtype).itemsize
    gp, gc = (rng.standard_normal((nv, j, nl)).astype(eng.lam_dtype) for _ in range(2))
    x = rng.standard_normal(j - 1 + h).astype(sd)
    dx, dp, dc = eng.to_device(x), eng.to_device(gp), eng.to_device(gc)
    buf = np.full(pad + nv * h * nl + pad, -777.0, dtype=sd)
    dout = eng.to_device(buf)
    import ctypes
    inner = ctypes.c_void_p(dout.ptr.value + pad * isz)
    eng._chk(eng.lib.apv_fir_synthesis(eng.h, dx.ptr, dp.ptr, dc.ptr, nv, nl, j, h, inner))
    back = dout.download(buf.shape, sd)
    assert np.all(back[:pad] == -777.0) and np.all(back[-pad:] == -777.0)
    ref, S = fir_reference(x, gp, gc, h)
    assert np.all(np.abs(back[pad:-pad].reshape(nv, h, nl) - ref) <= bound(j, dtype) * S)
    for b in (dx, dp, dc, dout):
        b.free()
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------
def test_entry_refusals():
    from ap_vast_unofficial_amd import _capi
    eng = _capi.Engine(N // 2 + 1, L, M, block_size=N, hop_size=H)
    with pytest.raises(_capi.ApvError):                                   # J = 0
        eng.fir_synthesis(np.zeros(15), np.zeros((1, 0, 4)), np.zeros((1, 0, 4)), 16)
    with pytest.raises(_capi.ApvError):                                   # H = 0
        eng.fir_synthesis(np.zeros(3), np.zeros((1, 4, 4)), np.zeros((1, 4, 4)), 0)
    d = eng.alloc(1024)
    assert eng.lib.apv_fir_synthesis(eng.h, None, d.ptr, d.ptr, 1, 4, 4, 4, d.ptr) == _capi.ERR_ARG
    assert eng.lib.apv_fir_synthesis(eng.h, d.ptr, d.ptr, d.ptr, 1, 4, 4, 4, None) == _capi.ERR_ARG
    d.free()
    assert eng.lib.apv_stream_set_synthesis(eng.h, 2) == _capi.ERR_ARG     # an unknown mode
    assert eng.lib.apv_stream_set_synthesis(eng.h, -1) == _capi.ERR_ARG
    with pytest.raises(ValueError):
        eng.set_synthesis("ola")
    eng.set_synthesis("fir")
    rirA, rirB = synth_rirs(P, L, M, 1)
    with pytest.raises(_capi.ApvError, match="filter taps"):             # FIR without taps
        eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    eng.set_filter_taps(J)
    eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    assert eng.lib.apv_stream_set_synthesis(eng.h, 0) == _capi.ERR_ARG     # after apv_stream_init
    assert eng.state_bytes("fir_synth_taps_A") == 1 * J * L * 8            # one rank, float64 filters
    assert eng.state_bytes("fir_synth_history1") == (J - 1) * 8
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------
def run_self_consistent(dtype, shape, taps, run_A=True, run_B=True, hops=HOPS):
    """every hop's outputs against the definition evaluated on the taps w_time_* of that hop and of the hop before, and on the
    inputs as the device holds them, at the derived bound; the target paths exactly"""
    n, h, l, m, p = shape
    ap, _ = make_fir_pair(dtype, run_A=run_A, run_B=run_B, shape=shape, taps=taps)
    sd = ap._eng.s_dtype
    x = signal(hops, h)
    xd = x.astype(sd).astype(np.float64)
    ref = FirStreamReference(taps, h, l, V, DELAY, REF_A, run_A, run_B)
    worst = 0.0
    for k in range(hops):
        got = hop(ap, x, k, h)
        exp, S = ref.hop(xd[0, k * h:(k + 1) * h], xd[1, k * h:(k + 1) * h], [ap.w_time_A, ap.w_time_B])
        for z, run in enumerate((run_A, run_B)):
            if not run:
                assert got[z] is None
                continue
            err = np.abs(np.stack(got[z]) - np.stack(exp[z]))
            worst = max(worst, (err[S[z] > 0] / S[z][S[z] > 0]).max() / bound(taps, dtype))
            assert np.all(err <= bound(taps, dtype) * S[z]), (k, z, worst)
        for q in (2, 3):
            assert np.array_equal(np.stack(got[q]), np.stack(exp[q])), (k, q)
    print(f"{dtype} N={n} H={h} J={taps} A={run_A} B={run_B}: largest error / bound {worst:.3f}")
    ap.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("run_A,run_B", [(True, True), (False, True), (True, False)])
def test_stream_self_consistent(dtype, run_A, run_B):
    run_self_consistent(dtype, (N, H, L, M, P), J, run_A, run_B)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n,h,j", [(60, 20, 45), (68, 34, 6)])
def test_stream_self_consistent_other_shapes(dtype, n, h, j):
    """(60, 20, 45): a hop other than N/2, a history longer than two hops and than the input block ring reaches, a 30-point
    transform in the projection; (68, 34, 6): the Bluestein projection feeds the synthesis"""
    run_self_consistent(dtype, (n, h, L, M, P), j)


# 4 ---------------------------------------------------------------------------------------------------------------
def run_vs_oracle(dtype, shape=(N, H, L, M, P), taps=J, hops=HOPS, mu_at=None, **kw):
    n, h, l, m, p = shape
    ap, orc = make_fir_pair(dtype, shape=shape, taps=taps, **kw)
    x = signal(hops, h)
    ref = FirStreamReference(taps, h, l, V, DELAY, REF_A)
    got, exp = [], []
    for k in range(hops):
        if mu_at is not None and k == mu_at:
            ap.mu = orc.mu = 30.0
        got.append(hop(ap, x, k, h))
        hop(orc, x, k, h)
        exp.append(ref.hop(x[0, k * h:(k + 1) * h], x[1, k * h:(k + 1) * h], orc.w_time)[0])
    for q in range(2):
        peak = max(np.abs(np.stack(e[q])).max() for e in exp)
        print(f"{dtype} {kw} zone {q}: per-hop output error / peak",
              ["%.1e" % (np.abs(np.stack(g[q]) - np.stack(e[q])).max() / peak) for g, e in zip(got, exp)])
    exp = [tuple(np.stack(e[q]) if q < 2 else e[q][0] for q in range(4)) for e in exp]      # the shapes the stream oracles return
    check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    ap.close()


@pytest.mark.parametrize("dtype,kw", [("f64", {}), ("f32", {}), ("f64", {"statistics_forgetting": 0.9}), ("f64", {"statistics_hops": 3})])
def test_stream_vs_oracle(dtype, kw):
    run_vs_oracle(dtype, **kw)


def test_stream_vs_oracle_mu_reassigned():
    run_vs_oracle("f64", mu_at=3)                 # "after hop 2": before the hop with index 3


def test_stream_vs_oracle_order_70():
    """L = 70, M = 8, N = 16: csrc/kernels_gevd128.hip designs, five loudspeaker tiles per group, the last of them partial"""
    run_vs_oracle("f64", shape=(16, 8, 70, 8, 12), taps=6, hops=4)


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_design_half_untouched(dtype):
    fir, _ = make_fir_pair(dtype)
    wola, _ = make_pair(dtype)
    x = signal(HOPS)
    differ = False
    for k in range(HOPS):
        a, b = hop(fir, x, k, H), hop(wola, x, k, H)
        for name in ("w_A", "w_B", "lambda_A", "lambda_B", "w_time_A", "w_time_B"):
            assert np.array_equal(getattr(fir, name), getattr(wola, name)), (k, name)
        differ = differ or not np.array_equal(np.stack(a[0]), np.stack(b[0]))
    assert differ                                 # ... and the synthesis is another one
    # the overlap buffers of the WOLA synthesis are not touched by the FIR hops
    assert not fir.get_state()["out_overlap"].any() and wola.get_state()["out_overlap"].any()
    fir.close()
    wola.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "mixed"])
def test_process_signal_and_resume_are_bit_for_bit(dtype):
    a, _ = make_fir_pair(dtype)
    b, _ = make_fir_pair(dtype)
    x = signal(HOPS)
    loop = [hop(a, x, k, H) for k in range(HOPS)]
    sig = b.process_signal(x[0], x[1])
    for q in range(4):
        for v in range(V):
            assert np.array_equal(np.concatenate([o[q][v] for o in loop]), sig[q][v]), (q, v)
    c, _ = make_fir_pair(dtype)
    d, _ = make_fir_pair(dtype, seed=1)
    for k in range(3):
        hop(c, x, k, H)
    st = c.get_state()
    assert st["fir_synthesis_taps"].shape == (2, V, J, L) and st["fir_synthesis_history"].shape == (2, J - 1)
    assert np.array_equal(st["fir_synthesis_taps"][0], c.w_time_A) and np.array_equal(st["fir_synthesis_taps"][1], c.w_time_B)
    sd = c._eng.s_dtype
    assert np.array_equal(st["fir_synthesis_history"], x[:, 3 * H - (J - 1):3 * H].astype(sd).astype(np.float64))
    d.set_state(st)
    for k in range(3, HOPS):
        same_outputs(hop(c, x, k, H), loop[k])
        same_outputs(hop(d, x, k, H), loop[k])
    for o in (a, b, c, d):
        o.close()


def test_state_keys_only_with_the_keyword():
    from ap_vast_unofficial_amd import _capi
    wola, _ = make_pair("f64")
    fir, _ = make_fir_pair("f64", run_B=False)
    x = signal(1)
    hop(wola, x, 0, H)
    hop(fir, x, 0, H)
    st = wola.get_state()
    assert "fir_synthesis_taps" not in st and "fir_synthesis_history" not in st
    with pytest.raises(KeyError):
        wola.set_state({"fir_synthesis_taps": np.zeros((2, V, J, L))})
    with pytest.raises(KeyError):
        fir.set_state({"fir_synthesis_tap": np.zeros((1, V, J, L))})        # unknown keys keep raising
    for name in ("fir_synth_taps_A", "fir_synth_taps_B", "fir_synth_history0", "fir_synth_history1", "fir_synthesis_kernel_ms"):
        with pytest.raises(_capi.ApvError, match="unknown state name"):
            wola._eng.state_bytes(name)
    assert fir.get_state()["fir_synthesis_taps"].shape == (1, V, J, L)       # zone programs that run
    with pytest.raises(_capi.ApvError, match="unknown state name"):
        fir._eng.state_bytes("fir_synth_taps_B")
    with pytest.raises(ValueError, match="fir_synthesis_taps must have shape"):
        fir.set_state({"fir_synthesis_taps": np.zeros((2, V, J, L))})
    wola.close()
    fir.close()

"""Filter-length constraint of the subband stream (apvast(..., constrain_filter_length=True), apv_stream_set_filter_taps,
csrc/kernels_constrain.hip): the kernel against the three-line NumPy definition, the stream against the stream oracles with the
projection between their filter and synthesis steps (tests/constraint_oracle.py).

Tolerances.  The projection is one inverse and one forward transform of the STFT kernels' device code, so the kernel is held to
what those kernels are held to, relative to the largest reference value: 3e-6 with float32 filters (the synthesis bound of
test_stft_roundtrip_vs_oracle in tests/test_gpu_parity.py; its analysis bound is 2e-6) and 1e-13 with float64 filters
(TOL["f64"]["spec"] of tests/test_gpu_stream.py, the bound of the float64 transforms).  The stream is held to the table TOL of
tests/test_gpu_stream.py as it stands."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from constraint_oracle import ConstrainedForgettingOracle, ConstrainedSubbandOracle, project  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import TOL, check_last_hop_state, check_outputs, synth_rirs  # noqa: E402

KTOL = {"f32": 3e-6, "f64": 1e-13}

# the issue's stream shape: N = 32, H = 16, L = 4, M = 6, 24-tap responses, V = 2, J = 8, six hops
N, H, L, M, P, V, J, HOPS = 32, 16, 4, 6, 24, 2, 8, 6
DELAY, REF_A, REF_B = 3, 1, 2


def make_pair(dtype="f64", run_A=True, run_B=True, seed=0, shape=(N, H, L, M, P), taps=J, **kw):
    """a constrained apvast object and the matching oracle started from the same response buffers; kw: statistics_hops /
    statistics_forgetting, handed to both"""
    from ap_vast_unofficial_amd.apvast import apvast
    n, h, l, m, p = shape
    rirA, rirB = synth_rirs(p, l, m, 1)
    ap = apvast(n, rirA, rirB, taps, DELAY, REF_A, REF_B, V, 1.0, 4 * n, hop_size=h, run_A=run_A, run_B=run_B, perceptual=False,
                seed=seed, dtype=dtype, constrain_filter_length=True, **kw)
    rs = np.random.RandomState(seed)
    init_r = np.stack([1e-3 * rs.randn(n, l, m) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(n, m) for _ in range(2)])
    args = (n, rirA, rirB, DELAY, REF_A, REF_B, list(range(1, V + 1)), 1.0)
    okw = dict(hop_size=h, run_A=run_A, run_B=run_B, init_response=init_r, init_target_response=init_t, filter_taps=taps)
    if "statistics_forgetting" in kw:
        orc = ConstrainedForgettingOracle(*args, beta=kw["statistics_forgetting"], **okw)
    else:
        orc = ConstrainedSubbandOracle(*args, stat_hops=kw.get("statistics_hops", 1), **okw)
    return ap, orc


def signal(hops, h=H, seed=99):
    return np.random.default_rng(seed).standard_normal((2, hops * h))


# 1, 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [16, 60, 68])          # radix 2/4; N/2 = 2 * 3 * 5; N/2 = 2 * 17 (Bluestein)
def test_kernel_against_numpy(n, dtype):
    """Engine.constrain_filters on random (K, V, L) filters against the definition, J in {1, 5, N/2, N}, (V, L) in {(1, 3), (4, 16),
    (2, 70)} (L = 70 is not a multiple of the four loudspeakers a workgroup takes, L = 3 is less than one tile); then idempotence
    and rfft(pad(taps)) == W', all to KTOL."""
    from ap_vast_unofficial_amd._capi import Engine
    rng = np.random.default_rng(n)
    eng = Engine(n // 2 + 1, 4, 4, compute_dtype=dtype)
    tol, worst = KTOL[dtype], 0.0
    for nv, nl in ((1, 3), (4, 16), (2, 70)):
        w = (rng.standard_normal((n // 2 + 1, nv, nl)) + 1j * rng.standard_normal((n // 2 + 1, nv, nl))).astype(eng.w_dtype)
        for j in (1, 5, n // 2, n):
            ref, ref_taps = project(w.astype(np.complex128), n, j)
            scale = np.abs(ref).max()
            got, taps = eng.constrain_filters(w, n, j)
            assert got.dtype == eng.w_dtype and taps.dtype == eng.lam_dtype and taps.shape == (nv, j, nl)
            e_w = np.abs(got - ref).max() / scale
            e_t = np.abs(taps.transpose(1, 0, 2) - ref_taps).max() / np.abs(ref_taps).max()
            again, taps2 = eng.constrain_filters(got, n, j)
            e_i = max(np.abs(again - got).max() / scale, np.abs(taps2 - taps).max() / np.abs(ref_taps).max())
            pad = np.zeros((n, nv, nl))
            pad[:j] = taps.transpose(1, 0, 2)
            e_p = np.abs(np.fft.rfft(pad, axis=0) - got).max() / scale
            worst = max(worst, e_w, e_t, e_i, e_p)
            print(f"N={n} {dtype} V={nv} L={nl} J={j}: w {e_w:.1e} taps {e_t:.1e} idempotence {e_i:.1e} rfft(pad) {e_p:.1e}")
            assert max(e_w, e_t, e_i, e_p) < tol, (nv, nl, j, e_w, e_t, e_i, e_p)
            assert np.all(got[[0, -1]].imag == 0)
            if j == n:       # nothing is cut: W' is W, except that bins 0 and N/2 come out real
                assert np.abs(got[1:-1] - w[1:-1]).max() < tol * np.abs(w).max()
                assert np.abs(got[[0, -1]].real - w[[0, -1]].real).max() < tol * np.abs(w).max()
    print(f"N={n} {dtype}: largest error {worst:.2e} (bound {tol:.0e})")
    eng.close()


def test_kernel_entry_refusals():
    from ap_vast_unofficial_amd import _capi
    eng = _capi.Engine(9, 4, 4)
    w = np.ones((9, 1, 4), dtype=np.complex128)
    for j in (0, 17):                                    # J out of 1..N
        with pytest.raises(_capi.ApvError):
            eng.constrain_filters(w, 16, j)
    dw = eng.to_device(w)
    assert eng.lib.apv_constrain_filters(eng.h, dw.ptr, 9, 1, 4, 18, 4, None) == _capi.ERR_ARG     # n_bins != N / 2 + 1
    assert eng.lib.apv_constrain_filters(eng.h, dw.ptr, 9, 1, 4, 16, 4, None) == _capi.OK          # taps not wanted
    assert np.abs(dw.download((9, 1, 4), np.complex128) - project(w, 16, 4)[0]).max() < 1e-13
    dw.free()
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kw", [("f64", {}), ("f32", {}), ("f64", {"statistics_forgetting": 0.9}), ("f64", {"statistics_hops": 3})])
def test_stream_vs_oracle(dtype, kw):
    """every hop's outputs, the last hop's spectra, w_* (the projected filters) and lambda_* at the plain bounds"""
    ap, orc = make_pair(dtype, **kw)
    x = signal(HOPS)
    got = [hop(ap, x, h, H) for h in range(HOPS)]
    exp = [hop(orc, x, h, H) for h in range(HOPS)]
    check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    check_last_hop_state(ap, orc, TOL[dtype], N // 2 + 1, L, M)
    fs = ap.filter_spectra_A
    assert len(fs) == V and np.array_equal(np.stack(fs), ap.w_A)
    ap.close()


def test_stream_vs_oracle_order_70():
    """L = 70, M = 8, N = 16 (K = 9): csrc/kernels_gevd128.hip feeds the projection, 18 tiles of four loudspeakers per rank.  The
    plain float64 bounds, errors printed."""
    shape = (16, 8, 70, 8, 12)
    ap, orc = make_pair("f64", shape=shape, taps=6)
    x = signal(4, 8)
    got = [hop(ap, x, h, 8) for h in range(4)]
    exp = [hop(orc, x, h, 8) for h in range(4)]
    for q in range(2):
        peak = max(np.abs(e[q]).max() for e in exp)
        print(f"zone {q}: per-hop output error / peak", ["%.1e" % (np.abs(np.stack(g[q]) - e[q]).max() / peak) for g, e in zip(got, exp)])
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], 9, 70, 8)
    assert ap.w_time_A.shape == (V, 6, 70)
    ap.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_w_time(dtype):
    ap, orc = make_pair(dtype, run_B=False)
    assert ap.w_time_A is None and ap.w_time_B is None             # before the first hop
    x = signal(3)
    for h in range(3):
        hop(ap, x, h, H)
        hop(orc, x, h, H)
    t = ap.w_time_A
    assert ap.w_time_B is None                                     # run_B=False
    assert t.shape == (V, J, L) and t.dtype == np.float64
    g = np.fft.irfft(ap.w_A, N, axis=1)                            # (V, N, L)
    scale = np.abs(g).max()
    print(f"{dtype}: taps vs irfft {np.abs(g[:, :J] - t).max() / scale:.1e}, beyond J {np.abs(g[:, J:]).max() / scale:.1e}")
    assert np.abs(g[:, :J] - t).max() < KTOL[dtype] * scale
    assert np.abs(g[:, J:]).max() < KTOL[dtype] * scale
    ref = orc.w_time[0]
    assert np.abs(t - ref).max() < TOL[dtype]["w_max"] * np.abs(ref).max()
    ap.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_process_signal_and_resume_are_bit_for_bit(dtype):
    a, _ = make_pair(dtype)
    b, _ = make_pair(dtype)
    x = signal(5)
    loop = [hop(a, x, h, H) for h in range(5)]
    sig = b.process_signal(x[0], x[1])
    for q in range(4):
        for v in range(V):
            assert np.array_equal(np.concatenate([o[q][v] for o in loop]), sig[q][v]), (q, v)
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
        assert np.array_equal(getattr(a, "w_time_" + z), getattr(b, "w_time_" + z))
    c, _ = make_pair(dtype)
    d, _ = make_pair(dtype, seed=1)
    for h in range(3):
        hop(c, x, h, H)
    d.set_state(c.get_state())
    for h in range(3, 5):
        same_outputs(hop(c, x, h, H), loop[h])
        same_outputs(hop(d, x, h, H), loop[h])
    for z in "AB":
        assert np.array_equal(getattr(d, "w_" + z), getattr(a, "w_" + z))
        assert np.array_equal(getattr(d, "w_time_" + z), getattr(a, "w_time_" + z))
    for o in (a, b, c, d):
        o.close()


# 6 ---------------------------------------------------------------------------------------------------------------
def test_mu_reassigned_between_hops():
    ap, orc = make_pair("f64")
    x = signal(HOPS)
    got, exp = [], []
    for h in range(HOPS):
        if h == 3:
            ap.mu = orc.mu = 30.0
        got.append(hop(ap, x, h, H))
        exp.append(hop(orc, x, h, H))
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    check_last_hop_state(ap, orc, TOL["f64"], N // 2 + 1, L, M)
    ap.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    from ap_vast_unofficial_amd import _capi
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 1)
    mk = lambda **kw: apvast(N, rirA, rirB, J, DELAY, REF_A, REF_B, V, 1.0, 4 * N, hop_size=H, perceptual=False, seed=0, **kw)
    off, plain, on = mk(constrain_filter_length=False), mk(), mk(constrain_filter_length=True)
    x = signal(4)
    moved = 0.0
    for h in range(4):
        o, p, c = hop(off, x, h, H), hop(plain, x, h, H), hop(on, x, h, H)
        same_outputs(o, p)
        moved = max(moved, np.abs(np.stack(c[0]) - np.stack(p[0])).max() / np.abs(np.stack(p[0])).max())
    assert moved > 0.01                                            # ... and on is on
    for ap in (off, plain):
        assert ap.w_time_A is None and ap._eng.filter_taps == 0
        with pytest.raises(_capi.ApvError, match="unknown state name"):
            ap._eng.state_bytes("w_time_A")
    assert on._eng.state_bytes("w_time_A") == V * J * L * 8
    # the setter is refused once the stream runs, and out of range
    e = on._eng
    assert e.lib.apv_stream_set_filter_taps(e.h, 4) == _capi.ERR_ARG and e.filter_taps == J
    for o in (off, plain, on):
        o.close()
    eng = _capi.Engine(N // 2 + 1, L, M, block_size=N, hop_size=H)
    assert eng.lib.apv_stream_set_filter_taps(eng.h, -1) == _capi.ERR_ARG
    assert eng.lib.apv_stream_set_filter_taps(eng.h, N + 1) == _capi.ERR_ARG
    assert eng.lib.apv_stream_set_filter_taps(eng.h, N) == _capi.OK
    assert eng.lib.apv_stream_set_filter_taps(eng.h, 0) == _capi.OK
    eng.set_filter_taps(2)
    with pytest.raises(_capi.ApvError, match="modeling_delay"):      # delay 3 >= 2 taps
        eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    eng.close()

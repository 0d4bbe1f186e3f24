"""K1, the RIR convolution into the response rings, at the boundaries between its forms and at its tile tails.

The state arrays "response<p>" / "target_response<z>" are K1's output rings and SubbandStreamOracle.response / .target_response
the same rings by lfilter in float64, so K1 is compared on its own at the spectra tolerance of test_gpu_stream.TOL (1e-13 of the
ring's largest value in float64, 1e-6 in float32), after every hop, for ceil(N / H) + 2 hops: the ring turns over once.
  "f64": fir_f64_mfma_kernel (<1>, and <4> from H = 256) and the double-precision fast-convolution forms,
  "f32": fir_mfma_kernel and the float forms.
Forms (kernels_stft.hip, apv_fir_fft_size / apv_fir_partitions): direct below 64 taps, one overlap-save segment of
F = pow2 >= P - 1 + H while F <= 4096 doubles / 8192 floats, uniformly partitioned (H taps per partition) beyond.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_stream import TOL, run_pair, synth_rirs  # noqa: E402
from test_gpu_stream_hops import check_rings  # noqa: E402


def k1_run(N, H, rir_len, L, M, dtype, delay=0):
    """ceil(N / H) + 2 hops of a one-rank stream, K1's six rings against the oracle's after every hop; returns the pair"""
    rirA, rirB = synth_rirs(rir_len, L, M, 11)
    refA, refB = (1, 0) if L > 1 else (0, 0)
    ap, orc, _, _ = run_pair(N, H, rirA, rirB, delay, refA, refB, 1, 1.0, hops=0, dtype=dtype)
    hops = -(-N // H) + 2
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    for h in range(hops):
        ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        check_rings(ap, orc, TOL[dtype]["spec"], ("hop", h), inputs=False)
    return ap, orc


def history_samples(ap):
    e = ap._eng
    return e.state_bytes("input_history0") // np.dtype(e.s_dtype).itemsize


# ---- the direct form's tails -------------------------------------------------------------------------------------------------
# fir_mfma_kernel: taps in groups of 16 (prologue skipped when there is no whole group), pairs up to Peven, then the odd tap;
# fir_f64_mfma_kernel: ceil(P / 4) k-steps split over four waves (P <= 12: waves without a step), taps past P as zero operands
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("rir_len", [1, 2, 3, 5, 13, 15, 16, 17, 31, 63])
def test_direct_form_tap_tails(rir_len, dtype):
    ap, orc = k1_run(64, 32, rir_len, 3, 5, dtype)
    assert history_samples(ap) == rir_len - 1 + 32
    ap.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N,H,L,M", [(64, 32, 3, 11),       # C = 33: one live channel in the last tile of 32 (f32) and of 16 (f64); targets M = 11
                                     (280, 140, 3, 5),      # the second 128-sample tile holds 12 samples
                                     (250, 100, 3, 5),      # N % 4 != 0: the float32 kernel's scalar stores
                                     (64, 37, 3, 5),        # odd hop, ring_off odd
                                     (600, 300, 3, 5),      # H >= 256: four sample tiles per workgroup (f64), 300 = 4 * 64 + 44
                                     (600, 275, 3, 5)])     # ... 275 = 4 * 64 + 19, H does not divide N
def test_direct_form_tile_tails(N, H, L, M, dtype):
    rir_len = 17 if M == 11 else 21
    ap, orc = k1_run(N, H, rir_len, L, M, dtype)
    assert history_samples(ap) == rir_len - 1 + H
    ap.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_direct_form_target_is_last_tap(dtype):
    """modeling_delay = P - 1: the target response is one tap, the last"""
    ap, orc = k1_run(64, 32, 17, 3, 5, dtype, delay=16)
    assert history_samples(ap) == 17 - 1 + 32
    ap.close()


# ---- direct | one segment: 63 | 64 taps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("rir_len", [63, 64])
def test_direct_to_segment_switch(rir_len, dtype, monkeypatch):
    """At 63 taps the default run IS the direct form: its spectra equal those under APV_FIR_DIRECT bit for bit.  At 64 it is the
    fast form: some bit differs, and the two agree within the spectra tolerance.  Every run meets the oracle."""
    N, H, L, M = 256, 128, 3, 5
    K = N // 2 + 1
    runs = {}
    for form in ("default", "direct"):
        if form == "direct":
            monkeypatch.setenv("APV_FIR_DIRECT", "1")
        ap, orc = k1_run(N, H, rir_len, L, M, dtype)
        assert history_samples(ap) == rir_len - 1 + H
        runs[form] = np.stack([ap._eng.get_state(f"spectra{p}", (K, M, L), ap._eng.sc_dtype) for p in range(4)])
        ap.close()
    if rir_len < 64:
        assert np.array_equal(runs["default"], runs["direct"])
    else:
        assert not np.array_equal(runs["default"], runs["direct"])
        scale = np.abs(runs["direct"]).max()
        assert np.abs(runs["default"] - runs["direct"]).max() <= TOL[dtype]["spec"] * scale


# ---- segment sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N,H,rir_len", [(256, 128, 129),     # P - 1 + H = 256 exactly: F = 256
                                         (256, 128, 130),     # one more: F = 512
                                         (32, 1, 64),         # the smallest segment, F = 64 exactly
                                         (32, 2, 64)])        # F = 128
def test_segment_size_boundaries(N, H, rir_len, dtype):
    ap, orc = k1_run(N, H, rir_len, 3, 5, dtype)
    assert history_samples(ap) == rir_len - 1 + H
    ap.close()


# ---- one segment | partitioned ---------------------------------------------------------------------------------------------
#   (dtype, N, H, P, partitions; 0 = one segment)
LONG = [("f64", 256, 128, 3969, 0),        # P - 1 + H = 4096 doubles: the largest single segment
        ("f64", 256, 128, 3970, 32),       # the last partition holds 2 taps
        ("f64", 256, 128, 4096, 32),       # the last partition is full
        ("f64", 256, 128, 4097, 33),       # the last partition holds one tap
        ("f32", 256, 128, 8065, 0),        # P - 1 + H = 8192 floats
        ("f32", 256, 128, 8066, 64),
        ("f64", 4096, 2048, 2049, 0),      # F = 4096 = 2 H either side of the switch
        ("f64", 4096, 2048, 2050, 2),      # two partitions
        ("f64", 128, 64, 4034, 64)]        # many short partitions (P - 1 + H = 4097)


@pytest.mark.parametrize("dtype,N,H,rir_len,n_part", LONG)
def test_segment_to_partitioned_switch(dtype, N, H, rir_len, n_part):
    """The form that ran shows in the length of the input history: (n_part + 1) H samples when partitioned, P - 1 + H otherwise
    (as test_stream_partitioned_convolution).  Partitioned: process_signal over five hops equals the hop loop bit for bit."""
    from ap_vast_unofficial_amd.apvast import apvast
    L, M = 1, 2
    ap, orc = k1_run(N, H, rir_len, L, M, dtype)
    if n_part:
        assert n_part == -(-rir_len // H)
        assert history_samples(ap) == (n_part + 1) * H
    else:
        assert history_samples(ap) == rir_len - 1 + H
    if n_part:
        rirA, rirB = synth_rirs(rir_len, L, M, 11)
        b = apvast(N, rirA, rirB, 16, 0, 0, 0, 1, 1.0, 4 * N, hop_size=H, perceptual=False, seed=9, dtype=dtype)
        b.set_state(ap.get_state())
        x = np.random.default_rng(4).standard_normal((2, 5 * H))
        ref = [ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(5)]
        sig = b.process_signal(x[0], x[1])
        for q in range(4):
            assert np.array_equal(np.concatenate([r[q][0] for r in ref]), sig[q][0]), q
        sa, sb = ap.get_state(), b.get_state()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
        b.close()
    ap.close()

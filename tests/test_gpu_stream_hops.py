"""The subband stream at hops other than block_size / 2, against the float64 oracle.

Every ring kernel bakes ring_off = (ring_off + H) mod N in (the K1 stores, the input update, the analysis jobs, rows_copy, the state
getters), and the hop's launches are replayed from one captured hipGraph per phase: N / gcd(N, H) phases, doubled when odd, cached
up to 16 and launched eagerly beyond (stream.hip, end of apv_stream_init).  At H = N / 2 there are two phases and ring_off is 0 or
N / 2; here: more phases, an odd count, the largest cached count, the eager path, hops that do not divide N, odd hops (ring_off
odd: no float4 stores in fir_mfma_kernel), N % 4 != 0, H = N and H = 1.  The rings are compared after EVERY hop, so a ring written
or unrotated at the wrong offset in any phase shows.  Tolerances: test_gpu_stream.TOL, unchanged.
No state array tells whether a hop was replayed from a graph or launched eagerly, and a failed capture falls back to eager
launches silently (run_hop): "cached" and "eager" below say what apv_stream_init chooses for the geometry, not something asserted.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_stream import TOL, _hop_loop, check_last_hop_state, check_outputs, run_pair, synth_rirs  # noqa: E402

L, M, P, V = 3, 5, 21, 2

# (N, H, hops): 2 period + 2 hops where the graphs are cached (every captured graph is replayed at least once), else ceil(N / H) + 3
GEOMETRY = [(64, 16, 10),       # period 4
            (96, 32, 14),       # odd period 3, doubled to 6
            (128, 8, 34),       # period 16, the largest cached
            (136, 8, 20),       # period 17 -> 34: eager (and N / 2 = 68 = 4 * 17: Bluestein transforms)
            (96, 36, 18),       # H does not divide N, period 8
            (250, 100, 22),     # N % 4 != 0, period 5 -> 10
            (64, 37, 5),        # odd hop, eager
            (64, 62, 5),        # H just under N, eager
            (64, 64, 6),        # H == N: no overlap, period 1 -> 2
            (32, 1, 35)]        # one-sample hop, eager


def check_rings(ap, orc, tol_spec, where, inputs=True):
    """The four response rings, the two target rings and (inputs) the input-block ring as the state getters hand them out, in
    logical order, against the oracle's: each whole ring to tol_spec of its largest reference value.  Returns the worst error
    ratio, which a measuring run records (profiles/stream_hop_geometry.md says how)."""
    e = ap._eng
    N, nL, nM = ap.block_size, ap.number_of_srcs, ap.number_of_mics
    C = nL * nM
    pairs = [(f"response{p}", e.get_state(f"response{p}", (C, N), e.s_dtype), orc.response[p].transpose(2, 1, 0).reshape(C, N))
             for p in range(4)]                                                         # channel c = m L + l
    pairs += [(f"target_response{z}", e.get_state(f"target_response{z}", (nM, N), e.s_dtype), orc.target_response[z].T)
              for z in range(2)]
    if inputs:
        pairs.append(("input_block", e.get_state("input_block", (2, N), e.s_dtype), orc.input_block))
    worst = 0.0
    for name, got, ref in pairs:
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= tol_spec, (where, name, err)
        worst = max(worst, err)
    return worst


def run_hops(N, H, rirA, rirB, delay, refA, refB, nV, hops, dtype, run_A=True, run_B=True, inputs=True):
    """run_pair's object and oracle (python dialect: random start rings, so what K1 has not overwritten yet is visible), driven
    hop by hop with the rings compared after every hop."""
    ap, orc, got, exp = run_pair(N, H, rirA, rirB, delay, refA, refB, nV, 1.0, hops=0, run_A=run_A, run_B=run_B, dtype=dtype)
    x = np.random.default_rng(99).standard_normal((2, hops * H))
    for h in range(hops):
        got.append(ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]))
        exp.append(orc.process(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]))
        check_rings(ap, orc, TOL[dtype]["spec"], ("hop", h), inputs=inputs)
    return ap, orc, got, exp


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N,H,hops", GEOMETRY)
def test_hop_geometry_vs_oracle(N, H, hops, dtype):
    rirA, rirB = synth_rirs(P, L, M, 1)
    ap, orc, got, exp = run_hops(N, H, rirA, rirB, 5, 1, 2, V, hops, dtype)
    tol = TOL[dtype]
    check_outputs(got, exp, tol["out"], tol["tgt"])
    check_last_hop_state(ap, orc, tol, N // 2 + 1, L, M)
    assert len(got[0][0]) == V and got[0][0][0].shape == (H, L)
    ap.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("run_A,run_B", [(True, False), (False, True)])
def test_hop_geometry_single_zone(run_A, run_B, dtype):
    """One zone program at (96, 32), six phases: the analysis and solver launches have job tables of their own; K1 still fills
    all six rings."""
    N, H, hops = 96, 32, 14
    rirA, rirB = synth_rirs(P, L, M, 1)
    ap, orc, got, exp = run_hops(N, H, rirA, rirB, 5, 1, 2, V, hops, dtype, run_A=run_A, run_B=run_B)
    tol = TOL[dtype]
    check_outputs(got, exp, tol["out"], tol["tgt"])
    check_last_hop_state(ap, orc, tol, N // 2 + 1, L, M, zones=(0,) if run_A else (1,))
    assert (got[0][0] is None) == (not run_A) and (got[0][1] is None) == (not run_B)
    ap.close()


def _same_samples(ref, got, shape):
    for q in range(4):
        for v in range(len(ref[q])):
            assert got[q][v].shape == ref[q][v].shape == shape, (q, v)
            assert np.array_equal(got[q][v], ref[q][v]), (q, v)


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    for z in "AB":
        assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z)), z
        assert np.array_equal(getattr(a, "lambda_" + z), getattr(b, "lambda_" + z)), z


ODD_GEOMETRY = [(96, 36), (64, 37)]     # period 8 (cached graphs) and an odd hop (eager, ring_off odd)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("rir_len,n_hops", [(21, 33), (70, 33), (70, 1), (70, 16), (70, 17)])
@pytest.mark.parametrize("N,H", ODD_GEOMETRY)
def test_process_signal_equals_hop_loop_any_hop(N, H, rir_len, n_hops, dtype):
    """process_signal against the hop loop, bit for bit (as test_process_signal_equals_hop_loop at H = N / 2).  21 taps: direct K1,
    the hop-by-hop pipeline; 70 taps: one fast-convolution segment, the chunked driver (fir_chunk_spectra_kernel, linear buffers
    of N - H + 16 H samples, rows_copy back into the rings at the ring offset n_hops hops on): 16 hops per chunk, so one hop, one
    full chunk, one chunk and a hop, two chunks and a hop.  Two per-hop calls afterwards: the per-hop path and its graphs carry on
    from the rings, histories and phase the signal left."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(rir_len, L, M, 11)
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, V, 1.0, 4 * N, hop_size=H, seed=3, dtype=dtype, perceptual=False)
    a, b = mk(), mk()
    x = np.random.default_rng(8).standard_normal((2, (n_hops + 2) * H))
    ref = _hop_loop(a, x, 0, n_hops)
    got = list(b.process_signal(x[0, :n_hops * H], x[1, :n_hops * H]))
    _same_samples(ref, got, (n_hops * H, L))
    _same_state(a, b)
    _same_samples(_hop_loop(a, x, n_hops, n_hops + 2), _hop_loop(b, x, n_hops, n_hops + 2), (2 * H, L))
    _same_state(a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N,H", ODD_GEOMETRY)
def test_state_roundtrip_mid_ring(N, H, dtype):
    """test_state_roundtrip with the state taken after three hops of another hop size: ring_off is 12 of 96, or 47 of 64 (odd), in
    the object that hands the state out and 0 in the one that takes it, and their phases differ.  Two more hops are the same
    in every output sample and every state array."""
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 3)
    mk = lambda seed: apvast(N, rirA, rirB, 16, 5, 1, 2, V, 1.0, 4 * N, hop_size=H, seed=seed, dtype=dtype, perceptual=False)
    a, b = mk(5), mk(6)
    x = np.random.default_rng(1).standard_normal((2, 5 * H))
    _hop_loop(a, x, 0, 3)
    b.set_state(a.get_state())
    for h in range(3, 5):
        _same_samples(_hop_loop(a, x, h, h + 1), _hop_loop(b, x, h, h + 1), (H, L))
        _same_state(a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_captured_phases_equal_eager_launches(dtype, monkeypatch):
    """(96, 32): six captured graphs, each replayed at least once, against the same hops launched eagerly (APV_NO_GRAPH)."""
    from ap_vast_unofficial_amd.apvast import apvast
    N, H, hops = 96, 32, 14
    rirA, rirB = synth_rirs(P, L, M, 1)
    mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, V, 1.0, 4 * N, hop_size=H, seed=3, dtype=dtype, perceptual=False)
    x = np.random.default_rng(8).standard_normal((2, hops * H))
    a = mk()
    monkeypatch.setenv("APV_NO_GRAPH", "1")
    b = mk()                                         # read once, when the stream is set up
    monkeypatch.delenv("APV_NO_GRAPH")
    for h in range(hops):
        _same_samples(_hop_loop(a, x, h, h + 1), _hop_loop(b, x, h, h + 1), (H, L))
    _same_state(a, b)
    a.close()
    b.close()

"""Block sizes whose half has a prime factor above 7 (the MATLAB demo's blockSize = 1020 = 4 * 3 * 5 * 17, main.m:37): the
transforms take the Bluestein (chirp-z) form, and every layer above them -- the per-hop and chunked analyses, synthesis,
the broadband filter spectra, both front ends -- must work as at 7-smooth sizes, against the same oracles."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from oracle import subband  # noqa: E402  (checker only)
from oracle.subband_stream import SubbandStreamOracle  # noqa: E402  (checker only)

# tolerances of tests/test_gpu_stream.py (see there)
TOL = {
    "f64": dict(spec=1e-13, w_med=1e-10, w_max=1e-7, lam=1e-9, out=1e-9, tgt=1e-11),
    "mixed": dict(spec=1e-6, w_med=5e-5, w_max=1e-2, lam=3e-4, out=5e-5, tgt=1e-5),
}


def synth_rirs(P, L, M, seed):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(P) / (P / 6.0))[:, None, None]
    return (rng.standard_normal((P, L, M)) * env * 1e-3, rng.standard_normal((P, L, M)) * env * 1e-3)


def run_pair(block, hop, rirA, rirB, delay, refA, refB, V, hops, dtype="f64", seed=0):
    from ap_vast_unofficial_amd.apvast import apvast
    P, L, M = rirA.shape
    ap = apvast(block, rirA, rirB, 16, delay, refA, refB, V, 1.0, 4 * block, hop_size=hop, perceptual=False, seed=seed,
                dtype=dtype)
    rs = np.random.RandomState(seed)
    init_r = np.stack([1e-3 * rs.randn(block, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(block, M) for _ in range(2)])
    orc = SubbandStreamOracle(block, rirA, rirB, delay, refA, refB, list(range(1, V + 1)), 1.0, hop_size=hop,
                              init_response=init_r, init_target_response=init_t)
    x = np.random.default_rng(99).standard_normal((2, hops * hop))
    got, exp = [], []
    for h in range(hops):
        got.append(ap.process_input_buffers(x[0, h * hop:(h + 1) * hop], x[1, h * hop:(h + 1) * hop]))
        exp.append(orc.process(x[0, h * hop:(h + 1) * hop], x[1, h * hop:(h + 1) * hop]))
    return ap, orc, got, exp


def check_outputs(got, exp, tol, tol_target):
    for q in range(4):
        scale = max(max(np.abs(e[q]).max() for e in exp), 1e-30)
        t = tol if q < 2 else tol_target
        for h, (g, e) in enumerate(zip(got, exp)):
            ref = e[q] if q < 2 else np.broadcast_to(e[q], (len(g[q]),) + e[q].shape)
            err = np.abs(np.stack(g[q]) - ref).max()
            assert err <= t * scale, (h, q, err / scale)


def check_last_hop_state(ap, orc, tol, K, L, M):
    e = ap._eng
    for p in range(4):
        X = e.get_state(f"spectra{p}", (K, M, L), e.sc_dtype)
        ref = orc.spectra[p].transpose(0, 2, 1)
        assert np.abs(X - ref).max() <= tol["spec"] * np.abs(ref).max(), (p, np.abs(X - ref).max() / np.abs(ref).max())
    for z in (0, 1):
        name = "AB"[z]
        w, wr = getattr(ap, "w_" + name), orc.w[z].transpose(1, 0, 2)
        err = np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
        assert np.median(err) < tol["w_med"] and err.max() < tol["w_max"], (name, np.median(err), err.max())
        lam, lr = getattr(ap, "lambda_" + name), orc.lam[z]
        V = w.shape[0]
        assert (np.abs(lam[:, :V] - lr[:, :V]).max(axis=1) / lr[:, 0]).max() < tol["lam"], name


ROUNDTRIP = [(N, H) for N in (22, 34, 508, 1018, 1020, 2040, 4078, 4094) for H in (N // 2, N // 4) if N % 4 == 0 or H == N // 2]


@pytest.mark.parametrize("N,H", ROUNDTRIP)
def test_stft_roundtrip_any_even_block(N, H):
    """Analysis and synthesis + OLA (apvast.py:246-255, 265-293) against numpy.fft at the bounds of the 7-smooth sizes."""
    from ap_vast_unofficial_amd import Engine
    rng = np.random.default_rng(N)
    n_ch = 19
    x = rng.standard_normal((n_ch, N)).astype(np.float32)
    eng = Engine(1, 4, 4, block_size=N, hop_size=H)
    spec = eng.stft_analysis(x)
    win = subband.sine_window(N)
    ref = subband.analysis(x.T.astype(np.float64), win).T
    assert np.abs(spec - ref).max() < 2e-6 * np.abs(ref).max()
    ov = rng.standard_normal((n_ch, N)).astype(np.float32)
    spec_in = (ref * (1.0 + 0.1j)).astype(np.complex64)
    ov_new, out = eng.istft_ola(spec_in, ov)
    eng.close()
    ov_ref = subband.synthesis_ola(spec_in.T.astype(np.complex128), win, ov.T.astype(np.float64), H).T
    assert np.abs(ov_new - ov_ref).max() < 3e-6 * np.abs(ov_ref).max()
    assert np.abs(out - ov_ref[:, :H]).max() < 3e-6 * np.abs(ov_ref).max()


@pytest.mark.parametrize("dtype", ["f64", "mixed"])
@pytest.mark.parametrize("N,H,L,M,P", [(1020, 510, 16, 32, 200),     # the order-16 kernel, K = 511
                                       (1018, 509, 4, 8, 90),
                                       (4094, 2047, 2, 4, 90)])       # M = 4096: 64 KB of LDS per double-precision transform
def test_stream_any_block_vs_oracle(dtype, N, H, L, M, P):
    rirA, rirB = synth_rirs(P, L, M, 5)
    ap, orc, got, exp = run_pair(N, H, rirA, rirB, 7, 1, 0, 2, hops=5, dtype=dtype)
    tol = TOL[dtype]
    check_last_hop_state(ap, orc, tol, N // 2 + 1, L, M)
    check_outputs(got, exp, tol["out"], tol["tgt"])
    ap.close()


def test_stream_long_response_non_smooth_hop_takes_direct_form():
    """P - 1 + H > 4096: the partitioned form would take segments of F = 2 H = 1020, which is not 7-smooth; the direct form runs."""
    rirA, rirB = synth_rirs(5000, 2, 4, 31)
    N, H = 1020, 510
    ap, orc, got, exp = run_pair(N, H, rirA, rirB, 5, 1, 0, 2, hops=5)
    n_part = -(-5000 // H)
    assert ap._eng.state_bytes("input_history0") != (n_part + 1) * H * 8
    check_last_hop_state(ap, orc, TOL["f64"], N // 2 + 1, 2, 4)
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    ap.close()


_SIGNAL = """
import sys, numpy as np
sys.path.insert(0, %r)
from ap_vast_unofficial_amd.apvast import apvast
dtype, L = %r, %d
rng = np.random.default_rng(5)
env = np.exp(-np.arange(200) / (200 / 6.0))[:, None, None]
rirA, rirB = (rng.standard_normal((200, 16, 32))[:, :L] * env * 1e-3 for _ in range(2))
N, H, n_hops = 1020, 510, 19
mk = lambda: apvast(N, rirA, rirB, 16, 5, 1, 2, 2, 1.0, 4 * N, hop_size=H, seed=3, dtype=dtype, perceptual=False)
a, b = mk(), mk()
x = np.random.default_rng(8).standard_normal((2, n_hops * H))
outs = [a.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H]) for h in range(n_hops)]
got = b.process_signal(x[0], x[1])
for q in range(4):
    for v in range(2):
        assert np.array_equal(np.concatenate([o[q][v] for o in outs]), got[q][v]), (q, v)
sa, sb = a.get_state(), b.get_state()
for k in sa:
    assert np.array_equal(sa[k], sb[k]), k
for z in "AB":
    assert np.array_equal(getattr(a, "w_" + z), getattr(b, "w_" + z))
print("SIGNAL_OK")
"""


@pytest.mark.parametrize("batched", ["1", "0"])
@pytest.mark.parametrize("dtype", ["f64", "mixed"])
def test_process_signal_equals_hop_loop_1020(dtype, batched):
    """The whole-signal path (chunked analyses, chunk-wide K1 spectra, batched or per-hop diagonalisations) returns the hop
    loop's samples bit for bit at N = 1020.  batched = "1": 16 loudspeakers, the chunk's joint diagonalisations in one launch;
    "0": the same responses cut to 8 loudspeakers, an order the batched launch does not take, hop by hop on the back streams.
    Each case runs in a child process."""
    L = 16 if batched == "1" else 8
    r = subprocess.run([sys.executable, "-c", _SIGNAL % (ROOT, dtype, L)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SIGNAL_OK" in r.stdout, r.stdout + r.stderr


def _bb_matlab(rirs):
    from ap_vast_unofficial_amd.apvast import apvast
    return apvast(1020, rirs["rirA"], rirs["rirB"], 40, 5, 1, 1, [1, 160, 320], 1.0, 1020, sampling_rate=8000,
                  perceptual=True, mode="broadband", dialect="matlab", fullscale_db_spl=94.0)


def test_broadband_matlab_main_m_construction(golden):
    """main.m:36-45 scaled to the bundled 800-tap, 8 x 8 responses: N = 1020, J = 40 (modelling delay J / 8 as there), ranks
    1, J L / 2 and J L, perceptual weighting at 94 dB full scale and 8 kHz, against the restatement of apVast.m from shared small noise (see
    test_broadband_matlab_dialect_vs_oracle); process_signal against its own hop loop."""
    from oracle.broadband_matlab import MatlabBroadbandOracle
    from oracle.perceptual import Model
    rirs = golden("rirs_cfg1")
    ranks = [1, 160, 320]
    ap = _bb_matlab(rirs)
    orc = MatlabBroadbandOracle(1020, rirs["rirA"], rirs["rirB"], 40, 5, 1, 1, ranks, 1.0, 1020, sampling_rate=8000,
                                model=Model(1020, 8000, 94.0))
    rng = np.random.default_rng(21)
    orc.response[:] = 1e-3 * rng.standard_normal(orc.response.shape)
    orc.target_response[:] = 1e-3 * rng.standard_normal(orc.target_response.shape)
    start = {"response": orc.response.copy(), "target_response": orc.target_response.copy()}
    ap.set_state(start)
    H = ap.hop_size
    x = np.random.default_rng(8).standard_normal((2, 3 * H))
    per_hop = []
    for h in range(3):
        got = ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        exp = orc.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        per_hop.append(got)
        for q in range(4):
            e = exp[q]
            assert np.abs(np.stack(got[q]) - e).max() <= 1e-6 * max(np.abs(e).max(), 1e-30), (h, q)
    for i in range(len(ranks)):
        assert np.linalg.norm(ap.w_A[i, :, 0] - orc.w_A[i]) <= 1e-6 * np.linalg.norm(orc.w_A[i]), i
    # the whole-signal call from the same start, at the hop loop's bound of tests/test_gpu_broadband.py (its joint
    # diagonalisations are solved as one batch)
    b = _bb_matlab(rirs)
    b.set_state(start)
    whole = b.process_signal(x[0], x[1])
    for q in range(4):
        for v in range(len(ranks)):
            ref = np.concatenate([per_hop[h][q][v] for h in range(3)])
            assert np.abs(whole[q][v] - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-30), (q, v)
    ap.close()
    b.close()


def test_broadband_python_dialect_1020(golden):
    from ap_vast_unofficial_amd.apvast import apvast
    from oracle.broadband import BroadbandOracle
    rirs = golden("rirs_cfg1")
    rA, rB = rirs["rirA"][:, :4, :6], rirs["rirB"][:, :4, :6]
    N, J, S, V = 1020, 40, 1020, 4
    ap = apvast(N, rA, rB, J, 8, 1, 2, V, 1.0, S, perceptual=False, mode="broadband", seed=4)
    np.random.seed(4)
    orc = BroadbandOracle(N, rA, rB, J, 8, 1, 2, V, 1.0, S)
    H = ap.hop_size
    x = np.random.default_rng(8).standard_normal((2, 3 * H))
    for h in range(3):
        got = ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        exp = orc.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        for q in range(4):
            e = exp[q]
            assert np.abs(np.stack(got[q]) - e).max() <= 1e-7 * max(np.abs(e).max(), 1e-30), (h, q)
    assert np.abs(ap.lambda_A[:V] / orc.lambda_A[:V] - 1).max() < 1e-8
    ap.close()


def test_block_size_refusals():
    """Odd sizes stay refused; above 4096 N/2 must still be 7-smooth (8190 = 2 * 9 * 5 * 7 * 13), and 8198 is out of range;
    8192 works."""
    from ap_vast_unofficial_amd import Engine
    from ap_vast_unofficial_amd.apvast import apvast
    r = np.random.default_rng(0).standard_normal((20, 2, 2)) * 1e-3
    with pytest.raises(RuntimeError, match="block size must be modulo 2"):
        apvast(1021, r, r, 16, 5, 1, 0, 1, 1.0, 4096, perceptual=False)
    for N in (8190, 8198):
        with pytest.raises(RuntimeError, match="above 4096, N/2 must factor into 2, 3, 5 and 7"):
            apvast(N, r, r, 16, 5, 1, 0, 1, 1.0, 4 * N, perceptual=False, dtype="f32")
        eng = Engine(1, 4, 4, block_size=N, hop_size=N // 2)
        with pytest.raises(RuntimeError, match="above 4096"):
            eng.stft_analysis(np.zeros((1, N), np.float32))
        eng.close()
    ap = apvast(8192, r, r, 16, 5, 1, 0, 1, 1.0, 4 * 8192, perceptual=False, dtype="f32")
    out = ap.process_input_buffers(np.ones(4096), np.ones(4096))
    assert np.isfinite(np.stack(out[0])).all()
    ap.close()

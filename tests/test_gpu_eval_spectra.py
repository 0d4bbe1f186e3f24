"""Per-bin evaluation spectra of the subband stream (apvast(..., evaluation_spectra=True), apv_stream_set_evaluation_spectra,
apv_eval_spectrum_step, csrc/kernels_evalspec.hip): the three launches against the NumPy restatement of
tests/eval_spectra_oracle.py, which also derives the bound every element is held to:

    |got - ref| <= 4 c(N) u N sum_t ||w f_t[:, m]||_2^2,   c(N) = 8 (log2 N + 2), three times that with log2 M for Bluestein sizes

(4 c(N) N u stays below 1e-11 at every size tested here).  The stream tests feed the helper with the device's own per-hop
predicted_pressure(), which separates this stage from the pressure kernel."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from eval_spectra_oracle import KEYS, SpectraReference, bound_factor, check, stack_sets  # noqa: E402
from oracle.subband import sine_window  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import L, M, P, V, DELAY, REF_A, REF_B, make, signal  # noqa: E402

NH = [(32, 16), (60, 20), (68, 34), (32, 12), (36, 10), (32, 32)]
ZEM = [(1, 1, 1), (2, 2, 5), (2, 1, 17), (1, 3, 33)]


def split_totals(t, E):
    """(Z, 3 E + 1, K, Mv) as the device keeps them -> the dict of (Z, E, Mv, K) / (Z, Mv, K)"""
    t = t.transpose(0, 1, 3, 2)
    return {"bright": t[:, :E], "dark": t[:, E:2 * E], "error": t[:, 2 * E:3 * E], "target": t[:, 3 * E]}


def logical(ring, off):
    """(sets, Mv, N) as stored -> (sets, N, Mv), oldest sample first"""
    return np.roll(ring, -off, axis=2).transpose(0, 2, 1)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h", NH)
def test_kernel_against_numpy(n, h):
    """consecutive steps from a zero ring, past one period of the ring offset; then the same steps on guard-padded buffers"""
    from ap_vast_unofficial_amd._capi import Engine
    assert bound_factor(n) < 1e-11
    eng = Engine(9, 4, 4)
    steps = max(6, n // np.gcd(n, h) + 2)
    worst, pad = [0.0], 64
    for Z, E, Mv in ZEM:
        rng = np.random.default_rng(1000 * n + 10 * h + Mv)
        sets, K = Z * (2 * E + 1), n // 2 + 1
        ps = rng.standard_normal((steps, sets, h, Mv))
        ref = SpectraReference(n, h, Z, E, Mv)
        ring, tot, off = np.zeros((sets, Mv, n)), np.zeros((Z, 3 * E + 1, K, Mv)), 0
        for t in range(steps):
            off = (off + h) % n
            ring, tot = eng.eval_spectrum_step(ps[t], ring, off, tot, Z, E)
            ref.hop(ps[t].reshape(Z, 2 * E + 1, h, Mv))
            assert np.array_equal(logical(ring, off), ref.ring.reshape(sets, n, Mv)), (Z, E, Mv, t)
            check(split_totals(tot, E), ref, worst)
        # canaries in front of and behind the ring, the totals and the pressures; everything stays on the device between the steps
        gr, gt = np.full(pad + ring.size + pad, -777.0), np.full(pad + tot.size + pad, -777.0)
        gr[pad:-pad] = 0.0
        gt[pad:-pad] = 0.0
        dr, dt = eng.to_device(gr), eng.to_device(gt)
        gp = np.full(pad + ps[0].size + pad, -777.0)
        inner = lambda d: ctypes.c_void_p(d.ptr.value + pad * 8)
        off = 0
        for t in range(steps):
            off = (off + h) % n
            gp[pad:-pad] = ps[t].ravel()
            dp = eng.to_device(gp)
            eng._chk(eng.lib.apv_eval_spectrum_step(eng.h, inner(dp), inner(dr), off, n, h, Z, E, Mv, inner(dt)))
            back = dp.download(gp.shape, np.float64)
            assert np.array_equal(back, gp)
            dp.free()
        br, bt = dr.download(gr.shape, np.float64), dt.download(gt.shape, np.float64)
        for b in (br, bt):
            assert np.all(b[:pad] == -777.0) and np.all(b[-pad:] == -777.0)
        assert np.array_equal(br[pad:-pad].reshape(ring.shape), ring)           # and the bits do not depend on the buffer
        assert np.array_equal(bt[pad:-pad].reshape(tot.shape), tot)
        dr.free()
        dt.free()
    print(f"N={n} H={h}: largest error / bound {worst[0]:.4f}")
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k0", [(32, 1), (32, 7), (32, 14), (60, 11), (68, 5)])
def test_known_answer_half_bin_cosine(n, k0):
    """p[n] = cos(2 pi (k0 + 1/2) n / N) on every bright channel, dark and target zero, H = N/2: under the sine window
    w f = [sin(2 pi (k0 + 1) i / N) - sin(2 pi k0 i / N)] / 2, so a full frame adds N^2 / 16 to bins k0 and k0 + 1 and nothing
    elsewhere; error equals bright, target is zero exactly"""
    from ap_vast_unofficial_amd._capi import Engine
    eng = Engine(9, 4, 4)
    Z, E, Mv, h, steps = 2, 2, 5, n // 2, 6
    sets, K = Z * (2 * E + 1), n // 2 + 1
    x = np.cos(2 * np.pi * (k0 + 0.5) * np.arange(steps * h) / n)
    ring, tot, off = np.zeros((sets, Mv, n)), np.zeros((Z, 3 * E + 1, K, Mv)), 0
    for t in range(steps):
        p = np.zeros((Z, 2 * E + 1, h, Mv))
        p[:, :E] = x[t * h:(t + 1) * h, None]
        off = (off + h) % n
        if t == steps - 1:
            tot[:] = 0.0                                  # the last step's increment alone
        ring, tot = eng.eval_spectrum_step(p.reshape(sets, h, Mv), ring, off, tot, Z, E)
    got = split_totals(tot, E)
    frame = x[(steps - 2) * h:]
    assert np.allclose(sine_window(n) * frame, 0.5 * (np.sin(2 * np.pi * (k0 + 1) * np.arange(n) / n)
                                                       - np.sin(2 * np.pi * k0 * np.arange(n) / n)), rtol=0, atol=1e-13)
    bound = bound_factor(n) * np.sum((sine_window(n) * frame) ** 2)
    exp = np.zeros(K)
    exp[k0] = exp[k0 + 1] = n * n / 16.0
    share = np.abs(got["bright"] - exp).max() / bound
    print(f"N={n} k0={k0}: largest error / bound {share:.4f}")
    assert np.all(np.abs(got["bright"] - exp) <= bound)
    assert np.array_equal(got["error"], got["bright"])
    assert np.all(got["dark"] == 0.0) and np.all(got["target"] == 0.0)
    eng.close()


# 3 ---------------------------------------------------------------------------------------------------------------
def run_stream(ap, x, hops, h, Z, E, Mv, n):
    """`hops` hops through process_input_buffers; the helper fed with the device's own pressures"""
    ref = SpectraReference(n, h, Z, E, Mv)
    outs = []
    for k in range(hops):
        outs.append(hop(ap, x, k, h))
        ref.hop(stack_sets(ap.predicted_pressure()))
    return ref, outs


@pytest.mark.parametrize("run_A,run_B", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
@pytest.mark.parametrize("fir", [False, True])
@pytest.mark.parametrize("n,h", [(32, 16), (60, 20), (68, 34), (32, 12), (36, 10)])
def test_stream_against_helper(n, h, fir, dtype, run_A, run_B):
    """evaluation_ranks None and [1, 3]; eight hops hop by hop and through process_signal, which must agree bit for bit.
    (36, 10) has a period of 18 hops: no captured graphs"""
    assert bound_factor(n) < 1e-11
    Z, Mv, K, hops = int(run_A) + int(run_B), 5, n // 2 + 1, 8
    x = signal(hops, h)
    worst = [0.0]
    for ranks in (None, [1, 3]):
        E = V if ranks is None else len(ranks)
        kw = dict(dtype=dtype, fir=fir, run_A=run_A, run_B=run_B, N=n, H=h, Pv=9, Mv=Mv, ranks=ranks, evaluation_spectra=True)
        a, b = make(**kw), make(**kw)
        assert a.evaluation_spectra() is None
        ref, outs = run_stream(a, x, hops, h, Z, E, Mv, n)
        got = a.evaluation_spectra()
        for k in ("bright", "dark", "error"):
            assert got[k].shape == (Z, E, Mv, K) and got[k].dtype == np.float64
        assert got["target"].shape == (Z, Mv, K)
        check(got, ref, worst)
        sig = b.process_signal(x[0], x[1])
        assert b.signal_schedule == (0, hops)
        for q in range(4):
            if sig[q] is not None:
                for v in range(V):
                    assert np.array_equal(sig[q][v], np.concatenate([o[q][v] for o in outs])), (q, v)
        gb = b.evaluation_spectra()
        for k in KEYS:
            assert np.array_equal(gb[k], got[k]), k
        a.close()
        b.close()
    print(f"N={n} H={h} fir={fir} {dtype} A={run_A} B={run_B}: largest error / bound {worst[0]:.4f}")


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n,h", [(32, 16), (60, 20), (32, 8)])
def test_parseval_without_an_fft(n, h, dtype):
    """N / H an integer >= 2: sum_k c_k S[..., m, k] / N = sum_n g[n] p[n, m]^2, g[n] the sum of w^2 over the frames that cover
    sample n (N / (2 H) everywhere but the last N - H samples); the right side in NumPy from the recorded pressures"""
    hops, Mv = 8, 5
    ap = make(dtype=dtype, N=n, H=h, Pv=9, Mv=Mv, ranks=[1, 3], evaluation_spectra=True)
    x = signal(hops, h)
    rec = []
    for k in range(hops):
        hop(ap, x, k, h)
        rec.append(stack_sets(ap.predicted_pressure()))
    p = np.concatenate(rec, axis=2)                       # (Z, 2 E + 1, hops H, Mv)
    w2 = sine_window(n) ** 2
    g = np.zeros(hops * h)
    for t in range(hops):
        start = (t + 1) * h - n
        lo = max(start, 0)
        g[lo:(t + 1) * h] += w2[lo - start:]
    assert np.allclose(g[:hops * h - (n - h)], n / (2.0 * h), rtol=1e-12, atol=0)
    E = 2
    sets = {"bright": p[:, :E], "dark": p[:, E:2 * E], "target": p[:, 2 * E]}
    sets["error"] = sets["target"][:, None] - sets["bright"]
    got = ap.evaluation_spectra()
    ck = np.full(n // 2 + 1, 2.0)
    ck[0] = ck[-1] = 1.0
    worst = 0.0
    for k in KEYS:
        rhs = np.sum(g[:, None] * sets[k] ** 2, axis=-2)  # = sum_t ||w f_t||^2 as well
        lhs = np.sum(ck * got[k], axis=-1) / n
        assert lhs.shape == rhs.shape
        worst = max(worst, (np.abs(lhs - rhs) / (bound_factor(n) * rhs)).max())
        assert np.all(np.abs(lhs - rhs) <= bound_factor(n) * rhs), (k, worst)
    print(f"N={n} H={h} {dtype}: Parseval, largest error / bound {worst:.4f}")
    ap.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h", [(32, 16), (32, 12)])
def test_state_resume_and_reset(n, h):
    kw = dict(N=n, H=h, Pv=9, Mv=5, ranks=[1, 3], evaluation_spectra=True)
    a, b = make(**kw), make(**kw)
    Z, E, Mv, K = 2, 2, 5, n // 2 + 1
    x = signal(8, h)
    rec = []
    for k in range(8):
        hop(a, x, k, h)
        rec.append(stack_sets(a.predicted_pressure()))
        if k == 4:
            st = a.get_state()
            assert st["evaluation_spectra"].shape == (Z, 3 * E + 1, K, Mv) and st["evaluation_ring"].shape == (Z, 2 * E + 1, Mv, n)
            # the ring holds the last N samples, oldest first
            last = np.concatenate([np.zeros_like(rec[0])] * (n // h + 1) + rec, axis=2)[:, :, -n:]
            assert np.array_equal(st["evaluation_ring"], last.transpose(0, 1, 3, 2))
            b.set_state(st)
    for k in range(5, 8):
        hop(b, x, k, h)
    ga, gb = a.evaluation_spectra(), b.evaluation_spectra()
    for k in KEYS:
        assert np.array_equal(ga[k], gb[k]), k
    sa, sb = a.get_state(), b.get_state()
    for k in ("evaluation_spectra", "evaluation_ring"):
        assert np.array_equal(sa[k], sb[k]), k
    # reset: three more hops give the last three frames' own energies from a zero ring
    a.reset_evaluation()
    assert not a.get_state()["evaluation_ring"].any() and not a.get_state()["evaluation_spectra"].any()
    ref = SpectraReference(n, h, Z, E, Mv)
    for k in range(3):
        hop(a, x, k, h)
        ref.hop(stack_sets(a.predicted_pressure()))
    share = check(a.evaluation_spectra(), ref)
    print(f"N={n} H={h}: after reset, largest error / bound {share:.4f}")
    for key, shape in (("evaluation_spectra", (Z, 3 * E + 1, Mv, K)), ("evaluation_ring", (Z, 2 * E + 1, n, Mv))):
        with pytest.raises(ValueError, match=key):
            b.set_state({key: np.zeros(shape)})
    plain = make(N=n, H=h, Pv=9, Mv=5, ranks=[1, 3])
    assert "evaluation_spectra" not in plain.get_state() and "evaluation_ring" not in plain.get_state()
    with pytest.raises(KeyError):
        plain.set_state({"evaluation_ring": sa["evaluation_ring"]})
    with pytest.raises(RuntimeError):
        plain.evaluation_spectra()
    for o in (a, b, plain):
        o.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nothing_else_moves(dtype):
    """outputs, w_*, lambda_*, evaluation_totals(), evaluation_hops(), predicted_pressure() and signal_schedule of a stream with
    the keyword equal those of the same stream without, six hops"""
    a, b = make(dtype, Pv=9, Mv=5, evaluation_spectra=True), make(dtype, Pv=9, Mv=5)
    x = signal(6, 16)
    for k in range(6):
        same_outputs(hop(a, x, k, 16), hop(b, x, k, 16))
        for name in ("w_A", "w_B", "lambda_A", "lambda_B"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), (k, name)
        for f in ("evaluation_totals", "evaluation_hops", "predicted_pressure"):
            da, db = getattr(a, f)(), getattr(b, f)()
            for q in da:
                assert np.array_equal(da[q], db[q]), (k, f, q)
        assert a.signal_schedule == b.signal_schedule
    sa, sb = a.get_state(), b.get_state()
    assert sorted(set(sa) - set(sb)) == ["evaluation_ring", "evaluation_spectra"]
    for k in sb:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k
    a.close()
    b.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from ap_vast_unofficial_amd import _capi
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = (np.ascontiguousarray(r, dtype=np.float64) for r in synth_rirs(P, L, M, 1))
    rv = np.ones((5, L, 2))
    mk = lambda **kw: apvast(32, rirA, rirB, 8, DELAY, REF_A, REF_B, V, 1.0, 128, hop_size=16, perceptual=False, seed=0, **kw)
    with pytest.raises(ValueError, match="needs validation_rir_A"):
        mk(evaluation_spectra=True)
    with pytest.raises(ValueError, match="a subband keyword"):
        mk(evaluation_spectra=True, mode="broadband")
    with pytest.raises(ValueError, match="must be a bool"):
        mk(evaluation_spectra=1, validation_rir_A=rv, validation_rir_B=rv)
    # the C setter: values, after init, and init without the evaluation stage
    eng = _capi.Engine(17, L, M, ranks=(1, 3), block_size=32, hop_size=16)
    s = eng.lib.apv_stream_set_evaluation_spectra
    assert s(eng.h, 2) == _capi.ERR_ARG and s(eng.h, -1) == _capi.ERR_ARG
    assert s(eng.h, 1) == _capi.OK
    assert eng.lib.apv_stream_init(eng.h, P, _capi._ptr(rirA), _capi._ptr(rirB), REF_A, REF_B, DELAY) == _capi.ERR_ARG
    assert b"apv_stream_set_evaluation" in eng.lib.apv_last_error(eng.h)
    eng.set_evaluation(rv, rv, [1, 3])
    eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    assert s(eng.h, 0) == _capi.ERR_ARG and s(eng.h, 1) == _capi.ERR_ARG      # after apv_stream_init
    assert eng.state_bytes("eval_spectra") == 1 * 7 * 17 * 2 * 8
    assert eng.state_bytes("eval_ring") == 1 * 5 * 2 * 32 * 8
    eng.close()
    plain = _capi.Engine(17, L, M, ranks=(1, 3), block_size=32, hop_size=16, evaluation=(rv, rv, [1, 3]))
    plain.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    for name in ("eval_spectra", "eval_ring"):
        with pytest.raises(_capi.ApvError):
            plain.state_bytes(name)
    # the kernel-level entry
    d = plain.alloc(1 << 16)
    f = plain.lib.apv_eval_spectrum_step
    good = dict(p=d.ptr, ring=d.ptr, off=0, N=32, H=16, Z=1, E=1, Mv=2, tot=d.ptr)
    call = lambda **kw: f(plain.h, *[{**good, **kw}[k] for k in ("p", "ring", "off", "N", "H", "Z", "E", "Mv", "tot")])
    for bad in (dict(p=None), dict(ring=None), dict(tot=None), dict(N=0), dict(H=0), dict(Z=0), dict(E=0), dict(Mv=0), dict(N=-32),
                dict(H=-1), dict(N=31), dict(N=4098), dict(off=-1), dict(off=32), dict(H=33), dict(Z=3)):
        assert call(**bad) == _capi.ERR_ARG, bad
    d.free()
    plain.close()
    # a float32 stream with a block above 4096: refused by apv_stream_init, before anything is allocated or launched
    big = _capi.Engine(4097, L, M, ranks=(1, 3), compute_dtype="f32", block_size=8192, hop_size=4096, evaluation=(rv, rv, [1, 3]),
                       evaluation_spectra=True)
    assert big.lib.apv_stream_init(big.h, P, _capi._ptr(rirA), _capi._ptr(rirB), REF_A, REF_B, DELAY) == _capi.ERR_ARG
    msg = big.lib.apv_last_error(big.h).decode()
    assert "evaluation spectra" in msg and "4096" in msg and "float64" in msg
    big.close()

"""Evaluation stage of the subband stream (apvast(..., validation_rir_A=, validation_rir_B=, evaluation_ranks=),
apv_stream_set_evaluation, apv_eval_pressure, csrc/kernels_streameval.hip): the pressure kernel against NumPy, the stream against
the SciPy helper (tests/evaluation_oracle.py) run on the outputs the calls returned.

Bounds, derived (not measured).  The arithmetic is float64 for every dtype -- float32 samples are widened exactly -- so u = 2^-53
throughout.  A dot product of L Pv terms summed in any order errs by at most about L Pv u S, S = sum_l sum_j |rv| |y|, and the float64
reference carries the same: every pressure sample is held to |got - ref| <= 2 (L Pv + 6) u S.  An energy of H squared samples is
held to (H + 8) u E of the same energy recomputed in float64 from the device's OWN pressures, which separates the reduction from
the convolution.  Totals are the sequential float64 sum of the per-hop records, bit for bit."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from constraint_oracle import ConstrainedSubbandOracle  # noqa: E402
from evaluation_oracle import StreamEvaluation, energy_bound, pressure_bound, window_pressure  # noqa: E402
from fir_synthesis_oracle import FirStreamReference  # noqa: E402
from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import synth_rirs  # noqa: E402

L, M, P, V, J = 3, 4, 12, 3, 8
DELAY, REF_A, REF_B = 3, 1, 2
KEYS = ("bright", "dark", "error", "target")


def validation_rirs(Pv, l, Mv, seed=11):
    rng = np.random.default_rng(seed)
    env = np.exp(-np.arange(Pv) / (Pv / 4.0 + 1.0))[:, None, None]
    return rng.standard_normal((Pv, l, Mv)) * env, rng.standard_normal((Pv, l, Mv)) * env


def make(dtype="f64", fir=False, run_A=True, run_B=True, N=32, H=16, Pv=9, Mv=5, ranks=None, evaluate=True, rv=None, **kw):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 1)
    if fir:
        kw.update(constrain_filter_length=True, synthesis="fir")
    if evaluate:
        rvA, rvB = validation_rirs(Pv, L, Mv) if rv is None else rv
        kw.update(validation_rir_A=rvA, validation_rir_B=rvB, evaluation_ranks=ranks)
    return apvast(N, rirA, rirB, J, DELAY, REF_A, REF_B, V, 1.0, 4 * N, hop_size=H, run_A=run_A, run_B=run_B, perceptual=False,
                  seed=0, dtype=dtype, **kw)


def signal(hops, h, seed=99):
    return np.random.default_rng(seed).standard_normal((2, hops * h))


def check_hop(ap, ref, H, Pv, worst):
    """predicted_pressure() against the helper's hop `ref`, evaluation_hops() against the device's own pressures"""
    p = ap.predicted_pressure()
    for k in ("bright", "dark", "target"):
        err, S = np.abs(p[k] - ref[k]), ref["S_" + k]
        assert p[k].shape == ref[k].shape
        if (S > 0).any():
            worst[0] = max(worst[0], (err[S > 0] / S[S > 0]).max() / pressure_bound(L, Pv))
        assert np.all(err <= pressure_bound(L, Pv) * S), (k, worst)
    eh = ap.evaluation_hops()
    own = {"bright": np.sum(p["bright"] ** 2, axis=2), "dark": np.sum(p["dark"] ** 2, axis=2),
           "error": np.sum((p["target"][:, None] - p["bright"]) ** 2, axis=2), "target": np.sum(p["target"] ** 2, axis=1)}
    for k in KEYS:
        assert eh[k].shape == (1,) + own[k].shape
        err = np.abs(eh[k][0] - own[k])
        if (own[k] > 0).any():
            worst[1] = max(worst[1], (err[own[k] > 0] / own[k][own[k] > 0]).max() / energy_bound(H))
        assert np.all(err <= energy_bound(H) * own[k]), (k, worst)
    return eh


# 1 ---------------------------------------------------------------------------------------------------------------
PVH = [(1, 16), (5, 16), (37, 30), (40, 16), (200, 64), (7, 272)]
LMG = [(3, 1, 1), (16, 17, 4), (70, 33, 2)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("pv,h", PVH)
def test_kernel_against_numpy(pv, h, dtype):
    """no history (Pv = 1), a history longer than the hop, remainder tiles in samples, microphones and loudspeakers, an order above
    64, four sample tiles per workgroup (H = 272); then the same launch into guard-padded buffers"""
    from ap_vast_unofficial_amd._capi import Engine
    eng = Engine(9, 4, 4, compute_dtype=dtype)
    rng = np.random.default_rng(1000 * pv + h)
    worst, pad = 0.0, 256
    for nl, mv, g in LMG:
        y = rng.standard_normal((g, pv - 1 + h, nl)).astype(eng.s_dtype)
        rv = rng.standard_normal((pv, nl, mv))
        got = eng.eval_pressure(y, rv, h)
        assert got.shape == (g, h, mv) and got.dtype == np.float64
        refs = [window_pressure(y[i], rv, h) for i in range(g)]
        ref, S = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
        worst = max(worst, (np.abs(got - ref) / S).max() / pressure_bound(nl, pv))
        assert np.all(np.abs(got - ref) <= pressure_bound(nl, pv) * S), (nl, mv, g, worst)
        # canaries in front of and behind d_p; the inputs end where their last element ends
        dy, dr = eng.to_device(y), eng.to_device(rv)
        buf = np.full(pad + g * h * mv + pad, -777.0)
        dp = eng.to_device(buf)
        inner = ctypes.c_void_p(dp.ptr.value + pad * 8)
        eng._chk(eng.lib.apv_eval_pressure(eng.h, dy.ptr, dr.ptr, g, nl, pv, h, mv, inner))
        back = dp.download(buf.shape, np.float64)
        assert np.all(back[:pad] == -777.0) and np.all(back[-pad:] == -777.0)
        assert np.array_equal(back[pad:-pad].reshape(g, h, mv), got)            # and the bits do not depend on the buffer
        for b in (dy, dr, dp):
            b.free()
    print(f"Pv={pv} H={h} {dtype}: largest pressure error / bound {worst:.3f}")
    eng.close()


def test_kernel_long_response():
    """Pv = 8192: one loudspeaker's window takes 64 KB of LDS and more, the loudspeakers go through one per pass"""
    from ap_vast_unofficial_amd._capi import Engine
    eng = Engine(9, 4, 4)
    rng = np.random.default_rng(8)
    pv, h, nl, mv = 8192, 16, 2, 3
    y = rng.standard_normal((1, pv - 1 + h, nl))
    rv = rng.standard_normal((pv, nl, mv))
    got = eng.eval_pressure(y, rv, h)
    ref, S = window_pressure(y[0], rv, h)
    share = (np.abs(got[0] - ref) / S).max() / pressure_bound(nl, pv)
    print(f"Pv=8192: largest pressure error / bound {share:.3f}")
    assert np.all(np.abs(got[0] - ref) <= pressure_bound(nl, pv) * S)
    eng.close()


def test_entry_refusals():
    from ap_vast_unofficial_amd import _capi
    eng = _capi.Engine(17, L, M, ranks=(1, 3), block_size=32, hop_size=16)
    d = eng.alloc(4096)
    f = eng.lib.apv_eval_pressure
    assert f(eng.h, None, d.ptr, 1, 2, 2, 4, 2, d.ptr) == _capi.ERR_ARG
    assert f(eng.h, d.ptr, None, 1, 2, 2, 4, 2, d.ptr) == _capi.ERR_ARG
    assert f(eng.h, d.ptr, d.ptr, 1, 2, 2, 4, 2, None) == _capi.ERR_ARG
    for bad in ((0, 2, 2, 4, 2), (1, 0, 2, 4, 2), (1, 2, 0, 4, 2), (1, 2, 2, 0, 2), (1, 2, 2, 4, 0), (65536, 2, 2, 4, 2),
                (1, 2, 20466, 4, 2)):                                          # the last: a window LDS cannot hold
        assert f(eng.h, d.ptr, d.ptr, *bad, d.ptr) == _capi.ERR_ARG, bad
    d.free()
    rv = np.ones((5, L, 2))
    s = eng.lib.apv_stream_set_evaluation
    r13, r31, r2, r11 = (np.array(v, dtype=np.int32) for v in ([1, 3], [3, 1], [2], [1, 1]))
    ptr = _capi._ptr
    assert s(eng.h, 5, 2, None, ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), None, 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, None) == _capi.ERR_ARG
    assert s(eng.h, 0, 2, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 0, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 20466, 2, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG     # the window does not fit LDS
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 0, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 3, ptr(r13)) == _capi.ERR_ARG         # more ranks than the handle has
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, ptr(r31)) == _capi.ERR_ARG         # not ascending
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, ptr(r11)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 1, ptr(r2)) == _capi.ERR_ARG          # not in the rank list
    assert eng.lib.apv_stream_reset_evaluation(eng.h) == _capi.ERR_ARG             # no stream
    with pytest.raises(ValueError):
        eng.set_evaluation(np.ones((5, L + 1, 2)), np.ones((5, L + 1, 2)), [1])
    eng.set_evaluation(rv, rv, [1, 3])
    rirA, rirB = synth_rirs(P, L, M, 1)
    eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG         # after apv_stream_init
    assert eng.state_bytes("eval_pressure") == 1 * 5 * 16 * 2 * 8                  # one program, two ranks: 2 * 2 + 1 sets
    assert eng.state_bytes("eval_totals") == 1 * 7 * 2 * 8
    assert eng.state_bytes("eval_history") == 1 * 3 * 4 * L * 8
    assert eng.state_bytes("eval_hops") == 0
    with pytest.raises(_capi.ApvError):
        eng.set_state("eval_pressure", np.zeros((5, 16, 2)))
    eng.close()
    plain = _capi.Engine(17, L, M, block_size=32, hop_size=16)
    plain.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    for name in ("eval_pressure", "eval_hops", "eval_totals", "eval_history"):
        with pytest.raises(_capi.ApvError):
            plain.state_bytes(name)
    assert plain.lib.apv_stream_reset_evaluation(plain.h) == _capi.ERR_ARG
    plain.close()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_A,run_B", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("dtype", ["f64", "mixed", "f32"])
@pytest.mark.parametrize("fir", [False, True])
@pytest.mark.parametrize("n,h", [(32, 16), (60, 20), (68, 34)])
def test_stream_self_consistent(n, h, fir, dtype, run_A, run_B):
    """Pv in {1, 9, 40} (Pv - 1 below, near and above H), Mv in {1, 5}, evaluation_ranks None and [1, V], 5 hops each"""
    worst = [0.0, 0.0]
    x = signal(5, h)
    for pv in (1, 9, 40):
        for mv in (1, 5):
            for ranks in (None, [1, V]):
                ap = make(dtype, fir, run_A, run_B, n, h, pv, mv, ranks)
                assert ap.predicted_pressure() is None and ap.evaluation_hops() is None and ap.evaluation_totals() is None
                rvA, rvB = validation_rirs(pv, L, mv)
                ev = StreamEvaluation(rvA, rvB, ranks or range(1, V + 1), run_A, run_B)
                run = None
                for k in range(5):
                    eh = check_hop(ap, ev.hop(hop(ap, x, k, h)), h, pv, worst)
                    run = {q: eh[q][0] for q in KEYS} if run is None else {q: run[q] + eh[q][0] for q in KEYS}
                    tot = ap.evaluation_totals()
                    for q in KEYS:
                        assert np.array_equal(tot[q], run[q]), (pv, mv, ranks, k, q)
                ap.close()
    print(f"N={n} H={h} fir={fir} {dtype} A={run_A} B={run_B}: largest pressure / energy error over bound {worst[0]:.3f} / {worst[1]:.3f}")


# 3 ---------------------------------------------------------------------------------------------------------------
def same_state(sa, sb):
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k


@pytest.mark.parametrize("fir", [False, True])
def test_process_signal_resume_and_reset_are_bit_for_bit(fir):
    kw = dict(fir=fir, Pv=40, Mv=5, ranks=[1, V])
    a, b, c = make(**kw), make(**kw), make(**kw)
    x = signal(7, 16)
    loop, recs = [], []
    for k in range(7):
        loop.append(hop(a, x, k, 16))
        recs.append(a.evaluation_hops())
        if k == 2:
            c.set_state(a.get_state())                       # resumed after hop 3
    assert "evaluation_history" in a.get_state() and "evaluation_totals" in a.get_state()
    sig = b.process_signal(x[0], x[1])
    assert b.signal_schedule == (0, 7)
    for q in range(4):
        for v in range(V):
            assert np.array_equal(sig[q][v], np.concatenate([o[q][v] for o in loop])), (q, v)
    eh = b.evaluation_hops()
    for q in KEYS:
        assert eh[q].shape[0] == 7
        assert np.array_equal(eh[q], np.concatenate([r[q] for r in recs])), q
        assert np.array_equal(b.evaluation_totals()[q], a.evaluation_totals()[q]), q
    same_state(a.get_state(), b.get_state())
    pa, pb = a.predicted_pressure(), b.predicted_pressure()
    for q in pa:
        assert np.array_equal(pa[q], pb[q])
    assert c.predicted_pressure() is None                    # resumed, no hop yet
    for k in range(3, 7):
        same_outputs(hop(c, x, k, 16), loop[k])
        for q in KEYS:
            assert np.array_equal(c.evaluation_hops()[q], recs[k][q]), (k, q)
    for q in KEYS:
        assert np.array_equal(c.evaluation_totals()[q], a.evaluation_totals()[q]), q
    same_state(a.get_state(), c.get_state())
    # a per-hop call after a whole signal: the record is one slot again
    hop(b, x, 0, 16)
    assert b.evaluation_hops()["bright"].shape[0] == 1
    # reset: the next hop's totals are its own record, its pressures those of outputs that start from silence
    a.reset_evaluation()
    out = hop(a, x, 1, 16)
    rvA, rvB = validation_rirs(40, L, 5)
    fresh = StreamEvaluation(rvA, rvB, [1, V]).hop(out)
    check_hop(a, fresh, 16, 40, [0.0, 0.0])
    for q in KEYS:
        assert np.array_equal(a.evaluation_totals()[q], a.evaluation_hops()[q][0]), q
    for o in (a, b, c):
        o.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fir", [False, True])
def test_design_and_synthesis_untouched(fir, dtype):
    """outputs, w_*, lambda_* and the common state of a stream with the keywords equal those of the same stream without, 4 hops"""
    a, b = make(dtype, fir, Pv=9, Mv=5), make(dtype, fir, evaluate=False)
    x = signal(4, 16)
    for k in range(4):
        same_outputs(hop(a, x, k, 16), hop(b, x, k, 16))
        for name in ("w_A", "w_B", "lambda_A", "lambda_B"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), (k, name)
    sa, sb = a.get_state(), b.get_state()
    assert sorted(set(sa) - set(sb)) == ["evaluation_history", "evaluation_totals"]
    same_state({k: sa[k] for k in sb}, sb)
    with pytest.raises(KeyError):
        b.set_state({"evaluation_totals": sa["evaluation_totals"]})
    with pytest.raises(RuntimeError):
        b.evaluation_totals()
    a.close()
    b.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["window", "forgetting", "reassigned"])
def test_changes_between_hops(case):
    kw = {"window": dict(statistics_hops=3), "forgetting": dict(statistics_forgetting=0.9), "reassigned": {}}[case]
    ap = make(Pv=9, Mv=5, **kw)
    rvA, rvB = validation_rirs(9, L, 5)
    ev = StreamEvaluation(rvA, rvB, range(1, V + 1))
    x = signal(6, 16)
    worst = [0.0, 0.0]
    for k in range(6):
        if case == "reassigned" and k == 2:
            ap.mu = 30.0
        if case == "reassigned" and k == 4:
            ap.rir_A = synth_rirs(P, L, M, 5)[0]
        check_hop(ap, ev.hop(hop(ap, x, k, 16)), 16, 9, worst)
    print(f"{case}: largest pressure / energy error over bound {worst[0]:.3f} / {worst[1]:.3f}")
    ap.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fir", [False, True])
def test_known_answer_identity_responses(fir, dtype):
    """unit impulses at tap 0 into microphone m = loudspeaker l: the pressures ARE the outputs"""
    eye = np.eye(L)[None]
    ap = make(dtype, fir, Pv=1, Mv=L, rv=(eye, eye))
    x = signal(3, 16)
    for k in range(3):
        out = hop(ap, x, k, 16)
        p = ap.predicted_pressure()
        for z in range(2):
            assert np.array_equal(p["bright"][z], np.stack(out[z])) and np.array_equal(p["dark"][z], np.stack(out[z]))
            assert np.array_equal(p["target"][z], out[2 + z][0])
            ref = np.sum((out[2 + z][0][None] - np.stack(out[z])) ** 2, axis=1)
            assert np.all(np.abs(ap.evaluation_hops()["error"][0, z] - ref) <= energy_bound(16) * ref)
    ap.close()


def test_known_answer_full_rank_beats_rank_one():
    """validation = control responses, V = L, mu small, FIR stream, stationary (white) input: the total NMSE at rank L is below
    that at rank 1.  The oracle (constrained subband oracle + the FIR synthesis definition + the SciPy helper) shows the ordering
    on its own; the device is asserted to show it too.  Only the ordering is asserted.  Both reference loudspeakers are REF_A
    here: the target OUTPUTS A_t and B_t are the delayed inputs in column reference_index_A for both programs (apvast.py:389-390),
    so program B's target pressure is the one its filters were designed for only when reference_index_B is the same column."""
    from ap_vast_unofficial_amd.apvast import apvast
    from ap_vast_unofficial_amd.evaluation import metrics
    n, h, l, m, p, hops, mu = 32, 16, 4, 6, 24, 8, 1e-6
    rirA, rirB = synth_rirs(p, l, m, 1)
    ap = apvast(n, rirA, rirB, J, DELAY, REF_A, REF_A, l, mu, 4 * n, hop_size=h, perceptual=False, seed=0,
                constrain_filter_length=True, synthesis="fir", validation_rir_A=rirA, validation_rir_B=rirB, evaluation_ranks=[1, l])
    rs = np.random.RandomState(0)
    init_r = np.stack([1e-3 * rs.randn(n, l, m) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(n, m) for _ in range(2)])
    orc = ConstrainedSubbandOracle(n, rirA, rirB, DELAY, REF_A, REF_A, list(range(1, l + 1)), mu, stat_hops=1, hop_size=h,
                                   init_response=init_r, init_target_response=init_t, filter_taps=J)
    ref = FirStreamReference(J, h, l, l, DELAY, REF_A)
    ev = StreamEvaluation(rirA, rirB, [1, l])
    x = signal(hops, h)
    for k in range(hops):
        hop(ap, x, k, h)
        hop(orc, x, k, h)
        ev.hop(ref.hop(x[0, k * h:(k + 1) * h], x[1, k * h:(k + 1) * h], orc.w_time)[0])
    exp = metrics(ev.totals)["nmse"]
    got = metrics(ap.evaluation_totals())["nmse"]
    print("oracle nmse [z, (rank 1, rank L)]", exp.tolist(), "device", got.tolist())
    assert np.all(exp[:, 1] < exp[:, 0])                     # the oracle alone
    assert np.all(got[:, 1] < got[:, 0])
    ap.close()

"""Evaluation stage of the subband stream (validation_rir_A / validation_rir_B): what can be checked without a GPU -- the SciPy
helper against the whole-signal oracle, the metrics against evaluation.nmse / acoustic_contrast_db, the derived bounds on two
float64 summation orders, the keywords' validation (it runs before any engine exists), the unchanged state keys, and the C ABI's
declarations and exports."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from evaluation_oracle import PressureFilter, StreamEvaluation, energies, energy_bound, metrics, pressure_bound, window_pressure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, L, Pv, Mv)
SHAPES = [(16, 3, 1, 2), (16, 3, 5, 4), (30, 5, 37, 3), (16, 16, 40, 17), (64, 2, 200, 5), (20, 70, 9, 33)]


@pytest.mark.parametrize("H,L,Pv,Mv", SHAPES)
def test_helper_hop_by_hop_is_predict_pressure(H, L, Pv, Mv):
    """the helper run over 4 hops against oracle.static_vast.predict_pressure on the concatenated signal, within the pressure bound;
    and against the kernel's windowed definition"""
    from oracle.static_vast import predict_pressure
    rng = np.random.default_rng(H + L + Pv + Mv)
    hops = 4
    rv = rng.standard_normal((Pv, L, Mv))
    y = rng.standard_normal((hops * H, L))
    f = PressureFilter(rv)
    got = [f.hop(y[h * H:(h + 1) * H]) for h in range(hops)]
    p, S = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    ref = predict_pressure(y, rv)
    assert p.shape == ref.shape == (hops * H, Mv)
    share = (np.abs(p - ref) / S).max() / pressure_bound(L, Pv)
    print(f"helper vs predict_pressure: largest error / bound {share:.3f}")
    assert np.all(np.abs(p - ref) <= pressure_bound(L, Pv) * S)
    assert np.all(np.abs(p) <= S * (1 + 1e-12))
    ypad = np.concatenate([np.zeros((Pv - 1, L)), y])
    for h in range(hops):
        w, Sw = window_pressure(ypad[h * H:h * H + Pv - 1 + H], rv, H)
        assert np.all(np.abs(w - got[h][0]) <= pressure_bound(L, Pv) * Sw)
        assert np.all(np.abs(Sw - got[h][1]) <= pressure_bound(L, Pv) * Sw)


@pytest.mark.parametrize("H,L,Pv,Mv", SHAPES)
def test_two_summation_orders_stay_inside_the_bounds(H, L, Pv, Mv):
    """the same sums in two float64 orders (einsum over (l, j) against a loop over j of matrix products; np.sum against a running
    sum): within 0.10 of the pressure bound and 0.08 of the energy bound"""
    rng = np.random.default_rng(7 * H + Pv)
    rv = rng.standard_normal((Pv, L, Mv))
    y = rng.standard_normal((Pv - 1 + H, L))
    a, S = window_pressure(y, rv, H)
    b = np.zeros((H, Mv))
    for j in range(Pv):
        b += y[Pv - 1 - j:Pv - 1 - j + H] @ rv[j]
    assert (np.abs(a - b) / S).max() <= 0.10 * pressure_bound(L, Pv)
    e1 = np.sum(a ** 2, axis=0)
    e2 = np.zeros(Mv)
    for n in range(H):
        e2 = e2 + a[n] * a[n]
    assert (np.abs(e1 - e2) / e1).max() <= 0.08 * energy_bound(H)


def test_metrics_from_summed_energies():
    """evaluation.metrics on energies summed hop by hop == evaluation.nmse / acoustic_contrast_db on the concatenated pressures"""
    from ap_vast_unofficial_amd.evaluation import acoustic_contrast_db, metrics as dev_metrics, nmse
    rng = np.random.default_rng(3)
    Z, E, H, Mv, hops = 2, 3, 16, 5, 6
    pb = rng.standard_normal((hops, Z, E, H, Mv))
    pd = 0.1 * rng.standard_normal((hops, Z, E, H, Mv))
    pt = pb[:, :, 0] + 0.3 * rng.standard_normal((hops, Z, H, Mv))
    tot = {k: 0.0 for k in ("bright", "dark", "error", "target")}
    for h in range(hops):
        tot["bright"] = tot["bright"] + np.sum(pb[h] ** 2, axis=2)
        tot["dark"] = tot["dark"] + np.sum(pd[h] ** 2, axis=2)
        tot["error"] = tot["error"] + np.sum((pt[h][:, None] - pb[h]) ** 2, axis=2)
        tot["target"] = tot["target"] + np.sum(pt[h] ** 2, axis=1)
    m = dev_metrics(tot)
    assert m["nmse"].shape == m["contrast_db"].shape == (Z, E)
    for z in range(Z):
        for e in range(E):
            cb = np.concatenate([pb[h, z, e] for h in range(hops)])
            cd = np.concatenate([pd[h, z, e] for h in range(hops)])
            ct = np.concatenate([pt[h, z] for h in range(hops)])
            assert abs(m["nmse"][z, e] - nmse(ct, cb)) <= 1e-12 * abs(nmse(ct, cb))
            assert abs(m["contrast_db"][z, e] - acoustic_contrast_db(cb, cd)) <= 1e-12 * abs(acoustic_contrast_db(cb, cd))
            hn, hc = metrics(tot["bright"][z, e], tot["dark"][z, e], tot["error"][z, e], tot["target"][z])
            assert abs(hn - m["nmse"][z, e]) <= 1e-12 * abs(hn) and abs(hc - m["contrast_db"][z, e]) <= 1e-12 * abs(hc)


def test_stream_evaluation_helper_shapes_and_totals():
    rng = np.random.default_rng(4)
    L, V, H, Pv, Mv = 3, 3, 8, 5, 2
    rvA, rvB = rng.standard_normal((2, Pv, L, Mv))
    ev = StreamEvaluation(rvA, rvB, [1, 3], run_A=False)
    sums = None
    for _ in range(3):
        B = [rng.standard_normal((H, L)) for _ in range(V)]
        At, Bt = [rng.standard_normal((H, L))] * V, [rng.standard_normal((H, L))] * V
        r = ev.hop((None, B, At, Bt))
        assert r["bright"].shape == r["dark"].shape == (1, 2, H, Mv) and r["target"].shape == (1, H, Mv)
        eb, ed, ee, et = energies(r["bright"][0, 1], r["dark"][0, 1], r["target"][0])
        assert np.array_equal(eb, r["e_bright"][0, 1]) and np.array_equal(ed, r["e_dark"][0, 1])
        assert np.array_equal(ee, r["e_error"][0, 1]) and np.array_equal(et, r["e_target"][0])
        # program B: bright through zone B's responses, of rank 3 = B[2]
        w, _ = window_pressure(np.concatenate([np.zeros((Pv - 1, L)), B[2]]), rvB, H)
        if sums is None:
            assert np.abs(w - r["bright"][0, 1]).max() < 1e-12
        sums = r["e_error"] if sums is None else sums + r["e_error"]
    assert np.array_equal(sums, ev.totals["error"])


def test_keywords_signature_and_validation():
    from ap_vast_unofficial_amd.apvast import apvast
    sig = inspect.signature(apvast).parameters
    for k in ("validation_rir_A", "validation_rir_B", "evaluation_ranks"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY and sig[k].default is None
    r = np.zeros((10, 2, 2))
    rv = np.ones((5, 2, 3))
    mk = lambda **kw: apvast(256, r, r, 16, 4, 0, 0, 2, 1.0, 512, 128, perceptual=False, **kw)
    # all of it before the engine is created: none of these needs a GPU or the library
    with pytest.raises(ValueError, match="both or neither"):
        mk(validation_rir_A=rv)
    with pytest.raises(ValueError, match="both or neither"):
        mk(validation_rir_B=rv)
    with pytest.raises(ValueError, match="one shape"):
        mk(validation_rir_A=rv, validation_rir_B=np.ones((5, 2, 4)))
    with pytest.raises(ValueError, match="one shape"):
        mk(validation_rir_A=np.ones((5, 6)), validation_rir_B=np.ones((5, 6)))
    with pytest.raises(ValueError, match="L = 2 loudspeakers"):
        mk(validation_rir_A=np.ones((5, 3, 3)), validation_rir_B=np.ones((5, 3, 3)))
    with pytest.raises(ValueError, match="L = 2 loudspeakers"):
        mk(validation_rir_A=np.ones((0, 2, 3)), validation_rir_B=np.ones((0, 2, 3)))
    for bad in (np.nan, np.inf):
        nf = rv.copy()
        nf[2, 1, 0] = bad
        with pytest.raises(ValueError, match="must be finite"):
            mk(validation_rir_A=rv, validation_rir_B=nf)
        with pytest.raises(ValueError, match="must be finite"):
            mk(validation_rir_A=nf, validation_rir_B=rv)
    with pytest.raises(ValueError, match="evaluation_ranks needs validation_rir_A"):
        mk(evaluation_ranks=[1])
    with pytest.raises(ValueError, match="a subband keyword"):
        mk(validation_rir_A=rv, validation_rir_B=rv, mode="broadband")
    for bad in ([], [0], [3], [2, 1], [1, 1], [1.5], [True], 2, "12"):
        with pytest.raises(ValueError, match="strictly ascending"):
            mk(validation_rir_A=rv, validation_rir_B=rv, evaluation_ranks=bad)
    a, b, ranks = apvast._check_evaluation(rv, rv, None, 2, 2, "subband")
    assert ranks == [1, 2] and a.dtype == np.float64 and a is not rv
    assert apvast._check_evaluation(rv, rv, (2,), 2, 2, "subband")[2] == [2]
    assert apvast._check_evaluation(None, None, None, 2, 2, "broadband") is None


def test_state_keys_unchanged_without_the_keywords():
    from ap_vast_unofficial_amd.apvast import apvast
    assert apvast._EVAL_STATE == ("evaluation_history", "evaluation_totals")
    others = apvast._SB_STATE + apvast._BB_STATE + apvast._LIVE_STATE + apvast._WIN_STATE + apvast._FORGET_STATE + apvast._FIR_STATE
    assert not set(apvast._EVAL_STATE) & set(others)
    assert apvast._SB_STATE == ("response", "target_response", "input_block", "input_history", "out_overlap")
    # get_state and set_state take the evaluation keys only in subband mode and behind the object's own evaluation stage
    rows = [r for r in apvast._STATE_ROWS if r.key in apvast._EVAL_STATE]
    flags = lambda **kw: [bool(f(SimpleNamespace(**kw))) for r in rows for f in (r.accepts, r.reports or r.accepts)]
    assert len(rows) == len(apvast._EVAL_STATE)
    assert not any(flags(mode="subband", _evaluation=None))
    assert all(flags(mode="subband", _evaluation=(None, None, [1])))
    assert not any(flags(mode="broadband", _evaluation=(None, None, [1])))
    for name in ("evaluation_hops", "evaluation_totals", "predicted_pressure", "reset_evaluation"):
        assert callable(getattr(apvast, name))


def test_abi_declared_and_exported():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert re.search(r"int\s+apv_stream_set_evaluation\(apv_handle\* h, int32_t Pv, int32_t Mv, const double\* h_rvA, const double\* h_rvB, "
                     r"int32_t n_ranks,\s+const int32_t\* ranks\);", text)
    assert re.search(r"int\s+apv_stream_reset_evaluation\(apv_handle\* h\);", text)
    assert re.search(r"int\s+apv_eval_pressure\(apv_handle\* h, const void\* d_y, const double\* d_rv, int32_t G, int32_t L, int32_t Pv, "
                     r"int32_t H, int32_t Mv,\s+double\* d_p\);", text)
    assert int(re.search(r"#define APV_ABI_VERSION (\d+)", text).group(1)) == 2
    for name in ("apv_stream_set_evaluation", "apv_stream_reset_evaluation", "apv_eval_pressure"):
        assert name in _capi.EXPORTS
    assert inspect.signature(_capi.Engine.__init__).parameters["evaluation"].default is None
    for name in ("set_evaluation", "reset_evaluation", "eval_pressure"):
        assert hasattr(_capi.Engine, name)
    mk = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "Makefile")).read()
    assert "kernels_streameval.hip" in mk
    internal = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "apv_internal.h")).read()
    assert "apv_launch_eval_pressure" in internal and "apv_launch_eval_advance" in internal

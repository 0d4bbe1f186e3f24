"""Detectability stage of the broadband stream (apvast.enable_evaluation_detectability, apv_bb_set_evaluation_detectability, the
hop-batched launches of csrc/kernels_evaldetect.hip) against the NumPy restatement of tests/detectability_oracle.py, fed after
every hop with the device's own predicted_pressure(): that separates this stage from the pressure kernel.  Every value is held to
StreamReference.hop's derived per-element bound -- 2 (2 K + C + 16) u D plus the first-order propagation of the transform's error
-- and every test asserts that the bound is below 1e-10 D wherever D > 0 and that the device gives 0 exactly where the reference
is 0 (a silent disturbance), so the bound cannot hide a failure.  process_signal, which evaluates a whole group of hops in three
launches, is held to the hop loop bit for bit.

The object is a small one of its own: the N = 32 of tests/test_gpu_broadband_evaluation.py cannot be calibrated by the model."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import detectability_oracle as do  # noqa: E402
from eval_spectra_oracle import stack_sets  # noqa: E402
from test_gpu_broadband_evaluation import MATLAB_RANKS, same_outputs, same_state, validation_rirs  # noqa: E402
from test_gpu_evaluation_detectability import fold, tables_of  # noqa: E402
from test_gpu_stream import synth_rirs  # noqa: E402

J, L, M, V, P = 4, 3, 4, 3, 10
DELAY, REF_A, REF_B = 1, 1, 2
# dialect, block, hop, sampling rate, channels of the model
PY_A, PY_B, MATLAB = ("python", 96, 24, 48000, 44), ("python", 136, 40, 16000, 34), ("matlab", 96, 48, 48000, 44)
MV = 5


def make(size=PY_A, run_A=True, run_B=True, perceptual=False):
    from ap_vast_unofficial_amd.apvast import apvast
    dialect, n, h, fs, _ = size
    rirA, rirB = synth_rirs(P, L, M, 1)
    nev = MATLAB_RANKS if dialect == "matlab" else V
    return apvast(n, rirA, rirB, J, DELAY, REF_A, REF_B, nev, 1.0, 4 * n, hop_size=h, sampling_rate=fs, run_A=run_A, run_B=run_B,
                  perceptual=perceptual, mode="broadband", dialect=dialect, seed=0)


def switched_on(size=PY_A, Pv=9, ranks=None, detect=True, Mv=MV, **kw):
    ap = make(size, **kw)
    ap.enable_evaluation(*validation_rirs(Pv, Mv), ranks)
    ap.enable_evaluation_spectra()
    if detect:
        ap.enable_evaluation_detectability()
    return ap


def signal(size, hops, seed=99):
    return np.random.default_rng(seed).standard_normal((2, hops * size[2]))


def hop(ap, x, k):
    h = ap.hop_size
    return ap.process_input_buffers(x[0, k * h:(k + 1) * h], x[1, k * h:(k + 1) * h])


def dims(ap):
    Z, E, _, Mv = ap._eval_dims()
    return Z, E, Mv


def reference_of(ap):
    Z, E, Mv = dims(ap)
    return do.StreamReference(ap.detectability_model, ap.block_size, ap.hop_size, Z, E, Mv)


def within(got, ref, bound, worst):
    """|got - ref| <= bound with bound < 1e-10 ref where ref > 0; got == 0 exactly where ref == 0"""
    assert got.shape == ref.shape == bound.shape
    pos = ref > 0
    assert np.all(ref >= 0) and np.all(got[~pos] == 0.0)
    assert np.all(bound[pos] < 1e-10 * ref[pos])
    err = np.abs(got - ref)
    if pos.any():
        worst[0] = max(worst[0], float((err[pos] / bound[pos]).max()))
    assert np.all(err[pos] <= bound[pos]), worst


def hop_against_helper(ap, ref, tot, worst):
    """the last hop of the record against the helper fed the device's own pressures; returns the totals one hop later, folded in
    the device's arithmetic from the device's own values"""
    want, bound = ref.hop(stack_sets(ap.predicted_pressure()))
    got = ap.evaluation_detectability_hops()
    for key in ("error", "leak"):
        within(got[key][-1], want[key], bound[key], worst)
    return fold(tot, np.concatenate([got["error"][-1], got["leak"][-1]], axis=1), want["error"].shape[1])


def same_totals(t, tot, hops):
    Z, sixE, Mv = tot.shape
    dev = tot.reshape(Z, 2, 3, sixE // 6, Mv)
    assert t["hops"] == hops and t["error_audible"].dtype == np.int64
    for i, key in enumerate(("error", "leak")):
        assert np.array_equal(t[key], dev[:, i, 0]) and np.array_equal(t[key + "_max"], dev[:, i, 1]), key
        assert np.array_equal(t[key + "_audible"], dev[:, i, 2].astype(np.int64)), key


def same_dicts(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        assert sorted(a) == sorted(b)
        for q in a:
            assert np.array_equal(a[q], b[q]), q


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_A,run_B", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("size", [PY_A, PY_B, MATLAB], ids=lambda s: f"{s[0]}-{s[1]}")
def test_per_hop_stream_against_numpy(size, run_A, run_B):
    """Pv in {1, 9}, every emitted rank and a strict subset, the design weighting on and off, six hops each"""
    from ap_vast_unofficial_amd.evaluation import detectability_metrics
    worst = [0.0]
    x = signal(size, 6)
    subset = [6, 12] if size[0] == "matlab" else [1, V]
    for Pv in (1, 9):
        for ranks in (None, subset):
            perceptual = (Pv == 9) == (ranks is None)
            ap = switched_on(size, Pv, ranks, run_A=run_A, run_B=run_B, perceptual=perceptual)
            tb = ap.detectability_model
            assert tb.n_channels == size[4] and (not perceptual or ap.model is tb)
            assert ap.evaluation_detectability() is None and ap.evaluation_detectability_hops() is None
            Z, E, Mv = dims(ap)
            assert (Z, E, Mv) == (int(run_A) + int(run_B), len(ranks or range(V)), MV)
            ref, tot = reference_of(ap), np.zeros((Z, 6 * E, Mv))
            for k in range(6):
                hop(ap, x, k)
                got = ap.evaluation_detectability_hops()
                assert got["error"].shape == got["leak"].shape == (1, Z, E, Mv)
                tot = hop_against_helper(ap, ref, tot, worst)
                same_totals(ap.evaluation_detectability(), tot, k + 1)
            met = detectability_metrics(ap.evaluation_detectability())
            assert met["error_mean"].shape == (Z, E) and np.all(met["leak_audible_share"] <= 1.0)
            assert ap.get_state()["evaluation_detectability"].shape == (Z, 6 * E + 1, Mv)
            ap.close()
    print(f"{size[0]} N={size[1]} A={run_A} B={run_B}: largest error / bound {worst[0]:.4f}")


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [PY_B, MATLAB], ids=lambda s: f"{s[0]}-{s[1]}")
def test_whole_signal_equals_the_hop_loop(size):
    """19 hops are a group of 16 and a group of 3; a second call of 5 hops one group of 5.  Record and totals of process_signal
    equal the hop loop's bit for bit; the hop loop is held to the helper."""
    worst = [0.0]
    ranks = [6, 12] if size[0] == "matlab" else [1, V]
    a, b = switched_on(size, ranks=ranks), switched_on(size, ranks=ranks)
    Z, E, Mv = dims(a)
    ref, tot = reference_of(a), np.zeros((Z, 6 * E, Mv))
    h = size[2]
    x = signal(size, 24)
    done = 0
    for hops in (19, 5):
        b.process_signal(x[0, done * h:(done + hops) * h], x[1, done * h:(done + hops) * h])
        rec = {"error": [], "leak": []}
        for k in range(done, done + hops):
            hop(a, x, k)
            tot = hop_against_helper(a, ref, tot, worst)
            r = a.evaluation_detectability_hops()
            for key in rec:
                rec[key].append(r[key][0])
        done += hops
        rb = b.evaluation_detectability_hops()
        for key in rec:
            assert rb[key].shape == (hops, Z, E, Mv)
            assert np.array_equal(rb[key], np.stack(rec[key])), key
        same_totals(a.evaluation_detectability(), tot, done)
        same_dicts(b.evaluation_detectability(), a.evaluation_detectability())
        assert np.array_equal(b.get_state()["evaluation_detectability"], a.get_state()["evaluation_detectability"])
    print(f"{size[0]} N={size[1]}, 24 hops: largest error / bound {worst[0]:.4f}")
    a.close()
    b.close()


# 3 ---------------------------------------------------------------------------------------------------------------
def test_switched_on_mid_stream():
    """after 3 hops: totals and record start at the switch, the spectra's ring goes on -- the helper is fed the three hops before
    too, its values dropped -- and spectra, ring and energies are those of an object that never gets the switch"""
    worst = [0.0]
    a, b = switched_on(detect=False), switched_on(detect=False)
    x = signal(PY_A, 8)
    Z, E, Mv = dims(a)
    ref = do.StreamReference(tables_of(PY_A[1], PY_A[3]), a.block_size, a.hop_size, Z, E, Mv)
    for k in range(3):
        same_outputs(hop(a, x, k), hop(b, x, k))
        ref.hop(stack_sets(a.predicted_pressure()))
    for f in (a.evaluation_detectability, a.evaluation_detectability_hops):
        with pytest.raises(RuntimeError, match=r"enable_evaluation_detectability\(\)"):
            f()
    assert "evaluation_detectability" not in a.get_state()
    a.enable_evaluation_detectability()
    assert np.array_equal(a.detectability_model.G2, ref.tables.G2) and a.detectability_model.Ca == ref.tables.Ca
    assert a.evaluation_detectability() is None and a.evaluation_detectability_hops() is None
    assert a.predicted_pressure() is not None and a.evaluation_spectra() is not None    # the stages before go on as they were
    assert not a.get_state()["evaluation_detectability"].any()
    tot = np.zeros((Z, 6 * E, Mv))
    for k in range(3, 8):
        same_outputs(hop(a, x, k), hop(b, x, k))
        assert a.evaluation_detectability_hops()["error"].shape[0] == 1
        tot = hop_against_helper(a, ref, tot, worst)
        same_totals(a.evaluation_detectability(), tot, k - 2)
        same_dicts(a.evaluation_spectra(), b.evaluation_spectra())
        same_dicts(a.evaluation_totals(), b.evaluation_totals())
    sa, sb = a.get_state(), b.get_state()
    assert np.array_equal(sa["evaluation_ring"], sb["evaluation_ring"]) and np.array_equal(sa["evaluation_spectra"], sb["evaluation_spectra"])
    print(f"switched on after 3 hops: largest error / bound {worst[0]:.4f}")
    a.close()
    b.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [PY_A, MATLAB], ids=lambda s: f"{s[0]}-{s[1]}")
def test_nothing_else_moves(size):
    """outputs, filters, eigenvalues, every other state key, energies, pressures and spectra of a stream with the switch are bit
    for bit those of the same stream without it, hop by hop and over a whole signal of a group of 16 and one of 4"""
    a, b = switched_on(size), switched_on(size, detect=False)
    h = size[2]
    x = signal(size, 4 + 20)

    def compare():
        for name in ("evaluation_hops", "evaluation_totals", "predicted_pressure", "evaluation_spectra"):
            same_dicts(getattr(a, name)(), getattr(b, name)())
        for name in ("w_A", "w_B", "lambda_A", "lambda_B"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        sa, sb = a.get_state(), b.get_state()
        assert sorted(set(sa) - set(sb)) == ["evaluation_detectability"] and not set(sb) - set(sa)
        same_state({k: sa[k] for k in sb}, sb)

    for k in range(4):
        same_outputs(hop(a, x, k), hop(b, x, k))
        compare()
    same_outputs(a.process_signal(x[0, 4 * h:], x[1, 4 * h:]), b.process_signal(x[0, 4 * h:], x[1, 4 * h:]))
    compare()
    assert a.evaluation_detectability_hops()["leak"].shape[0] == 20 and a.evaluation_detectability()["hops"] == 24
    a.close()
    b.close()


# 5 ---------------------------------------------------------------------------------------------------------------
def test_resume_and_reset():
    size = PY_B
    a, b, c = switched_on(size, ranks=[1, V]), switched_on(size, ranks=[1, V]), switched_on(size, ranks=[1, V], detect=False)
    Z, E, Mv = dims(a)
    x = signal(size, 9)
    for k in range(4):
        hop(a, x, k)
    st = a.get_state()
    assert st["evaluation_detectability"].shape == (Z, 6 * E + 1, Mv) and np.all(st["evaluation_detectability"][:, -1] == 4)
    assert sorted(set(st) - set(c.get_state())) == ["evaluation_detectability"]
    b.set_state(st)
    same_state(b.get_state(), st)
    assert b.evaluation_detectability() is None              # no hop of its own yet
    for k in range(4, 8):
        same_outputs(hop(b, x, k), hop(a, x, k))
        same_dicts(b.evaluation_detectability_hops(), a.evaluation_detectability_hops())
        same_dicts(b.evaluation_detectability(), a.evaluation_detectability())
    assert a.evaluation_detectability()["hops"] == 8
    same_state(a.get_state(), b.get_state())
    # reset: the next hop's totals are its own values
    a.reset_evaluation()
    assert not a.get_state()["evaluation_detectability"].any()
    t = a.evaluation_detectability()
    assert t["hops"] == 0 and not any(np.any(v) for v in t.values())
    hop(a, x, 8)
    t, r = a.evaluation_detectability(), a.evaluation_detectability_hops()
    assert t["hops"] == 1
    for key in ("error", "leak"):
        assert np.array_equal(t[key], r[key][0]) and np.array_equal(t[key + "_max"], r[key][0])
        assert np.array_equal(t[key + "_audible"], (r[key][0] > 1.0).astype(np.int64))
    # an object without the switch does not know the key
    with pytest.raises(KeyError):
        c.set_state({"evaluation_detectability": st["evaluation_detectability"]})
    with pytest.raises(KeyError):
        c.set_state(st)
    for bad in (np.zeros((Z, 6 * E, Mv)), np.zeros((Z, 6 * E + 1, Mv + 1))):
        with pytest.raises(ValueError, match="evaluation_detectability"):
            b.set_state({"evaluation_detectability": bad})
    neg = st["evaluation_detectability"].copy()
    neg[:, -1] = -1.0
    with pytest.raises(ValueError, match="hop count"):
        b.set_state({"evaluation_detectability": neg})
    for ap in (a, b, c):
        ap.close()


# 6 ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from ap_vast_unofficial_amd import _capi
    from ap_vast_unofficial_amd.apvast import apvast
    from test_gpu_evaluation_detectability import make as make_subband
    sub = make_subband(96, 24, 48000, detect=None)
    with pytest.raises(RuntimeError, match="evaluation_detectability=True to the constructor"):
        sub.enable_evaluation_detectability()
    sub.close()
    ap = make()
    with pytest.raises(RuntimeError, match=r"after enable_evaluation_spectra\(\)"):
        ap.enable_evaluation_detectability()
    with pytest.raises(RuntimeError, match=r"no evaluation stage"):
        ap.evaluation_detectability()
    ap.enable_evaluation(*validation_rirs(9, MV))
    with pytest.raises(RuntimeError, match=r"after enable_evaluation_spectra\(\)"):
        ap.enable_evaluation_detectability()
    ap.enable_evaluation_spectra()
    for f in (ap.evaluation_detectability, ap.evaluation_detectability_hops):
        with pytest.raises(RuntimeError, match=r"enable_evaluation_detectability\(\)"):
            f()
    # the library's own refusals: nothing changes, the switch still works afterwards
    tb = tables_of(PY_A[1], PY_A[3])
    eng, G2 = ap._eng, np.ascontiguousarray(tb.G2)
    K, C = G2.shape
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nan, inf = np.array(G2), np.array(G2)
    nan[3, 1], inf[K - 1, C - 1] = np.nan, np.inf
    setter = eng.lib.apv_bb_set_evaluation_detectability
    for args in ((C, None, tb.Cs, tb.Ca, tb.Leff), (C, ptr(nan), tb.Cs, tb.Ca, tb.Leff), (C, ptr(inf), tb.Cs, tb.Ca, tb.Leff),
                 (C, ptr(G2), tb.Cs, 0.0, tb.Leff), (C, ptr(G2), tb.Cs, -1.0, tb.Leff), (C, ptr(G2), np.nan, tb.Ca, tb.Leff),
                 (C, ptr(G2), tb.Cs, tb.Ca, np.inf), (0, ptr(G2), tb.Cs, tb.Ca, tb.Leff), (-1, ptr(G2), tb.Cs, tb.Ca, tb.Leff),
                 (513, ptr(G2), tb.Cs, tb.Ca, tb.Leff)):
        assert setter(eng.h, *args) == _capi.ERR_ARG, args
    with pytest.raises(_capi.ApvError):
        eng.bb_get_state("eval_detect", (2, 6 * V, MV))
    ap.enable_evaluation_detectability()
    with pytest.raises(RuntimeError, match="already"):
        ap.enable_evaluation_detectability()
    assert setter(eng.h, C, ptr(G2), tb.Cs, tb.Ca, tb.Leff) == _capi.ERR_ARG             # a second call
    x = signal(PY_A, 1)
    hop(ap, x, 0)
    assert ap.evaluation_detectability()["hops"] == 1
    ap.close()
    # a block the model cannot calibrate: what the tables raise, the object as it was and still usable
    rirA, rirB = synth_rirs(P, L, M, 1)
    small = apvast(64, rirA, rirB, J, DELAY, REF_A, REF_B, V, 1.0, 256, hop_size=32, sampling_rate=48000, perceptual=False,
                   mode="broadband", seed=0)
    small.enable_evaluation(*validation_rirs(9, MV))
    small.enable_evaluation_spectra()
    with pytest.raises(RuntimeError, match="bisection"):
        small.enable_evaluation_detectability()
    assert small.detectability_model is None and "evaluation_detectability" not in small.get_state()
    y = np.random.default_rng(1).standard_normal((2, 32))
    small.process_input_buffers(y[0], y[1])
    assert small.evaluation_spectra() is not None
    with pytest.raises(RuntimeError, match=r"enable_evaluation_detectability\(\)"):
        small.evaluation_detectability()
    with pytest.raises(RuntimeError, match="bisection"):
        small.enable_evaluation_detectability()              # still switchable to nothing
    small.close()
    # the constructor keyword keeps its message in broadband mode
    with pytest.raises(ValueError, match="evaluation_detectability is a subband keyword"):
        apvast(96, rirA, rirB, J, DELAY, REF_A, REF_B, V, 1.0, 384, hop_size=24, sampling_rate=48000, mode="broadband",
               evaluation_detectability=True)

"""Per-bin evaluation spectra of the broadband stream (apvast.enable_evaluation_spectra, apv_bb_set_evaluation_spectra,
csrc/kernels_bbevalspec.hip) against the NumPy restatement of tests/eval_spectra_oracle.py, fed after every hop with the device's
own predicted_pressure(): that separates this stage from the pressure kernel.  Every accumulated element is held to that file's
derived bound,

    |got - ref| <= 4 c(N) u N sum_t ||w f_t[:, m]||_2^2,   c(N) = 8 (log2 N + 2) at N = 32.

process_signal, which transforms a whole group of hops per launch, is held to the hop loop bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from eval_spectra_oracle import KEYS, SpectraReference, bound_factor, check, stack_sets  # noqa: E402
from oracle.subband import sine_window  # noqa: E402
from test_gpu_broadband_evaluation import H, MATLAB_RANKS, N, V, hop, make, same_outputs, same_state, signal, validation_rirs  # noqa: E402

K = N // 2 + 1
MV = 5


def switched_on(Pv=9, ranks=None, spectra=True, **kw):
    ap = make(**kw)
    ap.enable_evaluation(*validation_rirs(Pv, MV), ranks)
    if spectra:
        ap.enable_evaluation_spectra()
    return ap


def dims(ap):
    Z, E, _, Mv = ap._eval_dims()
    return Z, E, Mv


def same_spectra(a, b):
    assert (a is None) == (b is None)
    if a is not None:
        for q in KEYS:
            assert np.array_equal(a[q], b[q]), q


def logical_ring(ap):
    """get_state()'s (Z, 2 E + 1, Mv, N) -> the helper's (Z, 2 E + 1, N, Mv)"""
    return ap.get_state()["evaluation_ring"].transpose(0, 1, 3, 2)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run_A,run_B", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("dialect", ["python", "matlab"])
def test_per_hop_stream_against_numpy(dialect, run_A, run_B):
    """Pv in {1, 9}, every emitted rank and a strict subset, six hops each"""
    worst = [0.0]
    x = signal(6)
    subset = [6, 12] if dialect == "matlab" else [1, V]
    for Pv in (1, 9):
        for ranks in (None, subset):
            ap = switched_on(Pv, ranks, dialect=dialect, run_A=run_A, run_B=run_B)
            assert ap.evaluation_spectra() is None
            Z, E, Mv = dims(ap)
            assert (Z, E, Mv) == (int(run_A) + int(run_B), len(ranks or (MATLAB_RANKS if dialect == "matlab" else range(V))), MV)
            ref = SpectraReference(N, H, Z, E, Mv)
            for k in range(6):
                hop(ap, x, k)
                ref.hop(stack_sets(ap.predicted_pressure()))
                got = ap.evaluation_spectra()
                assert got["bright"].shape == (Z, E, Mv, K) and got["target"].shape == (Z, Mv, K)
                check(got, ref, worst)
                assert np.array_equal(logical_ring(ap), ref.ring), k
            st = ap.get_state()
            assert st["evaluation_spectra"].shape == (Z, 3 * E + 1, K, Mv) and st["evaluation_ring"].shape == (Z, 2 * E + 1, Mv, N)
            ap.close()
    print(f"{dialect} A={run_A} B={run_B}: largest error / bound {worst[0]:.4f}")


# 2 ---------------------------------------------------------------------------------------------------------------
def test_whole_signal_equals_the_hop_loop():
    """19 hops are a group of 16 and a group of 3; a second call of 5 hops one group of 5.  Spectra and ring of process_signal
    equal the hop loop's bit for bit; the hop loop is held to the helper."""
    worst = [0.0]
    a, b = switched_on(ranks=[1, V]), switched_on(ranks=[1, V])
    Z, E, Mv = dims(a)
    ref = SpectraReference(N, H, Z, E, Mv)
    x = signal(24)
    done = 0
    for hops in (19, 5):
        b.process_signal(x[0, done * H:(done + hops) * H], x[1, done * H:(done + hops) * H])
        for k in range(done, done + hops):
            hop(a, x, k)
            ref.hop(stack_sets(a.predicted_pressure()))
        done += hops
        check(a.evaluation_spectra(), ref, worst)
        same_spectra(b.evaluation_spectra(), a.evaluation_spectra())
        assert np.array_equal(b.get_state()["evaluation_ring"], a.get_state()["evaluation_ring"])
        assert np.array_equal(logical_ring(a), ref.ring)
    print(f"24 hops: largest error / bound {worst[0]:.4f}")
    a.close()
    b.close()


# 3 ---------------------------------------------------------------------------------------------------------------
def test_parseval_against_the_devices_own_pressures():
    """No FFT in the reference: with c_k the one-sided weights of evaluation.spectral_metrics (1 for bins 0 and N/2, 2 otherwise)
    sum_k c_k |P_t[k]|^2 = N ||w f_t||^2, so sum_k c_k S[k] / N = sum_t ||w f_t||^2 = sum_n g[n] p[n]^2, g[n] the sum of w^2 over
    the frames that hold sample n.  Tolerance: every S[k] lies within 2 c(N) u N sum_t ||w f_t||^2 of its exact value (half the
    helper's bound, which spans two computed values) and sum_k c_k = N, so the left side errs by 2 c(N) u N R, R the right side;
    the other half of bound_factor(N) R is left to the (hops N + K) u R of the two NumPy sums."""
    hops = 7
    ap = switched_on(ranks=[1, V])
    x = signal(hops)
    ps = []
    for k in range(hops):
        hop(ap, x, k)
        ps.append(stack_sets(ap.predicted_pressure()))
    p = np.concatenate(ps, axis=2)                           # (Z, 2 E + 1, hops H, Mv)
    w2 = sine_window(N) ** 2
    g = np.zeros(hops * H)
    for t in range(hops):
        lo = (t + 1) * H - N
        g[max(lo, 0):(t + 1) * H] += w2[max(-lo, 0):]
    E = dims(ap)[1]
    sets = {"bright": p[:, :E], "dark": p[:, E:2 * E], "target": p[:, 2 * E], "error": p[:, 2 * E][:, None] - p[:, :E]}
    c = np.full(K, 2.0)
    c[0] = c[K - 1] = 1.0
    got, worst = ap.evaluation_spectra(), 0.0
    for q in KEYS:
        R = np.sum(g[:, None] * sets[q] ** 2, axis=-2)
        lhs = np.sum(c * got[q], axis=-1) / N
        assert lhs.shape == R.shape and np.all(R > 0)
        worst = max(worst, (np.abs(lhs - R) / (bound_factor(N) * R)).max())
        assert np.all(np.abs(lhs - R) <= bound_factor(N) * R), (q, worst)
    print(f"Parseval: largest error / bound {worst:.4f}")
    ap.close()


# 4 ---------------------------------------------------------------------------------------------------------------
def test_switched_on_mid_stream():
    """after 3 hops: the spectra are those of a helper that starts from an empty ring at that hop, and the three hops before are
    those of an object that never gets the switch"""
    worst = [0.0]
    a, b = switched_on(spectra=False), switched_on(spectra=False)
    x = signal(8)
    for k in range(3):
        same_outputs(hop(a, x, k), hop(b, x, k))
    same_state(a.get_state(), b.get_state())
    with pytest.raises(RuntimeError, match=r"enable_evaluation_spectra\(\)"):
        a.evaluation_spectra()
    a.enable_evaluation_spectra()
    assert a.evaluation_spectra() is None
    assert a.predicted_pressure() is not None               # the stage itself goes on as it was
    with pytest.raises(RuntimeError, match="already"):
        a.enable_evaluation_spectra()
    st = a.get_state()
    assert np.all(st["evaluation_spectra"] == 0.0) and np.all(st["evaluation_ring"] == 0.0)
    Z, E, Mv = dims(a)
    ref = SpectraReference(N, H, Z, E, Mv)
    for k in range(3, 8):
        same_outputs(hop(a, x, k), hop(b, x, k))
        ref.hop(stack_sets(a.predicted_pressure()))
        check(a.evaluation_spectra(), ref, worst)
        for q in KEYS:
            assert np.array_equal(a.evaluation_totals()[q], b.evaluation_totals()[q]), (k, q)
    assert np.array_equal(logical_ring(a), ref.ring)
    a.close()
    b.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dialect", ["python", "matlab"])
def test_everything_else_untouched(dialect):
    """outputs, evaluation_hops(), evaluation_totals(), predicted_pressure() and every shared state key of a stream with the
    evaluation stage alone are bit for bit those of the same stream with the spectra too, hop by hop and over a whole signal"""
    a, b = switched_on(dialect=dialect), switched_on(spectra=False, dialect=dialect)
    x = signal(4 + 20)

    def compare():
        for name in ("evaluation_hops", "evaluation_totals", "predicted_pressure"):
            u, v = getattr(a, name)(), getattr(b, name)()
            assert sorted(u) == sorted(v)
            for q in u:
                assert np.array_equal(u[q], v[q]), (name, q)
        for name in ("w_A", "w_B", "lambda_A", "lambda_B"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        sa, sb = a.get_state(), b.get_state()
        assert sorted(set(sa) - set(sb)) == ["evaluation_ring", "evaluation_spectra"] and not set(sb) - set(sa)
        same_state({k: sa[k] for k in sb}, sb)
        return sa

    for k in range(4):
        same_outputs(hop(a, x, k), hop(b, x, k))
        sa = compare()
    with pytest.raises(KeyError):
        b.set_state({"evaluation_spectra": sa["evaluation_spectra"]})
    same_outputs(a.process_signal(x[0, 4 * H:], x[1, 4 * H:]), b.process_signal(x[0, 4 * H:], x[1, 4 * H:]))
    compare()
    assert a.evaluation_hops()["bright"].shape[0] == 20
    a.close()
    b.close()


# 6 ---------------------------------------------------------------------------------------------------------------
def test_reset_evaluation():
    worst = [0.0]
    ap = switched_on(Pv=9)
    x = signal(6)
    for k in range(3):
        hop(ap, x, k)
    assert np.any(ap.get_state()["evaluation_spectra"] > 0.0)
    ap.reset_evaluation()
    st = ap.get_state()
    assert np.all(st["evaluation_spectra"] == 0.0) and np.all(st["evaluation_ring"] == 0.0)
    assert all(np.all(v == 0.0) for v in ap.evaluation_spectra().values())
    Z, E, Mv = dims(ap)
    ref = SpectraReference(N, H, Z, E, Mv)
    for k in range(3, 6):
        hop(ap, x, k)
        ref.hop(stack_sets(ap.predicted_pressure()))
        check(ap.evaluation_spectra(), ref, worst)
    assert np.array_equal(logical_ring(ap), ref.ring)
    ap.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_resume_is_bit_for_bit():
    a, b, c = switched_on(Pv=40, ranks=[1, V]), switched_on(Pv=40, ranks=[1, V]), switched_on(Pv=40, ranks=[1, V], spectra=False)
    x = signal(8)
    for k in range(4):
        hop(a, x, k)
    st = a.get_state()
    assert st["evaluation_spectra"].shape == (2, 7, K, MV) and st["evaluation_ring"].shape == (2, 5, MV, N)
    b.set_state(st)
    same_state(b.get_state(), st)
    for k in range(4, 8):
        same_outputs(hop(b, x, k), hop(a, x, k))
        same_spectra(b.evaluation_spectra(), a.evaluation_spectra())
    same_state(a.get_state(), b.get_state())
    # an object without the switch does not know the two keys
    with pytest.raises(KeyError):
        c.set_state(st)
    with pytest.raises(KeyError):
        c.set_state({"evaluation_ring": st["evaluation_ring"]})
    with pytest.raises(ValueError):
        b.set_state({"evaluation_spectra": np.zeros((2, 7, K, MV + 1))})
    for ap in (a, b, c):
        ap.close()


# 8 ---------------------------------------------------------------------------------------------------------------
def test_metrics_per_band():
    from ap_vast_unofficial_amd.evaluation import spectral_metrics, third_octave_bands
    ap = switched_on()
    x = signal(8)
    ap.process_signal(x[0], x[1])
    centres, bands = third_octave_bands(8000, N)
    m = spectral_metrics(ap.evaluation_spectra(), bands)
    Z, E, _ = dims(ap)
    for name in ("contrast_db", "nmse"):
        assert m[name].shape == (Z, E, len(bands)) and np.all(np.isfinite(m[name])), name
    per_bin = spectral_metrics(ap.evaluation_spectra())
    assert per_bin["nmse"].shape == (Z, E, K)
    assert len(centres) == len(bands) > 3
    ap.close()

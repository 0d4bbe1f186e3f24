"""get_state / set_state of class apvast: the keys a configuration has, the shape and dtype of every value, a checkpoint carried
into a second object, and what set_state refuses.  Key sets, shapes and dtypes are literal.

Configurations (those of test_gpu_state_names.py), each with dtype "f32" and "f64":
  (i)  everything that combines, at N = 96: the perceptual model's own tables need a block of 96 samples or more (N // 48 names the
       calibration bin), so this is the nearest block to 32 the class accepts with perceptual=True.  H = 8, so three hops leave the
       rings at offset 24; rir_A is reassigned before the third hop, which brings the two correction keys in;
  (ii) forgetting statistics alone, at N = 32;
and a broadband object at the smallest shape of test_gpu_broadband.py (N = 128, H = 64, J = 40, S = 300, two loudspeakers and
microphones, 200-tap responses)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import signal, validation_rirs  # noqa: E402

H, L, M, P, V = 8, 4, 2, 5, 2
T, J, PV, MV, E, Z = 3, 8, 4, 2, 2, 2
HOPS = 3
F8, C16 = np.float64, np.complex128


def base_shapes(N, n_out):
    return {"response": ((4, N, L, M), F8), "target_response": ((2, N, M), F8), "input_block": ((2, N), F8),
            "input_history": ((2, P - 1 + H), F8), "out_overlap": ((n_out, N), F8)}


def make_all(dtype, seed, plain=False):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 1)
    if plain:
        return apvast(96, rirA, rirB, J, 2, 0, 1, V, 1.0, 384, hop_size=H, perceptual=False, seed=seed, dtype=dtype)
    rvA, rvB = validation_rirs(PV, L, MV)
    return apvast(96, rirA, rirB, J, 2, 0, 1, V, 1.0, 384, hop_size=H, perceptual=True, seed=seed, dtype=dtype, statistics_hops=T,
                  constrain_filter_length=True, synthesis="fir", validation_rir_A=rvA, validation_rir_B=rvB,
                  evaluation_ranks=[1, 2], evaluation_spectra=True, evaluation_detectability=True)


def shapes_all(dtype):
    N, K = 96, 49
    d = base_shapes(N, 2 * V * L + 2 * L)
    d.update({"statistics_window": ((2, T, K, 2 * L * L + L), C16), "statistics_window_fill": ((), int),
              "fir_synthesis_taps": ((2, V, J, L), F8), "fir_synthesis_history": ((2, J - 1), F8),
              "evaluation_history": ((Z, E + 1, PV - 1, L), F8), "evaluation_totals": ((Z, 3 * E + 1, MV), F8),
              "evaluation_spectra": ((Z, 3 * E + 1, K, MV), F8), "evaluation_ring": ((Z, 2 * E + 1, MV, N), F8),
              "evaluation_detectability": ((Z, 6 * E + 1, MV), F8),
              "fir_correction": ((4, P - 1, L, M), F8), "target_fir_correction": ((2, P - 1, M), F8)})
    return d


def make_forgetting(dtype, seed, plain=False):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 1)
    return apvast(32, rirA, rirB, J, 2, 0, 1, V, 1.0, 128, hop_size=H, perceptual=False, seed=seed, dtype=dtype,
                  statistics_forgetting=None if plain else 0.9)


def shapes_forgetting(dtype):
    d = base_shapes(32, 2 * V * L + 2 * L)
    # the sums stay in the precision the device keeps them in
    d["statistics_forgetting_sums"] = ((2, 17, 2 * L * L + L), np.complex64 if dtype == "f32" else C16)
    return d


BB = dict(N=128, H=64, J=40, S=300, L=2, M=2, P=200)


def make_broadband(seed):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(BB["P"], BB["L"], BB["M"], 1)
    return apvast(BB["N"], rirA, rirB, BB["J"], 3, 0, 1, V, 1.0, BB["S"], hop_size=BB["H"], perceptual=False, mode="broadband",
                  seed=seed)


def shapes_broadband():
    N, S, l, m = BB["N"], BB["S"], BB["L"], BB["M"]
    return {"response": ((4, N, l, m), F8), "target_response": ((2, N, m), F8), "stats": ((4, S, l, m), F8),
            "target_stats": ((2, S, m), F8), "overlap": ((4, N, l, m), F8), "target_overlap": ((2, N, m), F8),
            "input_block": ((2, N), F8), "input_history": ((2, BB["P"] - 1 + BB["H"]), F8),
            "out_overlap": ((2 * V * l + 2 * l, N), F8)}


def check_state(st, want):
    assert set(st) == set(want), sorted(set(st) ^ set(want))
    for k, (shape, dt) in want.items():
        if dt is int:
            assert type(st[k]) is int, (k, type(st[k]))
        else:
            assert isinstance(st[k], np.ndarray) and st[k].shape == shape and st[k].dtype == dt, (k, st[k].shape, st[k].dtype)


def same_state(sa, sb):
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k


def refusals(obj, want, checked, plain, off_keys):
    """a wrong shape for every shape-checked key, an unknown key, and on the plain object the keys of the features it lacks"""
    for k in checked:
        shape = want[k][0]
        with pytest.raises(ValueError, match="must have shape"):
            obj.set_state({k: np.zeros(shape[:-1] + (shape[-1] + 1,))})
    with pytest.raises(KeyError, match="no such state array"):
        obj.set_state({"responses": np.zeros(3)})
    for k in off_keys:
        with pytest.raises(KeyError, match="no such state array"):
            plain.set_state({k: np.zeros(3)})


def resume(a, b, x, h_size, want, rir_A=None):
    """HOPS hops on a (rir_A assigned before the last), the checkpoint into b, whose rings stand elsewhere; then the same bits in
    every array, and in the outputs of one more hop"""
    for h in range(HOPS):
        if rir_A is not None and h == HOPS - 1:
            a.rir_A = rir_A
        hop(a, x, h, h_size)
    hop(b, x[::-1], 0, h_size)                         # b has a history of its own before the restore
    if rir_A is not None:
        b.rir_A = rir_A                                # the responses are not state: b is given a's
    sa = a.get_state()
    check_state(sa, want)
    b.set_state(sa)
    same_state(b.get_state(), sa)
    same_outputs(hop(a, x, HOPS, h_size), hop(b, x, HOPS, h_size))
    same_state(a.get_state(), b.get_state())


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_every_stage(dtype):
    a, b, plain = make_all(dtype, 5), make_all(dtype, 6), make_all(dtype, 7, plain=True)
    want = shapes_all(dtype)
    resume(a, b, signal(HOPS + 1, H), H, want, rir_A=synth_rirs(P, L, M, 7)[0])
    checked = ["statistics_window", "fir_synthesis_taps", "fir_synthesis_history", "evaluation_history", "evaluation_totals",
               "evaluation_spectra", "evaluation_ring", "evaluation_detectability"]
    off = sorted(set(want) - set(base_shapes(96, 0)) - {"fir_correction", "target_fir_correction"}) + ["statistics_forgetting_sums"]
    refusals(a, want, checked, plain, off)
    bad = a.get_state()["evaluation_detectability"]
    bad[0, 6 * E, 0] += 0.5
    with pytest.raises(ValueError, match="the last row must hold one hop count"):
        a.set_state({"evaluation_detectability": bad})
    # the correction keys are taken by every object, and reported once an update has reached the device
    assert "fir_correction" not in plain.get_state()
    plain.set_state({k: np.zeros(want[k][0]) for k in ("fir_correction", "target_fir_correction")})
    assert "fir_correction" in plain.get_state() and "target_fir_correction" in plain.get_state()
    for o in (a, b, plain):
        o.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_forgetting_only(dtype):
    a, b, plain = make_forgetting(dtype, 5), make_forgetting(dtype, 6), make_forgetting(dtype, 7, plain=True)
    want = shapes_forgetting(dtype)
    resume(a, b, signal(HOPS + 1, H), H, want)
    refusals(a, want, ["statistics_forgetting_sums"], plain, ["statistics_forgetting_sums", "statistics_window", "stats"])
    for k in ("statistics_window", "statistics_window_fill", "fir_synthesis_taps", "evaluation_totals", "evaluation_ring",
              "evaluation_detectability", "overlap"):
        with pytest.raises(KeyError, match="no such state array"):
            a.set_state({k: np.zeros(3)})
    check_state(plain.get_state(), base_shapes(32, 2 * V * L + 2 * L))
    for o in (a, b, plain):
        o.close()


def test_broadband():
    a, b = make_broadband(5), make_broadband(6)
    want = shapes_broadband()
    resume(a, b, signal(HOPS + 1, BB["H"]), BB["H"], want)
    # no key of this mode has a shape check of its own: the device's size check refuses
    from ap_vast_unofficial_amd._capi import ApvError
    with pytest.raises(ApvError, match="state size mismatch"):
        a.set_state({"stats": np.zeros((4, BB["S"] + 1, BB["L"], BB["M"]))})
    with pytest.raises(KeyError, match="no such state array"):
        a.set_state({"responses": np.zeros(3)})
    for k in ("statistics_window", "statistics_forgetting_sums", "fir_synthesis_taps", "evaluation_totals", "evaluation_spectra",
              "evaluation_detectability"):
        with pytest.raises(KeyError, match="no such state array"):
            a.set_state({k: np.zeros(3)})
    a.close()
    b.close()

"""The named state arrays of the subband stream at the C level (apv_state_bytes / apv_get_state / apv_set_state through
Engine.state_bytes / get_state / set_state): which names a configuration has, their byte counts, what a get -> set -> get leaves,
and which refusal a call gets.  Every list below is literal: a name that appears, disappears, changes its size or its refusal
fails here.

Shape: N = 32, H = 8, L = 4, M = 2, five-tap responses, ranks (1, 2), three hops before the state is read -- the rings then stand at
offset 24 and the hops run from their captured graphs.  The perceptual tables are synthetic ones of the stream's 17 bins (the model's own
need a block of 48 samples or more), as in test_gpu_stream_lifecycle.py.

Configurations, each with the float32 and the float64 front-end:
  (i)   everything that combines: statistics window T = 3, J = 8 taps with FIR synthesis, evaluation (Pv = 4, Mv = 2, both ranks)
        with spectra and detectability, perceptual weighting, responses reassigned before the last hop;
  (ii)  forgetting statistics (beta = 0.9) and nothing else;
  (iii) a plain stream of 16 loudspeakers (class apvast, python dialect: absolute loading, no bright loading).  With the float64
        front-end its joint diagonalisation is the order-16 kernel that reads grouped slabs (apv_gevd_reads_groups), so the device
        keeps the control-point spectra in groups of four bins and the getter regroups them; with the float32 front-end they are
        bin-major and can be set."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_stream import TOL, run_pair, synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import signal, validation_rirs  # noqa: E402

N, H, K, L, M, P = 32, 8, 17, 4, 2, 5
RANKS = (1, 2)
NV = len(RANKS)
REF_A, REF_B, DELAY = 0, 1, 2
T, J, PV, MV, E, Z = 3, 8, 4, 2, 2, 2
SETS, NHIST = Z * (2 * E + 1), Z * (E + 1)
HOPS = 3

RO = "{} is read-only"
UNKNOWN = "unknown state name: {}"
MISMATCH = "state size mismatch"
GROUPED = "the control-point spectra are recomputed by every hop and cannot be set"


def tables(nch, seed=4):
    return SimpleNamespace(G2=np.random.default_rng(seed).random((K, nch)) + 0.1, Cs=1.0, Ca=1.0, Leff=0.1)


def sizes(f64, l):
    """bytes of a real sample, a spectrum element, a filter coefficient, an eigenvalue / tap, a statistics element"""
    return SimpleNamespace(e1=8 if f64 else 4, e2=16 if f64 else 8, w=16 if f64 else 8, lam=8 if f64 else 4, stat=16 if f64 else 8,
                           C=l * M, n_out=2 * NV * l + 2 * l, slot=2 * l * l + l)


def base_names(f64, l, grouped=False):
    """name -> (bytes, refusal of a set of the right size or None, refusal of a set of one byte more): what every subband stream has"""
    q = sizes(f64, l)
    d = {}
    for p in range(4):
        d[f"response{p}"] = q.C * N * q.e1
        d[f"spectra{p}"] = K * q.C * q.e2
        d[f"fir_correction{p}"] = q.e1 * q.C * (P - 1)
    for z in range(2):
        d[f"target_response{z}"] = M * N * q.e1
        d[f"input_history{z}"] = (P - 1 + H) * q.e1
        d[f"target_spectra{z}"] = K * M * q.e2
        d[f"target_fir_correction{z}"] = q.e1 * M * (P - 1)
        d["w_" + "AB"[z]] = K * NV * l * q.w
        d["lambda_" + "AB"[z]] = K * l * q.lam
    d["input_block"] = 2 * N * q.e1
    d["out_overlap"] = q.n_out * N * q.e1
    d["input_spectrum"] = 2 * K * q.e2
    out = {k: (v, None, MISMATCH) for k, v in d.items()}
    if grouped:
        for p in range(4):
            out[f"spectra{p}"] = (K * q.C * q.e2, GROUPED, MISMATCH)              # the size is checked first
    out["signal_schedule"] = (8, RO.format("signal_schedule"), RO.format("signal_schedule"))
    return out


def names_all(f64):
    q = sizes(f64, L)
    out = base_names(f64, L)
    rw = {"weights0": K * M * q.e1, "weights1": K * M * q.e1,
          "w_time_A": NV * J * L * q.lam, "w_time_B": NV * J * L * q.lam,
          "fir_synth_taps_A": NV * J * L * q.lam, "fir_synth_taps_B": NV * J * L * q.lam,
          "fir_synth_history0": (J - 1) * q.e1, "fir_synth_history1": (J - 1) * q.e1,
          "eval_totals": 8 * Z * (3 * E + 1) * MV, "eval_history": NHIST * (PV - 1) * L * q.e1,
          "eval_spectra": 8 * Z * (3 * E + 1) * K * MV, "eval_ring": 8 * SETS * MV * N,
          "eval_detect": 8 * Z * 6 * E * MV,
          "stat_window0": T * K * q.slot * q.stat, "stat_window1": T * K * q.slot * q.stat, "stat_window_fill": 4}
    out.update({k: (v, None, MISMATCH) for k, v in rw.items()})
    # read-only on the device: the refusal comes before the size check; one hop in the last call, so one slot in the records
    for k, v in {"eval_pressure": 8 * SETS * H * MV, "eval_hops": 8 * Z * (3 * E + 1) * MV * 1,
                 "eval_detect_hops": 8 * Z * 2 * E * MV * 1}.items():
        out[k] = (v, RO.format(k), RO.format(k))
    out["stat_window_kernel_ms"] = (16, RO.format("stat_window_kernel_ms"), MISMATCH)    # here the size check comes first
    for k in ("filter_constraint_kernel_ms", "fir_synthesis_kernel_ms"):                 # host timers: a set does not know them
        out[k] = (16, UNKNOWN.format(k), UNKNOWN.format(k))
    return out


def names_forgetting(f64):
    q = sizes(f64, L)
    out = base_names(f64, L)
    for z in range(2):
        out[f"stat_forget{z}"] = (K * q.slot * q.stat, None, MISMATCH)
    out["stat_window_kernel_ms"] = (16, RO.format("stat_window_kernel_ms"), MISMATCH)
    return out


MISSPELT = ["respons0", "response4", "response00", "response", "w_C", "spectra", "target_response2", "fir_correction4",
            "stat_window2", "stat_forget2", "eval_rings", ""]


def engine(dtype, **kw):
    from ap_vast_unofficial_amd._capi import Engine
    return Engine(K, L, M, ranks=RANKS, compute_dtype=dtype, block_size=N, hop_size=H, n_zones=3, **kw)


def run_hops(eng, x, first, count):
    n_out = 2 * NV * eng.L + 2 * eng.L
    return [eng.process_block(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H], n_out) for h in range(first, first + count)]


def stream_all(dtype):
    eng = engine(dtype, stat_hops=T, filter_taps=J, synthesis="fir", evaluation=validation_rirs(PV, L, MV) + (list(RANKS),),
                 evaluation_spectra=True, evaluation_detectability=tables(5))
    rirA, rirB = synth_rirs(P, L, M, 1)
    eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    eng.stream_set_perceptual(tables(5), "python")
    x = signal(HOPS, H)
    run_hops(eng, x, 0, HOPS - 1)
    eng.stream_set_rirs(P, rir_A=synth_rirs(P, L, M, 7)[0])
    run_hops(eng, x, HOPS - 1, 1)
    return eng


def stream_forgetting(dtype):
    eng = engine(dtype, stat_forgetting=0.9)
    rirA, rirB = synth_rirs(P, L, M, 1)
    eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)
    run_hops(eng, signal(HOPS, H), 0, HOPS)
    return eng


def fetch(eng, name, nbytes):
    return eng.get_state(name, (nbytes,), np.uint8)


def refused(call, text):
    from ap_vast_unofficial_amd._capi import ApvError
    with pytest.raises(ApvError) as ei:
        call()
    assert f"libapvast_hip: {text} (code" in str(ei.value), (text, str(ei.value))


def check_names(eng, names, foreign):
    # sizes, and a get of one byte more
    for name, (nbytes, _, _) in names.items():
        assert nbytes > 0 and eng.state_bytes(name) == nbytes, (name, eng.state_bytes(name), nbytes)
        refused(lambda: fetch(eng, name, nbytes + 1), MISMATCH)
    before = {name: fetch(eng, name, nbytes) for name, (nbytes, _, _) in names.items()}
    # every array back in, in the order of the list ("stat_window_fill" behind the windows: it says where they now start), or the
    # refusal; then one byte more
    for name, (nbytes, no, no_big) in names.items():
        if no is None:
            eng.set_state(name, before[name])
        else:
            refused(lambda: eng.set_state(name, before[name]), no)
        refused(lambda: eng.set_state(name, np.zeros(nbytes + 1, np.uint8)), no_big)
    for name, (nbytes, _, _) in names.items():
        assert np.array_equal(fetch(eng, name, nbytes), before[name]), name
    for name in list(foreign) + MISSPELT:
        assert name not in names
        refused(lambda: eng.state_bytes(name), UNKNOWN.format(name))
        refused(lambda: fetch(eng, name, 8), UNKNOWN.format(name))
        refused(lambda: eng.set_state(name, np.zeros(8, np.uint8)), UNKNOWN.format(name))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_every_stage(dtype):
    f64 = dtype == "f64"
    eng = stream_all(dtype)
    names = names_all(f64)
    assert len(names) == 50
    check_names(eng, names, ["stat_forget0", "stat_forget1"])
    # the rings stand at offset 24: a ramp goes in and comes out in logical order
    sd = eng.s_dtype
    for name, shape, dt in (("response0", (L * M, N), sd), ("input_block", (2, N), sd), ("eval_ring", (SETS * MV, N), np.float64)):
        ramp = np.arange(np.prod(shape), dtype=dt).reshape(shape)
        eng.set_state(name, ramp)
        assert np.array_equal(eng.get_state(name, shape, dt), ramp), name
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_forgetting_only(dtype):
    eng = stream_forgetting(dtype)
    names = names_forgetting(dtype == "f64")
    assert len(names) == 31
    other = set(names_all(dtype == "f64")) - set(names)
    assert {"stat_window0", "stat_window_fill", "weights0", "w_time_A", "eval_ring", "filter_constraint_kernel_ms"} <= other
    check_names(eng, names, sorted(other))
    eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_plain_order_16(dtype):
    l = 16
    rirA, rirB = synth_rirs(P, l, M, 1)
    ap, orc, _, _ = run_pair(N, H, rirA, rirB, DELAY, REF_A, REF_B, NV, 1.0, hops=HOPS, dtype=dtype)
    eng = ap._eng
    f64 = dtype == "f64"
    names = base_names(f64, l, grouped=f64)
    assert len(names) == 28
    other = (set(names_all(f64)) | set(names_forgetting(f64))) - set(names)
    check_names(eng, names, sorted(other))
    # the spectra the getter hands out are bin-major [K][M][L] whatever the device keeps: against the oracle's, as
    # test_gpu_stream.check_last_hop_state compares them and to its tolerance
    for p in range(4):
        X = eng.get_state(f"spectra{p}", (K, M, l), eng.sc_dtype)
        ref = orc.spectra[p].transpose(0, 2, 1)
        err = np.abs(X - ref).max() / np.abs(ref).max()
        print(f"{dtype} spectra{p}: error {err:.2e} of the largest reference value")
        assert err <= TOL[dtype]["spec"], (p, err)
    ap.close()

"""Lifecycle of the stream states (csrc/apv_owned.h): everything a subband or broadband stream allocates -- device
buffers, page-locked blocks, events, streams -- is back when the engine is closed or the stream is initialised again, whatever
features ran in between; an init that fails half-way and a rejected perceptual call leave nothing behind and change nothing.

The counts are the library's own (apv_debug_live_resources: what all owners of the process hold), not the card's free memory,
which moves with the other processes on it.  Outputs are compared bit for bit: both sides run the same kernels on the same inputs."""
import gc
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_stream import synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import signal, validation_rirs  # noqa: E402

N, H, K = 32, 16, 17
L, M, RANKS = 4, 4, (1, 2)
REF_A, REF_B, DELAY = 0, 1, 2


def baseline():
    from ap_vast_unofficial_amd._capi import Engine
    gc.collect()                                   # engines earlier tests dropped without close() go now, not in the middle of a case
    return Engine.debug_live_resources()


def live():
    from ap_vast_unofficial_amd._capi import Engine
    return Engine.debug_live_resources()


def engine(dtype="f64", l=L, m=M, **kw):
    from ap_vast_unofficial_amd._capi import Engine
    return Engine(K, l, m, ranks=RANKS, compute_dtype=dtype, block_size=N, hop_size=H, n_zones=3, **kw)


def start(eng, P):
    rirA, rirB = synth_rirs(P, eng.L, eng.M, 1)
    eng.stream_init(rirA, rirB, REF_A, REF_B, DELAY)


def n_out(eng):
    return 2 * len(RANKS) * eng.L + 2 * eng.L


def hops(eng, x, first, count):
    return [eng.process_block(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H], n_out(eng)) for h in range(first, first + count)]


def whole(eng, x, first, count):
    return eng.process_signal(x[0, first * H:(first + count) * H], x[1, first * H:(first + count) * H], n_out(eng))


def tables(nch, seed=4):
    """perceptual tables of the stream's K bins (the model's own need a block of 48 samples or more)"""
    return SimpleNamespace(G2=np.random.default_rng(seed).random((K, nch)) + 0.1, Cs=1.0, Ca=1.0, Leff=0.1)


def evaluation(ranks=RANKS):
    return validation_rirs(9, L, 5) + (list(ranks),)


# 1 ---------------------------------------------------------------------------------------------------------------
def run_plain(eng, x):
    hops(eng, x, 0, 3)
    whole(eng, x, 3, 6)


def run_perceptual(eng, x):
    eng.stream_set_perceptual(tables(5), "python")
    hops(eng, x, 0, 2)
    eng.stream_set_perceptual(None, "python")
    hops(eng, x, 2, 2)
    eng.stream_set_perceptual(tables(7, seed=5), "python")           # the tables are replaced
    hops(eng, x, 4, 2)


def run_set_rirs(eng, x):
    hops(eng, x, 0, 2)
    eng.stream_set_rirs(eng._P, rir_A=synth_rirs(eng._P, L, M, 7)[0])
    hops(eng, x, 2, 2)
    eng.stream_set_rirs(eng._P, rir_B=synth_rirs(eng._P, L, M, 8)[1], target_rir_A=synth_rirs(eng._P, L, M, 9)[0][:, 0])
    hops(eng, x, 4, 2)


def run_statistics(eng, x):
    hops(eng, x, 0, 2)
    for _ in range(2):
        assert np.isfinite(eng.stream_statistics(0, want_U=True)[4]).all()


def run_signal_40(eng, x):
    assert np.isfinite(whole(eng, x, 0, 40)).all()


def run_signal_20(eng, x):
    assert np.isfinite(whole(eng, x, 0, 20)).all()


FEATURES = {
    "f32": (dict(dtype="f32"), 8, run_plain),
    "f64": (dict(), 8, run_plain),
    "window3": (dict(stat_hops=3), 8, run_plain),
    "forgetting": (dict(stat_forgetting=0.9), 8, run_plain),
    "taps8": (dict(filter_taps=8), 8, run_plain),
    "taps8_fir": (dict(filter_taps=8, synthesis="fir"), 8, run_plain),
    "taps8_fir_chunked": (dict(filter_taps=8, synthesis="fir"), 64, run_plain),
    "evaluation": (dict(evaluation=evaluation()), 8, run_plain),
    "evaluation_spectra": (dict(evaluation=evaluation(), evaluation_spectra=True), 8, run_plain),
    "perceptual": (dict(), 8, run_perceptual),
    "set_rirs": (dict(), 8, run_set_rirs),
    "set_rirs_fast_convolution": (dict(), 64, run_set_rirs),
    "statistics_twice": (dict(), 8, run_statistics),
    "signal_40_pipelined": (dict(), 8, run_signal_40),
    "signal_40_chunked": (dict(), 64, run_signal_40),
    "order40_chunked": (dict(l=40, m=40), 64, run_signal_20),
}


@pytest.mark.parametrize("name", list(FEATURES))
def test_every_feature_is_released(name):
    kw, P, run = FEATURES[name]
    base = baseline()
    eng = engine(**kw)
    eng._P = P
    start(eng, P)
    assert live() != base                          # the stream's buffers are counted at all
    run(eng, signal(40, H))
    eng.close()
    assert live() == base


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [8, 64])
def test_reinit_leaves_nothing_behind(P):
    """P = 8: the hop-by-hop pipeline of the whole-signal call; P = 64: the chunk schedule"""
    x = signal(5, H)
    base = baseline()
    fresh = engine()
    start(fresh, P)
    ref = whole(fresh, x, 0, 5).copy()
    fresh.close()
    assert live() == base
    eng = engine()
    start(eng, P)
    first = live()
    whole(eng, x, 0, 5)
    assert live() != first                         # the whole-signal path made its own buffers, events and streams
    start(eng, P)
    assert live() == first
    assert np.array_equal(whole(eng, x, 0, 5), ref)
    eng.close()
    assert live() == base


def bb_engine():
    from ap_vast_unofficial_amd import _capi
    eng = _capi.Engine(K, L, M, ranks=(1,), compute_dtype="f64", block_size=N, hop_size=H, n_zones=3, dialect="python",
                       reg_mode=_capi.REG_ABS, reg_dark=1e-7)
    eng.bb_set_rank_list([])
    return eng


def bb_run(eng, x):
    """one hop alone, then whole signals of 2 and of 4 hops: the group buffers and both page-locked stagings are replaced"""
    rirA, rirB = synth_rirs(8, L, M, 1)
    eng.bb_init(rirA, rirB, REF_A, REF_B, DELAY, 4, 48, 2)
    after_init = live()
    no = 2 * 2 * L + 2 * L
    out = [eng.bb_process_block(x[0, :H], x[1, :H], no).copy()]
    out.append(eng.bb_process_signal(x[0, H:3 * H], x[1, H:3 * H], no).copy())
    out.append(eng.bb_process_signal(x[0, 3 * H:7 * H], x[1, 3 * H:7 * H], no).copy())
    return after_init, out


def test_broadband_reinit_leaves_nothing_behind():
    x = signal(7, H)
    base = baseline()
    fresh = bb_engine()
    _, ref = bb_run(fresh, x)
    fresh.close()
    assert live() == base
    eng = bb_engine()
    first, _ = bb_run(eng, x)
    assert live() != first
    second, out = bb_run(eng, x)
    assert second == first
    for a, b in zip(out, ref):
        assert np.array_equal(a, b)
    eng.close()
    assert live() == base


# 3 ---------------------------------------------------------------------------------------------------------------
def test_failed_init_is_cleaned_up():
    """an evaluated rank that the rank list no longer holds: apv_stream_init finds out after the response banks and their spectra
    are allocated, and returns APV_ERR_ARG"""
    from ap_vast_unofficial_amd import _capi
    x = signal(5, H)
    base = baseline()
    fresh = engine(evaluation=evaluation([2]))
    start(fresh, 64)
    ref = np.stack(hops(fresh, x, 0, 5))
    fresh.close()
    eng = engine(evaluation=evaluation([2]))
    eng.set_rank_list([1])
    with pytest.raises(_capi.ApvError) as err:
        start(eng, 64)
    assert err.value.code == _capi.ERR_ARG
    assert live() == base                          # the half-built stream is gone already
    eng.set_rank_list(list(RANKS))
    start(eng, 64)
    assert np.array_equal(np.stack(hops(eng, x, 0, 5)), ref)
    eng.close()
    assert live() == base


# 4 ---------------------------------------------------------------------------------------------------------------
def stored_hop(eng):
    """what the last hop left on the device, read through the layout the stream believes it has: R_B, R_D, r of zone A and the
    bright spectra"""
    return eng.stream_statistics(0, want_U=False)[:3] + (eng.get_state("spectra0", (K, eng.L * eng.M), eng.sc_dtype),)


def test_rejected_perceptual_call_changes_nothing():
    """float64 at order 16: the spectra are kept in groups of four bins, which the weighting would undo.  Right after the rejected
    call, before any hop rewrites them, the stored spectra and the statistics formed from them read as in a stream that never
    made the call (with the layout switched they would be regrouped wrongly); then the next hops are the same too."""
    from ap_vast_unofficial_amd import _capi
    x = signal(6, H)
    base = baseline()
    plain = engine(l=16, m=16)
    start(plain, 8)
    ref = hops(plain, x, 0, 2)
    ref_stored = stored_hop(plain)
    assert all(np.abs(a).max() > 0 for a in ref_stored)
    ref += hops(plain, x, 2, 4)
    plain.close()
    eng = engine(l=16, m=16)
    start(eng, 8)
    got = hops(eng, x, 0, 2)
    with pytest.raises(_capi.ApvError) as err:
        eng.stream_set_perceptual(tables(513), "python")
    assert err.value.code == _capi.ERR_ARG
    for a, b in zip(stored_hop(eng), ref_stored):
        assert np.array_equal(a, b)
    got += hops(eng, x, 2, 4)
    assert np.array_equal(np.stack(got), np.stack(ref))
    eng.close()
    assert live() == base

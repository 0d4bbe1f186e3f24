"""Kernels of the broadband stream's evaluation stage (apv_eval_energies, csrc/kernels_bbeval.hip; apv_eval_pressure over a group
of hops): the energy reduction against NumPy, its independence of the launch, the property the group launch of
apv_bb_process_signal rests on, and the refusals of the new entries.

Bounds, derived (not measured).  An energy of H squared float64 samples summed in any order errs by at most about H u E,
u = 2^-53, and the NumPy reference carries the same: energy_bound(H) = (H + 8) u (tests/evaluation_oracle.py).  The error energy
squares differences p_target - p_bright that both sides form from the same float64 pressures, exactly alike.  Totals are one
addition per hop in hop order: bit for bit the in-order sum of the device's own record."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from evaluation_oracle import energy_bound  # noqa: E402

GUARD = -777.0


def reference(p, H):
    """p (Z, 2 E + 1, n H, Mv) -> (n, Z, 3 E + 1, Mv): [bright of the E ranks | dark | error | target] per hop"""
    Z, S, T, Mv = p.shape
    E, n = (S - 1) // 2, T // H
    q = p.reshape(Z, S, n, H, Mv)
    out = np.empty((n, Z, 3 * E + 1, Mv))
    out[:, :, :2 * E] = np.sum(q[:, :2 * E] ** 2, axis=3).transpose(2, 0, 1, 3)
    out[:, :, 2 * E:3 * E] = np.sum((q[:, 2 * E:2 * E + 1] - q[:, :E]) ** 2, axis=3).transpose(2, 0, 1, 3)
    out[:, :, 3 * E] = np.sum(q[:, 2 * E] ** 2, axis=2).transpose(1, 0, 2)
    return out


@pytest.fixture(scope="module")
def eng():
    from ap_vast_unofficial_amd._capi import Engine
    e = Engine(9, 4, 4)
    yield e
    e.close()


@pytest.mark.parametrize("H", [1, 16, 63, 64, 65, 130])
def test_energies_against_numpy(eng, H):
    """the wave-width edges of H, one microphone, a remainder tile and more than one tile of 16, one and two programs and ranks, one
    hop and three"""
    rng = np.random.default_rng(100 + H)
    worst = 0.0
    for Mv in (1, 5, 17):
        for E in (1, 2):
            for Z in (1, 2):
                for n in (1, 3):
                    p = rng.standard_normal((Z, 2 * E + 1, n * H, Mv))
                    start = rng.standard_normal((Z, 3 * E + 1, Mv)) ** 2
                    rec, tot = eng.eval_energies(p, H, totals=start)
                    ref = reference(p, H)
                    assert rec.shape == ref.shape == (n, Z, 3 * E + 1, Mv) and tot.shape == start.shape
                    err = np.abs(rec - ref)
                    worst = max(worst, (err / ref).max() / energy_bound(H))
                    assert np.all(err <= energy_bound(H) * ref), (Mv, E, Z, n, worst)
                    run = start.copy()
                    for i in range(n):
                        run = run + rec[i]
                    assert np.array_equal(tot, run), (Mv, E, Z, n)
    print(f"H={H}: largest energy error / bound {worst:.3f}")


@pytest.mark.parametrize("H,Mv,E,Z", [(16, 5, 2, 2), (65, 17, 1, 1), (130, 1, 2, 2)])
def test_energies_do_not_depend_on_the_launch(eng, H, Mv, E, Z):
    """one launch over three hops == three launches over one hop each, record and totals bit for bit; the words around the record
    and the totals stay untouched"""
    rng = np.random.default_rng(7 * H + Mv)
    n, pad, slot = 3, 64, Z * (3 * E + 1) * Mv
    p = rng.standard_normal((Z, 2 * E + 1, n * H, Mv))
    start = rng.standard_normal(slot) ** 2
    f = eng.lib.apv_eval_energies

    def buffers():
        rec = np.full(pad + n * slot + pad, GUARD)
        tot = np.full(pad + slot + pad, GUARD)
        tot[pad:pad + slot] = start
        return eng.to_device(rec), eng.to_device(tot)

    def inner(buf, doubles):
        return ctypes.c_void_p(buf.ptr.value + 8 * doubles)

    def fetch(dr, dt):
        rec, tot = dr.download((pad + n * slot + pad,), np.float64), dt.download((pad + slot + pad,), np.float64)
        for b in (rec, tot):
            assert np.all(b[:pad] == GUARD) and np.all(b[-pad:] == GUARD)
        return rec[pad:-pad].reshape(n, Z, 3 * E + 1, Mv), tot[pad:-pad].reshape(Z, 3 * E + 1, Mv)

    dp = eng.to_device(p)
    dr, dt = buffers()
    eng._chk(f(eng.h, dp.ptr, Z, E, H, Mv, n, inner(dr, pad), inner(dt, pad)))
    rec3, tot3 = fetch(dr, dt)
    for b in (dp, dr, dt):
        b.free()
    dr, dt = buffers()
    for i in range(n):
        dh = eng.to_device(np.ascontiguousarray(p[:, :, i * H:(i + 1) * H]))
        eng._chk(f(eng.h, dh.ptr, Z, E, H, Mv, 1, inner(dr, pad + i * slot), inner(dt, pad)))
        eng.sync()
        dh.free()
    rec1, tot1 = fetch(dr, dt)
    for b in (dr, dt):
        b.free()
    assert np.array_equal(rec3, rec1) and np.array_equal(tot3, tot1)
    # and through the wrapper, which starts from zeros
    rec, tot = eng.eval_energies(p, H)
    assert np.array_equal(rec, rec3)


@pytest.mark.parametrize("Pv", [1, 9, 120])
@pytest.mark.parametrize("H", [16, 96])
def test_pressure_launch_over_a_group_equals_three_hops(eng, H, Pv):
    """One apv_eval_pressure launch over 3 H samples == three launches over H samples with the history advanced by hand, bit for
    bit: what lets apv_bb_process_signal evaluate a group of hops in one launch.  At H = 96 the long launch (288 samples) runs four
    sample tiles per workgroup and the short ones one."""
    rng = np.random.default_rng(1000 * Pv + H)
    for L, Mv, G in ((3, 5, 2), (16, 17, 1)):
        y = rng.standard_normal((G, Pv - 1 + 3 * H, L))
        rv = rng.standard_normal((Pv, L, Mv))
        whole = eng.eval_pressure(y, rv, 3 * H)
        assert whole.shape == (G, 3 * H, Mv)
        for i in range(3):
            part = eng.eval_pressure(y[:, i * H:Pv - 1 + (i + 1) * H], rv, H)
            assert np.array_equal(whole[:, i * H:(i + 1) * H], part), (L, Mv, G, i)


def test_entry_refusals(eng):
    from ap_vast_unofficial_amd import _capi
    d = eng.alloc(1 << 16)
    f = eng.lib.apv_eval_energies
    assert f(eng.h, None, 1, 1, 4, 2, 1, d.ptr, d.ptr) == _capi.ERR_ARG
    assert f(eng.h, d.ptr, 1, 1, 4, 2, 1, None, d.ptr) == _capi.ERR_ARG
    assert f(eng.h, d.ptr, 1, 1, 4, 2, 1, d.ptr, None) == _capi.ERR_ARG
    for bad in ((0, 1, 4, 2, 1), (3, 1, 4, 2, 1), (1, 0, 4, 2, 1), (1, 1, 0, 2, 1), (1, 1, 4, 0, 1), (1, 1, 4, 2, 0), (1, 1, 4, 2, -1),
                (1, 1, 1 << 30, 2, 2)):                                            # the last: n_hops x H reaches 2^31
        assert f(eng.h, d.ptr, *bad, d.ptr, d.ptr) == _capi.ERR_ARG, bad
        assert eng.lib.apv_last_error(eng.h)
    d.free()
    with pytest.raises(ValueError):
        eng.eval_energies(np.zeros((1, 2, 8, 2)), 4)              # an even number of pressure sets
    with pytest.raises(ValueError):
        eng.eval_energies(np.zeros((1, 3, 9, 2)), 4)              # not a whole number of hops
    # the stream's entries without a broadband stream
    rv = np.ones((5, 4, 2))
    r1 = np.array([1], dtype=np.int32)
    ptr = _capi._ptr
    assert eng.lib.apv_bb_set_evaluation(eng.h, 5, 2, ptr(rv), ptr(rv), 1, ptr(r1)) == _capi.ERR_ARG
    assert eng.lib.apv_bb_reset_evaluation(eng.h) == _capi.ERR_ARG


def test_channel_major_stream_evaluates_hop_by_hop():
    """cfg.out_layout = 0 emits [n_out][H]: apv_bb_process_signal evaluates such a stream hop by hop, through strides.  The same
    stream with out_layout = 1 (one launch per group) emits the same samples and keeps the same evaluation, bit for bit."""
    from ap_vast_unofficial_amd import _capi
    rng = np.random.default_rng(4)
    L, M, P, N, H, J, V, hops, Pv, Mv = 3, 4, 10, 32, 16, 4, 3, 19, 20, 5
    rirA, rirB = rng.standard_normal((2, P, L, M)) * 1e-3
    rv = rng.standard_normal((2, Pv, L, Mv))
    x = rng.standard_normal((2, hops * H))
    n_out = 2 * V * L + 2 * L
    got = []
    for layout in (0, 1):
        eng = _capi.Engine(N // 2 + 1, L, M, block_size=N, hop_size=H, n_zones=3, out_layout=layout, reg_mode=_capi.REG_ABS, reg_dark=1e-7)
        eng.bb_set_rank_list([])
        eng.bb_init(rirA, rirB, 1, 2, 1, J, 4 * N, V)
        noise = np.random.default_rng(1)                     # the start buffers of the Python dialect (apvast.py:124-129)
        for p in range(4):
            eng.bb_set_state(f"response{p}", 1e-3 * noise.standard_normal((M, L, N)))
        for z in range(2):
            eng.bb_set_state(f"target_response{z}", 1e-3 * noise.standard_normal((M, N)))
        eng.bb_set_evaluation(rv[0], rv[1], [1, 3])
        out = eng.bb_process_signal(x[0], x[1], n_out)
        if layout == 0:                                      # (hops, n_out, H) -> (groups, hops H, L)
            out = out.reshape(hops, n_out // L, L, H).transpose(1, 0, 3, 2).reshape(n_out // L, hops * H, L)
        got.append((out, eng.bb_get_state("eval_hops", (hops, 2, 7, Mv)), eng.bb_get_state("eval_totals", (2, 7, Mv)),
                    eng.bb_get_state("eval_pressure", (2, 5, H, Mv)), eng.bb_get_state("eval_history", (2, 3, Pv - 1, L))))
        eng.close()
    for a, b in zip(*got):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert np.all(got[0][1] > 0.0)
    # the history is the tail of what was emitted: program A's rank 1 is group 0, its target group 2 V
    assert np.array_equal(got[1][4][0, 0], got[1][0][0, -(Pv - 1):]) and np.array_equal(got[1][4][0, 2], got[1][0][2 * V, -(Pv - 1):])


def test_stream_entry_refusals():
    from ap_vast_unofficial_amd import _capi
    rng = np.random.default_rng(3)
    L, M, P, N, H, J = 3, 4, 10, 32, 16, 4
    rirA, rirB = rng.standard_normal((2, P, L, M))
    eng = _capi.Engine(N // 2 + 1, L, M, block_size=N, hop_size=H, n_zones=3, out_layout=1, reg_mode=_capi.REG_ABS, reg_dark=1e-7)
    eng.bb_set_rank_list([])
    eng.bb_init(rirA, rirB, 1, 2, 1, J, 4 * N, 3)
    rv = np.ones((5, L, 2))
    s, ptr = eng.lib.apv_bb_set_evaluation, _capi._ptr
    r13, r31, r11, r4 = (np.array(v, dtype=np.int32) for v in ([1, 3], [3, 1], [1, 1], [4]))
    assert eng.lib.apv_bb_reset_evaluation(eng.h) == _capi.ERR_ARG                 # the stage is off
    with pytest.raises(_capi.ApvError):
        eng.bb_get_state("eval_totals", (2, 7, 2))
    assert s(eng.h, 5, 2, None, ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), None, 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, None) == _capi.ERR_ARG
    assert s(eng.h, 0, 2, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 0, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 20466, 2, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG      # the window does not fit LDS
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 0, ptr(r13)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 4, ptr(r13)) == _capi.ERR_ARG          # more ranks than the stream emits
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, ptr(r31)) == _capi.ERR_ARG          # not ascending
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, ptr(r11)) == _capi.ERR_ARG
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 1, ptr(r4)) == _capi.ERR_ARG           # not emitted
    assert eng.lib.apv_last_error(eng.h)
    with pytest.raises(ValueError):
        eng.bb_set_evaluation(np.ones((5, L + 1, 2)), np.ones((5, L + 1, 2)), [1])
    eng.bb_set_evaluation(rv, rv, [1, 3])
    assert s(eng.h, 5, 2, ptr(rv), ptr(rv), 2, ptr(r13)) == _capi.ERR_ARG          # a second call
    # two programs, two ranks: 2 * 5 sets, 2 * 7 energies, 2 * 3 histories of 4 samples
    assert np.all(eng.bb_get_state("eval_totals", (2, 7, 2)) == 0.0)
    assert np.all(eng.bb_get_state("eval_history", (2, 3, 4, L)) == 0.0)
    assert np.all(eng.bb_get_state("eval_pressure", (2, 5, H, 2)) == 0.0)
    for name, shape in (("eval_totals", (2, 7, 3)), ("eval_history", (2, 3, 5, L)), ("eval_pressure", (2, 5, H, 3)), ("eval_hops", (1, 2, 7, 2))):
        with pytest.raises(_capi.ApvError):
            eng.bb_get_state(name, shape)                                          # a size mismatch; no hop yet: "eval_hops" is empty
    for name, shape in (("eval_pressure", (2, 5, H, 2)), ("eval_hops", (1, 2, 7, 2))):
        with pytest.raises(_capi.ApvError, match="read-only"):
            eng.bb_set_state(name, np.zeros(shape))
    eng.bb_set_state("eval_totals", np.full((2, 7, 2), 2.5))
    assert np.all(eng.bb_get_state("eval_totals", (2, 7, 2)) == 2.5)
    eng.bb_reset_evaluation()
    assert np.all(eng.bb_get_state("eval_totals", (2, 7, 2)) == 0.0)
    eng.close()

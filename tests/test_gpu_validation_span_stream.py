"""The rank choice by validation contrast in the subband stream (apvast(..., validation_floor_db=), apv_stream_set_validation_span /
apv_get_validation_span) against tests/validation_span_oracle.py.  N = 32, H = 16 (17 bins), 4 hops, validation responses Pv = 9,
Mv = 5 made as in tests/test_gpu_stream_evaluation.py, V = L.

Bounds.  With t = TOL[dtype]["w_max"] (tests/test_gpu_stream.py) the device's filter is w (1 + e), |e| <= t, and an energy is
quadratic in it: |got - ref| <= (2 t + t^2) ||G[k]||_F^2 |w_t|^2.  A slot is DECIDED when the oracle's margin |bright - phi dark|
exceeds that bound (bright's plus phi times dark's); a bin, when all its slots are and, where its first slots are inadmissible, the
cross-multiplied comparisons of their running best have margins too.  In every slot the device's decisions must be the definition
applied to its own energies, exactly; in decided slots its admissibility is the oracle's, in decided bins its sources and filters.

The floor.  The filters do not depend on the floor (the stage only copies), so a run of the oracle without a floor gives the
contrast curves the floors are set from.  In float64 the bound is 2e-7 of ||G||^2 |w|^2 and a floor at the median of the curves
leaves every slot decided (asserted).  In float32 / mixed it is 2 % of ||G||^2 |w|^2, about 0.02 L of an energy: at the median of
curves that span some 8 dB, 23 % (L = 4) to 7 % (L = 16) of the slots would be decided.  There the (2, K) table takes per program
and bin the value NEAREST the median at which every slot of the bin is decided (the undecided values of a slot form an interval;
the table entry is the end of one nearest the median that lies in no other).  Both branches still occur, over the bins (asserted),
and the share of decided slots is asserted from the oracle alone to be at least 90 % before the device is looked at.  Observed on
the hops that are checked: 100 % in float64, 99.6 % to 100 % in float32 / mixed; of the bins, 100 % and 24 % to 71 %."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_gpu_stat_window import hop, same_outputs  # noqa: E402
from test_gpu_stream import TOL, check_outputs, synth_rirs  # noqa: E402
from test_gpu_stream_evaluation import validation_rirs  # noqa: E402
from validation_span_oracle import (ValidationConstrainedOracle, ValidationForgettingOracle, ValidationSubbandOracle, choose,  # noqa: E402
                                    decide, transfer)

N, H, HOPS, K, PV, MV, P = 32, 16, 4, 17, 9, 5, 12
DELAY, REF_A, REF_B, MU = 3, 1, 2, 1.0
DTYPES = ["f64", "mixed", "f32"]
SHAPES = [(4, 6), (16, 20)]
X = np.random.default_rng(99).standard_normal((2, HOPS * H))


def db(lin):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(lin)


def oracle(L, M, floor, cls=ValidationSubbandOracle, run=(True, True), **okw):
    rirA, rirB = synth_rirs(P, L, M, 1)
    rvA, rvB = validation_rirs(PV, L, MV)
    rs = np.random.RandomState(0)
    init_r = np.stack([1e-3 * rs.randn(N, L, M) for _ in range(4)])
    init_t = np.stack([1e-3 * rs.randn(N, M) for _ in range(2)])
    return cls(N, rirA, rirB, DELAY, REF_A, REF_B, list(range(1, L + 1)), MU, hop_size=H, init_response=init_r,
               init_target_response=init_t, run_A=run[0], run_B=run[1], rv_A=rvA, rv_B=rvB, validation_floor=floor, **okw)


def device(L, M, floor_db, dtype="f64", run=(True, True), validate=True, **kw):
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 1)
    if validate:
        rvA, rvB = validation_rirs(PV, L, MV)
        kw.update(validation_rir_A=rvA, validation_rir_B=rvB)
    return apvast(N, rirA, rirB, kw.pop("filter_length", 16), DELAY, REF_A, REF_B, L, MU, 4 * N, hop_size=H, run_A=run[0], run_B=run[1],
                  perceptual=False, seed=0, dtype=dtype, validation_floor_db=floor_db, **kw)


def bounds(orc, z, dtype):
    """the energy bounds (bright, dark), (K, V), of zone program z from the oracle's filters of the last hop"""
    t = TOL[dtype]["w_max"]
    G = orc.validation_G
    w2 = (np.abs(orc.w_unchosen[z]) ** 2).sum(-1)
    f = 2 * t + t * t
    return f * (np.abs(G[z]) ** 2).sum((1, 2))[:, None] * w2, f * (np.abs(G[1 - z]) ** 2).sum((1, 2))[:, None] * w2


def decided(orc, z, dtype):
    """(slots (K, V), bins (K,)) of zone program z that are decided on the oracle's last hop"""
    b, d, phi = orc.validation_bright[z], orc.validation_dark[z], orc.validation_floor[z][:, None]
    bb, bd = bounds(orc, z, dtype)
    slots = np.abs(b - phi * d) > bb + phi * bd
    bins = slots.all(axis=1)
    adm = b >= phi * d
    for k in np.nonzero(bins & ~adm[:, 0])[0]:
        n = adm.shape[1] if not adm[k].any() else int(np.argmax(adm[k]))       # the leading slots without an admissible one
        for i in range(n):
            for j in range(i + 1, n):
                slack = bb[k, i] * d[k, j] + b[k, i] * bd[k, j] + bb[k, j] * d[k, i] + b[k, j] * bd[k, i] + bb[k, i] * bd[k, j] + bb[k, j] * bd[k, i]
                bins[k] = bins[k] and abs(b[k, i] * d[k, j] - b[k, j] * d[k, i]) > slack
    return slots, bins


def floor_near(b, d, bb, bd, target):
    """the value nearest `target` (in dB) among those at which the most slots of the curves b, d (with energy bounds bb, bd) are
    decided -- every slot, unless the slots' undecided intervals cover the whole axis between them"""
    lo = np.maximum(b - bb, 0.0) / (d + bd)
    with np.errstate(divide="ignore"):
        hi = np.where(d > bd, (b + bb) / np.where(d > bd, d - bd, 1.0), np.inf)
    cand = [target] + [p for p in np.concatenate([lo * (1 - 1e-3), hi[np.isfinite(hi)] * (1 + 1e-3)]) if p > 0]
    return min(cand, key=lambda p: (int(((lo <= p) & (p <= hi)).sum()), abs(np.log(p / target))))


def curves(L, M, dtype, cls=ValidationSubbandOracle, run=(True, True), **okw):
    """the oracle without a floor, hop by hop: per hop and zone program (bright, dark, bound_b, bound_d)"""
    orc = oracle(L, M, np.zeros((2, K)), cls, run, **okw)
    out = []
    for h in range(HOPS):
        hop(orc, X, h, H)
        out.append([(orc.validation_bright[z], orc.validation_dark[z]) + bounds(orc, z, dtype) if run[z] else None for z in range(2)])
    return out


def table_from(cv, kind, run=(True, True)):
    """a floor (linear) of the kind asked for from one hop's curves: "scalar" the median of every contrast, "row" (K,) the per-bin
    median over both programs, "table" (2, K) per program and bin the decided value nearest the program's median"""
    live = [z for z in range(2) if run[z]]
    con = {z: cv[z][0] / cv[z][1] for z in live}
    if kind == "scalar":
        return float(np.median(np.concatenate([con[z].ravel() for z in live])))
    if kind == "row":
        return np.median(np.concatenate([con[z] for z in live], axis=1), axis=1)
    t = np.ones((2, K))
    for z in live:
        med = np.median(con[z])
        t[z] = [floor_near(*(a[k] for a in cv[z]), med) for k in range(K)]
    return t


def check_zone(ap, orc, z, dtype, tag=""):
    """the last hop's outputs and filters of zone program z; the share of decided slots is asserted first, from the oracle alone"""
    name, tol = "AB"[z], TOL[dtype]
    slots, bins = decided(orc, z, dtype)
    ob, od, phi = orc.validation_bright[z], orc.validation_dark[z], orc.validation_floor[z]
    adm_o = ob >= phi[:, None] * od
    print(f"{tag} {dtype} {name}: decided slots {slots.mean():.3f}, decided bins {bins.mean():.3f}, admissible {adm_o.mean():.2f}")
    assert slots.mean() >= 0.9
    if dtype == "f64":
        assert slots.all() and bins.all()
    b, d, src, rank, w = (getattr(ap, a + name) for a in ("validation_bright_", "validation_dark_", "validation_source_",
                                                          "validation_rank_", "w_"))
    V = ob.shape[1]
    assert b.shape == d.shape == src.shape == (K, V) and rank.shape == (K,)
    assert b.dtype == d.dtype == np.float64 and src.dtype == rank.dtype == np.int32
    bb, bd = bounds(orc, z, dtype)
    print(f"    energies at {max((np.abs(b - ob) / bb).max(), (np.abs(d - od) / bd).max()):.2e} of their bound")
    assert (np.abs(b - ob) <= bb).all() and (np.abs(d - od) <= bd).all()
    # every slot: what the definition gives on the device's own energies
    src_d, top_d = decide(b, d, phi)
    assert np.array_equal(src, src_d) and np.array_equal(rank, top_d)             # the ranks are 1 .. V
    # decided slots: the oracle's admissibility; decided bins: its sources, rank and filters
    assert np.array_equal((b >= phi[:, None] * d)[slots], adm_o[slots])
    assert np.array_equal(src[bins], orc.validation_src[z][bins]) and np.array_equal(rank[bins], orc.validation_rank[z][bins])
    wr = orc.w[z].transpose(1, 0, 2)
    err = (np.linalg.norm(w - wr, axis=-1) / np.linalg.norm(wr, axis=-1))[:, bins]
    assert np.median(err) < tol["w_med"] and err.max() < tol["w_max"], (name, np.median(err), err.max())
    return bins.all()


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,M", SHAPES)
def test_table_vs_oracle_with_a_floor_reassigned(L, M, dtype):
    """a (2, K) floor from the curves of hop 1, another from those of hop 3 assigned before hop 2; checked after hops 1 and 3"""
    cv = curves(L, M, dtype)
    t1, t3 = table_from(cv[1], "table"), table_from(cv[3], "table")
    ap, orc = device(L, M, db(t1), dtype), oracle(L, M, t1)
    assert ap.validation_bright_A is None and ap.validation_rank_B is None                  # before the first hop
    got, exp, whole = [], [], True
    for h in range(HOPS):
        if h == 2:
            ap.validation_floor_db = db(t3)
            orc.validation_floor = t3
        got.append(hop(ap, X, h, H))
        exp.append(hop(orc, X, h, H))
        if h in (1, 3):
            for z in range(2):
                whole = check_zone(ap, orc, z, dtype, f"L={L} hop {h}") and whole
                adm = orc.validation_src[z] == np.arange(L)
                assert adm.any() and (~adm).any()                                            # both branches occur
        elif dtype == "f64":
            for z in range(2):
                assert decided(orc, z, dtype)[1].all()
    if dtype == "f64":
        assert whole
        check_outputs(got, exp, TOL[dtype]["out"], TOL[dtype]["tgt"])
    assert np.array_equal(ap.validation_floor_db, db(t3))
    with pytest.raises(ValueError, match="validation_floor_db"):
        ap.validation_floor_db = None
    with pytest.raises(ValueError, match="validation_floor_db"):
        ap.validation_floor_db = np.full(K, np.nan)
    ap.close()


@pytest.mark.parametrize("kind", ["scalar", "row"])
@pytest.mark.parametrize("run", [(True, False), (False, True), (True, True)])
def test_floor_kinds_and_zone_programs(kind, run):
    L, M = SHAPES[0]
    floor = table_from(curves(L, M, "f64", run=run)[3], kind, run)
    ap, orc = device(L, M, db(floor), "f64", run), oracle(L, M, floor, run=run)
    got, exp = [], []
    for h in range(HOPS):
        got.append(hop(ap, X, h, H))
        exp.append(hop(orc, X, h, H))
        for z in range(2):
            if run[z]:
                assert check_zone(ap, orc, z, "f64", f"{kind} hop {h}")
    check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    for z in range(2):
        if not run[z]:
            assert all(getattr(ap, f"validation_{q}_{'AB'[z]}") is None for q in ("bright", "dark", "source", "rank"))
        else:
            adm = orc.validation_src[z] == np.arange(L)
            assert adm.any() and (~adm).any()
    assert ap.validation_floor_db.shape == (2, K)
    ap.close()


# 2 ---------------------------------------------------------------------------------------------------------------
COMBOS = {
    "effort": (ValidationSubbandOracle, dict(effort_limit=np.full((2, K), 10.0 ** -1.2)), dict(effort_limit_db=-12.0)),
    "wola": (ValidationConstrainedOracle, dict(filter_taps=8), dict(filter_length=8, constrain_filter_length=True)),
    "fir": (ValidationConstrainedOracle, dict(filter_taps=8), dict(filter_length=8, constrain_filter_length=True, synthesis="fir")),
    "window": (ValidationSubbandOracle, dict(stat_hops=3), dict(statistics_hops=3)),
    "forgetting": (ValidationForgettingOracle, dict(beta=0.9), dict(statistics_forgetting=0.9)),
    "span": (ValidationSubbandOracle, dict(floor_db=2.0), dict(contrast_floor_db=2.0)),
}


@pytest.mark.parametrize("combo", list(COMBOS))
def test_composition_vs_oracle(combo):
    """the stage between the span and the effort limit / the projection: the later stages act on the chosen filters"""
    L, M = SHAPES[0]
    cls, okw, kw = COMBOS[combo]
    floor = table_from(curves(L, M, "f64", cls, **okw)[3], "table")
    ap, orc = device(L, M, db(floor), "f64", **kw), oracle(L, M, floor, cls, **okw)
    got, exp = [], []
    for h in range(HOPS):
        got.append(hop(ap, X, h, H))
        exp.append(hop(orc, X, h, H))
        for z in range(2):
            slots, bins = decided(orc, z, "f64")
            # (the span leaves copies of one filter in several slots: their contrasts tie, and which of them is the running
            # best is decided by the last bit.  The filters are the same either way)
            assert slots.all() and (bins.all() or combo == "span"), (h, z)
    if combo != "fir":                                     # (the oracle synthesises by overlap-add)
        check_outputs(got, exp, TOL["f64"]["out"], TOL["f64"]["tgt"])
    for z, name in enumerate("AB"):
        bins = decided(orc, z, "f64")[1]
        assert np.array_equal(getattr(ap, "validation_source_" + name)[bins], orc.validation_src[z][bins])
        assert np.array_equal(getattr(ap, "validation_rank_" + name)[bins], orc.validation_rank[z][bins])
        bb, bd = bounds(orc, z, "f64")
        assert (np.abs(getattr(ap, "validation_bright_" + name) - orc.validation_bright[z]) <= bb).all()
        assert (np.abs(getattr(ap, "validation_dark_" + name) - orc.validation_dark[z]) <= bd).all()
        assert (orc.validation_src[z] != np.arange(L)).any()
        wr = orc.w[z].transpose(1, 0, 2)                   # chosen, then limited / projected
        err = np.linalg.norm(getattr(ap, "w_" + name) - wr, axis=-1) / np.linalg.norm(wr, axis=-1)
        assert np.median(err) < TOL["f64"]["w_med"] and err.max() < TOL["f64"]["w_max"], (name, np.median(err), err.max())
        if combo in ("wola", "fir"):
            tr, tg = orc.w_time[z], np.asarray(getattr(ap, "w_time_" + name))
            assert tg.shape == tr.shape and np.abs(tg - tr).max() <= TOL["f64"]["w_max"] * np.abs(tr).max()
        if combo == "effort":
            assert (orc.effort[z] > orc.effort_limit[z][:, None]).any()
            assert np.array_equal(getattr(ap, "effort_rank_" + name), orc.effort_rank[z])
        if combo == "span":
            assert np.array_equal(getattr(ap, "span_rank_" + name), orc.span_rank[z])
    ap.close()


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_process_signal_equals_hop_loop(dtype):
    L, M = SHAPES[1]
    hops = 6
    x = np.random.default_rng(7).standard_normal((2, hops * H))
    floor = db(table_from(curves(L, M, dtype)[3], "scalar"))
    a, b = (device(L, M, floor, dtype) for _ in range(2))
    loop = [hop(a, x, h, H) for h in range(hops)]
    sig = b.process_signal(x[0], x[1])
    assert tuple(b.signal_schedule) == (0, hops)
    for q in range(4):
        for v in range(len(sig[q])):
            assert np.array_equal(np.concatenate([o[q][v] for o in loop]), sig[q][v]), (q, v)
    for z in "AB":
        for name in ("w_", "validation_bright_", "validation_dark_", "validation_source_", "validation_rank_"):
            assert np.array_equal(getattr(a, name + z), getattr(b, name + z)), name + z
        assert (getattr(a, "validation_source_" + z) != np.arange(L)).any()                 # the choice acts
    a.close()
    b.close()


def test_state_keys_and_resume():
    L, M = SHAPES[0]
    floor = db(table_from(curves(L, M, "f64")[3], "scalar"))
    plain = device(L, M, None, "f64")
    a, b = (device(L, M, floor, "f64") for _ in range(2))
    for h in range(2):
        hop(plain, X, h, H)
        hop(a, X, h, H)
    st = a.get_state()
    assert sorted(st) == sorted(plain.get_state())
    b.set_state(st)
    assert b.validation_bright_A is None                                                    # b has run no hop of its own
    for h in range(2, HOPS):
        same_outputs(hop(a, X, h, H), hop(b, X, h, H))
    for z in "AB":
        for name in ("w_", "validation_bright_", "validation_dark_", "validation_source_", "validation_rank_"):
            assert np.array_equal(getattr(a, name + z), getattr(b, name + z)), name + z
    for ap in (plain, a, b):
        ap.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_neutral_floor_is_the_stream_with_the_responses_alone(dtype):
    L, M = SHAPES[1]
    plain, free = device(L, M, None, dtype), device(L, M, -np.inf, dtype)
    for h in range(HOPS):
        same_outputs(hop(plain, X, h, H), hop(free, X, h, H))
    G = [transfer(r, N) for r in validation_rirs(PV, L, MV)]
    for i, z in enumerate("AB"):
        w = getattr(free, "w_" + z)
        assert np.array_equal(getattr(plain, "w_" + z), w) and np.array_equal(getattr(plain, "lambda_" + z), getattr(free, "lambda_" + z))
        assert (getattr(free, "validation_source_" + z) == np.arange(L)).all() and (getattr(free, "validation_rank_" + z) == L).all()
        # the energies are those of the filters the stream holds
        wk = w.transpose(1, 0, 2).astype(np.complex128)
        for q, g in (("bright", G[i]), ("dark", G[1 - i])):
            p = np.einsum("kml,ktl->ktm", g, wk)
            e = (p.real ** 2 + p.imag ** 2).sum(-1)
            s = (np.einsum("kml,ktl->ktm", np.abs(g), np.abs(wk)) ** 2).sum(-1)
            assert (np.abs(getattr(free, f"validation_{q}_{z}") - e) <= 4 * (L + MV + 4) * 2.0 ** -53 * s).all()
        assert all(getattr(plain, f"validation_{q}_{z}") is None for q in ("bright", "dark", "source", "rank"))
    assert plain.validation_floor_db is None and np.isneginf(free.validation_floor_db).all()
    with pytest.raises(ValueError, match="validation_floor_db was not given"):
        plain.validation_floor_db = 3.0
    plain.close()
    free.close()


# 4 ---------------------------------------------------------------------------------------------------------------
def _null_rows(A, n):
    """n orthonormal rows orthogonal to every column of A (L, c), c + n <= L"""
    q, _ = np.linalg.qr(np.concatenate([A, np.eye(A.shape[0])], axis=1))
    return q[:, A.shape[1]:A.shape[1] + n].conj().T


@pytest.mark.parametrize("zero", ["dark", "bright"])
def test_known_answer(zero):
    """Pv = 1: the transfer functions are the validation matrices themselves, real and constant over frequency.  One zone's matrix
    is built from the oracle's filters: every row orthogonal to the real and to the imaginary part of program A's filter of rank 1
    in bin K0 of the last hop (L = 4 loudspeakers leave two such directions).  The device's filter is the oracle's within
    t = 1e-7, so that slot's energy on this bank is at most t^2 ||G||_F^2 |w|^2: zero next to every other energy.
    "dark": the matrix is zone B's, program A's dark bank.  Slot 0 of the bin holds a floor of 100 dB, which no other slot
    does, so every slot of the bin takes slot 0.
    "bright": the matrix is zone A's, program A's bright bank.  No slot holds the floor, slot 0 has the smallest contrast by far,
    and every later slot takes the first slot of largest contrast among 1 .. t."""
    L, M = SHAPES[0]
    K0 = 5
    orc = oracle(L, M, np.zeros((2, K)))
    for h in range(HOPS):
        hop(orc, X, h, H)
    w0 = orc.w_unchosen[0][K0, 0]
    B = _null_rows(np.stack([w0.real, w0.imag], axis=1), 2).real                            # (2, L)
    assert np.abs(B @ w0).max() <= 1e-14 * np.linalg.norm(w0)
    rng = np.random.default_rng(4)
    other = rng.standard_normal((1, L, MV))
    mine = np.zeros((1, L, MV))
    mine[0] = B.T @ np.concatenate([np.eye(2), rng.standard_normal((2, MV - 2))], axis=1)   # every microphone in those directions
    rvA, rvB = (other, mine) if zero == "dark" else (mine, other)
    from ap_vast_unofficial_amd.apvast import apvast
    rirA, rirB = synth_rirs(P, L, M, 1)
    ap = apvast(N, rirA, rirB, 16, DELAY, REF_A, REF_B, L, MU, 4 * N, hop_size=H, perceptual=False, seed=0, dtype="f64",
                validation_rir_A=rvA, validation_rir_B=rvB, validation_floor_db=100.0)
    for h in range(HOPS):
        hop(ap, X, h, H)
    b, d, src = ap.validation_bright_A[K0], ap.validation_dark_A[K0], ap.validation_source_A[K0]
    zeroed, full = (d, b) if zero == "dark" else (b, d)
    assert zeroed[0] <= (2e-7) ** 2 * (np.abs(mine) ** 2).sum() * (np.abs(w0) ** 2).sum()
    assert full[0] >= 1e10 * zeroed[0] and (b[1:] < 1e10 * d[1:]).all() and (d[1:] < 1e10 * b[1:]).all()
    assert np.array_equal(ap.validation_source_A, decide(ap.validation_bright_A, ap.validation_dark_A, 1e10)[0])
    if zero == "dark":
        assert np.array_equal(src, np.zeros(L, dtype=np.int32)) and ap.validation_rank_A[K0] == 1
        assert all(np.array_equal(ap.w_A[v][K0], ap.w_A[0][K0]) for v in range(L))
    else:
        best = [0] + [1 + int(np.argmax(b[1:t + 1] / d[1:t + 1])) for t in range(1, L)]
        assert np.array_equal(src, best) and ap.validation_rank_A[K0] == best[-1] + 1
    ap.close()


def test_errors():
    from ap_vast_unofficial_amd._capi import ApvError
    L, M = SHAPES[0]
    # a first call once the stream is initialised: refused, and the stream carries on unchanged
    plain, ref = device(L, M, None, "f64"), device(L, M, None, "f64")
    same_outputs(hop(plain, X, 0, H), hop(ref, X, 0, H))
    G = np.ones((K, MV, L), dtype=np.complex128)
    with pytest.raises(ApvError):
        plain._eng.set_validation_span(np.ones(K), G, G)
    with pytest.raises(ApvError):
        plain._eng.validation_span(0, 0)
    same_outputs(hop(plain, X, 1, H), hop(ref, X, 1, H))
    plain.close()
    ref.close()
    # without the evaluation stage the first call has nothing to size the banks by
    bare = device(L, M, None, "f64", validate=False)
    with pytest.raises(ApvError):
        bare._eng.set_validation_span(np.ones(K), G, G)
    bare.close()
    on = device(L, M, 0.0, "f64")
    for bad in (-np.ones(K), np.full(K, np.nan), np.full(K, np.inf)):
        with pytest.raises(ApvError):
            on._eng.set_validation_span(bad)
    with pytest.raises(ApvError):
        on._eng.set_validation_span(np.ones(K), G, None)                                     # one bank without the other
    with pytest.raises(ApvError):
        on._eng.validation_span(2, 0)
    with pytest.raises(ApvError):
        on._eng.validation_span(0, 4)
    with pytest.raises(ValueError):
        on._eng.set_validation_span(np.ones(K + 1))
    on._eng.set_validation_span(np.zeros((2, K)))                                            # 0 is a value like any other
    on.close()

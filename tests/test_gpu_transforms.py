"""The LDS transforms (csrc/stft_fft.h, csrc/kernels_stft.hip) on their own, in both precisions, against the long-double reference
of tests/transform_oracle.py: every plan family (in-place radix 4/2 with one and with several butterflies per thread, mixed radix
with 3, 5 and 7, Bluestein at its fill edges), the kernel forms the streams launch (the job kernel with its workgroup remap, three
spectrum layouts and chunk form; the MI = 1 instantiations) and every kernel argument (zero padding, no window, ring offset, row
stride, synthesis hops, strides, emit forms).

Every comparison is per channel and normwise, ||got_c - ref_c||_2 <= c(N) u ||ref_c||_2 (transform_oracle.py derives it), on 19
channels whose amplitudes span six decades.  Each check prints the share of the bound it used; the largest per (precision, family)
are printed when the module ends (pytest -s) and kept in profiles/r13/transform_error_shares.md."""
import ctypes as C

import numpy as np
import pytest

import transform_oracle as to

pytestmark = pytest.mark.gpu

WORST = {}          # (what, dtype, family) -> (share, N, note)
JOB_SETS = (1, 2, 16, 3, 5, 1, 32, 7)          # 67 channels: no multiple of 8, so the XCD remap has a remainder
JOB_LAYOUTS = ("bin", "grouped", "channel", "grouped", "bin", "grouped", "grouped", "channel")


def case_id(v):
    return "-".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


class engine:
    def __init__(self, N, H=None):
        self.N, self.H = N, N // 2 if H is None else H

    def __enter__(self):
        from ap_vast_unofficial_amd import Engine
        self.eng = Engine(1, 4, 4, block_size=self.N, hop_size=self.H)
        return self.eng

    def __exit__(self, *exc):
        self.eng.close()


@pytest.fixture(scope="module", autouse=True)
def share_table():
    yield
    print("\nlargest share of the bound c(N) u ||ref_c|| per (case, precision, family):")
    for (what, dtype, family), (s, N, note) in sorted(WORST.items()):
        print(f"SHARE | {what:<22} | {dtype} | {family:<9} | {s:9.4f} | N = {N} {note}")


def check(got, ref, N, dtype, what, scale=None, note="", factor=1.0):
    """every channel within factor * the bound; prints and records the largest share"""
    s = to.shares(got, ref, N, dtype, scale)
    worst, c = float(s.max()) if s.size else 0.0, int(s.argmax()) if s.size else -1
    key = (what, dtype, to.plan_of(N)["family"])
    if worst >= WORST.get(key, (-1.0,))[0]:
        WORST[key] = (worst, N, note)
    print(f"share {what} N={N} {dtype} {note}: {worst:.4f} (channel {c})")
    assert worst <= factor, (what, N, dtype, note, "channel", c, "shares", np.round(s, 4).tolist())
    return worst


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def many_channels(N, dtype, n, length=None):
    """n channels from as many input sets (seeds 0, 1, ...) as it takes"""
    sets = [to.inputs(N, dtype, length, seed) for seed in range(-(-n // to.N_CH))]
    return np.concatenate(sets)[:n]


def split(x, counts):
    at = np.cumsum((0,) + tuple(counts))
    return [x[a:b] for a, b in zip(at[:-1], at[1:])]


# ---- analysis -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,dtype", to.cases(), ids=case_id)
def test_analysis_every_size(N, dtype):
    """Windowed, full length, ring offset 0: the stand-alone kernel (always instantiated for four butterflies per thread) and the
    job kernel with one set (instantiated for one where the plan needs no more) against the reference, and bit for bit against
    each other: they run the same arithmetic."""
    x, ref = to.analysis_case(N, dtype)
    with engine(N) as eng:
        alone = eng.analysis(x, dtype)
        (jobs,), stray = eng.analysis_jobs([x], dtype)
    check(alone, ref, N, dtype, "analysis")
    check(jobs, ref, N, dtype, "analysis jobs")
    assert same_bits(alone, jobs) and stray == [0]


@pytest.mark.parametrize("in_len", ["0", "1", "2", "3", "N/2-1", "N/2", "N-1"])
@pytest.mark.parametrize("N,dtype", to.cases(to.ANALYSIS_ARG_SIZES), ids=case_id)
def test_analysis_zero_padding(N, dtype, in_len):
    """in_len < N, odd lengths included, without and with the window, rows packed (x_stride = in_len: what follows sample
    in_len - 1 is the next channel) and spread (x_stride = N + 3: what follows is NaN)"""
    n_in = {"0": 0, "1": 1, "2": 2, "3": 3, "N/2-1": N // 2 - 1, "N/2": N // 2, "N-1": N - 1}[in_len]
    x = to.inputs(N, dtype, n_in)
    with engine(N) as eng:
        for use_win in (False, True):
            ref = to.analysis(x, N, use_window=use_win)
            for stride in (n_in, N + 3):
                got = eng.analysis(x, dtype, window=use_win, x_stride=stride)
                check(got, ref, N, dtype, "analysis in_len<N", note=f"in_len={n_in} window={int(use_win)} x_stride={stride}")


@pytest.mark.parametrize("N,dtype", to.cases(to.ANALYSIS_ARG_SIZES), ids=case_id)
def test_analysis_ring_offset(N, dtype):
    """logical sample n at (n + ring_off) mod N of the row, odd, negative and beyond-N offsets, rows N and N + 3 apart; the job
    kernel with the same offset bit for bit"""
    x = to.inputs(N, dtype)
    with engine(N) as eng:
        for i, off in enumerate((1, N // 2, N - 1, N + 5, -3)):
            ref = to.analysis(x, N, ring_off=off)
            got = eng.analysis(x, dtype, ring_off=off, x_stride=N + 3 * (i % 2))
            check(got, ref, N, dtype, "analysis ring", note=f"ring_off={off}")
            (jobs,), stray = eng.analysis_jobs([x], dtype, ring_off=off)
            assert same_bits(got, jobs) and stray == [0], off


@pytest.mark.parametrize("N,dtype", to.cases(to.ANALYSIS_ARG_SIZES), ids=case_id)
def test_analysis_channel_counts(N, dtype):
    """1, 7, 8, 9 and 19 channels (around the eight-way remap of the job kernel), channel-major and bin-major spectra"""
    x, ref = to.analysis_case(N, dtype)
    with engine(N) as eng:
        for n in (1, 7, 8, 9, 19):
            cm = eng.analysis(x[-n:], dtype)
            bm = eng.analysis(x[-n:], dtype, layout="bin")
            (jobs,), stray = eng.analysis_jobs([x[-n:]], dtype, layouts=["bin"])
            check(cm, ref[-n:], N, dtype, "analysis n_ch", note=f"n_ch={n}")
            assert same_bits(cm, bm) and same_bits(cm, jobs) and stray == [0], n


# ---- the job kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [JOB_SETS, (1, 2, 3), (8,), (3, 0, 6)], ids=case_id)
@pytest.mark.parametrize("N,dtype", to.cases(to.JOBS_SIZES), ids=case_id)
def test_jobs_sets_and_layouts(N, dtype, counts):
    """several channel sets in one launch, each in one of the three spectrum layouts (the grouped one with g = 4 and a partial last
    group), one shared odd ring offset; launches of 67 workgroups, of fewer than eight, of exactly eight and with an empty set.
    Every set against the reference; nothing outside the mapped elements written."""
    x = many_channels(N, dtype, sum(counts))
    ref = to.analysis(x, N, ring_off=7)
    with engine(N) as eng:
        spectra, stray = eng.analysis_jobs(split(x, counts), dtype, ring_off=7, layouts=JOB_LAYOUTS[:len(counts)])
    assert stray == [0] * len(counts), stray
    for j, (got, r) in enumerate(zip(spectra, split(ref, counts))):
        if got.size:
            check(got, r, N, dtype, "jobs", note=f"sets={counts} set {j} ({JOB_LAYOUTS[j]})")


@pytest.mark.parametrize("n_hops", [1, 3])
@pytest.mark.parametrize("N,dtype", to.cases(to.JOBS_SIZES), ids=case_id)
def test_jobs_chunk_form(N, dtype, n_hops):
    """the hop in blockIdx.y: rows longer than N (and x_stride longer than the rows), hop i reads H samples further on and
    writes its spectra spec_hop further on, with a gap between the hops that must stay untouched"""
    H = N // 2
    W = N + (n_hops - 1) * H + 3
    x = many_channels(N, dtype, sum(JOB_SETS), W)
    with engine(N, H) as eng:
        spectra, stray = eng.analysis_jobs(split(x, JOB_SETS), dtype, layouts=JOB_LAYOUTS, n_hops=n_hops, x_stride=W + 2)
    assert stray == [0] * len(JOB_SETS), stray
    for i in range(n_hops):
        ref = to.analysis(x[:, i * H:i * H + N], N)
        for j, r in enumerate(split(ref, JOB_SETS)):
            assert spectra[j].shape == (n_hops,) + r.shape
            check(spectra[j][i], r, N, dtype, "jobs chunk", note=f"n_hops={n_hops} hop {i} set {j} ({JOB_LAYOUTS[j]})")


# ---- synthesis --------------------------------------------------------------------------------------------------------
def check_synthesis(eng, N, H, dtype, what, note="", n_ch=to.N_CH, **kw):
    S, ov, ref, scale = to.synthesis_case(N, dtype, H)
    ov_new, out, details = eng.synthesize(S[:n_ch], ov[:n_ch], dtype, **kw)
    check(ov_new, ref[:n_ch], N, dtype, what, scale=scale[:n_ch], note=note)
    if kw.get("emit", True):
        assert same_bits(out, np.ascontiguousarray(ov_new[:, :H])), (what, note)
        assert details["stray"] == 0, (what, note, details)
    else:
        assert out is None
    return ov_new, details


@pytest.mark.parametrize("N,dtype", to.cases(), ids=case_id)
def test_synthesis_every_size(N, dtype):
    """spectra = reference spectra * (1 + 0.1j) (the imaginary parts this leaves at DC and Nyquist must be ignored), random overlap,
    H = N/2"""
    with engine(N) as eng:
        check_synthesis(eng, N, N // 2, dtype, "synthesis")


@pytest.mark.parametrize("hop", ["1", "3", "N/4", "N/2+1", "N-1", "N"])
@pytest.mark.parametrize("N,dtype", to.cases(to.SYNTHESIS_ARG_SIZES), ids=case_id)
def test_synthesis_hops(N, dtype, hop):
    """hops other than N/2 and N/4: the shifted overlap (n < N - H) ? ov[n + H] : 0 from nearly all of the block to none of it"""
    H = {"1": 1, "3": 3, "N/4": N // 4, "N/2+1": N // 2 + 1, "N-1": N - 1, "N": N}[hop]
    with engine(N, H) as eng:
        check_synthesis(eng, N, H, dtype, "synthesis hops", note=f"H={H}")


@pytest.mark.parametrize("N,dtype", to.cases(to.SYNTHESIS_ARG_SIZES), ids=case_id)
def test_synthesis_layouts_and_emit(N, dtype):
    """bin-major spectra, the sample-major emit in groups of 1, 4 and 19 channels, groups further apart than they are long, a group
    that does not divide the channel count (the emit is then channel-major), and no emit at all: the same overlap bit for bit"""
    H = N // 2
    with engine(N, H) as eng:
        plain, _ = check_synthesis(eng, N, H, dtype, "synthesis args", note="channel-major")
        runs = [("bin-major", 19, dict(layout="bin"), "channel"),
                ("out_group=1", 19, dict(out_group=1), "grouped"),
                ("out_group=19", 19, dict(out_group=19), "grouped"),
                ("out_group=4 of 19 channels", 19, dict(out_group=4), "channel"),
                ("out_group=4 of 16 channels", 16, dict(out_group=4), "grouped"),
                ("out_group=4, out_gstride=4H+5", 16, dict(out_group=4, out_gstride=4 * H + 5, layout="bin"), "grouped"),
                ("out_group=1, out_gstride=H+3", 19, dict(out_group=1, out_gstride=H + 3), "grouped"),
                ("no emit", 19, dict(emit=False), "channel")]
        for note, n_ch, kw, emit in runs:
            ov_new, details = check_synthesis(eng, N, H, dtype, "synthesis args", note=note, n_ch=n_ch, **kw)
            assert details["emit"] == emit, (note, details)
            assert same_bits(ov_new, plain[:n_ch]), note


# ---- linearity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_analysis_is_linear(dtype):
    """analysis(a x + b y) against a X + b Y of two other launches at twice the bound (each side carries one transform's error);
    a, b > 0, so that a X + b Y of the impulse and sinusoid channels, which x and y share, does not cancel"""
    N, a, b = 1020, 0.75, 1.5
    x, y = to.inputs(N, dtype, seed=0), to.inputs(N, dtype, seed=1)
    z = (to.LD(a) * x.astype(to.LD) + to.LD(b) * y.astype(to.LD)).astype(to.REAL[dtype])
    with engine(N) as eng:
        X, Y, Z = (eng.analysis(v, dtype) for v in (x, y, z))
    check(Z, to.CLD(a) * X.astype(to.CLD) + to.CLD(b) * Y.astype(to.CLD), N, dtype, "linearity", factor=2.0)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_through_the_new_entries():
    """sizes without a plan are refused in the rule's words, double precision above 4096 in the streams' words"""
    for N, dtype, words in [(n, d, to.RULE) for n in to.REFUSED for d in ("f32", "f64")] + [(6000, "f64", to.F64_RULE)]:
        rdt, cdt = to.REAL[dtype], to.CPLX[dtype]
        with engine(N) as eng:
            with pytest.raises(RuntimeError, match=words):
                eng.analysis(np.zeros((1, N), rdt), dtype)
            with pytest.raises(RuntimeError, match=words):
                eng.analysis_jobs([np.zeros((1, N), rdt)], dtype)
            with pytest.raises(RuntimeError, match=words):
                eng.synthesize(np.zeros((1, N // 2 + 1), cdt), np.zeros((1, N), rdt), dtype)


def test_entries_refuse_what_the_kernels_take_on_trust():
    """the C entries themselves (not the checks Engine makes first): APV_ERR_ARG and a message, nothing launched"""
    from ap_vast_unofficial_amd import _capi
    N = 32
    with engine(N) as eng:
        x, s, ov = eng.to_device(np.zeros((3, N + 3))), eng.to_device(np.zeros((3, N), np.complex128)), eng.to_device(np.zeros((3, N)))
        lib, h = eng.lib, eng.h

        def refused(rc, words):
            assert rc == _capi.ERR_ARG and words in lib.apv_last_error(h).decode(), (rc, lib.apv_last_error(h))

        K = N // 2 + 1
        refused(lib.apv_analysis_dev(h, 1, 2, x.ptr, N, -1, 0, 1, s.ptr, K, 1), "in_len")
        refused(lib.apv_analysis_dev(h, 1, 2, x.ptr, N + 1, N + 1, 0, 1, s.ptr, K, 1), "in_len")
        refused(lib.apv_analysis_dev(h, 1, 2, x.ptr, 7, 8, 0, 1, s.ptr, K, 1), "x_stride")
        refused(lib.apv_analysis_dev(h, 1, 2, x.ptr, N, N - 1, 1, 1, s.ptr, K, 1), "ring offset")
        refused(lib.apv_analysis_dev(h, 1, 2, x.ptr, N - 1, N - 1, -3, 1, s.ptr, K, 1), "ring offset")
        refused(lib.apv_analysis_dev(h, 1, 2, None, N, N, 0, 1, s.ptr, K, 1), "null")
        vp1, i32_1, i64_1 = C.c_void_p * 1, C.c_int32 * 1, C.c_int64 * 1
        vp9, i32_9, i64_9 = C.c_void_p * 9, C.c_int32 * 9, C.c_int64 * 9
        one = (vp1(x.ptr.value), i32_1(1), vp1(s.ptr.value), i64_1(K), i64_1(1))
        nine = (vp9(*[x.ptr.value] * 9), i32_9(*[0] * 9), vp9(*[s.ptr.value] * 9), i64_9(*[K] * 9), i64_9(*[1] * 9))
        refused(lib.apv_analysis_jobs_dev(h, 1, 0, *one, 0, 0, 0, 0, None), "n_jobs")
        refused(lib.apv_analysis_jobs_dev(h, 1, 9, *nine, 0, 0, 0, 0, None), "n_jobs")
        refused(lib.apv_analysis_jobs_dev(h, 1, 1, *one, 0, 65536, 1 << 40, 1, i64_1(K)), "n_hops")
        refused(lib.apv_analysis_jobs_dev(h, 1, 1, *one, 0, -1, N, 0, None), "n_hops")
        refused(lib.apv_analysis_jobs_dev(h, 1, 1, *one, 1, 1, N, 0, None), "ring_off")
        refused(lib.apv_analysis_jobs_dev(h, 1, 1, *one, 0, 2, N + 15, 16, i64_1(K)), "x_stride")
        refused(lib.apv_analysis_jobs_dev(h, 1, 1, *one, 0, 2, N + 16, 16, None), "spec_hop")
        refused(lib.apv_synthesis_dev(h, 1, 2, s.ptr, K, 1, None, None, 0, 0), "null")
        refused(lib.apv_synthesis_dev(h, 1, 2, s.ptr, K, 1, ov.ptr, None, -1, 0), "out_group")
        refused(lib.apv_synthesis_dev(h, 1, 2, s.ptr, K, 1, ov.ptr, None, 2, N - 1), "out_gstride")
        for b in (x, s, ov):
            b.free()
    with engine(0, 0) as eng:                                  # a handle without an STFT geometry
        x = eng.to_device(np.zeros(8))
        assert eng.lib.apv_analysis_dev(eng.h, 1, 1, x.ptr, 4, 4, 0, 1, x.ptr, 3, 1) == _capi.ERR_ARG
        assert "without an STFT geometry" in eng.lib.apv_last_error(eng.h).decode()
        x.free()

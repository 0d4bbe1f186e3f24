"""tests/transform_oracle.py on its own, without a GPU: the long-double reference against a direct DFT, the restated plan rule,
the coverage conditions of the size list of tests/test_gpu_transforms.py, the constants of the bound, and the argument rules and
ABI declarations of the stand-alone transform entries."""
import os
import re

import numpy as np
import pytest

import transform_oracle as to
from eval_spectra_oracle import bluestein_length, coeff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_double_is_wider_than_double_and_fft_keeps_it():
    assert to.EPS_LD <= 2.0 ** -63 and to.CLD == np.dtype("complex256")
    x = np.ones((2, 12), dtype=to.LD)
    assert np.fft.rfft(x).dtype == to.CLD and np.fft.irfft(np.fft.rfft(x), n=12).dtype == to.LD
    assert abs(float(to.PI - to.LD(np.pi))) < 2e-16 and float(to.PI) == np.pi


@pytest.mark.parametrize("N", [6, 22, 210, 1020, 1600])
def test_rfft_agrees_with_the_direct_dft(N):
    x = to.inputs(N, "f64").astype(to.LD)
    X, D = to.rfft(x), to.dft(x)
    assert X.dtype == to.CLD and D.dtype == to.CLD
    err = np.abs(X - D).max(axis=1)
    assert np.all(err <= 64 * to.EPS_LD * to.norms(x)), (err / to.norms(x)).max() / to.EPS_LD
    # and the inverse, with imaginary parts at DC and Nyquist that it must drop
    S = X * (1 + 0.1j)
    S0 = S.copy()
    S0[:, 0], S0[:, -1] = S[:, 0].real, S[:, -1].real
    back = to.irfft(S, N)
    assert np.all(np.abs(to.rfft(back) - S0).max(axis=1) <= 64 * to.EPS_LD * to.norms(x) * 1.1)


def test_reference_forms():
    N, rng = 12, np.random.default_rng(0)
    x = rng.standard_normal((3, N))
    w = np.sin(np.pi * np.arange(N) / N)
    assert np.abs(to.analysis(x, N) - np.fft.rfft(w * x)).max() < 1e-14
    assert np.abs(to.analysis(x, N, use_window=False) - np.fft.rfft(x)).max() < 1e-14
    assert np.abs(to.analysis(x[:, :5], N, use_window=False) - np.fft.rfft(x[:, :5], n=N)).max() < 1e-14
    assert np.abs(to.analysis(x, N, in_len=5) - np.fft.rfft(w[:5] * x[:, :5], n=N)).max() < 1e-14
    assert np.all(to.analysis(x[:, :0], N) == 0)
    for off in (1, N - 1, N + 5, -3):
        assert np.abs(to.analysis(x, N, ring_off=off) - np.fft.rfft(w * np.roll(x, -off, axis=1))).max() < 1e-14
    S, ov = np.fft.rfft(x) * (1 + 0.1j), rng.standard_normal((3, N))
    for H in (1, 3, 6, 7, 11, 12):
        new = w * np.fft.irfft(S, n=N)
        exp = np.concatenate([ov[:, H:], np.zeros((3, H))], axis=1) + new
        got, scale = to.synthesis(S, ov, N, H)
        assert np.abs(got - exp).max() < 1e-14
        assert np.allclose(scale.astype(float), np.linalg.norm(new, axis=1) + np.linalg.norm(ov, axis=1))


def test_plan_rule():
    for N in range(4, 8194, 2):
        p, M = to.plan_of(N), bluestein_length(N)
        if p is None:
            assert N > 4096 and M, N
            continue
        assert p["M"] == M and (p["family"] == "bluestein") == bool(M), N
        prod = int(np.prod(p["radix"]))
        assert prod == (M if M else N // 2), N
        assert p["lds"]["f32"] <= 65536 and (N > 4096 or p["lds"]["f64"] <= 65536), N
        if p["family"] != "mixed":
            assert set(p["radix"]) <= {2, 4} and 1 <= p["max_it"] <= 4, N
    for N in (2, 3, 5, 1021, 8194) + to.REFUSED:
        assert to.plan_of(N) is None


def test_size_list_meets_its_coverage_conditions():
    fam = lambda N: to.plan_of(N)["family"]
    small = [fam(N) for N in to.EVEN_TO_128]
    assert to.EVEN_TO_128 == tuple(range(4, 129, 2))
    assert (small.count("inplace"), small.count("mixed"), small.count("bluestein")) == (6, 29, 28)
    for N, r in ((4, 2), (6, 3), (8, 4), (10, 5), (14, 7)):
        assert to.plan_of(N)["radix"] == [r]
    assert min(N for N in to.EVEN_TO_128 if fam(N) == "bluestein") == 22 and to.plan_of(22)["M"] == 32
    # the one-butterfly boundary of the in-place form
    for N in (1024, 2048):
        assert fam(N) == "inplace" and to.plan_of(N)["max_it"] == 1
    p = to.plan_of(4096)
    assert p["family"] == "inplace" and p["radix"] == [4] * 5 + [2] and p["max_it"] == 4
    assert (2048 // 4) // 256 == 2 and (2048 // 2) // 256 == 4
    assert fam(8192) == "inplace" and to.plan_of(8192)["max_it"] == 4 and to.plan_of(8192)["lds"]["f32"] == 32768
    # Bluestein fill edges
    for N in (1018, 1020, 1022):
        assert (to.plan_of(N)["M"], to.plan_of(N)["max_it"]) == (1024, 1)
    for N in (1026, 1030, 2046):
        assert (to.plan_of(N)["M"], to.plan_of(N)["max_it"]) == (2048, 4)
    for N in (2050, 4094):
        assert to.plan_of(N)["M"] == 4096 and to.plan_of(N)["lds"]["f64"] == 65536
    assert set(to.BLUESTEIN_EDGE) == {1018, 1020, 1022, 1026, 1030, 2046, 2050, 4094}
    # odd radices alone and mixed
    for N, r in ((1458, 3), (1250, 5), (686, 7)):
        assert to.plan_of(N)["radix"] == [r] * len(to.plan_of(N)["radix"]) and len(to.plan_of(N)["radix"]) >= 3
    assert sorted(set(to.plan_of(210)["radix"])) == [3, 5, 7] and sorted(set(to.plan_of(1600)["radix"])) == [2, 4, 5]
    assert fam(4050) == "mixed" and to.plan_of(4050)["lds"]["f64"] == 64800
    assert max(to.plan_of(N)["lds"]["f64"] for N in range(4, 4098, 2) if fam(N) == "mixed") == 64800
    assert set(to.ODD_RADIX) == {1458, 1250, 686, 210, 1600, 4050}
    # 7-smooth above 4096
    assert set(to.ABOVE_4096) == {4374, 4802, 6000, 6144, 7000, 8064, 8100}
    for N in to.ABOVE_4096:
        assert N > 4096 and fam(N) == "mixed" and to.plan_of(N)["lds"]["f32"] <= 65536
    # both precisions everywhere, float32 alone above 4096
    cs = to.cases()
    assert len(set(cs)) == len(cs) == 2 * len(to.ALL_SIZES) - len(to.ABOVE_4096) - 1
    assert all((N, "f32") in cs and ((N, "f64") in cs) == (N <= 4096) for N in to.ALL_SIZES)
    for sizes in (to.ANALYSIS_ARG_SIZES, to.JOBS_SIZES, to.SYNTHESIS_ARG_SIZES):
        assert {fam(N) for N in sizes} == {"inplace", "mixed", "bluestein"}
    # K = N/2 + 1 is no multiple of 4 (odd, but for 250 where it is 126): the last group of 4 bins is partial
    assert all((N // 2 + 1) % 4 != 0 for N in to.JOBS_SIZES)


def test_bound_constants():
    assert to.U == {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
    assert coeff(1024) == 8 * 12 and coeff(8192) == 8 * 15 and coeff(6) == 8 * (np.log2(6) + 2)
    assert coeff(1020) == 3 * 8 * 12 and coeff(22) == 3 * 8 * 7 and coeff(4094) == 3 * 8 * 14
    assert np.allclose(to.AMPLITUDES, np.logspace(-3, 3, 19)) and to.N_CH == 19
    assert (to.KINDS.count("noise"), sum(k.startswith("imp") for k in to.KINDS), sum(k.startswith("sin") for k in to.KINDS)) == (13, 3, 3)
    got = np.array([[1.0, 2.0], [0.0, 0.0], [0.0, 0.0]])
    ref = np.array([[1.0, 2.0 + 4 * coeff(8) * 2.0 ** -53], [0.0, 0.0], [0.0, 1e-300]])
    s = to.shares(got, ref, 8, "f64")
    assert 0.3 < s[0] < 3 and s[1] == 0 and s[2] > 1


def test_inputs():
    for N, length in ((32, 32), (70, 34), (32, 1), (32, 0)):
        x = to.inputs(N, "f32", length)
        assert x.shape == (19, length) and x.dtype == np.float32 and not x.flags.writeable
        if length:
            assert np.allclose(np.abs(x).max(axis=1) / to.AMPLITUDES, 1, atol=4) and np.all(np.abs(x).max(axis=1) > 0)
    x = to.inputs(64, "f64")
    X = np.abs(np.fft.rfft(x))
    assert X[to.KINDS.index("sin1")].argmax() == 1 and X[to.KINDS.index("sinny")].argmax() == 31
    assert x[to.KINDS.index("imp1"), 1] != 0 and x[to.KINDS.index("implast"), 63] != 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_numpy_own_transforms_use_a_small_share_of_the_bound(dtype):
    """what the docstring of the oracle says of NumPy's transforms in the device's precision, measured again"""
    worst = 0.0
    for N in (4, 6, 22, 64, 210, 1020, 1600, 4094, 8192):
        x, ref = to.analysis_case(N, dtype)
        w = to.window(N).astype(to.REAL[dtype])
        got = np.fft.rfft(w * x).astype(to.CPLX[dtype])
        assert got.dtype == to.CPLX[dtype]
        worst = max(worst, to.shares(got, ref, N, dtype).max())
        for H in (N // 2, N):
            S, ov, ov_ref, scale = to.synthesis_case(N, dtype, H)
            assert S.dtype == to.CPLX[dtype] and ov.dtype == to.REAL[dtype] and S[:, 0].imag.any() and S[:, -1].imag.any()
            new = (w * np.fft.irfft(S, n=N)).astype(to.REAL[dtype])
            got = np.concatenate([ov[:, H:], np.zeros((to.N_CH, H), to.REAL[dtype])], axis=1) + new
            assert got.dtype == to.REAL[dtype]
            worst = max(worst, to.shares(got, ov_ref, N, dtype, scale).max())
    assert worst < 0.25, worst


def test_argument_rules_of_the_new_entries():
    from ap_vast_unofficial_amd import _capi
    ok = _capi.check_analysis_args
    for a in ((32, 0, 0, 0), (32, 32, 32, 5), (32, 32, 35, -3), (32, 7, 7, 0), (32, 7, 35, 32), (32, 32, 32, 37)):
        ok(*a)
    for a in ((32, -1, 32, 0), (32, 33, 40, 0), (32, 8, 7, 0), (32, 16, 32, 1), (32, 31, 32, -3)):
        with pytest.raises(ValueError):
            ok(*a)
    _capi.check_jobs_args(64, 8, 0, 5, 64, 0)
    _capi.check_jobs_args(64, 1, 3, 0, 64 + 2 * 32, 32)
    for a in ((64, 0, 0, 0, 64, 0), (64, 9, 0, 0, 64, 0), (64, 1, 65536, 0, 10 ** 7, 32), (64, 1, -1, 0, 64, 0), (64, 1, 2, 1, 96, 32),
              (64, 1, 3, 0, 64 + 2 * 32 - 1, 32)):
        with pytest.raises(ValueError):
            _capi.check_jobs_args(*a)
    assert _capi.transform_dtypes("f32") == (0, np.float32, np.complex64) and _capi.transform_dtypes("f64")[0] == 1
    with pytest.raises(ValueError):
        _capi.transform_dtypes("f16")
    with pytest.raises(ValueError):
        _capi.spectrum_layout("diagonal", 3, 5)
    # every layout is a bijection of (channel, bin) into its buffer; the grouped one leaves the tail of the last group free
    for layout in _capi.SPECTRUM_LAYOUTS:
        for n_ch, K in ((1, 33), (3, 33), (7, 126), (32, 511)):
            sc, sk, size, index = _capi.spectrum_layout(layout, n_ch, K, 4)
            assert index.shape == (n_ch, K) and len(set(index.ravel())) == n_ch * K and 0 <= index.min() and index.max() < size
            assert size == (n_ch * K if layout != "grouped" else -(-K // 4) * 4 * n_ch)
            c, k = n_ch - 1, K - 1
            grouped = sc > 1 and sk > 1                       # the kernel's own test (stft_analysis_jobs_kernel)
            at = c * sc + ((k // sc) * sc * sk + k % sc if grouped else k * sk)
            assert index[c, k] == at, (layout, n_ch, K)


def test_abi_declarations():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    n_args = {"apv_analysis_dev": 11, "apv_analysis_jobs_dev": 13, "apv_synthesis_dev": 10}
    lib = _capi.load()
    for name, n in n_args.items():
        assert name in _capi.EXPORTS
        decl = re.search(r"int\s+" + name + r"\s*\((.*?)\);", text, flags=re.S).group(1)
        assert len(decl.split(",")) == n, name
        assert len(getattr(lib, name).argtypes) == n, name
    assert _capi.STFT_MAX_JOBS == 8
    src = open(os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc", "apv_internal.h")).read()
    assert re.search(r"APV_STFT_MAX_JOBS = 8;", src)

"""Long-double reference of the LDS transforms (csrc/stft_fft.h, csrc/kernels_stft.hip) for tests/test_gpu_transforms.py, NumPy only.

analysis :  X_c = rfft(w * y_c),  y_c[n] = row_c[(n + ring_off) mod N] for n < in_len, 0 for in_len <= n < N
synthesis:  new_c = w * irfft(S_c) (imaginary parts of DC and Nyquist ignored),  overlap_c <- shift(overlap_c, H) + new_c,
            out_c = overlap_c[0:H],  any 1 <= H <= N
with w[n] = sin(pi n / N) (window=True) or 1.  Everything is formed in numpy.longdouble (x87 extended here: eps = 1.08e-19, 2^11
below float64's), numpy.fft keeping that type (NumPy >= 2.0); dft() is the direct sum with phases reduced in integers that pins it,
and what rfft() falls back to, chunked over bins, should numpy.fft ever hand back complex128.

Bound (derived, not measured).  An FFT errs normwise: ||fl(X) - X||_2 <= c u ||X||_2 with c a small constant times the number of
stages, so every channel on its own is held to
    ||got_c - ref_c||_2 <= c(N) u ||ref_c||_2,            u = 2^-24 (float32), 2^-53 (float64),
c(N) = eval_spectra_oracle.coeff(N) = 8 (log2 N + 2) for a 7-smooth N/2 and 3 * 8 (log2 M + 2) for a Bluestein size (three M-point
passes); for the synthesis with ||w * irfft(S_c)||_2 + ||overlap_c||_2 on the right.  NumPy's own float32 / float64 transforms use
0.2 % ... 8 % of it at N = 4 ... 8192 (test_cpu_transform_oracle.py measures that again).  The 19 channels of inputs() span six
decades of amplitude, so that a channel that is wrong cannot hide behind a louder one."""
import functools

import numpy as np

from eval_spectra_oracle import bluestein_length, coeff

LD = np.longdouble
CLD = np.result_type(LD, np.complex64).type       # complex256 where long double is wider than double
EPS_LD = float(np.finfo(LD).eps)
PI = LD(4) * np.arctan(LD(1))
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
REAL = {"f32": np.float32, "f64": np.float64}
CPLX = {"f32": np.complex64, "f64": np.complex128}

# ---- the plan rule of make_plan (csrc/kernels_stft.hip), restated -------------------------------------------------
STFT_TPB, INPLACE_MAX_IT, STFT_MAX_N, STFT_MAX_BLUESTEIN_N = 256, 4, 8192, 4096
RULE = "above 4096, N/2 must factor into 2, 3, 5 and 7"
F64_RULE = r"block_size <= 4096 \(double-precision FFT in LDS\)"


def _stages(L):
    st = []
    for r in (4, 2, 3, 5, 7):
        while L % r == 0 and L > 1:
            st.append(r)
            L //= r
    return st, L


def plan_of(N):
    """None for a refused size; else dict(family "inplace" | "mixed" | "bluestein", radix: stage radices (of the M-point transforms for
    a Bluestein size), M, buf, max_it, lds: {"f32": bytes, "f64": bytes})"""
    if N < 4 or N > STFT_MAX_N or N % 2:
        return None
    st, rem = _stages(N // 2)
    M, buf = 0, N // 2
    if rem != 1:
        if N > STFT_MAX_BLUESTEIN_N:
            return None
        M = 1
        while M < N - 1:
            M *= 2
        buf = M
        st, rem = _stages(M)
        assert rem == 1
    inplace = all(r in (2, 4) and buf // r <= INPLACE_MAX_IT * STFT_TPB for r in st)
    max_it = max([1] + [-(-(buf // r) // STFT_TPB) for r in st]) if inplace else INPLACE_MAX_IT
    family = "bluestein" if M else ("inplace" if inplace else "mixed")
    return dict(family=family, radix=st, M=M, buf=buf, max_it=max_it,
                lds={"f32": 8 * (1 if inplace else 2) * buf, "f64": 16 * (1 if inplace else 2) * buf})


# ---- the sizes of tests/test_gpu_transforms.py (their coverage conditions: test_cpu_transform_oracle.py) ---------------
EVEN_TO_128 = tuple(range(4, 130, 2))
INPLACE_EDGE = (1024, 2048, 4096, 8192)
BLUESTEIN_EDGE = (1018, 1020, 1022, 1026, 1030, 2046, 2050, 4094)
ODD_RADIX = (1458, 1250, 686, 210, 1600, 4050)
ABOVE_4096 = (4374, 4802, 6000, 6144, 7000, 8064, 8100)
ALL_SIZES = EVEN_TO_128 + INPLACE_EDGE + BLUESTEIN_EDGE + ODD_RADIX + ABOVE_4096
REFUSED = (8190, 4100)
ANALYSIS_ARG_SIZES = (32, 70, 210, 1020, 1600, 2048)
JOBS_SIZES = (64, 250, 1020, 2048)
SYNTHESIS_ARG_SIZES = (32, 70, 1020, 2048)


def cases(sizes=ALL_SIZES):
    """(N, dtype) for every size in both precisions, float32 alone above 4096"""
    return [(N, d) for N in sizes for d in ("f32", "f64") if d == "f32" or N <= 4096]


# ---- reference transforms ---------------------------------------------------------------------------------------
def window(N):
    return np.sin(PI * np.arange(N, dtype=LD) / LD(N))


def _roots(N):
    """exp(-2 pi i m / N), m < N, in long double: the angle is reduced to [0, pi/4] in integers (octant q and remainder t of 8 m / N),
    so that every root is within an ulp or two of the exact one"""
    q, t = np.divmod(8 * np.arange(N, dtype=np.int64), N)
    a = np.where(q % 2 == 0, t, N - t).astype(LD) * (PI / LD(4)) / LD(N)
    c, s = np.cos(a), np.sin(a)
    cos = np.choose(q, [c, s, -s, -c, -c, -s, s, c])
    sin = np.choose(q, [s, c, c, s, -s, -c, -c, -s])
    return cos - 1j * sin


def dft(x, bins=None, chunk=32):
    """direct long-double DFT of the last axis of real x at `bins` (default 0 .. N/2): phases n k reduced modulo N in integers, the N
    products of a bin summed pairwise (numpy's reduction of a contiguous axis), so that the sum errs by O(log N) ulps, not O(N)"""
    x = np.asarray(x, dtype=LD)
    N = x.shape[-1]
    bins = np.arange(N // 2 + 1) if bins is None else np.asarray(bins)
    root, n = _roots(N), np.arange(N, dtype=np.int64)
    out = np.empty(x.shape[:-1] + (bins.size,), dtype=CLD)
    for s in range(0, bins.size, chunk):
        k = bins[s:s + chunk].astype(np.int64)
        r = root[(k[:, None] * n[None, :]) % N]                              # (bins of the chunk, N)
        prod = np.ascontiguousarray(x[..., None, :] * r)
        out[..., s:s + chunk] = prod.real.sum(axis=-1) + 1j * prod.imag.sum(axis=-1)
    return out


def rfft(x):
    x = np.asarray(x, dtype=LD)
    X = np.fft.rfft(x, axis=-1)
    return X if X.dtype == CLD else dft(x)


def irfft(S, N):
    S = np.asarray(S, dtype=CLD)
    x = np.fft.irfft(S, n=N, axis=-1)
    if x.dtype == LD:
        return x
    # direct inverse: x[n] = (Re S_0 + (-1)^n Re S_{N/2} + 2 Re sum_{0 < k < N/2} S_k e^{+2 pi i n k / N}) / N
    root, n, k = np.conj(_roots(N)), np.arange(N, dtype=np.int64), np.arange(1, N // 2, dtype=np.int64)
    acc = (S[..., 1:N // 2] @ root[(k[:, None] * n[None, :]) % N]).real * 2
    return (acc + S[..., :1].real + S[..., -1:].real * (1 - 2 * (n % 2))) / LD(N)


def frame(rows, N, in_len=None, ring_off=0):
    """y of the module docstring, (n_ch, N) long double, from rows as stored (n_ch, >= in_len)"""
    rows = np.asarray(rows, dtype=LD)
    in_len = rows.shape[1] if in_len is None else in_len
    y = np.zeros((rows.shape[0], N), dtype=LD)
    if in_len:
        at = (np.arange(in_len) + ring_off) % N if ring_off % N else np.arange(in_len)
        y[:, :in_len] = rows[:, at]
    return y


def analysis(rows, N, in_len=None, ring_off=0, use_window=True):
    y = frame(rows, N, in_len, ring_off)
    return rfft(y * window(N) if use_window else y)


def synthesis(S, overlap, N, H):
    """(new overlap (n_ch, N), norm of the bound's right side per channel): out is new overlap[:, :H]"""
    assert 1 <= H <= N
    new = window(N) * irfft(S, N)
    ov = np.asarray(overlap, dtype=LD)
    shifted = np.concatenate([ov[:, H:], np.zeros((ov.shape[0], H), dtype=LD)], axis=1)
    return shifted + new, norms(new) + norms(ov)


# ---- the bound ----------------------------------------------------------------------------------------------------
def norms(a):
    a = np.asarray(a)
    return np.sqrt(np.sum(a.real.astype(LD) ** 2 + a.imag.astype(LD) ** 2, axis=-1))


def shares(got, ref, N, dtype, scale=None):
    """per channel ||got_c - ref_c||_2 / (c(N) u scale_c), scale_c = ||ref_c||_2 unless given; a channel whose scale is 0 must be
    exact (share 0) or counts as infinitely wrong"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = norms(got.astype(CLD if np.iscomplexobj(ref) else LD) - ref)
    scale = norms(ref) if scale is None else np.asarray(scale, dtype=LD)
    b = LD(coeff(N) * U[dtype]) * scale
    out = np.where(err == 0, LD(0), np.inf)
    np.divide(err, b, out=out, where=b > 0)
    return out.astype(np.float64)


# ---- input sets -----------------------------------------------------------------------------------------------------
N_CH = 19
AMPLITUDES = np.logspace(-3, 3, N_CH)
# kind of channel c, spread so that every kind meets small, middle and large amplitudes: 13 noise, 3 impulses, 3 sinusoids
KINDS = ("noise", "imp0", "noise", "sin1", "noise", "noise", "imp1", "noise", "sinhalf", "noise", "noise", "implast", "noise",
         "noise", "sinny", "noise", "noise", "noise", "noise")


@functools.lru_cache(maxsize=None)
def _inputs(N, length, dtype, seed):
    rng = np.random.default_rng((N, length, seed))
    n = np.arange(length)
    x = np.zeros((N_CH, length))
    for c, kind in enumerate(KINDS):
        if kind == "noise":
            x[c] = rng.standard_normal(length)
        elif kind.startswith("imp") and length:
            x[c, min({"imp0": 0, "imp1": 1, "implast": length - 1}[kind], length - 1)] = 1.0
        elif kind.startswith("sin"):
            f = {"sin1": 1.0, "sinny": N / 2 - 1.0, "sinhalf": N // 4 + 0.5}[kind]
            x[c] = np.cos(2 * np.pi * f * n / N + 0.3)
    x = (x * AMPLITUDES[:, None]).astype(REAL[dtype])
    x.setflags(write=False)
    return x


def inputs(N, dtype, length=None, seed=0):
    """(19, length) in the device's precision, read-only: amplitudes logspace(-3, 3, 19); 13 Gaussian noise, unit impulses at n = 0,
    1 and length - 1, real sinusoids on bin 1, bin N/2 - 1 and the half-integer bin N/4 + 1/2"""
    return _inputs(N, N if length is None else length, dtype, seed)


@functools.lru_cache(maxsize=None)
def analysis_case(N, dtype):
    """the full-length windowed case every size runs: (x, reference spectra), computed once and read-only"""
    x = inputs(N, dtype)
    ref = analysis(x, N)
    ref.setflags(write=False)
    return x, ref


@functools.lru_cache(maxsize=None)
def synthesis_case(N, dtype, H):
    """spectra = reference spectra * (1 + 0.1j) in the device's precision (DC and Nyquist carry imaginary parts that irfft drops),
    a random overlap of each channel's amplitude, and the reference: (S, overlap, new overlap, bound norms)"""
    _, X = analysis_case(N, dtype)
    S = (X * CLD(1 + 0.1j)).astype(CPLX[dtype])
    ov = (np.random.default_rng((N, H, 7)).standard_normal((N_CH, N)) * AMPLITUDES[:, None]).astype(REAL[dtype])
    ref, scale = synthesis(S, ov, N, H)
    for a in (S, ov, ref, scale):
        a.setflags(write=False)
    return S, ov, ref, scale

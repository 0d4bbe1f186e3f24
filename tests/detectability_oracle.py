"""NumPy restatement of the detectability stage of the subband stream (apvast(..., evaluation_detectability=True),
csrc/kernels_evaldetect.hip), for tests/test_gpu_evaluation_detectability.py and tests/test_cpu_evaluation_detectability.py.

In the reference's order (perceptualModel.m:118-139, 192-206), float64 with numpy.longdouble sums: the squared weighting curve of
the masker spectrum S, scaled by sqrt(2)/N,
    w2_S[k] = Cs Leff sum_c G2[k, c] / (f sum_j G2[j, c] |S[j]|^2 + Ca),     f = 2 / N^2,
then D = sum_{k >= 1} w2_S[k] f |X[k]|^2 for the disturbance X.  ``tables`` is anything with G2 (K, C), Cs, Ca, Leff: the
PerceptualTables the device received, or ``from_model(oracle.perceptual.Model(...))``.

Bounds (derived, not measured), u = 2^-53.
  * spectra given: T - B is formed in float64 first (one rounding, the device's own), so every sum is of non-negative terms and
    any order of summation stays within relative (n - 1) u: K + 2 roundings per masker power, C + 3 per curve value, K + 4 for
    the weighted sum, together below 2 (2 K + C + 16) u D.
  * spectra from pressures: add the first-order propagation of the transform's error delta_S = c(N) u ||w f||_2 per bin (c(N)
    from tests/eval_spectra_oracle.py):
        sum_{k>=1} w2[k] f (2 |X[k]| delta_X + delta_X^2) + D max_c(dmask_c / (mask_c + Ca)),
        dmask_c = f sum_k G2[k, c] (2 |T[k]| delta_T + delta_T^2)."""
import numpy as np

from eval_spectra_oracle import coeff
from oracle.subband import sine_window

U = 2.0 ** -53
LD = np.longdouble


class Tables:
    def __init__(self, G2, Cs, Ca, Leff):
        self.G2, self.Cs, self.Ca, self.Leff = np.asarray(G2, dtype=np.float64), float(Cs), float(Ca), float(Leff)


def from_model(model):
    """the same tables from oracle.perceptual.Model's own constants"""
    return Tables(model.cr ** 2, model.Cs, model.Ca, model.Leff)


def masker_power(tables, S, N):
    """(..., K) complex -> (..., C): f sum_j G2[j, c] |S[j]|^2, longdouble"""
    p = (2.0 / (float(N) * N)) * (S.real ** 2 + S.imag ** 2)
    return np.tensordot(p.astype(LD), tables.G2.astype(LD), axes=([-1], [0]))


def curve(tables, S, N):
    """squared weighting curve, (..., K) longdouble, of the masker spectra S (..., K) (unscaled rfft); S = None: silence"""
    G2 = tables.G2.astype(LD)
    if S is None:
        den = np.full(G2.shape[1], LD(tables.Ca))
    else:
        den = masker_power(tables, S, N) + LD(tables.Ca)
    return LD(tables.Cs) * LD(tables.Leff) * np.sum(G2 / den[..., None, :], axis=-1)


def detectability(w2, X, N):
    """sum_{k>=1} w2[k] f |X[k]|^2 over the last axis, float64 result"""
    p = (2.0 / (float(N) * N)) * (X.real ** 2 + X.imag ** 2)
    return np.sum(w2[..., 1:] * p[..., 1:].astype(LD), axis=-1).astype(np.float64)


def detectability_channel_form(tables, S, X, N):
    """the other order of summation: Cs Leff sum_c (f sum_{k>=1} G2[k, c] |X[k]|^2) / (mask_c + Ca)"""
    G2 = tables.G2.astype(LD)
    p = ((2.0 / (float(N) * N)) * (X.real ** 2 + X.imag ** 2)).astype(LD)
    num = np.tensordot(p[..., 1:], G2[1:], axes=([-1], [0]))
    den = (masker_power(tables, S, N) if S is not None else 0) + LD(tables.Ca)
    return (LD(tables.Cs) * LD(tables.Leff) * np.sum(num / den, axis=-1)).astype(np.float64)


def split(spec, Z, E):
    """bin-major spectra (K, Z (2 E + 1), Mv) -> B, Dk (Z, E, Mv, K) and T (Z, Mv, K)"""
    K, sets, Mv = spec.shape
    s = np.moveaxis(spec.reshape(K, Z, 2 * E + 1, Mv), 0, -1)
    return s[:, :E], s[:, E:2 * E], s[:, 2 * E]


def reference(tables, B, Dk, T, N):
    """error, leak (Z, E, Mv) and the curves used: w2 of T (Z, Mv, K) and of the leak's masker (Z, Mv, K)"""
    Z = T.shape[0]
    wT = curve(tables, T, N)
    if Z == 2:
        wL = wT[::-1]
    else:
        wL = np.broadcast_to(curve(tables, None, N), wT.shape)
    X = T[:, None] - B                                       # float64 first, as the device forms it
    return detectability(wT[:, None], X, N), detectability(wL[:, None], Dk, N), wT, wL


def bound_given(K, C, D):
    return 2.0 * (2 * K + C + 16) * U * D


def delta_spectrum(N, frame):
    """c(N) u ||w f||_2 of frames (..., N, Mv) -> (..., Mv)"""
    w = sine_window(N)[:, None]
    return coeff(N) * U * np.sqrt(np.sum((w * frame) ** 2, axis=-2))


def bound_from_pressures(tables, N, D, w2, X, dX, T, dT):
    """the second bound per element: D (..., ) of disturbance X (..., K) under the curve w2 (..., K) of the masker T (..., K);
    dX, dT (...,) the transform's error per bin of X and of T (None: a silent masker)"""
    f = 2.0 / (float(N) * N)
    K, C = tables.G2.shape
    w2 = np.asarray(w2, dtype=np.float64)
    aX = np.abs(X)
    first = np.sum(w2[..., 1:] * f * (2 * aX[..., 1:] * dX[..., None] + dX[..., None] ** 2), axis=-1)
    rel = 0.0
    if T is not None:
        aT = np.abs(T)
        dmask = f * np.tensordot(2 * aT * dT[..., None] + dT[..., None] ** 2, tables.G2, axes=([-1], [0]))
        mask = np.asarray(masker_power(tables, T, N), dtype=np.float64)
        rel = np.max(dmask / (mask + tables.Ca), axis=-1)
    return bound_given(K, C, D) + first + D * rel


class StreamReference:
    """The stage in NumPy, fed hop by hop with the pressures (Z, 2 E + 1, H, Mv) the device itself computed"""

    def __init__(self, tables, N, H, Z, E, Mv):
        self.tables, self.N, self.H, self.Z, self.E = tables, N, H, Z, E
        self.ring = np.zeros((Z, 2 * E + 1, N, Mv))

    def hop(self, p):
        N, E, Z = self.N, self.E, self.Z
        p = np.asarray(p, dtype=np.float64)
        self.ring = np.concatenate([self.ring, p], axis=2)[:, :, -N:]
        w = sine_window(N)[:, None]
        spec = np.swapaxes(np.fft.rfft(w * self.ring, axis=2), 2, 3)         # (Z, 2 E + 1, Mv, K)
        B, Dk, T = spec[:, :E], spec[:, E:2 * E], spec[:, 2 * E]
        err, leak, wT, wL = reference(self.tables, B, Dk, T, N)
        d = delta_spectrum(N, self.ring)                                      # (Z, 2 E + 1, Mv)
        dB, dD, dT = d[:, :E], d[:, E:2 * E], d[:, 2 * E]
        b_err = bound_from_pressures(self.tables, N, err, wT[:, None], T[:, None] - B, dT[:, None] + dB, T[:, None], dT[:, None])
        if Z == 2:
            b_leak = bound_from_pressures(self.tables, N, leak, wL[:, None], Dk, dD, T[::-1][:, None], dT[::-1][:, None])
        else:
            b_leak = bound_from_pressures(self.tables, N, leak, wL[:, None], Dk, dD, None, None)
        return {"error": err, "leak": leak}, {"error": b_err, "leak": b_leak}


def white_noise_case(tables, N, rng, amplitude, ratio_db, Mv=3):
    """windowed white noise: a masker of the given amplitude and a disturbance ratio_db below it; D, both bounds' parts"""
    w = sine_window(N)[:, None]
    t = amplitude * rng.standard_normal((N, Mv))
    x = amplitude * 10.0 ** (ratio_db / 20.0) * rng.standard_normal((N, Mv))
    T, X = np.fft.rfft(w * t, axis=0).T, np.fft.rfft(w * x, axis=0).T        # (Mv, K)
    w2 = curve(tables, T, N)
    D = detectability(w2, X, N)
    dT, dX = delta_spectrum(N, t), delta_spectrum(N, x)
    return D, bound_from_pressures(tables, N, D, w2, X, dX, T, dT), T, X

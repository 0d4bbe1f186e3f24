"""NumPy restatement of the per-bin evaluation spectra of the subband stream (apvast(..., evaluation_spectra=True),
csrc/kernels_evalspec.hip), for tests/test_gpu_eval_spectra.py.

After hop t (t = 0 first) the frame of pressure set s is f_t[s][i, m] = p[s][(t + 1) H - N + i, m], i < N, zero before sample 0;
P_t[s][k, m] = numpy.fft.rfft(w * f_t[s][:, m])[k] with w = oracle.subband.sine_window(N); and
    bright += |P_bright|^2, dark += |P_dark|^2, error += |P_target - P_bright|^2, target += |P_target|^2,
total = total + hop, in float64.

Bound (derived, not measured).  A length-N float64 transform errs normwise by about c u ||X||_2, u = 2^-53, c a small constant
times the number of stages, and |X_k| <= sqrt(N) ||w f||_2; so the device's and NumPy's |X_k|^2 both lie within
2 c u N ||w f||_2^2 of the exact value, and every accumulated element is held to
    |got - ref| <= 4 c(N) u N sum_t ||w f_t[:, m]||_2^2           (for "error", f = target - bright)
with c(N) = 8 (log2 N + 2) when N/2 is 7-smooth, and three times that with log2 M for a Bluestein size, M the padded length of
the plan (the power of two >= N - 1)."""
import numpy as np

from oracle.subband import sine_window

U = 2.0 ** -53
KEYS = ("bright", "dark", "error", "target")


def bluestein_length(N):
    """0 when N/2 factors into 2, 3, 5, 7; else the power of two >= N - 1 the chirp-z plan pads to"""
    r = N // 2
    for q in (2, 3, 5, 7):
        while r % q == 0:
            r //= q
    if r == 1:
        return 0
    M = 1
    while M < N - 1:
        M *= 2
    return M


def coeff(N):
    M = bluestein_length(N)
    return 3 * 8 * (np.log2(M) + 2) if M else 8 * (np.log2(N) + 2)


def bound_factor(N):
    """4 c(N) u N: times sum_t ||w f_t||^2 it bounds an accumulated element"""
    return 4 * coeff(N) * U * N


def stack_sets(p):
    """predicted_pressure()'s dict -> (Z, 2 E + 1, H, Mv): bright of the E ranks, dark, target"""
    return np.concatenate([p["bright"], p["dark"], p["target"][:, None]], axis=1)


def frame_energies(frame, N):
    """frame (Z, 2 E + 1, N, Mv) -> the hop's four |P|^2 as (Z, E, Mv, K) / (Z, Mv, K), and the four ||w f||^2 as (Z, E, Mv) /
    (Z, Mv)"""
    E = (frame.shape[1] - 1) // 2
    w = sine_window(N)[:, None]
    wf = {"bright": w * frame[:, :E], "dark": w * frame[:, E:2 * E], "target": w * frame[:, 2 * E]}
    wf["error"] = wf["target"][:, None] - wf["bright"]
    spec = {k: np.fft.rfft(wf[k], axis=-2) for k in ("bright", "dark", "target")}
    spec["error"] = spec["target"][:, None] - spec["bright"]
    en = {k: np.swapaxes(spec[k].real ** 2 + spec[k].imag ** 2, -1, -2) for k in KEYS}
    nrm = {k: np.sum(wf[k] ** 2, axis=-2) for k in KEYS}
    return en, nrm


class SpectraReference:
    """The stage in NumPy, fed hop by hop with the pressures (Z, 2 E + 1, H, Mv) the device itself computed"""

    def __init__(self, N, H, Z, E, Mv):
        self.N, self.H = N, H
        self.ring = np.zeros((Z, 2 * E + 1, N, Mv))              # the last N samples, oldest first
        K = N // 2 + 1
        self.totals = {"bright": np.zeros((Z, E, Mv, K)), "dark": np.zeros((Z, E, Mv, K)), "error": np.zeros((Z, E, Mv, K)),
                       "target": np.zeros((Z, Mv, K))}
        self.norms = {"bright": np.zeros((Z, E, Mv)), "dark": np.zeros((Z, E, Mv)), "error": np.zeros((Z, E, Mv)),
                      "target": np.zeros((Z, Mv))}
        self.last = None

    def hop(self, p):
        p = np.asarray(p, dtype=np.float64)
        assert p.shape == self.ring.shape[:2] + (self.H, self.ring.shape[3])
        self.ring = np.concatenate([self.ring, p], axis=2)[:, :, -self.N:]
        en, nrm = frame_energies(self.ring, self.N)
        for k in KEYS:
            self.totals[k] = self.totals[k] + en[k]
            self.norms[k] = self.norms[k] + nrm[k]
        self.last = en
        return en

    def bound(self, key):
        """per element of totals[key]"""
        return bound_factor(self.N) * self.norms[key][..., None]


def check(got, ref, worst=None):
    """every element of the four accumulated arrays within the bound; returns the largest share of it"""
    share = 0.0
    for k in KEYS:
        assert got[k].shape == ref.totals[k].shape, (k, got[k].shape)
        err, b = np.abs(got[k] - ref.totals[k]), np.broadcast_to(ref.bound(k), got[k].shape)
        if (b > 0).any():
            share = max(share, (err[b > 0] / b[b > 0]).max())
        assert np.all(err <= b), (k, share)
    if worst is not None:
        worst[0] = max(worst[0], share)
    return share

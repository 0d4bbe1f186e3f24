"""Evaluation helpers and the static solver of the reference's MATLAB side, on the device.

  predict_pressure   Matlab/ControlMethods/predictPressure.m:1-17
  nmse, acoustic_contrast_db   Matlab/main.m:120-130
  metrics            the same two from the energies a subband stream's evaluation stage accumulates on the device
  validation_contrast_db   the contrast the validation span (apvast(..., validation_floor_db=)) predicts per bin and filter
  spectral_metrics   contrast and NMSE per bin or band from the per-bin energies (apvast.evaluation_spectra())
  detectability_metrics   mean detectability and audible share of hops (apvast.evaluation_detectability())
  third_octave_bands the bin ranges of base-2 third-octave bands, for spectral_metrics
  vast               Matlab/ControlMethods/vast.m:1-97 (signal-independent VAST from the RIRs)

MATLAB/Octave are not available where this was built, so these follow the .m files by reading only
(parity unpinned); tests check them against a NumPy restatement in oracle/ and against
the closed-form limits (KA-4)."""
import numpy as np

from . import _capi

_engine = None


def _eng(device=0):
    global _engine
    if _engine is None or _engine[0] != device:
        _engine = (device, _capi.Engine(1, 4, 4, device=device))
    return _engine[1]


def predict_pressure(loudspeaker_signals, rirs, device=0):
    """loudspeaker_signals (T, L), rirs (rir_len, L, M) -> predicted pressure (T, M)."""
    return _eng(device).predict_pressure(loudspeaker_signals, rirs)


def nmse(target_pressure, pressure):
    """Mean over microphones of ||target - p||^2 / ||target||^2 (main.m:120-127)."""
    t = np.asarray(target_pressure, dtype=float)
    p = np.asarray(pressure, dtype=float)
    return float(np.mean(np.sum((t - p) ** 2, axis=0) / np.sum(t ** 2, axis=0)))


def acoustic_contrast_db(pressure_bright, pressure_dark):
    """10 log10(||p_bright||_F^2 / ||p_dark||_F^2) (main.m:129-130)."""
    return float(10.0 * np.log10(np.sum(np.asarray(pressure_bright) ** 2) / np.sum(np.asarray(pressure_dark) ** 2)))


def metrics(totals):
    """NMSE and acoustic contrast from accumulated energies (main.m:120-130): ``totals`` as apvast.evaluation_totals() returns
    them (or a slot of evaluation_hops()): "bright", "dark", "error" (Z, E, Mv) and "target" (Z, Mv) ->
    {"nmse": (Z, E), "contrast_db": (Z, E)} with nmse[z, v] = mean_m error[z, v, m] / target[z, m] and
    contrast_db[z, v] = 10 log10(sum_m bright[z, v, m] / sum_m dark[z, v, m])."""
    bright = np.asarray(totals["bright"], dtype=np.float64)
    dark = np.asarray(totals["dark"], dtype=np.float64)
    error = np.asarray(totals["error"], dtype=np.float64)
    target = np.asarray(totals["target"], dtype=np.float64)
    return {"nmse": np.mean(error / target[..., None, :], axis=-1),
            "contrast_db": 10.0 * np.log10(np.sum(bright, axis=-1) / np.sum(dark, axis=-1))}


def validation_contrast_db(bright, dark):
    """10 log10(bright / dark) (main.m:129-130) of the energies a validation span reports (apvast.validation_bright_* /
    validation_dark_*, any shape): +inf where dark = 0 < bright, NaN where both are 0 or either is not finite."""
    b = np.asarray(bright, dtype=np.float64)
    d = np.asarray(dark, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = 10.0 * np.log10(b / d)
    return np.where(np.isfinite(b) & np.isfinite(d), c, np.nan)


def detectability_metrics(totals):
    """Mean detectability per hop and the audible share of hops from accumulated detectabilities: ``totals`` as
    apvast.evaluation_detectability() returns them -- "error", "leak" (sums, (Z, E, Mv)), "error_audible", "leak_audible" (hops
    with D > 1, (Z, E, Mv)) and "hops" -> {"error_mean", "leak_mean", "error_audible_share", "leak_audible_share"}, each (Z, E):
    mean[z, v] = mean_m sum[z, v, m] / hops (D = 1: just audible) and share[z, v] = mean_m audible[z, v, m] / hops."""
    hops = int(totals["hops"])
    if hops < 1:
        raise ValueError("detectability_metrics: totals of at least one hop")
    out = {}
    for name in ("error", "leak"):
        out[name + "_mean"] = np.mean(np.asarray(totals[name], dtype=np.float64), axis=-1) / hops
        out[name + "_audible_share"] = np.mean(np.asarray(totals[name + "_audible"], dtype=np.float64), axis=-1) / hops
    return out


def spectral_metrics(spectra, bands=None):
    """Contrast and NMSE over frequency from per-bin energies: ``spectra`` as apvast.evaluation_spectra() returns them, "bright",
    "dark", "error" (Z, E, Mv, K) and "target" (Z, Mv, K), K = N/2 + 1 -> {"contrast_db": (Z, E, B), "nmse": (Z, E, B)} with
    contrast_db = 10 log10(sum_m bright / sum_m dark) and nmse = sum_m error / sum_m target: a ratio of sums, since a single
    microphone's target can vanish in a bin.  ``bands=None``: one band per bin (B = K).  Otherwise a sequence of half-open bin
    ranges (k0, k1), 0 <= k0 < k1 <= K; the energies of a range are pooled with the one-sided weights c_k (1 for bin 0 and bin
    N/2, 2 otherwise), so a band's energy is its share of the two-sided spectrum."""
    bright = np.asarray(spectra["bright"], dtype=np.float64).sum(axis=-2)          # (Z, E, K)
    dark = np.asarray(spectra["dark"], dtype=np.float64).sum(axis=-2)
    error = np.asarray(spectra["error"], dtype=np.float64).sum(axis=-2)
    target = np.asarray(spectra["target"], dtype=np.float64).sum(axis=-2)[..., None, :]
    if bands is not None:
        K = bright.shape[-1]
        try:
            bands = [(k0, k1) for k0, k1 in bands]
        except (TypeError, ValueError):
            raise ValueError("bands must be None or a sequence of half-open bin ranges (k0, k1)")
        for k0, k1 in bands:
            if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (k0, k1)) or not 0 <= k0 < k1 <= K:
                raise ValueError(f"band ({k0}, {k1}): half-open bin ranges with 0 <= k0 < k1 <= {K}")
        if not bands:
            raise ValueError("bands must hold at least one bin range")
        c = np.full(K, 2.0)
        c[0] = c[K - 1] = 1.0
        pool = lambda a: np.stack([np.sum(c[k0:k1] * a[..., k0:k1], axis=-1) for k0, k1 in bands], axis=-1)
        bright, dark, error, target = pool(bright), pool(dark), pool(error), pool(target)
    return {"contrast_db": 10.0 * np.log10(bright / dark), "nmse": error / target}


def third_octave_bands(sample_rate, block_size, f_min=None, f_max=None):
    """(centres_hz, bands) for spectral_metrics: base-2 third-octave bands around 1 kHz, centres 1000 * 2^(i/3) Hz, band i holding
    the bins whose centre frequencies k * sample_rate / block_size lie in [centre * 2^(-1/6), centre * 2^(1/6)).  Bands whose
    centre lies outside [f_min, f_max] (defaults: the first bin above 0 Hz, the Nyquist frequency) or that hold no bin centre
    are dropped.  The ranges are ascending and do not overlap."""
    fs, N = float(sample_rate), int(block_size)
    if not fs > 0 or N < 2 or N % 2:
        raise ValueError("third_octave_bands: a positive sample rate and an even block size")
    K = N // 2 + 1
    lo = fs / N if f_min is None else float(f_min)
    hi = fs / 2 if f_max is None else float(f_max)
    if not 0 < lo <= hi:
        raise ValueError("third_octave_bands: 0 < f_min <= f_max")
    centres, bands = [], []
    for i in range(int(np.floor(3 * np.log2(lo / 1000.0))) - 1, int(np.ceil(3 * np.log2(hi / 1000.0))) + 2):
        fc = 1000.0 * 2.0 ** (i / 3.0)
        if not lo <= fc <= hi:
            continue
        # first bin whose centre is at or above each edge; neighbouring bands share the edge 1000 * 2^((2 i + 1) / 6), same expression
        k0 = int(np.ceil(1000.0 * 2.0 ** ((2 * i - 1) / 6.0) * N / fs))
        k1 = int(np.ceil(1000.0 * 2.0 ** ((2 * i + 1) / 6.0) * N / fs))
        k0, k1 = max(k0, 0), min(k1, K)
        if k1 > k0:
            centres.append(fc)
            bands.append((k0, k1))
    return np.array(centres), bands


def vast(gB, gD, filter_length, modelling_delay, reference_index, number_of_eigenvectors, mu, device=0):
    """Static VAST filters.  gB (Nb, rir_len, L), gD (Nd, rir_len, L) as in vast.m; ``reference_index`` is
    0-based (vast.m's is 1-based).  Returns w of shape (filter_length * L,), loudspeaker-major taps
    [w_1(0..J-1), ..., w_L(0..J-1)] (vast.m:38-39)."""
    return _eng(device).vast_static(gB, gD, filter_length, modelling_delay, reference_index,
                                    number_of_eigenvectors, mu)

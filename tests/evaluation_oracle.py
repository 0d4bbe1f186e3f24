"""NumPy / SciPy restatement of the subband stream's evaluation stage (apvast(..., validation_rir_A=, validation_rir_B=),
csrc/kernels_streameval.hip): predictPressure.m:12-16 carried across hops -- scipy.signal.lfilter per (loudspeaker, microphone)
with its state zi kept from hop to hop, summed over the loudspeakers -- the four energies per hop and microphone, and the metrics
of main.m:120-130 from summed energies.  Everything float64."""
import numpy as np
import scipy.signal

U64 = 2.0 ** -53


def pressure_bound(L, Pv):
    """|got - ref| <= pressure_bound(L, Pv) * S, S = sum_l sum_j |rv| |y|: a dot product of L Pv terms summed in any order errs by at
    most about L Pv u S, and the reference carries the same."""
    return 2 * (L * Pv + 6) * U64


def energy_bound(H):
    """|got - ref| <= energy_bound(H) * E for an energy E of H squared samples summed in any order."""
    return (H + 8) * U64


class PressureFilter:
    """p[n, m] = sum_l sum_{j < Pv} rv[j, l, m] y[n - j, l] over consecutive hops, y zero before the first (lfilter with zero zi).
    hop(y) returns (p, S) for the hop y (H, L): S the same sum of absolute values, the scale of the rounding error."""

    def __init__(self, rv):
        self.rv = np.array(rv, dtype=np.float64)
        self.Pv, self.L, self.Mv = self.rv.shape
        self.zi = np.zeros((2, self.L, self.Mv, self.Pv - 1))

    def hop(self, y):
        y = np.asarray(y, dtype=np.float64)
        assert y.ndim == 2 and y.shape[1] == self.L
        out = np.zeros((2, y.shape[0], self.Mv))
        for q, (b, x) in enumerate(((self.rv, y), (np.abs(self.rv), np.abs(y)))):
            for l in range(self.L):
                for m in range(self.Mv):
                    if self.Pv == 1:
                        out[q, :, m] += b[0, l, m] * x[:, l]
                    else:
                        r, self.zi[q, l, m] = scipy.signal.lfilter(b[:, l, m], 1.0, x[:, l], zi=self.zi[q, l, m])
                        out[q, :, m] += r
        return out[0], out[1]


def window_pressure(y, rv, H):
    """The kernel's own definition on one group: y (Pv - 1 + H, L) -- the Pv - 1 samples in front of the hop, then the hop -- and
    rv (Pv, L, Mv) -> (p, S) (H, Mv), p[n, m] = sum_l sum_j rv[j, l, m] y[Pv - 1 + n - j, l]."""
    y = np.asarray(y, dtype=np.float64)
    rv = np.asarray(rv, dtype=np.float64)
    Pv = rv.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(y, Pv, axis=0)[:H, :, ::-1]      # (H, L, Pv): win[n, l, j] = y[Pv - 1 + n - j, l]
    return np.einsum("nlj,jlm->nm", win, rv), np.einsum("nlj,jlm->nm", np.abs(win), np.abs(rv))


def energies(p_bright, p_dark, p_target):
    """(H, Mv) pressures of one hop -> bright, dark, error, target, each (Mv,)."""
    return (np.sum(p_bright ** 2, axis=0), np.sum(p_dark ** 2, axis=0), np.sum((p_target - p_bright) ** 2, axis=0),
            np.sum(p_target ** 2, axis=0))


def metrics(bright, dark, error, target):
    """main.m:120-130 from energies summed over the signal, each (Mv,): (nmse, contrast_db)."""
    return float(np.mean(error / target)), float(10.0 * np.log10(np.sum(bright) / np.sum(dark)))


class StreamEvaluation:
    """The evaluation of a stream's returned outputs: fed with what process_input_buffers returns, hop by hop, it keeps one
    PressureFilter per pressure set and the running totals.  Shapes follow apvast: Z zone programs that run (A first), the
    evaluated ranks `ranks` (1-based), bright / dark / error (Z, E, ...), target (Z, ...)."""

    def __init__(self, rv_A, rv_B, ranks, run_A=True, run_B=True):
        self.zones = [z for z, run in enumerate((run_A, run_B)) if run]
        self.ranks = list(ranks)
        rv = (np.asarray(rv_A, dtype=np.float64), np.asarray(rv_B, dtype=np.float64))
        self.f_bright = [[PressureFilter(rv[z]) for _ in self.ranks] for z in self.zones]
        self.f_dark = [[PressureFilter(rv[1 - z]) for _ in self.ranks] for z in self.zones]
        self.f_target = [PressureFilter(rv[z]) for z in self.zones]
        self.totals = None

    def hop(self, out):
        """out = (A, B, A_t, B_t) of one hop -> dict of the hop's pressures "bright", "dark" (Z, E, H, Mv), "target" (Z, H, Mv),
        their error scales "S_bright", "S_dark", "S_target", and the energies "e_bright", "e_dark", "e_error" (Z, E, Mv),
        "e_target" (Z, Mv)."""
        pb, pd, pt, sb, sd, st = [], [], [], [], [], []
        for i, z in enumerate(self.zones):
            b = [self.f_bright[i][e].hop(out[z][v - 1]) for e, v in enumerate(self.ranks)]
            d = [self.f_dark[i][e].hop(out[z][v - 1]) for e, v in enumerate(self.ranks)]
            t = self.f_target[i].hop(out[2 + z][0])
            pb.append(np.stack([q[0] for q in b])); sb.append(np.stack([q[1] for q in b]))
            pd.append(np.stack([q[0] for q in d])); sd.append(np.stack([q[1] for q in d]))
            pt.append(t[0]); st.append(t[1])
        r = {"bright": np.stack(pb), "dark": np.stack(pd), "target": np.stack(pt),
             "S_bright": np.stack(sb), "S_dark": np.stack(sd), "S_target": np.stack(st)}
        r["e_bright"] = np.sum(r["bright"] ** 2, axis=2)
        r["e_dark"] = np.sum(r["dark"] ** 2, axis=2)
        r["e_error"] = np.sum((r["target"][:, None] - r["bright"]) ** 2, axis=2)
        r["e_target"] = np.sum(r["target"] ** 2, axis=1)
        e = {k: r["e_" + k] for k in ("bright", "dark", "error", "target")}
        self.totals = e if self.totals is None else {k: self.totals[k] + e[k] for k in e}
        return r

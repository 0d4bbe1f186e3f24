"""Test helper (not collected): the streaming subband oracles with the filter-length constraint.

Between the filter step and the synthesis of a hop every filter is projected onto the spectra of J-tap responses,

    g = irfft(W[:, v, l], N);  g[J:] = 0;  W'[:, v, l] = rfft(g, N)

(`project` below: the three lines of the definition).  The projection sits where the windowed helper already intercepts
oracle.subband.update -- what that call returns is what SubbandStreamOracle.process multiplies the input spectrum with and stores
as self.w -- so oracle/ is imported unchanged.  ConstrainedSubbandOracle with stat_hops = 1 is SubbandStreamOracle plus the
projection (the windowed helper with one hop equals it bit for bit, tests/test_cpu_stat_window.py); stat_hops = T and
ConstrainedForgettingOracle are the window and the forgetting helper plus the projection."""
import numpy as np

from forgetting_oracle import ForgettingSubbandOracle
from windowed_oracle import WindowedSubbandOracle


def project(w, N, J):
    """w (K, ...) complex, bins along axis 0 -> (w', taps): the definition, and g[:J]"""
    g = np.fft.irfft(w, N, axis=0)
    g[J:] = 0
    return np.fft.rfft(g, N, axis=0), g[:J].copy()


class _Projection:
    def _init_projection(self, filter_taps):
        self.J = int(filter_taps)
        if not 1 <= self.J <= self.N:
            raise ValueError("filter_taps must be in 1..block_size")
        self.w_time = [None, None]                 # per zone program: (nV, J, L), the taps of the last hop

    def _windowed_update(self, XB, XD, d, mu, ranks, reg):
        z = self._zone_order[0]                    # the parent pops it
        w, lam, status = super()._windowed_update(XB, XD, d, mu, ranks, reg)
        w, taps = project(w, self.N, self.J)       # (K, nV, L), (J, nV, L)
        self.w_time[z] = taps.transpose(1, 0, 2)
        return w, lam, status


class ConstrainedSubbandOracle(_Projection, WindowedSubbandOracle):
    def __init__(self, *args, filter_taps, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_projection(filter_taps)


class ConstrainedForgettingOracle(_Projection, ForgettingSubbandOracle):
    def __init__(self, *args, filter_taps, beta, **kwargs):
        super().__init__(*args, beta=beta, **kwargs)
        self._init_projection(filter_taps)

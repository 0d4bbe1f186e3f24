"""Test helper (not collected): the streaming subband oracle with per-bin statistics over a window of hops.

WindowedSubbandOracle stacks the last `stat_hops` hops' (X_B, X_D, d) along the control-point axis and hands the stack to
oracle.subband.update: X^H X of the stack is the sum over the hops of X^H X, which is the definition of the windowed
statistics.  Everything else is SubbandStreamOracle; with stat_hops = 1 the two are equal bit for bit."""
from collections import deque

import numpy as np

import oracle.subband_stream as _stream
from oracle import subband
from oracle.subband_stream import SubbandStreamOracle


class _WindowedSubband:
    """oracle.subband as SubbandStreamOracle.process sees it, with `update` going through the owner's window."""

    def __init__(self, owner):
        self._owner = owner

    def __getattr__(self, name):
        return getattr(subband, name)

    def update(self, XB, XD, d, mu, ranks, reg=None):
        return self._owner._windowed_update(XB, XD, d, mu, ranks, reg)


class WindowedSubbandOracle(SubbandStreamOracle):
    """solver="jdiag": oracle.subband.update (the reference's route); "eigh": oracle.subband.update_vectorised (batched LAPACK
    cholesky -> inverse -> eigh), a second float64 evaluation of the same definition: how far the two lie apart on an input says
    how well that input determines its answer in float64.

    process() swaps the module global oracle.subband_stream.subband for the duration of the call and tells the zone programs
    apart by the order in which the parent calls update (A, then B).  test_cpu_stat_window's bit-for-bit equality with
    SubbandStreamOracle at stat_hops = 1 is what guards both assumptions."""

    def __init__(self, *args, stat_hops=1, solver="jdiag", **kwargs):
        super().__init__(*args, **kwargs)
        self.stat_hops = int(stat_hops)
        self.solver = solver
        self.window_hops = [deque(maxlen=self.stat_hops), deque(maxlen=self.stat_hops)]    # per zone program: (XB, XD, d), oldest first

    def _windowed_update(self, XB, XD, d, mu, ranks, reg):
        z = self._zone_order.pop(0)
        self.window_hops[z].append((XB.copy(), XD.copy(), d.copy()))
        XBs, XDs, ds = (np.concatenate([hop[i] for hop in self.window_hops[z]], axis=1) for i in range(3))
        if self.solver == "eigh":
            w, lam = subband.update_vectorised(XBs, XDs, ds, mu, ranks, reg=self.reg)
            return w, lam, np.zeros(len(w), dtype=np.int32)
        return subband.update(XBs, XDs, ds, mu, ranks, reg=reg)

    def process(self, xA, xB):
        self._zone_order = [z for z in range(2) if self.run[z]]
        saved = _stream.subband
        _stream.subband = _WindowedSubband(self)
        try:
            return super().process(xA, xB)
        finally:
            _stream.subband = saved

    def window_statistics(self, z):
        """R_B, R_D (K, L, L) and r (K, L) of zone program z: the sums over the hops in the window, formed hop by hop."""
        parts = [subband.correlate(*hop) for hop in self.window_hops[z]]
        return tuple(sum(p[i] for p in parts) for i in range(3))

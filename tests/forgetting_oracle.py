"""Test helper (not collected): the streaming subband oracle with exponentially forgetting per-bin statistics.

ForgettingSubbandOracle keeps every hop since the start and hands oracle.subband.update the stack (along the control-point axis,
oldest first) in which the hop of age a -- 0 for the newest -- is scaled by beta^(a/2), X_B, X_D and d alike.  X^H X of that
stack is sum_a beta^a X^(h-a)H X^(h-a), and X_B^H d likewise: the recursion R <- beta R + G from R = 0, exactly.  Everything
else is WindowedSubbandOracle; with beta = 1 the stack is that of a window that never fills, bit for bit (x 1.0 is exact)."""
from collections import deque

import numpy as np

from oracle import subband
from windowed_oracle import WindowedSubbandOracle


class ForgettingSubbandOracle(WindowedSubbandOracle):
    def __init__(self, *args, beta, solver="jdiag", **kwargs):
        super().__init__(*args, stat_hops=1, solver=solver, **kwargs)
        if not 0.0 < beta <= 1.0:
            raise ValueError("beta must be in (0, 1]")
        self.beta = float(beta)
        self.window_hops = [deque(), deque()]         # every hop since the start, oldest first

    def _stack(self, z):
        n = len(self.window_hops[z])
        scale = [self.beta ** ((n - 1 - i) / 2) for i in range(n)]
        return tuple(np.concatenate([s * hop[i] for s, hop in zip(scale, self.window_hops[z])], axis=1) for i in range(3))

    def _windowed_update(self, XB, XD, d, mu, ranks, reg):
        z = self._zone_order.pop(0)
        self.window_hops[z].append((XB.copy(), XD.copy(), d.copy()))
        XBs, XDs, ds = self._stack(z)
        if self.solver == "eigh":
            w, lam = subband.update_vectorised(XBs, XDs, ds, mu, ranks, reg=self.reg)
            return w, lam, np.zeros(len(w), dtype=np.int32)
        return subband.update(XBs, XDs, ds, mu, ranks, reg=reg)

    def forgetting_statistics(self, z):
        """R_B, R_D (K, L, L) and r (K, L) of zone program z after the last hop: the statistics of the scaled stack."""
        return subband.correlate(*self._stack(z))

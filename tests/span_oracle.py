"""Test helper (not collected): the subband oracles with the per-bin span.

Per bin k of zone program z, after oracle.gevd.jdiag (lambda_1 >= ... >= lambda_L, sorted columns u_i), in NumPy float64:

    mu_k  = mu * m[z, k]                              a_i = (u_i^H r) / (lambda_i + mu_k)
    num_v = sum_{i<=v} lambda_i |a_i|^2               den_v = sum_{i<=v} |a_i|^2          c_v = num_v / den_v (0 where den_v = 0)
    f_k   = number of leading v with num_v >= phi den_v, at least 1 (L without a floor),  phi = 10^(floor_db / 10)
    s_k   = min(cap[z, k], f_k)                       slot t holds w_{min(ranks[t], s_k)}

`span_gevd_vast` is that for a batch of bins (the kernel-level tests); `SpanSubbandOracle` puts it where the windowed helper
intercepts oracle.subband.update, so statistics windows, forgetting and the projection of the constrained stream compose with it.
With no span part set the helpers call their parents and are equal to them bit for bit."""
import numpy as np

from oracle import gevd, subband
from constraint_oracle import _Projection
from forgetting_oracle import ForgettingSubbandOracle
from windowed_oracle import WindowedSubbandOracle


def span_bin(U, lam, r, mu_k, cap, phi, ranks):
    """One bin: (w (nV, L), s_k, c (L,))."""
    L = lam.size
    a = (U.conj().T @ np.asarray(r).reshape(-1)) / (lam + mu_k)
    e = a.real * a.real + a.imag * a.imag
    den = np.cumsum(e)
    num = np.cumsum(lam * e)
    c = np.zeros(L)
    np.divide(num, den, out=c, where=den > 0)
    f = L
    if phi is not None:
        ok = num >= phi * den
        f = L if ok.all() else int(np.argmin(ok))
        f = max(f, 1)
    s = min(int(cap), f)
    w = np.stack([U[:, :min(V, s)] @ a[:min(V, s)] for V in ranks])
    return w, s, c


def span_gevd_vast(RB, RD, r, mu, ranks, reg, mu_profile=None, rank_cap=None, floor_db=None):
    """Batch of bins from explicit statistics: w (K, nV, L), lam (K, L), span_rank (K,), span_contrast (K, L)."""
    K, L, _ = RB.shape
    phi = None if floor_db is None else 10.0 ** (floor_db / 10.0)
    w = np.zeros((K, len(ranks), L), dtype=np.complex128)
    lam = np.zeros((K, L))
    rank = np.zeros(K, dtype=np.int32)
    con = np.zeros((K, L))
    for k in range(K):
        U, lam[k] = gevd.jdiag(RB[k], RD[k], gevd.REG_MODE_ABS, reg)
        mu_k = mu * (1.0 if mu_profile is None else float(mu_profile[k]))
        cap = L if rank_cap is None else rank_cap[k]
        w[k], s, con[k] = span_bin(U, lam[k], r[k], mu_k, cap, phi, ranks)
        rank[k] = min(ranks[-1], s)
    return w, lam, rank, con


class _SpanRule:
    """Mixin in front of a windowed helper: attributes mu_profile, rank_cap ((2, K) or None) and floor_db (float or None) may be
    reassigned between hops, like the object's under test."""

    def _init_span(self, mu_profile, rank_cap, floor_db):
        def rows(a):
            if a is None:
                return None
            a = np.asarray(a)
            return np.stack([a, a]) if a.ndim == 1 else a
        self.mu_profile, self.rank_cap, self.floor_db = rows(mu_profile), rows(rank_cap), floor_db
        self.span_rank = [None, None]
        self.span_contrast = [None, None]

    def _windowed_update(self, XB, XD, d, mu, ranks, reg):
        z = self._zone_order[0]                    # the parent pops it
        out = super()._windowed_update(XB, XD, d, mu, ranks, reg)       # keeps the window; its solve is the plain stream's
        if self.mu_profile is None and self.rank_cap is None and self.floor_db is None:
            return out
        if hasattr(self, "_stack"):
            XBs, XDs, ds = self._stack(z)
        else:
            XBs, XDs, ds = (np.concatenate([hop[i] for hop in self.window_hops[z]], axis=1) for i in range(3))
        RB, RD, r = subband.correlate(XBs, XDs, ds)
        w, lam, rank, con = span_gevd_vast(RB, RD, r, mu, ranks, reg,
                                           None if self.mu_profile is None else self.mu_profile[z],
                                           None if self.rank_cap is None else self.rank_cap[z], self.floor_db)
        self.span_rank[z], self.span_contrast[z] = rank, con
        return w, lam, np.zeros(len(w), dtype=np.int32)


class SpanSubbandOracle(_SpanRule, WindowedSubbandOracle):
    def __init__(self, *args, mu_profile=None, rank_cap=None, floor_db=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_span(mu_profile, rank_cap, floor_db)


class SpanForgettingOracle(_SpanRule, ForgettingSubbandOracle):
    def __init__(self, *args, mu_profile=None, rank_cap=None, floor_db=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_span(mu_profile, rank_cap, floor_db)


class SpanConstrainedOracle(_Projection, _SpanRule, WindowedSubbandOracle):
    def __init__(self, *args, filter_taps, mu_profile=None, rank_cap=None, floor_db=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_span(mu_profile, rank_cap, floor_db)
        self._init_projection(filter_taps)

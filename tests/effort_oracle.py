"""Test helper (not collected): the subband oracles with the per-bin array-effort limit.

Per bin k, with the limit E > 0 (linear, +inf: none) and the hop's filters W[k, t, :], t = 0 .. nV - 1, in NumPy float64:

    e_t    = sum_l |W[k, t, l]|^2                     slot t is admissible if e_t is finite and e_t <= E
    src_t  = the largest admissible t' <= t
    slot t = itself where src_t = t, a copy of slot src_t where src_t < t, W[k, t, :] sqrt(E / e_t) where there is no src_t;
             a slot whose e_t is not finite is left as it is

`limit_effort` is that for a batch of bins; `_EffortLimit` puts it where the windowed helper intercepts oracle.subband.update,
behind the span (span_oracle._SpanRule) and ahead of the projection (constraint_oracle._Projection).  With no limit set the helpers
call their parents and are equal to them bit for bit."""
import numpy as np

from constraint_oracle import _Projection
from forgetting_oracle import ForgettingSubbandOracle
from span_oracle import _SpanRule
from windowed_oracle import WindowedSubbandOracle


def decide(e, E, ranks):
    """The decisions an effort curve e (K, nV) leads to under the limit E (a float or (K,)): (src (K, nV), the source slot of
    every slot, -1 where it has none; effort_rank (K,) int32 and gain (K,) of the top slot)."""
    e = np.asarray(e, dtype=np.float64)
    K, nV = e.shape
    E = np.broadcast_to(np.asarray(E, dtype=np.float64), (K,))
    fin = np.isfinite(e)
    src = np.where(fin, np.maximum.accumulate(np.where(fin & (e <= E[:, None]), np.arange(nV), -1), axis=1), -1)
    top, scaled = src[:, -1], (src[:, -1] < 0) & fin[:, -1]
    r = np.asarray(ranks, dtype=np.int32)
    rank = np.where(top >= 0, r[np.maximum(top, 0)], np.where(scaled, r[-1], 0)).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = np.where(scaled, np.sqrt(E / e[:, -1]), 1.0)
    return src, rank, gain


def limit_effort(W, E, ranks):
    """W (K, nV, L) complex, E a float or (K,), ranks the nV ranks of the slots -> (W', effort (K, nV), effort_rank (K,) int32,
    gain (K,), src (K, nV))."""
    W = np.asarray(W)
    K, nV, _ = W.shape
    E = np.broadcast_to(np.asarray(E, dtype=np.float64), (K,))
    e = (W.real.astype(np.float64) ** 2 + W.imag.astype(np.float64) ** 2).sum(axis=-1)
    src, rank, gain = decide(e, E, ranks)
    out = W.copy()
    for k, t in zip(*np.nonzero(src != np.arange(nV))):
        if src[k, t] >= 0:
            out[k, t] = W[k, src[k, t]]
        elif np.isfinite(e[k, t]):
            out[k, t] = (W[k, t].astype(np.complex128) * np.sqrt(E[k] / e[k, t])).astype(W.dtype)
    return out, e, rank, gain, src


class _EffortLimit:
    """Mixin in front of a windowed helper (and of the span rule): attribute effort_limit ((2, K) linear, or None) may be
    reassigned between hops, like the object's under test."""

    def _init_effort(self, effort_limit):
        self.effort_limit = None if effort_limit is None else np.broadcast_to(np.asarray(effort_limit, dtype=np.float64),
                                                                               (2, self.N // 2 + 1))
        self.effort = [None, None]
        self.effort_rank = [None, None]
        self.effort_gain = [None, None]
        self.effort_src = [None, None]
        self.w_unlimited = [None, None]            # (K, nV, L): what the stage was given

    def _windowed_update(self, XB, XD, d, mu, ranks, reg):
        z = self._zone_order[0]                    # the parent pops it
        w, lam, status = super()._windowed_update(XB, XD, d, mu, ranks, reg)
        if self.effort_limit is None:
            return w, lam, status
        self.w_unlimited[z] = w
        w, self.effort[z], self.effort_rank[z], self.effort_gain[z], self.effort_src[z] = limit_effort(w, self.effort_limit[z], ranks)
        return w, lam, status


class EffortSubbandOracle(_EffortLimit, _SpanRule, WindowedSubbandOracle):
    def __init__(self, *args, effort_limit=None, mu_profile=None, rank_cap=None, floor_db=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_span(mu_profile, rank_cap, floor_db)
        self._init_effort(effort_limit)


class EffortForgettingOracle(_EffortLimit, _SpanRule, ForgettingSubbandOracle):
    def __init__(self, *args, effort_limit=None, mu_profile=None, rank_cap=None, floor_db=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_span(mu_profile, rank_cap, floor_db)
        self._init_effort(effort_limit)


class EffortConstrainedOracle(_Projection, _EffortLimit, _SpanRule, WindowedSubbandOracle):
    def __init__(self, *args, filter_taps, effort_limit=None, mu_profile=None, rank_cap=None, floor_db=None, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_span(mu_profile, rank_cap, floor_db)
        self._init_effort(effort_limit)
        self._init_projection(filter_taps)

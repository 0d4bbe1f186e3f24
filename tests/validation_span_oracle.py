"""Test helper (not collected): the subband oracles with the rank choice by the contrast at validation microphones.

With rv_z (Pv, L, Mv) the validation responses of zone z and N the block size, in NumPy float64:

    G_z[k, m, l]  = sum_j rv_z[j, l, m] exp(-2 pi i j k / N),  k = 0 .. N/2                                   (`transfer`)
    bright[k, t]  = sum_m |sum_l G_own[k, m, l] W[k, t, l]|^2,  dark likewise with G_other                    (`energies`)
    slot t' is admissible if both energies are finite and bright >= phi dark
    src[t] = the largest admissible t' <= t; where there is none, the running best of the slots t' <= t with finite energies (the
             scan goes up from slot 0 and takes t' when better(t', best): t' is not 0/0 and best is, or neither is and
             bright_t' dark_best > bright_best dark_t'); -1 where no slot t' <= t has finite energies; with phi = 0 ("no floor")
             t itself, -1 where its energies are not finite                                                    (`decide`)
    slot t becomes a copy of slot src[t]                                                                       (`choose`)

`_ValidationSpan` puts it where the windowed helper intercepts oracle.subband.update, behind the span (span_oracle._SpanRule) and
ahead of the effort limit (effort_oracle._EffortLimit) and the projection (constraint_oracle._Projection).  With no floor set the
helpers call their parents and are equal to them bit for bit."""
import numpy as np

from constraint_oracle import _Projection
from effort_oracle import _EffortLimit
from forgetting_oracle import ForgettingSubbandOracle
from span_oracle import _SpanRule
from windowed_oracle import WindowedSubbandOracle


def transfer(rv, N):
    """rv (Pv, L, Mv) real -> G (N/2 + 1, Mv, L) complex128: the direct sum, term by term."""
    rv = np.asarray(rv, dtype=np.float64)
    Pv = rv.shape[0]
    k = np.arange(N // 2 + 1)
    # the phase of tap j in bin k from the reduced product j k mod N: exact integers, so a long response loses nothing
    ph = np.exp(-2j * np.pi * ((np.arange(Pv)[:, None] * k[None, :]) % N) / N)          # (Pv, K)
    return np.einsum("jlm,jk->kml", rv, ph)


def energies(G_B, G_D, W):
    """G_B, G_D (K, Mv, L), W (K, nV, L) -> bright, dark (K, nV) float64"""
    W = np.asarray(W).astype(np.complex128)
    pb = np.einsum("kml,ktl->ktm", np.asarray(G_B, dtype=np.complex128), W)
    pd = np.einsum("kml,ktl->ktm", np.asarray(G_D, dtype=np.complex128), W)
    return (pb.real ** 2 + pb.imag ** 2).sum(-1), (pd.real ** 2 + pd.imag ** 2).sum(-1)


def energy_scale(G_B, G_D, W):
    """S = sum_m (sum_l |G| |W|)^2 of both banks, (K, nV): what the rounding errors of `energies` are proportional to"""
    aw = np.abs(np.asarray(W).astype(np.complex128))
    sb = np.einsum("kml,ktl->ktm", np.abs(G_B), aw)
    sd = np.einsum("kml,ktl->ktm", np.abs(G_D), aw)
    return (sb ** 2).sum(-1), (sd ** 2).sum(-1)


def _better(b1, d1, b2, d2):
    n1, n2 = b1 != 0.0 or d1 != 0.0, b2 != 0.0 or d2 != 0.0
    if n1 != n2:
        return n1
    if not n1:
        return False
    with np.errstate(over="ignore"):
        return bool(np.float64(b1) * np.float64(d2) > np.float64(b2) * np.float64(d1))


def decide(bright, dark, phi):
    """bright, dark (K, nV), phi a float or (K,) -> (src (K, nV) int32, the source slot of every slot, -1 where it is left as it
    is; top (K,) int32 = src of the top slot + 1, the rank of its source when the ranks are 1 .. nV, 0 where it has none)."""
    bright, dark = np.asarray(bright, dtype=np.float64), np.asarray(dark, dtype=np.float64)
    K, nV = bright.shape
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (K,))
    src = np.full((K, nV), -1, dtype=np.int32)
    fin = np.isfinite(bright) & np.isfinite(dark)
    for k in range(K):
        last = best = -1
        for t in range(nV):
            if fin[k, t]:
                with np.errstate(invalid="ignore", over="ignore"):
                    if bright[k, t] >= phi[k] * dark[k, t]:
                        last = t
                if best < 0 or _better(bright[k, t], dark[k, t], bright[k, best], dark[k, best]):
                    best = t
            if phi[k] == 0.0:
                src[k, t] = t if fin[k, t] else -1
            else:
                src[k, t] = last if last >= 0 else best
    return src, (src[:, -1] + 1).astype(np.int32)


def choose(W, src):
    """W (K, nV, L) with every slot replaced by its source"""
    out = W.copy()
    for k, t in zip(*np.nonzero((src >= 0) & (src != np.arange(W.shape[1])))):
        out[k, t] = W[k, src[k, t]]
    return out


def validation_span(W, G_B, G_D, phi):
    """-> (W', bright, dark, src, top)"""
    bright, dark = energies(G_B, G_D, W)
    src, top = decide(bright, dark, phi)
    return choose(np.asarray(W), src), bright, dark, src, top


class _ValidationSpan:
    """Mixin in front of the span rule (and behind the effort limit): attribute validation_floor ((2, K) linear phi, or None) may
    be reassigned between hops, like the object's under test."""

    def _init_validation(self, rv_A, rv_B, validation_floor):
        K = self.N // 2 + 1
        self.validation_floor = None if validation_floor is None else np.broadcast_to(np.asarray(validation_floor, dtype=np.float64), (2, K))
        self.validation_G = None if rv_A is None else (transfer(rv_A, self.N), transfer(rv_B, self.N))
        self.validation_bright = [None, None]
        self.validation_dark = [None, None]
        self.validation_src = [None, None]
        self.validation_rank = [None, None]
        self.w_unchosen = [None, None]             # (K, nV, L): what the stage was given

    def _windowed_update(self, XB, XD, d, mu, ranks, reg):
        z = self._zone_order[0]                    # the parent pops it
        w, lam, status = super()._windowed_update(XB, XD, d, mu, ranks, reg)
        if self.validation_floor is None:
            return w, lam, status
        self.w_unchosen[z] = w
        G = self.validation_G
        w, self.validation_bright[z], self.validation_dark[z], src, top = validation_span(w, G[z], G[1 - z], self.validation_floor[z])
        self.validation_src[z] = src
        r = np.asarray(ranks, dtype=np.int32)
        self.validation_rank[z] = np.where(top > 0, r[np.maximum(top - 1, 0)], 0).astype(np.int32)
        return w, lam, status


def _init_all(self, kw):
    self._init_span(kw.get("mu_profile"), kw.get("rank_cap"), kw.get("floor_db"))
    self._init_validation(kw.get("rv_A"), kw.get("rv_B"), kw.get("validation_floor"))
    self._init_effort(kw.get("effort_limit"))


_OWN = ("mu_profile", "rank_cap", "floor_db", "rv_A", "rv_B", "validation_floor", "effort_limit")


def _split(kwargs):
    return {k: kwargs.pop(k) for k in _OWN if k in kwargs}


class ValidationSubbandOracle(_EffortLimit, _ValidationSpan, _SpanRule, WindowedSubbandOracle):
    def __init__(self, *args, **kwargs):
        own = _split(kwargs)
        super().__init__(*args, **kwargs)
        _init_all(self, own)


class ValidationForgettingOracle(_EffortLimit, _ValidationSpan, _SpanRule, ForgettingSubbandOracle):
    def __init__(self, *args, **kwargs):
        own = _split(kwargs)
        super().__init__(*args, **kwargs)
        _init_all(self, own)


class ValidationConstrainedOracle(_Projection, _EffortLimit, _ValidationSpan, _SpanRule, WindowedSubbandOracle):
    def __init__(self, *args, filter_taps, **kwargs):
        own = _split(kwargs)
        super().__init__(*args, **kwargs)
        _init_all(self, own)
        self._init_projection(filter_taps)

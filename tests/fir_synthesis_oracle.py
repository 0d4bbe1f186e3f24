"""Test helper (not collected): the FIR synthesis of a constrained subband stream (apvast(..., synthesis="fir")) in float64 NumPy.

For hop h, sample t = 0..H-1, n = h H + t and a_t = (t + 1) / H,

    y[v][n, l] = (1 - a_t) sum_{j < J} g_prev[v, j, l] x[n - j]  +  a_t sum_{j < J} g_cur[v, j, l] x[n - j]

`fir_reference` is that for one hop; `FirStreamReference` carries the J - 1 samples of history and the previous hop's taps from hop
to hop and returns a hop's outputs in the shape process_input_buffers returns them, target paths (pure delays) included."""
import numpy as np


def fir_reference(x, taps_prev, taps_cur, H):
    """x (J - 1 + H,): the J - 1 samples in front of the hop, then the hop; taps_* (nV, J, L).  Returns (y, S), both (nV, H, L):
    the definition and the magnitude sum S = sum |g_prev| |x| + sum |g_cur| |x| that scales the rounding error of any evaluation."""
    x = np.asarray(x, dtype=np.float64).ravel()
    gp, gc = np.asarray(taps_prev, dtype=np.float64), np.asarray(taps_cur, dtype=np.float64)
    J, H = gp.shape[1], int(H)
    assert gp.shape == gc.shape and x.size == J - 1 + H
    T = x[(J - 1) + np.arange(H)[:, None] - np.arange(J)[None, :]]            # (H, J): T[t, j] = x[n - j]
    a = ((np.arange(H) + 1) / H)[None, :, None]
    y = (1 - a) * np.einsum("tj,vjl->vtl", T, gp) + a * np.einsum("tj,vjl->vtl", T, gc)
    S = np.einsum("tj,vjl->vtl", np.abs(T), np.abs(gp)) + np.einsum("tj,vjl->vtl", np.abs(T), np.abs(gc))
    return y, S


class FirStreamReference:
    """The synthesis of a whole stream: zero history and zero taps before the first hop."""

    def __init__(self, J, H, L, V, delay, ref, run_A=True, run_B=True):
        self.J, self.H, self.L, self.V, self.delay, self.ref = J, H, L, V, delay, ref
        self.run = (run_A, run_B)
        self.hist = np.zeros((2, J - 1))
        self.prev = [np.zeros((V, J, L)), np.zeros((V, J, L))]

    def hop(self, x_A, x_B, taps):
        """x_A, x_B (H,): the hop as the device holds it; taps: per zone program the (V, J, L) taps after this hop (None for a
        program that does not run).  Returns (outputs, S): outputs = (A, B, A_t, B_t) like process_input_buffers (lists over the
        ranks of (H, L) arrays, None for a program that does not run), S = (S_A, S_B) the matching magnitude sums."""
        J, H, L = self.J, self.H, self.L
        xw = [np.concatenate([self.hist[g], np.asarray(x, dtype=np.float64).ravel()]) for g, x in enumerate((x_A, x_B))]
        out, S = [], []
        for z in range(2):
            if not self.run[z]:
                out.append(None)
                S.append(None)
                continue
            cur = np.asarray(taps[z], dtype=np.float64)
            y, s = fir_reference(xw[z], self.prev[z], cur, H)
            out.append(list(y))
            S.append(s)
            self.prev[z] = cur.copy()
        for g in range(2):
            t = np.zeros((H, L))
            t[:, self.ref] = xw[g][J - 1 - self.delay: J - 1 - self.delay + H]
            out.append([t] * self.V)
            self.hist[g] = xw[g][H:]
        return tuple(out), tuple(S)

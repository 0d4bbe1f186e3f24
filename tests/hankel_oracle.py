"""Plain reference of the broadband Hankel statistics (apvast.py:329-364, apVast.m:410-447, vast.m:46-70), for
tests/test_gpu_hankel_statistics.py; tests/test_cpu_hankel_oracle.py pins it to the oracles restated from the reference.

TEST INFRASTRUCTURE ONLY.  It forms every data matrix outright and multiplies it with its transpose: no displacement
structure, no tiles, no chunks -- nothing it could share a mistake with in csrc/kernels_bb.hip.

Layout (that of the kernels): stats [njobs][M L][S], row m L + s the ring of loudspeaker s at microphone m; the ring's logical
sample t lives at (t + off) mod S.  tstats [M][S] pairs with job 0.
"""
import numpy as np

LD = np.longdouble


def unwrapped(row, off, J, skip):
    """The sequence g the data matrix is made of: the ring read from `off`, sample J dropped when `skip` is set
    (scipy.linalg.toeplitz ignores the first entry of its row argument, apvast.py:334-338)."""
    g = np.roll(row, -off)
    return np.concatenate([g[:J], g[J + 1:]]) if skip else g


def data_matrix(rows, J, off, skip, ncols):
    """Y_m [(s, i)][c] = g_{s,m}[J - 1 - i + c] for the L rings `rows` (L, S) of one microphone: (J L, ncols)."""
    out = []
    for row in rows:
        g = unwrapped(row, off, J, skip)
        assert J - 1 + ncols <= g.size, "the last window runs past the sequence"
        W = np.lib.stride_tricks.sliding_window_view(g, ncols)          # W[u] = g[u : u + ncols]
        out.append(W[J - 1::-1])                                       # J rows: row i starts at u = J - 1 - i
    return np.concatenate(out, axis=0)


def reference(stats, tstats, J, L, M, off, skip, ncols, toff, dtype=np.float64):
    """R (njobs, n, n) = sum_m Y_m Y_m^T per job and r (n,) = sum_m Y_m d_m for job 0 (None without tstats),
    d_m[c] = unwrapped tstats_m[toff + c]; everything in `dtype` (float64 or long double)."""
    st = np.asarray(stats, dtype=dtype)
    if st.ndim == 2:
        st = st[None]
    njobs, rows, S = st.shape
    assert rows == M * L
    n = J * L
    R = np.zeros((njobs, n, n), dtype=dtype)
    r = None
    if tstats is not None:
        ts = np.asarray(tstats, dtype=dtype)
        assert ts.shape == (M, S) and toff + ncols <= S
        r = np.zeros(n, dtype=dtype)
    for j in range(njobs):
        for m in range(M):
            Y = np.ascontiguousarray(data_matrix(st[j, m * L:(m + 1) * L], J, off, skip, ncols))
            R[j] += Y @ Y.T
            if j == 0 and r is not None:
                r += Y @ np.roll(ts[m], -off)[toff:toff + ncols]
    return R, r


def pack_buffers(buf, off=0):
    """The oracles' statistics buffers (S, L, M) -> rings [M L][S] written so that sample 0 sits at `off`."""
    S, L, M = buf.shape
    return np.roll(np.ascontiguousarray(buf.transpose(2, 1, 0)).reshape(M * L, S), off, axis=1)


def pack_static(g, J, S):
    """apv_vast_static's packing of impulse responses g (Nm, P, L) into rings [Nm L][S]: g'[u] = g[u - (J - 1)], so that the
    contiguous data matrix (skip = 0, off = 0) holds vast.m's regressors y[s J + j](t) = g_s[t - 1 - j]."""
    Nm, P, L = g.shape
    out = np.zeros((Nm * L, S))
    q = min(P, S - (J - 1))
    out[:, J - 1:J - 1 + q] = g[:, :q, :].transpose(0, 2, 1).reshape(Nm * L, q)
    return out


def pack_static_target(gB, J, S, delay, ref):
    """The target ring of apv_vast_static [Nb][S]: the reference loudspeaker's response delayed by `delay`, from sample J on
    (vast.m:59; read with toff = J)."""
    Nb, P, _ = gB.shape
    out = np.zeros((Nb, S))
    q = min(P, S - J)
    if q > delay:
        out[:, J + delay:J + q] = gB[:, :q - delay, ref]
    return out

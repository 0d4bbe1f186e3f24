"""Writes tests/golden/g9_live_update.npz: the reference class at cfg1 with its responses and mu reassigned between hops.

    python tools/make_golden_live_update.py            (needs the reference project; APVAST_REFERENCE points at it)

Schedule over 10 hops: rir_A and rir_B replaced after hop 3 by a second set derived below, target_rir_A replaced after hop 5,
mu = 0.25 after hop 6 (the reference reads all of them on every hop: apvast.py:161, 167-193).  Recorded: the inputs, the
second response set, the new target, the outputs of ranks 1 and 8 (A and B; A_t and B_t once, they do not depend on the rank)
and the last hop's w_A / w_B.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import CFG1, OUT, cfg1_rirs, load_reference, make_ref_obj  # noqa: E402

HOPS = 10
RANKS = (0, 7)                  # ranks 1 and 8
SCHEDULE = dict(rirs_after=3, target_after=5, mu_after=6, mu=0.25)


def second_rirs(rirA, rirB):
    """The room after the listener moved: each zone's responses delayed by a few samples, scaled and mixed with the other
    zone's, rounded to float32 values so that the fixture holds them exactly in half the space."""
    a2 = 0.8 * np.roll(rirA, 3, axis=0) + 0.2 * rirB
    b2 = 0.7 * np.roll(rirB, 5, axis=0) - 0.1 * rirA
    a2[:3] = 0.0
    b2[:5] = 0.0
    return a2.astype(np.float32).astype(np.float64), b2.astype(np.float32).astype(np.float64)


def second_target(rirA2):
    """target_rir_A built as apvast.py:100-112 would from the second set, at reference loudspeaker 2 instead of 0."""
    P, d = rirA2.shape[0], CFG1["modeling_delay"]
    t = np.zeros((P, rirA2.shape[2]))
    t[d:] = rirA2[: P - d, 2, :]
    return t


def run(ref):
    rirA, rirB = cfg1_rirs()
    rirA2, rirB2 = second_rirs(rirA, rirB)
    tA2 = second_target(rirA2)
    ap = make_ref_obj(ref, rirA, rirB, seed=0)
    H = CFG1["hop_size"]
    x = np.random.default_rng(9).standard_normal((2, HOPS * H))
    L = rirA.shape[1]
    out = np.zeros((HOPS, 2, len(RANKS), H, L))
    out_t = np.zeros((HOPS, 2, H, L))
    for h in range(HOPS):
        if h == SCHEDULE["rirs_after"] + 1:
            ap.rir_A, ap.rir_B = rirA2.copy(), rirB2.copy()
        if h == SCHEDULE["target_after"] + 1:
            ap.target_rir_A = tA2.copy()
        if h == SCHEDULE["mu_after"] + 1:
            ap.mu = SCHEDULE["mu"]
        o = ap.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        for z in range(2):
            for t, i in enumerate(RANKS):
                out[h, z, t] = o[z][i]
            out_t[h, z] = o[2 + z][0]
    np.savez_compressed(os.path.join(OUT, "g9_live_update.npz"), x=x, rirA2=rirA2.astype(np.float32),
                        rirB2=rirB2.astype(np.float32), target_rir_A2=tA2.astype(np.float32), outputs=out, outputs_t=out_t,
                        ranks=np.array(RANKS), w_A=ap.w_A[:, :, 0], w_B=ap.w_B[:, :, 0],
                        schedule=np.array([SCHEDULE["rirs_after"], SCHEDULE["target_after"], SCHEDULE["mu_after"]]),
                        mu2=np.array(SCHEDULE["mu"]))


if __name__ == "__main__":
    run(load_reference())
    path = os.path.join(OUT, "g9_live_update.npz")
    print(path, os.path.getsize(path), "bytes")

"""Responses and mu reassigned between hops: the CPU oracle against the reference's own numbers (g9_live_update.npz, written by
tools/make_golden_live_update.py from the reference class at cfg1)."""
import numpy as np

from oracle.broadband import BroadbandOracle

CFG1 = dict(block_size=256, filter_length=32, modeling_delay=16, reference_index_A=0, reference_index_B=0,
            number_of_eigenvectors=8, mu=1.0, statistics_buffer_length=512, hop_size=128)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_broadband_oracle_follows_reassignments(golden):
    g, rirs = golden("g9_live_update"), golden("rirs_cfg1")
    p = CFG1
    np.random.seed(0)                           # the reference's response buffers start from the global RNG (apvast.py:124-129)
    o = BroadbandOracle(p["block_size"], rirs["rirA"], rirs["rirB"], p["filter_length"], p["modeling_delay"],
                        p["reference_index_A"], p["reference_index_B"], p["number_of_eigenvectors"], p["mu"],
                        p["statistics_buffer_length"], hop_size=p["hop_size"], perceptual=False)
    H = p["hop_size"]
    x = g["x"]
    after_rirs, after_target, after_mu = (int(v) for v in g["schedule"])
    ranks = list(g["ranks"])
    for h in range(x.shape[1] // H):
        if h == after_rirs + 1:
            o.rir = (g["rirA2"].astype(np.float64), g["rirB2"].astype(np.float64))
        if h == after_target + 1:
            o.target_rir[0] = g["target_rir_A2"].astype(np.float64)
        if h == after_mu + 1:
            o.mu = float(g["mu2"])
        out = o.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
        for z in range(2):
            assert _rel(out[z][ranks], g["outputs"][h, z]) < 1e-11, (h, z)
            assert _rel(out[2 + z][0], g["outputs_t"][h, z]) < 1e-11, (h, z)
    assert _rel(np.asarray(o.w_A).reshape(g["w_A"].shape), g["w_A"]) < 1e-9
    assert _rel(np.asarray(o.w_B).reshape(g["w_B"].shape), g["w_B"]) < 1e-9


def test_fixture_schedule_changes_the_outputs(golden):
    """The updates of the fixture are not no-ops: ignoring them (the stream before this feature) departs from the reference."""
    g, rirs = golden("g9_live_update"), golden("rirs_cfg1")
    p = CFG1
    np.random.seed(0)
    o = BroadbandOracle(p["block_size"], rirs["rirA"], rirs["rirB"], p["filter_length"], p["modeling_delay"],
                        p["reference_index_A"], p["reference_index_B"], p["number_of_eigenvectors"], p["mu"],
                        p["statistics_buffer_length"], hop_size=p["hop_size"], perceptual=False)
    H, x = p["hop_size"], g["x"]
    for h in range(x.shape[1] // H):
        out = o.process_input_buffers(x[0, h * H:(h + 1) * H], x[1, h * H:(h + 1) * H])
    assert _rel(out[0][list(g["ranks"])], g["outputs"][-1, 0]) > 1e-3

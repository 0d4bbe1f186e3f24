"""csrc/state_layout.h -- the ring rotation and the regrouping of grouped spectra that the state getters and setters of both
streams share -- against NumPy.  tests/host/state_layout_main.cpp is built with the host compiler and the address and
undefined-behaviour sanitizers and run as a program of its own: its buffers have exactly the sizes the functions are told.
Also the table behind get_state / set_state of class apvast against the key tuples of the class, on stand-in objects."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN = 5
DTYPES = {4: np.float32, 8: np.float64, 16: np.complex128}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("state_layout") / "state_layout_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "ap_vast_unofficial_amd", "csrc"), os.path.join(ROOT, "tests", "host", "state_layout_main.cpp"),
                    "-o", exe], check=True)

    def run(what, a, b, c, x):
        r = subprocess.run([exe, what, str(a), str(b), str(c), str(x.dtype.itemsize)], input=x.tobytes(), capture_output=True)
        assert r.returncode == 0, (what, a, b, c, r.returncode, r.stderr.decode()[-2000:])
        return np.frombuffer(r.stdout, dtype=x.dtype)
    return run


def values(shape, esz):
    x = np.arange(1, int(np.prod(shape)) + 1, dtype=np.float64).reshape(shape)
    return (x + 0.5j * x).astype(DTYPES[esz]) if esz == 16 else x.astype(DTYPES[esz])


@pytest.mark.parametrize("esz", [4, 8, 16])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("off", [0, 1, LEN - 1])
def test_ring_rotation(program, off, rows, esz):
    """logical element t of a row stands at physical index (t + off) mod len"""
    x = values((rows, LEN), esz)
    got = program("to_logical", rows, LEN, off, x).reshape(rows, LEN)
    assert np.array_equal(got, np.roll(x, -off, axis=1))
    assert np.array_equal(got, x[:, (np.arange(LEN) + off) % LEN])
    back = program("from_logical", rows, LEN, off, x).reshape(rows, LEN)
    assert np.array_equal(back, np.roll(x, off, axis=1))
    assert np.array_equal(program("round_trip", rows, LEN, off, x).reshape(rows, LEN), x)


def test_state_table_of_the_class_agrees_with_its_key_tuples():
    """apvast._STATE_ROWS against the literal tuples other tests read: the same keys, each once, the correction keys last, and for
    a plain object of either mode exactly the mode's base keys and the correction keys accepted, the base keys reported"""
    from types import SimpleNamespace
    from ap_vast_unofficial_amd.apvast import apvast as A
    keys = [r.key for r in A._STATE_ROWS]
    features = A._WIN_STATE + A._FORGET_STATE + A._FIR_STATE + A._EVAL_STATE + A._EVALSPEC_STATE + A._EVALDETECT_STATE
    assert len(keys) == len(set(keys)) and set(keys) == set(A._BB_STATE + features + A._LIVE_STATE)
    assert set(A._SB_STATE) <= set(A._BB_STATE) and tuple(keys[-2:]) == A._LIVE_STATE
    assert keys.index("statistics_window") < keys.index("statistics_window_fill")
    for mode, base in (("subband", A._SB_STATE), ("broadband", A._BB_STATE)):
        plain = SimpleNamespace(mode=mode, statistics_hops=1, statistics_forgetting=None, synthesis="wola", _evaluation=None,
                                _evaluation_spectra=False, _evaluation_detectability=False, _live_applied=False)
        assert {r.key for r in A._STATE_ROWS if r.accepts(plain)} == set(base + A._LIVE_STATE)
        assert {r.key for r in A._STATE_ROWS if (r.reports or r.accepts)(plain)} == set(base)


@pytest.mark.parametrize("esz", [8, 16])
def test_grouped_to_bin_major(program, esz):
    """K = 17 bins in groups of 8 (three groups, the last one padded), C = 3 channels: element (k, c) of the bin-major array is
    element (k // g) g C + c g + k % g of the grouped one"""
    K, C, g = 17, 3, 8
    Kp = -(-K // g) * g
    x = values((Kp * C,), esz)
    k, c = np.meshgrid(np.arange(K), np.arange(C), indexing="ij")
    want = x[(k // g) * g * C + c * g + k % g]
    assert np.array_equal(program("bin_major", K, C, g, x).reshape(K, C), want)
    # the same through the layout's own axes: [Kp / g][C][g] -> [Kp][C], the first K bins
    assert np.array_equal(want, x.reshape(Kp // g, C, g).transpose(0, 2, 1).reshape(Kp, C)[:K])

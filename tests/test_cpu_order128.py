"""CPU checks of the order-128 subband surface: the size constants of the header and the ctypes binding agree."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_srcs_matches_header_and_max_n_unchanged():
    from ap_vast_unofficial_amd import _capi
    text = open(os.path.join(ROOT, "include", "apvast_hip.h")).read()
    assert int(re.search(r"#define APV_MAX_SRCS (\d+)", text).group(1)) == _capi.MAX_SRCS == 128
    assert int(re.search(r"#define APV_MAX_N (\d+)", text).group(1)) == _capi.MAX_N == 64
    assert "apv_set_rank_list" in _capi.EXPORTS
    assert re.search(r"int\s+apv_set_rank_list\(apv_handle\* h, int32_t n, const int32_t\* ranks\);", text)


def test_engine_rank_bound_follows_order():
    """More than 64 ranks are an argument error below order 65 (before any device is touched) and allowed above it."""
    import pytest
    from ap_vast_unofficial_amd import _capi
    with pytest.raises(ValueError, match="between 1 and 64 ranks"):
        _capi.Engine(4, 64, 70, ranks=range(1, 66))
    with pytest.raises(ValueError, match="between 1 and n_srcs = 96 ranks"):
        _capi.Engine(4, 96, 100, ranks=range(1, 98))

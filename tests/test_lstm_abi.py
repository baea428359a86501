"""CPU: the argument checks of csrc/lstm.hip's entry points (include/sar_hip.h, TemporalSampler) run before anything is launched,
so they answer on a machine without a GPU: SAR_E_ARG / SAR_E_UNSUP with the entry point named in sar_last_error_string()."""
import ctypes

import pytest

from sar_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _rejected(lib, rc, want, name):
    assert rc == want, "%s returned %d, expected %d" % (name, rc, want)
    assert name.encode() in lib.sar_last_error_string()


def test_null_operands_are_argument_errors(lib):
    _rejected(lib, lib.sar_lstm_fwd_f32(None, 8, None, None, 8, None, 0, None, 0, 4, 2, 4, None), _lib.SAR_E_ARG, "sar_lstm_fwd_f32")
    _rejected(lib, lib.sar_lstm_bwd_f32(None, 8, None, 8, None, 8, None, None, 8, 4, 2, 4, None), _lib.SAR_E_ARG, "sar_lstm_bwd_f32")
    _rejected(lib, lib.sar_topk_desc_f32(None, 4, 1, 2, 4, 2, None, None, None, None), _lib.SAR_E_ARG, "sar_topk_desc_f32")
    _rejected(lib, lib.sar_frame_gather_f32(None, None, None, None, 1, 1, 4, 1, 2, None), _lib.SAR_E_ARG, "sar_frame_gather_f32")
    _rejected(lib, lib.sar_frame_gather_bwd_f32(None, None, None, None, None, None, 4, 1, None, 1, 1, 4, 1, 2, None), _lib.SAR_E_ARG,
              "sar_frame_gather_bwd_f32")
    _rejected(lib, lib.sar_lstm_pack_f32(None, None, 8, 2, 1, 4, 1, None), _lib.SAR_E_ARG, "sar_lstm_pack_f32")
    _rejected(lib, lib.sar_lstm_unpack_add_f32(None, 8, None, 2, 1, 4, 1, None), _lib.SAR_E_ARG, "sar_lstm_unpack_add_f32")


def test_limits_are_checked_before_any_launch(lib):
    """host buffers stand in for device pointers: a rejected call dereferences nothing"""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    # u > 128: not built; T N columns need ld >= T N; gates and c come together
    _rejected(lib, lib.sar_lstm_fwd_f32(p, 8, p, p, 8, p, 8, p, 8, 129, 2, 4, None), _lib.SAR_E_UNSUP, "sar_lstm_fwd_f32")
    _rejected(lib, lib.sar_lstm_bwd_f32(p, 8, p, 8, p, 8, p, p, 8, 129, 2, 4, None), _lib.SAR_E_UNSUP, "sar_lstm_bwd_f32")
    _rejected(lib, lib.sar_lstm_fwd_f32(p, 7, p, p, 8, p, 8, p, 8, 4, 2, 4, None), _lib.SAR_E_ARG, "sar_lstm_fwd_f32")
    _rejected(lib, lib.sar_lstm_fwd_f32(p, 8, p, p, 8, p, 8, None, 8, 4, 2, 4, None), _lib.SAR_E_ARG, "sar_lstm_fwd_f32")
    _rejected(lib, lib.sar_lstm_fwd_f32(p, 1 << 31, p, p, 1 << 31, None, 0, None, 0, 4, 1 << 16, 1 << 15, None), _lib.SAR_E_ARG,
              "sar_lstm_fwd_f32")
    _rejected(lib, lib.sar_lstm_bwd_f32(p, 8, p, 8, p, 8, p, p, 7, 4, 2, 4, None), _lib.SAR_E_ARG, "sar_lstm_bwd_f32")
    _rejected(lib, lib.sar_lstm_fwd_f32(p, 8, p, p, 8, None, 0, None, 0, 0, 2, 4, None), _lib.SAR_E_ARG, "sar_lstm_fwd_f32")
    # 1 <= k <= T <= 2048
    _rejected(lib, lib.sar_topk_desc_f32(p, 4, 1, 2, 4, 5, p, p, p, None), _lib.SAR_E_ARG, "sar_topk_desc_f32")
    _rejected(lib, lib.sar_topk_desc_f32(p, 4, 1, 2, 4, 0, p, p, p, None), _lib.SAR_E_ARG, "sar_topk_desc_f32")
    _rejected(lib, lib.sar_topk_desc_f32(p, 2049, 1, 2, 2049, 7, p, p, p, None), _lib.SAR_E_UNSUP, "sar_topk_desc_f32")
    _rejected(lib, lib.sar_frame_gather_f32(p, p, p, p, 1, 1, 4, 1, 5, None), _lib.SAR_E_ARG, "sar_frame_gather_f32")
    _rejected(lib, lib.sar_frame_gather_bwd_f32(p, p, p, p, p, p, 4, 1, None, 1, 1, 4, 1, 5, None), _lib.SAR_E_ARG,
              "sar_frame_gather_bwd_f32")
    _rejected(lib, lib.sar_lstm_pack_f32(p, p, 7, 2, 1, 4, 1, None), _lib.SAR_E_ARG, "sar_lstm_pack_f32")
    _rejected(lib, lib.sar_lstm_unpack_add_f32(p, 7, p, 2, 1, 4, 1, None), _lib.SAR_E_ARG, "sar_lstm_unpack_add_f32")

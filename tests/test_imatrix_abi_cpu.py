"""The C ABI of the importance matrix's column-sum tap and the weighted quantiser, checked without a card: declared in include/rca.h, exported by the
library, bound in _native; and what rca_quantize_rows_w refuses before any HIP call."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMATRIX = ("rca_lm_imatrix_rows_tap",)


def _lib():
    from realtime_codec_agent_amd import _native
    if _native.needs_build():
        _native.build()
    return _native, _native.lib()


def test_header_declares_library_exports_and_native_binds_the_calls():
    """without the feature this fails (and with it every GPU test of test_imatrix_gpu.py)"""
    N, lib = _lib()
    header = open(os.path.join(ROOT, "include", "rca.h")).read()
    assert re.search(r"\bint\s+rca_lm_imatrix_rows_tap\s*\(", header)
    assert re.search(r"\bint\s+rca_quantize_rows_w\s*\([^)]*const\s+float\s*\*\s*col_weights\s*,\s*void\s*\*\s*blocks_host", header)
    for sym in IMATRIX + ("rca_quantize_rows_w",):
        assert sym in N.ABI_SYMBOLS, sym
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes is not None and getattr(lib, sym).restype is ctypes.c_int, sym
    assert len(lib.rca_quantize_rows_w.argtypes) == len(lib.rca_quantize_rows.argtypes) + 1
    # null handles are refused before any HIP call (this machine may have no GPU at all)
    assert lib.rca_lm_imatrix_rows_tap(None, None, None, 1, 256, 1, None) == -1 and b"null" in lib.rca_last_error()


def test_quantize_rows_w_refuses_bad_arguments_before_any_hip_call():
    N, lib = _lib()
    w = np.zeros((2, 256), np.float32)
    qw = np.ones(256, np.float32)
    out = np.full(2 * 144, 0xA5, np.uint8)

    def call(src=w, rule=1, weights=qw, type=N.RCA_Q4_K, nbytes=None):
        return lib.rca_quantize_rows_w(0, src.ctypes.data if src is not None else None, N.RCA_F32, 2, 256, type, rule,
                                       weights.ctypes.data if weights is not None else None, out.ctypes.data, out.nbytes if nbytes is None else nbytes)

    assert call(src=None) == -1 and b"null pointer" in lib.rca_last_error()
    assert call(rule=0) == -1 and b"column weights need rule 1" in lib.rca_last_error()
    for col, v in ((0, -1.0), (200, np.nan), (255, np.inf), (17, -np.inf)):
        bad = qw.copy()
        bad[col] = v
        assert call(weights=bad) == -1
        assert f"the weight of column {col} is negative or not finite".encode() in lib.rca_last_error(), lib.rca_last_error()
    bad = qw.copy()
    bad[3] = np.nan
    assert call(weights=bad, type=N.RCA_Q8_0, nbytes=2 * 8 * 34) == -1 and b"column 3" in lib.rca_last_error()      # checked though Q8_0 ignores them
    assert call(nbytes=7) == -1 and b"blocks_bytes" in lib.rca_last_error()
    assert (out == 0xA5).all()
    # the unweighted entry's own refusals are unchanged
    assert lib.rca_quantize_rows(0, None, N.RCA_F32, 2, 256, N.RCA_Q4_K, 1, out.ctypes.data, out.nbytes) == -1

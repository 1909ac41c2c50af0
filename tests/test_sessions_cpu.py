"""CPU: the sessions section of the C ABI (include/hnet.h) loads and rejects NULL contexts / sessions / pointers with HNET_ERR_INVALID_ARG before any
device work."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def _lib():
    from cuahn_vio_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _capi, _capi.lib()


def test_sessions_calls_reject_null_handles():
    _capi, L = _lib()
    out = ctypes.c_void_p()
    assert L.hnet_create_sessions(None, 4, ctypes.byref(out)) == INVALID
    assert L.hnet_create_sessions(None, 4, None) == INVALID
    assert not out.value
    ids = np.zeros(1, np.int32)
    frame = np.zeros((224, 320), np.uint8)
    mean, cov = np.zeros(8, np.float32), np.zeros(64, np.float32)
    cam = _capi.Camera(1, 480, 640, (ctypes.c_double * 4)(275.0, 275.0, 316.0, 242.0), (ctypes.c_double * 4)(0, 0, 0, 0))
    cid = ctypes.c_int(-1)
    assert L.hnet_sessions_push(None, 1, ids.ctypes.data, frame.ctypes.data, 320, frame.nbytes, None) == INVALID
    assert L.hnet_sessions_push_raw(None, 1, ids.ctypes.data, frame.ctypes.data, 224, 320, 320, frame.nbytes, None) == INVALID
    assert L.hnet_sessions_add_camera(None, ctypes.byref(cam), ctypes.byref(cid)) == INVALID and cid.value == -1
    assert L.hnet_sessions_bind_camera(None, 0, 0) == INVALID
    assert L.hnet_sessions_infer(None, 1, ids.ctypes.data, None, mean.ctypes.data, cov.ctypes.data, None) == INVALID
    assert L.hnet_sessions_set_seq(None, 0, 5) == INVALID
    assert L.hnet_sessions_reset(None, 0) == INVALID
    assert L.hnet_sessions_get_frame(None, 0, 1, frame.ctypes.data) == INVALID
    assert L.hnet_sessions_last_timing(None, ctypes.byref(_capi.Timing())) == INVALID
    assert L.hnet_sessions_image_count(None, 0) == -1
    assert L.hnet_sessions_latest_time(None, 0) == -1.0
    assert L.hnet_sessions_seq(None, 0) == 0
    L.hnet_destroy_sessions(None)                                        # a no-op
    buf = ctypes.c_void_p(1 << 20)                                       # never dereferenced: the NULL context is refused first
    assert L.hnet_infer_batch_seqs_packed_device(None, buf, buf, 0, None, 1, buf, buf, None, None) == INVALID


def test_sessions_section_is_declared_in_the_header():
    _capi, _ = _lib()
    header = open(os.path.join(ROOT, "include", "hnet.h")).read()
    for name in ("hnet_create_sessions", "hnet_sessions_infer", "hnet_sessions_push_raw", "hnet_infer_batch_seqs_packed_device"):
        assert name in header and name in _capi.SYMBOLS

"""pli_search_local_points / pli_search_local_lines: the header declares them, the library exports them, the binding knows them, and
the argument checks answer before any device call (these run on a machine without a GPU)."""
import ctypes as C
import os
import re

import numpy as np

from pli_slam_amd import capi
from pli_slam_amd.frontend import Frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLI_ERR_INVALID = -1


def test_the_header_the_library_and_the_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "pli_frontend.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    for name, nargs in (("pli_search_local_points", 21), ("pli_search_local_lines", 16)):
        assert re.search(r"pli_status\s+%s\s*\(" % name, hdr), name
        assert name in capi._PROTOS and len(capi._PROTOS[name][1]) == nargs, name
        assert hasattr(lib, name), name
    assert hasattr(Frontend, "search_local_points") and hasattr(Frontend, "search_local_lines")
    assert capi.LOCAL_VIEW_DT.itemsize == 32
    assert re.search(r"typedef struct pli_local_view \{[^}]*float proj_x, proj_y, proj_xr, depth, view_cos;\s*int32_t level, in_view, pad;", hdr)


def test_a_null_context_is_refused_before_any_device_call():
    L = capi.lib()
    cam = capi.FuseCamera(435.0, 435.0, 367.0, 252.0, 47.9, 0.0, 752.0, 0.0, 480.0)
    pose = np.zeros(15, np.float32)
    lr = np.ones(7, np.float32)
    buf = np.zeros(64, np.uint8)
    n1, n2 = C.c_int32(7), C.c_int32(7)
    p = capi.ptr
    assert L.pli_search_local_points(None, p(buf), p(buf), 0, p(pose), C.byref(cam), 0.5, 1.0, 0, 0.0, 0.8, p(lr), None, None,
                                     None, None, 0, p(buf), p(buf), C.byref(n1), C.byref(n2)) == PLI_ERR_INVALID
    assert L.pli_search_local_lines(None, p(buf), p(buf), p(buf), 0, p(pose), C.byref(cam), None, 0, 0.9, p(buf), p(buf), p(buf),
                                    p(buf), C.byref(n1), C.byref(n2)) == PLI_ERR_INVALID
    assert b"bad argument" in L.pli_last_error()
    # (Negative counts need a live context to be told apart from the NULL one, which answers first; without a device there is none:
    # tests/test_local_map_gpu.py::test_negative_counts_with_a_live_context checks nq, ncur, nl and n2 < 0.)

"""CPU check of calico_covariance_options after control_points took the place of one reserved word: the ctypes mirror keeps
the header's size and the defaults leave the trajectory's blocks off."""
import ctypes as C
import os
import re

import helpers
from calico_amd import _capi


def test_covariance_options_layout_and_defaults():
    import __graft_entry__ as g
    g.build_hip()
    lib = C.CDLL(_capi.hip_library_path())
    assert C.sizeof(_capi.CovarianceOptions) == 32
    assert _capi.CovarianceOptions.control_points.offset == 8
    header = open(os.path.join(helpers.ROOT, "include", "calico_hip.h")).read()
    body = re.search(r"typedef struct calico_covariance_options \{(.*?)\} calico_covariance_options;", header, re.S).group(1)
    assert re.findall(r"(int32_t|double)\s+(\w+)", body) == [("double", "min_relative_pivot"), ("int32_t", "control_points"),
                                                             ("int32_t", "reserved")]
    o = _capi.CovarianceOptions()
    o.control_points = 7
    for i in range(5):
        o.reserved[i] = 7
    lib.calico_default_covariance_options.restype = None
    lib.calico_default_covariance_options(C.byref(o))
    assert o.control_points == 0 and list(o.reserved) == [0] * 5 and o.min_relative_pivot == 1e-12

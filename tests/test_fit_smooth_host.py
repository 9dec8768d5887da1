"""calico_fit_spline_smooth without a GPU: every argument rule returns its code with a message that names the call, before the device
is touched (the device ordinal of these calls does not exist); the defaults are the documented ones; the ctypes structs have the
header's sizes; the header, the binding and the library agree on the two new symbols."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import fit_ref
import helpers
from calico_amd import _capi, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

NO_DEVICE = 10 ** 6
NAME = "calico_fit_spline_smooth"


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class _Call:
    """calico_fit_spline_smooth on fifty samples of a 2.5 s trajectory at a device that does not exist, one argument replaced at a time."""

    def __init__(self, api):
        self.api, self.order = api, 6
        self.knots = fit_ref.uniform_knots(30, self.order)
        self.basis = np.ascontiguousarray(syn.basis_matrices(self.knots, self.order))
        vk = self.knots[self.order - 1:len(self.knots) - self.order + 1]
        self.first, self.last = vk[0], vk[-1]
        self.stamps = np.linspace(self.first, self.last, 50)
        self.data, self.weights, self.ctrl = np.zeros((50, 6)), np.ones((50, 2)), np.full((30, 6), 7.5)
        self.summary = _capi.SplineFitSummary()

    def __call__(self, options=None, **kw):
        a = dict(device=NO_DEVICE, order=self.order, n_knots=len(self.knots), knots=self.knots, basis=self.basis, n=50, stamps=self.stamps,
                 data=self.data, weights=self.weights, ctrl=self.ctrl, summary=C.byref(self.summary))
        a.update(kw)
        st = self.api.fit_spline_smooth(a["device"], a["order"], a["n_knots"], _dp(a["knots"]), _dp(a["basis"]), a["n"], _dp(a["stamps"]),
                                        _dp(a["data"]), _dp(a["weights"]), None if options is None else C.byref(options), _dp(a["ctrl"]), None,
                                        None, a["summary"])
        assert (self.ctrl == 7.5).all()
        return st


def _message(api, st, code, *words):
    assert st == code, (st, code, api.last_error(None).decode())
    msg = api.last_error(None).decode()
    assert msg.startswith(NAME + ": "), msg
    for w in words:
        assert w in msg, (w, msg)


def test_argument_rules_need_no_device(api):
    call = _Call(api)

    def invalid(st, *words):
        _message(api, st, _capi.INVALID_ARGUMENT, *words)
    # shared with calico_fit_spline
    for v in (1, 9):
        invalid(call(order=v), "order must be in [2, 8]")
    for name in ("knots", "basis", "stamps", "data", "ctrl", "summary"):
        invalid(call(**{name: None}), "null")
    invalid(call(n=0), "n must be > 0")
    unsorted = call.stamps.copy()
    unsorted[10] = unsorted[8]
    invalid(call(stamps=unsorted), "sample stamps are not sorted", "sample 10")
    off = call.stamps.copy()
    off[49] = call.last + 1e-9
    invalid(call(stamps=off), "sample stamp 49 lies off the valid knots")
    _message(api, call(n=2 ** 31), _capi.UNIMPLEMENTED, "2^31 - 1 samples")
    # weights
    for bad in (-1.0, np.nan, np.inf):
        w = call.weights.copy()
        w[17, 1] = bad
        invalid(call(weights=w), "weight 1 of sample 17 must be finite and >= 0")
    w = call.weights.copy()
    w[:, 0] = 0.0
    invalid(call(weights=w), "rotation weights: no sample has a weight > 0")
    # options
    o = lambda **kw: _capi.default_spline_fit_options(api, **kw)      # noqa: E731
    for v in (0, 4, -1):
        invalid(call(o(derivative=v)), "derivative must be in [1, 3] at order 6")
    invalid(call(o(derivative=2), order=2, n_knots=len(call.knots) - 8, knots=call.knots[4:-4]), "derivative must be in [1, 1] at order 2")
    for v in (0, -3, 33):
        invalid(call(o(n_lambda=v)), "n_lambda must be in [1, 32]")
    invalid(call(o(lambda_rot=[1e-3, 1e-3])), "lambda_rot must be strictly ascending: entry 1")
    invalid(call(o(lambda_pos=[1e-3, 1e-2, 1e-4], lambda_rot=[1.0, 2.0, 3.0])), "lambda_pos must be strictly ascending: entry 2")
    for bad in (-1e-3, np.nan, np.inf):
        invalid(call(o(lambda_rot=bad)), "lambda_rot[0] must be finite and >= 0")
        invalid(call(o(lambda_pos=[0.0, bad], lambda_rot=[0.0, 1.0])), "lambda_pos[1] must be finite and >= 0")
        invalid(call(o(target_rms_rot=bad)), "target_rms_rot must be finite and >= 0")
        invalid(call(o(target_rms_pos=bad)), "target_rms_pos must be finite and >= 0")
    # the length the on-chip solve cannot hold: UNIMPLEMENTED before the device, one control point fewer reaches it
    for n_ctrl, code, word in ((2219, _capi.UNIMPLEMENTED, "too long"), (2218, _capi.INTERNAL, "no usable HIP device")):
        c = fit_ref.inputs(fit_ref._ragged(6, 1.0, n_ctrl, 20.0))
        ctrl, summary = np.full((n_ctrl, 6), 7.5), _capi.SplineFitSummary()
        st = api.fit_spline_smooth(NO_DEVICE, 6, len(c.knots), _dp(c.knots), _dp(c.basis), len(c.stamps), _dp(c.stamps), _dp(c.data), None, None,
                                   _dp(ctrl), None, None, C.byref(summary))
        _message(api, st, code, word)
        assert (ctrl == 7.5).all()
    # a valid call, lambda 0 and weights of 0 included, reaches the device
    w = call.weights.copy()
    w[::3, 0] = 0.0
    _message(api, call(o(lambda_rot=[0.0, 1.0], lambda_pos=[0.0, 1e-9]), weights=w), _capi.INTERNAL, "no usable HIP device", str(NO_DEVICE))
    _message(api, call(weights=None), _capi.INTERNAL, "no usable HIP device")


def test_defaults_are_the_documented_ones(api):
    o = _capi.default_spline_fit_options(api)
    assert (o.derivative, o.relative, o.n_lambda, o.target_rms_rot, o.target_rms_pos) == (2, 1, 1, 0.0, 0.0)
    assert list(o.lambda_rot) == [1e-3] + [0.0] * 31 and list(o.lambda_pos) == [1e-3] + [0.0] * 31
    o = _capi.default_spline_fit_options(api, lambda_rot=[1e-4, 1e-2], derivative=1)
    assert o.n_lambda == 2 and list(o.lambda_rot)[:3] == [1e-4, 1e-2, 0.0] and o.derivative == 1
    with pytest.raises(TypeError):
        _capi.default_spline_fit_options(api, no_such_field=1)
    assert (_capi.FIT_MAX_LAMBDAS, _capi.FIT_OK, _capi.FIT_NOT_POSITIVE_DEFINITE, _capi.FIT_TARGET_NOT_MET) == (32, 0, 1, 2)


def test_structs_and_symbols_match_the_header(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_spline_fit_options", "fit_spline_smooth"):
        assert re.search(r"\bcalico_%s\s*\(" % name, header) and name in _capi.ABI_SYMBOLS and hasattr(api.lib, "calico_" + name)
    for macro, value in (("CALICO_FIT_MAX_LAMBDAS", 32), ("CALICO_FIT_OK", 0), ("CALICO_FIT_NOT_POSITIVE_DEFINITE", 1), ("CALICO_FIT_TARGET_NOT_MET", 2)):
        assert re.search(r"#define %s %d\b" % (macro, value), header)
    # the header's layouts: 3 int32 (+ 4 bytes of padding), 2 x 32 doubles, 2 doubles; 2 int32, 4 doubles; 2 + 2 int32, 2 int64
    assert C.sizeof(_capi.SplineFitOptions) == 16 + 2 * 32 * 8 + 16 == 544
    assert C.sizeof(_capi.SplineFitRow) == 40 and C.sizeof(_capi.SplineFitSummary) == 32
    assert _capi.SplineFitOptions.lambda_rot.offset == 16 and _capi.SplineFitOptions.target_rms_pos.offset == 536
    for struct, c_name in ((_capi.SplineFitOptions, "calico_spline_fit_options"), (_capi.SplineFitRow, "calico_spline_fit_row"),
                           (_capi.SplineFitSummary, "calico_spline_fit_summary")):
        body = re.search(r"typedef struct \{((?:[^{}]|\{[^{}]*\})*)\} %s;" % c_name, header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.match(r"\s*\w+\s+(\w+)", d).group(1) for d in body.split(";") if d.strip()]
        assert fields == [n.rstrip("_") for n, _ in struct._fields_], (c_name, fields)

"""calico_fit_spline_robust without a GPU: every argument rule returns its code with a message that names the call, before the device
is touched (the device ordinal of these calls does not exist) and with the outputs untouched; the defaults are the documented
ones; the ctypes structs have the header's sizes, offsets and fields; the header, the binding and the library agree on the two
new symbols."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import fit_ref
from calico_amd import _capi, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

NO_DEVICE = 10 ** 6
NAME = "calico_fit_spline_robust"


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class _Call:
    """calico_fit_spline_robust on fifty samples of a 2.5 s trajectory at a device that does not exist, one argument replaced at a time."""

    def __init__(self, api):
        self.api, self.order = api, 6
        self.knots = fit_ref.uniform_knots(30, self.order)
        self.basis = np.ascontiguousarray(syn.basis_matrices(self.knots, self.order))
        vk = self.knots[self.order - 1:len(self.knots) - self.order + 1]
        self.first, self.last = vk[0], vk[-1]
        self.stamps = np.linspace(self.first, self.last, 50)
        self.data, self.weights, self.ctrl = np.zeros((50, 6)), np.ones((50, 2)), np.full((30, 6), 7.5)
        self.u, self.e = np.full((50, 2), 7.5), np.full((50, 2), 7.5)
        self.summary = _capi.SplineRobustSummary()

    def __call__(self, fit=None, robust=None, **kw):
        a = dict(device=NO_DEVICE, order=self.order, n_knots=len(self.knots), knots=self.knots, basis=self.basis, n=50, stamps=self.stamps,
                 data=self.data, weights=self.weights, ctrl=self.ctrl, summary=C.byref(self.summary))
        a.update(kw)
        st = self.api.fit_spline_robust(a["device"], a["order"], a["n_knots"], _dp(a["knots"]), _dp(a["basis"]), a["n"], _dp(a["stamps"]),
                                        _dp(a["data"]), _dp(a["weights"]), None if fit is None else C.byref(fit),
                                        None if robust is None else C.byref(robust), _dp(a["ctrl"]), _dp(self.u), _dp(self.e), a["summary"])
        assert (self.ctrl == 7.5).all() and (self.u == 7.5).all() and (self.e == 7.5).all()
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
    # everything calico_fit_spline_smooth refuses
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
    for bad in (-1.0, np.nan, np.inf):
        w = call.weights.copy()
        w[17, 1] = bad
        invalid(call(weights=w), "weight 1 of sample 17 must be finite and >= 0")
    w = call.weights.copy()
    w[:, 1] = 0.0
    invalid(call(weights=w), "position weights: no sample has a weight > 0")
    o = lambda **kw: _capi.default_spline_fit_options(api, **kw)      # noqa: E731
    for v in (0, 4):
        invalid(call(o(derivative=v)), "derivative must be in [1, 3] at order 6")
    for bad in (-1e-3, np.nan, np.inf):
        invalid(call(o(lambda_rot=bad)), "lambda_rot[0] must be finite and >= 0")
        invalid(call(o(target_rms_pos=bad)), "target_rms_pos must be finite and >= 0")
    for v in (0, 33):
        invalid(call(o(n_lambda=v)), "n_lambda must be in [1, 32]")
    # the robust fit's own rules
    invalid(call(o(lambda_rot=[1e-3, 1e-2], lambda_pos=[1e-3, 1e-2])), "n_lambda must be 1")
    invalid(call(o(target_rms_rot=0.1)), "target_rms_rot and target_rms_pos must be 0")
    invalid(call(o(target_rms_pos=0.1)), "target_rms_rot and target_rms_pos must be 0")
    r = lambda **kw: _capi.default_spline_robust_options(api, **kw)      # noqa: E731
    for v in (0, 3, -1):
        invalid(call(robust=r(loss=v)), "unknown loss %d" % v)
    for v in (-1, 65):
        invalid(call(robust=r(max_iterations=v)), "max_iterations must be in [0, 64]")
    for field in ("tuning_rot", "tuning_pos", "scale_rot", "scale_pos", "min_scale_rot", "min_scale_pos", "step_tolerance"):
        for bad in (-1e-3, np.nan, np.inf):
            invalid(call(robust=r(**{field: bad})), field + " must be finite and >= 0")
    # the length the on-chip solve cannot hold: UNIMPLEMENTED before the device, one control point fewer reaches it
    for n_ctrl, code, word in ((2219, _capi.UNIMPLEMENTED, "too long"), (2218, _capi.INTERNAL, "no usable HIP device")):
        c = fit_ref.inputs(fit_ref._ragged(6, 1.0, n_ctrl, 20.0))
        ctrl, summary = np.full((n_ctrl, 6), 7.5), _capi.SplineRobustSummary()
        st = api.fit_spline_robust(NO_DEVICE, 6, len(c.knots), _dp(c.knots), _dp(c.basis), len(c.stamps), _dp(c.stamps), _dp(c.data), None, None,
                                   None, _dp(ctrl), None, None, C.byref(summary))
        _message(api, st, code, word)
        assert (ctrl == 7.5).all()
    # valid calls reach the device: the limits of every range, both losses, weights of 0, no weights, no optional output
    w = call.weights.copy()
    w[::3, 0] = 0.0
    for robust in (r(max_iterations=0), r(max_iterations=64, loss=_capi.ROBUST_TUKEY, step_tolerance=0.0), r(scale_rot=1e300, tuning_pos=1.5, min_scale_pos=1e-6)):
        _message(api, call(o(lambda_rot=0.0), robust, weights=w), _capi.INTERNAL, "no usable HIP device", str(NO_DEVICE))
    _message(api, call(weights=None), _capi.INTERNAL, "no usable HIP device")


def test_defaults_are_the_documented_ones(api):
    o = _capi.default_spline_robust_options(api)
    assert (o.loss, o.max_iterations, o.step_tolerance) == (_capi.ROBUST_HUBER, 20, 1e-9)
    assert (o.tuning_rot, o.tuning_pos, o.scale_rot, o.scale_pos, o.min_scale_rot, o.min_scale_pos) == (0.0,) * 6
    o = _capi.default_spline_robust_options(api, loss=_capi.ROBUST_TUKEY, scale_pos=0.25)
    assert (o.loss, o.scale_pos, o.max_iterations) == (2, 0.25, 20)
    with pytest.raises(TypeError):
        _capi.default_spline_robust_options(api, no_such_field=1)
    assert (_capi.FIT_MAX_ITERATIONS, _capi.FIT_SCALE_ZERO, _capi.ROBUST_HUBER, _capi.ROBUST_TUKEY, _capi.FIT_ROBUST_ITERATION_LIMIT) == (3, 4, 1, 2, 64)


def test_structs_and_symbols_match_the_header(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_spline_robust_options", "fit_spline_robust"):
        assert re.search(r"\bcalico_%s\s*\(" % name, header) and name in _capi.ABI_SYMBOLS and hasattr(api.lib, "calico_" + name)
    for macro, value in (("CALICO_FIT_MAX_ITERATIONS", 3), ("CALICO_FIT_SCALE_ZERO", 4), ("CALICO_ROBUST_HUBER", 1), ("CALICO_ROBUST_TUKEY", 2),
                         ("CALICO_FIT_ROBUST_ITERATION_LIMIT", 64)):
        assert re.search(r"#define %s %d\b" % (macro, value), header)
    # the header's layouts: 2 int32, 7 doubles; 3 x 2 int32, 3 x 2 int64, 5 x 2 doubles
    R, S = _capi.SplineRobustOptions, _capi.SplineRobustSummary
    assert C.sizeof(R) == 8 + 7 * 8 == 64 and (R.loss.offset, R.max_iterations.offset, R.tuning_rot.offset, R.step_tolerance.offset) == (0, 4, 8, 56)
    assert C.sizeof(S) == 24 + 48 + 80 == 152
    assert (S.status.offset, S.iterations.offset, S.replaced_pivots.offset, S.n_used.offset, S.n_rejected.offset, S.lambda_.offset,
            S.rss.offset) == (0, 8, 16, 24, 56, 72, 136)
    for struct, c_name in ((R, "calico_spline_robust_options"), (S, "calico_spline_robust_summary")):
        body = re.search(r"typedef struct \{((?:[^{}]|\{[^{}]*\})*)\} %s;" % c_name, header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.match(r"\s*\w+\s+(\w+)", d).group(1) for d in body.split(";") if d.strip()]
        assert fields == [n.rstrip("_") for n, _ in struct._fields_], (c_name, fields)

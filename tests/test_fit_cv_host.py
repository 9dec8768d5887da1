"""calico_fit_spline_cv without a GPU: every argument rule returns its code with a message that names the call, before the device is
touched (the device ordinal of these calls does not exist) and with the outputs untouched; the defaults are the documented ones;
the ctypes structs have the header's sizes, offsets and fields; the header, the binding and the library agree on the two new
symbols."""
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
NAME = "calico_fit_spline_cv"


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


class _Call:
    """calico_fit_spline_cv on fifty samples of a 2.5 s trajectory at a device that does not exist, one argument replaced at a time."""

    def __init__(self, api):
        self.api, self.order = api, 6
        self.knots = fit_ref.uniform_knots(30, self.order)
        self.basis = np.ascontiguousarray(syn.basis_matrices(self.knots, self.order))
        vk = self.knots[self.order - 1:len(self.knots) - self.order + 1]
        self.first, self.last = vk[0], vk[-1]
        self.stamps = np.linspace(self.first, self.last, 50)
        self.data, self.weights, self.ctrl = np.zeros((50, 6)), np.ones((50, 2)), np.full((30, 6), 7.5)
        self.ctrl_all, self.h, self.loo = np.full((32, 30, 6), 7.5), np.full((50, 2), 7.5), np.full((50, 2), 7.5)
        self.rows, self.cv_rows = (_capi.SplineFitRow * 64)(), (_capi.SplineCvRow * 64)()
        for i in range(64):
            self.rows[i].rss = self.cv_rows[i].edf = 7.5
        self.summary = _capi.SplineCvSummary()
        self.summary.chosen[0] = self.summary.chosen[1] = 75

    def __call__(self, fit=None, cv=None, **kw):
        a = dict(device=NO_DEVICE, order=self.order, n_knots=len(self.knots), knots=self.knots, basis=self.basis, n=50, stamps=self.stamps,
                 data=self.data, weights=self.weights, ctrl=self.ctrl, summary=C.byref(self.summary))
        a.update(kw)
        st = self.api.fit_spline_cv(a["device"], a["order"], a["n_knots"], _dp(a["knots"]), _dp(a["basis"]), a["n"], _dp(a["stamps"]),
                                    _dp(a["data"]), _dp(a["weights"]), None if fit is None else C.byref(fit), None if cv is None else C.byref(cv),
                                    _dp(a["ctrl"]), _dp(self.ctrl_all), self.rows, self.cv_rows, _dp(self.h), _dp(self.loo), a["summary"])
        assert (self.ctrl == 7.5).all() and (self.ctrl_all == 7.5).all() and (self.h == 7.5).all() and (self.loo == 7.5).all()
        assert all(self.rows[i].rss == 7.5 and self.cv_rows[i].edf == 7.5 for i in range(64)) and list(self.summary.chosen) == [75, 75]
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
    invalid(call(o(lambda_rot=[1e-2, 1e-3], lambda_pos=[1e-3, 1e-2])), "lambda_rot must be strictly ascending: entry 1 is not")
    invalid(call(o(lambda_rot=[1e-3, 1e-2], lambda_pos=[1e-3, 1e-3])), "lambda_pos must be strictly ascending: entry 1 is not")
    # the cross-validated fit's own rules: choosing is its job, and the criterion is one of two
    invalid(call(o(target_rms_rot=0.1)), "target_rms_rot and target_rms_pos must be 0")
    invalid(call(o(target_rms_pos=0.1)), "target_rms_rot and target_rms_pos must be 0")
    c = lambda **kw: _capi.default_spline_cv_options(api, **kw)      # noqa: E731
    for v in (2, -1, 7):
        invalid(call(cv=c(criterion=v)), "unknown criterion %d" % v)
    # the length the on-chip solve cannot hold: UNIMPLEMENTED before the device, at the smoothing fit's ceiling and no lower
    for n_ctrl, code, word in ((2219, _capi.UNIMPLEMENTED, "too long"), (2218, _capi.INTERNAL, "no usable HIP device")):
        case = fit_ref.inputs(fit_ref._ragged(6, 1.0, n_ctrl, 20.0))
        ctrl, summary = np.full((n_ctrl, 6), 7.5), _capi.SplineCvSummary()
        st = api.fit_spline_cv(NO_DEVICE, 6, len(case.knots), _dp(case.knots), _dp(case.basis), len(case.stamps), _dp(case.stamps), _dp(case.data),
                               None, None, None, _dp(ctrl), None, None, None, None, None, C.byref(summary))
        _message(api, st, code, word)
        assert (ctrl == 7.5).all()
    # valid calls reach the device: both criteria, a full grid, weights of 0, no weights, no options
    w = call.weights.copy()
    w[::3, 0] = 0.0
    grid = tuple(10.0 ** np.linspace(-6, 2, 32))
    for cv in (c(), c(criterion=_capi.FIT_CV_PRESS)):
        _message(api, call(o(lambda_rot=grid, lambda_pos=grid), cv, weights=w), _capi.INTERNAL, "no usable HIP device", str(NO_DEVICE))
    _message(api, call(o(lambda_rot=0.0, relative=0)), _capi.INTERNAL, "no usable HIP device")
    _message(api, call(weights=None), _capi.INTERNAL, "no usable HIP device")


def test_defaults_are_the_documented_ones(api):
    o = _capi.SplineCvOptions(criterion=9, reserved=9)
    api.default_spline_cv_options(C.byref(o))
    assert (o.criterion, o.reserved) == (_capi.FIT_CV_GCV, 0)
    api.default_spline_cv_options(None)      # a null pointer is ignored
    o = _capi.default_spline_cv_options(api, criterion=_capi.FIT_CV_PRESS)
    assert (o.criterion, o.reserved) == (1, 0)
    with pytest.raises(TypeError):
        _capi.default_spline_cv_options(api, no_such_field=1)
    assert (_capi.FIT_CV_AT_GRID_END, _capi.FIT_CV_GCV, _capi.FIT_CV_PRESS) == (5, 0, 1)


def test_structs_and_symbols_match_the_header(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_spline_cv_options", "fit_spline_cv"):
        assert re.search(r"\bcalico_%s\s*\(" % name, header) and name in _capi.ABI_SYMBOLS and hasattr(api.lib, "calico_" + name)
    for macro, value in (("CALICO_FIT_CV_AT_GRID_END", 5), ("CALICO_FIT_CV_GCV", 0), ("CALICO_FIT_CV_PRESS", 1)):
        assert re.search(r"#define %s %d\b" % (macro, value), header)
    # the new status is none of the earlier ones
    assert len({_capi.FIT_OK, _capi.FIT_NOT_POSITIVE_DEFINITE, _capi.FIT_TARGET_NOT_MET, _capi.FIT_MAX_ITERATIONS, _capi.FIT_SCALE_ZERO,
                _capi.FIT_CV_AT_GRID_END}) == 6
    # the header's layouts: 2 int32; 4 doubles; 2 x 2 int32, 2 int64, 2 x 2 doubles
    O, R, S = _capi.SplineCvOptions, _capi.SplineCvRow, _capi.SplineCvSummary
    assert C.sizeof(O) == 8 and (O.criterion.offset, O.reserved.offset) == (0, 4)
    assert C.sizeof(R) == 32 and (R.edf.offset, R.gcv.offset, R.press.offset, R.max_leverage.offset) == (0, 8, 16, 24)
    assert C.sizeof(S) == 16 + 16 + 32 == 64
    assert (S.status.offset, S.chosen.offset, S.n_used.offset, S.edf.offset, S.score.offset) == (0, 8, 16, 32, 48)
    for struct, c_name in ((O, "calico_spline_cv_options"), (R, "calico_spline_cv_row"), (S, "calico_spline_cv_summary")):
        body = re.search(r"typedef struct \{((?:[^{}]|\{[^{}]*\})*)\} %s;" % c_name, header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.match(r"\s*\w+\s+(\w+)", d).group(1) for d in body.split(";") if d.strip()]
        assert fields == [n.rstrip("_") for n, _ in struct._fields_], (c_name, fields)
    # the pybind module and the C++ facade name the call too
    assert "calico_fit_spline_cv(" in open(os.path.join(ROOT, "include", "calico", "calico.hpp")).read()
    assert '"FitSplineCV"' in open(os.path.join(entry.CSRC, "pybind_calico.cpp")).read()

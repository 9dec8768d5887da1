"""calico_imu_allan without a GPU, through calico_amd._capi: every argument rule gives its code and the words of its message before
the device is touched (so a device ordinal that does not exist changes nothing), the gap rule names the sample, the explicit list
of cluster sizes has its own rules, a call that meets them all without a device is INTERNAL "no usable HIP device", and the
new names are where the rest of the project looks for them (the header, ABI_SYMBOLS, HIP_SOURCES)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import allan_ref as ar
import helpers
from calico_amd import _capi

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

NO_DEVICE = 10 ** 6
N = 400


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _call(api, samples=None, stamps=None, rate=200.0, device=NO_DEVICE, **options):
    y = np.zeros((N, 3)) if samples is None else samples
    with pytest.raises(_capi.CalicoError) as e:
        _capi.imu_allan(api, y, stamps, rate, _capi.default_allan_options(api, **options) if options else None, device)
    assert e.value.message.startswith("calico_imu_allan: "), e.value.message
    assert api.last_error(None).decode() == e.value.message
    return e.value


def _invalid(api, *words, **kw):
    e = _call(api, **kw)
    assert e.code == _capi.INVALID_ARGUMENT, (e.code, e.message)
    for w in words:
        assert w in e.message, (w, e.message)


def test_defaults(api):
    o = _capi.default_allan_options(api)
    assert (o.points_per_decade, o.max_tau_fraction, o.n_cluster_sizes, o.reserved) == (10, 0.1, 0, 0) and not o.cluster_sizes
    assert o.terms == _capi.ALLAN_TERM_WHITE | _capi.ALLAN_TERM_BIAS_INSTABILITY | _capi.ALLAN_TERM_RATE_RANDOM_WALK == ar.DEFAULT_TERMS
    assert C.sizeof(_capi.AllanNoise) == 64 and C.sizeof(_capi.AllanOptions) == 32 and C.sizeof(_capi.AllanSummary) == 48
    api.default_allan_options(None)      # (a null pointer is ignored)


def test_the_count_and_the_buffers(api):
    for n in (0, 1, 2):
        _invalid(api, "n must be >= 3", samples=np.zeros((n, 3)))
    D = C.POINTER(C.c_double)
    y = np.zeros((N, 3))
    nc, m, out = C.c_int32(0), np.zeros(256, np.int64), np.zeros((256, 3))
    noise, summary = (_capi.AllanNoise * 3)(), _capi.AllanSummary()
    good = [NO_DEVICE, N, None, 200.0, y.ctypes.data_as(D), None, C.byref(nc), m.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(D),
            out.ctypes.data_as(D), out.ctypes.data_as(D), noise, C.byref(summary)]
    for at in (4, 6, 7, 8, 9, 10, 11, 12):
        args = list(good)
        args[at] = None
        assert api.imu_allan(*args) == _capi.INVALID_ARGUMENT
        assert api.last_error(None).decode() == "calico_imu_allan: null samples or output buffer"
    args = list(good)
    args[1] = 2 ** 31      # more samples than the kernels index: refused before a sample is read
    assert api.imu_allan(*args) == _capi.UNIMPLEMENTED and "2^31 - 1 samples" in api.last_error(None).decode()


def test_the_rate(api):
    for rate in (0.0, -200.0, np.nan, np.inf):
        _invalid(api, "sample_rate_hz must be finite and > 0", rate=rate)
    t = np.arange(N) / 200.0
    bad = t.copy()
    bad[7] = np.nan
    _invalid(api, "stamp 7 is not finite", stamps=bad)
    bad = t.copy()
    bad[9] = bad[8]
    _invalid(api, "strictly increasing", "sample 9", stamps=bad)
    bad = t.copy()
    bad[300] = bad[298]
    _invalid(api, "strictly increasing", "sample 300", stamps=bad)
    # a gap: the first step outside [0.5, 1.5] of the mean step is named, and the advice
    bad = t.copy()
    bad[123:] += 0.004
    _invalid(api, "the step to sample 123", "a gap: split the log", stamps=bad)
    bad = t.copy()
    bad[200] = 0.5 * (bad[199] + bad[200]) - 1e-4      # a short step (0.48), then a long one (1.52)
    _invalid(api, "the step to sample 200", "a gap: split the log", stamps=bad)
    # with stamps the rate argument is not read: jitter inside the band passes the rules and reaches the device's error
    jitter = t + 1e-3 * np.sin(np.arange(N))
    e = _call(api, stamps=jitter, rate=np.nan)
    assert e.code == _capi.INTERNAL and "no usable HIP device" in e.message


def test_the_options(api):
    _invalid(api, "points_per_decade must be >= 1", points_per_decade=0)
    for f in (0.0, -0.1, 0.500001, np.nan, np.inf):
        _invalid(api, "max_tau_fraction must be in (0, 0.5]", max_tau_fraction=f)
    for terms in (0, 32, -1, 2 | 64):
        _invalid(api, "terms must be a non-empty mask", terms=terms)
    _invalid(api, "the log is too short", samples=np.zeros((5, 3)))      # 0.1 n < 1: the default grid holds no cluster size
    # an argument error and a device that does not exist: still the argument's error
    _invalid(api, "points_per_decade", points_per_decade=-3, device=NO_DEVICE)


def test_the_explicit_list(api):
    for sizes, words in (([0, 1], ("cluster size 0", "1 <= m and 2 m < n")), ([1, 200], ("cluster size 1", "2 m < n")),
                         ([1, 5, 5], ("strictly increasing", "entry 2")), ([3, 2], ("strictly increasing", "entry 1")),
                         ([-4], ("cluster size 0",)), ([1, 2 ** 40], ("cluster size 1",))):
        _invalid(api, *words, cluster_sizes=sizes)
    _invalid(api, "n_cluster_sizes must be in [0, 256]", cluster_sizes=np.arange(1, 258))
    o = _capi.default_allan_options(api)
    o.n_cluster_sizes = 3
    with pytest.raises(_capi.CalicoError) as e:
        _capi.imu_allan(api, np.zeros((N, 3)), None, 200.0, o, NO_DEVICE)
    assert e.value.code == _capi.INVALID_ARGUMENT and "null cluster_sizes" in e.value.message
    # the list is read instead of the grid's options: those are then not checked
    e = _call(api, cluster_sizes=[1, 2, 199], points_per_decade=0, max_tau_fraction=7.0)
    assert e.code == _capi.INTERNAL and "no usable HIP device" in e.message


def test_a_valid_call_without_a_device_says_so(api):
    for device in (NO_DEVICE, -1):
        e = _call(api, device=device)
        assert e.code == _capi.INTERNAL and "no usable HIP device" in e.message
    e = _call(api, samples=np.zeros((3, 3)), cluster_sizes=[1])
    assert e.code == _capi.INTERNAL
    if not helpers.has_gpu():
        e = _call(api, device=0)
        assert e.code == _capi.INTERNAL and "no usable HIP device 0" in e.message


def test_where_the_names_live():
    header = open(os.path.join(helpers.ROOT, "include", "calico_hip.h")).read()
    for name in ("default_allan_options", "imu_allan"):
        assert name in _capi.ABI_SYMBOLS and re.search(r"\bcalico_%s\(" % name, header), name
    assert "calico_accel_align, calico_imu_allan)" in header      # calico_last_error's list of the calls without a handle
    assert "#define CALICO_ALLAN_MAX_CLUSTERS 256" in header and _capi.ALLAN_MAX_CLUSTERS == ar.MAX_CLUSTERS == 256
    for f in ("allan.cpp", "allan_kernels.hip"):
        assert f in entry.HIP_SOURCES, f
    csrc = entry.CSRC
    kernels = open(os.path.join(csrc, "kernels.hpp")).read()
    assert "constexpr int kAllanScanBlock = %d;" % ar.SCAN_BLOCK in kernels and "constexpr int kAllanTermChunk = %d;" % ar.TERM_CHUNK in kernels
    assert "kAllanScanBlock = %d" % ar.SCAN_BLOCK in header and "kAllanTermChunk = %d" % ar.TERM_CHUNK in header
    assert "launch_imu_allan" in kernels
    host = open(os.path.join(csrc, "allan.cpp")).read()
    assert "getenv" not in host and "hipMalloc" not in host and "FreeCall call{\"calico_imu_allan\"}" in host
    assert host.count(".download(") == 1      # one readback
    for rule in ("allan_options_error", "allan_rate_error", "allan_grid_error"):
        assert rule in host and rule in open(os.path.join(csrc, "arg_rules.hpp")).read(), rule
    for code, name in enumerate(("OK", "NO_WHITE_NOISE", "TOO_FEW_POINTS", "NONFINITE")):
        assert "#define CALICO_ALLAN_%s %d" % (name, code) in header and getattr(_capi, "ALLAN_" + name) == getattr(ar, name) == code

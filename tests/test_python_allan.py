"""The noise characterisation through `from calico_amd import calico`: without a GPU, the names, SetImuNoise's arithmetic on a
characterisation given as a dict, and the library's argument errors as RuntimeError("Error: ..."); on the GPU (`-m gpu`),
CharacterizeImuNoise on the synthetic log returns the C ABI's numbers, and SetImuNoise leaves N_pooled sqrt(rate) in the sensor,
the rate taken from the sensor's own stamps where none is given.

`calico` is imported inside the tests: the GPU test asks for the `hip` fixture first, which brings PyTorch's HIP runtime into the
process before the library's (conftest.py)."""
import numpy as np
import pytest

import allan_ref as ar
from calico_amd import _capi

RATE = 200.0


def _gyroscope(stamps):
    from calico_amd import calico
    g = calico.Gyroscope()
    g.SetModel(calico.GyroscopeIntrinsicsModel.kGyroscopeScaleAndBias)
    ms = []
    for i, t in enumerate(stamps):
        m = calico.GyroscopeMeasurement()
        m.measurement = np.zeros(3)
        m.id.stamp, m.id.sequence = float(t), i
        ms.append(m)
    assert g.AddMeasurements(ms).ok()
    return g


def test_set_imu_noise_on_the_host():
    from calico_amd import calico
    noise = {"summary": {"N_pooled": 1.7e-4}}
    g = _gyroscope(3.0 + np.arange(101)[::-1] / 400.0)      # (out of order: the rate is (n - 1) / (last - first) all the same)
    assert g.GetMeasurementNoise() == 1.0 and g.MeasurementRate() == 400.0
    assert calico.SetImuNoise(g, noise) == 1.7e-4 * np.sqrt(400.0) == g.GetMeasurementNoise()
    assert calico.SetImuNoise(g, noise, rate_hz=200.0) == 1.7e-4 * np.sqrt(200.0) == g.GetMeasurementNoise()
    a = calico.Accelerometer()
    a.SetModel(calico.AccelerometerIntrinsicsModel.kAccelerometerScaleAndBias)
    with pytest.raises(RuntimeError, match="Error: .*fewer than two measurements"):
        calico.SetImuNoise(a, noise)
    assert calico.SetImuNoise(a, noise, 100.0) == 1.7e-4 * 10.0
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="Error: ApplyNoise: rate_hz"):
            calico.SetImuNoise(a, noise, bad)
    with pytest.raises(RuntimeError, match="Error: ApplyNoise: .*no white-noise density"):
        calico.SetImuNoise(a, {"summary": {"N_pooled": 0.0}}, 100.0)
    assert a.GetMeasurementNoise() == 1.7e-4 * 10.0      # (a refused call changes nothing)


def test_argument_errors_surface_as_runtime_errors():
    from calico_amd import calico
    t = np.arange(400) / RATE
    gap = t.copy()
    gap[77:] += 0.02
    with pytest.raises(RuntimeError, match=r"Error: calico_imu_allan: the step to sample 77 .*a gap: split the log"):
        calico.CharacterizeImuNoise(gap, np.zeros((400, 3)))
    with pytest.raises(RuntimeError, match="Error: calico_imu_allan: max_tau_fraction"):
        calico.CharacterizeImuNoise(t, np.zeros((400, 3)), {"max_tau_fraction": 0.7})
    with pytest.raises(RuntimeError, match="Error: CharacterizeImuNoise: one stamp per sample"):
        calico.CharacterizeImuNoise(t[:-1], np.zeros((400, 3)))
    with pytest.raises(TypeError, match="no Allan variance option 'tau'"):
        calico.CharacterizeImuNoise(t, np.zeros((400, 3)), {"tau": 1})


@pytest.mark.gpu
def test_characterize_returns_the_c_abis_numbers(hip):
    from calico_amd import calico
    rate = 256.0      # (a power of two: the stamps and the rate they give are exact)
    y = ar.synthetic_log(0, n=2 ** 16, rate=rate)
    t = 5.0 + np.arange(len(y)) / rate
    got = calico.CharacterizeImuNoise(t, y)
    want = _capi.imu_allan(hip, y, t)
    for name in ("cluster_sizes", "tau", "rel_err", "avar"):
        assert np.array_equal(got[name], want[name]), name
    assert got["noise"] == want["noise"] and got["summary"] == want["summary"]
    assert len(got["tau"]) == len(ar.grid(len(y))) and all(a["status"] == ar.OK for a in got["noise"])
    # options travel: an explicit list and every term
    sizes = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    got = calico.CharacterizeImuNoise(t, y, {"cluster_sizes": sizes, "terms": 31})
    want = _capi.imu_allan(hip, y, t, 0.0, _capi.default_allan_options(hip, cluster_sizes=sizes, terms=31))
    assert np.array_equal(got["avar"], want["avar"]) and got["noise"] == want["noise"] and list(got["cluster_sizes"]) == sizes
    # into the sensor: the rate of the sensor's own measurements (100 Hz here), or the one given
    noise = calico.CharacterizeImuNoise(t, y)
    g = _gyroscope(np.arange(51) / 100.0)
    assert calico.SetImuNoise(g, noise) == noise["summary"]["N_pooled"] * np.sqrt(100.0) == g.GetMeasurementNoise()
    assert noise["summary"]["sample_rate_hz"] == rate and calico.SetImuNoise(g, noise, rate) == noise["summary"]["sigma_at_rate"]
    assert abs(noise["summary"]["N_pooled"] / 1e-3 - 1) <= 0.02

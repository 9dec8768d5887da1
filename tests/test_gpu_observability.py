"""Observability report (calico_observability_compute) against a CPU reference built from the oracle.

Reference (observability_ref.py): the same seeded scene in the oracle with the GPU's parameter values copied in, the
oracle's dense JᵀJ from evaluate(), then numpy: S = C - Eᵀ A⁻¹ E (A equilibrated by its diagonal), zero-diagonal border
columns dropped, scaled by sqrt(diag C), symmetrised, eigh.

Bounds. TOL_LAMBDA and TOL_PROJ are ten times the largest deviation measured on an MI355X over the scenes below (the two
sides form S by different eliminations of a band whose equilibrated condition number is 6e4 .. 6e8 here, so the deviation
scales with that and not with the eigensolver); the measured values are listed next to them. TOL_DECOMP is derived: each
column takes at most sweeps·(n - 1) rotations with a relative error of a few eps each; n <= 256, 30 sweeps and 6 eps per
rotation stay below 5e-12."""
import ctypes as C
import time

import numpy as np
import pytest

import observability_ref as R
from calico_amd import _capi, synthetic as syn
from helpers import _state, run_two_ranks, solve

pytestmark = pytest.mark.gpu

# Measured (|λ_gpu - λ_ref|_max / λ_max per scene): see MEASURED_LAMBDA; the derivable ceiling is eps times the largest
# equilibrated band condition number of these scenes (5.7e8, the camera-only ones), about 6e-8.
# Camera-only scenes at the start values (band condition 3e8 .. 5.7e8): 2.8e-10 (model 1), 2.4e-10 (2), 9.1e-11 (3), 3.0e-10 (4),
# 1.1e-10 (5), 2.9e-10 (6), 1.6e-11 (7), gauge 2.5e-10; scenes with an IMU (condition 6e4 .. 3e6): 1.4e-14 .. 1.9e-12;
# configs[3] 1.4e-13, configs[4] 4.2e-14.
MEASURED_LAMBDA = 3.02e-10     # largest over the scenes of test_spectrum_parity and the full-size ones
TOL_LAMBDA = 10 * MEASURED_LAMBDA
# OpenCV8 5.3e-13, gauge 3.6e-9 (the reference's own gap is the smallest there: 4e8), VectorNav 2.3e-11 / 1.9e-11 (robust),
# configs[3] 3.0e-11, configs[4] 7.4e-11.
MEASURED_PROJ = 3.56e-9        # largest |P_gpu - P_ref|_F over the singular scenes, full size included
TOL_PROJ = 10 * MEASURED_PROJ
TOL_DECOMP = 1e-11

ALL_SCENES = dict(R.TABLE_SCENES)
ALL_SCENES.update(R.MORE_SCENES)
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_reports():
    """The cached reports keep their library handles (and those the device memory they allocated from) only while this module
    runs: a later test that measures what the library holds on the device must not see them."""
    yield
    import gc
    for c in _cache.values():
        c["gpu"].problem.close()
    _cache.clear()
    gc.collect()


def report(name, hip, oracle):
    """The GPU's report of a named scene and the reference at the same values (computed once per session)."""
    if name not in _cache:
        mk, iters, n_weak = ALL_SCENES[name]
        scene = mk()
        gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
        if iters:
            solve(gpu.problem, hip, iters)
        info = gpu.problem.observability_compute()
        R.copy_values(gpu, ref)
        r = R.reference(ref, info["dim"], scene.order)
        _cache[name] = dict(scene=scene, gpu=gpu, info=info, ref=r, n_weak=n_weak, lam=gpu.problem.observability_spectrum(),
                            V=gpu.problem.observability_directions(), S=gpu.problem.observability_matrix(),
                            dbg=gpu.problem.observability_debug())
    return _cache[name]


@pytest.mark.parametrize("name", list(ALL_SCENES))
def test_spectrum_parity(name, hip, oracle):
    c = report(name, hip, oracle)
    r, info, lam = c["ref"], c["info"], c["lam"]
    assert r["lam"] is not None, ("the oracle's band is not positive definite", r["band_pivot"])
    assert info["n_unobserved"] == int((~r["keep"]).sum())
    assert len(lam) == len(r["lam"]) == info["dim"] - info["n_unobserved"]
    dev = np.abs(lam - r["lam"]).max() / r["lam"][-1]
    print("observability spectrum %s: dim %d kept %d sweeps %d rotations %d in_lds %d, lowest gpu %s ref %s, max %.4f, "
          "|dλ|/λmax %.2e (band cond %.1e, band pivot gpu %.2e ref %.2e, root pivot %.2e)" % (
              name, info["dim"], len(lam), info["sweeps"], c["dbg"]["rotations"], c["dbg"]["in_lds"], lam[:c["n_weak"] + 2],
              r["lam"][:c["n_weak"] + 2], lam[-1], dev, r["band_cond"], c["dbg"]["min_relative_pivot_band"], r["band_pivot"],
              c["dbg"]["min_relative_pivot_root"]))
    assert np.all(np.diff(lam) >= 0.0)
    assert info["lambda_min"] == lam[0] and info["lambda_max"] == lam[-1]
    assert dev <= TOL_LAMBDA, dev
    assert info["n_weak"] == c["n_weak"] == R.weak_count(r["lam"])


def _subspace(c):
    """(|P_gpu - P_ref|_F, P_gpu, P_ref on the kept columns) across the reference's spectral gap."""
    r, k = c["ref"], c["info"]["n_weak"]
    lr = r["lam"]
    assert k == R.weak_count(lr) and k > 0
    gap = lr[k] / np.abs(lr[:k]).max()
    assert gap >= R.GAP, gap      # the comparison only means something across a gap: a scene without one fails here
    keep = r["keep"]
    Vg = c["V"][:, keep].T         # columns: eigenvectors on the kept columns
    assert np.all(c["V"][:, ~keep] == 0.0)
    Pg, Pr = R.projector(Vg, k), R.projector(r["V"], k)
    return np.linalg.norm(Pg - Pr), Pg, Pr, gap


@pytest.mark.parametrize("name", R.SINGULAR_SCENES)
def test_weak_count_and_subspace(name, hip, oracle):
    c = report(name, hip, oracle)
    assert c["info"]["n_weak"] == c["n_weak"]
    d, _, _, gap = _subspace(c)
    print("observability subspace %s: n_weak %d, reference gap %.1e, |P_gpu - P_ref|_F %.2e" % (name, c["n_weak"], gap, d))
    assert d <= TOL_PROJ, d


@pytest.mark.parametrize("name", R.SINGULAR_SCENES)
def test_where_the_directions_live(name, hip, oracle):
    c = report(name, hip, oracle)
    gpu, scene, k = c["gpu"], c["scene"], c["info"]["n_weak"]
    _, _, Pr, _ = _subspace(c)
    layout, dim = R.border_layout(gpu, scene)
    assert dim == c["info"]["dim"]
    kept_pos = np.cumsum(c["ref"]["keep"]) - 1      # border column -> index among the kept ones
    named = set(R.null_space_blocks(name, gpu, scene))
    outside_ref = 0.0
    for b, (off, t) in layout.items():
        shares = [gpu.problem.observability_block(i, b)[1] for i in range(k)]
        rows = [kept_pos[j] for j in range(off, off + t) if c["ref"]["keep"][j]]
        want = float(np.trace(Pr[np.ix_(rows, rows)])) if rows else 0.0
        assert abs(sum(shares) - want) <= np.sqrt(t) * TOL_PROJ, (b, sum(shares), want)
        # the block reader returns the rows of the direction reader
        for units in (False, True):
            row, _ = gpu.problem.observability_block(0, b, tangent_units=units)
            assert np.array_equal(row, gpu.problem.observability_directions(0, 1, tangent_units=units)[0, off:off + t])
        if b not in named:
            outside_ref += want
    print("observability null space %s: share outside the named blocks (reference) %.2e" % (name, outside_ref))
    assert outside_ref <= 1e-8 * k


@pytest.mark.parametrize("name", list(ALL_SCENES))
def test_decomposition(name, hip, oracle):
    """V orthonormal and V Λ Vᵀ = S̃ as the device formed it: independent of the oracle."""
    c = report(name, hip, oracle)
    keep = np.abs(c["V"]).sum(axis=0) != 0.0
    assert keep.sum() == len(c["lam"])
    V = c["V"][:, keep].T
    S = c["S"][np.ix_(keep, keep)]
    assert np.all(c["S"][~keep] == 0.0) and np.all(c["S"][:, ~keep] == 0.0)
    assert np.array_equal(S, S.T)
    orth = np.abs(V.T @ V - np.eye(len(V))).max()
    rec = np.abs((V * c["lam"]) @ V.T - S).max() / c["lam"][-1]
    print("observability decomposition %s: |VᵀV - I|_max %.2e, |VΛVᵀ - S̃|_max/λmax %.2e, sweeps %d" % (name, orth, rec, c["info"]["sweeps"]))
    assert orth <= TOL_DECOMP and rec <= TOL_DECOMP
    # sign convention and tangent units
    for v in c["V"]:
        assert v[np.argmax(np.abs(v))] > 0.0
    Dl = c["gpu"].problem.observability_directions(tangent_units=True)
    assert np.allclose(np.linalg.norm(Dl, axis=1), 1.0, rtol=0, atol=1e-14)


def test_trajectory_deficiency(hip, oracle):
    """The camera-only scene solved to the iteration limit: the band itself is singular there, S does not exist."""
    scene = R.small_scene(camera_model=1, imu=False)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    R.copy_values(gpu, ref)
    _, mc = R.border_layout(gpu, scene)
    r = R.reference(ref, mc, scene.order)
    print("observability, camera 1 solved: the oracle's natural-order band pivot %.3e" % r["band_pivot"])
    assert r["band_pivot"] < 1e-12      # (<= 0, or below min_relative_pivot)
    with pytest.raises(_capi.CalicoError) as e:
        gpu.problem.observability_compute()
    print("  ->", e.value.message)
    assert e.value.code == _capi.FAILED_PRECONDITION and "trajectory" in e.value.message
    for call in (gpu.problem.observability_info, gpu.problem.observability_spectrum, gpu.problem.observability_matrix,
                 gpu.problem.observability_directions):
        with pytest.raises(_capi.CalicoError) as e:
            call()
        assert e.value.code == _capi.FAILED_PRECONDITION
    with pytest.raises(_capi.CalicoError) as e:       # the covariance's message is about the border, this one is not
        gpu.problem.covariance_compute()
    assert "trajectory" not in e.value.message


def test_no_side_effects(hip):
    scene = R.small_scene(camera_model=1, imu=True)
    a, b = syn.build_problem(hip, scene), syn.build_problem(hip, scene)
    for x in (a, b):
        x.problem.set_phase_timing(0x7f)
    sa1 = solve(a.problem, hip, 5)
    sb1 = solve(b.problem, hip, 5)
    for x in (a, b):
        x.problem.covariance_compute()
    cov_before = b.problem.covariance_dense()
    na = [a.problem.phase_time(k)[1] for k in range(7)]
    before = _state(b, scene)
    b.problem.observability_compute()
    after = _state(b, scene)
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k])
    for (rx, vx), (ry, vy) in zip(before[1], after[1]):
        assert np.array_equal(rx, ry) and np.array_equal(vx, vy)
    assert np.array_equal(b.problem.covariance_dense(), cov_before)      # a stored covariance is left alone
    assert np.array_equal(b.problem.covariance_dense(), a.problem.covariance_dense())
    assert [(r.iteration, r.cost) for r in b.problem.iterations()] == [(r.iteration, r.cost) for r in a.problem.iterations()]
    assert b.problem.plan_info() == a.problem.plan_info()
    assert [b.problem.phase_time(k)[1] for k in range(7)] == na      # the pass records no launches into the phase timer
    sa2 = solve(a.problem, hip, 30)
    sb2 = solve(b.problem, hip, 30)
    keys = [k for k, _ in _capi.Summary._fields_ if "time" not in k]
    d1a, d1b, d2a, d2b = (x.as_dict() for x in (sa1, sb1, sa2, sb2))
    assert [d1a[k] for k in keys] == [d1b[k] for k in keys]
    assert [d2a[k] for k in keys] == [d2b[k] for k in keys]
    ia = [(r.iteration, r.step_is_successful, r.cost, r.cost_change, r.trust_region_radius) for r in a.problem.iterations()]
    ib = [(r.iteration, r.step_is_successful, r.cost, r.cost_change, r.trust_region_radius) for r in b.problem.iterations()]
    assert ia == ib
    va, _ = _state(a, scene)
    vb, _ = _state(b, scene)
    for k in va:
        assert np.array_equal(va[k], vb[k])


def test_determinism(hip):
    scene = R.small_scene(camera_model=1, imu=True, imu_model=3)
    g = syn.build_problem(hip, scene)
    solve(g.problem, hip)
    g.problem.observability_compute()
    l1, v1, d1 = g.problem.observability_spectrum(), g.problem.observability_directions(), g.problem.observability_directions(tangent_units=True)
    g.problem.observability_compute()
    l2, v2, d2 = g.problem.observability_spectrum(), g.problem.observability_directions(), g.problem.observability_directions(tangent_units=True)
    assert np.array_equal(l1, l2) and np.array_equal(v1, v2) and np.array_equal(d1, d2)


def test_errors(hip):
    scene = R.small_scene(camera_model=1, imu=True)
    g = syn.build_problem(hip, scene)
    P = g.problem
    intr = g.sensor_blocks[0]["intrinsics"]
    for call in (P.observability_info, P.observability_spectrum, P.observability_matrix, lambda: P.observability_block(0, intr)):
        with pytest.raises(_capi.CalicoError) as e:
            call()
        assert e.value.code == _capi.FAILED_PRECONDITION
    assert hip.observability_compute(None, None) == _capi.INVALID_ARGUMENT
    with pytest.raises(_capi.CalicoError) as e:
        P.observability_compute(weak_threshold=-1.0)
    assert e.value.code == _capi.INVALID_ARGUMENT
    info = P.observability_compute()
    kept = info["dim"] - info["n_unobserved"]
    assert info["n_unobserved"] >= 3          # the gyroscope's translation block: registered, used by no residual
    D = C.POINTER(C.c_double)
    out = np.zeros(info["dim"] * 2)
    sh = C.c_double(0)
    assert hip.observability_get_spectrum(P.h, None) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_matrix(P.h, None) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_directions(P.h, 0, 1, 0, None) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_directions(P.h, -1, 1, 0, out.ctypes.data_as(D)) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_directions(P.h, kept, 1, 0, out.ctypes.data_as(D)) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_directions(P.h, 0, kept + 1, 0, out.ctypes.data_as(D)) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_directions(P.h, kept, 0, 0, out.ctypes.data_as(D)) == _capi.OK
    assert hip.observability_get_block(P.h, 0, 10 ** 6, 0, out.ctypes.data_as(D), C.byref(sh)) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_block(P.h, 0, -1, 0, out.ctypes.data_as(D), C.byref(sh)) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_block(P.h, kept, intr, 0, out.ctypes.data_as(D), C.byref(sh)) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_block(P.h, 0, intr, 0, None, None) == _capi.INVALID_ARGUMENT
    assert hip.observability_get_block(P.h, 0, int(g.ctrl_blocks[3]), 0, out.ctypes.data_as(D), C.byref(sh)) == _capi.INVALID_ARGUMENT
    # constant blocks (gravity, the chart pose) and the unobserved gyroscope translation: zeros
    row, share = P.observability_block(0, g.gravity_block)
    assert np.all(row == 0.0) and share == 0.0
    row, share = P.observability_block(0, g.body_q_block)
    assert row.shape == (3,) and np.all(row == 0.0) and share == 0.0
    gyro = [b for s, b in zip(scene.sensors, g.sensor_blocks) if s.kind == _capi.SENSOR_GYROSCOPE][0]
    assert all(P.observability_block(i, gyro["t"])[1] == 0.0 for i in range(kept))
    # the shares of all blocks of a direction add up to 1
    layout, _ = R.border_layout(g, scene)
    assert abs(sum(P.observability_block(0, b)[1] for b in layout) - 1.0) <= 1e-12


def test_stale_result_is_refused_after_the_problem_changes(hip):
    scene = R.small_scene(camera_model=1, imu=True)
    g = syn.build_problem(hip, scene)
    P = g.problem
    P.observability_compute()
    before = P.observability_spectrum()
    solve(P, hip, 3)                       # values change, the structure does not: the result stays readable
    assert np.array_equal(P.observability_spectrum(), before)
    new = P.add_param_block(np.ones(3))    # a structural change
    for call in (P.observability_info, P.observability_spectrum, P.observability_matrix, P.observability_directions):
        with pytest.raises(_capi.CalicoError) as e:
            call()
        assert e.value.code == _capi.FAILED_PRECONDITION
    solve(P, hip, 3)                       # re-finalised: still refused until computed again
    with pytest.raises(_capi.CalicoError) as e:
        P.observability_block(0, new)
    assert e.value.code == _capi.FAILED_PRECONDITION
    P.observability_compute()
    assert P.observability_block(0, new)[1] == 0.0      # (unused by any residual)


def test_border_above_256_columns_is_unimplemented(hip):
    """Free model points on the 144-point chart: a border of more than 256 columns."""
    scene = R.small_scene(camera_model=1, n_cameras=2, imu=True, free_points=True, chart="april", seed=5)
    g = syn.build_problem(hip, scene)
    _, dim = R.border_layout(g, scene)
    assert dim > 256
    with pytest.raises(_capi.CalicoError) as e:
        g.problem.observability_compute()
    assert e.value.code == _capi.UNIMPLEMENTED and str(dim) in e.value.message and "256" in e.value.message


def test_multirank_two_handles_agree(hip):
    """Two ranks on one device, each a handle sharded to its time window with a host exchange (sum in rank order): both
    hold the same report bit for bit, equal to the single-rank one to rounding."""
    scene = R.small_scene(camera_model=1, imu=True, imu_model=3, robust=True, seed=3)
    single = syn.build_problem(hip, scene)
    solve(single.problem, hip)
    vals = {b: single.problem.get_param_block(b, n) for b, n in dict(single.problem._sizes).items()}
    i1 = single.problem.observability_compute()
    l1 = single.problem.observability_spectrum()

    def per_rank(b):
        info = b.problem.observability_compute()
        return info, b.problem.observability_spectrum(), b.problem.observability_directions(), b.problem.observability_matrix()
    results = run_two_ranks(hip, scene, vals, per_rank)
    assert results[0][0] == results[1][0]
    for x, y in zip(results[0][1:], results[1][1:]):
        assert np.array_equal(x, y)
    assert results[0][0]["n_weak"] == i1["n_weak"] == 6
    assert np.abs(results[0][1] - l1).max() <= 1e-9 * l1[-1]


@pytest.mark.parametrize("index,n_weak,in_lds", [(3, 6, 1), (4, 12, 0)])
def test_full_size(index, n_weak, in_lds, hip, oracle):
    """configs[3] / configs[4] as they are (their own VectorNav IMUs: the problems the covariance cannot serve), at their
    start values, against the oracle at full size. Both size classes of the kernel: 88 kept columns in LDS, 183 in the
    global workspace. No time bound: the wall time is printed. Measured on an MI355X: 4.06 ms / 58.3 ms for a synchronised
    compute, of which the kernel (rocprofv3 --kernel-trace --stats) 3.50 ms / 57.0 ms; 16 / 19 sweeps."""
    scene = syn.config_scene(index)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    info = gpu.problem.observability_compute()
    dbg = gpu.problem.observability_debug()
    lam, V = gpu.problem.observability_spectrum(), gpu.problem.observability_directions()
    r = R.reference(ref, info["dim"], scene.order)
    c = dict(ref=r, info=info, V=V)
    assert info["n_unobserved"] == int((~r["keep"]).sum())
    k = R.weak_count(r["lam"])
    dev = np.abs(lam - r["lam"]).max() / r["lam"][-1]
    d, _, _, gap = _subspace(c)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        gpu.problem.observability_compute()
        ts.append(time.perf_counter() - t0)
    assert np.array_equal(gpu.problem.observability_spectrum(), lam)
    print("observability configs[%d]: dim %d kept %d n_weak %d (reference %d, gap %.1e), lowest %s, next %.2e, max %.3f, |dλ|/λmax %.2e, "
          "|P_gpu - P_ref|_F %.2e, sweeps %d rotations %d in_lds %d reduced rows %d, compute wall time %.3f ms (median of 3 after a "
          "warm-up)" % (index, info["dim"], len(lam), info["n_weak"], k, gap, lam[:k], lam[k], lam[-1], dev, d, info["sweeps"],
                        dbg["rotations"], dbg["in_lds"], dbg["reduced_rows"], 1e3 * np.median(ts)))
    assert info["n_weak"] == k == n_weak
    assert dbg["in_lds"] == in_lds
    assert dev <= TOL_LAMBDA and d <= TOL_PROJ
    with pytest.raises(_capi.CalicoError) as e:       # the covariance refuses these
        gpu.problem.covariance_compute()
    assert e.value.code == _capi.FAILED_PRECONDITION

"""Every way a solve can end, as a table of cases shared by test_solve_endings_oracle.py (CPU: the cases do on the oracle what
they were built for) and test_gpu_solve_endings.py (the device's loop forms against the oracle, case by case).

A case is a scene, solver options, and the ending the oracle's restatement of Ceres' trust_region_minimizer.cc gives for them:
reason string, termination type, Summary::num_iterations. No threshold is written down here: threshold_between() takes them from
the oracle's own log of the scene, solved with the three tolerances at 0 and a budget of 30, as the geometric mean of the
deciding quantity in the two rows the ending has to fall between -- and refuses a pair of rows less than a factor 10 apart, so
that the rounding differences between two implementations cannot move an ending to another iteration.

Scenes (the smallest that still have frames, cells, a tree with a root and a dense border):
  A  test_ceres_log's budget scene: one camera + IMU, 600 camera observations, spline order 6; every step up to row 8 accepted
  B  the ladder scene of test_gpu_reference_branches (built here, imported there): rows 1-6 rejected, two of them at candidates
     that cannot be evaluated, acceptance from row 7 on
     (and once started with the near point BEHIND the camera: the first evaluation fails, the solve ends before row 0)
  C  helpers.small_scene(camera_model=1, n_cameras=1, imu=True) with min_lm_diagonal = 0: the gyroscope's lever arm has
     structurally zero columns, the damped pivot is exactly 0 and every step is invalid

The module also holds what both sides of a comparison go through: run_case() -> Run (summary, log rows, parameter blocks, the
start), and the comparison rules (assert_same_ending, assert_rows_close, assert_estimates_close, assert_costs_close)."""
import collections
import functools

import numpy as np

import helpers
from calico_amd import _capi, synthetic as syn

DBL_MAX = float(np.finfo(np.float64).max)

MSG_BUDGET = "Maximum number of iterations reached."
MSG_GRADIENT = "Gradient tolerance reached."
MSG_RADIUS = "Minimum trust region radius reached."
MSG_PARAMETER = "Parameter tolerance reached."
MSG_FUNCTION = "Function tolerance reached."
MSG_INITIAL_FAILURE = "Initial residual and Jacobian evaluation failed."
MSG_INVALID_STEPS = "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps."


# ---- the crafted scenes of test_gpu_reference_branches.py (static camera at the origin, hand-placed points) ----

def crafted_camera(model, intr, meas, stamps, pidx, latency=0.0, free_latency=False, free_extrinsics=False):
    return syn.SensorSpec(_capi.SENSOR_CAMERA, model, "cam", np.asarray(intr, float), np.array([0.0, 0, 0, 1.0]), np.zeros(3),
                          latency, np.asarray(intr, float), np.array([0.0, 0, 0, 1.0]), np.zeros(3), latency, True,
                          free_extrinsics, free_latency, sigma=1.0, loss=0, loss_scale=1.0, meas=np.asarray(meas, float),
                          stamps=np.asarray(stamps, float), point_idx=np.asarray(pidx, np.int32))


def crafted_scene(ctrl_fn, points, sensors_fn, t1=1.0, knot_frequency=10.0, order=6):
    knots = syn.knot_vector(0.0, t1, order, knot_frequency)
    basis = syn.basis_matrices(knots, order)
    n_ctrl = len(knots) - order
    ctrl = np.array([ctrl_fn(i) for i in range(n_ctrl)], float)
    sc = syn.Scene(order, knots, basis, ctrl.copy(), ctrl.copy(), np.asarray(points, float), np.array([0.0, 0, 0, 1.0]), np.zeros(3),
                   np.array([0.0, 0.0, -9.80665]), [])
    sc.sensors = sensors_fn(sc)
    return sc


def static_points():
    # camera at the origin looking down +z (all poses identity): the first point sits 5e-10 off the optical axis, inside
    # the r < 1e-9 branch. (EXACTLY on the axis the reference's autodiff differentiates sqrt(x^2 + y^2) at 0 and hands
    # Ceres a NaN Jacobian -- the oracle does the same; that input is a failed evaluation, not a branch to mirror.)
    return np.array([[5e-10, 0.0, 1.0], [0.1, 0.0, 1.0], [0.0, -0.2, 1.5], [0.3, 0.25, 2.0], [-0.2, 0.1, 0.8], [1e-4, -2e-4, 1.0],
                     [-0.4, -0.3, 1.2], [0.05, 0.4, 1.1]])


def observe_all_points(scene, stamps, model, intr, noise=0.3, seed=5, **kw):
    rng = np.random.default_rng(seed)
    spl = (scene.knots, scene.basis, scene.ctrl_true, scene.order)
    px, valid, st, _, pidx = syn.project_camera(spl, model, np.asarray(intr, float), np.array([0.0, 0, 0, 1.0]), np.zeros(3), 0.0,
                                                 np.asarray(stamps, float), scene.points, scene.body_q, scene.body_t)
    assert valid.all()
    return [crafted_camera(model, intr, px + noise * rng.standard_normal(px.shape), st, pidx, **kw)]


def ladder_scene():
    """A point one centimetre in front of the camera, the start three centimetres back: steps push the point behind the
    camera, the candidate's cost cannot be evaluated, the step is rejected with cost 1.797693e+308 and the radius goes down
    the /2 /4 /8 ladder until a step is short enough to be accepted."""
    cv = syn._TRUE_INTRINSICS[1].copy()
    pts = static_points().copy()
    pts[5] = [0.002, -0.001, 0.01]
    scene = crafted_scene(lambda i: [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], pts,
                          lambda sc: observe_all_points(sc, [0.05, 0.31, 0.52, 0.77], 1, cv, noise=0.0))
    scene.ctrl = scene.ctrl + np.array([0.0, 0.0, 0.0, 0.0, 0.0, -0.03])
    return scene


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "A":
        import test_ceres_log
        return test_ceres_log._budget_scene()
    if name == "B":
        return ladder_scene()
    if name == "B-behind":      # the ladder scene started three centimetres FORWARD: the near point is behind the camera at the start
        sc = ladder_scene()
        sc.ctrl = sc.ctrl + np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.06])
        return sc
    if name == "C":
        return helpers.small_scene(camera_model=1, n_cameras=1, imu=True)
    raise KeyError(name)


# ---- one solve, recorded ----

SUMMARY_COUNTS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_jacobian_evaluations",
                  "num_cost_evaluations")
ROW_FLAGS = ("iteration", "step_is_valid", "step_is_successful")
ROW_VALUES = ("cost", "trust_region_radius", "gradient_max_norm", "step_norm", "relative_decrease")

Run = collections.namedtuple("Run", "summary rows start params built")      # summary: dict; rows: list of dicts; start, params: {block: values}


def make_options(api, fields, sync_every=1):
    o = api.default_options()
    o.minimizer_progress_to_stdout = 0
    o.sync_every = sync_every
    for k, v in fields.items():
        if not hasattr(o, k):
            raise TypeError("no solver option %r" % k)
        setattr(o, k, v)
    return o


def read_params(built):
    P = built.problem
    return {int(b): P.get_param_block(int(b), n) for b, n in dict(P._sizes).items()}


def write_params(built, values):
    for b, v in values.items():
        built.problem.set_param_block(b, v)


def record(built, summary, start):
    rows = [{k: getattr(r, k) for k in ROW_FLAGS + ROW_VALUES + ("cost_change",)} for r in built.problem.iterations()]
    return Run(summary.as_dict(), rows, start, read_params(built), built)


def run_case(api, scene_name, fields, sync_every=1, prepare=None):
    """Build scene `scene_name` on `api`, solve it with the default options changed by `fields`, return the Run.
    prepare(built): called on the fresh handle before the solve (a shard, an exchange)."""
    built = syn.build_problem(api, scene(scene_name))
    if prepare is not None:
        prepare(built)
    start = read_params(built)
    return record(built, built.problem.solve(make_options(api, fields, sync_every)), start)


# ---- thresholds from the oracle's own log ----

NO_TOLERANCES = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)


@functools.lru_cache(maxsize=None)
def free_run(scene_name):
    """The oracle's log of the scene with nothing but the budget (30) to end the solve."""
    return run_case(helpers.oracle_api(), scene_name, dict(NO_TOLERANCES, max_num_iterations=30))


def start_reduced_norm(scene_name):
    """|x| over the parameters the solve moves, at the start (the x_norm of the parameter-tolerance test)."""
    sc = scene(scene_name)
    s = float(np.sum(np.asarray(sc.ctrl, float) ** 2))
    for sensor in sc.sensors:
        if sensor.enable_intrinsics:
            s += float(np.sum(np.asarray(sensor.intrinsics, float) ** 2))
        if sensor.enable_extrinsics:
            s += float(np.sum(np.asarray(sensor.t, float) ** 2) + np.sum(np.asarray(sensor.q, float) ** 2))
        if sensor.enable_latency:
            s += float(sensor.latency) ** 2
    return float(np.sqrt(s))


def deciding_quantity(scene_name, kind):
    """Per row of the free run, the quantity the ending of `kind` compares with its threshold (row 0: None where the quantity
    belongs to a step)."""
    rows = free_run(scene_name).rows
    if kind == "gradient":
        return [r["gradient_max_norm"] for r in rows]
    if kind == "parameter":
        return [None] + [r["step_norm"] for r in rows[1:]]
    if kind == "function":      # |cost_change| / x_cost, x_cost being the cost of the point the step started from
        assert all(r["step_is_successful"] for r in rows[1:8]), "the previous row's cost is only x_cost while every step is accepted"
        return [None] + [abs(r["cost_change"]) / rows[k]["cost"] for k, r in enumerate(rows[1:])]
    raise KeyError(kind)


def threshold_between(scene_name, kind, row):
    """The geometric mean of the deciding quantity of rows `row - 1` and `row`: rows before `row` stay above it, `row` falls
    below. Input condition: the two are at least a factor 10 apart, and no earlier row is below the threshold."""
    q = deciding_quantity(scene_name, kind)
    hi, lo = q[row - 1], q[row]
    assert hi >= 10.0 * lo > 0.0, "rows %d and %d of scene %s are not a factor 10 apart in %s: %r, %r" % (row - 1, row, scene_name, kind, hi, lo)
    t = float(np.sqrt(hi * lo))
    assert all(v is None or v > t for v in q[:row]), "an earlier row of scene %s is already below the %s threshold" % (scene_name, kind)
    return t


def parameter_tolerance_for(threshold, x_norm):
    """ptol with ptol (x_norm + ptol) = threshold (the positive root, in the form that does not cancel)."""
    return 2.0 * threshold / (x_norm + float(np.sqrt(x_norm * x_norm + 4.0 * threshold)))


# ---- the cases ----

Case = collections.namedtuple("Case", "name scene options message termination num_iterations untouched note")


def _opts(**kw):
    return lambda: dict(NO_TOLERANCES, **kw)


def _gradient_at(row):
    return lambda: dict(NO_TOLERANCES, max_num_iterations=30, gradient_tolerance=threshold_between("A", "gradient", row))


def _gradient_at_start():
    return dict(NO_TOLERANCES, max_num_iterations=30, gradient_tolerance=2.0 * free_run("A").rows[0]["gradient_max_norm"])


def _parameter_at(row):
    def make():
        ptol = parameter_tolerance_for(threshold_between("A", "parameter", row), start_reduced_norm("A"))
        return dict(NO_TOLERANCES, max_num_iterations=30, parameter_tolerance=ptol)
    return make


def _function_at(row):
    return lambda: dict(NO_TOLERANCES, max_num_iterations=30, function_tolerance=threshold_between("A", "function", row))


def _min_radius_above_start():
    return dict(NO_TOLERANCES, max_num_iterations=30, min_trust_region_radius=2.0 * helpers.oracle_api().default_options().initial_trust_region_radius)


def _invalid(limit):
    return _opts(max_num_iterations=30, min_lm_diagonal=0.0, max_num_consecutive_invalid_steps=limit)


CONV, NOCONV, FAIL = _capi.CONVERGENCE, _capi.NO_CONVERGENCE, _capi.FAILURE

# num_iterations is Summary::num_iterations = the last LOGGED iteration: the endings by parameter and function tolerance and by
# invalid steps do not log the iteration that ended them (as in Ceres), so a step of iteration 6 that ends the solve leaves 5.
CASES = [
    Case("A-gradient-5", "A", _gradient_at(5), MSG_GRADIENT, CONV, 5, False, "gradient tolerance between rows 4 and 5"),
    Case("A-gradient-6", "A", _gradient_at(6), MSG_GRADIENT, CONV, 6, False, "gradient tolerance between rows 5 and 6"),
    Case("A-gradient-0", "A", _gradient_at_start, MSG_GRADIENT, CONV, 0, True, "gradient tolerance above the initial gradient: the first post_eval ends the solve"),
    Case("A-parameter-6", "A", _parameter_at(6), MSG_PARAMETER, CONV, 5, False, "the step of iteration 6 is shorter than ptol (x_norm + ptol)"),
    Case("A-function-6", "A", _function_at(6), MSG_FUNCTION, CONV, 5, False, "the step of iteration 6 changes the cost by less than ftol x_cost"),
    Case("A-min-radius-0", "A", _min_radius_above_start, MSG_RADIUS, CONV, 0, True, "min_trust_region_radius = 2 x the initial radius"),
    Case("A-max-radius", "A", _opts(max_num_iterations=6, max_trust_region_radius=2e4), MSG_BUDGET, NOCONV, 6, False, "the radius is clamped to 2e4 from row 3 on"),
    Case("A-budget-0", "A", _opts(max_num_iterations=0), MSG_BUDGET, NOCONV, 0, True, "no iteration at all"),
    Case("A-budget-1", "A", _opts(max_num_iterations=1), MSG_BUDGET, NOCONV, 1, False, "one accepted step"),
    Case("A-budget-6", "A", _opts(max_num_iterations=6), MSG_BUDGET, NOCONV, 6, False, "six accepted steps"),
    Case("B-min-radius-4", "B", _opts(max_num_iterations=30, min_trust_region_radius=100.0), MSG_RADIUS, CONV, 4, True, "four rejections take the radius to 9.77 < 100"),
    Case("B-budget-2", "B", _opts(max_num_iterations=2), MSG_BUDGET, NOCONV, 2, True, "the last step of the budget is rejected"),
    Case("B-budget-8", "B", _opts(max_num_iterations=8), MSG_BUDGET, NOCONV, 8, False, "the last step of the budget is accepted"),
    Case("B-initial-failure", "B-behind", _opts(max_num_iterations=30), MSG_INITIAL_FAILURE, FAIL, 0, True, "a point behind the camera at the start: nothing is logged"),
    Case("C-invalid-1", "C", _invalid(1), MSG_INVALID_STEPS, FAIL, 0, True, "the first invalid step ends the solve"),
    Case("C-invalid-2", "C", _invalid(2), MSG_INVALID_STEPS, FAIL, 1, True, "the second"),
    Case("C-invalid-5", "C", _invalid(5), MSG_INVALID_STEPS, FAIL, 4, True, "the fifth (Ceres' default)"),
]
CASE_IDS = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    c = next(c for c in CASES if c.name == name)
    return run_case(helpers.oracle_api(), c.scene, c.options())


def oracle_run(case):
    """The oracle's Run of a case, computed once."""
    return _oracle_run(case.name)


# ---- the comparison rules ----

def relative_difference(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def assert_same_ending(got, ref, what=""):
    """Everything about an ending that is a whole number or a string: equal."""
    for k in SUMMARY_COUNTS + ("message",):
        assert got.summary[k] == ref.summary[k], "%s %s: %r, expected %r" % (what, k, got.summary[k], ref.summary[k])
    assert len(got.rows) == len(ref.rows), "%s log rows: %d, expected %d" % (what, len(got.rows), len(ref.rows))
    for a, b in zip(got.rows, ref.rows):
        for k in ROW_FLAGS:
            assert a[k] == b[k], "%s row %d %s: %r, expected %r" % (what, b["iteration"], k, a[k], b[k])


def assert_rows_close(got, ref, what="", first_rtol=1e-9, rtol=1e-6, worst=None):
    """Row 0 (the same point on both sides): cost and gradient_max_norm to first_rtol. Later rows: the logged columns to rtol;
    what a side shows as +-1.7976931348623157e308 (a candidate that cannot be evaluated) is that number exactly on both.
    worst: {column: largest relative difference seen}, updated."""
    assert len(got.rows) == len(ref.rows)
    for a, b in zip(got.rows, ref.rows):
        first = b["iteration"] == 0
        for k in (("cost", "gradient_max_norm") if first else ROW_VALUES):
            if abs(b[k]) >= DBL_MAX or abs(a[k]) >= DBL_MAX or not np.isfinite(b[k]):
                assert a[k] == b[k], "%s row %d %s: %r, expected exactly %r" % (what, b["iteration"], k, a[k], b[k])
                continue
            d = 0.0 if a[k] == b[k] else relative_difference(a[k], b[k])
            if worst is not None:
                key = ("row 0 " + k) if first else k
                worst[key] = max(worst.get(key, 0.0), d)
            assert d <= (first_rtol if first else rtol), "%s row %d %s: %r, expected %r (relative difference %.3e)" % (what, b["iteration"], k, a[k], b[k], d)
        if first:
            assert a["trust_region_radius"] == b["trust_region_radius"] and a["step_norm"] == 0.0 and a["relative_decrease"] == 0.0


def assert_estimates_close(got, ref, scene_name, what="", rtol=1e-6):
    """test_gpu_parity.assert_estimates_close's rule over every parameter block: a block agrees to rtol of its largest entry
    (at least 1e-3), the control points as one array to rtol of theirs (at least 1)."""
    sc = scene(scene_name)
    ctrl = set(int(b) for b in got.built.ctrl_blocks)
    assert set(got.params) == set(ref.params)
    for b, v in ref.params.items():
        if b in ctrl:
            continue
        scale = max(1e-3, np.abs(v).max())
        assert np.abs(got.params[b] - v).max() <= rtol * scale, "%s block %d: %r, expected %r" % (what, b, got.params[b], v)
    cg = np.stack([got.params[int(b)] for b in got.built.ctrl_blocks])
    cr = np.stack([ref.params[int(b)] for b in ref.built.ctrl_blocks])
    assert cg.shape == (len(sc.ctrl), 6)
    assert np.abs(cg - cr).max() <= rtol * max(1.0, np.abs(cr).max()), "%s control points: off by %.3e" % (what, np.abs(cg - cr).max())


def assert_untouched(run, what=""):
    """The parameters are the start's, bit for bit."""
    for b, v in run.start.items():
        assert np.array_equal(run.params[b], v), "%s block %d moved: %r, start %r" % (what, b, run.params[b], v)


def assert_costs_close(got, ref, what="", rtol=1e-8):
    """initial_cost and final_cost as test_gpu_edge_cases._compare has them (a FAILURE reports final_cost 0 on both sides)."""
    for k in ("initial_cost", "final_cost"):
        a, b = got.summary[k], ref.summary[k]
        assert abs(a - b) <= rtol * max(abs(b), 1e-300) or a == b, "%s %s: %r, expected %r" % (what, k, a, b)


def assert_run_matches(got, ref, case, what="", worst=None):
    """The whole comparison of one solve with the reference solve of the same case."""
    assert_same_ending(got, ref, what)
    assert_rows_close(got, ref, what, worst=worst)
    assert_costs_close(got, ref, what)
    assert_estimates_close(got, ref, case.scene, what)
    if case.untouched:
        assert_untouched(got, what)

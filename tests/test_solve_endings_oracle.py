"""The cases of solve_endings.py do on the CPU oracle what they were built for: every case ends with the termination type,
the reason string and the iteration count its row of the table states, its threshold sits between two rows of the oracle's own
log that are at least a factor 10 apart, and the log has num_iterations + 1 rows whatever ended the solve (the endings by
parameter and function tolerance and by invalid steps do not log the iteration that ended them, as in Ceres). The device's
loop forms are held to these runs by test_gpu_solve_endings.py; a case that does not meet its condition here is a wrong case."""
import numpy as np
import pytest

import helpers
import solve_endings as se
from calico_amd import synthetic as syn


@pytest.fixture(scope="module", autouse=True)
def _oracle_built(oracle):
    return oracle


@pytest.mark.parametrize("case", se.CASES, ids=se.CASE_IDS)
def test_case_ends_as_the_table_says(case):
    run = se.oracle_run(case)      # (building the options asserts the factor-10 condition of the case's threshold)
    s = run.summary
    assert (s["termination_type"], s["message"], s["num_iterations"]) == (case.termination, case.message, case.num_iterations), case.note
    if case.message == se.MSG_INITIAL_FAILURE:      # the one ending in front of row 0
        assert run.rows == [] and s["num_jacobian_evaluations"] == 1 and s["initial_cost"] == 0.0
        se.assert_untouched(run)
        return
    assert len(run.rows) == s["num_iterations"] + 1
    assert [r["iteration"] for r in run.rows] == list(range(len(run.rows)))
    assert s["num_successful_steps"] + s["num_unsuccessful_steps"] == s["num_iterations"]
    assert s["num_successful_steps"] == sum(r["step_is_successful"] for r in run.rows)
    assert s["num_jacobian_evaluations"] == 1 + s["num_successful_steps"]
    if case.untouched:
        se.assert_untouched(run)
        assert s["num_successful_steps"] == 0
    else:
        assert s["num_successful_steps"] > 0 and any(not np.array_equal(run.params[b], v) for b, v in run.start.items())


def test_scene_a_rows_are_far_apart_where_the_thresholds_sit():
    """Every step of the free run up to row 8 is accepted, and the rows a case puts its threshold between are a factor 10 apart
    in the deciding quantity (the gradient norm of rows 4/5, all three quantities of rows 5/6 and 6/7; the step norms of rows
    4/5 are only a factor 7 apart, and no case sits there): a threshold placed there ends the solve at the same iteration on
    two implementations that agree to 1e-6."""
    rows = se.free_run("A").rows
    assert all(r["step_is_valid"] and r["step_is_successful"] for r in rows[1:9])
    for kind, first in (("gradient", 5), ("parameter", 6), ("function", 6)):
        q = se.deciding_quantity("A", kind)
        for row in range(first, 8):
            assert q[row - 1] >= 10.0 * q[row] > 0.0, (kind, row, q[row - 1], q[row])
    # the start's reduced norm stands in for the x_norm of iteration 6: the steps up to there move it by far less than the
    # factor sqrt(10) the threshold keeps from either row
    steps = sum(r["step_norm"] for r in rows[1:7])
    assert steps < 0.5 * se.start_reduced_norm("A")


def test_gradient_and_step_endings_stop_where_the_threshold_says():
    """The tolerance cases against the free run: the rows up to the ending are the free run's rows, bit for bit (the tolerances
    only decide when to stop), and the quantity that ended the solve is below its threshold while the row before is above."""
    free = se.free_run("A").rows
    for name, kind, row in (("A-gradient-5", "gradient", 5), ("A-gradient-6", "gradient", 6), ("A-parameter-6", "parameter", 6),
                            ("A-function-6", "function", 6)):
        case = next(c for c in se.CASES if c.name == name)
        run = se.oracle_run(case)
        assert run.rows == free[:len(run.rows)], name
        assert len(run.rows) == (row + 1 if kind == "gradient" else row), name
        t = se.threshold_between("A", kind, row)
        q = se.deciding_quantity("A", kind)
        assert q[row] < t / 3.0 and q[row - 1] > 3.0 * t, name


def test_max_radius_clamps_and_min_radius_counts_rejections():
    run = se.oracle_run(next(c for c in se.CASES if c.name == "A-max-radius"))
    radii = [r["trust_region_radius"] for r in run.rows]
    assert radii[0] == 1e4 and 1.7e4 < radii[1] < radii[2] < 2e4 and radii[3:] == [2e4] * 4
    free = [r["trust_region_radius"] for r in se.free_run("A").rows]
    assert radii[1:3] == free[1:3] and free[3] > 2e4      # (the clamp is what changed the third radius)
    run = se.oracle_run(next(c for c in se.CASES if c.name == "B-min-radius-4"))
    assert [r["trust_region_radius"] for r in run.rows] == [1e4, 5e3, 1.25e3, 156.25, 9.765625]
    assert run.summary["num_successful_steps"] == 0 and run.summary["num_unsuccessful_steps"] == 4
    assert run.summary["final_cost"] == run.summary["initial_cost"]


def test_ladder_scene_rejects_six_steps_two_of_them_not_evaluable():
    rows = se.free_run("B").rows
    assert [r["step_is_successful"] for r in rows[1:8]] == [0, 0, 0, 0, 0, 0, 1]
    assert [r["iteration"] for r in rows if r["cost"] == se.DBL_MAX] == [4, 5]
    assert all(r["relative_decrease"] == -se.DBL_MAX for r in rows[4:6])
    # budget 2 ends on a rejected step, budget 8 on an accepted one
    assert rows[2]["step_is_successful"] == 0 and rows[8]["step_is_successful"] == 1


def test_invalid_step_scene_has_three_structurally_zero_columns():
    """Scene C: the gyroscope's lever arm is a free block no residual depends on. With min_lm_diagonal = 0 its damped pivots are
    exactly 0, the factorisation fails and every step is invalid: no cost evaluation, one Jacobian evaluation, the radius
    halved per logged row, FAILURE with final_cost 0."""
    built = syn.build_problem(helpers.oracle_api(), se.scene("C"))
    _, g, H = built.problem.evaluate()
    assert len(g) == 240
    assert list(np.where(np.diag(H) == 0.0)[0]) == [222, 223, 224]
    assert not H[222:225].any() and not H[:, 222:225].any() and not g[222:225].any()
    for limit, iterations in ((1, 0), (2, 1), (5, 4)):
        run = se.oracle_run(next(c for c in se.CASES if c.name == "C-invalid-%d" % limit))
        s = run.summary
        assert s["num_iterations"] == iterations and s["final_cost"] == 0.0 and s["initial_cost"] > 0.0
        assert s["num_jacobian_evaluations"] == 1 and s["num_cost_evaluations"] == 0
        assert s["num_successful_steps"] == 0 and s["num_unsuccessful_steps"] == iterations
        for k, r in enumerate(run.rows):
            assert r["trust_region_radius"] == 1e4 * 0.5 ** k
            assert r["cost"] == s["initial_cost"] and r["gradient_max_norm"] == run.rows[0]["gradient_max_norm"]
            if k:
                assert (r["step_is_valid"], r["step_is_successful"], r["step_norm"], r["relative_decrease"]) == (0, 0, 0.0, 0.0)


def test_every_reason_but_eleven_has_a_case():
    """Reason 11 (an ACCEPTED point cannot be evaluated)
    cannot be reached with the speculative evaluation, where the accepted point has been evaluated as a candidate already."""
    assert {c.message for c in se.CASES} == {se.MSG_INITIAL_FAILURE, se.MSG_BUDGET, se.MSG_GRADIENT, se.MSG_RADIUS, se.MSG_PARAMETER, se.MSG_FUNCTION,
                                            se.MSG_INVALID_STEPS}

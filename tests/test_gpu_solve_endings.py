"""The device's LM loop driven through every way a solve can end, in every form of the loop, against the CPU oracle (`-m gpu`).

Whichever stage ends a solve -- post_eval_body by the budget, the gradient tolerance, the minimum radius or a failed first
evaluation; control_body by the parameter tolerance, the function tolerance or too many invalid steps -- has to set
`terminated`, write state, log and parameters into pinned host memory and raise the progress word, and those stages ride in
different launches depending on the form of the loop. A wrong ending is not a slightly wrong number: the solve returns the
candidate instead of the last accepted point, the log has a row too many, the counters are stale, or the host spins until its
watchdog. So every case of solve_endings.py (scenes A, B, C; proved on the oracle by test_solve_endings_oracle.py) is solved in
every form:

  default                  streaming loop, tree solver: post_eval in level 0's extra workgroup (the first one too), the
                           control stage in the gather's last workgroup
  CALICO_PREDICT_END=0     the same, always one iteration ahead
  CALICO_STREAM_DEPTH=0    batched loop, stand-alone control / post_eval kernels, sync_every 1 and 4
  CALICO_SPECULATIVE=0     cost-first loop, sync_every 1 and 4
  CALICO_SOLVER=band       streaming loop, banded solver: post_eval rides in prepare
  world of one + identity all-reduce callback, CALICO_MULTIRANK_ASYNC 1 and 0, sync_every 4: commit_kernel instead of the
                           buffer swap

and compared with the oracle's solve of the same case (computed once per case):
  * equal: termination type, message, num_iterations, number of log rows, per row iteration / step_is_valid /
    step_is_successful, successful and unsuccessful steps, Jacobian and cost evaluations;
  * row 0: cost and gradient_max_norm to 1e-9 (the same point on both sides; gradient_max_norm is |x - Plus(x, -g)|, quaternion
    blocks included); later rows: cost, trust_region_radius, gradient_max_norm, step_norm, relative_decrease to 1e-6; what cannot
    be evaluated shows exactly 1.7976931348623157e308; the clamped radius is exactly 2e4;
  * every parameter block and the control points to 1e-6 (assert_estimates_close's rule) -- the parameter- and function-tolerance
    cases end at a step of 2e-2, a stage that committed the candidate would be off by four decades --, bit for bit the start
    where the ending must not have moved anything; initial_cost and final_cost to 1e-8;
  * across forms the whole numbers and strings are the default form's, and the default form repeats itself bit for bit;
  * after every ending, on the default form: evaluate() right behind the ended solve is the oracle's at the returned point
    (1e-9), and a second solve on the same handle from the re-set start walks the iterations of a fresh handle bit for bit (the
    epoch of the progress words, the `published` flag, the early-exit kernels left on the stream).

Reason 11 ("Residual and Jacobian evaluation failed.") has no case: it needs an ACCEPTED point that cannot be evaluated, and
with the speculative evaluation an accepted point has been evaluated as a candidate already; contriving one would test a
different code path than the one that ships.

Observed worst relative differences to the oracle over all cases and forms (MI355X, first run; the tolerances above are the
issue's and were not tuned to these): row 0 cost 7.7e-16, row 0 gradient_max_norm 6.4e-15; later rows cost 1.7e-10,
trust_region_radius 8.6e-13, gradient_max_norm 1.6e-7, step_norm 3.4e-10, relative_decrease 7.3e-8. Per form a solve (handle
built, solved, read back) took 1.1 - 5.7 ms. With the control stage of the commit before this file, the three invalid-step cases
fail on num_cost_evaluations (1, 2, 5 against 0; run on the default form)."""
import collections
import time

import numpy as np
import pytest

import solve_endings as se
from calico_amd import synthetic as syn

pytestmark = pytest.mark.gpu

Form = collections.namedtuple("Form", "name env sync_every exchange")
FORMS = [
    Form("default", {}, 1, False),
    Form("predict-end-0", {"CALICO_PREDICT_END": "0"}, 1, False),
    Form("batched-sync1", {"CALICO_STREAM_DEPTH": "0"}, 1, False),
    Form("batched-sync4", {"CALICO_STREAM_DEPTH": "0"}, 4, False),
    Form("cost-first-sync1", {"CALICO_SPECULATIVE": "0"}, 1, False),
    Form("cost-first-sync4", {"CALICO_SPECULATIVE": "0"}, 4, False),
    Form("band", {"CALICO_SOLVER": "band"}, 1, False),
    Form("exchange-async", {"CALICO_MULTIRANK_ASYNC": "1"}, 4, True),
    Form("exchange-sync", {"CALICO_MULTIRANK_ASYNC": "0"}, 4, True),
]
FORM_IDS = [f.name for f in FORMS]
SWITCHES = sorted({k for f in FORMS for k in f.env})

_runs = {}          # (case name, form name, repeat) -> Run
_seconds = {}       # form name -> [seconds spent in its solves (handle built, solved, read back), solves]
_worst = {}         # column -> largest relative difference to the oracle


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, (sec, n) in _seconds.items():
        print("solve endings, form %-18s %3d solves, %.3f s (%.1f ms each)" % (name, n, sec, 1e3 * sec / max(n, 1)))
    for col, d in sorted(_worst.items()):
        print("solve endings, worst relative difference to the oracle, %-24s %.3e" % (col, d))


def _identity_exchange(built):
    built.problem.set_shard(0, 1)
    built.problem.set_allreduce(lambda ctx, buf, n, strm: 0)      # one rank: the sum over ranks is the buffer itself


def _set_form(monkeypatch, form):
    """The form's switches and no other of the list: they are read when a handle is finalised or per solve, so every run
    builds a new handle behind this."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in form.env.items():
        monkeypatch.setenv(k, v)


def _device_run(hip, monkeypatch, case, form, repeat=0):
    key = (case.name, form.name, repeat)
    if key not in _runs:
        _set_form(monkeypatch, form)
        t0 = time.perf_counter()
        _runs[key] = se.run_case(hip, case.scene, case.options(), form.sync_every, _identity_exchange if form.exchange else None)
        acc = _seconds.setdefault(form.name, [0.0, 0])
        acc[0] += time.perf_counter() - t0
        acc[1] += 1
    return _runs[key]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("case", se.CASES, ids=se.CASE_IDS)
def test_ending_matches_the_oracle(hip, oracle, monkeypatch, case, form):
    ref = se.oracle_run(case)
    got = _device_run(hip, monkeypatch, case, form)
    what = "%s / %s:" % (case.name, form.name)
    assert (got.summary["termination_type"], got.summary["message"]) == (case.termination, case.message), what
    se.assert_run_matches(got, ref, case, what, worst=_worst)
    if case.name == "A-max-radius":
        assert [r["trust_region_radius"] for r in got.rows[3:]] == [2e4] * 4, what
    if case.scene == "B":
        shown = [r["iteration"] for r in got.rows if r["cost"] == se.DBL_MAX]
        assert shown == [k for k in (4, 5) if k < len(got.rows)], what


@pytest.mark.parametrize("case", se.CASES, ids=se.CASE_IDS)
def test_forms_agree_and_the_default_repeats_itself(hip, monkeypatch, case):
    first = _device_run(hip, monkeypatch, case, FORMS[0])
    again = _device_run(hip, monkeypatch, case, FORMS[0], repeat=1)
    se.assert_same_ending(again, first, case.name + " / default, second run:")
    assert again.rows == first.rows, "the default form's log differs between two runs"
    assert again.summary["initial_cost"] == first.summary["initial_cost"] and again.summary["final_cost"] == first.summary["final_cost"]
    for b, v in first.params.items():
        assert np.array_equal(again.params[b], v), "the default form's estimates differ between two runs (block %d)" % b
    for form in FORMS[1:]:
        se.assert_same_ending(_device_run(hip, monkeypatch, case, form), first, "%s / %s against the default form:" % (case.name, form.name))


_fresh = {}      # scene name -> (summary, rows, params) of the plain solve on a fresh handle


def _plain_solve(hip, built):
    s = built.problem.solve(se.make_options(hip, dict(max_num_iterations=15)))
    return se.record(built, s, None)


def _assert_evaluation_close(got, ref, rtol=1e-9):
    """[cost, g, H] of two backends at the same point. cost: relative. H: relative to the geometric mean of the two diagonal
    entries, the project's rule. g: entry i is a sum of J_ki r_k whose rounding error scales with sum |J_ki| |r_k| <=
    |J_i| |r| = sqrt(H_ii) sqrt(2 cost), not with the entry itself (near a minimum the sum cancels): relative to that bound."""
    (cg, gg, Hg), (cr, gr, Hr) = got, ref
    assert abs(cg - cr) <= rtol * abs(cr)
    d = np.sqrt(np.diag(Hr))
    d = np.where(d > 0, d, 1.0)      # structurally zero columns (the gyroscope's lever arm)
    assert np.all(np.abs(gg - gr) <= rtol * d * np.sqrt(2.0 * cr))
    assert np.all(np.abs(Hg - Hr) <= rtol * np.outer(d, d))


@pytest.mark.parametrize("case", se.CASES, ids=se.CASE_IDS)
def test_handle_goes_on_after_the_ending(hip, oracle, monkeypatch, case):
    _set_form(monkeypatch, FORMS[0])
    if case.scene not in _fresh:
        _fresh[case.scene] = _plain_solve(hip, syn.build_problem(hip, se.scene(case.scene)))
    fresh = _fresh[case.scene]
    built = syn.build_problem(hip, se.scene(case.scene))
    start = se.read_params(built)
    s = built.problem.solve(se.make_options(hip, case.options()))
    assert s.message.decode() == case.message
    if case.message != se.MSG_INITIAL_FAILURE:
        # evaluate() right behind the ended solve, against the oracle at the point the solve returned
        got = built.problem.evaluate()
        at = syn.build_problem(oracle, se.scene(case.scene))
        se.write_params(at, se.read_params(built))
        _assert_evaluation_close(got, at.problem.evaluate())
    # a second solve on the same handle, from the start: the iterations of a fresh handle, bit for bit
    se.write_params(built, start)
    again = _plain_solve(hip, built)
    se.assert_same_ending(again, fresh, case.name + ", second solve on the handle:")
    assert again.rows == fresh.rows, "the second solve's log differs from a fresh handle's"
    for k in ("initial_cost", "final_cost"):
        assert again.summary[k] == fresh.summary[k], k
    for b, v in fresh.params.items():
        assert np.array_equal(again.params[b], v), "the second solve's estimates differ from a fresh handle's (block %d)" % b

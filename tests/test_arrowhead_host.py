"""The arrowhead estimators (calico_camera_calibrate, calico_rig_calibrate) share one core, read from the sources: the device code
of calico_amd/csrc/arrowhead_dev.hpp, the control word's head LmControl (kernels.hpp) and the host's loop and resection start of
lm_host.hpp are defined once, and the two kernel files and the two host files hold no copy of them."""
import os
import re

import __graft_entry__ as entry

KERNEL_FILES = ("calib_kernels.hip", "rig_kernels.hip")


def _sources():
    return {f: open(os.path.join(entry.CSRC, f)).read() for f in sorted(os.listdir(entry.CSRC)) if f.endswith((".cpp", ".hip", ".hpp", ".h"))}


def test_the_kernel_files_hold_no_copy_of_the_shared_device_code():
    src = _sources()
    shared = src["arrowhead_dev.hpp"]
    for f in KERNEL_FILES:
        assert "kLmLambdaMax" not in src[f] and "lm_loop_decision(" not in src[f] and "lm_rule(" not in src[f], f
        assert '#include "arrowhead_dev.hpp"' in src[f] and '#include "resect_dev.hpp"' not in src[f], f
        for name in ("eliminate_frame_block(", "bty(", "sum_shares<", "chol_inverse_gram(", "lm_control_decide(", "lm_control_not_pd(",
                     "lm_control_finish(", "put_pose_out(", "slot_q("):
            assert name in src[f], (f, name)
        # what the shared functions hold is not written out again: the 6x6 solve, the sum over the shares, L^-1
        for copy in ("b[i] = v / W[6 * i + i]", "sum += act ? v : 0.0", "r < lane ? 0.0 :", "accepted == 0"):
            assert copy not in src[f] and copy in shared, (f, copy)
        # the retraction R <- exp([d]x) R is retract_pose's, in the evaluation's prologue and the rig's camera update alike
        assert "angle_axis_to_quat(" not in src[f] and "retract_pose(" in src[f], f
        for name in ("huber(", "gram_store<N>(", "put_slot_pose("):
            assert name in src[f], (f, name)
    assert "kLmLambdaMax" in shared and len(re.findall(r"angle_axis_to_quat\(", shared)) == 1
    # the resection takes the Huber weight, the retraction and the inverse of its 6x6 system from the same header
    for name in ("huber(", "retract_pose(", "chol_inverse_gram("):
        assert name in src["resect_kernels.hip"], name
    assert "angle_axis_to_quat(" not in src["resect_kernels.hip"]
    # the two Cholesky factorisations give different bits and stay two: the one by rows lives with the arrowhead code
    assert "bool lds_chol_rows(" in shared and "rig_chol" not in "".join(src.values())


def test_both_control_words_begin_with_the_shared_head():
    hdr = _sources()["kernels.hpp"]
    head = re.search(r"struct LmControl \{(.*?)\n\};", hdr, re.S).group(1)
    assert re.match(r"\s*int done;", head)      # the host polls the first field
    for field in ("status", "cur", "first", "redo", "iterations", "accepted", "final_ok", "frames_used", "pairs_used", "lambda", "step",
                  "initial_cost", "final_cost", "rms"):
        assert re.search(r"\b%s\b" % field, head), field
    for name in ("CalibControl", "RigControl"):
        assert re.search(r"struct %s \{\s*LmControl lm;" % name, hdr), name
        assert re.search(r"static_assert\(offsetof\(%s, lm\.done\) == 0" % name, hdr), name


def test_the_host_loop_and_the_resection_start_are_defined_once():
    src = _sources()
    assert [f for f, s in src.items() if "the device loop did not end" in s] == ["lm_host.hpp"]
    assert [f for f, s in src.items() if "PollCycles" in s] == ["lm_host.hpp"]
    for f in ("chart.cpp", "rig.cpp"):
        assert "run_device_lm(" in src[f] and "ResectRun " in src[f], f
    # a ResectArgs is made in one place, ResectRun::args
    made = [f for f, s in src.items() for _ in re.findall(r"\bResectArgs\s+\w+\s*(?:=|;|\{)", s)]
    assert made == ["lm_host.hpp"], made

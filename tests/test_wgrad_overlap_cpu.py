"""CPU (-m "not gpu"): the schedule of the weight-gradient overlap (csrc/wgrad_overlap_plan.hpp), checked as data."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wgrad_overlap_plan_orders_every_operand(tmp_path):
    """tests/native/wgrad_overlap_plan_check.cpp compiled for the host: for L in {1, 2, 3, 4, 5, 12, 24} the happens-before graph of
    a backward (caller-stream order, side-stream order, record -> wait) built from the plan header that runtime.hip executes.  Every
    buffer copy, slab region and gradient range that a layer's grouped weight-gradient launch or its slab reduce reads is written
    before it and not overwritten until after it, the join at the end of the embed stage orders every gradient and sq_partials write
    before the caller's next operation, a backward abandoned after its first layer leaves nothing in flight under the next one, and
    -- the checker's own check -- removing any single wait of the plan is reported as a violation."""
    exe = str(tmp_path / "wgrad_overlap_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "wgrad_overlap_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "wgrad overlap plan ok" in out.stdout, out.stdout[-3000:]
    for L in (1, 2, 3, 4, 5, 12, 24):
        assert f"L={L:2d}:" in out.stdout, out.stdout[-3000:]

"""The error behaviour of the camera entry points, pinned: pih_render, pih_render_ex, pih_render_cam, pih_render_view and pih_render_lit
(on a handle of either task) answer every call of the table in tests/render_error_cases.py with the return code and the exact
pih_last_error text that tools/record_render_errors.py recorded in tests/golden/render_errors.json -- NULL out, zero sizes, env ranges, a
misaligned out pointer, every flag bit alone, both formats, both camera frames, the device flags with NULL arrays, the handle of the wrong
task, the degenerate cameras, NaN and +inf in each camera word, the bad lights of tests/render_cases.py, double
faults (which of two simultaneous faults is reported), and good calls that return 0.  The file was recorded from the build before the
argument checks of pih_hip.hip were merged into shared helpers; a characterisation test: a difference is a change of behaviour.
The `env_count > 65535` branch is not in the table: a 3-env handle cannot reach it (the env range is tested first)."""
import json
import os

import pytest


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.mark.gpu
def test_codes_and_texts_equal_the_recording(torch_mod):
    from peg_in_hole_gym_amd.vec_env import PihVecEnv
    from tests import render_error_cases as R
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_errors.json")) as f:
        want = json.load(f)
    got = R.run_table(R.Handles(torch_mod, PihVecEnv(R.N), PihVecEnv(R.N, task_id=1)))
    assert [r[:2] for r in got] == [r[:2] for r in want], "the table and the recording list different cases"
    print("%d rows, %d with a non-zero return code" % (len(got), sum(r[2] != 0 for r in got)))
    for g, w in zip(got, want):
        assert g == w

"""The second seed of sets (i) and (ii) of the lane tests.  Everything is in tests/test_step_lane_equivalence.py:
one harness, one plain yardstick, the input sets and the assertions; this file only calls it.  It holds no parent
form of anything.  It keeps its name because its test ids are part of the suite's record."""
import pytest

import test_step_lane_equivalence as lane_tests
from test_step_lane_equivalence import lane  # noqa: F401  (the fixture; the harness is built once for both files)


@pytest.mark.parametrize("R,every,sets", lane_tests.WINDOW_CASES)
def test_valid_mask_window_patterns(lane, R, every, sets):
    lane_tests.window_patterns(lane, 1, 10, R, every, sets)


def test_window_patterns_eight_columns(lane):
    lane_tests.window_patterns(lane, 1, 8, 20, 16, ("default", "catalogue9"))


@pytest.mark.parametrize("R,n_boards", lane_tests.STEADY_CASES)
def test_steady_state_boards(lane, R, n_boards):
    lane_tests.steady_state_boards(lane, 1, R, n_boards)


def test_yardstick_is_the_oracle(lane):
    lane_tests.yardstick_is_the_oracle(lane, 1)

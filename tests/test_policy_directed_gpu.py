"""The population and softmax kernels (greedy_rows_kernel, play_linear_kernel, softmax_rows_kernel,
play_softmax_kernel) against the oracle on the directed boards, on the MI355X, at every kernel variant
(tests/policy_directed_cases.py)."""
import pytest

import policy_directed_cases as pd

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("C,R", pd.PICK_GEOMETRIES)
def test_greedy_rows(orc, C, R):
    pd.greedy_rows_directed(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", pd.PICK_GEOMETRIES)
def test_softmax_rows(orc, C, R):
    pd.softmax_rows_directed(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", pd.PLAY_GEOMETRIES)
def test_play_linear(orc, C, R):
    pd.play_linear_directed(DEV, orc, C, R)


@pytest.mark.parametrize("C,R,T,directed", pd.SOFTMAX_PLAY_SETTINGS)
def test_play_softmax(orc, C, R, T, directed):
    pd.play_softmax_directed(DEV, orc, C, R, T, directed)


@pytest.mark.parametrize("C,R,T,directed", pd.SOFTMAX_PLAY_SETTINGS)
def test_play_softmax_equals_composition(orc, C, R, T, directed):
    pd.play_softmax_composition_directed(DEV, orc, C, R, T, directed)

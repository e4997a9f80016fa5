"""tetris_hip_expand_envs against the oracle on the directed boards, on the MI355X: expand_kernel at every column count
and every (word, storage, chunk count) variant it is instantiated for, through the C-ABI
(tests/expand_directed_cases.py has the cases, the geometry list and the coverage conditions)."""
import pytest

import expand_cases as ec
import expand_directed_cases as ed

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEYS = sorted(ed.bk.KEY_CASES)


@pytest.mark.parametrize("C,R", ed.EXPAND_GEOMETRIES)
def test_two_generations(orc, C, R):
    ed.two_generations(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", ed.DIRECTION_GEOMETRIES)
def test_feature_directions(orc, C, R):
    ed.feature_directions(DEV, orc, C, R)


@pytest.mark.parametrize("C,R", ed.DRAWN_GEOMETRIES)
def test_drawn_same_for_every_child(orc, C, R):
    ed.drawn_same_for_every_child(DEV, orc, C, R)


@pytest.mark.parametrize("name", KEYS)
def test_drawn_at_key_edges(orc, name):
    ed.drawn_at_key_edges(DEV, orc, name)


@pytest.mark.parametrize("C,R,n", ed.SET_SIZE_CASES)
def test_bag_set_sizes(orc, C, R, n):
    ed.bag_set_sizes(DEV, orc, C, R, n)


@pytest.mark.parametrize("C,R", ed.TWO_PLY_GEOMETRIES)
def test_two_ply_vs_oracle(orc, C, R):
    ec.two_ply_vs_oracle(DEV, orc, C, R)

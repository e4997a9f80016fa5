"""The footprint of every C-ABI entry point on the CPU harness (tetris_host_*): the same argument lists, sizes and
masks as tests/test_footprint_gpu.py, so that a wrong pointer or size in a case shows here first."""
import pytest

import footprint_cases as fc


@pytest.fixture(scope="module")
def lib():
    import harness_backend
    return harness_backend.binding()


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("how,mode", fc.STEP_FORMS)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_step_family(lib, C, R, how, mode, B):
    fc.step_family(lib, "cpu", C, R, B, how, mode)


def test_step_gather_payload_first_512_lane_batch(lib):
    fc.step_family(lib, "cpu", 10, 20, fc.FIRST_512_TILE_BATCH, "gather", "policy")


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_step_many(lib, C, R, policy, B):
    fc.step_many(lib, "cpu", C, R, B, policy)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_reset(lib, C, R, masked, B):
    fc.reset(lib, "cpu", C, R, B, masked)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_refresh(lib, C, R, B):
    fc.refresh(lib, "cpu", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("with_all", [False, True])
@pytest.mark.parametrize("layout", fc.AFTER_LAYOUTS)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_afterstates(lib, C, R, layout, with_all, B):
    fc.afterstates(lib, "cpu", C, R, B, layout, with_all)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_policy_greedy(lib, C, R, B):
    fc.policy_greedy(lib, "cpu", C, R, B)


@pytest.mark.parametrize("B", fc.ROLLOUT_BATCHES)
@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_rollouts(lib, C, R, policy, B):
    fc.rollouts(lib, "cpu", C, R, B, policy)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_gather_envs(lib, C, R, B):
    fc.gather_envs(lib, "cpu", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_decode(lib, C, R, B):
    fc.decode(lib, "cpu", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_encode(lib, C, R, B):
    fc.encode(lib, "cpu", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
def test_pack_done_bits(lib, B):
    fc.pack_done_bits(lib, "cpu", B)


@pytest.mark.parametrize("B", fc.BATCHES)
def test_policy_random(lib, B):
    fc.policy_random(lib, "cpu", B)


@pytest.mark.parametrize("B", fc.BATCHES)
def test_numpy_bag_stream(lib, B):
    fc.numpy_bag_stream(lib, "cpu", B)

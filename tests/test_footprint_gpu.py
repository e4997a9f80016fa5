"""The footprint of every C-ABI entry point on the MI355X (tetris_hip_*): kernels whose grids are larger than the
batch must write nothing outside the sizes include/tetris_hip.h documents, and nothing inside them where it says
they write nothing.  The cases are those of tests/test_footprint_host.py.

On the kernel before the guard `(i & ~63u) < p.B` of step_kernel's done_bits store, exactly the gather-payload cases
failed here: every (geometry, B) of test_step_family[...-gather-*] and the 65537-env case, by 2-3 words past
done_bits on 256-lane tiles and 3-7 words on 512-lane tiles."""
import pytest

import footprint_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from tetris_amd import _lib
    old = _lib._install_test_backend(None)  # the real library, whatever a test before this module bound
    try:
        return _lib.load()
    finally:
        _lib._install_test_backend(old)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("how,mode", fc.STEP_FORMS)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_step_family(lib, C, R, how, mode, B):
    fc.step_family(lib, "cuda", C, R, B, how, mode)


def test_step_gather_payload_first_512_lane_batch(lib):
    fc.step_family(lib, "cuda", 10, 20, fc.FIRST_512_TILE_BATCH, "gather", "policy")


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_step_many(lib, C, R, policy, B):
    fc.step_many(lib, "cuda", C, R, B, policy)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_reset(lib, C, R, masked, B):
    fc.reset(lib, "cuda", C, R, B, masked)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_refresh(lib, C, R, B):
    fc.refresh(lib, "cuda", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("with_all", [False, True])
@pytest.mark.parametrize("layout", fc.AFTER_LAYOUTS)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_afterstates(lib, C, R, layout, with_all, B):
    fc.afterstates(lib, "cuda", C, R, B, layout, with_all)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_policy_greedy(lib, C, R, B):
    fc.policy_greedy(lib, "cuda", C, R, B)


@pytest.mark.parametrize("B", fc.ROLLOUT_BATCHES)
@pytest.mark.parametrize("policy", [0, 1])
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_rollouts(lib, C, R, policy, B):
    fc.rollouts(lib, "cuda", C, R, B, policy)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_gather_envs(lib, C, R, B):
    fc.gather_envs(lib, "cuda", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_decode(lib, C, R, B):
    fc.decode(lib, "cuda", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
@pytest.mark.parametrize("C,R", fc.GEOMETRIES)
def test_encode(lib, C, R, B):
    fc.encode(lib, "cuda", C, R, B)


@pytest.mark.parametrize("B", fc.BATCHES)
def test_pack_done_bits(lib, B):
    fc.pack_done_bits(lib, "cuda", B)


@pytest.mark.parametrize("B", fc.BATCHES)
def test_policy_random(lib, B):
    fc.policy_random(lib, "cuda", B)


@pytest.mark.parametrize("B", fc.BATCHES)
def test_numpy_bag_stream(lib, B):
    fc.numpy_bag_stream(lib, "cuda", B)

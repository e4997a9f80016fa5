"""The device bag at every set size and the draw keys at their 64-bit edges on the MI355X: the select table staged in
LDS, the in-kernel key derivation of step_many / play / the counted step, the parameter blocks and the MT19937 stream
kernel, through the C-ABI and VecTetris (tests/bag_key_cases.py has the cases, the geometry list and the coverage
conditions; tests/test_bag_keys_host.py lists what the oracle produced for them)."""
import pytest

import bag_key_cases as bk

pytestmark = pytest.mark.gpu

KEYS = sorted(bk.KEY_CASES)


# ---- 1. set sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_step_lockstep(orc, C, R, n):
    bk.step_lockstep("cuda", orc, C, R, n)


@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_step_many_random(orc, C, R, n):
    bk.step_many_random("cuda", orc, C, R, n)


@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_step_many_greedy(orc, C, R, n):
    bk.step_many_greedy("cuda", orc, C, R, n)


@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_masked_reset(orc, C, R, n):
    bk.masked_reset("cuda", orc, C, R, n)


@pytest.mark.parametrize("C,R", bk.TWELVE_CASES)
def test_rollouts(orc, C, R):
    bk.rollouts("cuda", orc, C, R)


@pytest.mark.parametrize("C,R", bk.TWELVE_CASES)
def test_play(orc, C, R):
    bk.play("cuda", orc, C, R)


@pytest.mark.parametrize("C,R", bk.TWELVE_CASES)
def test_play_sampled(orc, C, R):
    bk.play_sampled("cuda", orc, C, R)


def test_bit63_on_the_host(orc):
    assert bk.bit63_on_the_host("cuda", orc) > 0


def test_facade_mask_under_a_full_bag():
    bk.facade_mask_under_a_full_bag("cuda")


def test_geometry_list():
    """every geometry of the case list: one of each (word, storage, chunk rows) the variant choice can produce"""
    assert {(10, 20), (12, 20), (10, 24), (10, 40), (10, 45), (10, 6)} <= set(bk.LAYOUTS)
    assert set(bk.FULL_GEOMETRIES + bk.OTHER_GEOMETRIES) == set(bk.LAYOUTS)
    for (C, R), (word_bytes, packed, _) in bk.LAYOUTS.items():  # tetris_entry.hpp: kernel_variant
        assert word_bytes == (4 if R + 4 <= 31 else 8) and packed == (R + 4 <= 6 * word_bytes)
    assert [len(set(bk.piece_list(n))) for n in (8, 9, 12)] == [8, 9, 9]


# ---- 2. keys at their edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KEYS)
def test_keys_step(orc, name):
    bk.step_lockstep("cuda", orc, 10, 20, 12, steps=bk.KEY_STEPS, covered=False, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_step_many(orc, name):
    bk.step_many_random("cuda", orc, 10, 20, 12, steps=bk.KEY_STEPS, k_launch=bk.KEY_STEPS, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_play(orc, name):
    bk.play("cuda", orc, 10, 20, K=bk.KEY_STEPS, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_play_sampled(orc, name):
    bk.play_sampled("cuda", orc, 10, 20, K=bk.KEY_STEPS, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_sample_and_random_actions(orc, name):
    bk.keys_sample_and_random_actions("cuda", orc, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_reset_and_rollouts(orc, name):
    bk.keys_reset_and_rollouts("cuda", orc, **bk.KEY_CASES[name])


def test_keys_rollout_uid(orc):
    bk.keys_rollout_uid("cuda", orc)


def test_shards_across_the_wrap(orc):
    bk.shards_across_the_wrap("cuda", orc)


def test_graph_across_the_wrap(orc):
    bk.graph_across_the_wrap("cuda", orc)


# ---- 3. tetris_hip_numpy_bag_stream -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 13))
def test_numpy_bag_stream(orc, n):
    bk.numpy_bag_stream("cuda", orc, n)

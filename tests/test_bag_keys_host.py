"""The device bag at every set size and the draw keys at their 64-bit edges on CPU (harness backend): the per-env
bodies the kernels run, the C-ABI text and the host logic (tests/bag_key_cases.py has the cases, the geometry list and
the coverage conditions).

What the oracle produced on the piece lists of bag_key_cases.piece_list (B = 549, seed 7; 48 steps, 72 on boards of more
than 40 rows) -- episodes ended / deep third-nibble draws; every list index was seen at the step draw and after an
auto-reset in every entry:

    10x20  n=1 545  n=2 547  n=3 553  n=4 565  n=5 591  n=8 574  n=9 588  n=10 586 / 1322  n=11 569 / 2863
           n=12 572 / 4250
    10x6   n=1 1888  n=2 1877  n=3 2235  n=4 2292  n=5 2303  n=8 2333  n=9 2345  n=10 2334 / 1341  n=11 2256 / 2881
           n=12 2333 / 4386
    12x20  n=4 548  n=5 549  n=12 549 / 4278        10x24  n=4 549  n=5 550  n=12 549 / 4279
    10x40  n=4 123  n=5 188  n=12 140 / 4255        10x44  n=4 549  n=5 549  n=12 547 / 6402 (72 steps)
    10x45  n=4 546  n=5 545  n=12 546 / 6355 (72 steps; after 48: 26 / 48 / 29 episodes, below the floor of 100)"""
import pytest

import bag_key_cases as bk

KEYS = sorted(bk.KEY_CASES)


# ---- 1. set sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_step_lockstep(host_backend, orc, C, R, n):
    bk.step_lockstep("cpu", orc, C, R, n)


@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_step_many_random(host_backend, orc, C, R, n):
    bk.step_many_random("cpu", orc, C, R, n)


@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_step_many_greedy(host_backend, orc, C, R, n):
    bk.step_many_greedy("cpu", orc, C, R, n)


@pytest.mark.parametrize("C,R,n", bk.SET_SIZE_CASES)
def test_masked_reset(host_backend, orc, C, R, n):
    bk.masked_reset("cpu", orc, C, R, n)


@pytest.mark.parametrize("C,R", bk.TWELVE_CASES)
def test_rollouts(host_backend, orc, C, R):
    bk.rollouts("cpu", orc, C, R)


@pytest.mark.parametrize("C,R", bk.TWELVE_CASES)
def test_play(host_backend, orc, C, R):
    bk.play("cpu", orc, C, R)


@pytest.mark.parametrize("C,R", bk.TWELVE_CASES)
def test_play_sampled(host_backend, orc, C, R):
    bk.play_sampled("cpu", orc, C, R)


def test_bit63_on_the_host(host_backend, orc):
    assert bk.bit63_on_the_host("cpu", orc) > 0


def test_facade_mask_under_a_full_bag(host_backend):
    bk.facade_mask_under_a_full_bag("cpu")


def test_geometry_list():
    """every geometry of the case list: one of each (word, storage, chunk rows) the variant choice can produce"""
    assert {(10, 20), (12, 20), (10, 24), (10, 40), (10, 45), (10, 6)} <= set(bk.LAYOUTS)
    assert set(bk.FULL_GEOMETRIES + bk.OTHER_GEOMETRIES) == set(bk.LAYOUTS)
    for (C, R), (word_bytes, packed, _) in bk.LAYOUTS.items():  # tetris_entry.hpp: kernel_variant
        assert word_bytes == (4 if R + 4 <= 31 else 8) and packed == (R + 4 <= 6 * word_bytes)
    assert [len(set(bk.piece_list(n))) for n in (8, 9, 12)] == [8, 9, 9]


# ---- 2. keys at their edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KEYS)
def test_keys_step(host_backend, orc, name):
    bk.step_lockstep("cpu", orc, 10, 20, 12, steps=bk.KEY_STEPS, covered=False, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_step_many(host_backend, orc, name):
    bk.step_many_random("cpu", orc, 10, 20, 12, steps=bk.KEY_STEPS, k_launch=bk.KEY_STEPS, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_play(host_backend, orc, name):
    bk.play("cpu", orc, 10, 20, K=bk.KEY_STEPS, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_play_sampled(host_backend, orc, name):
    bk.play_sampled("cpu", orc, 10, 20, K=bk.KEY_STEPS, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_sample_and_random_actions(host_backend, orc, name):
    bk.keys_sample_and_random_actions("cpu", orc, **bk.KEY_CASES[name])


@pytest.mark.parametrize("name", KEYS)
def test_keys_reset_and_rollouts(host_backend, orc, name):
    bk.keys_reset_and_rollouts("cpu", orc, **bk.KEY_CASES[name])


def test_keys_rollout_uid(host_backend, orc):
    bk.keys_rollout_uid("cpu", orc)


def test_shards_across_the_wrap(host_backend, orc):
    bk.shards_across_the_wrap("cpu", orc)


def test_graph_across_the_wrap(host_backend, orc):
    bk.graph_across_the_wrap("cpu", orc)


# ---- 3. tetris_hip_numpy_bag_stream -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 13))
def test_numpy_bag_stream(host_backend, orc, n):
    bk.numpy_bag_stream("cpu", orc, n)

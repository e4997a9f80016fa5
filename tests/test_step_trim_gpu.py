"""step_kernel and step_many_kernel (in-kernel uniform policy) in lock step with the oracle after the trim of
the stamp (table row, unclamped padded scratch), and of the epilogue's counters: 48 steps with auto-reset,
every output and the boards, at the batch sizes where that code can go wrong -- a single lane, one env into a
second wave (ballots, counters), one env past a 512-env tile, and the first size on the 512-env-tile variant.

The oracle runs once per case and is shared by both tests.  Each seed was chosen on the CPU so that the ORACLE'S
run alone contains a cleared line, a finished game and a placement that touches the rightmost column (asserted
below from the oracle's outputs, never from the kernel's)."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc

K = 48
# (columns, rows, batch) -> seed
CASES = {
    (10, 20, 1): 7,
    (10, 20, 65): 0,
    (10, 20, 513): 0,
    (10, 20, 65537): 0,
    (5, 20, 513): 0,
    (8, 20, 513): 0,
    (12, 20, 513): 0,
    (10, 40, 513): 7,
}
IDS = ["%dx%d-B%d" % (c, r, b) for (c, r, b) in CASES]


def _cells_to_cols(cells):
    """int8 0/1 [B, rows, C] -> uint64 [B, C], bit r of word c = cell (r, c)   (orc.cells_to_cols, by bytes)"""
    bits = np.packbits(np.ascontiguousarray(cells.transpose(0, 2, 1)).view(np.uint8), axis=-1, bitorder="little")
    wide = np.zeros(bits.shape[:-1] + (8,), np.uint8)
    wide[..., :bits.shape[-1]] = bits
    return wide.view("<u8")[..., 0]


@functools.lru_cache(maxsize=None)
def oracle_run(C, R, B):
    """K steps of the oracle with its restatement of the built-in policy: per-step outputs, the boards after
    every step as column words [K, B, C], and what the run contains."""
    ref = orc.OracleVecEnv(C, R, B, auto_reset=True, seed=CASES[(C, R, B)], nthreads=0)
    wt = np.uint32 if R + 4 <= 32 else np.uint64
    out = dict(obs=np.zeros((K, B, 8), np.float32), reward=np.zeros((K, B), np.int32), done=np.zeros((K, B), np.uint8),
               lines=np.zeros((K, B), np.uint8), action=np.zeros((K, B), np.int32), n_valid=np.zeros((K, B), np.uint8),
               cols=np.zeros((K, B, C), wt))
    rightmost = False
    for t in range(K):
        before = ref.cells.copy()
        obs, rew, done, lines, n_bad = ref.step(None)
        assert n_bad == 0
        plain = (lines == 0) & (done == 0)  # the board is the old one plus the piece
        rightmost = rightmost or bool(((ref.cells[plain, :, C - 1] - before[plain, :, C - 1]) != 0).any())
        for k, v in (("obs", obs), ("reward", rew), ("done", done), ("lines", lines), ("action", ref.action),
                     ("n_valid", ref.n_valid)):
            out[k][t] = v
        out["cols"][t] = _cells_to_cols(ref.cells).astype(wt)
    out["has"] = dict(line=bool((out["lines"] >= 1).any()), done=bool(out["done"].any()), rightmost=rightmost)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _assert_run_contains(o):
    assert o["has"]["line"], "the oracle's run clears no line: choose another seed"
    assert o["has"]["done"], "the oracle's run ends no game: choose another seed"
    assert o["has"]["rightmost"], "the oracle's run places nothing in the rightmost column: choose another seed"


def _totals_want(o, B):
    return [0, int(o["done"].sum()), int(o["lines"].astype(np.int64).sum()), K * B]


def _cols_of(env):
    return env.columns().t().cpu().numpy().astype(np.uint64)  # [B, C]


@pytest.mark.gpu
@pytest.mark.parametrize("C,R,B", list(CASES), ids=IDS)
def test_step_kernel_lock_step_with_oracle(C, R, B):
    from tetris_amd import VecTetris
    o = oracle_run(C, R, B)
    _assert_run_contains(o)
    env = VecTetris(C, R, B, device="cuda:0", auto_reset=True, seed=CASES[(C, R, B)])
    for t in range(K):
        obs, rew, done, lines = env.step()
        assert np.array_equal(env.action.cpu().numpy(), o["action"][t]), "action, step %d" % t
        assert np.array_equal(obs.cpu().numpy(), o["obs"][t]), "obs, step %d" % t
        assert np.array_equal(rew.cpu().numpy(), o["reward"][t]), "reward, step %d" % t
        assert np.array_equal(done.cpu().numpy(), o["done"][t].astype(bool)), "done, step %d" % t
        assert np.array_equal(lines.cpu().numpy(), o["lines"][t]), "lines, step %d" % t
        assert np.array_equal(env.n_valid.cpu().numpy(), o["n_valid"][t]), "n_valid, step %d" % t
        assert np.array_equal(_cols_of(env), o["cols"][t].astype(np.uint64)), "boards, step %d" % t
    assert env.totals().cpu().numpy().tolist() == _totals_want(o, B)


@pytest.mark.gpu
@pytest.mark.parametrize("C,R,B", list(CASES), ids=IDS)
def test_step_many_kernel_lock_step_with_oracle(C, R, B):
    from tetris_amd import VecTetris
    o = oracle_run(C, R, B)
    _assert_run_contains(o)
    env = VecTetris(C, R, B, device="cuda:0", auto_reset=True, seed=CASES[(C, R, B)])
    tr = env.step_many(K, policy="random")
    for k in ("action", "obs", "reward", "lines", "n_valid"):
        assert np.array_equal(tr[k].cpu().numpy(), o[k]), k
    assert np.array_equal(tr["done"].cpu().numpy(), o["done"].astype(bool))
    assert np.array_equal(_cols_of(env), o["cols"][K - 1].astype(np.uint64)), "boards after the last step"
    assert env.totals().cpu().numpy().tolist() == _totals_want(o, B)

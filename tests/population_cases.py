"""Shared cases for the greedy play of a population of linear policies: tetris_hip_policy_greedy_rows and
tetris_hip_play_linear, VecTetris.greedy_actions(weights=[P, 8], rows=...) and VecTetris.play.  Each takes the torch
device: "cuda" (tests/test_population_gpu.py, the HIP kernels) or "cpu" with the harness backend
(tests/test_population_host.py, the same per-env bodies compiled by g++).

The yardsticks are the existing calls with ONE weight vector -- tetris_hip_policy_greedy, step_many(policy="greedy")
-- and the oracle (afterstate features evaluated in NumPy float32, left to right; OracleVecEnv.step)."""
import ctypes

import numpy as np
import pytest
import torch

import directed_boards
import footprint_cases as fc

STANDARD7 = ["Straight", "RCorner", "LCorner", "Square", "SnakeR", "SnakeL", "T"]
GEOMETRIES = [
    pytest.param(10, 20, "default", id="10x20-u32-packed"),
    pytest.param(10, 40, STANDARD7, id="10x40-u64-packed-standard7"),
    pytest.param(6, 10, "default", id="6x10-unpacked"),
    pytest.param(12, 20, STANDARD7, id="12x20-12-bit-fields-standard7"),
]
B = 197                 # three tiles and a tail of 5
B_MULTI = 2 * 512 + 37  # 10x20: two workgroups of the play kernel (512 envs each) and a tail
BCTS = np.asarray([-24.04, -19.77, -13.08, -12.63, -10.49, -9.22, 6.6, -1.61], np.float32)  # game.py:111-118
INT32_MIN = -2**31


def weight_rows(seed=0):
    """float32 [7, 8]: BCTS, its negation, zeros (every placement ties: the lowest index wins), four random rows"""
    rng = np.random.RandomState(seed)
    return np.concatenate([BCTS[None], -BCTS[None], np.zeros((1, 8), np.float32),
                           (rng.randn(4, 8) * 10).astype(np.float32)]).astype(np.float32)


def random_rows(n, P, seed):
    return np.random.RandomState(seed).randint(0, P, size=n).astype(np.int32)


def _t(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), device=device)


def _env(device, C, R, pieces, n, seed, steps=12, **kw):
    """n envs after `steps` random steps without auto-reset (on small boards some games are over by then)"""
    from tetris_amd import VecTetris
    env = VecTetris(C, R, n, device=device, pieces=pieces, auto_reset=False, seed=seed, **kw)
    for _ in range(steps):
        env.step()
    env.status.zero_()  # (a random step of an env that is over counts as invalid: not this file's business)
    return env


def _with_directed_boards(env):
    """the first envs get the hand-built boards of directed_boards.structured (current pieces kept)"""
    boards = directed_boards.structured(env.num_rows, env.num_columns, 1)
    directed_boards.check_boards(boards, env.num_rows)
    n = min(len(boards), env.batch_size // 2)
    cells = env.boards().clone()
    cells[:n] = _t(boards[:n], env.device)
    env.set_boards(cells)
    return n


def snapshot(env):
    return dict(cols=env.cols.clone(), meta=env.meta.clone(), n_valid=env.n_valid.clone(), piece=env.piece.clone(),
                status=env.status.clone())


def lanes(cols, envs):
    """rows [len(envs), n_planes] of a raw cols tensor: every stored word of those envs"""
    return cols[envs // 64, :, envs % 64]


def raw_play(env, K, weights, rows, lines, pieces, n_valid=None, piece=None, status=None, step_idx0=None):
    """one tetris_hip_play_linear launch on env's storage; the caller owns every output"""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = env._lib.play_linear(ctypes.byref(env.desc), p(env.cols), p(env.meta), K, p(weights), weights.shape[0], p(rows),
                              p(lines), p(pieces), p(n_valid), p(piece), p(status), env.seed,
                              env.step_idx if step_idx0 is None else step_idx0, env.env_offset, env.batch_size,
                              env._hip_stream())
    assert rc == 0, rc


def raw_greedy_rows(env, weights, rows, best_action, best_value=None, status=None):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = env._lib.policy_greedy_rows(ctypes.byref(env.desc), p(env.cols), p(env.meta), p(weights), weights.shape[0],
                                     p(rows), p(best_action), p(best_value), p(status), env.batch_size, env._hip_stream())
    assert rc == 0, rc


def totals(env):
    z = lambda: torch.zeros(env.batch_size, dtype=torch.int32, device=env.device)
    return z(), z()


# ---- the NumPy yardstick of the pick ------------------------------------------------------------------------
def numpy_pick(feats, nv, w):
    """feats [B, A, 8] float32 (rows >= nv are padding), w [B, 8] float32 -> (best_action int32 [B], best_value
    float32 [B]): float32 products summed left to right (NumPy rounds every operation: no FMA), first maximum."""
    assert feats.dtype == np.float32 and w.dtype == np.float32
    acc = feats[:, :, 0] * w[:, None, 0]
    for q in range(1, 8):
        acc = acc + feats[:, :, q] * w[:, None, q]
    assert acc.dtype == np.float32
    valid = np.arange(feats.shape[1])[None, :] < nv[:, None]
    best = np.argmax(np.where(valid, acc, -np.inf), axis=1).astype(np.int32)  # (the first of equal maxima)
    value = acc[np.arange(len(best)), best]
    none = nv == 0
    return np.where(none, -1, best).astype(np.int32), np.where(none, np.float32(0), value).astype(np.float32)


def oracle_twin(orc, env, pieces):
    """an OracleVecEnv holding env's boards, pieces and bags, with its seed / step index"""
    ref = orc.OracleVecEnv(env.num_columns, env.num_rows, env.batch_size, pieces=pieces, auto_reset=False, seed=env.seed,
                           env_offset=env.env_offset, nthreads=0)
    ref.cells[:] = env.boards().cpu().numpy()
    ref.piece[:] = env.piece.cpu().numpy()
    ref.bag[:] = ((env.meta.cpu().numpy().view(np.uint64) >> np.uint64(52)) & np.uint64(0xFFF)).astype(np.uint16)
    ref.step_idx = env.step_idx
    return ref


# ---- 1. the pick ------------------------------------------------------------------------------------------------
def pick(device, C, R, pieces, rows_mode, orc=None):
    env = _env(device, C, R, pieces, B, seed=5)
    assert _with_directed_boards(env) >= 20
    W = weight_rows()
    rows = random_rows(B, len(W), seed=B)
    assert set(rows.tolist()) == set(range(len(W)))
    if rows_mode == "rows":
        got = env.greedy_actions(weights=_t(W, device), rows=_t(rows, device))
    else:  # rows = NULL: env i uses row i of a [B, 8] matrix
        got = env.greedy_actions(weights=_t(W[rows], device))
    ba, bv = (t.clone() for t in got)
    rows_t = _t(rows, device)
    for r in range(len(W)):  # tetris_hip_policy_greedy, once per distinct row, on the envs using it
        a, v = env.greedy_actions(weights=W[r].tolist())
        mine = rows_t == r
        assert torch.equal(ba[mine], a[mine]), "row %d" % r
        assert torch.equal(bv[mine].view(torch.int32), v[mine].view(torch.int32)), "row %d" % r
    assert int((ba == -1).sum()) == int((env.n_valid == 0).sum())
    assert bool(((ba >= 0) == (env.n_valid > 0)).all())
    assert env.stats()["invalid"] == 0
    if orc is not None:  # the oracle's features, evaluated in NumPy
        ref = oracle_twin(orc, env, pieces)
        feats, nv, _, _ = ref.afterstates()
        assert np.array_equal(nv, env.n_valid.cpu().numpy())
        want_a, want_v = numpy_pick(feats, nv, W[rows])
        assert np.array_equal(ba.cpu().numpy(), want_a)
        assert np.array_equal(bv.cpu().numpy(), want_v)
        zero = rows == 2  # all-zero weights: every placement ties, the lowest index wins
        assert np.array_equal(want_a[zero & (nv > 0)], np.zeros(int((zero & (nv > 0)).sum()), np.int32))


# ---- 2. play equals step_many ---------------------------------------------------------------------------------------
def play_equals_step_many(device, C, R, pieces, n=B, K=24, w=BCTS):
    env = _env(device, C, R, pieces, n, seed=9)
    twin = env.fork(torch.arange(n))
    nv0 = env.n_valid.clone()
    Wm = _t(np.tile(np.asarray(w, np.float32)[None], (3, 1)), device)  # every row the same vector
    rows = _t(random_rows(n, 3, seed=1), device)
    lines, pcs = totals(env)
    n_valid, piece = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
    raw_play(env, K, Wm, rows, lines, pcs, n_valid, piece, env.status)
    out = twin.step_many(K, policy="greedy", weights=[float(x) for x in w])
    assert torch.equal(env.cols, twin.cols) and torch.equal(env.meta, twin.meta)
    assert torch.equal(n_valid, out["n_valid"][K - 1]) and torch.equal(piece, out["piece"][K - 1])
    before = torch.cat([nv0[None], out["n_valid"][:-1]])  # n_valid in front of step k: 0 = that step was invalid
    valid = before > 0
    assert torch.equal(lines.long(), (out["lines"].long() * valid).sum(0))
    assert torch.equal(pcs.long(), valid.sum(0))
    assert torch.equal(valid, out["action"] >= 0)
    got, want = env.status.view(-1, 4), twin.status.view(-1, 4)
    assert torch.equal(got[:, 1:], want[:, 1:])       # episodes, lines, steps: step_many's
    assert int(got[:, 0].sum()) == 0                  # a frozen env is not invalid (step_many counts its steps)
    assert int(want[:, 0].sum()) == int((~valid).sum())
    return int(valid.sum()), int((~valid).sum())


# ---- 3. play against the oracle, distinct rows ---------------------------------------------------------------------
ORACLE_PLAY = {(10, 20): dict(K=40, seed=21), (6, 10): dict(K=14, seed=21)}


def oracle_play_rows(n):
    """three envs in eight on the BCTS row, the rest spread over the other six"""
    rows = np.where(np.arange(n) % 8 < 3, 0, 1 + np.arange(n) % 6).astype(np.int32)
    return rows


def oracle_play(orc, C, R, pieces, K, seed, n=B):
    """(ref, lines, pieces placed, over_before_K, alive_after_K): the oracle plays K greedy steps, every env on its
    own row by numpy_pick; envs without a valid action are skipped"""
    ref = orc.OracleVecEnv(C, R, n, pieces=pieces, auto_reset=False, seed=seed, nthreads=0)
    W, rows = weight_rows(), oracle_play_rows(n)
    lines, placed = np.zeros(n, np.int64), np.zeros(n, np.int64)
    over_before = None
    for k in range(K):
        feats, nv, _, _ = ref.afterstates()
        if k == K - 1:
            over_before = nv == 0
        action, _ = numpy_pick(feats, nv, W[rows])
        _, _, _, ln, n_bad = ref.step(action)
        alive = nv > 0
        assert n_bad == int((~alive).sum())
        lines += np.where(alive, ln, 0)
        placed += alive
    return ref, lines, placed, over_before, ref.n_valid > 0


def play_vs_oracle(device, orc, C, R, pieces):
    from tetris_amd import VecTetris
    K, seed = ORACLE_PLAY[(C, R)]["K"], ORACLE_PLAY[(C, R)]["seed"]
    ref, want_lines, want_placed, over_before, alive_after = oracle_play(orc, C, R, pieces, K, seed)
    # on the oracle's side: a quarter of the games are over before step K, a quarter still run after it
    assert over_before.mean() >= 0.25 and alive_after.mean() >= 0.25, (over_before.mean(), alive_after.mean())
    env = VecTetris(C, R, B, device=device, pieces=pieces, auto_reset=True, seed=seed)  # (play ignores auto_reset)
    res = env.play(_t(weight_rows(), device), rows=_t(oracle_play_rows(B), device), max_steps=K, chunk=K)
    assert env.step_idx == K
    assert np.array_equal(env.boards().cpu().numpy(), ref.cells)
    assert np.array_equal(env.piece.cpu().numpy(), ref.piece)
    assert np.array_equal(env.n_valid.cpu().numpy(), ref.n_valid)
    assert np.array_equal(res["lines"].cpu().numpy().astype(np.int64), want_lines)
    assert np.array_equal(res["pieces"].cpu().numpy().astype(np.int64), want_placed)
    assert np.array_equal(res["done"].cpu().numpy(), ~alive_after)
    s = env.stats()
    assert (s["invalid"], s["episodes"], s["lines"], s["steps"]) == (0, int((~alive_after).sum()), int(want_lines.sum()),
                                                                   int(want_placed.sum()))


# ---- 4. chunks compose ------------------------------------------------------------------------------------------------
def chunks_compose(device, C, R, pieces, a=5, b=11):
    one = _env(device, C, R, pieces, B, seed=13)
    two = one.fork(torch.arange(B))
    Wm, rows = _t(weight_rows(), device), _t(random_rows(B, 7, seed=2), device)
    l1, p1 = totals(one)
    l2, p2 = totals(two)
    nv1, pc1, nv2, pc2 = (torch.full_like(one.n_valid, 77) for _ in range(4))
    raw_play(one, a + b, Wm, rows, l1, p1, nv1, pc1, one.status)
    raw_play(two, a, Wm, rows, l2, p2, nv2, pc2, two.status)
    assert int(p2.sum()) > 0 and not torch.equal(p2, p1)
    raw_play(two, b, Wm, rows, l2, p2, nv2, pc2, two.status, step_idx0=two.step_idx + a)
    assert torch.equal(one.cols, two.cols) and torch.equal(one.meta, two.meta)
    assert torch.equal(l1, l2) and torch.equal(p1, p2) and torch.equal(nv1, nv2) and torch.equal(pc1, pc2)
    assert torch.equal(one.status, two.status)
    assert int(p1.max()) > a  # some env played on in the second launch


# ---- 5. frozen envs -------------------------------------------------------------------------------------------------
def frozen_envs(device, C=6, R=10, pieces="default", K=9):
    env = _env(device, C, R, pieces, B, seed=17, steps=0)
    Wm = _t(weight_rows(), device)
    rows = _t(np.where(np.arange(B) % 2 == 0, 1, 0).astype(np.int32), device)  # negated BCTS: over within a few pieces
    lines, pcs = totals(env)
    raw_play(env, 12, Wm, rows, lines, pcs, env.n_valid, env.piece, env.status)
    env.step_idx += 12
    over = env.n_valid == 0
    assert B // 4 <= int(over.sum()) < B
    before, l0, p0 = snapshot(env), lines.clone(), pcs.clone()
    nv, pc = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
    raw_play(env, K, Wm, rows, lines, pcs, nv, pc, env.status)
    idx = torch.nonzero(over).flatten()
    assert torch.equal(lanes(env.cols, idx), lanes(before["cols"], idx))
    assert torch.equal(env.meta[idx], before["meta"][idx])
    assert torch.equal(lines[idx], l0[idx]) and torch.equal(pcs[idx], p0[idx])
    assert torch.equal(env.status.view(-1, 4)[:, 0], before["status"].view(-1, 4)[:, 0])  # frozen is not invalid
    assert int(env.status.view(-1, 4)[:, 0].sum()) == 0
    assert int(nv[idx].max()) == 0 and torch.equal(pc[idx], before["piece"][idx])  # n_valid 0 = game over
    alive = torch.nonzero(~over).flatten()
    assert bool((pcs[alive] > p0[alive]).all())  # every other env moved
    steps = env.status.view(-1, 4)[:, 3].sum() - before["status"].view(-1, 4)[:, 3].sum()
    assert int(steps) == int((pcs - p0).sum())


# ---- 6. rows outside [0, P) ------------------------------------------------------------------------------------------
def bad_rows(device, C, R, pieces, n_steps):
    env = _env(device, C, R, pieces, B, seed=19)
    W = weight_rows()
    P = len(W)
    rows = random_rows(B, P, seed=3)
    bad = {5: -1, 70: P, B - 1: INT32_MIN}  # wave 0, wave 1, the last lane of the partial tile
    for j, v in bad.items():
        rows[j] = v
    Wm, rows_t = _t(W, device), _t(rows, device)
    bad_idx = torch.as_tensor(sorted(bad), device=device)
    want = np.zeros(env.status.numel() // 4, np.int64)
    for j in bad:
        want[j >> 6] += 1
    # the pick
    ba = torch.full((B,), -7, dtype=torch.int32, device=device)
    bv = torch.full((B,), -7.0, dtype=torch.float32, device=device)
    raw_greedy_rows(env, Wm, rows_t, ba, bv, env.status)
    assert ba[bad_idx].tolist() == [-7] * 3 and bv[bad_idx].tolist() == [-7.0] * 3
    good = torch.ones(B, dtype=torch.bool, device=device)
    good[bad_idx] = False
    assert bool((ba[good] != -7).all())
    assert np.array_equal(env.status.view(-1, 4)[:, 0].cpu().numpy(), want)
    # the play: the env and every output untouched, counted once whatever n_steps is
    env.status.zero_()
    before = snapshot(env)
    lines, pcs = (torch.full((B,), 1000, dtype=torch.int32, device=device) for _ in range(2))
    nv, pc = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
    raw_play(env, n_steps, Wm, rows_t, lines, pcs, nv, pc, env.status)
    assert torch.equal(lanes(env.cols, bad_idx), lanes(before["cols"], bad_idx))
    assert torch.equal(env.meta[bad_idx], before["meta"][bad_idx])
    for t, sentinel in ((lines, 1000), (pcs, 1000), (nv, 99), (pc, 99)):
        assert t[bad_idx].tolist() == [sentinel] * 3
    alive = good & (before["n_valid"] > 0)
    assert bool((pcs[alive] > 1000).all()) and bool((nv[good] != 99).all())
    assert np.array_equal(env.status.view(-1, 4)[:, 0].cpu().numpy(), want)
    with pytest.raises(IndexError):
        env.check()


# ---- 7. footprint (the method of footprint_cases.py) -----------------------------------------------------------------
FOOTPRINT_BATCHES = [197, 65, 513]  # B = 197 and B = 64 k + 1
GREEDY_ROWS_OPTIONAL = ["none", "rows", "best_value", "status"]
PLAY_OPTIONAL = ["none", "rows", "n_valid", "piece", "status"]


def _population_inputs(n, device, null_rows):
    """(weights, rows, bad): without a row list the matrix has one row per env and no row can be out of range"""
    W = weight_rows()
    rows = random_rows(n, len(W), seed=n)
    if null_rows:
        return _t(W[rows], device), None, torch.zeros(n, dtype=torch.bool, device=device)
    bad = fc._one_per_wave(n, device)
    rows_t = _t(rows, device)
    rows_t[bad] = torch.where((torch.arange(n, device=device) // 64)[bad] % 2 == 0, len(W), -1).to(torch.int32)
    return _t(W, device), rows_t, bad


def footprint_greedy_rows(device, C, R, n, null_arg):
    from tetris_amd import _lib
    lib = _lib.load()
    geo, st = fc.state(lib, device, C, R, n)
    Wm, rows, bad = _population_inputs(n, device, null_arg == "rows")

    def call(A):
        A.launch(lib.policy_greedy_rows, geo.d, A.new("cols", init=st["cols"], keep=True), A.new("meta", init=st["meta"], keep=True),
                 A.new("weights", init=Wm, keep=True), Wm.shape[0], A.new("rows", init=rows, keep=True) if rows is not None else None,
                 A.new("best_action", 4 * n, keep=fc._elems(bad, 4)),
                 A.new("best_value", 4 * n, keep=fc._elems(bad, 4)) if null_arg != "best_value" else None,
                 A.new("status", init=st["status"]) if null_arg != "status" else None, n, None)

    g, _ = fc.footprint(device, call)
    if null_arg not in ("status", "rows"):
        invalid = g.bufs["status"].body.view(torch.int32).view(-1, 4)[:, 0] - st["status"].view(-1, 4)[:, 0]
        assert int(invalid.sum()) == int(bad.sum()) > 0


def footprint_play(device, C, R, n, null_arg, K=3):
    from tetris_amd import _lib
    lib = _lib.load()
    geo, st = fc.state(lib, device, C, R, n)
    Wm, rows, bad = _population_inputs(n, device, null_arg == "rows")
    k1, k4 = fc._elems(bad, 1), fc._elems(bad, 4)
    start = torch.arange(n, dtype=torch.int32, device=device) + 1000

    def call(A):
        A.launch(lib.play_linear, geo.d, A.new("cols", init=st["cols"], keep=geo.kept_lanes(n, bad, device)),
                 A.new("meta", init=st["meta"], keep=fc._elems(bad, 8)), K, A.new("weights", init=Wm, keep=True), Wm.shape[0],
                 A.new("rows", init=rows, keep=True) if rows is not None else None,
                 A.new("lines_total", init=start, keep=k4), A.new("pieces_total", init=start, keep=k4),
                 A.new("n_valid", init=st["n_valid"] + 100, keep=k1) if null_arg != "n_valid" else None,
                 A.new("piece", init=st["piece"] + 100, keep=k1) if null_arg != "piece" else None,
                 A.new("status", init=st["status"]) if null_arg != "status" else None, fc.SEED, st["step_idx"], 0, n, None)

    g, _ = fc.footprint(device, call)
    assert not torch.equal(g.bufs["meta"].body, g.bufs["meta"].before)
    placed = g.bufs["pieces_total"].body.view(torch.int32) - start
    assert int(placed[bad].abs().sum()) == 0 and bool(((placed[~bad] >= 1) & (placed[~bad] <= K)).all())
    assert int(placed.max()) == K


# ---- 8. the facade ------------------------------------------------------------------------------------------------------
def facade(device):
    from tetris_amd import VecTetris
    # every game ends: play stops early, after whole chunks
    env = VecTetris(6, 10, B, device=device, auto_reset=True, seed=23)
    Wm = _t(weight_rows(), device)
    all_negated = torch.ones(B, dtype=torch.int32, device=device)
    res = env.play(Wm, rows=all_negated, max_steps=4096, chunk=8)
    assert bool(res["done"].all()) and int(env.n_valid.max()) == 0
    assert 8 <= env.step_idx < 4096 and env.step_idx % 8 == 0
    longest = int(res["pieces"].cpu().numpy().astype(np.int64).max())
    assert env.step_idx - 8 < longest <= env.step_idx  # the chunk in which the last game ended was the last one
    assert res["lines"].dtype == torch.uint32 and res["pieces"].dtype == torch.uint32 and res["done"].dtype == torch.bool
    assert env.stats()["episodes"] == B and env.stats()["invalid"] == 0
    assert not bool(env.boards().sum(dim=(1, 2)).eq(0).any())  # auto_reset is ignored: no board was emptied
    again = env.play(Wm, rows=all_negated, max_steps=16, chunk=8)  # all over: one launch, nothing moves
    assert env.step_idx == longest_chunk(longest, 8) + 8 and int(again["pieces"].cpu().numpy().astype(np.int64).sum()) == 0

    # max_steps stops it otherwise (a last chunk of 4); a following step() continues exactly as the twin does
    env = _env(device, 10, 20, "default", B, seed=29, steps=3)
    twin = env.fork(torch.arange(B))
    feats_before = env.get_after_states()[0].clone()
    rows = _t(random_rows(B, 7, seed=4), device)
    res = env.play(Wm, rows=rows, max_steps=20, chunk=8)
    assert env.step_idx == twin.step_idx + 20
    lines, pcs = totals(twin)
    raw_play(twin, 20, Wm, rows, lines, pcs, twin.n_valid, twin.piece, twin.status)
    twin.step_idx += 20
    assert torch.equal(res["lines"].view(torch.int32), lines) and torch.equal(res["pieces"].view(torch.int32), pcs)
    assert torch.equal(res["done"], twin.n_valid == 0) and not bool(res["done"].all())
    assert torch.equal(env.n_valid, twin.n_valid) and torch.equal(env.piece, twin.piece)
    # afterstates asked for now describe the boards after the play, not the ones before it
    feats, nv = env.get_after_states()
    want_feats, want_nv = twin.get_after_states()
    assert torch.equal(feats.view(torch.int32), want_feats.view(torch.int32)) and torch.equal(nv, want_nv)
    assert torch.equal(nv, env.n_valid) and not torch.equal(feats, feats_before)
    env.check()
    a = twin.random_actions().clone()
    assert torch.equal(env.random_actions(), a)
    for g, w in zip(env.step(a), twin.step(a)):
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
    assert torch.equal(env.cols, twin.cols) and torch.equal(env.meta, twin.meta)
    assert env.step_idx == twin.step_idx and env.stats() == twin.stats()

    # refusals of the host
    replay = VecTetris(10, 20, B, device=device, piece_stream=np.zeros((8, B), dtype=np.uint8))
    with pytest.raises(ValueError, match="replay"):
        replay.play(Wm, rows=rows)
    for bad_w in (Wm[:, :7], Wm[0], Wm.tolist()):
        with pytest.raises(ValueError):
            env.play(bad_w, rows=rows)
    with pytest.raises(ValueError):
        env.play(Wm)  # no rows: needs a row per env
    with pytest.raises(ValueError):
        env.greedy_actions(weights=Wm)
    with pytest.raises(ValueError):
        env.greedy_actions(weights=Wm, rows=rows, include_fitness=True)
    with pytest.raises(ValueError):
        env.greedy_actions(rows=rows)
    with pytest.raises(ValueError):
        env.play(Wm, rows=rows[:-1])


def longest_chunk(steps, chunk):
    return (steps + chunk - 1) // chunk * chunk

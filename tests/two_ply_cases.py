"""Shared cases for the two-piece lookahead in one kernel (VecTetris.lookahead on tetris_hip_policy_two_ply).  Each takes
the torch device: "cuda" (tests/test_two_ply_gpu.py, the HIP kernel) or "cpu" with the harness backend
(tests/test_two_ply_host.py, the same per-lane body compiled by g++).

Every comparison is bit for bit; there is no tolerance anywhere.  The yardsticks are never the new call:
 1. the table `values` against the oracle (placements -> child -> placements per piece -> float32 left-to-right fitness
    maximum) and against the existing VecTetris.two_ply_values;
 2. `q`, `n_bag`, `best_action`, `best_value` against NumPy float32 on the call's own table and the bag bits of meta;
 3. the outputs of an env against those of the same env in other batches (position in the workgroup, workgroup edges);
 4. the footprint helpers of tests/footprint_cases.py;
 6. play: every action against the NumPy pick on that round's two_ply_values, and the trace against a stored one."""
import ctypes
import os

import numpy as np
import torch

import directed_boards as db
import footprint_cases as fc
import gather_cases as gc

BCTS = np.array([-24.04, -19.77, -13.08, -12.63, -10.49, -9.22, 6.6, -1.61], np.float32)  # game.py:111-118
NINF = -float("inf")
MASK48 = (1 << 48) - 1
BLOCK = 512  # lanes of a workgroup of two_ply_kernel: EPB = BLOCK // a_max envs
DEATH_VALUES = [NINF, -1000.0]
OUTPUTS = ("values", "q", "n_bag", "best_action", "best_value")

# every (word, storage, chunk count) variant tet::kernel_variant picks and both widths of the 12-bit mask fields' word
TABLE_GEOMETRIES = [(6, 10, "default"), (10, 20, "default"), (10, 20, gc.STANDARD7), (10, 40, "default"), (12, 59, "default"),
                    (11, 27, "default"), (10, 26, "default")]


def _names(pieces):
    from tetris_amd.tetromino import resolve_pieces
    return list(resolve_pieces(pieces))


def _np(t):
    return t.cpu().numpy()


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def call(env, death_value=NINF, weights=BCTS, which=OUTPUTS):
    """tetris_hip_policy_two_ply of the library `env` is bound to, into fresh tensors: dict of NumPy arrays"""
    B, A, P, dev = env.batch_size, env.a_max, len(env.piece_names), env.device
    shapes = dict(values=((B, A, P), torch.float32), q=((B, A), torch.float32), n_bag=((B,), torch.uint8),
                  best_action=((B,), torch.int32), best_value=((B,), torch.float32))
    out = {k: torch.zeros(shapes[k][0], dtype=shapes[k][1], device=dev) for k in which}
    ptr = lambda k: ctypes.c_void_p(out[k].data_ptr()) if k in out else None
    w = (ctypes.c_float * 8)(*[float(x) for x in weights])
    rc = env._lib.policy_two_ply(ctypes.byref(env.desc), ctypes.c_void_p(env.cols.data_ptr()), ctypes.c_void_p(env.meta.data_ptr()),
                                 w, float(death_value), ptr("values"), ptr("q"), ptr("n_bag"), ptr("best_action"),
                                 ptr("best_value"), B, env._hip_stream())
    assert rc == 0, rc
    return {k: _np(v) for k, v in out.items()}


def _popcount(x):
    x = x.astype(np.uint64)
    n = np.zeros(x.shape, np.int64)
    for b in range(64):
        n += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return n


def meta_fields(meta, n_pieces):
    """(n_valid, bag as the call reads it, raw bag bits) of int64 meta words"""
    m = np.ascontiguousarray(meta).view(np.uint64)
    raw = (m >> np.uint64(52)).astype(np.int64)
    every = (1 << n_pieces) - 1
    bag = raw & every
    bag[bag == 0] = every
    return _popcount(m & np.uint64(MASK48)), bag, raw


def numpy_sums(values, meta, death_value):
    """q, n_bag, best_action, best_value in NumPy float32 from a table and the meta words: the pieces of the bag in
    ascending p, additions from the first term, -inf replaced by death_value, GreedyPick's first maximum"""
    B, A, P = values.shape
    nv, bag, _ = meta_fields(meta, P)
    q = np.zeros((B, A), np.float32)
    started = np.zeros(B, bool)
    with np.errstate(invalid="ignore"):
        for p in range(P):
            inbag = ((bag >> p) & 1) == 1
            v = values[:, :, p]
            t = np.where(np.isneginf(v), np.float32(death_value), v).astype(np.float32)
            s = q + t
            assert s.dtype == np.float32
            q = np.where(inbag[:, None], np.where(started[:, None], s, t), q)
            started |= inbag
        q[np.arange(A)[None, :] >= nv[:, None]] = np.nan
        best, row = np.zeros(B, np.float32), np.full(B, -1, np.int32)
        for k in range(A):
            v = q[:, k]
            take = (k < nv) & ((row < 0) | (v > best))
            best, row = np.where(take, v, best), np.where(take, np.int32(k), row)
    return dict(q=q, n_bag=_popcount(bag).astype(np.uint8), best_action=row, best_value=best.astype(np.float32))


def assert_sums(got, meta, death_value):
    want = numpy_sums(got["values"], meta, death_value)
    np.testing.assert_array_equal(_i32(got["q"]), _i32(want["q"]))
    np.testing.assert_array_equal(got["n_bag"], want["n_bag"])
    np.testing.assert_array_equal(got["best_action"], want["best_action"])
    np.testing.assert_array_equal(_i32(got["best_value"]), _i32(want["best_value"]))
    return want


# ---- 1. the table against the oracle and against two_ply_values ----------------------------------------------------
def _fitness(f, w):
    """float32, left to right (fitness_of's order)"""
    v = np.float32(f[0] * w[0])
    for q in range(1, 8):
        v = np.float32(v + np.float32(f[q] * w[q]))
    return v


_ORACLE_TABLES = {}


def oracle_table(orc, C, R, pieces, cells, piece, a_max):
    """the oracle's table of 24 boards, computed once per geometry; asserts the coverage the case asks of it"""
    key = (C, R, tuple(_names(pieces)))
    if key not in _ORACLE_TABLES:
        names = _names(pieces)
        desc = orc.make_desc(C, R, names)
        B, P = len(cells), len(names)
        want = np.full((B, a_max, P), np.nan, np.float32)
        for i in range(B):
            pl = orc.placements(desc, cells[i], names[piece[i]])
            for k, child in enumerate(pl["cells"][pl["terminal"] == 0]):
                for p, name in enumerate(names):
                    pl2 = orc.placements(desc, child, name)
                    vals = [_fitness(f, BCTS) for f in pl2["feats"][pl2["terminal"] == 0]]
                    want[i, k, p] = max(vals) if vals else -np.inf
        assert np.isnan(want).any() and np.isneginf(want).any() and np.isfinite(want).sum() > B
        _ORACLE_TABLES[key] = (cells.copy(), piece.copy(), want)
    kept_cells, kept_piece, want = _ORACLE_TABLES[key]
    assert np.array_equal(kept_cells, cells) and np.array_equal(kept_piece, piece)  # the same start state on every backend
    return want


def table_source(device, C, R, pieces):
    """expand_cases.two_ply_vs_oracle's construction: 16 played envs, 8 near-top / structured boards behind them"""
    boards = np.concatenate([db.near_top(8, R, C, seed=R + C), db.structured(R, C, seed=C)[1::9][:8]])
    n_dir = len(boards)
    env = gc.played(device, C, R, pieces, 24, 3, 12)
    cells = env.boards()
    cells[24 - n_dir:] = torch.as_tensor(boards, device=device)
    env.set_boards(cells)
    return env


def table_vs_oracle(device, orc, C, R, pieces):
    env = table_source(device, C, R, pieces)
    snap = gc.snapshot(env)
    A, P = env.a_max, len(env.piece_names)
    want = oracle_table(orc, C, R, pieces, _np(snap["boards"]), _np(env.piece).astype(np.int64), A)
    got = call(env)
    values = got["values"]
    assert values.shape == (24, A, P) and values.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(values), np.isnan(want))
    np.testing.assert_array_equal(np.isneginf(values), np.isneginf(want))
    fin = np.isfinite(want)
    np.testing.assert_array_equal(_i32(values[fin]), _i32(want[fin]))
    np.testing.assert_array_equal(_i32(values), _i32(_np(env.two_ply_values())))
    assert_sums(got, _np(env.meta), NINF)
    action, mean, q_mean, table = env.lookahead(return_q=True, return_values=True)
    np.testing.assert_array_equal(_i32(_np(table)), _i32(values))
    np.testing.assert_array_equal(_np(action), got["best_action"])
    n = got["n_bag"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(_i32(_np(mean)), _i32(got["best_value"] / n))
        np.testing.assert_array_equal(_i32(_np(q_mean)), _i32(got["q"] / n[:, None]))
    assert torch.equal(env.cols, snap["cols"]) and torch.equal(env.meta, snap["meta"])


# ---- 2. sums and pick against NumPy from the table ---------------------------------------------------------------
SYMMETRIC_BAG = 0b1001001  # Straight, Square, T of the standard seven: the pieces that are their own mirror image
BAGS = [0, 1 << 0, 1 << 6, 0b11, 0b1010100, (1 << 7) - 1, 1 << 3, 0b1100000]


def sums_source(device):
    """10x20, the standard seven, 48 envs: played boards, near-top boards (children that are over), empty boards with the
    Square (mirror placements tie), a full board with one well (the Square has no placement: n_valid == 0); bags of
    every size set in meta"""
    from tetris_amd import VecTetris
    C, R, B = 10, 20, 48
    env = gc.played(device, C, R, gc.STANDARD7, B, 5, 14)
    env.auto_reset = False
    cells, piece = _np(env.boards()).copy(), _np(env.piece).astype(np.int64)
    near = db.near_top(20, R, C, seed=77)
    cells[8:28] = near
    piece[8:28] = np.arange(20) % 7
    cells[28:36] = 0
    piece[28:36] = 3  # Square
    well = np.zeros((R + 4, C), np.int8)
    well[:R, :] = 1
    well[:R, 4] = 0
    cells[36:38] = well
    piece[36:38] = 3
    db.check_boards(cells, R)
    bag = np.array([BAGS[i % len(BAGS)] for i in range(B)], np.uint64)
    bag[28:32] = SYMMETRIC_BAG
    bag[32:36] = 0
    meta = _np(env.meta).view(np.uint64)
    meta = (meta & np.uint64((1 << 52) - 1)) | (bag << np.uint64(52))
    env.meta.copy_(torch.as_tensor(meta.view(np.int64), device=device))
    env.set_boards(cells, piece)  # (refresh: the masks of these boards and pieces; the bags stay)
    assert np.array_equal(_np(env.meta).view(np.uint64) >> np.uint64(52), bag)
    return env


def sums_and_pick(device):
    env = sums_source(device)
    snap = gc.snapshot(env)
    meta = _np(env.meta)
    P = len(env.piece_names)
    nv, bag, raw = meta_fields(meta, P)
    sizes = _popcount(raw)
    assert (sizes == 0).any() and (sizes == 1).any() and (sizes >= 2).any()
    np.testing.assert_array_equal(nv, _np(env.n_valid).astype(np.int64))
    over = np.nonzero(nv == 0)[0]
    assert len(over)
    got = {}
    for death in DEATH_VALUES:
        g = got[death] = call(env, death)
        assert_sums(g, meta, death)
        np.testing.assert_array_equal(_i32(g["values"]), _i32(got[DEATH_VALUES[0]]["values"]))  # the table does not depend on it
        assert (g["best_action"][over] == -1).all() and (_i32(g["best_value"][over]) == 0).all()
        assert np.isnan(g["values"][over]).all() and np.isnan(g["q"][over]).all()
        alive = nv > 0
        assert ((g["best_action"][alive] >= 0) & (g["best_action"][alive] < nv[alive])).all()
        # lookahead() is the same call with the mean taken in torch
        action, mean = env.lookahead(death_value=death)
        np.testing.assert_array_equal(_np(action), g["best_action"])
        np.testing.assert_array_equal(_i32(_np(mean)), _i32(g["best_value"] / g["n_bag"].astype(np.float32)))
    a, b = got[DEATH_VALUES[0]], got[DEATH_VALUES[1]]
    # a child that is over with a piece of the bag: q differs between the two death values there
    dead = np.isneginf(a["values"]) & (((bag[:, None] >> np.arange(P)[None, :]) & 1) == 1)[:, None, :]
    assert dead.any()
    hit = dead.any(axis=2)
    assert (np.isneginf(a["q"][hit])).all() and np.isfinite(b["q"][hit]).all()
    assert (_i32(a["q"]) != _i32(b["q"])).any()
    # an exact tie at the maximum goes to the lower index
    ties = 0
    for i in range(28, 36):
        row = a["q"][i, :nv[i]]
        at = np.nonzero(row == row.max())[0]
        ties += len(at) > 1
        assert a["best_action"][i] == at[0]
    assert ties > 0
    assert torch.equal(env.cols, snap["cols"]) and torch.equal(env.meta, snap["meta"])
    assert env.stats()["invalid"] == 0


# ---- 3. position independence and workgroup edges -------------------------------------------------------------------
def _same(a, b, rows):
    for k in OUTPUTS:
        np.testing.assert_array_equal(_i32(a[k]) if a[k].dtype == np.float32 else a[k],
                                      (_i32(b[k]) if b[k].dtype == np.float32 else b[k])[rows], err_msg=k)


def position_independence(device, C, R, pieces):
    src = gc.played(device, C, R, pieces, 200, 3, 20)
    epb = BLOCK // src.a_max
    assert 1 < epb < 64
    whole = call(src)
    assert_sums(whole, _np(src.meta), NINF)
    for B in (1, epb - 1, epb, epb + 1, 2 * epb + 3):
        _same(call(src.fork(torch.arange(B))), whole, slice(0, B))
    for cut in (64, epb):
        for lo in range(0, 200, cut):
            hi = min(lo + cut, 200)
            _same(call(src.fork(torch.arange(lo, hi))), whole, slice(lo, hi))


def many_workgroups(device, B=4099):
    env = gc.played(device, 10, 20, "default", B, 9, 25)
    assert B // (BLOCK // env.a_max) > 250
    got = call(env, -1000.0)
    nv = meta_fields(_np(env.meta), len(env.piece_names))[0]
    absent = np.arange(env.a_max)[None, :] >= nv[:, None]
    np.testing.assert_array_equal(np.isnan(got["values"]).all(axis=2), absent)
    np.testing.assert_array_equal(np.isnan(got["values"]).any(axis=2), absent)
    assert_sums(got, _np(env.meta), -1000.0)
    best, _ = env.greedy_actions()  # one ply agrees with itself on the same boards: the batch was read where it lies
    assert ((_np(best) >= 0) == (got["best_action"] >= 0)).all()


# ---- 4. footprint -------------------------------------------------------------------------------------------------
FOOTPRINT_FORMS = ["all"] + list(OUTPUTS) + ["none"]


def footprint(lib, device, C, R, B, form):
    geo, st = fc.state(lib, device, C, R, B)
    A, P = geo.a_max, geo.n_pieces
    sizes = dict(values=4 * B * A * P, q=4 * B * A, n_bag=B, best_action=4 * B, best_value=4 * B)
    asked = OUTPUTS if form == "all" else (() if form == "none" else (form,))

    def run(arena):
        ptr = {k: arena.new(k, sizes[k]) if k in asked else None for k in OUTPUTS}
        arena.new("status", init=st["status"], keep=True)  # (no argument of the call: it stays as it is)
        arena.launch(lib.policy_two_ply, geo.d, arena.new("cols", init=st["cols"], keep=True),
                     arena.new("meta", init=st["meta"], keep=True), fc.WEIGHTS, -1000.0, ptr["values"], ptr["q"], ptr["n_bag"],
                     ptr["best_action"], ptr["best_value"], B, None)

    g, _ = fc.footprint(device, run)
    if form == "all":
        got = {k: _np(g.bufs[k].body.view(torch.uint8)).view(np.uint8 if k == "n_bag" else (np.int32 if k == "best_action" else np.float32))
               for k in OUTPUTS}
        got["values"], got["q"] = got["values"].reshape(B, A, P), got["q"].reshape(B, A)
        assert_sums(got, _np(st["meta"]), -1000.0)


# ---- 6. it plays ------------------------------------------------------------------------------------------------------
TRACE_FILE = "g12_two_ply_trace.npy"  # int8 [40, 64]: the actions of the run below on the CPU harness


def plays(device, rounds=40):
    """64 envs of 10x20 with the standard seven under auto-reset: lookahead() then step(); every action is the NumPy
    pick on that round's two_ply_values.  Returns the action trace int8 [rounds, 64]."""
    from tetris_amd import VecTetris
    env = VecTetris(10, 20, 64, device=device, pieces=gc.STANDARD7, auto_reset=True, seed=12)
    trace = np.zeros((rounds, 64), np.int8)
    for t in range(rounds):
        table = _np(env.two_ply_values())
        want = numpy_sums(table, _np(env.meta), NINF)
        action, mean = env.lookahead()
        np.testing.assert_array_equal(_np(action), want["best_action"], err_msg="round %d" % t)
        with np.errstate(invalid="ignore"):
            np.testing.assert_array_equal(_i32(_np(mean)), _i32(want["best_value"] / want["n_bag"].astype(np.float32)))
        trace[t] = _np(action)
        env.step(action)
    env.check()
    assert env.stats()["steps"] == rounds * 64
    return trace


def stored_trace(golden_dir):
    return np.load(os.path.join(golden_dir, TRACE_FILE))


def replay_mode(device):
    """nothing is drawn: an env on a piece stream looks ahead like one on the bag with the same boards and meta"""
    from tetris_amd import VecTetris
    stream = np.random.RandomState(4).randint(0, 2, size=(16, 70)).astype(np.uint8)
    env = VecTetris(10, 20, 70, device=device, piece_stream=stream)
    for _ in range(6):
        env.step()
    action, mean = env.lookahead()
    twin = VecTetris(10, 20, 70, device=device)
    twin.cols.copy_(env.cols)
    twin.meta.copy_(env.meta)
    twin.refresh()
    want = numpy_sums(_np(twin.two_ply_values()), _np(twin.meta), NINF)
    np.testing.assert_array_equal(_np(action), want["best_action"])
    env.check()

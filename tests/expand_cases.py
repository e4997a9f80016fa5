"""Shared cases for expanding envs into their afterstates as envs (VecTetris.expand_from / expand / two_ply_values on
tetris_hip_expand_envs).  Each takes the torch device: "cuda" (tests/test_expand_gpu.py, the HIP kernel) or "cpu" with
the harness backend (tests/test_expand_host.py, the same per-env body compiled by g++).

The yardstick is never the new call: it is the oracle (oracle.placements: the child cells, n_cleared, terminal and
features of every placement in reference order, the k-th non-terminal one being action k), the reference's own
recorded children (tests/golden/g1_placements_*.npz) and the existing step(), boards() and get_after_states()."""
import os

import numpy as np
import pytest
import torch

import directed_boards as db
import footprint_cases as fc
import gather_cases as gc

GEOMETRIES = gc.GEOMETRIES + [pytest.param(6, 10, "default", id="6x10-u32-one-chunk")]
N_PLAYED = 200
BCTS = np.array([-24.04, -19.77, -13.08, -12.63, -10.49, -9.22, 6.6, -1.61], np.float32)  # game.py:111-118


def _names(pieces):
    from tetris_amd.tetromino import resolve_pieces
    return list(resolve_pieces(pieces))


def _np(t):
    return t.cpu().numpy()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def directed_source(device, C, R, pieces, seed=3, n_near=24, **kw):
    """200 envs after 30 random auto-reset steps, then the near-top and the structured boards of directed_boards.py
    (rows missing one column complete under the right piece; a well between full columns leaves a wide piece no
    placement: a parent that is over) set over the envs behind them with the pieces of the set in turn; the bags and
    the first 200 pieces stay as played."""
    boards = np.concatenate([db.near_top(n_near, R, C, seed=R * 100 + C), db.structured(R, C, seed=C)])
    db.check_boards(boards, R)
    env = gc.played(device, C, R, pieces, N_PLAYED + len(boards), seed, 30, **kw)
    cells, piece = env.boards(), env.piece.clone()
    cells[N_PLAYED:] = torch.as_tensor(boards, device=device)
    piece[N_PLAYED:] = torch.arange(len(boards), device=device).to(torch.uint8) % len(env.piece_names)
    env.set_boards(cells, piece)
    env.auto_reset = False
    return env


def oracle_children(orc, desc, names, cells, piece, a_max):
    """the non-terminal placements of every env, in reference order: child cells [B, A, rows, C], n_cleared [B, A],
    features [B, A, 8], count [B]"""
    B = len(cells)
    out = dict(cells=np.zeros((B, a_max) + cells.shape[1:], np.int8), lines=np.zeros((B, a_max), np.int64),
               feats=np.zeros((B, a_max, 8), np.float32), nv=np.zeros(B, np.int64))
    for i in range(B):
        pl = orc.placements(desc, cells[i], names[piece[i]])
        ok = pl["terminal"] == 0
        n = int(ok.sum())
        out["nv"][i] = n
        out["cells"][i, :n], out["lines"][i, :n], out["feats"][i, :n] = pl["cells"][ok], pl["n_cleared"][ok], pl["feats"][ok]
    return out


def oracle_n_valid(orc, desc, name, cells):
    """the oracle's count of non-terminal placements of one piece on each board"""
    return np.array([int((orc.placements(desc, c, name)["terminal"] == 0).sum()) for c in cells], np.int64)


# ---- 1. children against the oracle ----------------------------------------------------------------------------
def children_vs_oracle(device, orc, C, R, pieces):
    names = _names(pieces)
    desc = orc.make_desc(C, R, names)
    src = directed_source(device, C, R, pieces)
    B, A = src.batch_size, src.a_max
    src_snap = gc.snapshot(src)
    piece = _np(src.piece).astype(np.int64)
    want = oracle_children(orc, desc, names, _np(src_snap["boards"]), piece, A)
    feats, nv = (t.clone() for t in src.get_after_states())
    np.testing.assert_array_equal(_np(nv), want["nv"])
    want_present = np.arange(A)[None, :] < want["nv"][:, None]
    assert (want["nv"] < A).any() and (want["nv"] == 0).any()  # a parent with fewer placements, a parent that is over
    at = np.nonzero(want_present.reshape(-1))[0]
    parent_bag = (_np(src.meta).astype(np.uint64) >> np.uint64(52))[at // A]
    seen = dict(lines=False, done=False)
    for p, name in enumerate(names):
        child, present = src.expand(p)
        assert child.batch_size == B * A and child.step_idx == src.step_idx and child.auto_reset is False
        np.testing.assert_array_equal(_np(present), want_present)
        np.testing.assert_array_equal(_np(child.boards())[at], want["cells"].reshape((B * A,) + want["cells"].shape[2:])[at])
        lines, n_valid, done = _np(child.lines)[at].astype(np.int64), _np(child.n_valid)[at].astype(np.int64), _np(child.done)[at]
        np.testing.assert_array_equal(lines, want["lines"].reshape(-1)[at])
        assert torch.equal(_bits(child.obs)[at], _bits(feats.reshape(B * A, 8))[at])
        np.testing.assert_array_equal(_np(child.obs)[at], want["feats"].reshape(-1, 8)[at])
        np.testing.assert_array_equal(n_valid, oracle_n_valid(orc, desc, name, _np(child.boards())[at]))
        np.testing.assert_array_equal(done, n_valid == 0)
        np.testing.assert_array_equal(_np(child.reward)[at], lines - 1 - 100 * done)
        assert (_np(child.piece)[at] == p).all()
        meta = _np(child.meta).astype(np.uint64)[at]
        np.testing.assert_array_equal(meta >> np.uint64(52), parent_bag)
        np.testing.assert_array_equal((meta >> np.uint64(48)) & np.uint64(15), np.full(len(at), p, np.uint64))
        assert child.stats()["invalid"] == 0  # absent children are not errors
        child.check()
        absent = torch.nonzero(~present.reshape(-1)).flatten()
        assert not child.boards()[absent].any() and bool((child.n_valid[absent] > 0).all())  # freshly reset envs
        seen["lines"] |= bool((lines >= 1).any())
        seen["done"] |= bool(done.any())
    assert seen["lines"] and seen["done"], seen
    assert torch.equal(src.cols, src_snap["cols"]) and torch.equal(src.meta, src_snap["meta"])


# ---- 2. the reference's own children ---------------------------------------------------------------------------
def children_vs_golden(device, golden_dir, fname):
    from oracle import oracle as orc
    from tetris_amd import VecTetris
    from tetris_amd.tetromino import CATALOGUE
    g = np.load(os.path.join(golden_dir, fname))
    R, C = int(g["R"]), int(g["C"])
    nb = len(g["boards"])
    cells = orc.cols_to_cells(g["boards"], R + 4)
    env = VecTetris(C, R, nb, device=device, pieces=list(CATALOGUE))
    A = env.a_max
    term = g["terminal"].astype(bool)
    n_children = 0
    for pi in range(len(CATALOGUE)):
        env.set_boards(cells, piece=np.full(nb, pi))
        child, present = env.expand(0)
        cols, lines, present = _np(child.columns()).astype(np.uint64).T.reshape(nb, A, C), _np(child.lines).reshape(nb, A), _np(present)
        for b in range(nb):
            sel = (g["board_ix"] == b) & (g["piece"] == pi) & ~term
            n = int(sel.sum())
            assert present[b].sum() == n and present[b, :n].all()
            np.testing.assert_array_equal(cols[b, :n], g["cols"][sel])
            np.testing.assert_array_equal(lines[b, :n], g["n_cleared"][sel])
            n_children += n
        child.check()
    assert n_children == int((~term).sum()) > 0


# ---- 3. a drawn piece is a step ------------------------------------------------------------------------------------
OUTPUTS = ("obs", "reward", "_done", "lines", "n_valid", "piece")


def drawn_equals_step(device, C, R, pieces, B_src=N_PLAYED, B_dst=N_PLAYED, env_offset=1000):
    """dst env j against env parent[j] of src.fork(arange).step(action) without auto-reset, bit for bit: identity
    parents in front (B_dst == B_src: the whole raw cols tensor), random ones, with repeats, behind them"""
    src = gc.played(device, C, R, pieces, B_src, 3, 30, env_offset=env_offset)
    snap = gc.snapshot(src)
    a = src.random_actions().clone()
    twin = src.fork(torch.arange(B_src))
    twin.auto_reset = False
    twin.step(a)
    twin.check()
    dst = gc.played(device, C, R, pieces, B_dst, 11, 17)
    rng = np.random.RandomState(B_dst)
    parent = rng.randint(0, B_src, size=B_dst)
    n_id = min(B_src, B_dst) if B_dst > B_src else B_dst // 2
    parent[:n_id] = np.arange(n_id)
    if B_dst == B_src:
        parent[:] = np.arange(B_src)
    parent = torch.as_tensor(parent, device=device)
    step_idx = src.step_idx
    assert dst.expand_from(src, parent, a[parent]) is dst
    assert src.step_idx == step_idx and torch.equal(src.cols, snap["cols"]) and torch.equal(src.meta, snap["meta"])
    at = parent.long()
    everyone = torch.arange(B_dst, device=device)
    assert torch.equal(gc.lanes(dst, everyone), gc.lanes(twin, at))  # every stored word
    assert torch.equal(dst.meta, twin.meta[at])
    for k in OUTPUTS:
        assert torch.equal(_bits(getattr(dst, k)), _bits(getattr(twin, k)[at])), k
    if B_dst == B_src:
        live = torch.zeros(dst.n_tiles * 64, dtype=torch.bool, device=device)
        live[:B_dst] = True
        live = live.view(dst.n_tiles, 1, 64).expand_as(dst.cols)
        assert torch.equal(dst.cols[live], twin.cols[live])
    assert dst.stats()["invalid"] == 0
    return src, twin, dst, parent


def repeated_parents_share_the_piece(device, C, R, pieces):
    """the dense expansion with a drawn piece: every child of a parent faces the piece and holds the bag the parent's
    own step draws, and plays on from the parent's next step index"""
    src = gc.played(device, C, R, pieces, N_PLAYED, 3, 30, env_offset=77)
    twin = src.fork(torch.arange(N_PLAYED))
    twin.auto_reset = False
    twin.step(torch.zeros(N_PLAYED, dtype=torch.int32, device=device))  # (placement 0 exists wherever one does)
    child, present = src.expand()
    assert child.step_idx == src.step_idx + 1 == twin.step_idx
    A = src.a_max
    own = torch.arange(N_PLAYED, device=device)[:, None].expand(N_PLAYED, A)[present]
    rows = torch.nonzero(present.reshape(-1)).flatten()
    assert torch.equal(child.piece[rows], twin.piece[own])
    assert torch.equal(child.meta[rows] >> 52, twin.meta[own] >> 52)
    first = torch.nonzero(present[:, 0]).flatten()
    assert torch.equal(child.boards()[first * A], twin.boards()[first]) and torch.equal(child.meta[first * A], twin.meta[first])
    assert len(set(child.piece[rows].tolist())) > 1
    child.check()


def shard_draws_the_batchs_pieces(device, C, R, pieces):
    """a shard of whole tiles with its env_offset expands to what the whole batch's expansion holds for those envs"""
    whole = gc.played(device, C, R, pieces, N_PLAYED, 3, 30, env_offset=1000)
    shard = whole.fork(torch.arange(128, N_PLAYED), env_offset=1128)
    wc, wp = whole.expand()
    sc, sp = shard.expand()
    A = whole.a_max
    assert torch.equal(sp, wp[128:])
    rows = torch.nonzero(sp.reshape(-1)).flatten()
    assert torch.equal(sc.meta[rows], wc.meta[128 * A + rows]) and torch.equal(sc.boards()[rows], wc.boards()[128 * A + rows])
    assert torch.equal(sc.piece[rows], wc.piece[128 * A + rows])
    other = whole.fork(torch.arange(128, N_PLAYED), env_offset=0).expand()[0]  # (another offset draws other pieces)
    assert not torch.equal(other.piece[rows], sc.piece[rows])


# ---- 4. untouched and invalid entries --------------------------------------------------------------------------------
def untouched_and_invalid(device, C, R, pieces, B_dst):
    B_src = N_PLAYED
    src = directed_source(device, C, R, pieces)  # (holds parents that are over)
    B_src = src.batch_size
    n_pieces = len(_names(pieces))
    dst = gc.played(device, C, R, pieces, B_dst, 11, 17)
    for k in ("_obs_buf", "_reward_buf", "_done_buf", "_lines_buf"):  # outputs that are not zero where untouched
        getattr(dst, k).copy_(torch.arange(getattr(dst, k).numel(), device=device).view_as(getattr(dst, k)) % 101 + 1)
    nv = _np(src.n_valid).astype(np.int64)
    over, alive = np.nonzero(nv == 0)[0], np.nonzero(nv > 0)[0]
    assert len(over) and len(alive)
    rng = np.random.RandomState(B_dst + 1)
    parent = alive[rng.randint(0, len(alive), size=B_dst)].astype(np.int64)
    action = (rng.rand(B_dst) * nv[parent]).astype(np.int64)
    nxt = rng.randint(0, n_pieces, size=B_dst)
    kept = rng.rand(B_dst) < 0.25
    parent[kept] = -1
    # one bad entry of each kind, spread over the waves and on the last lane of the partial tile
    slots = [5, 20, 63, 64, 70, 100, B_dst - 3, B_dst - 2, B_dst - 1]
    assert len(set(slots)) == len(slots)
    kept[slots] = False
    good_parent = int(alive[0])
    for j in slots:
        parent[j], action[j], nxt[j] = good_parent, 0, 0
    parent[slots[0]] = -2
    parent[slots[1]] = B_src
    parent[slots[2]] = 2**31 - 1
    action[slots[3]] = -1
    action[slots[4]] = nv[good_parent]
    parent[slots[5]], action[slots[5]] = int(over[0]), 255
    nxt[slots[6]] = n_pieces
    nxt[slots[7]] = 255
    parent[slots[8]], action[slots[8]] = int(over[-1]), 0
    bad_rows = torch.as_tensor(sorted(slots), device=device)
    untouched = torch.as_tensor(np.nonzero(kept)[0].tolist() + sorted(slots), device=device)
    good = torch.as_tensor([j for j in range(B_dst) if not kept[j] and j not in slots], device=device)
    src_snap, before = gc.snapshot(src), gc.snapshot(dst)
    outs_before = {k: getattr(dst, k).clone() for k in OUTPUTS}
    dst.expand_from(src, torch.as_tensor(parent, device=device), torch.as_tensor(action, device=device),
                    torch.as_tensor(nxt, device=device))
    gc.assert_untouched(dst, before, untouched)
    gc.assert_raw_cols_kept(dst, before, untouched)
    for k in OUTPUTS:
        assert torch.equal(_bits(getattr(dst, k))[untouched], _bits(outs_before[k])[untouched]), k
    assert bool((dst.piece[good] == torch.as_tensor(nxt, device=device)[good].to(torch.uint8)).all())
    assert not torch.equal(dst.meta[good], before["meta"][good])
    assert dst.stats()["invalid"] == len(slots)
    per_wave = _np(dst.status.view(-1, 4)[:, 0])
    want = np.zeros_like(per_wave)
    for j in slots:
        want[j >> 6] += 1
    np.testing.assert_array_equal(per_wave, want)
    assert torch.equal(src.cols, src_snap["cols"]) and torch.equal(src.meta, src_snap["meta"])
    assert torch.equal(src.n_valid, src_snap["n_valid"]) and torch.equal(src.piece, src_snap["piece"])
    with pytest.raises(IndexError):
        dst.check()
    return bad_rows


# ---- 5. footprint ---------------------------------------------------------------------------------------------------
def footprint(lib, device, C, R, B, with_optional, B_src=200):
    """every buffer of tetris_hip_expand_envs between guard bands: a quarter of dst kept, one bad entry per wave"""
    geo, src = fc.state(lib, device, C, R, B_src, seed=11, steps=9)
    _, dst = fc.state(lib, device, C, R, B)
    assert dst["cols"].numel() == geo.cols_bytes(B) == int(lib.board_words(geo.d, B)) * geo.wb
    gen = torch.Generator().manual_seed(B)
    alive = torch.nonzero(src["n_valid"].cpu() > 0).flatten()
    parent = alive[torch.randint(0, len(alive), (B,), generator=gen)].to(torch.int32)
    action = (torch.rand(B, generator=gen) * src["n_valid"].cpu()[parent.long()]).to(torch.int32)
    parent[torch.rand(B, generator=gen) < 0.25] = -1
    parent, action = parent.to(device), action.to(device)
    nxt = torch.randint(0, geo.n_pieces, (B,), generator=gen).to(torch.uint8).to(device)
    bad = fc._one_per_wave(B, device)
    kind = (torch.arange(B, device=device) // 64)[bad] % 3
    parent[bad] = torch.where(kind == 0, B_src, torch.where(kind == 1, -2, 0)).to(torch.int32)
    action[bad] = torch.where(kind == 2, 255, 0).to(torch.int32)
    kept = (parent == -1) | bad
    k1, k4 = fc._elems(kept, 1), fc._elems(kept, 4)

    def call(A):
        opt = with_optional
        A.launch(lib.expand_envs, geo.d, A.new("src_cols", init=src["cols"], keep=True), A.new("src_meta", init=src["meta"], keep=True),
                 B_src, A.new("dst_cols", init=dst["cols"], keep=geo.kept_lanes(B, kept, device)),
                 A.new("dst_meta", init=dst["meta"], keep=fc._elems(kept, 8)), A.new("parent", init=parent, keep=True),
                 A.new("action", init=action, keep=True), A.new("next_piece", init=nxt, keep=True) if opt else None,
                 A.new("obs", nbytes=32 * B, keep=fc._elems(kept, 32)) if opt else None,
                 A.new("reward", nbytes=4 * B, keep=k4), A.new("done", nbytes=B, keep=k1), A.new("lines", nbytes=B, keep=k1),
                 A.new("n_valid", init=dst["n_valid"] + 100, keep=k1), A.new("piece", init=dst["piece"] + 100, keep=k1),
                 A.new("status", init=dst["status"]) if opt else None, 3, 9, 0, B, None)

    g, _ = fc.footprint(device, call)
    if with_optional:
        status = g.bufs["status"].body.view(torch.int32).view(-1, 4) - dst["status"].view(-1, 4)
        assert int(status[:, 0].sum()) == int(bad.sum()) and not status[:, 1:].any()
    touched = ~kept
    assert bool(touched.any()) or B == 1


# ---- 6. Python-side refusals ---------------------------------------------------------------------------------------
def host_refusals(device):
    from tetris_amd import VecTetris
    env = VecTetris(10, 20, 70, device=device, seed=1)
    ok = torch.zeros(70, dtype=torch.int32)
    for other in (VecTetris(10, 24, 70, device=device), VecTetris(9, 20, 70, device=device),
                  VecTetris(10, 20, 70, device=device, pieces=gc.STANDARD7)):
        with pytest.raises(ValueError):
            env.expand_from(other, ok, ok)
    with pytest.raises(ValueError):
        env.expand_from(env, ok, ok)
    src = VecTetris(10, 20, 50, device=device, seed=2)
    for bad in (torch.zeros(50, dtype=torch.int32), torch.zeros((70, 1), dtype=torch.int32), torch.zeros(70)):
        with pytest.raises(ValueError):
            env.expand_from(src, bad, ok)
        with pytest.raises(ValueError):
            env.expand_from(src, ok, bad)
        with pytest.raises(ValueError):
            env.expand_from(src, ok, ok, bad)
    replay = VecTetris(10, 20, 70, device=device, piece_stream=np.zeros((8, 70), dtype=np.uint8))
    seeded = VecTetris(10, 20, 70, device=device, numpy_seeds=np.arange(70), stream_len=8)
    for bad in (replay, seeded):
        with pytest.raises(ValueError):
            env.expand_from(bad, ok, ok)
        with pytest.raises(ValueError):
            bad.expand_from(env, ok, ok)
        with pytest.raises(ValueError):
            bad.expand()
        with pytest.raises(ValueError):
            bad.two_ply_values()
    for p in (-1, 2, 255):
        with pytest.raises(ValueError):
            env.expand(p)
    if torch.device(device).type == "cuda" and torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            env.expand_from(VecTetris(10, 20, 70, device="cuda:1"), ok, ok)
    before = gc.snapshot(env)
    env.expand_from(src, ok.tolist(), ok.tolist(), 1)  # anything as_tensor takes, one piece for all
    assert not torch.equal(env.meta, before["meta"]) and bool((env.piece == 1).all())
    env.check()


# ---- 7. composition ---------------------------------------------------------------------------------------------------
def child_is_an_env(device, C, R, pieces):
    src = gc.played(device, C, R, pieces, 64, 3, 30)
    child, present = src.expand()
    rows = torch.nonzero(present.reshape(-1)).flatten()
    feats, nv = child.get_after_states()
    assert torch.equal(nv[rows], child.n_valid[rows])
    best, _ = child.greedy_actions()
    alive = rows[child.n_valid[rows] > 0]
    assert bool(((best[alive] >= 0) & (best[alive] < child.n_valid[alive].to(torch.int32))).all())
    a = torch.where(child.n_valid > 0, best.clamp(min=0), torch.zeros_like(best))
    over = child.n_valid == 0
    child.step(a)
    assert child.stats()["invalid"] == int(over.sum())  # only the children that were over already refuse an action
    child.status.zero_()
    w = torch.as_tensor(BCTS, device=device).reshape(1, 8)
    out = child.play(w, rows=torch.zeros(child.batch_size, dtype=torch.int32, device=device), max_steps=8, chunk=4)
    assert int(out["pieces"].to(torch.int64).sum()) > 0
    child.check()


def _fitness(f, w):
    """float32, left to right (fitness_of's order)"""
    v = np.float32(0)
    for q in range(8):
        v = np.float32(v + np.float32(f[q] * w[q]))
    return v


def two_ply_vs_oracle(device, orc, C, R, pieces="default"):
    from tetris_amd import VecTetris
    names = _names(pieces)
    desc = orc.make_desc(C, R, names)
    boards = np.concatenate([db.near_top(8, R, C, seed=R + C), db.structured(R, C, seed=C)[1::9][:8]])
    n_dir = len(boards)
    env = gc.played(device, C, R, pieces, 24, 3, 12)
    cells = env.boards()
    cells[24 - n_dir:] = torch.as_tensor(boards, device=device)
    env.set_boards(cells)
    snap = gc.snapshot(env)
    got = _np(env.two_ply_values())
    B, A, P = 24, env.a_max, len(names)
    assert got.shape == (B, A, P) and got.dtype == np.float32
    cells, piece = _np(snap["boards"]), _np(env.piece).astype(np.int64)
    want = np.full((B, A, P), np.nan, np.float32)
    for i in range(B):
        pl = orc.placements(desc, cells[i], names[piece[i]])
        for k, child in enumerate(pl["cells"][pl["terminal"] == 0]):
            for p, name in enumerate(names):
                pl2 = orc.placements(desc, child, name)
                vals = [_fitness(f, BCTS) for f in pl2["feats"][pl2["terminal"] == 0]]
                want[i, k, p] = max(vals) if vals else -np.inf
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    assert np.isnan(want).any() and np.isneginf(want).any() and np.isfinite(want).sum() > B
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[fin].view(np.int32), want[fin].view(np.int32))
    assert torch.equal(env.cols, snap["cols"]) and torch.equal(env.meta, snap["meta"])
    again = _np(env.two_ply_values(list(BCTS)))  # the child batch is reused
    np.testing.assert_array_equal(again.view(np.int32), got.view(np.int32))

"""Shared cases for copying envs between batches by index (VecTetris.copy_envs_from / fork / gather_ on
tetris_hip_gather_envs).  Each takes the torch device: "cuda" (tests/test_gather_gpu.py, the HIP kernel) or
"cpu" with the harness backend (tests/test_gather_host.py, the same per-env body compiled by g++).

The yardstick is always the existing API on the SOURCE -- boards(), meta, n_valid, piece, get_after_states(),
greedy_actions(), step() -- never the new call."""
import numpy as np
import pytest
import torch

STANDARD7 = ["Straight", "RCorner", "LCorner", "Square", "SnakeR", "SnakeL", "T"]

# one geometry per storage class (tetris_hip_n_planes) and the widest packed board
GEOMETRIES = [
    pytest.param(10, 20, "default", id="10x20-u32-packed-8-planes"),
    pytest.param(6, 26, "default", id="6x26-u32-plane-per-column"),
    pytest.param(10, 40, STANDARD7, id="10x40-u64-packed"),
    pytest.param(5, 50, "default", id="5x50-u64-plane-per-column"),
    pytest.param(12, 20, "default", id="12x20-9-planes"),
]
B_SRC = 200            # 3 tiles + 8 lanes
B_DSTS = [130, 321]    # 2 tiles + 2 lanes, 5 tiles + 1 lane: both last tiles are partial


def played(device, C, R, pieces, B, seed, steps, **kw):
    """B envs after `steps` random steps with auto-reset: boards, pieces and bags differ between envs."""
    from tetris_amd import VecTetris
    env = VecTetris(C, R, B, device=device, pieces=pieces, auto_reset=True, seed=seed, **kw)
    for _ in range(steps):
        env.step()
    env.check()
    return env


def pair(device, C, R, pieces, B_src, B_dst):
    """(src, dst): dst is played with another seed, so that "untouched" is not "zero"."""
    return played(device, C, R, pieces, B_src, 3, 30), played(device, C, R, pieces, B_dst, 11, 17)


def snapshot(env):
    return dict(boards=env.boards().clone(), meta=env.meta.clone(), n_valid=env.n_valid.clone(), piece=env.piece.clone(),
                cols=env.cols.clone())


def lanes(env, envs):
    """rows [len(envs), n_planes] of the raw cols tensor: every stored word of those envs"""
    return env.cols[envs // 64, :, envs % 64]


def assert_copied(dst, src_snap, index, rows):
    """dst envs `rows` equal the source envs index[rows], by the source's own read-outs"""
    at = index[rows].long()
    assert torch.equal(dst.boards()[rows], src_snap["boards"][at])
    assert torch.equal(dst.meta[rows], src_snap["meta"][at])  # all 64 bits: mask, piece, bag
    assert torch.equal(dst.n_valid[rows], src_snap["n_valid"][at])
    assert torch.equal(dst.piece[rows], src_snap["piece"][at])


def assert_untouched(dst, before, rows):
    assert torch.equal(dst.boards()[rows], before["boards"][rows])
    assert torch.equal(dst.meta[rows], before["meta"][rows])
    assert torch.equal(dst.n_valid[rows], before["n_valid"][rows])
    assert torch.equal(dst.piece[rows], before["piece"][rows])


def assert_raw_cols_kept(dst, before, untouched_rows):
    """the raw storage: every lane of an untouched env and every padding lane of the last tile is as it was"""
    keep = torch.zeros(dst.n_tiles * 64, dtype=torch.bool, device=dst.device)
    keep[untouched_rows] = True
    keep[dst.batch_size:] = True
    assert dst.n_tiles * 64 > dst.batch_size  # there ARE padding lanes
    keep = keep.view(dst.n_tiles, 1, 64).expand_as(dst.cols)
    assert torch.equal(dst.cols[keep], before["cols"][keep])


def random_index(B_src, B_dst, seed, keep_share=0.25):
    rng = np.random.RandomState(seed)
    index = rng.randint(0, B_src, size=B_dst)  # with repeats
    index[rng.rand(B_dst) < keep_share] = -1
    index[[0, 1, 2, B_dst - 2, B_dst - 1]] = [0, B_src - 1, -1, -1, B_src - 1]  # both ends of src, the last lane of dst
    return index


# ---- 1. the copy is exact -------------------------------------------------------------------------------
def copy_is_exact(device, C, R, pieces, B_src, B_dst):
    src, dst = pair(device, C, R, pieces, B_src, B_dst)
    index = torch.as_tensor(random_index(B_src, B_dst, seed=B_dst), device=device)
    copied, kept = torch.nonzero(index >= 0).flatten(), torch.nonzero(index == -1).flatten()
    assert len(copied) > B_dst // 2 and len(kept) > B_dst // 8
    src_snap, before = snapshot(src), snapshot(dst)
    src_feats, src_nv = (t.clone() for t in src.get_after_states())
    src_best, src_value = (t.clone() for t in src.greedy_actions())

    assert dst.copy_envs_from(src, index) is dst

    assert_copied(dst, src_snap, index, copied)
    assert_untouched(dst, before, kept)
    assert_raw_cols_kept(dst, before, kept)
    at = index[copied].long()
    assert torch.equal(lanes(dst, copied), lanes(src, at))  # every plane word verbatim
    # what the kernels make of the copy: the source's rows bit for bit
    feats, nv = dst.get_after_states()
    assert torch.equal(nv[copied], src_nv[at]) and torch.equal(nv[copied], dst.n_valid[copied])
    assert torch.equal(feats[copied].view(torch.int32), src_feats[at].view(torch.int32))
    best, value = dst.greedy_actions()
    assert torch.equal(best[copied], src_best[at]) and torch.equal(value[copied].view(torch.int32), src_value[at].view(torch.int32))
    # the source is read only; nothing was reported
    assert torch.equal(src.cols, src_snap["cols"]) and torch.equal(src.meta, src_snap["meta"])
    assert dst.stats()["invalid"] == 0
    dst.check()


# ---- 2. the bag travels ------------------------------------------------------------------------------------
def bag_travels(device, C, R, pieces, B=B_SRC):
    src = played(device, C, R, pieces, B, 3, 30, env_offset=1000)
    twin = src.fork(torch.arange(B))
    assert (twin.seed, twin.env_offset, twin.step_idx, twin.auto_reset) == (src.seed, src.env_offset, src.step_idx, True)
    other = src.fork(torch.arange(B), env_offset=5000)
    assert other.env_offset == 5000 and other.step_idx == src.step_idx
    differs = False
    for t in range(20):
        a = src.random_actions().clone()
        want = [x.clone() for x in src.step(a)] + [src.piece.clone(), src.n_valid.clone()]
        got = list(twin.step(a)) + [twin.piece, twin.n_valid]
        for name, w, g in zip(("obs", "reward", "done", "lines", "piece", "n_valid"), want, got):
            assert torch.equal(w.view(torch.int32) if w.dtype == torch.float32 else w,
                               g.view(torch.int32) if g.dtype == torch.float32 else g), "%s at step %d" % (name, t)
        other.step()  # own draws: other pieces, still games
        differs = differs or not torch.equal(other.piece, src.piece)
    assert torch.equal(twin.boards(), src.boards()) and torch.equal(twin.meta, src.meta)
    assert differs
    other.check()
    assert other.stats()["steps"] == 20 * B and other.stats()["invalid"] == 0
    twin.check()


# ---- 3. out-of-range entries ---------------------------------------------------------------------------------
def out_of_range_entries(device, C, R, pieces, B_src, B_dst):
    src, dst = pair(device, C, R, pieces, B_src, B_dst)
    index = np.random.RandomState(5).randint(0, B_src, size=B_dst).astype(np.int64)
    bad = {5: B_src, 70: -2, B_dst - 1: 2**31 - 1}  # wave 0, wave 1, the last lane of the partial tile
    for j, v in bad.items():
        index[j] = v
    index = torch.as_tensor(index, device=device)
    bad_rows = torch.as_tensor(sorted(bad), device=device)
    good_rows = torch.as_tensor([j for j in range(B_dst) if j not in bad], device=device)
    src_snap, before = snapshot(src), snapshot(dst)
    dst.copy_envs_from(src, index)
    assert_untouched(dst, before, bad_rows)
    assert_raw_cols_kept(dst, before, bad_rows)
    assert_copied(dst, src_snap, index, good_rows)
    assert dst.stats()["invalid"] == len(bad)
    per_wave = dst.status.view(-1, 4)[:, 0].cpu().numpy()  # each in the slot of ITS dst wave
    want = np.zeros_like(per_wave)
    for j in bad:
        want[j >> 6] += 1
    np.testing.assert_array_equal(per_wave, want)
    with pytest.raises(IndexError):
        dst.check()


# ---- 4. gather_ in place ---------------------------------------------------------------------------------------
def gather_in_place(device, C, R, pieces, B=B_SRC):
    env = played(device, C, R, pieces, B, 5, 30, env_offset=64)  # (stepped: a call is bound)
    assert env._step_call is not None
    graph = env.capture_steps(2)
    before = env.fork(torch.arange(B))  # the state as it was, by the existing read-outs below
    before_snap = snapshot(before)
    assert torch.equal(before_snap["boards"], env.boards()) and torch.equal(before_snap["meta"], env.meta)
    rng = np.random.RandomState(9)
    perm = rng.permutation(B)
    perm[rng.rand(B) < 0.2] = -1
    perm[B - 1] = 0
    perm = torch.as_tensor(perm, device=device)
    own = torch.arange(B, device=device)
    resolved = torch.where(perm == -1, own, perm)

    assert env.gather_(perm) is env

    want = before.fork(resolved)
    assert_copied(env, before_snap, resolved, own)
    for k in ("boards", "meta", "n_valid", "piece"):
        assert torch.equal(snapshot(env)[k], snapshot(want)[k]), k
    assert env.stats()["invalid"] == 0
    # the env plays on from its new storage exactly as the fork does
    a = want.random_actions().clone()
    got, ref = env.step(a), want.step(a)
    for g, w in zip(got, ref):
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
    assert torch.equal(env.boards(), want.boards()) and torch.equal(env.meta, want.meta)
    assert torch.equal(env.n_valid, want.n_valid) and torch.equal(env.piece, want.piece)
    with pytest.raises(RuntimeError):
        graph.replay()  # captured on the old storage
    # a second gather_ (the spare pair swaps back), with an entry outside the batch: kept and counted
    now = snapshot(env)
    again = torch.roll(own, 1)
    again[7], again[B - 1] = B, -1
    env.gather_(again)
    moved = torch.as_tensor([j for j in range(B) if j not in (7, B - 1)], device=device)
    assert_copied(env, now, again, moved)
    assert_untouched(env, now, torch.as_tensor([7, B - 1], device=device))
    assert env.stats()["invalid"] == 1
    with pytest.raises(IndexError):
        env.check()


# ---- 5. host refusals -----------------------------------------------------------------------------------------
def host_refusals(device):
    from tetris_amd import VecTetris
    env = VecTetris(10, 20, 70, device=device, seed=1)
    ok = torch.zeros(70, dtype=torch.int32)
    for other in (VecTetris(10, 24, 70, device=device), VecTetris(9, 20, 70, device=device),
                  VecTetris(10, 20, 70, device=device, pieces=STANDARD7)):
        with pytest.raises(ValueError):
            env.copy_envs_from(other, ok)
    with pytest.raises(ValueError, match="gather_"):
        env.copy_envs_from(env, ok)
    src = VecTetris(10, 20, 50, device=device, seed=2)
    for index in (torch.zeros(50, dtype=torch.int32), torch.zeros((70, 1), dtype=torch.int32), torch.zeros(70)):
        with pytest.raises(ValueError):
            env.copy_envs_from(src, index)  # src's size, two dimensions, floats
    with pytest.raises(ValueError):
        env.gather_(torch.zeros(71, dtype=torch.int32))
    replay = VecTetris(10, 20, 70, device=device, piece_stream=np.zeros((8, 70), dtype=np.uint8))
    seeded = VecTetris(10, 20, 70, device=device, numpy_seeds=np.arange(70), stream_len=8)
    for bad in (replay, seeded):
        with pytest.raises(ValueError):
            env.copy_envs_from(bad, ok)
        with pytest.raises(ValueError):
            bad.copy_envs_from(env, ok)
        with pytest.raises(ValueError):
            bad.gather_(ok)
        with pytest.raises(ValueError):
            bad.fork(ok)
    with pytest.raises(ValueError):
        env.fork(torch.as_tensor([0, 3, -1]))
    before = snapshot(env)
    env.copy_envs_from(VecTetris(10, 20, 9, device=device, seed=4), ok.tolist())  # anything as_tensor takes
    assert not torch.equal(env.meta, before["meta"])
    env.check()

"""Shared cases for the random half of the library at the ends of its argument ranges: the device bag at every
piece-set size 1..12 (tet::bag_draw_lut through the select table staged in LDS, tet::bag_draw in the reset, the forked
bag of the rollouts) and the 64-bit keys of every draw -- hash_env(hash_key(seed, 4 * step_idx + c), env) -- with seeds
above 2^32, step indices at 2^32 and 2^62 and env offsets at and beyond 2^32.  Each case takes the torch device: "cuda"
(tests/test_bag_keys_gpu.py, the HIP kernels) or "cpu" with the harness backend (tests/test_bag_keys_host.py, the same
per-env bodies and the same C-ABI text compiled by g++).

Everything is bit-exact.  The yardstick is the oracle -- OracleVecEnv, BagSampler(NumpyLegacyRNG) -- and, for the
softmax draw, the NumPy restatement of the header's hash recipe in softmax_cases.uniforms (an env whose two largest
float64 Gumbel values lie within softmax_cases.TOL_Z is ambiguous in float32 and left out, as in
policy_directed_cases).  Two product paths are compared with each other only in shards_across_the_wrap and where a
forked env must step as its parent does.

Piece list of size n: [CATALOGUE[(2 * i + 1) % 9] for i in range(n)] -- all nine pieces by n = 9, repeats beyond.

Geometries, one per select-table layout that tet::env_step reads (tetris_entry.hpp, kernel_variant: u32 words up to
27 rows; packed planes while R + 4 <= 6 * sizeof(word); 10-row chunks up to 20 rows (u32) / 40 rows (u64) of a packed
board, else 12-row chunks):

    geometry  word  planes    step, step_many(random)                                greedy step_many, play, rollouts
    10x20     u32   packed    LutLayout<10>::kSelNib, packed feature entries staged  AfterLut::kSelNib
    10x6      u32   packed    the same kernel; games end every few steps             AfterLut::kSelNib
    12x20     u32   packed    LutLayout<10>::kSelNib, byte tables staged (C > 10)    AfterLut::kSelNib
    10x24     u32   per col.  LutLayout<12>::kSelNib, NCH = 0                        AfterLut::kSelNib
    10x40     u64   packed    LutLayout<10>::kSelNib, NCH = 4                        AfterLut::kSelNib
    10x44     u64   packed    LutLayout<12>::kSelNib, NCH = 4                        AfterLut::kSelNib
    10x45     u64   per col.  LutLayout<12>::kSelNib, NCH = 0                        AfterLut::kSelNib

(PACKW kernels -- those whose policy walks the afterstates -- read AfterLut::kSelNib at every geometry.)  The word size
and the plane count are checked against what the library reports (TetrisDesc.word_bytes, tetris_hip_n_planes).

Coverage asserted from the oracle's outputs alone, per geometry and n (B = 549, 48 steps -- 72 on boards of more
than 40 rows, see STEPS_TALL -- seed 7): at least 100 episodes
ended, every list index seen as a step draw and as the draw after an auto-reset, and for n >= 10 at least 100 draws of
an index >= 9 made while a lower bit of the bag's third nibble was still set.  What the oracle produced (episodes
ended / deep third-nibble draws) is printed by every lock-step case and listed in tests/test_bag_keys_host.py."""
import numpy as np
import torch

import population_cases as pc
import softmax_cases as sc
from population_cases import _t

B = 512 + 37   # a partial last tile and more than one workgroup
STEPS = 48
# Boards of more than 40 rows: the first games under the random policy end between step 45 and step 70, so 48 steps
# end fewer than 100 episodes there (the oracle: 42 / 56 / 48 at 10x44 and 26 / 48 / 29 at 10x45 for n = 4 / 5 / 12, and
# two list indices never follow an auto-reset at 10x45, n = 12).  Those geometries run 72 steps -- the 48 and 24 more,
# compared step by step like the others -- which ends every env's first game (545 .. 549 episodes).
STEPS_TALL = 72
SEED = 7
SIZES_ALL = [1, 2, 3, 4, 5, 8, 9, 10, 11, 12]
SIZES_SOME = [4, 5, 12]
# (C, R): (word bytes, packed planes, select table of step / step_many(random))
LAYOUTS = {
    (10, 20): (4, True, "LutLayout<10>, packed feature entries"),
    (10, 6): (4, True, "LutLayout<10>, packed feature entries"),
    (12, 20): (4, True, "LutLayout<10>, byte tables"),
    (10, 24): (4, False, "LutLayout<12>, NCH = 0"),
    (10, 40): (8, True, "LutLayout<10>, NCH = 4"),
    (10, 44): (8, True, "LutLayout<12>, NCH = 4"),
    (10, 45): (8, False, "LutLayout<12>, NCH = 0"),
}
FULL_GEOMETRIES = [(10, 20), (10, 6)]
OTHER_GEOMETRIES = [(12, 20), (10, 24), (10, 40), (10, 44), (10, 45)]
SET_SIZE_CASES = [(C, R, n) for C, R in FULL_GEOMETRIES for n in SIZES_ALL] + \
                 [(C, R, n) for C, R in OTHER_GEOMETRIES for n in SIZES_SOME]
TWELVE_CASES = [(C, R) for C, R in FULL_GEOMETRIES + OTHER_GEOMETRIES]
MIN_EPISODES, MIN_DEEP = 100, 100
K_MANY, K_GREEDY = 6, 24          # steps per step_many launch; steps of the greedy game
K_PLAY, CHUNK = 24, 8             # the population games: three launches of eight steps
MAX_DROPPED = 0.01                # ambiguous envs of a sampled game (policy_directed_cases.MAX_DROPPED)

# ---- the keys at their edges (10x20, n = 12, 12 steps) -----------------------------------------------------------
KEY_STEPS = 12
KEY_CASES = {
    "seed-0xDEADBEEF00000005": dict(seed=0xDEADBEEF00000005),
    "seed-2^32": dict(seed=2**32),
    "seed-2^64-1": dict(seed=2**64 - 1),
    "offset-2^31-100": dict(env_offset=2**31 - 100),
    "offset-2^32-100": dict(env_offset=2**32 - 100),   # the batch straddles the wrap
    "offset-2^33+7": dict(env_offset=2**33 + 7),
    "step-2^32-6": dict(step_idx0=2**32 - 6),
    "step-2^62-6": dict(step_idx0=2**62 - 6),          # 4 * step_idx wraps 2^64 at the seventh step
}
ROLL_LENGTH, ROLL_N = 3, 2


def steps_for(R):
    return STEPS if R <= 40 else STEPS_TALL


def piece_list(n):
    from tetris_amd.tetromino import CATALOGUE
    return [CATALOGUE[(2 * i + 1) % 9] for i in range(n)]


def bag_bits(meta):
    """the 12 bag bits of meta (bits 52..63), through uint64: an int64 shift would smear bit 63"""
    m = meta.cpu().numpy() if isinstance(meta, torch.Tensor) else np.asarray(meta)
    return ((m.view(np.uint64) >> np.uint64(52)) & np.uint64(0xFFF)).astype(np.uint16)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _eq(got, want, what, tag):
    got, want = _np(got), _np(want)
    if got.dtype == bool or want.dtype == bool:
        got, want = got.astype(bool), want.astype(bool)
    assert got.shape == want.shape, (tag, what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError("%s: %s differs in %d of %d envs; first env %d: got %r, want %r" % (
            tag, what, len(bad), len(got), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist()))


def make_env(device, C, R, n, seed=SEED, env_offset=0, step_idx0=0, batch=B, auto_reset=True):
    """A VecTetris on the piece list of size n; the constructor resets at step index 0, then the index is seated."""
    from tetris_amd import VecTetris
    env = VecTetris(C, R, batch, device=device, pieces=piece_list(n), auto_reset=auto_reset, seed=seed, env_offset=env_offset)
    env.step_idx = step_idx0
    word_bytes, packed, _ = LAYOUTS[(C, R)]
    assert env.desc.word_bytes == word_bytes and (env.n_planes < C) == packed, (C, R, env.desc.word_bytes, env.n_planes)
    return env


def make_ref(orc, C, R, n, seed=SEED, env_offset=0, step_idx0=0, batch=B, auto_reset=True):
    from tetris_amd.tetromino import CATALOGUE
    assert list(orc.CATALOGUE) == list(CATALOGUE)
    ref = orc.OracleVecEnv(C, R, batch, pieces=piece_list(n), auto_reset=auto_reset, seed=seed, env_offset=env_offset, nthreads=0)
    ref.step_idx = step_idx0
    ref.names = piece_list(n)
    return ref


def clone_ref(orc, ref):
    new = orc.OracleVecEnv(ref.C, ref.R, ref.B, pieces=ref.names, auto_reset=bool(ref.auto_reset), seed=ref.seed,
                           env_offset=ref.env_offset, nthreads=ref.nthreads)
    for k in ("cells", "piece", "bag", "n_valid"):
        getattr(new, k)[:] = getattr(ref, k)
    new.step_idx, new.names = ref.step_idx, ref.names
    return new


# ---- the oracle plays alone: computed once per setting, shared, read-only ------------------------------------------
class Trajectory:
    """The oracle's run with the built-in random policy and auto-reset: the state in front of step 0 and, per step,
    piece / action / done / n_valid / lines / reward / bag and the boards (bit-packed); `ref` is the oracle env after
    the last step (clone it before stepping on)."""

    def cells(self, t):
        return np.unpackbits(self.packed[t])[:self.cells_size].reshape(self.cells_shape).view(np.int8)


_TRAJECTORIES = {}
FIELDS = ("piece", "action", "done", "n_valid", "lines", "reward", "bag")


def trajectory(orc, C, R, n, steps=None, **key):
    steps = steps or steps_for(R)
    k = (C, R, n, steps, tuple(sorted(key.items())))
    if k in _TRAJECTORIES:
        return _TRAJECTORIES[k]
    ref = make_ref(orc, C, R, n, **key)
    tr = Trajectory()
    tr.C, tr.R, tr.n, tr.steps, tr.key = C, R, n, steps, key
    tr.piece0, tr.n_valid0, tr.bag0 = ref.piece.copy(), ref.n_valid.copy(), ref.bag.copy()
    for f in FIELDS:
        setattr(tr, f, [])
    tr.packed, tr.cells_shape, tr.cells_size = [], ref.cells.shape, ref.cells.size
    for t in range(steps):
        _, reward, done, lines, n_bad = ref.step()
        assert n_bad == 0
        for f, v in zip(FIELDS, (ref.piece, ref.action, done, ref.n_valid, lines, reward, ref.bag)):
            getattr(tr, f).append(v.copy())
        tr.packed.append(np.packbits(ref.cells.view(np.uint8)))
    for f in FIELDS:
        a = np.stack(getattr(tr, f))
        a.setflags(write=False)
        setattr(tr, f, a)
    tr.ref = ref
    _TRAJECTORIES[k] = tr
    return tr


def coverage(tr):
    """(episodes ended, list indices seen as a step draw, as the draw after an auto-reset, deep third-nibble draws),
    from the oracle's outputs alone.  The piece an env holds after a step is its last draw of that step -- the step
    draw, or the reset draw where the episode ended -- made from the bag it holds afterwards plus that piece's bit."""
    done = tr.done.astype(bool)
    piece = tr.piece.astype(np.int64)
    at_draw = tr.bag.astype(np.int64) | (1 << piece)
    deep = (piece >= 9) & ((at_draw & ((1 << piece) - 1) & 0xF00) != 0)
    return int(done.sum()), set(piece[~done].tolist()), set(piece[done].tolist()), int(deep.sum())


def assert_coverage(tr, tag):
    episodes, step_seen, reset_seen, deep = coverage(tr)
    print("bag coverage %s: episodes ended %d, indices at the step draw %d / %d, after an auto-reset %d / %d, deep "
          "third-nibble draws %d" % (tag, episodes, len(step_seen), tr.n, len(reset_seen), tr.n, deep))
    assert episodes >= MIN_EPISODES, (tag, episodes)
    assert step_seen == set(range(tr.n)) and reset_seen == set(range(tr.n)), (tag, step_seen, reset_seen)
    if tr.n >= 10:
        assert deep >= MIN_DEEP, (tag, deep)
    return episodes, deep


def _check_start(env, tr, tag):
    _eq(env.piece, tr.piece0, "piece after the constructor's reset", tag)
    _eq(env.n_valid, tr.n_valid0, "n_valid after the constructor's reset", tag)
    _eq(bag_bits(env.meta), tr.bag0, "bag bits after the constructor's reset", tag)


def _check_state(env, tr, t, tag):
    when = "after step %d" % t
    _eq(env.piece, tr.piece[t], "piece " + when, tag)
    _eq(env.n_valid, tr.n_valid[t], "n_valid " + when, tag)
    _eq(bag_bits(env.meta), tr.bag[t], "bag bits of meta " + when, tag)
    _eq(env.boards(), tr.cells(t), "boards " + when, tag)


# ---- 1. set sizes through every kernel that draws ---------------------------------------------------------------------
def step_lockstep(device, orc, C, R, n, steps=None, covered=True, **key):
    """step() with the built-in policy and auto-reset against the oracle, every output after every step"""
    steps = steps or steps_for(R)
    tag = "step %dx%d n=%d %r" % (C, R, n, key)
    tr = trajectory(orc, C, R, n, steps, **key)
    figures = assert_coverage(tr, tag) if covered else None
    env = make_env(device, C, R, n, **key)
    _check_start(env, tr, tag)
    for t in range(steps):
        _, reward, done, lines = env.step()
        _eq(env.action, tr.action[t], "action of step %d" % t, tag)
        _eq(done, tr.done[t], "done of step %d" % t, tag)
        _eq(lines, tr.lines[t], "lines of step %d" % t, tag)
        _eq(reward, tr.reward[t], "reward of step %d" % t, tag)
        _check_state(env, tr, t, tag)
    st = env.stats()
    assert (st["invalid"], st["episodes"], st["steps"]) == (0, int(tr.done.sum()), steps * B), (tag, st)
    return figures


def step_many_random(device, orc, C, R, n, steps=None, k_launch=K_MANY, **key):
    """launches of step_many(k_launch), policy 0, against the same oracle steps"""
    steps = steps or steps_for(R)
    tag = "step_many(%d) %dx%d n=%d %r" % (k_launch, C, R, n, key)
    tr = trajectory(orc, C, R, n, steps, **key)
    env = make_env(device, C, R, n, **key)
    out = None
    for t0 in range(0, steps, k_launch):
        out = env.step_many(k_launch, out=out)
        for k in range(k_launch):
            for f in ("piece", "action", "done", "n_valid", "lines", "reward"):
                _eq(out[f][k], getattr(tr, f)[t0 + k], "%s of step %d" % (f, t0 + k), tag)
        _check_state(env, tr, t0 + k_launch - 1, tag)
    assert env.stats()["episodes"] == int(tr.done.sum()) and env.stats()["invalid"] == 0


def _greedy_game(orc, C, R, n, steps, **key):
    """the oracle under the greedy BCTS policy (population_cases.numpy_pick on its own afterstates), auto-reset on"""
    k = ("greedy", C, R, n, steps, tuple(sorted(key.items())))
    if k not in _TRAJECTORIES:
        ref = make_ref(orc, C, R, n, **key)
        w = np.tile(pc.BCTS[None], (B, 1))
        g = dict(action=[], piece=[], done=[], n_valid=[], bag=[], cells=None)
        for t in range(steps):
            feats, nv, _, _ = ref.afterstates()
            action, _ = pc.numpy_pick(feats, nv.astype(np.int64), w)
            _, _, done, _, n_bad = ref.step(action)
            assert n_bad == 0
            for f, v in (("action", action), ("piece", ref.piece), ("done", done), ("n_valid", ref.n_valid), ("bag", ref.bag)):
                g[f].append(v.copy())
        g["cells"] = ref.cells.copy()
        _TRAJECTORIES[k] = g
    return _TRAJECTORIES[k]


def step_many_greedy(device, orc, C, R, n, steps=K_GREEDY, k_launch=K_MANY, **key):
    """launches of step_many(k_launch, policy="greedy"): the draw through AfterLut::kSelNib"""
    tag = "step_many(%d, greedy) %dx%d n=%d %r" % (k_launch, C, R, n, key)
    g = _greedy_game(orc, C, R, n, steps, **key)
    env = make_env(device, C, R, n, **key)
    for t0 in range(0, steps, k_launch):
        out = env.step_many(k_launch, policy="greedy")
        for k in range(k_launch):
            for f in ("action", "piece", "done", "n_valid"):
                _eq(out[f][k], g[f][t0 + k], "%s of step %d" % (f, t0 + k), tag)
        _eq(bag_bits(env.meta), g["bag"][t0 + k_launch - 1], "bag bits after step %d" % (t0 + k_launch - 1), tag)
    _eq(env.boards(), g["cells"], "boards after the last step", tag)
    assert env.stats()["invalid"] == 0
    return int(np.sum(g["done"]))


def stepped(device, orc, C, R, n, steps=None, **key):
    """(env after `steps` calls of step(), a clone of the oracle in the same state)"""
    tr = trajectory(orc, C, R, n, steps, **key)
    env = make_env(device, C, R, n, **key)
    for _ in range(tr.steps):
        env.step()
    _check_state(env, tr, tr.steps - 1, "stepped %dx%d n=%d %r" % (C, R, n, key))
    return env, clone_ref(orc, tr.ref)


def _check_ref(env, ref, when, tag):
    _eq(env.piece, ref.piece, "piece " + when, tag)
    _eq(env.n_valid, ref.n_valid, "n_valid " + when, tag)
    _eq(bag_bits(env.meta), ref.bag, "bag bits of meta " + when, tag)
    _eq(env.boards(), ref.cells, "boards " + when, tag)


def masked_reset(device, orc, C, R, n, steps=None, **key):
    """reset(mask = every third env), the bag kept (tet::bag_draw on the bags the steps left), then
    reset(init_bag=True), against orc_reset_batch"""
    tag = "reset %dx%d n=%d %r" % (C, R, n, key)
    env, ref = stepped(device, orc, C, R, n, steps, **key)
    mask = np.arange(B) % 3 == 0
    everyone = clone_ref(orc, ref)
    everyone.reset()
    for k in ("cells", "piece", "bag", "n_valid"):
        getattr(ref, k)[mask] = getattr(everyone, k)[mask]
    assert len(set(ref.piece[mask].tolist())) == min(n, 12) and bool((ref.cells[mask] == 0).all())
    env.reset(mask=_t(mask, device))
    _check_ref(env, ref, "after reset(mask)", tag)
    ref.reset(init_bag=True)
    env.reset(init_bag=True)
    _check_ref(env, ref, "after reset(init_bag=True)", tag)
    assert int(env.boards().abs().sum()) == 0


MIN_ROLLOUTS_DECIDED = 100


def rollout_start(orc, C, R, n, **key):
    """The number of steps after which the rollouts start: in front of the step that ends the most games of the
    oracle's run, where most boards stand near the top.  (From a low board every three-step rollout returns -2
    whatever it draws, and the comparison would hold for any bag and any key.)"""
    tr = trajectory(orc, C, R, n, **key)
    return max(1, int(np.argmax(tr.done.astype(np.int64).sum(axis=1))))


def rollouts(device, orc, C, R, n=12, **key):
    """rollouts(length=3, n=2), pieces=None (every rollout forks the env's bag), both policies, from the state
    rollout_start steps into the run.  Asserted on the oracle alone: deaths and survivals both occur, and its own
    means under another seed differ in at least 100 entries, so the draws decide what is compared."""
    tag = "rollouts %dx%d n=%d %r" % (C, R, n, key)
    env, ref = stepped(device, orc, C, R, n, rollout_start(orc, C, R, n, **key), **key)
    other = clone_ref(orc, ref)
    other.seed = ref.seed ^ 1
    before = (env.cols.clone(), env.meta.clone())
    for policy in ("random", "greedy"):
        want = ref.rollouts(length=ROLL_LENGTH, n=ROLL_N, policy=policy)
        assert len(np.unique(want[~np.isnan(want)])) > 2, tag
        elsewhere = other.rollouts(length=ROLL_LENGTH, n=ROLL_N, policy=policy)
        decided = int((np.nan_to_num(elsewhere, nan=7.0) != np.nan_to_num(want, nan=7.0)).sum())
        assert decided >= MIN_ROLLOUTS_DECIDED, (tag, policy, decided)
        got = env.rollouts(length=ROLL_LENGTH, n=ROLL_N, policy=policy).cpu().numpy()
        _eq(np.isnan(got), np.isnan(want), "NaN pattern (%s)" % policy, tag)
        _eq(np.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0), "mean returns (%s)" % policy, tag)
    assert torch.equal(env.cols, before[0]) and torch.equal(env.meta, before[1])
    return env, ref


# ---- play / play_sampled against the oracle's games -------------------------------------------------------------------
def _weights():
    W, rows = pc.weight_rows(), pc.oracle_play_rows(B)
    assert set(rows.tolist()) == set(range(len(W)))
    return W, rows


def _population_game(orc, C, R, n, kind, K, T=1.0, **key):
    """K steps of the oracle (no auto-reset, as play ignores it) with env i on weight row oracle_play_rows[i]: "linear"
    takes numpy_pick's action, "softmax" the argmax of the float64 Gumbel values on softmax_cases.uniforms; an env whose
    two largest values lie within TOL_Z at some step is dropped from that step on."""
    k = (kind, C, R, n, K, T, tuple(sorted(key.items())))
    if k in _TRAJECTORIES:
        return _TRAJECTORIES[k]
    ref = make_ref(orc, C, R, n, auto_reset=False, **key)
    W, rows = _weights()
    g = dict(lines=np.zeros(B, np.int64), placed=np.zeros(B, np.int64), dropped=np.zeros(B, bool))
    envs = (ref.env_offset + np.arange(B)) & sc._M
    for _ in range(K):
        feats, nv, _, _ = ref.afterstates()
        nv = nv.astype(np.int64)
        alive = nv > 0
        if kind == "linear":
            action, _ = pc.numpy_pick(feats, nv, W[rows])
        else:
            A = feats.shape[1]
            valid = np.arange(A)[None, :] < nv[:, None]
            u = sc.numpy_logits(feats, W[rows], T)
            U = sc.uniforms(ref.seed, ref.step_idx, envs, A)
            with np.errstate(divide="ignore"):
                z = np.where(valid, u.astype(np.float64) - np.log(-np.log(U)), -np.inf)
            action = np.where(alive, np.argmax(z, axis=1), -1).astype(np.int32)
            zs = np.sort(z, axis=1)
            top, second = zs[:, -1], zs[:, -2]
            with np.errstate(invalid="ignore"):
                gap = np.where(nv > 1, (top - second) / np.maximum(1.0, np.abs(np.where(np.isfinite(top), top, 1.0))), np.inf)
            g["dropped"] |= np.where(np.isnan(gap), 0.0, gap) <= sc.TOL_Z
        _, _, _, ln, n_bad = ref.step(action)
        assert n_bad == int((~alive).sum())
        g["lines"] += np.where(alive, ln, 0)
        g["placed"] += alive
    g.update(cells=ref.cells.copy(), piece=ref.piece.copy(), n_valid=ref.n_valid.copy(), bag=ref.bag.copy(), step_idx=ref.step_idx)
    assert g["dropped"].mean() <= MAX_DROPPED, (k, int(g["dropped"].sum()))
    assert int(g["placed"].sum()) >= 2 * B  # (at 10x6 most games are over within a few pieces)
    _TRAJECTORIES[k] = g
    return g


def _check_population_game(env, res, g, tag):
    kept = ~g["dropped"]
    assert env.step_idx == g["step_idx"], (tag, env.step_idx, g["step_idx"])
    for what, got, want in (("boards", env.boards(), g["cells"]), ("piece", env.piece, g["piece"]),
                            ("n_valid", env.n_valid, g["n_valid"]), ("bag bits of meta", bag_bits(env.meta), g["bag"]),
                            ("lines", _np(res["lines"]).astype(np.int64), g["lines"]),
                            ("pieces", _np(res["pieces"]).astype(np.int64), g["placed"]),
                            ("done", res["done"], g["n_valid"] == 0)):
        _eq(_np(got)[kept], _np(want)[kept], what, tag)
    assert env.stats()["invalid"] == 0


def play(device, orc, C, R, n=12, K=K_PLAY, chunk=CHUNK, **key):
    tag = "play %dx%d n=%d %r" % (C, R, n, key)
    g = _population_game(orc, C, R, n, "linear", K, **key)
    env = make_env(device, C, R, n, **key)
    W, rows = _weights()
    res = env.play(_t(W, device), rows=_t(rows, device), max_steps=K, chunk=chunk)
    _check_population_game(env, res, g, tag)


def play_sampled(device, orc, C, R, n=12, K=K_PLAY, chunk=CHUNK, T=1.0, **key):
    tag = "play_sampled %dx%d n=%d %r" % (C, R, n, key)
    g = _population_game(orc, C, R, n, "softmax", K, T, **key)
    env = make_env(device, C, R, n, **key)
    W, rows = _weights()
    res = env.play_sampled(_t(W, device), rows=_t(rows, device), temperature=T, max_steps=K, chunk=chunk)
    _check_population_game(env, res, g, tag)
    return int(g["dropped"].sum())


# ---- bit 63 of meta on the Python side ---------------------------------------------------------------------------------
def bit63_on_the_host(device, orc, C=10, R=20, n=12, more=6):
    """state_dict -> load_state_dict, fork(arange(B)), gather_(perm) and set_boards reproduce meta bit for bit with
    bit 63 set in some env; the loaded env, the forked env and the parent then step as the oracle does."""
    tag = "bit 63 %dx%d n=%d" % (C, R, n)
    env, ref = stepped(device, orc, C, R, n)
    meta0, cols0, cells0 = env.meta.clone(), env.cols.clone(), env.boards().clone()
    negative = int((meta0 < 0).sum())
    assert negative > 0 and negative == int((ref.bag >> 11).sum()), (tag, negative)  # bit 63 = list index 11 in the bag
    loaded = make_env(device, C, R, n, seed=SEED + 1)
    assert not torch.equal(loaded.meta, meta0)
    loaded.load_state_dict(env.state_dict())
    child = env.fork(torch.arange(B))
    for name, other in (("load_state_dict", loaded), ("fork", child)):
        assert torch.equal(other.meta, meta0) and torch.equal(other.cols, cols0), (tag, name)
        assert other.step_idx == env.step_idx and other.seed == env.seed
    perm = np.random.RandomState(3).permutation(B)
    shuffled = env.fork(torch.arange(B)).gather_(_t(perm, device))
    assert torch.equal(shuffled.meta, meta0[_t(perm, device)]), (tag, "gather_")
    assert torch.equal(shuffled.boards(), cells0[_t(perm, device)]), (tag, "gather_")
    assert int((shuffled.meta < 0).sum()) == negative
    same = env.fork(torch.arange(B))
    same.set_boards(cells0, env.piece)  # rewrites the piece field and the mask around the bag
    assert torch.equal(same.meta, meta0), (tag, "set_boards")
    for t in range(more):
        ref.step()
        for name, e in (("parent", env), ("load_state_dict", loaded), ("fork", child)):
            e.step()
            _eq(e.action, ref.action, "action", tag + " " + name)
            _check_ref(e, ref, "%d steps on" % (t + 1), tag + " " + name)
    return negative


def facade_mask_under_a_full_bag(device):
    """The facade reads the 48 mask bits of its env's meta row; with all twelve bag bits set above them (the facade
    itself replays NumPy's bag, so the kernels leave them zero) it must return the same afterstates."""
    from tetris_amd.game import Tetris
    np.random.seed(5)
    game = Tetris(10, 20, pieces=piece_list(12), device=device)
    for _ in range(4):
        f, _ = game.get_after_states()
        game.step(len(f) // 2)
    want, _ = game.get_after_states()
    game._env.meta[0] |= -(1 << 52)  # bits 52..63 as an int64
    assert int(game._env.meta[0]) < 0 and bag_bits(game._env.meta)[0] == 0xFFF
    got, _ = game.get_after_states()
    assert np.array_equal(got, want) and len(want) > 0


# ---- 2. keys at their edges -----------------------------------------------------------------------------------------------
def keys_sample_and_random_actions(device, orc, steps=KEY_STEPS, C=10, R=20, n=12, T=1.0, **key):
    """Before every step: random_actions() against the action the oracle's built-in policy takes, sample_actions()
    against the float64 Gumbel argmax on softmax_cases.uniforms; then step(random action)."""
    tag = "actions %r" % (key,)
    env, ref = make_env(device, C, R, n, **key), make_ref(orc, C, R, n, **key)
    W, rows = _weights()
    Wm, rows_t = _t(W, device), _t(rows, device)
    envs = (ref.env_offset + np.arange(B)) & sc._M
    dropped = 0
    for t in range(steps):
        assert env.step_idx == ref.step_idx
        feats, nv, _, _ = ref.afterstates()
        nv = nv.astype(np.int64)
        assert nv.min() > 0
        valid = np.arange(feats.shape[1])[None, :] < nv[:, None]
        u = sc.numpy_logits(feats, W[rows], T)
        U = sc.uniforms(ref.seed, ref.step_idx, envs, feats.shape[1])
        with np.errstate(divide="ignore"):
            z = np.where(valid, u.astype(np.float64) - np.log(-np.log(U)), -np.inf)
        zs = np.sort(z, axis=1)
        with np.errstate(invalid="ignore"):
            gap = np.where(nv > 1, (zs[:, -1] - zs[:, -2]) / np.maximum(1.0, np.abs(zs[:, -1])), np.inf)
        clear = ~(np.where(np.isnan(gap), 0.0, gap) <= sc.TOL_Z)
        dropped += int((~clear).sum())
        sampled = env.sample_actions(Wm, rows=rows_t, temperature=T, score=False)[0]
        _eq(_np(sampled)[clear], np.argmax(z, axis=1)[clear], "sample_actions in front of step %d" % t, tag)
        a = env.random_actions().clone()
        env.step(a)
        ref.step()
        _eq(a, ref.action, "random_actions in front of step %d" % t, tag)
        _check_ref(env, ref, "after step %d" % t, tag)
    assert dropped <= MAX_DROPPED * B * steps, (tag, dropped)
    assert env.stats()["invalid"] == 0


def keys_reset_and_rollouts(device, orc, C=10, R=20, n=12, **key):
    """(the rollouts start rollout_start steps in, not 12: see there; the step index stays beyond its edge)"""
    env, ref = rollouts(device, orc, C, R, n, **key)
    tag = "reset %r" % (key,)
    mask = np.arange(B) % 3 == 0
    everyone = clone_ref(orc, ref)
    everyone.reset()
    for k in ("cells", "piece", "bag", "n_valid"):
        getattr(ref, k)[mask] = getattr(everyone, k)[mask]
    env.reset(mask=_t(mask, device))
    _check_ref(env, ref, "after reset(mask)", tag)


def rollout_uid_offset(a_max):
    """an env_offset with (env_offset + i) * a_max * ROLL_N + r crossing 2^32 near the middle of the batch"""
    per_env = a_max * ROLL_N
    off = 2**32 // per_env - B // 2
    assert off * per_env < 2**32 <= (off + B - 1) * per_env
    return off


def keys_rollout_uid(device, orc, C=10, R=20, n=12):
    probe = make_ref(orc, C, R, n, batch=1)
    off = rollout_uid_offset(orc.a_max(probe.desc))
    env, _ = rollouts(device, orc, C, R, n, env_offset=off)
    assert rollout_uid_offset(env.a_max) == off
    return off


def shards_across_the_wrap(device, orc, C=10, R=20, n=12, cut=128, off=2**32 - 100):
    """Two shards of whole tiles -- env_offset below 2^32 and above it -- equal the single batch, which equals the
    oracle: step() x 6, step_many(6), random_actions, rollouts, reset(init_bag=True)."""
    tag = "shards at env_offset 2^32 - 100"
    assert cut % 64 == 0 and off < 2**32 < off + cut
    tr = trajectory(orc, C, R, n, KEY_STEPS, env_offset=off)
    one = make_env(device, C, R, n, env_offset=off)
    parts = [make_env(device, C, R, n, env_offset=off, batch=cut), make_env(device, C, R, n, env_offset=off + cut, batch=B - cut)]
    cat = lambda f: torch.cat([f(p) for p in parts])
    for e in [one] + parts:
        for _ in range(6):
            e.step()
        e.many = e.step_many(6)
    _check_state(one, tr, KEY_STEPS - 1, tag)
    for f in ("piece", "action", "done", "n_valid"):
        _eq(one.many[f][5], getattr(tr, f)[KEY_STEPS - 1], f + " of the last step", tag)
        _eq(cat(lambda p: p.many[f][5]), one.many[f][5], f + " of the last step, shards", tag)
    assert torch.equal(cat(lambda p: p.meta), one.meta) and torch.equal(cat(lambda p: p.boards()), one.boards()), tag
    assert torch.equal(cat(lambda p: p.random_actions().clone()), one.random_actions()), tag
    want = one.rollouts(length=ROLL_LENGTH, n=ROLL_N)
    got = cat(lambda p: p.rollouts(length=ROLL_LENGTH, n=ROLL_N))
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), tag
    for e in [one] + parts:
        e.reset(init_bag=True)
    assert torch.equal(cat(lambda p: p.meta), one.meta) and torch.equal(cat(lambda p: p.piece), one.piece), tag
    ref = clone_ref(orc, tr.ref)
    ref.reset(init_bag=True)
    _check_ref(one, ref, "after reset(init_bag=True)", tag)


def graph_across_the_wrap(device, orc, C=10, R=20, n=12, before=3, k_graph=8, replays=2):
    """capture_steps(8) seated at step_idx = 2^32 - 3 (three plain steps from 2^32 - 6) and replayed twice: the 64-bit
    counter tetris_hip_step_call_run_counted rebuilds on the device, against 3 + 16 oracle steps.  (This case found
    step_kernel putting the counter's halves together from two signed readfirstlane results: a low half of 2^31 or more
    sign-extended over the high half, so replays keyed every step index from 2^31 up wrongly.  The CPU twin adds the
    64-bit counter directly and never showed it.)"""
    tag = "capture_steps(%d) at 2^32 - 3" % k_graph
    key = dict(step_idx0=2**32 - 3 - before)
    tr = trajectory(orc, C, R, n, before + k_graph * replays, **key)
    env = make_env(device, C, R, n, **key)
    for _ in range(before):
        env.step()
    assert env.step_idx == 2**32 - 3
    _check_state(env, tr, before - 1, tag)
    graph = env.capture_steps(k_graph)
    for rep in range(replays):
        _, reward, done, lines = graph.replay()
        t = before + k_graph * (rep + 1) - 1
        assert env.step_idx == 2**32 - 3 + k_graph * (rep + 1)
        _eq(env.action, tr.action[t], "action of step %d" % t, tag)
        _eq(done, tr.done[t], "done of step %d" % t, tag)
        _eq(reward, tr.reward[t], "reward of step %d" % t, tag)
        _check_state(env, tr, t, tag)
    assert env.stats()["episodes"] == int(tr.done.sum()) and env.stats()["steps"] == tr.steps * B


# ---- 3. tetris_hip_numpy_bag_stream ---------------------------------------------------------------------------------------
STREAM_L, STREAM_B = 40, 65


def stream_seeds():
    rng = np.random.RandomState(11)
    seeds = rng.randint(0, 2**32, size=STREAM_B, dtype=np.uint64)
    seeds[:4] = [0, 2**32 - 1, 1, 2**31]
    return seeds


def numpy_bag_stream(device, orc, n):
    """the reference's sampler on NumPy's MT19937 stream for a bag of n pieces, 65 seeds (a wave and one lane)"""
    from tetris_amd import VecTetris
    seeds = stream_seeds()
    got = VecTetris.numpy_piece_stream(seeds, n, STREAM_L, device).cpu().numpy()
    assert got.shape == (STREAM_L, STREAM_B)
    want = np.zeros_like(got)
    for k, s in enumerate(seeds):
        bag = orc.BagSampler(orc.NumpyLegacyRNG(int(s)), n)
        want[:, k] = [bag.next() for _ in range(STREAM_L)]
    _eq(got.T, want.T, "stream (one row per seed)", "numpy_bag_stream n=%d" % n)
    assert set(want.flatten().tolist()) == set(range(n))

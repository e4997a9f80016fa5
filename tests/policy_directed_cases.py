"""The population and softmax kernels -- tetris_hip_policy_greedy_rows, tetris_hip_play_linear,
tetris_hip_policy_softmax_rows, tetris_hip_play_softmax -- against the oracle on the directed boards
(tests/directed_boards.py: the near_top family and the structured boards), one env per (board, catalogue piece), at
every kernel variant of parity_cases.AFTER_GEOMETRY_VARIANTS.  Each case takes the torch device: "cuda"
(tests/test_policy_directed_gpu.py, the HIP kernels) or "cpu" with the harness backend
(tests/test_policy_directed_host.py, the same per-env bodies compiled by g++).

Every yardstick is the oracle's output evaluated in NumPy (float32 left to right for the pick and the logits,
float64 for logz / logp / score and for the Gumbel draw); the one kernel-against-kernel comparison is
play_equals_composition (case 4b), which ties the float totals of tetris_hip_play_softmax down to the last bit once
case 4a has tied its games to the oracle.  The coverage floors are asserted from the oracle alone, before a kernel
runs: a case list that misses one would let a case pass by testing nothing.

Env i evaluates with row oracle_play_rows(n)[i] of weight_rows(): BCTS, its negation, zeros and four random rows, so
that neighbouring lanes differ."""
import numpy as np
import torch

import parity_cases as par
import population_cases as pc
import softmax_cases as sc
from population_cases import _t

PICK_GEOMETRIES = par.AFTER_GEOMETRIES
# one geometry at least of every entry of AFTER_GEOMETRY_VARIANTS, every width 5..12, the one-chunk board, the kernel of
# the last-VGPR hazard, the smallest u64 board and the tallest, widest one (tests/test_policy_directed_host.py asserts it)
PLAY_GEOMETRIES = [(5, 20), (6, 20), (7, 20), (8, 20), (9, 20), (10, 20), (11, 20), (12, 20), (6, 4), (11, 27), (10, 28),
                   (9, 40), (10, 40), (10, 45), (10, 57), (12, 59)]
PLAY_MUST_HOLD = [(6, 4), (9, 40), (10, 28), (12, 59)]
K_PLAY = 6
PLAY_STEP_IDX0 = 1   # the play cases run steps 1..6
PICK_STEP_IDX = 5    # the step whose key the softmax draw of case 2 uses
# (T, feature_directions) of the sampled games: T = 1 everywhere; the hot policy and the directed features where the
# packed u32 and the packed u64 kernels are
SOFTMAX_PLAY_SETTINGS = [(C, R, 1.0, False) for C, R in PLAY_GEOMETRIES] + \
                        [(C, R, T, d) for C, R in ((10, 20), (10, 40)) for T, d in ((20.0, False), (1.0, True))]
T_COLD = 2.0 ** -32  # 1 / T is exact; see softmax_rows_directed
# Coverage floors of the K = 6 games.  What the oracle produced (seed 29, steps 1..6; envs over at entry / ended during /
# alive after / with a cleared line, greedy game | sampled game at T = 1, then the ambiguous envs dropped from it):
#    5x20  B 1153  127  573 | 565  453 | 461  681 | 689  0      11x27  B 1315  175  506 | 506  634 | 634  608 | 616  0
#    6x20  B 1179  125  557 | 561  497 | 493  674 | 676  0      10x28  B 1287  175  512 | 520  600 | 592  587 | 590  0
#    7x20  B 1207  160  528 | 529  519 | 518  640 | 635  0       9x40  B 1261  173  527 | 531  561 | 557  608 | 602  0
#    8x20  B 1233  142  542 | 543  549 | 548  627 | 639  0      10x40  B 1287  184  517 | 520  586 | 583  596 | 593  0
#    9x20  B 1261  157  526 | 529  578 | 575  617 | 623  0      10x45  B 1287  170  499 | 508  618 | 609  598 | 597  1
#   10x20  B 1287  162  537 | 540  588 | 585  608 | 614  0      10x57  B 1287  167  518 | 526  602 | 594  598 | 599  1
#   11x20  B 1315  150  523 | 516  642 | 649  634 | 643  0      12x59  B 1341  166  484 | 493  691 | 682  612 | 609  0
#   12x20  B 1341  185  488 | 492  668 | 664  636 | 636  0        6x4  B  937  150  565 | 568  222 | 219  549 | 551  0
#   T = 20: 10x20  540 585 601, 0 dropped; 10x40  525 578 592, 0.  feature_directions: 10x20  554 571 609, 0; 10x40  552
#   551 596, 1.  The relative gap between the two largest z of the three dropped envs is 5.3e-08, 1.4e-07 and 3.1e-07
#   (TOL_Z = 4.8e-07); in the games without a dropped env the smallest gap is 6.1e-07.
MIN_OVER, MIN_ENDED, MIN_ALIVE, MIN_CLEARED = 100, 200, 200, 300
MIN_ONE_PLACEMENT = 10  # envs with exactly one placement (every geometry of PICK_GEOMETRIES has 156..208)
MIN_COLD_TIED = 20      # envs of the tie-rule check with several placements of maximal fitness (40..94)
MAX_DROPPED = 0.01


def _cases(orc, C, R, order="board-major"):
    cs = par.directed_cases(orc, C, R)
    bix, pcs = cs.after_order(order)
    return cs, bix, pcs


def _device_env(device, cs, bix, pcs, **kw):
    from tetris_amd import VecTetris
    env = VecTetris(cs.C, cs.R, len(bix), device=device, pieces=cs.catalogue, auto_reset=False, seed=par.AFTER_SEED, **kw)
    env.set_boards(cs.boards[bix], pcs)
    return env


def _weights(n):
    W, rows = pc.weight_rows(), pc.oracle_play_rows(n)
    assert set(rows.tolist()) == set(range(len(W)))
    return W, rows


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _per_wave(x, n):
    out = np.zeros((n + 63) // 64, np.int64)
    np.add.at(out, np.arange(n) // 64, np.asarray(x).astype(np.int64))
    return out


# ---- 1. tetris_hip_policy_greedy_rows -----------------------------------------------------------------------------------
def greedy_rows_directed(device, orc, C, R):
    """best_action / best_value bit-exact against numpy_pick on the oracle's valid matrix in both env orders through
    ONE env object, the outputs poisoned before every launch; rows given and rows = NULL with a [B, 8] matrix."""
    figures = par.after_coverage(orc, C, R)
    cs = par.directed_cases(orc, C, R)
    B = figures["B"]
    W, rows = _weights(B)
    Wm, rows_t, Wfull = _t(W, device), _t(rows, device), _t(W[rows], device)
    env = None
    ba = torch.empty(B, dtype=torch.int32, device=device)
    bv = torch.empty(B, dtype=torch.float32, device=device)
    for order in cs.AFTER_ORDERS:
        bix, pcs = cs.after_order(order)
        assert len(bix) == B
        (rf, rnv, _, _), _ = cs.after_reference(orc, order)
        nv = rnv.astype(np.int64)
        want_a, want_v = pc.numpy_pick(rf, nv, W[rows])
        none = nv == 0
        assert (want_a[none] == -1).all() and not want_v[none].view(np.int32).any()
        zero = (rows == 2) & ~none  # the all-zero row: every placement ties, the first wins
        assert zero.sum() >= 50 and not want_a[zero].any()
        if env is None:
            env = _device_env(device, cs, bix, pcs)
        else:
            env.set_boards(cs.boards[bix], pcs)
        env.status.zero_()
        for mode, wt, rt in (("rows", Wm, rows_t), ("rows = NULL", Wfull, None)):
            w = par._Where(cs, "greedy_rows, %s, %s B=%d" % (mode, order, B), bix, pcs)
            ba.fill_(-7)
            bv.fill_(float("nan"))
            pc.raw_greedy_rows(env, wt, rt, ba, bv, env.status)
            w.eq(ba, want_a, "best_action")
            w.eq(_bits(bv), _bits(want_v), "best_value (bits)")
        assert env.stats()["invalid"] == 0
    return figures


# ---- 2. tetris_hip_policy_softmax_rows ----------------------------------------------------------------------------------
def softmax_rows_directed(device, orc, C, R, report=None):
    """Board-major order, every temperature, without and with feature_directions: logits bit-exact against NumPy
    float32 on the oracle's features; logz, logp and score against float64 within TOL; the draw's float64 Gumbel value
    maximal within TOL_Z; envs that are over or have one placement.

    Then the tie rule of the draw, which no finite temperature reaches (two float32 z are equal once in 2^24): at
    T = 2^-32 the logit is the fitness times 2^32, exactly, and where the largest |fitness| is at least 0.5 the float32
    spacing at the largest logit is at least 128 while |log(-log U)| < 17, so z == u for the maximal placements and
    every other z stays below: the action must be the FIRST placement of maximal fitness, numpy_pick's."""
    figures = par.after_coverage(orc, C, R)
    cs, bix, pcs = _cases(orc, C, R)
    B = figures["B"]
    (rf, rnv, _, _), _ = cs.after_reference(orc, "board-major")
    nv = rnv.astype(np.int64)
    n_over, n_one = int((nv == 0).sum()), int((nv == 1).sum())
    assert n_over >= MIN_OVER and n_one >= MIN_ONE_PLACEMENT, (C, R, n_over, n_one)
    W, rows = _weights(B)
    Wm, rows_t = _t(W, device), _t(rows, device)
    A = rf.shape[1]
    valid = np.arange(A)[None, :] < nv[:, None]
    alive = np.nonzero(nv > 0)[0]
    U = sc.uniforms(par.AFTER_SEED, PICK_STEP_IDX, np.arange(B), A)  # (env_offset = 0)
    with np.errstate(divide="ignore"):
        gumbel = -np.log(-np.log(U))
    worst = dict(logz=0.0, logp=0.0, score=0.0, z=0.0, off_argmax=0)
    d32 = np.array(par.DIRS, np.float32)
    for directed in (False, True):
        env = _device_env(device, cs, bix, pcs, **(dict(feature_directions=par.DIRS) if directed else {}))
        assert env.a_max == A
        feats = rf * d32 if directed else rf
        assert feats.dtype == np.float32
        for T in sc.TEMPERATURES:
            w = par._Where(cs, "softmax_rows%s, T=%g B=%d" % (", feature_directions" if directed else "", T, B), bix, pcs)
            out = sc.raw_softmax(env, Wm, rows_t, T, sc.Out(env), env.status, step_idx=PICK_STEP_IDX).numpy()
            action, logp, score, logz, logits = out
            want_u = sc.numpy_logits(feats, W[rows], T)
            w.eq(np.where(valid, logits.view(np.int32), 0), np.where(valid, want_u.view(np.int32), 0), "logits (bits)")
            assert np.all(np.isneginf(logits[~valid])), w.tag
            sc.check_over_envs(out, nv)
            one = nv == 1
            assert not action[one].any() and not logp[one].any() and not score[one].any(), w.tag
            w.eq(_bits(logz), _bits(want_u[:, 0]), "logz of the envs with one placement (bits)", one)
            assert np.all((action[alive] >= 0) & (action[alive] < nv[alive])), w.tag
            for k, v in sc.errors_vs_float64(out, want_u, feats, nv).items():
                worst[k] = max(worst[k], v)
            z64 = np.where(valid, want_u.astype(np.float64) + gumbel, -np.inf)
            top, mine = z64[alive].max(axis=1), z64[alive, action[alive]]
            with np.errstate(invalid="ignore"):
                deficit = np.where(np.isinf(top) & np.isinf(mine), 0.0, top - mine) / np.maximum(1.0, np.abs(np.where(np.isinf(top), 1.0, top)))
            worst["z"] = max(worst["z"], float(deficit.max()))
            worst["off_argmax"] += int((np.argmax(z64[alive], axis=1) != action[alive]).sum())
        if not directed:  # the tie rule
            fitness = sc.numpy_logits(rf, W[rows], 1.0)
            want_a, _ = pc.numpy_pick(rf, nv, W[rows])
            ftop = np.where(valid, fitness, -np.inf).max(axis=1)
            decided = (nv > 0) & (np.abs(np.where(nv > 0, ftop, 0)) >= 0.5) & ~(np.where(valid, U, 0.0) == 1.0).any(axis=1)
            tied = decided & ((np.where(valid, fitness, -np.inf) == ftop[:, None]).sum(axis=1) > 1)
            assert int(tied.sum()) >= MIN_COLD_TIED, (C, R, int(tied.sum()))
            worst["cold_tied"] = int(tied.sum())
            cold = sc.raw_softmax(env, Wm, rows_t, T_COLD, sc.Out(env, score=False, logz=False), env.status,
                                  step_idx=PICK_STEP_IDX).numpy()
            w = par._Where(cs, "softmax_rows, T=2^-32 B=%d" % B, bix, pcs)
            w.eq(cold[0], want_a, "action in the cold limit (the first placement of maximal fitness)", decided)
            w.eq(np.where(valid, cold[4].view(np.int32), 0),
                 np.where(valid, sc.numpy_logits(rf, W[rows], T_COLD).view(np.int32), 0), "logits at T = 2^-32 (bits)")
        assert env.stats()["invalid"] == 0
    worst.update(over=n_over, one_placement=n_one)
    print("policy directed softmax_rows %s %dx%d %s: %r" % (device, C, R, par.after_geometry_variant(C, R), worst))
    if report is not None:
        report.append(((C, R), worst))
    assert worst["logz"] <= sc.TOL and worst["logp"] <= sc.TOL and worst["score"] <= sc.TOL, worst
    assert worst["z"] <= sc.TOL_Z, worst
    return worst


# ---- the oracle plays alone ---------------------------------------------------------------------------------------------
class _Game:
    """What the oracle's K steps from the directed positions left: boards, piece, n_valid, per-env totals, the envs
    over at entry / ended during / alive after, and (sampled game) the float64 sums and the ambiguous envs."""


def _oracle_game(orc, cs, env, kind, T=1.0, directed=False, K=K_PLAY):
    """kind "linear": afterstates -> numpy_pick -> step.  kind "softmax": at step k numpy_logits on the oracle's own
    features, uniforms(seed, step, env, a_max), z in float64, the action its argmax; an env whose two largest z lie
    within TOL_Z (relative to max(1, |z|)) is ambiguous from that step on.  The bag comes from the device meta
    (population_cases.oracle_twin); computed once per setting and shared."""
    key = (kind, T, directed, K)
    cache = cs.__dict__.setdefault("_policy_games", {})
    bag = ((env.meta.cpu().numpy().view(np.uint64) >> np.uint64(52)) & np.uint64(0xFFF)).astype(np.uint16)
    if key in cache:
        assert np.array_equal(cache[key].bag, bag)
        return cache[key]
    ref = pc.oracle_twin(orc, env, cs.catalogue)
    assert ref.step_idx == PLAY_STEP_IDX0
    n = env.batch_size
    W, rows = _weights(n)
    g = _Game()
    g.bag, g.K = bag, K
    g.lines, g.placed, g.ended = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    g.dropped = np.zeros(n, bool)
    g.logp, g.score, g.fmax = np.zeros(n), np.zeros((n, 8)), np.zeros((n, 8))
    g.min_gap = np.inf
    d32 = np.array(par.DIRS, np.float32)
    envs = (env.env_offset + np.arange(n)) & sc._M
    for k in range(K):
        feats, nv, _, _ = ref.afterstates()
        nv = nv.astype(np.int64)
        alive = nv > 0
        if k == 0:
            g.over0 = ~alive
            g.cells0, g.piece0 = ref.cells.copy(), ref.piece.copy()
        if kind == "linear":
            action, _ = pc.numpy_pick(feats, nv, W[rows])
        else:
            f = feats * d32 if directed else feats
            A = f.shape[1]
            valid = np.arange(A)[None, :] < nv[:, None]
            u = sc.numpy_logits(f, W[rows], T)
            Uk = sc.uniforms(env.seed, PLAY_STEP_IDX0 + k, envs, A)
            with np.errstate(divide="ignore"):
                z = np.where(valid, u.astype(np.float64) - np.log(-np.log(Uk)), -np.inf)
            action = np.where(alive, np.argmax(z, axis=1), -1).astype(np.int32)
            zs = np.sort(z, axis=1)
            top, second = zs[:, -1], zs[:, -2]
            with np.errstate(invalid="ignore"):
                gap = np.where(nv > 1, (top - second) / np.maximum(1.0, np.abs(np.where(np.isfinite(top), top, 1.0))), np.inf)
            gap = np.where(np.isnan(gap), 0.0, gap)  # (two U = 1: both +inf)
            g.min_gap = min(g.min_gap, float(gap.min()))
            g.dropped |= gap <= sc.TOL_Z
            logz, p, ef = sc.float64_softmax(u, f, nv)
            idx = np.nonzero(alive)[0]
            f64 = f.astype(np.float64)
            g.logp[idx] += u[idx, action[idx]].astype(np.float64) - logz[idx]
            g.score[idx] += f64[idx, action[idx]] - ef[idx]
            g.fmax = np.maximum(g.fmax, np.abs(np.where(valid[:, :, None], f64, 0.0)).max(axis=1))
        _, _, _, ln, n_bad = ref.step(action)
        assert n_bad == int((~alive).sum())
        g.lines += np.where(alive, ln, 0)
        g.placed += alive
        g.ended |= alive & (ref.n_valid == 0)
    g.alive = ref.n_valid > 0
    g.cells, g.piece, g.n_valid = ref.cells.copy(), ref.piece.copy(), ref.n_valid.copy()
    assert not (g.over0 & (g.placed > 0)).any() and np.array_equal(g.cells[g.over0], g.cells0[g.over0])
    g.figures = dict(C=cs.C, R=cs.R, B=n, over_at_entry=int(g.over0.sum()), ended_during=int(g.ended.sum()),
                     alive_after=int(g.alive.sum()), cleared_a_line=int((g.lines > 0).sum()))
    if kind == "softmax":
        g.figures.update(T=T, directed=directed, dropped=int(g.dropped.sum()), min_gap=g.min_gap)
    print("policy directed %s game %dx%d: %r" % (kind, cs.C, cs.R, g.figures))
    f = g.figures
    assert f["over_at_entry"] >= MIN_OVER and f["ended_during"] >= MIN_ENDED and f["alive_after"] >= MIN_ALIVE, f
    assert f["cleared_a_line"] >= MIN_CLEARED, f
    assert g.dropped.mean() <= MAX_DROPPED, f
    cache[key] = g
    return g


def _poison_padding(env, idx):
    """Sets a bit of the stored words of the envs `idx` that no column owns, where the storage has one: packed boards
    put four columns into three words, and with C % 4 columns left over the top bit of the env's last word is padding
    that unpack_board drops and pack_board writes as zero.  An env rewritten by a launch that should have left it
    alone then differs from what it held.  Returns whether a bit was set."""
    C = env.num_columns
    if env.n_planes == C or C % 4 == 0:
        return False
    idx = torch.as_tensor(idx, device=env.device)
    t, l = idx // 64, idx % 64
    cells = env.boards()
    env.cols[t, env.n_planes - 1, l] = env.cols[t, env.n_planes - 1, l] | torch.iinfo(env.word_dtype).min
    assert torch.equal(env.boards(), cells)  # the decode does not see the bit
    return True


def _start(device, orc, C, R, kind, T=1.0, directed=False):
    """(cases, device env at the directed positions with the padding of the envs over at entry poisoned, the oracle's
    game, a _Where)"""
    cs, bix, pcs = _cases(orc, C, R)
    base = _device_env(device, cs, bix, pcs, **(dict(feature_directions=par.DIRS) if directed else {}))
    base.step_idx = PLAY_STEP_IDX0
    g = _oracle_game(orc, cs, base, kind, T, directed)
    w = par._Where(cs, "%s B=%d" % (kind, len(bix)), bix, pcs)
    rnv = cs.after_reference(orc, "board-major")[0][1]
    w.eq(base.n_valid, rnv, "n_valid after set_boards")
    assert np.array_equal(rnv == 0, g.over0)
    _poison_padding(base, np.nonzero(g.over0)[0])
    return cs, base, g, w


def _check_game(env, base, g, w, when, lines, pcs, n_valid, piece, kept=None):
    """the env after its launches against the oracle's game; the envs over at entry against what `base` holds"""
    n = env.batch_size
    sel = kept
    w.eq(env.boards(), g.cells, "boards, " + when, sel)
    w.eq(piece, g.piece, "piece, " + when, sel)
    w.eq(n_valid, g.n_valid, "n_valid, " + when, sel)
    w.eq(lines.cpu().numpy().astype(np.int64), g.lines, "lines_total, " + when, sel)
    w.eq(pcs.cpu().numpy().astype(np.int64), g.placed, "pieces_total, " + when, sel)
    # the status slots, wave by wave (waves that hold a dropped env are left out)
    got = env.status.view(-1, 4).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    want = np.stack([np.zeros((n + 63) // 64, np.int64), _per_wave(g.ended, n), _per_wave(g.lines, n), _per_wave(g.placed, n)], axis=1)
    assert not got[len(want):].any()  # (tetris_hip_status_words rounds the slot count up)
    got = got[:len(want)]
    whole = np.ones(len(want), bool) if kept is None else _per_wave(~kept, n) == 0
    assert whole.sum() >= len(want) // 2, (w.tag, int(whole.sum()))
    assert np.array_equal(got[whole], want[whole]), (w.tag, when, "status (invalid, episodes, lines, steps) per wave")
    # over at entry: every byte of cols and meta kept (dropped envs included: the oracle alone says they were over)
    idx = torch.as_tensor(np.nonzero(g.over0)[0], device=env.device)
    w.eq(pc.lanes(env.cols, idx), pc.lanes(base.cols, idx), "stored words of the envs over at entry, " + when)
    w.eq(env.meta[idx], base.meta[idx], "meta of the envs over at entry, " + when)
    assert not lines[idx].any() and not pcs[idx].any(), (w.tag, when)


# ---- 3. tetris_hip_play_linear --------------------------------------------------------------------------------------------
def play_linear_directed(device, orc, C, R):
    """One launch of K steps, and launches of 2 + 4 steps, on forks of the directed positions, against the oracle
    playing alone."""
    cs, base, g, w = _start(device, orc, C, R, "linear")
    n = base.batch_size
    W, rows = _weights(n)
    Wm, rows_t = _t(W, device), _t(rows, device)
    for split in ([K_PLAY], [2, 4]):
        env = base.fork(torch.arange(n))
        assert env.step_idx == PLAY_STEP_IDX0 and torch.equal(env.cols, base.cols)
        env.status.zero_()
        lines, pcs = pc.totals(env)
        n_valid, piece = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
        done_k = 0
        for k in split:
            pc.raw_play(env, k, Wm, rows_t, lines, pcs, n_valid, piece, env.status, step_idx0=PLAY_STEP_IDX0 + done_k)
            done_k += k
        assert done_k == g.K
        _check_game(env, base, g, w, "launches of %r steps" % (split,), lines, pcs, n_valid, piece)
    return g.figures


# ---- 4a. tetris_hip_play_softmax against the oracle's sampled game ------------------------------------------------------------
def play_softmax_directed(device, orc, C, R, T=1.0, directed=False):
    """One K-step launch reproduces the oracle's sampled game on the envs that were never ambiguous: boards, piece,
    n_valid and the integer totals exactly, logp_total and score_total against the float64 sums within K * TOL."""
    cs, base, g, w = _start(device, orc, C, R, "softmax", T, directed)
    w.tag += " T=%g%s" % (T, " feature_directions" if directed else "")
    n = base.batch_size
    W, rows = _weights(n)
    Wm, rows_t = _t(W, device), _t(rows, device)
    env = base.fork(torch.arange(n))
    env.status.zero_()
    lines, pcs, logp, score = sc.totals(env)
    n_valid, piece = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
    sc.raw_play(env, g.K, Wm, rows_t, T, lines, pcs, logp, score, n_valid, piece, env.status, step_idx0=PLAY_STEP_IDX0)
    kept = ~g.dropped
    _check_game(env, base, g, w, "one launch of %d steps" % g.K, lines, pcs, n_valid, piece, kept=None if kept.all() else kept)
    logp, score = logp.cpu().numpy().astype(np.float64), score.cpu().numpy().astype(np.float64)
    err_logp = np.abs(logp - g.logp) / np.maximum(1.0, np.abs(g.logp))
    err_score = (np.abs(score - g.score) / np.maximum(1.0, g.fmax)).max(axis=1)
    figures = dict(g.figures, logp_total=float(err_logp[kept].max()), score_total=float(err_score[kept].max()))
    print("policy directed play_softmax %s %dx%d: %r" % (device, C, R, figures))
    bound = g.K * sc.TOL
    for name, err in (("logp_total", err_logp), ("score_total", err_score)):
        bad = kept & ~(err <= bound)
        assert not bad.any(), "%dx%d %s: %s off the float64 sum by %.3g (bound %.3g); first %s" % (
            C, R, w.tag, name, err[bad].max(), bound, w.env(int(np.nonzero(bad)[0][0])))
    assert not logp[g.over0].any() and not score[g.over0].any()
    return figures


# ---- 4b. tetris_hip_play_softmax == K x (tetris_hip_policy_softmax_rows, tetris_hip_step) -----------------------------------------
def play_softmax_composition_directed(device, orc, C, R, T=1.0, directed=False):
    """softmax_cases.play_equals_composition from the directed positions: bit for bit, the float totals included"""
    cs, bix, pcs_ = _cases(orc, C, R)
    base = _device_env(device, cs, bix, pcs_, **(dict(feature_directions=par.DIRS) if directed else {}))
    base.step_idx = PLAY_STEP_IDX0
    n, K = base.batch_size, K_PLAY
    W, rows = _weights(n)
    Wm, rows_t = _t(W, device), _t(rows, device)
    env, twin = base.fork(torch.arange(n)), base.fork(torch.arange(n))
    env.status.zero_()
    twin.status.zero_()
    w = par._Where(cs, "play_softmax == composition T=%g%s B=%d" % (T, " feature_directions" if directed else "", n), bix, pcs_)
    lines, pcs, logp, score = sc.totals(env)
    n_valid, piece = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
    sc.raw_play(env, K, Wm, rows_t, T, lines, pcs, logp, score, n_valid, piece, env.status, step_idx0=PLAY_STEP_IDX0)
    want_logp, want_score, want_lines, want_placed = sc._compose(twin, K, Wm, rows_t, T)
    assert twin.step_idx == PLAY_STEP_IDX0 + K
    w.eq(env.cols.permute(0, 2, 1).reshape(-1, env.n_planes)[:n], twin.cols.permute(0, 2, 1).reshape(-1, twin.n_planes)[:n], "cols")
    w.eq(env.meta, twin.meta, "meta")
    w.eq(n_valid, twin.n_valid, "n_valid")
    w.eq(piece, twin.piece, "piece")
    w.eq(lines.cpu().numpy().astype(np.int64), want_lines, "lines_total")
    w.eq(pcs.cpu().numpy().astype(np.int64), want_placed, "pieces_total")
    w.eq(_bits(logp), _bits(want_logp), "logp_total (bits)")
    w.eq(_bits(score), _bits(want_score), "score_total (bits)")
    got, want = env.status.view(-1, 4), twin.status.view(-1, 4)
    assert torch.equal(got[:, 1:], want[:, 1:])  # episodes, lines, steps
    assert int(got[:, 0].sum()) == 0             # a frozen env is not invalid (the step counts its -1 action)
    frozen = K * n - int(want_placed.sum())
    assert int(want[:, 0].sum()) == frozen
    assert frozen >= MIN_OVER * K and int(want_placed.sum()) >= MIN_ALIVE * K
    assert np.any(want_logp != 0) and np.any(want_score != 0)
    return int(want_placed.sum()), frozen

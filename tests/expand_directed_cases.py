"""Shared cases for tetris_hip_expand_envs (VecTetris.expand_from / expand / two_ply_values) against the oracle on the
directed boards of tests/directed_boards.py, at every column count and every kernel variant expand_kernel is instantiated
for.  Each case takes the torch device: "cuda" (tests/test_expand_directed_gpu.py, the HIP kernel) or "cpu" with the
harness backend (tests/test_expand_directed_host.py, the same per-env body compiled by g++).

Everything is bit-exact and the yardstick is the oracle alone: OracleVecEnv.step in replay mode (the dictated piece is
its stream row) or with its own bag (the drawn piece).  expand_from is never compared with itself or with step().

1. two_generations: the source batch holds one env per (board, catalogue piece) in board-major order; the destination
   batch holds one RUN entry per directed case (board, piece, action) -- through one fixed permutation, so the 64 lanes
   of a wave read parents from all over the source -- with KEPT entries (parent -1, about one in eight) and, for every
   (board, piece), one BAD entry (the first action that is no placement; action 0 for a parent that is over) mixed in
   at fixed positions.  Generation 1 expands src into dst, generation 2 expands dst into a third batch with a hashed
   action of every child and a second dictated piece: a wrong bit of the child's mask with the right popcount becomes
   a wrong placement there.  The refresh kernel's mask is compared after either generation.
2. feature_directions: generation 1 into a batch with direct_by.
3. drawn_same_for_every_child, drawn_at_key_edges, bag_set_sizes: next_piece = NULL against the oracle's bag.

Coverage floors (FLOORS) are asserted per geometry from the oracle's outputs alone, before a kernel runs; what the oracle
produced is printed by lists() and listed in tests/test_expand_directed_host.py."""
import numpy as np
import pytest
import torch

import bag_key_cases as bk
import gather_cases as gc
import parity_cases as par
import population_cases as pc
from population_cases import _t

# parity_cases.DIRECTED_GEOMETRIES and the variant switches that list lacks: u32 planes at the 20 | 21 switch, the
# smallest u64 board, five | six chunks of a u64 board with a plane per column (stored rows 60 | 61), the narrowest
# of the tallest
EXPAND_GEOMETRIES = par.DIRECTED_GEOMETRIES + [(10, 21), (10, 28), (10, 56), (10, 57), (5, 59)]
DIRECTION_GEOMETRIES = [(10, 20), (12, 20), (10, 40)]
DRAWN_GEOMETRIES = [(10, 20), (9, 40), (12, 59)]
SET_SIZE_CASES = [(C, R, n) for C, R in ((10, 20), (10, 45)) for n in (1, 5, 12)]
TWO_PLY_GEOMETRIES = [(10, 40), (12, 59), (11, 27)]
N_NEAR_TOP = 60  # near-top boards of every geometry's DirectedCases (parity_cases.directed_cases' default: shared)
# floors of the coverage conditions: run entries per count of cleared lines 1..4, children that are over under their
# dictated piece, parents that are over
FLOORS = dict(lines=5, children_over=100, parents_over=100)
KEPT, RUN, BAD = 0, 1, 2
KIND_NAMES = ("kept", "run", "bad")
PERM_SEED, SRC_SEED, DST_SEED = 20261021, 41, 11
MASK48 = np.uint64((1 << 48) - 1)
OUTPUTS = ("obs", "reward", "_done", "lines", "n_valid", "piece")


def _hash9(i, salt):
    """a fixed hash of the case index modulo 9: every catalogue piece follows every kind of board"""
    i = np.asarray(i, np.int64)
    return (((i + 1 + 977 * salt) * 2654435761 >> 11) % 9).astype(np.uint8)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _bits(x):
    """float32 as its int32 bits"""
    x = _np(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _popcount48(meta):
    """set bits of the valid mask (meta bits 0..47)"""
    m = np.ascontiguousarray(_np(meta).view(np.uint64) & MASK48)
    return np.unpackbits(m.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def _piece_field(meta):
    return ((_np(meta).view(np.uint64) >> np.uint64(48)) & np.uint64(15)).astype(np.uint8)


class _WhereDst(par._Where):
    """_Where over the destination order: names the kind of the entry too"""

    def __init__(self, L, tag):
        super().__init__(L.cs, tag, L.bix, L.pcs, L.action)
        self.kind, self.parent, self.nxt = L.kind, L.parent, L.nxt

    def env(self, i):
        if self.kind[i] == KEPT:
            return "env %d: kept entry (parent -1)" % i
        return "%s entry, parent %d, %s, next piece %d" % (KIND_NAMES[self.kind[i]], self.parent[i], super().env(i), self.nxt[i])


class ExpandLists:
    """The source and destination lists of one geometry and the oracle's two steps of the run entries, from the oracle
    alone.  Destination order: kind / parent / action / nxt / nxt2 / bix / pcs [N]; pos = the run entries' positions;
    gen1 / gen2 = the oracle's outputs per run entry (row r belongs to dst env pos[r]), read-only."""

    def __init__(self, orc, C, R):
        cs = self.cs = par.directed_cases(orc, C, R, N_NEAR_TOP)
        self.C, self.R = C, R
        nb, npc = len(cs.boards), len(cs.catalogue)
        assert npc == 9
        self.sbix, self.spcs = cs.after_order("board-major")  # src env b * 9 + p = (board b, piece p)
        self.B_src = len(self.sbix)
        n_run, n_bad = cs.n_cases, nb * npc
        order = np.random.RandomState(PERM_SEED).permutation(n_run)
        i = np.arange(n_run)
        run = dict(bix=cs.bix, pcs=cs.pcs, action=cs.act.astype(np.int64), nxt=_hash9(i, 0), nxt2=_hash9(i, 1))
        run = {k: v[order] for k, v in run.items()}
        b, p = np.repeat(np.arange(nb), npc), np.tile(np.arange(npc), nb)
        bad = dict(bix=b, pcs=p, action=cs.n_valid_table[p, b].astype(np.int64), nxt=_hash9(np.arange(n_bad), 2),
                   nxt2=np.zeros(n_bad, np.uint8))
        n_kept = (n_run + n_bad) // 7
        while (n_run + n_bad + n_kept) % 64 == 0:
            n_kept += 1
        N = self.N = n_run + n_bad + n_kept
        kind = np.full(N, RUN, np.int8)
        kept_at = (np.arange(n_kept) * N) // n_kept + 5
        assert kept_at.max() < N and len(np.unique(kept_at)) == n_kept
        kind[kept_at] = KEPT
        rest = np.nonzero(kind == RUN)[0]
        bad_at = rest[(np.arange(n_bad) * len(rest)) // n_bad + 1]
        assert len(np.unique(bad_at)) == n_bad
        kind[bad_at] = BAD
        self.kind = kind
        self.pos, self.bad_at, self.kept_at = np.nonzero(kind == RUN)[0], np.nonzero(kind == BAD)[0], np.nonzero(kind == KEPT)[0]
        assert (len(self.pos), len(self.bad_at), len(self.kept_at)) == (n_run, n_bad, n_kept)
        for k, fill in (("bix", 0), ("pcs", 0), ("action", 0), ("nxt", 0), ("nxt2", 0)):
            a = np.full(N, fill, run[k].dtype)
            a[self.pos], a[self.bad_at] = run[k], bad[k]
            setattr(self, k, a)
        # kept entries: the other arguments are never looked at, whatever they hold
        self.action[self.kept_at] = np.where(np.arange(n_kept) % 2 == 0, 255, 0)
        self.nxt[self.kept_at] = np.where(np.arange(n_kept) % 3 == 0, 200, 1)
        self.parent = np.where(kind == KEPT, -1, self.bix * npc + self.pcs).astype(np.int64)
        live = kind != KEPT
        assert (self.sbix[self.parent[live]] == self.bix[live]).all() and (self.spcs[self.parent[live]] == self.pcs[live]).all()
        assert N % 64 != 0 and self.B_src % 64 != 0
        self.per_wave_bad = np.bincount(self.bad_at >> 6, minlength=(N + 63) // 64)
        # the yardstick: one oracle env per run entry, the dictated pieces as its replay stream
        pos = self.pos
        stream = np.zeros((4, n_run), np.uint8)  # (row 0 goes to the constructor's reset)
        stream[1], stream[2] = self.nxt[pos], self.nxt2[pos]
        ref = orc.OracleVecEnv(C, R, n_run, pieces=cs.catalogue, auto_reset=False, piece_stream=stream, nthreads=0)
        ref.cells[:] = cs.boards[self.bix[pos]]
        ref.piece[:] = self.pcs[pos]
        _, _, _, _, n_wrong = ref.step(self.action[pos])
        assert n_wrong == 0, (C, R, n_wrong)
        self.gen1 = self._outputs(ref)
        self.act2 = par._second_actions(ref.n_valid)
        ref.step(self.act2)
        self.gen2 = self._outputs(ref)
        self.live2 = ref.invalid == 0
        self.per_wave_over = np.bincount(pos[~self.live2] >> 6, minlength=(N + 63) // 64)
        self.figures = self._coverage()

    @staticmethod
    def _outputs(ref):
        out = {k: getattr(ref, k).copy() for k in ("cells", "obs", "reward", "done", "lines", "n_valid", "piece")}
        for v in out.values():
            v.setflags(write=False)
        return out

    def _coverage(self):
        cs, g1, pos = self.cs, self.gen1, self.pos
        hist = np.bincount(g1["lines"], minlength=5)
        parents_over = int((cs.n_valid_table[self.spcs, self.sbix] == 0).sum())
        f = dict(C=self.C, R=self.R, B_src=self.B_src, N=self.N, run=len(pos), bad=len(self.bad_at), kept=len(self.kept_at),
                 lines_hist=hist.tolist(), children_over=int((g1["n_valid"] == 0).sum()), parents_over=parents_over,
                 children_over_in_gen2=int((~self.live2).sum()), lines_hist_gen2=np.bincount(self.gen2["lines"][self.live2], minlength=5).tolist(),
                 rescued=cs.n_rescued, parent_pieces=len(np.unique(self.pcs[pos])), dictated_pieces=len(np.unique(self.nxt[pos])))
        print("expand cases %dx%d: %s" % (self.C, self.R, f))
        assert len(hist) == 5 and (hist[1:] >= FLOORS["lines"]).all(), f
        assert f["children_over"] >= FLOORS["children_over"] and f["parents_over"] >= FLOORS["parents_over"], f
        assert f["parent_pieces"] == 9 and f["dictated_pieces"] == 9 and len(np.unique(self.nxt2[pos])) == 9, f
        assert cs.n_rescued > 0, f
        assert (g1["done"] != 0).sum() == f["children_over"] and 0 < f["children_over_in_gen2"] < len(pos), f
        return f


_LISTS = {}


def lists(orc, C, R):
    if (C, R) not in _LISTS:
        _LISTS[(C, R)] = ExpandLists(orc, C, R)
    return _LISTS[(C, R)]


def geometry_list(device):
    """no duplicates, every column count, every (word, storage, chunks) variant of the afterstate family's list, and
    the variant of every entry is the one the library picks for it"""
    from tetris_amd import VecTetris
    assert len(set(EXPAND_GEOMETRIES)) == len(EXPAND_GEOMETRIES) == len(par.DIRECTED_GEOMETRIES) + 5
    assert {C for C, _ in EXPAND_GEOMETRIES} == set(range(5, 13))
    want = {par.after_geometry_variant(C, R) for C, R in par.AFTER_GEOMETRIES}
    assert want == {v for v, _ in par.AFTER_GEOMETRY_VARIANTS} and len(want) == 5
    seen = set()
    for C, R in EXPAND_GEOMETRIES:
        variant = par.after_geometry_variant(C, R)
        env = VecTetris(C, R, 1, device=device)
        assert env.desc.word_bytes == (4 if variant[0] == "u32" else 8), (C, R)
        assert (env.n_planes < C) == (variant[1] == "packed"), (C, R, env.n_planes)
        seen.add(variant)
    assert seen == want, (seen, want)
    for g in DIRECTION_GEOMETRIES + DRAWN_GEOMETRIES:
        assert g in EXPAND_GEOMETRIES
    assert N_NEAR_TOP == 60 and FLOORS == dict(lines=5, children_over=100, parents_over=100)


# ---- batches ----------------------------------------------------------------------------------------------------------
def _source(device, L, **kw):
    """the source batch: a device-bag env per (board, piece), board-major"""
    from tetris_amd import VecTetris
    cs = L.cs
    src = VecTetris(cs.C, cs.R, L.B_src, device=device, pieces=cs.catalogue, auto_reset=False, seed=SRC_SEED, **kw)
    src.set_boards(cs.boards[L.sbix], L.spcs)
    return src


def _sentinels(env):
    """outputs that are not zero where untouched"""
    for k in ("_obs_buf", "_reward_buf", "_done_buf", "_lines_buf"):
        buf = getattr(env, k)
        buf.copy_(torch.arange(buf.numel(), device=env.device).view_as(buf) % 101 + 1)


def _destination(device, L, seed, steps, **kw):
    """a played batch of L.N envs (untouched is not zero) without auto-reset, its outputs pre-filled"""
    dst = gc.played(device, L.C, L.R, L.cs.catalogue, L.N, seed, steps, **kw)
    dst.auto_reset = False
    assert not dst.status.view(-1, 4)[:, 0].any()
    _sentinels(dst)
    return dst


def _args(L, device, nxt):
    return _t(L.parent, device), _t(L.action, device), (None if nxt is None else _t(nxt, device))


def _compare_children(dst, rows, want, parent_bag, nxt, w, when, sel=None):
    """the run entries `rows` of dst against the oracle's outputs, the meta fields and the mask's popcount"""
    rt = _t(rows, dst.device)
    w.eq(dst.boards()[rt], want["cells"], "boards, " + when, sel)
    w.eq(_bits(dst.obs[rt]), _bits(want["obs"]), "obs (as bits), " + when, sel)
    w.eq(dst.reward[rt], want["reward"], "reward, " + when, sel)
    w.eq(dst.done[rt], want["done"], "done, " + when, sel)
    w.eq(dst.lines[rt], want["lines"], "lines, " + when, sel)
    w.eq(dst.n_valid[rt], want["n_valid"], "n_valid, " + when, sel)
    w.eq(dst.piece[rt], want["piece"], "piece, " + when, sel)
    meta = _np(dst.meta)[rows]
    w.eq(bk.bag_bits(meta), parent_bag, "bag bits of meta (the parent's, unchanged), " + when, sel)
    if nxt is not None:
        w.eq(want["piece"], nxt, "the oracle's piece is the dictated one, " + when, sel)
    w.eq(_piece_field(meta), want["piece"].astype(np.uint8), "piece field of meta, " + when, sel)
    w.eq(_popcount48(meta), want["n_valid"].astype(np.int64), "popcount of the stored mask, " + when, sel)


def _invalid_per_wave(env):
    """the invalid counter of every wave of the batch (the status buffer is padded to whole workgroups: zero there)"""
    slots = _np(env.status.view(-1, 4)[:, 0])
    n_waves = (env.batch_size + 63) // 64
    assert not slots[n_waves:].any()
    return slots[:n_waves]


def _untouched(dst, before, outs_before, rows, per_wave, what):
    """the stored words and the outputs of dst envs `rows` are as they were; the per-wave counters hold `per_wave`"""
    rt = _t(rows, dst.device)
    gc.assert_untouched(dst, before, rt)
    gc.assert_raw_cols_kept(dst, before, rt)
    for k in OUTPUTS:
        got, was = getattr(dst, k), outs_before[k]
        if got.dtype == torch.float32:
            got, was = got.view(torch.int32), was.view(torch.int32)
        assert torch.equal(got[rt], was[rt]), (what, k)
    np.testing.assert_array_equal(_invalid_per_wave(dst), per_wave, err_msg=what)
    assert dst.stats()["invalid"] == int(per_wave.sum()), what
    with pytest.raises(IndexError):
        dst.check()


def _snap_outputs(env):
    return {k: getattr(env, k).clone() for k in OUTPUTS}


# ---- 1. two generations of dictated expansion ----------------------------------------------------------------------------
def two_generations(device, orc, C, R):
    from tetris_amd import VecTetris
    L = lists(orc, C, R)  # (the coverage floors are asserted in there, from the oracle alone)
    cs, pos, N = L.cs, L.pos, L.N
    w = par._Where(cs, "expand, generation 1, N=%d (env r = dst env pos[r], the r-th run entry)" % N, L.bix[pos], L.pcs[pos], L.action[pos])
    wd = _WhereDst(L, "expand, generation 1, N=%d" % N)
    src = _source(device, L)
    par._Where(cs, "expand, source batch", L.sbix, L.spcs).eq(src.n_valid, cs.n_valid_table[L.spcs, L.sbix],
                                                                "n_valid of the source after set_boards")
    src_snap = gc.snapshot(src)
    src_bag = bk.bag_bits(src_snap["meta"])
    dst = _destination(device, L, DST_SEED, 17)
    before, outs_before = gc.snapshot(dst), _snap_outputs(dst)
    parent, action, nxt = _args(L, device, L.nxt)
    assert dst.expand_from(src, parent, action, nxt) is dst
    # generation 1, the run entries
    _compare_children(dst, pos, L.gen1, src_bag[L.parent[pos]], L.nxt[pos], w, "generation 1")
    # kept and bad entries; the source
    _untouched(dst, before, outs_before, np.nonzero(L.kind != RUN)[0], L.per_wave_bad, "generation 1")
    for k in ("cols", "meta", "n_valid", "piece"):
        assert torch.equal(getattr(src, k), src_snap[k]), "the source's %s changed" % k
    # the mask expand stored == the refresh kernel's (kept and bad entries are played envs: theirs holds as well)
    par._refresh_leaves_state(dst, wd, "generation 1")
    # the twin without obs
    twin = VecTetris(C, R, N, device=device, pieces=cs.catalogue, auto_reset=False, seed=DST_SEED, compute_obs=False)
    _sentinels(twin)
    obs_before = twin._obs_buf.clone()
    twin.expand_from(src, parent, action, nxt)
    pt = _t(pos, device)
    w.tag += " compute_obs=False"
    w.eq(gc.lanes(twin, pt), gc.lanes(dst, pt), "stored words of the twin without obs")
    for k in ("meta", "reward", "done", "lines", "n_valid", "piece"):
        w.eq(getattr(twin, k)[pt], getattr(dst, k)[pt], k + " of the twin without obs")
    assert torch.equal(twin._obs_buf, obs_before)
    np.testing.assert_array_equal(_invalid_per_wave(twin), L.per_wave_bad)
    del twin
    # generation 2: every child plays a hashed action under a second dictated piece; the children that were over
    # (the oracle's invalid flags) stay as they are and are counted.  The entries generation 1 did not run have no
    # oracle twin: kept.
    w = par._Where(cs, "expand, generation 2, N=%d (env r = dst env pos[r], the r-th run entry)" % N, L.bix[pos], L.pcs[pos], L.action[pos])
    w.act2 = L.act2
    wd.tag = "expand, generation 2, N=%d" % N
    dst.status.zero_()
    child_snap = gc.snapshot(dst)
    child_bag = bk.bag_bits(child_snap["meta"])
    dst2 = _destination(device, L, DST_SEED + 2, 9)
    before2, outs_before2 = gc.snapshot(dst2), _snap_outputs(dst2)
    parent2 = np.where(L.kind == RUN, np.arange(N), -1)
    action2 = np.zeros(N, np.int64)
    action2[pos] = L.act2
    dst2.expand_from(dst, _t(parent2, device), _t(action2, device), _t(L.nxt2, device))
    _compare_children(dst2, pos, L.gen2, child_bag[pos], L.nxt2[pos], w, "generation 2", sel=L.live2)
    rows = np.nonzero(L.kind != RUN)[0].tolist() + pos[~L.live2].tolist()
    _untouched(dst2, before2, outs_before2, np.array(sorted(rows)), L.per_wave_over, "generation 2")
    for k in ("cols", "meta", "n_valid", "piece"):
        assert torch.equal(getattr(dst, k), child_snap[k]), "the child batch's %s changed" % k
    par._refresh_leaves_state(dst2, wd, "generation 2")
    return L.figures


# ---- 2. feature directions ------------------------------------------------------------------------------------------------
def feature_directions(device, orc, C, R):
    """generation 1 into a batch with direct_by: obs = the oracle's times the directions, everything else the same"""
    from tetris_amd import VecTetris
    L = lists(orc, C, R)
    cs, pos = L.cs, L.pos
    w = par._Where(cs, "expand, feature_directions, N=%d" % L.N, L.bix[pos], L.pcs[pos], L.action[pos])
    src = _source(device, L)
    src_bag = bk.bag_bits(src.meta)
    dst = VecTetris(C, R, L.N, device=device, pieces=cs.catalogue, auto_reset=False, seed=DST_SEED, feature_directions=par.DIRS)
    dst.expand_from(src, *_args(L, device, L.nxt))
    want = dict(L.gen1)
    want["obs"] = L.gen1["obs"] * np.array(par.DIRS, np.float32)
    assert (want["obs"] != L.gen1["obs"]).any()
    _compare_children(dst, pos, want, src_bag[L.parent[pos]], L.nxt[pos], w, "generation 1")
    np.testing.assert_array_equal(_invalid_per_wave(dst), L.per_wave_bad)


# ---- 3. the drawn piece -----------------------------------------------------------------------------------------------------
def drawn_same_for_every_child(device, orc, C, R, env_offset=2**31 - 700, step_idx=7):
    """next_piece = NULL on the lists of two_generations: every child of a parent, wherever it sits in dst, faces the
    piece and holds the bag an oracle twin of the SOURCE draws for that parent at src.step_idx under the parent's
    global id (the source's ids cross 2^31)."""
    L = lists(orc, C, R)
    cs, pos, N = L.cs, L.pos, L.N
    w = par._Where(cs, "expand, drawn piece, N=%d" % N, L.bix[pos], L.pcs[pos], L.action[pos])
    wd = _WhereDst(L, w.tag)
    src = _source(device, L, env_offset=env_offset)
    src.step_idx = step_idx
    assert env_offset < 2**31 < env_offset + L.B_src
    src_snap = gc.snapshot(src)
    twin = pc.oracle_twin(orc, src, cs.catalogue)
    bag_before = twin.bag.copy()
    alive = cs.n_valid_table[L.spcs, L.sbix] > 0
    twin.step(np.zeros(L.B_src, np.int32))  # placement 0 exists wherever one does; the draw does not depend on it
    np.testing.assert_array_equal(twin.invalid == 0, alive)
    par_of = L.parent[pos]
    assert alive[par_of].all()
    want_piece, want_bag = twin.piece[par_of], twin.bag[par_of]
    # from the oracle alone: the draws differ between parents, every piece is drawn, every draw left its bag
    assert len(np.unique(want_piece)) == 9 and (want_bag != bag_before[par_of]).all()
    dst = _destination(device, L, DST_SEED, 17)
    before, outs_before = gc.snapshot(dst), _snap_outputs(dst)
    dst.expand_from(src, *_args(L, device, None))
    assert src.step_idx == step_idx
    pt = _t(pos, device)
    w.eq(dst.piece[pt], want_piece, "piece (the parent's draw)")
    w.eq(bk.bag_bits(dst.meta)[pos], want_bag, "bag bits of meta (the parent's after its draw)")
    w.eq(_piece_field(dst.meta)[pos], want_piece.astype(np.uint8), "piece field of meta")
    first = L.action[pos] == 0  # (the twin played placement 0: these children are its envs)
    assert first.sum() == int((cs.n_valid_table > 0).sum())
    for k, got in (("cells", dst.boards()[pt]), ("n_valid", dst.n_valid[pt]), ("done", dst.done[pt]), ("reward", dst.reward[pt]),
                   ("lines", dst.lines[pt]), ("obs", _bits(dst.obs[pt]))):
        w.eq(got, _bits(getattr(twin, k)[par_of]), k + " of the children of placement 0", first)
    # what does not depend on the piece, against the dictated run's oracle
    w.eq(dst.boards()[pt], L.gen1["cells"], "boards")
    w.eq(dst.lines[pt], L.gen1["lines"], "lines")
    w.eq(_bits(dst.obs[pt]), _bits(L.gen1["obs"]), "obs (as bits)")
    w.eq(_popcount48(dst.meta)[pos], _np(dst.n_valid)[pos].astype(np.int64), "popcount of the stored mask")
    _untouched(dst, before, outs_before, np.nonzero(L.kind != RUN)[0], L.per_wave_bad, "drawn piece")
    for k in ("cols", "meta", "n_valid", "piece"):
        assert torch.equal(getattr(src, k), src_snap[k]), "the source's %s changed" % k
    par._refresh_leaves_state(dst, wd, "drawn piece")


def _drawn_children(device, orc, env, ref, tag, play_on=True):
    """env.expand() (drawn) against a per-parent oracle twin that plays placement 0 without auto-reset: every child's
    piece and bag, the children of placement 0 whole, child.step_idx; then one more step of the child batch in
    lock-step with an oracle batch of the child's size (a child's own draws are keyed by ITS global id) holding the
    twin's envs at the children of placement 0.  Returns the twin."""
    B, A = env.batch_size, env.a_max
    assert env.step_idx == ref.step_idx and bool((ref.n_valid > 0).all())
    twin = bk.clone_ref(orc, ref)
    twin.auto_reset = 0
    _, _, _, _, n_wrong = twin.step(np.zeros(B, np.int32))
    assert n_wrong == 0
    snap, step_idx = gc.snapshot(env), env.step_idx
    child, present = env.expand()
    assert child.step_idx == step_idx + 1 == twin.step_idx and env.step_idx == step_idx
    bk._eq(present, np.arange(A)[None, :] < ref.n_valid[:, None], "present", tag)
    rows = np.nonzero(_np(present).reshape(-1))[0]
    own = rows // A
    bk._eq(_np(child.piece)[rows], twin.piece[own], "piece of every child (its parent's draw)", tag)
    bk._eq(bk.bag_bits(child.meta)[rows], twin.bag[own], "bag bits of every child (its parent's after the draw)", tag)
    bk._eq(_piece_field(child.meta)[rows], twin.piece[own].astype(np.uint8), "piece field of meta of every child", tag)
    first = np.arange(B) * A
    ft = _t(first, device)
    for k, got in (("cells", child.boards()[ft]), ("n_valid", child.n_valid[ft]), ("done", child.done[ft]),
                   ("reward", child.reward[ft]), ("lines", child.lines[ft]), ("obs", _bits(child.obs[ft]))):
        bk._eq(got, _bits(getattr(twin, k)), k + " of the children of placement 0", tag)
    bk._eq(_popcount48(child.meta)[rows], _np(child.n_valid)[rows].astype(np.int64), "popcount of the stored mask", tag)
    assert child.stats()["invalid"] == 0
    assert torch.equal(env.cols, snap["cols"]) and torch.equal(env.meta, snap["meta"]), tag
    if play_on:
        big = orc.OracleVecEnv(ref.C, ref.R, B * A, pieces=ref.names, auto_reset=bool(child.auto_reset), seed=ref.seed,
                               env_offset=ref.env_offset, nthreads=0)
        for k in ("cells", "piece", "bag", "n_valid"):
            getattr(big, k)[first] = getattr(twin, k)
        big.step_idx = twin.step_idx
        a = np.zeros(B * A, np.int32)
        a[first] = par._second_actions(twin.n_valid)
        child.step(_t(a, device))
        big.step(a)
        live = big.invalid[first] == 0
        assert live.sum() > B // 2, (tag, int(live.sum()))
        assert child.step_idx == big.step_idx
        for k, got in (("cells", child.boards()[ft]), ("piece", child.piece[ft]), ("n_valid", child.n_valid[ft]),
                       ("bag", bk.bag_bits(child.meta)[first]), ("done", child.done[ft]), ("reward", child.reward[ft]),
                       ("obs", _bits(child.obs[ft]))):
            bk._eq(_np(got)[live], _bits(getattr(big, k)[first])[live], k + " one step on, children of placement 0", tag)
    return twin


def drawn_at_key_edges(device, orc, name, C=10, R=20, n=12, at=(5, 11)):
    """bag_key_cases.KEY_CASES through expand(): lock-step steps with the oracle, the expansion in front of step 5 (six
    pieces left in the bag) and in front of step 11 (the bags are empty: the draw refills them); the step-index cases
    stand on either side of their edge at the two."""
    key = bk.KEY_CASES[name]
    tag = "expand, drawn, %s" % name
    env, ref = bk.make_env(device, C, R, n, **key), bk.make_ref(orc, C, R, n, **key)
    ids = [key.get("env_offset", 0) + i for i in range(bk.B)]  # (every env is a parent: auto-reset keeps them alive)
    if name == "offset-2^32-100":
        assert min(ids) < 2**32 <= max(ids)  # parents on both sides of the wrap
    popc = lambda bag: np.unpackbits(bag.view(np.uint8).reshape(-1, 2), axis=1).sum(axis=1)
    for t in range(bk.KEY_STEPS):
        if t in at:
            left = popc(ref.bag)
            assert (left == (n - 1 - t) % n).sum() > bk.B // 2, (tag, t)  # (from the oracle: no game has ended yet)
            _drawn_children(device, orc, env, ref, "%s, in front of step %d" % (tag, t))
        env.step()
        ref.step()
        bk._eq(env.action, ref.action, "action of step %d" % t, tag)
        bk._check_ref(env, ref, "after step %d" % t, tag)
    assert max(at) < bk.KEY_STEPS and env.stats()["invalid"] == 0


def bag_set_sizes(device, orc, C, R, n, steps=7):
    """piece lists of 1, 5 and 12 entries: the drawn expansion against the oracle's bag, and a dictated one with
    next_piece = i % (n + 1) through scattered parents: index n is no piece of the set (bad), n - 1 is."""
    tag = "expand, %dx%d n=%d" % (C, R, n)
    env, ref = bk.make_env(device, C, R, n), bk.make_ref(orc, C, R, n)
    for _ in range(steps):
        env.step()
        ref.step()
    bk._check_ref(env, ref, "after %d steps" % steps, tag)
    twin = _drawn_children(device, orc, env, ref, tag + " drawn")
    if n == 1:
        assert not twin.piece.any() and not twin.bag.any()  # piece 0 from a bag refilled and emptied at once
    else:
        assert len(np.unique(twin.piece)) == n
    # dictated
    B = bk.B
    parent = np.random.RandomState(n).permutation(B)
    nxt = (np.arange(B) % (n + 1)).astype(np.uint8)
    good = nxt < n
    assert (nxt == n).sum() > 10 and (nxt == n - 1).sum() > 10
    stream = np.zeros((3, B), np.uint8)
    stream[1] = np.minimum(nxt, n - 1)
    want = orc.OracleVecEnv(C, R, B, pieces=ref.names, auto_reset=False, piece_stream=stream, nthreads=0)
    want.cells[:] = ref.cells[parent]
    want.piece[:] = ref.piece[parent]
    _, _, _, _, n_wrong = want.step(np.zeros(B, np.int32))
    assert n_wrong == 0
    dst = bk.make_env(device, C, R, n, seed=bk.SEED + 1, auto_reset=False)
    _sentinels(dst)
    before, outs_before = gc.snapshot(dst), _snap_outputs(dst)
    dst.expand_from(env, _t(parent, device), torch.zeros(B, dtype=torch.int32, device=device), _t(nxt, device))
    for k, got in (("cells", dst.boards()), ("piece", dst.piece), ("n_valid", dst.n_valid), ("done", dst.done),
                   ("reward", dst.reward), ("lines", dst.lines), ("obs", _bits(dst.obs))):
        bk._eq(_np(got)[good], _bits(getattr(want, k))[good], k + ", dictated", tag)
    bk._eq(_np(dst.piece)[good], nxt[good], "piece == next_piece, dictated", tag)
    bk._eq(_piece_field(dst.meta)[good], nxt[good], "piece field of meta, dictated", tag)
    bk._eq(bk.bag_bits(dst.meta)[good], ref.bag[parent][good], "bag bits (the parent's, unchanged), dictated", tag)
    bk._eq(_popcount48(dst.meta)[good], want.n_valid[good].astype(np.int64), "popcount of the stored mask, dictated", tag)
    _untouched(dst, before, outs_before, np.nonzero(~good)[0], np.bincount(np.nonzero(~good)[0] >> 6, minlength=(B + 63) // 64),
               tag + " dictated")

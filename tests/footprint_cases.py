"""Shared cases for the FOOTPRINT of every C-ABI entry point: what a call writes outside its buffers and inside
them where include/tetris_hip.h says it writes nothing.  Each takes the bound library and the torch device:
tests/test_footprint_host.py runs them on tetris_host_* ("cpu", the CPU harness), tests/test_footprint_gpu.py on
tetris_hip_* ("cuda", the kernels, whose grids are larger than the batch).

Every buffer of a call is one flat uint8 tensor of GUARD + n + GUARD bytes filled with 0xA5, handed over at offset
GUARD; n is exactly the size the header documents for that argument and that B.  GUARD is 64 KiB (a multiple of 16:
the alignment the kernels assume is kept), more than any tail lane of a 512-lane tile can overrun (511 * 32 B on
obs), so an overrun lands in memory the test owns.  After the call:
 (a) both guards of every buffer, inputs included, are still 0xA5;
 (b) every byte the header says the call leaves alone is as it was (`keep`);
 (c) the bytes the call owns equal what the same call of the same library writes into plain buffers that were
     filled with another byte (0x5A) -- a call that writes nothing fails here.
The values themselves are pinned to the oracle elsewhere."""
import ctypes

import numpy as np
import pytest
import torch

GUARD = 64 * 1024
FILL, PLAIN_FILL = 0xA5, 0x5A
PLAIN_SLACK = 1024  # unchecked room behind a plain buffer: what it takes is not this buffer's business

# one geometry per outcome of tet::kernel_variant and word size, and the narrowest board
GEOMETRIES = [
    pytest.param(10, 20, id="10x20-u32-packed-256-lane-tile"),
    pytest.param(10, 24, id="10x24-u32-plane-per-column-512-lane-tile"),
    pytest.param(10, 40, id="10x40-u64-packed"),
    pytest.param(12, 59, id="12x59-u64-plane-per-column"),
    pytest.param(5, 20, id="5x20-narrowest"),
]
# a single lane, a short wave, one env into a second wave, one past a 256-lane block, one past a 512-lane tile
BATCHES = [1, 63, 65, 257, 513]
ROLLOUT_BATCHES = [1, 65, 257]  # (B * a_max lanes)
FIRST_512_TILE_BATCH = 65537    # 10x20: the first size on the 512-lane variant of the step kernel
SEED = 3
WEIGHTS = (ctypes.c_float * 8)(-24.04, -19.77, -13.08, -12.63, -10.49, -9.22, 6.6, -1.61)  # game.py:111-118


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


class Geo:
    """descriptor and sizes of one geometry on one library"""

    def __init__(self, lib, C, R):
        from tetris_amd import _lib
        from tetris_amd.tetromino import CATALOGUE, resolve_pieces
        names = resolve_pieces("default")
        ids = (ctypes.c_int32 * len(names))(*[CATALOGUE.index(n) for n in names])
        self.desc = _lib.TetrisDesc()
        assert lib.desc_init(ctypes.byref(self.desc), C, R, ids, len(names), None) == 0
        self.lib, self.C, self.R = lib, C, R
        self.d = ctypes.byref(self.desc)
        self.wb, self.a_max, self.n_pieces = int(self.desc.word_bytes), int(self.desc.a_max), int(self.desc.n_pieces)
        self.n_planes = int(lib.n_planes(self.d))
        assert self.n_planes > 0

    def cols_bytes(self, B):
        words = int(self.lib.board_words(self.d, B))
        assert words == (B + 63) // 64 * self.n_planes * 64
        return words * self.wb

    def status_bytes(self, B):
        return int(self.lib.status_words(B)) * 4

    def kept_lanes(self, B, kept, device):
        """byte mask over `cols` (word[tile][plane][lane]): the lanes of the envs in `kept` (bool [B] or None) and
        the padding lanes of the last tile"""
        tiles = (B + 63) // 64
        slots = torch.ones(tiles * 64, dtype=torch.bool, device=device)
        slots[:B] = False if kept is None else kept
        return slots.view(tiles, 1, 64).expand(tiles, self.n_planes, 64).reshape(-1).repeat_interleave(self.wb)


def _elems(mask, size):
    """bool per element -> bool per byte"""
    return mask.repeat_interleave(size)


class Buf:
    def __init__(self, nbytes, device, guarded, init, keep, loose):
        g, tail = (GUARD, GUARD) if guarded else (0, PLAIN_SLACK)
        self.raw = torch.full((g + nbytes + tail,), FILL if guarded else PLAIN_FILL, dtype=torch.uint8, device=device)
        self.body, self.front, self.back = self.raw[g:g + nbytes], self.raw[:g], self.raw[g + nbytes:]
        if init is not None:
            self.body.copy_(_bytes(init))
        self.ptr = self.raw.data_ptr() + g
        assert self.ptr % 16 == 0
        self.keep, self.loose, self.before = keep, loose, None

    def mask(self, m):
        if m is None or m is False:
            return torch.zeros(self.body.numel(), dtype=torch.bool, device=self.body.device)
        if m is True:
            return torch.ones(self.body.numel(), dtype=torch.bool, device=self.body.device)
        assert m.dtype == torch.bool and m.numel() == self.body.numel()
        return m


class Arena:
    """the buffers of one call: guarded (0xA5 all round) or plain (0x5A, nothing checked around them)"""

    def __init__(self, device, guarded):
        self.device, self.guarded, self.bufs = device, guarded, {}

    def new(self, name, nbytes=None, init=None, keep=None, loose=None):
        """keep: None = an output the call owns wholly; True = the call may not write it (an input); a bool mask
        per byte = those bytes stay.  loose: bytes the header leaves open (neither checked).  An output starts as
        the fill, or as `init` (in/out arguments, and outputs whose kept bytes should differ from the fill)."""
        assert name not in self.bufs
        if nbytes is None:
            nbytes = _bytes(init).numel()
        self.bufs[name] = Buf(int(nbytes), self.device, self.guarded, init, keep, loose)
        return self.bufs[name].ptr

    def launch(self, fn, *args):
        for b in self.bufs.values():
            b.before = b.body.clone()
        _sync(self.device)
        rc = fn(*args)
        _sync(self.device)
        assert rc == 0, "%s returned %d" % (getattr(fn, "__name__", fn), rc)


def footprint(device, call):
    """call(arena) allocates the buffers of ONE entry-point call through arena.new and makes it through
    arena.launch.  Runs it on guarded and on plain buffers; checks (a), (b), (c) of every buffer and reports all
    that failed at once."""
    guarded, plain = Arena(device, True), Arena(device, False)
    call(guarded)
    call(plain)
    assert list(guarded.bufs) == list(plain.bufs)
    bad = []
    for name, b in guarded.bufs.items():
        for side, part in (("front", b.front), ("back", b.back)):
            hit = torch.nonzero(part != FILL).flatten()
            if hit.numel():  # (a)
                bad.append("%s: %d bytes of the %s guard written, offsets %d..%d of it" %
                           (name, hit.numel(), side, int(hit[0]), int(hit[-1])))
        keep, loose = b.mask(b.keep), b.mask(b.loose)
        changed = torch.nonzero(keep & (b.body != b.before)).flatten()
        if changed.numel():  # (b)
            bad.append("%s: %d bytes the call must leave alone changed, first at byte %d" % (name, changed.numel(), int(changed[0])))
        own = ~keep & ~loose
        differs = torch.nonzero(own & (b.body != plain.bufs[name].body)).flatten()
        if differs.numel():  # (c)
            bad.append("%s: %d owned bytes differ from the call into plain buffers, first at byte %d" %
                       (name, differs.numel(), int(differs[0])))
    assert bad == [], "\n".join(bad)
    return guarded, plain


# ---- inputs: states the library itself produced --------------------------------------------------------
_GEOS, _STATES = {}, {}


def geometry(lib, C, R):
    key = (lib.device_type, C, R)
    if key not in _GEOS:
        _GEOS[key] = Geo(lib, C, R)
    return _GEOS[key]


def _one_per_wave(B, device):
    """bool [B]: one env of every wave, at another lane each (the last wave: within B)"""
    m = torch.zeros(B, dtype=torch.bool, device=device)
    for w in range((B + 63) // 64):
        m[min(64 * w + (5 * w + 3) % 64, B - 1)] = True
    return m


def state(lib, device, C, R, B, seed=SEED, steps=6, replay_len=0):
    """(geo, dict of tensors): B envs after a reset and `steps` steps of the built-in policy with auto-reset, in
    plain buffers; the padding lanes of cols hold 0xA5.  replay_len: the replay-stream form instead (a random
    stream of that many rows, a reset that consumed row 0, no steps).  Built once per key; callers get copies."""
    geo = geometry(lib, C, R)
    key = (lib.device_type, C, R, B, seed, steps, replay_len)
    if key not in _STATES:
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=device)
        s = dict(cols=torch.full((geo.cols_bytes(B),), FILL, dtype=torch.uint8, device=device), meta=z(B, torch.int64),
                 piece=z(B, torch.uint8), n_valid=z(B, torch.uint8), status=z(geo.status_bytes(B) // 4, torch.int32))
        p = lambda k: s[k].data_ptr()
        if replay_len:
            gen = torch.Generator().manual_seed(seed)
            s["stream"] = torch.randint(0, geo.n_pieces, (replay_len, B), generator=gen).to(torch.uint8).to(device)
            s["cursor"] = z(B, torch.int32)
            assert lib.reset(geo.d, p("cols"), p("meta"), None, p("piece"), p("n_valid"), p("stream"), p("cursor"), replay_len,
                             p("status"), 1, seed, 0, 0, B, None) == 0
        else:
            assert lib.reset(geo.d, p("cols"), p("meta"), None, p("piece"), p("n_valid"), None, None, 0, p("status"), 1,
                             seed, 0, 0, B, None) == 0
            obs, reward, done, lines = z(B * 8, torch.float32), z(B, torch.int32), z(B, torch.uint8), z(B, torch.uint8)
            for t in range(steps):
                assert lib.step(geo.d, p("cols"), p("meta"), None, None, None, None, 0, obs.data_ptr(), reward.data_ptr(),
                                done.data_ptr(), lines.data_ptr(), p("n_valid"), p("piece"), p("status"), 1, seed, t, 0, B,
                                None) == 0
        _sync(device)
        s["cols"][geo.kept_lanes(B, None, device)] = FILL
        s["step_idx"] = steps
        _STATES[key] = s
    return geo, {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in _STATES[key].items()}


def _host_call_room(lib):
    """caller-owned HOST memory for a bound step call, 16-byte aligned (the owner is returned with the address)"""
    raw = ctypes.create_string_buffer(int(lib.step_call_size()) + 16)
    return raw, (ctypes.addressof(raw) + 15) & ~15


# ---- the step family -------------------------------------------------------------------------------------
STEP_FORMS = [("step", "policy"), ("step", "actions"), ("step", "replay"), ("run", "actions"), ("gather", "policy"),
              ("gather", "actions"), ("gather", "replay"), ("counted", "policy")]


def step_family(lib, device, C, R, B, how, mode):
    """how: tetris_*_step, or the bound call run plainly ("run"), with the gather payload ("gather"), or with its
    step index on the device ("counted").  mode: "policy" (action NULL: every env plays), "actions" (given, one env
    per wave out of range: its board and meta stay), "replay" (stream / cursor, action NULL, one env per wave
    with a stream too short for a step under auto-reset: board, meta and cursor stay)."""
    L = 4 if mode == "replay" else 0
    geo, st = state(lib, device, C, R, B, replay_len=L)
    bad = _one_per_wave(B, device) if mode != "policy" else torch.zeros(B, dtype=torch.bool, device=device)
    action = None
    if mode == "actions":
        action = torch.zeros(B, dtype=torch.int32, device=device)
        assert lib.policy_random(st["n_valid"].data_ptr(), action.data_ptr(), SEED, st["step_idx"], 0, B, None) == 0
        _sync(device)
        wave = torch.arange(B, device=device) // 64
        action[bad] = torch.where(wave[bad] % 2 == 0, geo.a_max + 1, -3).to(torch.int32)
    if mode == "replay":
        st["cursor"][bad] = L - 1  # one row left: not enough for a step that may end the episode under auto-reset
    step_idx = st["step_idx"]

    def call(A):
        cols = A.new("cols", init=st["cols"], keep=geo.kept_lanes(B, bad, device))
        meta = A.new("meta", init=st["meta"], keep=_elems(bad, 8))
        act = A.new("action", init=action, keep=True) if action is not None else None
        # bound calls write action_out only when the built-in policy drew the action
        act_out = None if (how == "step" and action is not None) else A.new("action_out", 4 * B, keep=action is not None)
        stream = A.new("stream", init=st["stream"], keep=True) if L else None
        cursor = A.new("cursor", init=st["cursor"], keep=_elems(bad, 4)) if L else None
        obs, reward = A.new("obs", 32 * B), A.new("reward", 4 * B)
        done, lines, n_valid, piece = A.new("done", B), A.new("lines", B), A.new("n_valid_next", B), A.new("piece_next", B)
        status = A.new("status", init=st["status"])
        assert _bytes(st["status"]).numel() == geo.status_bytes(B)
        if how == "step":
            A.launch(lib.step, geo.d, cols, meta, act, act_out, stream, cursor, L, obs, reward, done, lines, n_valid, piece,
                     status, 1, SEED, step_idx, 0, B, None)
            return
        owner, room = _host_call_room(lib)
        assert lib.step_call_init(room, geo.d, cols, meta, act_out, stream, cursor, L, obs, reward, done, lines, n_valid,
                                  piece, status, 1, SEED, 0, B) == 0
        if how == "run":
            A.launch(lib.step_call_run, room, act, step_idx, None)
        elif how == "gather":
            waves = (B + 63) // 64
            bits = A.new("done_bits", 8 * waves)  # uint64[ceil(B / 64)]: the header's size
            # the slots of the waves that hold envs are the copy the header promises; the rest of the
            # status_words(B) round-up holds no counters and is left open
            live = torch.arange(geo.status_bytes(B), device=device) < 16 * waves
            snap = A.new("status_snapshot", geo.status_bytes(B), loose=~live)
            A.launch(lib.step_call_run_gather, room, act, step_idx, bits, snap, None)
        else:
            counter = A.new("step_counter", init=torch.tensor([step_idx - 1], dtype=torch.int64), keep=True)
            A.launch(lib.step_call_run_counted, room, act, counter, 1, None)
        del owner

    g, p = footprint(device, call)
    if mode == "policy":  # the state moved: every env played
        assert not torch.equal(g.bufs["meta"].body, g.bufs["meta"].before)
    if how == "gather":  # the payload is the done array and the counters of this very call
        waves = (B + 63) // 64
        assert torch.equal(g.bufs["status_snapshot"].body[:16 * waves], g.bufs["status"].body[:16 * waves])
        want = torch.zeros(8 * waves, dtype=torch.uint8, device=device)
        assert lib.pack_done_bits(p.bufs["done"].ptr, want.data_ptr(), B, None) == 0
        _sync(device)
        assert torch.equal(g.bufs["done_bits"].body, want)


def step_many(lib, device, C, R, B, policy, K=3):
    """[K][B] trajectory buffers of exactly K * B elements: nothing past them"""
    geo, st = state(lib, device, C, R, B)

    def call(A):
        cols = A.new("cols", init=st["cols"], keep=geo.kept_lanes(B, None, device))
        meta = A.new("meta", init=st["meta"])
        n = K * B
        A.launch(lib.step_many, geo.d, cols, meta, K, policy, WEIGHTS if policy == 1 else None, A.new("action_out", 4 * n),
                 A.new("obs", 32 * n), A.new("reward", 4 * n), A.new("done", n), A.new("lines", n), A.new("n_valid_next", n),
                 A.new("piece_next", n), A.new("status", init=st["status"]), 1, SEED, st["step_idx"], 0, B, None)

    g, _ = footprint(device, call)
    assert not torch.equal(g.bufs["meta"].body, g.bufs["meta"].before)


# ---- reset, refresh ---------------------------------------------------------------------------------------
def reset(lib, device, C, R, B, masked):
    geo, st = state(lib, device, C, R, B)
    kept = None
    if masked:
        kept = torch.rand(B, generator=torch.Generator().manual_seed(B)).to(device) < 0.5
        kept[B - 1] = B > 1  # the last env of the partial tile stays (B = 1: it resets)
        kept[0] = False

    def call(A):
        k1 = True if kept is None else _elems(kept, 1)
        mask = A.new("reset_mask", init=(~kept).to(torch.uint8), keep=True) if masked else None
        A.launch(lib.reset, geo.d, A.new("cols", init=st["cols"], keep=geo.kept_lanes(B, kept, device)),
                 A.new("meta", init=st["meta"], keep=None if kept is None else _elems(kept, 8)), mask,
                 A.new("piece_out", init=st["piece"] + 100, keep=k1 if masked else None),
                 A.new("n_valid_out", init=st["n_valid"] + 100, keep=k1 if masked else None), None, None, 0,
                 A.new("status", init=st["status"], keep=True),  # (only a replay reset past its stream counts)
                 0 if masked else 1, SEED, st["step_idx"], 0, B, None)

    footprint(device, call)


def refresh(lib, device, C, R, B):
    geo, st = state(lib, device, C, R, B)
    st["meta"] &= ~((1 << 48) - 1)  # the valid mask is what the call recomputes: start without it

    def call(A):
        A.launch(lib.refresh, geo.d, A.new("cols", init=st["cols"], keep=True), A.new("meta", init=st["meta"]),
                 A.new("n_valid_out", B), B, None)

    g, _ = footprint(device, call)
    assert torch.equal(g.bufs["n_valid_out"].body, st["n_valid"])


# ---- the afterstate family ---------------------------------------------------------------------------------
AFTER_LAYOUTS = ["env_major", "env_major_gaps", "action_major"]


def afterstates(lib, device, C, R, B, layout, with_all):
    """the feature matrix in three stride forms; the floats between rows and after each env's rows stay 0xA5"""
    geo, st = state(lib, device, C, R, B)
    a = geo.a_max
    if layout == "env_major":
        rs, es, n = 8, a * 8, B * a * 8
    elif layout == "env_major_gaps":  # four floats between rows and four after each env
        rs, es = 12, a * 12 + 4
        n = B * es
    else:
        rs, es, n = B * 8, 8, a * B * 8
    rows = torch.zeros(n, dtype=torch.bool, device=device)
    at = (torch.arange(B, device=device) * es).view(B, 1, 1) + (torch.arange(a, device=device) * rs).view(1, a, 1) + \
        torch.arange(8, device=device).view(1, 1, 8)
    rows[at.flatten()] = True
    assert int(rows.sum()) == B * a * 8
    gaps = _elems(~rows, 4)

    def call(A):
        A.launch(lib.afterstates, geo.d, A.new("cols", init=st["cols"], keep=True), A.new("meta", init=st["meta"], keep=True),
                 A.new("feats", 4 * n, keep=gaps), A.new("n_valid", B), A.new("feats_all", 4 * n, keep=gaps) if with_all else None,
                 A.new("n_all", B) if with_all else None, es, rs, B, None)

    g, _ = footprint(device, call)
    assert torch.equal(g.bufs["n_valid"].body, st["n_valid"])


def policy_greedy(lib, device, C, R, B):
    geo, st = state(lib, device, C, R, B)

    def call(A):
        A.launch(lib.policy_greedy, geo.d, A.new("cols", init=st["cols"], keep=True), A.new("meta", init=st["meta"], keep=True),
                 WEIGHTS, A.new("best_action", 4 * B), A.new("best_value", 4 * B), A.new("fitness_all", 4 * B * geo.a_max), B, None)

    footprint(device, call)


def rollouts(lib, device, C, R, B, policy, length=2, n=2):
    """policy 0 on fed pieces, policy 1 on each rollout's own bag"""
    geo, st = state(lib, device, C, R, B)
    fed = None
    if policy == 0:
        gen = torch.Generator().manual_seed(B)
        fed = torch.randint(0, geo.n_pieces, (B * geo.a_max * n * length,), generator=gen).to(torch.uint8).to(device)

    def call(A):
        A.launch(lib.rollouts, geo.d, A.new("cols", init=st["cols"], keep=True), A.new("meta", init=st["meta"], keep=True),
                 A.new("returns", 8 * B * geo.a_max), length, n, policy, WEIGHTS if policy == 1 else None,
                 A.new("pieces", init=fed, keep=True) if fed is not None else None, SEED, st["step_idx"], 0, B, None)

    footprint(device, call)


# ---- copies and conversions ----------------------------------------------------------------------------------
def gather_envs(lib, device, C, R, B, B_src=200):
    """dst (B envs) from a source of 200: a quarter kept (-1), one entry per wave out of range"""
    geo, src = state(lib, device, C, R, B_src, seed=11, steps=9)
    _, dst = state(lib, device, C, R, B)
    gen = torch.Generator().manual_seed(B)
    index = torch.randint(0, B_src, (B,), generator=gen).to(torch.int32)
    index[torch.rand(B, generator=gen) < 0.25] = -1
    index = index.to(device)
    bad = _one_per_wave(B, device)
    if B > 1:
        bad[0] = False
        index[0] = B_src - 1
    index[bad] = torch.where((torch.arange(B, device=device) // 64)[bad] % 2 == 0, B_src, -2).to(torch.int32)
    kept = (index == -1) | bad
    k1 = _elems(kept, 1)

    def call(A):
        A.launch(lib.gather_envs, geo.d, A.new("src_cols", init=src["cols"], keep=True), A.new("src_meta", init=src["meta"], keep=True),
                 B_src, A.new("dst_cols", init=dst["cols"], keep=geo.kept_lanes(B, kept, device)),
                 A.new("dst_meta", init=dst["meta"], keep=_elems(kept, 8)), A.new("dst_n_valid", init=dst["n_valid"] + 100, keep=k1),
                 A.new("dst_piece", init=dst["piece"] + 100, keep=k1), A.new("index", init=index, keep=True),
                 A.new("status", init=dst["status"]), B, None)

    g, _ = footprint(device, call)
    invalid = g.bufs["status"].body.view(torch.int32).view(-1, 4)[:, 0] - dst["status"].view(-1, 4)[:, 0]
    assert int(invalid.sum()) == int(bad.sum())


def pack_done_bits(lib, device, B):
    done = torch.randint(0, 3, (B,), generator=torch.Generator().manual_seed(B)).to(torch.uint8).to(device)

    def call(A):
        A.launch(lib.pack_done_bits, A.new("done", init=done, keep=True), A.new("bits", 8 * ((B + 63) // 64)), B, None)

    g, _ = footprint(device, call)
    bits = g.bufs["bits"].body.cpu().numpy()
    assert np.array_equal(np.unpackbits(bits, bitorder="little")[:B], (done != 0).cpu().numpy().astype(np.uint8))


def policy_random(lib, device, B):
    n_valid = torch.randint(0, 37, (B,), generator=torch.Generator().manual_seed(B)).to(torch.uint8).to(device)

    def call(A):
        A.launch(lib.policy_random, A.new("n_valid", init=n_valid, keep=True), A.new("action", 4 * B), SEED, 5, 0, B, None)

    footprint(device, call)


def decode(lib, device, C, R, B):
    geo, st = state(lib, device, C, R, B)

    def call(A):
        A.launch(lib.decode, geo.d, A.new("cols", init=st["cols"], keep=True), A.new("cells", B * (R + 4) * C),
                 A.new("heights", 4 * B * C), B, None)

    footprint(device, call)


def encode(lib, device, C, R, B):
    """cells of a played state into storage that holds 0xA5 everywhere: the padding lanes keep it"""
    geo, st = state(lib, device, C, R, B)
    cells = torch.zeros(B * (R + 4) * C, dtype=torch.int8, device=device)
    assert lib.decode(geo.d, st["cols"].data_ptr(), cells.data_ptr(), None, B, None) == 0
    _sync(device)

    def call(A):
        A.launch(lib.encode, geo.d, A.new("cells", init=cells, keep=True),
                 A.new("cols", geo.cols_bytes(B), keep=geo.kept_lanes(B, None, device)), B, None)

    g, _ = footprint(device, call)
    assert torch.equal(g.bufs["cols"].body, st["cols"])  # the round trip, padding included


def numpy_bag_stream(lib, device, B, n_pieces=7, L=5):
    seeds = torch.arange(1000, 1000 + B, dtype=torch.int32, device=device)

    def call(A):
        A.launch(lib.numpy_bag_stream, A.new("seeds", init=seeds, keep=True), n_pieces, L, A.new("stream", L * B), B, None)

    g, _ = footprint(device, call)
    assert int(g.bufs["stream"].body.max()) < n_pieces

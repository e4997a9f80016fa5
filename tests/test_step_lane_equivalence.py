"""The step kernel's lane logic against one plain yardstick, on the CPU.

Everything of the lane tests is here: the harness build, the input sets, the assertions and the test that pins the
yardstick.  The tests of this file run every set, the seeded ones (i) and (ii) with their first seed.  The second
seed's runs of (i) and (ii) call the same functions from `tests/test_step_lane_parent_equivalence.py`, a file of
ten lines of code that is kept for its test ids alone (it once held a second yardstick; it holds none now).

`tests/harness/lane_equivalence.cpp` compares `valid_mask` (the top-rows form `env_step` uses AND the general form
`refresh_kernel` keeps) and `board_features` (the 12-row tables and, for R <= 20, the packed 10-row form the step
kernel runs) for `<uint32_t, 10>` with a yardstick that is no earlier form of them: loops over the board's cells,
no tables, no bit-parallel words.  The mask is worked out one placement at a time (land at max_j(h - b_j), add the
cells, remove the full rows among the piece's, terminal iff a cell remains at row >= R), the six feature integers
cell by cell.  `test_yardstick_is_the_oracle` pins the yardstick itself: its masks to the `terminal` flags of
`oracle.placements`, its features to `oracle.board_features`.  The inputs:

 (i)   boards whose rows R-4 .. R-1 run through every pattern of a 6-column window (2^24 patterns), the window
       at each of its five positions, the other columns and the rows below randomised with a fixed seed (two
       seeds), no cell at or above R.  This is the set that forces the rescue by a cleared row, taken and
       skipped, for every orientation; the test asserts that every piece met rescued placements.  The same on
       eight columns (three window positions): `board_features_u32_2x10` adds the last height by hand when C is
       a multiple of four, which ten columns never run.
 (ii)  boards sampled from oracle games at steady state (random play, two fixed seeds, after 256 steps).
 (iii) the boards of tests/golden g1 (10x20) and g4 that hold no cell at or above R.
 (iv)  the directed boards of tests/directed_boards.py (stacked rows with one gap, a deep well at every column,
       checkerboard, alternate full columns, towers): the only boards here whose wells pass 255, which random
       fill and random play never reach.

Every piece of the default set and of the nine-piece catalogue; the full 48-bit mask; all six feature integers on
every board of every set; zero mismatches, no board of (i) or (ii) left out.  R = 20, and R = 10 and R = 24 (the
extremes the 10-row-chunk tables and 32-bit boards serve).

(i) runs all 2^24 patterns x 5 positions for R = 20 with the nine-piece catalogue (the default set's two pieces are
members of it and are run on every 16th pattern as a set of their own); R = 10, R = 24 and the eight-column run
take every 16th pattern (the offset inside each block of 16 is hashed, so no pattern bit is fixed).  (ii) is
2,000,000 boards at R = 20 and 250,000 each at R = 10 and R = 24, per seed.

Measured on a machine with 8 CPUs, so on 8 threads (min(16, os.cpu_count())), the build included: 440 s for the two
test files run one after the other, against 268 s for them before, on the same machine (each then with one seed and
a harness of its own, a frozen bit-parallel copy of the product as its yardstick, and in one of the two no features
on (i)).  The plain yardstick costs more than the copies did: 156 s of the 440 are the two full R = 20 window runs
(74 s before), of which the product's own functions take about 60; 40 s are the two tests that pin the yardstick;
the oracle games of (ii) take about 150 s as before.  No input was cut to make up for it.
"""
import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import directed_boards
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "lane_equivalence.cpp")
NTHREADS = min(16, os.cpu_count() or 1)
CATALOGUE9 = list(range(9))
DEFAULT = [orc.CATALOGUE.index(n) for n in orc.PIECE_SETS["default"]]
SETS = {"default": DEFAULT, "catalogue9": CATALOGUE9}
WINDOW_SEEDS = (0x7E7215, 0x5EED05)  # first, second
STEADY_SEEDS = (1234, 4321)
N_PINNED = 20000


_LIB = []  # the harness, built and loaded once for both files


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    if _LIB:
        return _LIB[0]
    so = str(tmp_path_factory.mktemp("lane_equivalence") / "liblane_equivalence.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-shared", "-o", so, SRC])
    os.environ.setdefault("OMP_NUM_THREADS", str(NTHREADS))
    lib = ctypes.CDLL(so)
    lib.lane_vm_window.restype = ctypes.c_int64
    lib.lane_vm_window.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.lane_window_cols.restype = None
    lib.lane_window_cols.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    lib.lane_boards.restype = None
    lib.lane_boards.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                ctypes.c_void_p]
    lib.lane_yardstick_masks.restype = None
    lib.lane_yardstick_masks.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.lane_yardstick_features.restype = None
    lib.lane_yardstick_features.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    _LIB.append(lib)
    return lib


def _ids(pieces):
    return np.asarray(pieces, np.int32)


def _run_boards(lib, R, pieces, cols):
    cols = np.ascontiguousarray(cols, np.uint32)
    out = np.zeros(6, np.int64)
    ids = _ids(pieces)
    lib.lane_boards(R, len(ids), ids.ctypes.data, cols.ctypes.data, cols.shape[0], out.ctypes.data)
    return dict(mask_bad=int(out[0]), feat_bad=int(out[1]), dirty=int(out[2]), masks=int(out[3]),
                waves_rescue=int(out[4]), waves=int(out[5]))


def window_patterns(lib, which, C, R, every, sets):
    """Set (i) with seed `which` (0: first, 1: second) on C columns."""
    base = WINDOW_SEEDS[which]
    for name in sets:
        ids = _ids(SETS[name])
        rescued = np.zeros(16, np.int64)
        checked = np.zeros(1, np.int64)
        feat_bad = np.zeros(1, np.int64)
        bad = lib.lane_vm_window(C, R, len(ids), ids.ctypes.data, base + R, every, rescued.ctypes.data,
                                 checked.ctypes.data, feat_bad.ctypes.data)
        print("C=%d R=%d %s every=%d seed=%#x: %d masks compared, %d mismatches, %d feature mismatches, "
              "rescued placements per piece %s"
              % (C, R, name, every, base + R, checked[0], bad, feat_bad[0], rescued[:len(ids)].tolist()))
        assert checked[0] == (1 << 24) // every * (C - 5) * len(ids)  # nothing left out
        assert bad == 0 and feat_bad[0] == 0
        assert (rescued[:len(ids)] > 0).all(), "set (i) never reached the rescue for some piece"


WINDOW_CASES = [(20, 1, ("catalogue9",)), (20, 16, ("default",)), (10, 16, ("default", "catalogue9")),
                (24, 16, ("default", "catalogue9"))]  # R, every, sets
STEADY_CASES = [(20, 2000000), (10, 250000), (24, 250000)]  # R, n_boards

_STEADY_HEAD = {}  # (R, seed) -> the first N_PINNED boards of set (ii), kept by _steady_state_cols


def _steady_state_cols(R, n_boards, seed):
    B = 50000
    env = orc.OracleVecEnv(10, R, B, pieces="standard7", auto_reset=True, seed=seed, nthreads=NTHREADS)
    env2 = orc.OracleVecEnv(10, R, B, pieces="default", auto_reset=True, seed=seed + 1, nthreads=NTHREADS)
    for _ in range(256):
        env.step()
        env2.step()
    sh = np.arange(R + 4, dtype=np.uint32)[None, :, None]
    got = []
    while sum(len(g) for g in got) < n_boards:
        for e in (env, env2):
            e.step()
            got.append((e.cells.astype(np.uint32) << sh).sum(axis=1, dtype=np.uint32))
    cols = np.concatenate(got)[:n_boards]
    _STEADY_HEAD.setdefault((R, seed), cols[:N_PINNED].copy())
    return cols


def _steady_head(R, seed):
    """The first N_PINNED boards of set (ii): kept from the full run where there was one (256 warm-up steps of
    100,000 games are most of its cost), generated here otherwise.  The boards are the same either way."""
    if (R, seed) not in _STEADY_HEAD:
        _steady_state_cols(R, N_PINNED, seed)
    return _STEADY_HEAD[(R, seed)]


def steady_state_boards(lane, which, R, n_boards):
    """Set (ii) with seed `which`."""
    base = STEADY_SEEDS[which]
    cols = _steady_state_cols(R, n_boards, seed=base + R)
    assert cols.shape == (n_boards, 10)
    for name, pieces in SETS.items():
        r = _run_boards(lane, R, pieces, cols)
        print("R=%d %s seed=%d: %s" % (R, name, base + R, r))
        assert r["dirty"] == 0  # cap on skipped boards: 0
        assert r["masks"] == n_boards * len(pieces)
        assert r["mask_bad"] == 0 and r["feat_bad"] == 0


def golden_clean_cols():
    gdir = os.path.join(HERE, "golden")
    g1 = np.load(os.path.join(gdir, "g1_placements_10x20.npz"))
    g4 = np.load(os.path.join(gdir, "g4_edges.npz"))
    boards = [g1["boards"]] + [g4[k][None, :] for k in g4.files if k.endswith("_board")]
    cols = np.concatenate(boards).astype(np.uint64)
    return cols[(cols >> np.uint64(20)).max(axis=1) == 0].astype(np.uint32), len(cols)


def golden_boards(lane):
    clean, n_all = golden_clean_cols()
    assert len(clean) > 0
    for name, pieces in SETS.items():
        r = _run_boards(lane, 20, pieces, clean)
        print("golden %s: %d of %d boards clean, %s" % (name, len(clean), n_all, r))
        assert r["dirty"] == 0 and r["masks"] == len(clean) * len(pieces)
        assert r["mask_bad"] == 0 and r["feat_bad"] == 0


def _directed_cols(R):
    boards = directed_boards.structured(R, 10, seed=R)
    directed_boards.check_boards(boards, R)
    return orc.cells_to_cols(boards).astype(np.uint32)


def directed(lane, R):
    cols = _directed_cols(R)
    for name, pieces in SETS.items():
        r = _run_boards(lane, R, pieces, cols)
        print("directed R=%d %s: %d boards, %s" % (R, name, len(cols), r))
        assert r["dirty"] == 0 and r["masks"] == len(cols) * len(pieces)
        assert r["mask_bad"] == 0 and r["feat_bad"] == 0


def _placement_bits(desc, name):
    """Mask bit of every placement of a piece, in the oracle's order.

    The oracle lists placements loop by loop, column by column, the orientations of a loop side by side
    (tetris_oracle.c: orc_enumerate), so the orientation field k = 2L + o of a placement follows from the anchor
    columns alone: the column falls back to 0 where the next loop starts, and repeats inside a loop once per
    orientation."""
    p = orc.placements(desc, np.zeros((desc.num_rows + 4, 10), np.int8), name)
    loop, o, prev, bits = 0, 0, -1, []
    for c in p["anchor_col"].tolist():
        loop += c < prev
        o = o + 1 if c == prev else 0
        bits.append(12 * (2 * loop + o) + c)
        prev = c
    assert len(bits) == orc.n_placements(name, 10) and len(set(bits)) == len(bits)
    return np.uint64(1) << np.asarray(bits, np.uint64)


def _oracle_masks(desc, cells, bits):
    """[board, piece] valid masks from the `terminal` flags of the oracle's placements.  This is the call
    oracle.placements makes (orc_placements_flat), 1.3 million times, so its output arrays are allocated once per
    chunk of boards and the flags of every call are kept side by side and turned into masks at the end."""
    rows, n_max, n_pieces = desc.num_rows + 4, 64, len(bits)
    out = [np.zeros(shape, dt) for shape, dt in (((n_max, rows, 10), np.int8), ((n_max, 10), np.int32),
                                                 ((n_max,), np.int32), ((n_max,), np.int32), ((n_max,), np.int32),
                                                 ((n_max,), np.int32), ((n_max, 8), np.float32))]
    args = [a.ctypes.data_as(ctypes.c_void_p) for a in out]
    terminal = np.ones((len(cells), n_pieces, n_max), np.int32)
    fn, pdesc = orc.lib().orc_placements_flat, ctypes.byref(desc)
    for i in range(len(cells)):
        pcells = ctypes.c_void_p(cells.ctypes.data + i * cells.strides[0])
        for pid in range(n_pieces):
            args[3] = ctypes.c_void_p(terminal.ctypes.data + (i * n_pieces + pid) * n_max * 4)
            assert fn(pdesc, pcells, pid, *args) == len(bits[pid])
    masks = np.zeros((len(cells), n_pieces), np.uint64)
    for pid in range(n_pieces):
        alive = terminal[:, pid, :len(bits[pid])] == 0
        masks[:, pid] = (alive * bits[pid]).sum(axis=1, dtype=np.uint64)
    return masks


def yardstick_is_the_oracle(lane, which):
    """The harness's yardstick against the oracle, whole-set equality of the masks of all nine pieces and of the
    six feature integers: 20,000 window boards of (i) at R = 20 (every 4194th pattern, hashed as in the full run,
    x 5 positions) and the first 20,000 boards of (ii) at each R, both with seed `which`; with the first seed also
    every clean golden board and every directed board."""
    every = 4194
    window = np.zeros(((1 << 24) // every * 5, 10), np.uint32)
    lane.lane_window_cols(20, WINDOW_SEEDS[which] + 20, every, window.ctypes.data)
    assert len(window) == N_PINNED and (window >> 20).max() == 0
    inputs = [("window", 20, window)]
    if which == 0:
        inputs += [("golden", 20, golden_clean_cols()[0])] + [("directed", R, _directed_cols(R)) for R in (20, 10, 24)]
    for R in (20, 10, 24):
        seed = STEADY_SEEDS[which] + R
        head = _steady_head(R, seed)
        assert len(head) == N_PINNED and (head >> R).max() == 0
        inputs.append(("steady seed=%d" % seed, R, head))
    with ThreadPoolExecutor(NTHREADS) as pool:  # the oracle's calls run outside the interpreter lock
        for what, R, cols in inputs:
            cols = np.ascontiguousarray(cols, np.uint32)
            cells = np.ascontiguousarray(orc.cols_to_cells(cols, R + 4))
            desc = orc.make_desc(10, R, orc.CATALOGUE)
            bits = [_placement_bits(desc, name) for name in orc.CATALOGUE]
            chunks = np.array_split(np.arange(len(cols)), 4 * NTHREADS)
            want = np.concatenate(list(pool.map(
                lambda ix: _oracle_masks(desc, np.ascontiguousarray(cells[ix]), bits), chunks)))
            for pid, name in enumerate(orc.CATALOGUE):
                got = np.zeros(len(cols), np.uint64)
                lane.lane_yardstick_masks(R, pid, cols.ctypes.data, len(cols), got.ctypes.data)
                bad = int((got != want[:, pid]).sum())
                assert bad == 0, "%s R=%d %s: %d of %d masks differ from the oracle's" % (what, R, name, bad, len(cols))
            want_f = np.stack([orc.board_features(desc, c)[[0, 1, 2, 4, 5, 7]] for c in cells])
            got_f = np.zeros((len(cols), 6), np.int32)
            lane.lane_yardstick_features(R, cols.ctypes.data, len(cols), got_f.ctypes.data)
            bad = int((got_f != want_f).any(axis=1).sum())
            assert bad == 0, "%s R=%d: features of %d of %d boards differ from the oracle's" % (what, R, bad, len(cols))
            print("%s R=%d: %d boards, yardstick == oracle on the masks of %d pieces and on the features"
                  % (what, R, len(cols), len(orc.CATALOGUE)))


# ---- the tests of this file: every input set, (i) and (ii) with their first seed ----

@pytest.mark.parametrize("R,every,sets", WINDOW_CASES)
def test_valid_mask_window_patterns(lane, R, every, sets):
    window_patterns(lane, 0, 10, R, every, sets)


def test_window_patterns_eight_columns(lane):
    window_patterns(lane, 0, 8, 20, 16, ("default", "catalogue9"))


@pytest.mark.parametrize("R,n_boards", STEADY_CASES)
def test_steady_state_boards(lane, R, n_boards):
    steady_state_boards(lane, 0, R, n_boards)


def test_golden_boards(lane):
    golden_boards(lane)


@pytest.mark.parametrize("R", [20, 10, 24])
def test_directed_boards(lane, R):
    directed(lane, R)


def test_yardstick_is_the_oracle(lane):
    yardstick_is_the_oracle(lane, 0)

"""Hand-built boards for the directed step-kernel cases (parity_cases.step_directed_boards and
step_many_directed_boards).  Boards are int8 [n, R+4, C], row 0 = bottom; none has a cell at
row >= R or a full row.  NumPy only: no GPU, no oracle."""
import numpy as np

N_CATALOGUE = 9  # pieces of tetris_amd.tetromino.CATALOGUE


def near_top(n, R, C, seed):
    """Random stacks five rows or fewer below the top whose rows R-4..R-1 get 1-3 nearly full rows
    (a missing run of width 1..4): placements that poke above row R-1 are valid there only if their
    own line clear pulls the stack back."""
    rng = np.random.default_rng(seed)
    rows = R + 4
    cells = np.zeros((n, rows, C), np.int8)
    for b in range(n):
        hts = rng.integers(max(R - 5, 0), R + 1, size=C)
        for c in range(C):
            hc = int(hts[c])
            colv = (rng.random(hc) > 0.15).astype(np.int8)
            if hc:
                colv[hc - 1] = 1
            cells[b, :hc, c] = colv
        # make 1-3 of the top rows nearly full: missing run of width 1..4 (narrower on boards under five columns)
        for r in rng.choice(np.arange(max(R - 4, 0), R), size=rng.integers(1, 4), replace=False):
            w = int(rng.integers(1, min(4, C - 1) + 1))
            c0 = int(rng.integers(0, C - w + 1))
            cells[b, r, :] = 1
            cells[b, r, c0:c0 + w] = 0
            # columns in the gap must not have cells above the gap row (heights stay consistent)
            cells[b, r:, c0:c0 + w] = 0
        for r in range(rows):  # no full rows in a reachable board
            if cells[b, r].sum() == C:
                cells[b, r, rng.integers(0, C)] = 0
        # cells above a removed cell may now float: that is fine for the reference semantics
        # as long as heights are recomputed from the board (State(lowest_free_rows=None))
        cells[b, R:, :] = 0
    return cells


def _structured(R, C, seed):
    """(family name, board) pairs; see structured()."""
    rng = np.random.default_rng(seed)
    rows = R + 4

    def blank():
        return np.zeros((rows, C), np.int8)

    yield "empty", blank()
    # k stacked rows, full except one common column g, on random 70 % rubble that keeps g empty: Straight
    # clears k lines there, the other pieces fewer; at the top bases a piece that pokes above R-1 is
    # pulled back by its own clear
    for k in (1, 2, 3, 4):
        for base in sorted({0, R // 2 - 2, R - 4 - k, R - k}):
            if base < 0 or base + k > R:
                continue
            for g in (0, C // 2, C - 1):
                b = blank()
                below = (rng.random((base, C)) < 0.7).astype(np.int8)
                below[:, g] = 0
                b[:base] = below
                b[base:base + k, :] = 1
                b[base:base + k, g] = 0
                yield "gap_rows k=%d base=%d g=%d" % (k, base, g), b
    for g in range(C):  # deep well: every column but g full to height h
        for h in (R, R - 1, R // 2):
            b = blank()
            b[:h, :] = 1
            b[:h, g] = 0
            yield "well g=%d h=%d" % (g, h), b
    b = blank()
    b[0:R:2, 0::2] = 1
    b[1:R:2, 1::2] = 1
    yield "checkerboard", b
    b = blank()
    b[:R, 0::2] = 1
    yield "alternate_columns", b
    for c in (0, C - 1):
        b = blank()
        b[:R, c] = 1
        yield "tower c=%d" % c, b


def structured(R, C, seed):
    """The empty board; k = 1..4 stacked rows missing one common column at the bottom, the middle and the
    top; a deep well at every column; a checkerboard to row R-1; alternate columns full to R; one tower
    of height R at either edge."""
    return np.stack([b for _, b in _structured(R, C, seed)])


def structured_names(R, C):
    """Family name of every board of structured(R, C, .), for failure messages."""
    return [name for name, _ in _structured(R, C, 0)]


def check_boards(boards, R):
    """The module's promise: no cell at row >= R, no full row."""
    assert not boards[:, R:, :].any()
    assert not (boards.sum(axis=2) == boards.shape[2]).any()


def expand(boards, n_valid):
    """Flat case list (board_ix, piece, action): every action k < n_valid[piece][board] of every catalogue
    piece on every board, one env per case."""
    n_valid = np.asarray(n_valid)
    assert n_valid.shape == (N_CATALOGUE, len(boards))
    bix, piece, action = [], [], []
    for pi in range(N_CATALOGUE):
        for b in range(len(boards)):
            k = int(n_valid[pi][b])
            bix.append(np.full(k, b, np.int64))
            piece.append(np.full(k, pi, np.int64))
            action.append(np.arange(k, dtype=np.int32))
    return np.concatenate(bix), np.concatenate(piece), np.concatenate(action)

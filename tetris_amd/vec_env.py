"""VecTetris: a batch of placement-level Tetris envs resident in HBM.

The batched counterpart of the reference's ``game.Tetris`` (game.py:8-100):
``reset() / get_after_states() / step(actions)`` for B envs in lockstep.  All
state lives in PyTorch-ROCm tensors; every method enqueues one HIP kernel of
``libtetris_hip.so`` on the current stream through the C-ABI
(include/tetris_hip.h).  PyTorch is plumbing (memory + streams) only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .tetromino import CATALOGUE, Tetromino, resolve_pieces


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class VecTetris:
    """B independent envs with the semantics of game.Tetris.

    Parameters mirror ``Tetris(num_columns, num_rows, feature_directions=None)``
    (game.py:21-23) plus the batch knobs:

    batch_size   number of envs
    device       a CUDA (ROCm) device
    pieces       'default' (game.py:38-39), 'standard7' (game.py:41-47) or names
    auto_reset   reset finished envs inside the step kernel (game.py:53-63)
    seed         seed of the counter-based device bag
    piece_stream optional uint8 [L, B]: replay these list indices instead of the
                 device bag (parity runs against a recorded NumPy stream)
    numpy_seeds  optional [B] ints: env i draws the pieces of a reference game seeded with
                 ``np.random.seed(numpy_seeds[i])`` -- the reference's sampler on NumPy's MT19937
                 stream, generated on the device (``stream_len`` draws per env, replay mode)
    env_offset   global index of env 0 (shards of one logical batch draw the
                 same pieces as the unsharded batch)
    compute_obs  False: step() skips the BCTS observation (obs stays zero); for agents that
                 already hold get_after_states() features, whose row `action` is that observation
    afterstate_layout  storage of the get_after_states matrices: "env_major" (contiguous
                 [B, a_max, 8], default, fastest on MI355X) or "action_major"
                 ([a_max, B, 8] storage returned as a [B, a_max, 8] view)


    ``step`` returns views of buffers that the next ``step`` overwrites.
    """

    def __init__(self, num_columns, num_rows, batch_size, device="cuda", pieces="default", auto_reset=False,
                 seed=0, feature_directions=None, piece_stream=None, env_offset=0, afterstate_layout="env_major",
                 compute_obs=True, numpy_seeds=None, stream_len=4096):
        self._lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != self._lib.device_type:
            raise ValueError("VecTetris needs a %s device (got %s): the env only exists as HIP kernels"
                             % (self._lib.device_type, self.device))
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_columns, self.num_rows, self.batch_size = int(num_columns), int(num_rows), int(batch_size)
        self.piece_names = resolve_pieces(pieces)
        self.tetrominos = [Tetromino(n, i, self.num_columns) for i, n in enumerate(self.piece_names)]
        self._generation = 0  # bumped whenever something a bound step call / captured graph froze changes
        self._step_call = None
        self._auto_reset = bool(auto_reset)
        self._seed = int(seed)
        self._env_offset = int(env_offset)
        self.feature_directions = feature_directions
        if afterstate_layout not in ("action_major", "env_major"):
            raise ValueError("afterstate_layout must be 'action_major' or 'env_major'")
        self.afterstate_layout = afterstate_layout
        self._compute_obs = bool(compute_obs)
        self.loss_reward, self.timestep_reward = -100, -1  # game.py:34-35 (baked into the kernel)

        ids = (ctypes.c_int32 * len(self.piece_names))(*[CATALOGUE.index(n) for n in self.piece_names])
        dirs = None
        if feature_directions is not None:
            fd = np.asarray(feature_directions, dtype=np.float32)
            if fd.shape != (8,):
                raise ValueError("feature_directions must have 8 entries")
            dirs = (ctypes.c_float * 8)(*fd.tolist())
        self.desc = _lib.TetrisDesc()
        self._lib.check(self._lib.desc_init(ctypes.byref(self.desc), self.num_columns, self.num_rows, ids,
                                            len(self.piece_names), dirs), "tetris_hip_desc_init")
        if self.batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.a_max = int(self.desc.a_max)
        self.stored_rows = self.num_rows + 4
        self.word_dtype = torch.int32 if self.desc.word_bytes == 4 else torch.int64

        B, dev = self.batch_size, self.device
        with torch.device(dev):
            # tile-major column bitboards [ceil(B/64), n_planes, 64], opaque: one plane per column, or
            # bit-packed four columns to three words when the stored rows fit three quarters of the word
            # (tetris_hip_n_planes / tetris_hip_board_words)
            self.n_planes = int(self._lib.n_planes(ctypes.byref(self.desc)))
            if self.n_planes <= 0:
                self._lib.check(self.n_planes, "tetris_hip_n_planes")
            self.n_tiles = (B + 63) // 64
            assert int(self._lib.board_words(ctypes.byref(self.desc), B)) == self.n_tiles * self.n_planes * 64
            self.cols = torch.zeros((self.n_tiles, self.n_planes, 64), dtype=self.word_dtype)
            self.meta = torch.zeros(B, dtype=torch.int64)
            self._obs_buf = torch.zeros((B, 8), dtype=torch.float32)
            self._reward_buf = torch.zeros(B, dtype=torch.int32)
            self._done_buf = torch.zeros(B, dtype=torch.uint8)
            self._lines_buf = torch.zeros(B, dtype=torch.uint8)
            self.n_valid = torch.zeros(B, dtype=torch.uint8)
            self.piece = torch.zeros(B, dtype=torch.uint8)
            self.status = torch.zeros(int(self._lib.status_words(B)), dtype=torch.int32)  # [n_waves, 4]
            self._action_buf = torch.zeros(B, dtype=torch.int32)  # actions drawn by the built-in policy
        self._own_views()
        self._stream = None
        self._cursor = None
        if numpy_seeds is not None:
            if piece_stream is not None:
                raise ValueError("give either piece_stream or numpy_seeds")
            piece_stream = self.numpy_piece_stream(numpy_seeds, len(self.piece_names), stream_len, dev)
        if piece_stream is not None:
            ps = torch.as_tensor(piece_stream, dtype=torch.uint8)
            if ps.dim() != 2 or ps.shape[1] != B:
                raise ValueError("piece_stream must be [L, batch_size]")
            self._stream = ps.to(dev).contiguous()
            self._cursor = torch.zeros(B, dtype=torch.int32, device=dev)
        self._feats = None
        self._feats_all = None
        self._n_all = None
        self.step_idx = 0
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) if self.device.type == "cuda" else None
        self.reset(init_bag=True)

    MAX_REPLAY_STREAM_BYTES = 1 << 30  # one byte per (draw, env)

    @staticmethod
    def numpy_piece_stream(seeds, n_pieces, length, device="cuda"):
        """uint8 [length, B]: column i = what the reference's ``TetrominoSampler`` (tetromino.py:12-22)
        returns call after call in a process seeded ``np.random.seed(seeds[i])``, computed on the device
        (``tetris_hip_numpy_bag_stream``: MT19937 + NumPy's legacy permutation)."""
        lib = _lib.load()
        device = torch.device(device)
        n_bytes = int(length) * int(np.asarray(seeds).size)
        if n_bytes > VecTetris.MAX_REPLAY_STREAM_BYTES:
            raise ValueError("a replay stream of %d draws x %d envs is %.1f GiB (limit %.1f GiB): NumPy-exact replay "
                             "is a set-up mode for moderate batches -- pass a shorter stream_len, or use the "
                             "counter-based device bag (no numpy_seeds) for large batches"
                             % (int(length), int(np.asarray(seeds).size), n_bytes / 2.0**30,
                                VecTetris.MAX_REPLAY_STREAM_BYTES / 2.0**30))
        seeds32 = torch.from_numpy(np.asarray(seeds, dtype=np.uint32).view(np.int32).copy()).to(device)
        out = torch.empty((int(length), seeds32.numel()), dtype=torch.uint8, device=device)
        stream = None
        if device.type == "cuda":
            stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        lib.check(lib.numpy_bag_stream(_ptr(seeds32), int(n_pieces), int(length), _ptr(out), seeds32.numel(), stream),
                  "tetris_hip_numpy_bag_stream")
        return out

    # seed / auto_reset / compute_obs / env_offset are baked into the bound step call (and into every HIP
    # graph captured from it): assigning one drops the bound call, so that step(), step_many(), reset() and
    # random_actions() keep agreeing, and invalidates captured graphs (StepGraph.replay raises).
    def _frozen(name):  # noqa: N805
        def get(self):
            return getattr(self, "_" + name)

        def set_(self, value):
            setattr(self, "_" + name, type(getattr(self, "_" + name))(value))
            self._invalidate_bound_call()
        return property(get, set_)

    seed = _frozen("seed")
    auto_reset = _frozen("auto_reset")
    compute_obs = _frozen("compute_obs")
    env_offset = _frozen("env_offset")
    del _frozen

    def _invalidate_bound_call(self):
        self._step_call = None
        self._generation += 1

    # -- plumbing -----------------------------------------------------------------
    def _own_views(self):
        """Point the per-step attributes (obs, reward, done, lines, action) at this env's own buffers;
        after step_many they are views of the last row of its trajectory buffers instead."""
        self.obs, self.reward, self._done, self.lines = self._obs_buf, self._reward_buf, self._done_buf, self._lines_buf
        self.action = self._action_buf
        self.done = self._done.view(torch.bool)
        self._views_own = True

    def _hip_stream(self):
        if self.device.type == "cuda":
            return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    def _stream_args(self):
        if self._stream is None:
            return None, None, 0
        return _ptr(self._stream), _ptr(self._cursor), int(self._stream.shape[0])

    # -- Tetris.reset (game.py:53-63) -----------------------------------------------
    def reset(self, mask=None, init_bag=False):
        """Reset every env (or those where ``mask`` is true).  The bag is kept
        unless ``init_bag`` (the reference bag survives reset: game.py:50)."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            if m.shape != (self.batch_size,):
                raise ValueError("mask must be [batch_size]")
        s, c, n = self._stream_args()
        rc = self._lib.reset(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), _ptr(m), _ptr(self.piece),
                             _ptr(self.n_valid), s, c, n, _ptr(self.status), int(bool(init_bag)), self.seed,
                             self.step_idx, self.env_offset, self.batch_size, self._hip_stream())
        self._lib.check(rc, "tetris_hip_reset")

    # -- Tetris.get_after_states (game.py:67-80) --------------------------------------
    def get_after_states(self, include_terminal=False):
        """BCTS features of every placement of the current piece.

        Returns ``(features [B, a_max, 8] float32, n_valid [B] uint8)``; row k of
        env i is its k-th non-terminal placement (= action k), rows >= n_valid
        are zero.  With ``include_terminal`` also ``(features_all, n_all)`` in
        raw enumeration order (game.py:74-78)."""
        B, A = self.batch_size, self.a_max
        am = self.afterstate_layout == "action_major"
        shape = (A, B, 8) if am else (B, A, 8)
        env_stride, row_stride = (8, B * 8) if am else (A * 8, 8)
        if self._feats is None:
            self._feats = torch.empty(shape, dtype=torch.float32, device=self.device)
            self._nv_after = torch.empty(B, dtype=torch.uint8, device=self.device)
        fa = na = None
        if include_terminal:
            if self._feats_all is None:
                self._feats_all = torch.empty(shape, dtype=torch.float32, device=self.device)
                self._n_all = torch.empty(B, dtype=torch.uint8, device=self.device)
            fa, na = self._feats_all, self._n_all
        rc = self._lib.afterstates(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), _ptr(self._feats),
                                   _ptr(self._nv_after), _ptr(fa), _ptr(na), env_stride, row_stride, B,
                                   self._hip_stream())
        self._lib.check(rc, "tetris_hip_afterstates")
        view = (lambda t: t.permute(1, 0, 2)) if am else (lambda t: t)
        if include_terminal:
            return view(self._feats), self._nv_after, view(fa), na
        return view(self._feats), self._nv_after

    # -- Tetris.step (game.py:82-92) ------------------------------------------------------
    def gather_payload(self):
        """Buffers for one done/reset gather (``step(..., gather=payload)``): ``done_bits`` uint8
        [8 * ceil(B / 64)] -- the done bitmask, bit i % 8 of byte i // 8 -- and ``counters`` int32
        [n_waves, 4] -- the per-wave (invalid, episodes, lines, steps) slots as of that step.  The step
        kernel writes both from its epilogue; nothing else touches them, so a collective can read them
        on another stream (``tetris_hip_stream_link``) while the env keeps stepping."""
        return dict(done_bits=torch.zeros(((self.batch_size + 63) // 64) * 8, dtype=torch.uint8, device=self.device),
                    counters=torch.zeros_like(self.status).view(-1, 4))

    def step(self, action=None, gather=None):
        """``action`` [B] = index into each env's non-terminal placements; ``None`` = every env
        plays a uniform random valid action drawn inside the kernel (readable afterwards in
        ``self.action``; identical to ``step(random_actions())``).  ``gather``: a
        :meth:`gather_payload` this step fills in (done bitmask + counter snapshot).

        Returns ``(obs [B,8] f32, reward [B] i32, done [B] bool, lines [B] u8)``.
        Out-of-range actions leave that env untouched and are counted; call
        :meth:`check` to turn them into the reference's IndexError."""
        if not self._views_own:
            self._own_views()
        a = None
        if action is not None:
            a = torch.as_tensor(action, device=self.device)
            if a.shape != (self.batch_size,):
                raise ValueError("action must be [batch_size]")
            if a.dtype != torch.int32 or not a.is_contiguous():
                a = a.to(torch.int32).contiguous()
        # bound call (tetris_hip_step_call_*): pointers, geometry and the placement table are prepared once
        call = self._step_call
        if call is None:
            call = self._bind_step_call()
        if self._raw_stream is not None:
            stream = self._raw_stream(self.device.index)
        else:
            stream = self._hip_stream()
        if gather is None:
            rc = self._lib.step_call_run(call, None if a is None else a.data_ptr(), self.step_idx, stream)
        else:
            rc = self._lib.step_call_run_gather(call, None if a is None else a.data_ptr(), self.step_idx,
                                                gather["done_bits"].data_ptr(), gather["counters"].data_ptr(), stream)
        if rc:
            self._lib.check(rc, "tetris_hip_step_call_run")
        self.step_idx += 1
        return self.obs, self.reward, self.done, self.lines

    # -- HIP graph of K steps -------------------------------------------------------------------
    def capture_steps(self, n_steps, action_fn=None):
        """Capture ``n_steps`` consecutive steps in ONE HIP graph and return it (``StepGraph``); each
        ``replay()`` then advances the env by ``n_steps`` steps with a single graph launch.  For small
        batches, where one step kernel (5-8 us) is about as long as its host enqueue, this takes the
        host off the critical path.  ``action_fn(env, k)`` (optional) is called at capture time before
        step k and must enqueue, on the current stream, whatever produces the ``[B]`` int32 action
        tensor it returns (it is captured too); without it every env plays the built-in uniform
        random policy.  The step index lives in device memory (``tetris_hip_step_call_run_counted``), so
        replays are bit-identical to the same number of ``step()`` calls."""
        return StepGraph(self, int(n_steps), action_fn)

    def _bind_step_call(self):
        size = int(self._lib.step_call_size())
        buf = ctypes.create_string_buffer(size + 16)
        addr = (ctypes.addressof(buf) + 15) & ~15
        s, c, n = self._stream_args()
        rc = self._lib.step_call_init(addr, ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta),
                                      _ptr(self._action_buf), s, c, n,
                                      _ptr(self._obs_buf) if self.compute_obs else None, _ptr(self._reward_buf),
                                      _ptr(self._done_buf), _ptr(self._lines_buf), _ptr(self.n_valid), _ptr(self.piece),
                                      _ptr(self.status), int(self.auto_reset), self.seed, self.env_offset,
                                      self.batch_size)
        self._lib.check(rc, "tetris_hip_step_call_init")
        self._step_call_buf = buf  # keeps the memory alive
        self._step_call = addr
        return addr

    def step_many(self, n_steps, policy="random", weights=None, out=None):
        """``n_steps`` consecutive steps in ONE kernel launch with an in-kernel policy ("random":
        uniform valid action; "greedy": linear fitness on ``weights``): boards stay in registers
        between steps, every step's outputs are written.  Returns a dict of trajectory tensors
        ``obs [K,B,8] f32, reward [K,B] i32, done [K,B] bool, lines [K,B] u8, action [K,B] i32,
        n_valid [K,B] u8, piece [K,B] u8``; with policy "random" it is bit-identical to
        ``n_steps`` calls of ``step()``.  Pass the previous result as ``out`` to reuse buffers."""
        K, B, dev = int(n_steps), self.batch_size, self.device
        pol = {"random": 0, "greedy": 1}[policy]
        if self._stream is not None:
            raise ValueError("step_many draws pieces from the device bag (no replay stream)")
        if out is None or out["reward"].shape[0] != K:
            out = dict(obs=torch.zeros((K, B, 8), dtype=torch.float32, device=dev),
                       reward=torch.empty((K, B), dtype=torch.int32, device=dev),
                       _done=torch.empty((K, B), dtype=torch.uint8, device=dev),
                       lines=torch.empty((K, B), dtype=torch.uint8, device=dev),
                       action=torch.empty((K, B), dtype=torch.int32, device=dev),
                       n_valid=torch.empty((K, B), dtype=torch.uint8, device=dev),
                       piece=torch.empty((K, B), dtype=torch.uint8, device=dev))
            out["done"] = out["_done"].view(torch.bool)
        w = (ctypes.c_float * 8)(*(self.BCTS_WEIGHTS if weights is None else [float(x) for x in weights]))
        rc = self._lib.step_many(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), K, pol, w,
                                 _ptr(out["action"]), _ptr(out["obs"]) if self.compute_obs else None,
                                 _ptr(out["reward"]), _ptr(out["_done"]), _ptr(out["lines"]), _ptr(out["n_valid"]),
                                 _ptr(out["piece"]), _ptr(self.status), int(self.auto_reset), self.seed,
                                 self.step_idx, self.env_offset, B, self._hip_stream())
        self._lib.check(rc, "tetris_hip_step_many")
        self.step_idx += K
        # the per-step attributes keep describing the latest step: n_valid / piece (inputs of the next
        # reset / random_actions) are copied, the outputs become views of the last trajectory row
        self.n_valid.copy_(out["n_valid"][K - 1])
        self.piece.copy_(out["piece"][K - 1])
        if self.compute_obs:
            self.obs = out["obs"][K - 1]
        self.reward, self._done, self.lines = out["reward"][K - 1], out["_done"][K - 1], out["lines"][K - 1]
        self.action = out["action"][K - 1]
        self.done = self._done.view(torch.bool)
        self._views_own = False
        return out

    BCTS_WEIGHTS = (-24.04, -19.77, -13.08, -12.63, -10.49, -9.22, 6.6, -1.61)  # game.py:111-118

    def _population(self, weights, rows, what):
        """(weights float32 [P, 8] contiguous on the device, rows int32 [B] or None) for the per-env-row calls"""
        if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or weights.shape[1] != 8:
            raise ValueError("%s: weights must be a [P, 8] tensor" % what)
        if weights.device != self.device:
            raise ValueError("%s: weights live on %s, this env on %s" % (what, weights.device, self.device))
        if weights.dtype != torch.float32 or not weights.is_contiguous():
            weights = weights.to(torch.float32).contiguous()
        if weights.shape[0] < 1 or weights.data_ptr() % 16:
            raise ValueError("%s: weights need at least one row and 16-byte alignment" % what)
        if rows is None:
            if weights.shape[0] < self.batch_size:
                raise ValueError("%s: without rows env i uses row i: weights must have at least batch_size = %d rows "
                                 "(got %d)" % (what, self.batch_size, weights.shape[0]))
            return weights, None
        return weights, self._gather_index(rows, what)

    def greedy_actions(self, weights=None, include_fitness=False, rows=None):
        """Tetris.get_best_policy / fitness (game.py:102-120) for every env, without materialising
        the feature matrix: returns ``(best_action int32 [B], best_value float32 [B])`` -- the first
        non-terminal action of maximal linear fitness (-1 when the env has none) -- and with
        ``include_fitness`` also ``fitness_all float32 [B, a_max]`` over ALL placements in raw order
        (terminal included, the domain of the reference's policy vector).

        A population: ``weights`` as a 2-D tensor ``[P, 8]`` on the env's device and ``rows`` ``[B]`` ints (or
        ``None``: env i uses row i) evaluates every env with ITS row (``tetris_hip_policy_greedy_rows``; no
        ``include_fitness``).  A row outside ``[0, P)`` leaves that env's entries as they were and is counted,
        see :meth:`check`."""
        if isinstance(weights, torch.Tensor) and weights.dim() == 2:
            if include_fitness:
                raise ValueError("greedy_actions: include_fitness is not available with per-env weight rows")
            wt, idx = self._population(weights, rows, "greedy_actions")
            B = self.batch_size
            if not hasattr(self, "_best_action"):
                self._best_action = torch.empty(B, dtype=torch.int32, device=self.device)
                self._best_value = torch.empty(B, dtype=torch.float32, device=self.device)
                self._fitness_all = None
            rc = self._lib.policy_greedy_rows(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), _ptr(wt),
                                              wt.shape[0], _ptr(idx), _ptr(self._best_action), _ptr(self._best_value),
                                              _ptr(self.status), B, self._hip_stream())
            self._lib.check(rc, "tetris_hip_policy_greedy_rows")
            return self._best_action, self._best_value
        if rows is not None:
            raise ValueError("greedy_actions: rows needs weights as a [P, 8] tensor")
        w = (ctypes.c_float * 8)(*(self.BCTS_WEIGHTS if weights is None else [float(x) for x in weights]))
        B = self.batch_size
        if not hasattr(self, "_best_action"):
            self._best_action = torch.empty(B, dtype=torch.int32, device=self.device)
            self._best_value = torch.empty(B, dtype=torch.float32, device=self.device)
            self._fitness_all = None
        fa = None
        if include_fitness:
            if self._fitness_all is None:
                self._fitness_all = torch.empty((B, self.a_max), dtype=torch.float32, device=self.device)
            fa = self._fitness_all
        rc = self._lib.policy_greedy(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), w,
                                     _ptr(self._best_action), _ptr(self._best_value), _ptr(fa), B,
                                     self._hip_stream())
        self._lib.check(rc, "tetris_hip_policy_greedy")
        if include_fitness:
            return self._best_action, self._best_value, fa
        return self._best_action, self._best_value

    def play(self, weights, rows=None, max_steps=1 << 20, chunk=64):
        """Greedy play of a population of linear policies: env i plays the greedy policy on row ``rows[i]`` of
        ``weights`` (a ``[P, 8]`` tensor on the env's device; ``rows=None``: env i uses row i) until its game is
        over or ``max_steps`` steps have been played -- the evaluation half of a cross-entropy / CMA-style search
        over the weights, :meth:`gather_` / :meth:`fork` being the selection half.

        The steps run in launches of ``chunk`` steps (``tetris_hip_play_linear``: boards in registers, nothing
        but per-env totals written); after each launch one ``n_valid.any()`` read-back -- the only
        synchronisation -- decides whether to launch again.  Returns ``dict(lines uint32 [B], pieces uint32 [B],
        done bool [B])``: lines cleared and pieces placed by each env in THIS call (the losing placement
        included), and whether its game is over.

        ``play`` never resets an env, whatever ``auto_reset`` says: a finished env stays as it ended (reset it
        with :meth:`reset` or refill it with :meth:`copy_envs_from`).  An env that is already over is left
        alone.  ``step_idx`` advances by the steps launched and ``n_valid`` / ``piece`` describe the boards
        afterwards, so ``step()`` continues the surviving envs; like ``step_many`` it leaves earlier
        ``get_after_states()`` results describing the boards as they were.  A row outside ``[0, P)`` leaves its
        env untouched and is counted once per launch, see :meth:`check`.  Replay mode is refused."""
        if self._stream is not None:
            raise ValueError("play draws pieces from the device bag (no replay stream)")
        max_steps, chunk = int(max_steps), int(chunk)
        if max_steps < 0 or chunk < 1:
            raise ValueError("play: max_steps must be >= 0 and chunk >= 1")
        wt, idx = self._population(weights, rows, "play")
        B, dev = self.batch_size, self.device
        lines = torch.zeros(B, dtype=torch.int32, device=dev)
        pieces = torch.zeros(B, dtype=torch.int32, device=dev)
        played = 0
        while played < max_steps:
            k = min(chunk, max_steps - played)
            rc = self._lib.play_linear(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), k, _ptr(wt),
                                       wt.shape[0], _ptr(idx), _ptr(lines), _ptr(pieces), _ptr(self.n_valid),
                                       _ptr(self.piece), _ptr(self.status), self.seed, self.step_idx,
                                       self.env_offset, B, self._hip_stream())
            self._lib.check(rc, "tetris_hip_play_linear")
            self.step_idx += k
            played += k
            if not bool(self.n_valid.any()):
                break
        return dict(lines=lines.view(torch.uint32), pieces=pieces.view(torch.uint32), done=self.n_valid == 0)

    def _softmax_population(self, weights, rows, temperature, what):
        """(weights [P, 8], rows or None, temperature) for the softmax calls: a shared vector ``[8]`` becomes P = 1
        with a cached all-zero row list"""
        if isinstance(weights, torch.Tensor) and weights.dim() == 1:
            if weights.shape[0] != 8 or rows is not None:
                raise ValueError("%s: a shared weight vector has 8 entries and takes no rows" % what)
            if not hasattr(self, "_zero_rows"):
                self._zero_rows = torch.zeros(self.batch_size, dtype=torch.int32, device=self.device)
            weights, rows = weights.reshape(1, 8), self._zero_rows
        temperature = float(temperature)
        if not (0.0 < temperature < float("inf")):
            raise ValueError("%s: temperature must be positive and finite" % what)
        wt, idx = self._population(weights, rows, what)
        return wt, idx, temperature

    def sample_actions(self, weights, rows=None, temperature=1.0, score=True, logits=False):
        """One action per env drawn from the softmax linear policy of the reference's ``utils.py``
        (``compute_action_probabilities``): p(k) proportional to ``exp(features_k . weights / temperature)`` over
        the non-terminal placements, with the features ``get_after_states()`` returns (``feature_directions``
        applied).  ``weights`` is a tensor on the env's device, ``[8]`` (shared) or ``[P, 8]`` with ``rows`` as in
        :meth:`greedy_actions`.  Returns ``(action int32 [B], logp float32 [B])``, then ``score float32 [B, 8]``
        when ``score`` -- the gradient of ``logp`` with respect to the weights without the factor
        ``1 / temperature``, the reference's ``grad_of_log_action_probabilities`` -- then ``logits float32
        [B, a_max]`` when ``logits`` (``-inf`` past ``n_valid``).  An env that is over gets action -1, logp 0 and
        score 0.  The feature matrix is never written (``tetris_hip_policy_softmax_rows``).

        The draw is counter-based, keyed on ``seed``, ``step_idx`` and the env index: calling this twice in front
        of the same step returns the same draw; ``step(action)`` plays it and moves on to the next key.  The
        returned tensors are buffers the next call overwrites."""
        wt, idx, temperature = self._softmax_population(weights, rows, temperature, "sample_actions")
        B, dev = self.batch_size, self.device
        if not hasattr(self, "_sample_bufs"):
            self._sample_bufs = dict(action=torch.empty(B, dtype=torch.int32, device=dev),
                                     logp=torch.empty(B, dtype=torch.float32, device=dev))
        bufs = self._sample_bufs
        if score and "score" not in bufs:
            bufs["score"] = torch.empty((B, 8), dtype=torch.float32, device=dev)
        if logits and "logits" not in bufs:
            bufs["logits"] = torch.empty((B, self.a_max), dtype=torch.float32, device=dev)
        rc = self._lib.policy_softmax_rows(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), _ptr(wt), wt.shape[0],
                                           _ptr(idx), temperature, _ptr(bufs["action"]), _ptr(bufs["logp"]),
                                           _ptr(bufs["score"]) if score else None, None,
                                           _ptr(bufs["logits"]) if logits else None, _ptr(self.status), self.seed,
                                           self.step_idx, self.env_offset, B, self._hip_stream())
        self._lib.check(rc, "tetris_hip_policy_softmax_rows")
        out = [bufs["action"], bufs["logp"]]
        if score:
            out.append(bufs["score"])
        if logits:
            out.append(bufs["logits"])
        return tuple(out)

    def play_sampled(self, weights, rows=None, temperature=1.0, max_steps=1 << 20, chunk=64):
        """:meth:`play` with every action drawn from the softmax policy of :meth:`sample_actions` instead of the
        maximum (``tetris_hip_play_softmax``): launches of ``chunk`` steps, one ``n_valid.any()`` read-back per
        launch, until every game is over or ``max_steps`` steps are played.  Returns ``dict(lines uint32 [B],
        pieces uint32 [B], logp_total float32 [B], score_total float32 [B, 8], done bool [B])`` for THIS call:
        ``logp_total`` and ``score_total`` sum ``logp`` and ``score`` over the pieces each env placed -- what
        episodic REINFORCE needs: ``grad J ~ sum_env (return_env - baseline) * score_total_env``.  Everything
        :meth:`play` says about resets, finished envs, ``step_idx``, bad rows and replay mode holds here."""
        if self._stream is not None:
            raise ValueError("play_sampled draws pieces from the device bag (no replay stream)")
        max_steps, chunk = int(max_steps), int(chunk)
        if max_steps < 0 or chunk < 1:
            raise ValueError("play_sampled: max_steps must be >= 0 and chunk >= 1")
        wt, idx, temperature = self._softmax_population(weights, rows, temperature, "play_sampled")
        B, dev = self.batch_size, self.device
        lines = torch.zeros(B, dtype=torch.int32, device=dev)
        pieces = torch.zeros(B, dtype=torch.int32, device=dev)
        logp = torch.zeros(B, dtype=torch.float32, device=dev)
        score = torch.zeros((B, 8), dtype=torch.float32, device=dev)
        played = 0
        while played < max_steps:
            k = min(chunk, max_steps - played)
            rc = self._lib.play_softmax(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), k, _ptr(wt), wt.shape[0],
                                        _ptr(idx), temperature, _ptr(lines), _ptr(pieces), _ptr(logp), _ptr(score),
                                        _ptr(self.n_valid), _ptr(self.piece), _ptr(self.status), self.seed, self.step_idx,
                                        self.env_offset, B, self._hip_stream())
            self._lib.check(rc, "tetris_hip_play_softmax")
            self.step_idx += k
            played += k
            if not bool(self.n_valid.any()):
                break
        return dict(lines=lines.view(torch.uint32), pieces=pieces.view(torch.uint32), logp_total=logp, score_total=score,
                    done=self.n_valid == 0)

    def rollouts(self, length=5, n=5, policy="random", weights=None, pieces=None):
        """Tetris.perform_rollouts (game.py:150-160) for every env and every valid first action:
        ``returns float64 [B, a_max]`` = mean rollout return over ``n`` rollouts of ``length`` steps
        (NaN where the action does not exist).  ``policy`` = "random" or "greedy" (linear fitness
        on ``weights``, default the BCTS weights of game.py:111-118).  ``pieces`` (optional uint8
        ``[B, a_max, n, length]``): the list index every step of every rollout draws -- a recorded run
        of the reference's sampler; without it every rollout draws from its own fork of the env's bag.
        The envs are not modified."""
        pol = {"random": 0, "greedy": 1}[policy]
        w = (ctypes.c_float * 8)(*(self.BCTS_WEIGHTS if weights is None else [float(x) for x in weights]))
        out = torch.empty((self.batch_size, self.a_max), dtype=torch.float64, device=self.device)
        fed = None
        if pieces is not None:
            fed = torch.as_tensor(pieces, dtype=torch.uint8).to(self.device).contiguous()
            if tuple(fed.shape) != (self.batch_size, self.a_max, int(n), int(length)):
                raise ValueError("pieces must be [batch_size, a_max, n, length]")
            if int(fed.max()) >= len(self.piece_names):
                raise ValueError("pieces holds an index outside the piece list")
        rc = self._lib.rollouts(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), _ptr(out), int(length),
                                int(n), pol, w, _ptr(fed), self.seed, self.step_idx, self.env_offset, self.batch_size,
                                self._hip_stream())
        self._lib.check(rc, "tetris_hip_rollouts")
        return out

    def random_actions(self, out=None):
        """Uniform random valid action per env (the random-rollout policy)."""
        if not self._views_own:
            self._own_views()
        out = self.action if out is None else out
        rc = self._lib.policy_random(_ptr(self.n_valid), _ptr(out), self.seed, self.step_idx, self.env_offset,
                                     self.batch_size, self._hip_stream())
        self._lib.check(rc, "tetris_hip_policy_random")
        return out

    # -- inspection ---------------------------------------------------------------------------
    def boards(self):
        """State.representation for every env: int8 [B, R+4, C], row 0 = bottom."""
        cells = torch.empty((self.batch_size, self.stored_rows, self.num_columns), dtype=torch.int8,
                            device=self.device)
        rc = self._lib.decode(ctypes.byref(self.desc), _ptr(self.cols), _ptr(cells), None, self.batch_size,
                              self._hip_stream())
        self._lib.check(rc, "tetris_hip_decode")
        return cells

    def heights(self):
        """State.lowest_free_rows for every env: int32 [B, C]."""
        h = torch.empty((self.batch_size, self.num_columns), dtype=torch.int32, device=self.device)
        rc = self._lib.decode(ctypes.byref(self.desc), _ptr(self.cols), None, _ptr(h), self.batch_size,
                              self._hip_stream())
        self._lib.check(rc, "tetris_hip_decode")
        return h

    def set_boards(self, cells, piece=None):
        """Overwrite the boards (int8 [B, R+4, C]) and optionally the current
        pieces (list indices [B]); the valid masks are recomputed.

        The boards must be states a game can be in: a board with a cell in the overflow rows
        (row >= num_rows) is a terminal State (state.py:33-36), which the reference never steps
        from (game.py:69 keeps non-terminal afterstates only); the kernels' placement mask and
        10-row feature tables assume there is none, so such a board is refused here."""
        cells = torch.as_tensor(cells, device=self.device).to(torch.int8).contiguous()
        if cells.shape != (self.batch_size, self.stored_rows, self.num_columns):
            raise ValueError("cells must be [B, num_rows + 4, num_columns]")
        if bool((cells[:, self.num_rows:, :] != 0).any()):
            raise ValueError("boards with cells in the overflow rows (row >= num_rows) are terminal states "
                             "and cannot be set as current boards")
        rc = self._lib.encode(ctypes.byref(self.desc), _ptr(cells), _ptr(self.cols), self.batch_size,
                              self._hip_stream())
        self._lib.check(rc, "tetris_hip_encode")
        if piece is not None:
            p = torch.as_tensor(piece, device=self.device).to(torch.int64)
            if p.shape != (self.batch_size,):
                raise ValueError("piece must be [batch_size]")
            keep = ~(torch.tensor(15, dtype=torch.int64, device=self.device) << 48)
            self.meta.copy_((self.meta & keep) | (p << 48))
            self.piece.copy_(p.to(torch.uint8))
        self.refresh()

    def columns(self):
        """The boards as one bitboard per column, int64 [C, B] (bit r = cell (row r, column c)):
        the unpacked view of ``cols`` (debugging / tests; the kernels work on ``cols``)."""
        C, W = self.num_columns, 8 * self.desc.word_bytes
        planes = self.cols.permute(1, 0, 2).reshape(self.n_planes, -1)[:, :self.batch_size].to(torch.int64)
        if W == 32:
            planes = planes & 0xFFFFFFFF
        if self.n_planes == C:
            return planes
        F = W * 3 // 4
        full = (1 << W) - 1 if W < 64 else -1
        mask = (1 << F) - 1
        out = []

        def shr(x, n):  # logical shift right of a W-bit word held in int64
            if W == 64:
                return (x >> n) & ((1 << (64 - n)) - 1) if n else x
            return x >> n

        for c in range(C):
            b, k = 3 * (c // 4), c % 4
            if k == 0:
                v = planes[b]
            elif k == 1:
                v = shr(planes[b], F) | (planes[b + 1] << (W - F))
            elif k == 2:
                v = shr(planes[b + 1], 2 * F - W) | (planes[b + 2] << (2 * W - 2 * F))
            else:
                v = shr(planes[b + 2], 3 * F - 2 * W)
            out.append(v & mask)
        return torch.stack(out)

    def refresh(self):
        """Recompute valid masks / n_valid from (cols, piece) after a manual edit."""
        rc = self._lib.refresh(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), _ptr(self.n_valid),
                               self.batch_size, self._hip_stream())
        self._lib.check(rc, "tetris_hip_refresh")

    # -- moving envs: fork / resample / reset from a bank -------------------------------------------
    def _gather_index(self, index, what):
        """``index`` as a contiguous int32 [batch_size] tensor on the device; an entry no int32 can hold
        becomes -2 (out of range, reported like any other)."""
        idx = torch.as_tensor(index, device=self.device)
        if idx.shape != (self.batch_size,):
            raise ValueError("%s: index must be [batch_size] = [%d] (got %s)" % (what, self.batch_size, tuple(idx.shape)))
        if idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool:
            raise ValueError("%s: index must hold integers (got %s)" % (what, idx.dtype))
        if idx.dtype == torch.int64:
            idx = torch.where((idx < -1) | (idx > 2**31 - 1), torch.full_like(idx, -2), idx)
        if idx.dtype != torch.int32 or not idx.is_contiguous():
            idx = idx.to(torch.int32).contiguous()
        return idx

    def _gather_call(self, src_cols, src_meta, B_src, dst_cols, dst_meta, idx, status):
        rc = self._lib.gather_envs(ctypes.byref(self.desc), _ptr(src_cols), _ptr(src_meta), B_src, _ptr(dst_cols),
                                   _ptr(dst_meta), _ptr(self.n_valid), _ptr(self.piece), _ptr(idx), _ptr(status),
                                   self.batch_size, self._hip_stream())
        self._lib.check(rc, "tetris_hip_gather_envs")

    def copy_envs_from(self, src, index):
        """``self[j] := src[index[j]]`` for every env j: board, current piece, valid mask AND bag, one kernel on
        the stored words (``tetris_hip_gather_envs``; the batch form of restoring ``current_state`` /
        ``current_tetromino``, game.py:130-148).  ``src`` is another VecTetris on this device with the same
        columns, rows and piece set; ``index`` is ``[batch_size]`` ints.  ``-1`` leaves env j as it is; any
        other entry outside ``[0, src.batch_size)`` leaves it too and is counted, so that :meth:`check` raises
        IndexError.  ``n_valid`` and ``piece`` are updated; returns ``self``.

        Reset finished envs from a bank of stored states instead of the empty board::

            draws = torch.randint(bank.batch_size, (env.batch_size,), device=env.device)
            env.copy_envs_from(bank, torch.where(env.done, draws, -1))

        To permute or select within ONE batch use :meth:`gather_`; for a new batch :meth:`fork`."""
        self._check_source(src, "copy_envs_from", "the copy cannot run in place -- use gather_(index)")
        idx = self._gather_index(index, "copy_envs_from")
        self._gather_call(src.cols, src.meta, src.batch_size, self.cols, self.meta, idx, self.status)
        return self

    def _check_source(self, src, what, in_place):
        """what a call that reads envs of ``src`` into this batch asks of the pair"""
        if not isinstance(src, VecTetris):
            raise ValueError("%s: src must be a VecTetris" % what)
        if src is self:
            raise ValueError("%s: src is this env; %s" % (what, in_place))
        if (src.num_columns, src.num_rows, list(src.piece_names)) != (self.num_columns, self.num_rows,
                                                                       list(self.piece_names)):
            raise ValueError("%s: src is %dx%d %s, this env %dx%d %s" % (
                what, src.num_columns, src.num_rows, list(src.piece_names), self.num_columns, self.num_rows,
                list(self.piece_names)))
        if src.device != self.device:
            raise ValueError("%s: src lives on %s, this env on %s" % (what, src.device, self.device))
        if src._stream is not None or self._stream is not None:
            raise ValueError("%s: an env in replay mode (piece_stream / numpy_seeds) cannot take part: "
                             "its stream columns do not travel" % what)

    # -- afterstates as envs: children by (parent, action, next piece) ---------------------------------
    def expand_from(self, src, parent, action, next_piece=None, step_idx=None):
        """``self[j] := src[parent[j]]`` after placement ``action[j]``, in place (``tetris_hip_expand_envs``): the
        afterstate POSITIONS of ``src`` as envs of this batch -- the ``State`` objects the reference's
        ``get_after_states`` builds and ``step`` adopts (game.py:68-69, 82-92) -- for lookahead over the next
        piece, beam search, tree expansion, or a value network on :meth:`boards`.  One kernel; the board of a
        child never exists as a copy of its parent.  ``src`` is only read.

        ``parent`` and ``action`` are ``[batch_size]`` ints.  Env j becomes what ``src[parent[j]]`` is after
        ``step(action[j])`` without auto-reset, and ``obs / reward / done / lines / n_valid / piece`` of this
        batch are filled as a step fills them.  ``next_piece`` is ``uint8 [batch_size]`` list indices (or one
        int for all): the piece each child faces, its bag copied from the parent unchanged.  ``None`` draws the
        piece from the PARENT's bag exactly as ``src.step()`` would at ``step_idx`` (default ``src.step_idx``)
        -- with ``src``'s seed and the parent's global env index, so every child of one parent gets the same
        piece, and ``parent = arange(B)`` reproduces ``src.step(action)`` bit for bit in another batch.

        ``parent[j] == -1`` leaves env j and its outputs as they are.  Any other parent outside
        ``[0, src.batch_size)``, an action that is no placement of the parent (every action of a parent that is
        over) or a piece outside the set leaves env j too and is counted, so that :meth:`check` raises
        IndexError.  A child without a non-terminal placement of its piece has ``done`` set and ``n_valid`` 0;
        :meth:`play` and :meth:`greedy_actions` treat it as over.  ``src`` must be another VecTetris on this
        device with the same columns, rows and piece set; replay mode is refused.  This batch's ``step_idx`` is
        left alone.  Returns ``self``."""
        self._check_source(src, "expand_from", "a child batch is another VecTetris -- see expand()")
        par = self._gather_index(parent, "expand_from")
        act = self._gather_index(action, "expand_from")
        nxt = None
        if next_piece is not None:
            if isinstance(next_piece, int):
                next_piece = torch.full((self.batch_size,), next_piece if 0 <= next_piece < 255 else 255,
                                        dtype=torch.uint8, device=self.device)
            nxt = torch.as_tensor(next_piece, device=self.device)
            if nxt.shape != (self.batch_size,) or nxt.dtype.is_floating_point or nxt.dtype.is_complex or nxt.dtype == torch.bool:
                raise ValueError("expand_from: next_piece must be [batch_size] = [%d] list indices" % self.batch_size)
            if nxt.dtype != torch.uint8:  # an index no uint8 holds is outside every piece set
                nxt = torch.where((nxt < 0) | (nxt > 255), torch.full_like(nxt, 255), nxt).to(torch.uint8)
            nxt = nxt.contiguous()
        if not self._views_own:
            self._own_views()
        rc = self._lib.expand_envs(ctypes.byref(self.desc), _ptr(src.cols), _ptr(src.meta), src.batch_size,
                                   _ptr(self.cols), _ptr(self.meta), _ptr(par), _ptr(act), _ptr(nxt),
                                   _ptr(self._obs_buf) if self.compute_obs else None, _ptr(self._reward_buf),
                                   _ptr(self._done_buf), _ptr(self._lines_buf), _ptr(self.n_valid), _ptr(self.piece),
                                   _ptr(self.status), src.seed, src.step_idx if step_idx is None else int(step_idx),
                                   src.env_offset, self.batch_size, self._hip_stream())
        self._lib.check(rc, "tetris_hip_expand_envs")
        return self

    def _dense_children(self):
        """(parent int32 [B * a_max], action int32 [B * a_max], present bool [B, a_max]) of the dense expansion:
        child i * a_max + k is placement k of env i, absent (parent -1) where k >= n_valid[i]"""
        B, A, dev = self.batch_size, self.a_max, self.device
        k = torch.arange(A, dtype=torch.int32, device=dev)
        present = k[None, :] < self.n_valid[:, None].to(torch.int32)
        own = torch.arange(B, dtype=torch.int32, device=dev)[:, None].expand(B, A)
        parent = torch.where(present, own, torch.full_like(own, -1)).reshape(-1).contiguous()
        return parent, k.repeat(B), present

    def _child_batch(self, **kw):
        cfg = dict(auto_reset=self.auto_reset, compute_obs=self.compute_obs)
        cfg.update(kw)
        return VecTetris(self.num_columns, self.num_rows, self.batch_size * self.a_max, device=self.device,
                         pieces=list(self.piece_names), seed=self.seed, feature_directions=self.feature_directions,
                         env_offset=self.env_offset, afterstate_layout=self.afterstate_layout, **cfg)

    def expand(self, next_piece=None):
        """Every placement of every env as an env: returns ``(child, present)`` -- a NEW VecTetris of
        ``batch_size * a_max`` envs with the configuration :meth:`fork` passes on, child ``i * a_max + k`` being
        env i after placement k (:meth:`expand_from`), and ``present`` ``bool [B, a_max]``: ``k < n_valid[i]``.
        Absent children are freshly reset envs and are not counted as errors.  ``next_piece`` is one list index
        every child gets, or ``None``: each child faces the piece its parent would draw at this step, and
        ``child.step_idx = step_idx + 1`` (else ``step_idx``), so the children play on as the parent would have.
        This env is unchanged.

        Row k of ``get_after_states()`` is ``child.obs[i * a_max + k]``; ``child.boards()`` are the afterstate
        boards, ``child.reward / done / lines`` what the placement earns."""
        if self._stream is not None:
            raise ValueError("expand: an env in replay mode (piece_stream / numpy_seeds) cannot be expanded: its "
                             "stream columns do not travel")
        if next_piece is not None:
            next_piece = int(next_piece)
            if not 0 <= next_piece < len(self.piece_names):
                raise ValueError("expand: next_piece must be a list index below %d" % len(self.piece_names))
        parent, action, present = self._dense_children()
        child = self._child_batch()
        child.expand_from(self, parent, action, next_piece)
        child.step_idx = self.step_idx + (1 if next_piece is None else 0)
        return child, present

    def two_ply_values(self, weights=None):
        """``float32 [B, a_max, n_pieces]``: ``value[i, k, p]`` is the best linear fitness (``weights``: 8 floats,
        default the BCTS vector of game.py:111-118; :meth:`greedy_actions`' ``best_value``) among the
        non-terminal placements of piece ``p`` on the board env i has after ITS placement k -- the second ply of
        a two-piece lookahead.  ``-inf`` where that child is over with piece ``p``, ``NaN`` where
        ``k >= n_valid[i]``.  One :meth:`expand_from` into one child batch (kept for the next call) and one
        :meth:`greedy_actions` per piece; this env is unchanged.

        The two-piece-lookahead action averages over the pieces that can come next and takes the best first
        placement.  With a uniform bag::

            v = env.two_ply_values()
            action = torch.nan_to_num(v.mean(dim=2), nan=-float("inf")).argmax(dim=1)

        (weight the mean by the bag in ``meta`` bits 52-63 to follow the sampler exactly; add the first ply's
        own reward, ``expand()[0].lines``, for a score that counts both placements)."""
        if self._stream is not None:
            raise ValueError("two_ply_values: an env in replay mode (piece_stream / numpy_seeds) cannot be expanded")
        B, A, P, dev = self.batch_size, self.a_max, len(self.piece_names), self.device
        child = getattr(self, "_two_ply_child", None)
        if child is None:
            child = self._two_ply_child = self._child_batch(auto_reset=False, compute_obs=False)
        parent, action, present = self._dense_children()
        out = torch.empty((B, A, P), dtype=torch.float32, device=dev)
        nan = torch.full((B, A), float("nan"), dtype=torch.float32, device=dev)
        ninf = torch.full((B, A), -float("inf"), dtype=torch.float32, device=dev)
        for p in range(P):
            child.expand_from(self, parent, action, p)
            _, value = child.greedy_actions(weights)
            over = (child.n_valid == 0).view(B, A)
            out[:, :, p] = torch.where(present, torch.where(over, ninf, value.view(B, A)), nan)
        return out

    def lookahead(self, weights=None, death_value=-float("inf"), return_q=False, return_values=False):
        """The two-piece-lookahead policy in one kernel (``tetris_hip_policy_two_ply``): for every env, the first
        placement whose afterstate is best ON AVERAGE over the pieces the env's bag can hand out next, each next piece
        placed greedily on the linear fitness (``weights``: 8 floats, default the BCTS vector of game.py:111-118).
        Returns ``(action int32 [B], value float32 [B])``: the first action of maximal mean (the lowest of several
        that reach it exactly; -1 for an env that is over) and that mean -- the kernel's float32 sum over the bag's
        pieces in ascending order divided by their number (value 0 where the action is -1).

        The table behind it is :meth:`two_ply_values`' bit for bit, but no child env is built: the child boards stay
        in registers, so the call needs no child batch, runs at any batch size, and -- nothing being drawn -- works in
        replay mode too.  A next piece without a non-terminal placement counts ``death_value`` in the mean (``-inf``,
        the default: a first placement after which some piece of the bag ends the game is never preferred to one that
        survives every piece; a finite value trades that risk; NaN and ``+inf`` are refused).

        ``return_q`` appends ``q_mean float32 [B, a_max]``, the mean of every first action (NaN for
        ``k >= n_valid``), ``return_values`` the table ``values float32 [B, a_max, n_pieces]`` (``-inf`` where the
        child is over with that piece, NaN for ``k >= n_valid``).  The tensors are reused by the next call.  This env
        is unchanged; play the action with :meth:`step`."""
        w = (ctypes.c_float * 8)(*(self.BCTS_WEIGHTS if weights is None else [float(x) for x in weights]))
        B, A, P, dev = self.batch_size, self.a_max, len(self.piece_names), self.device
        if not hasattr(self, "_la_action"):
            self._la_action = torch.empty(B, dtype=torch.int32, device=dev)
            self._la_value = torch.empty(B, dtype=torch.float32, device=dev)
            self._la_n_bag = torch.empty(B, dtype=torch.uint8, device=dev)
            self._la_q = self._la_values = None
        q = v = None
        if return_q:
            if self._la_q is None:
                self._la_q = torch.empty((B, A), dtype=torch.float32, device=dev)
            q = self._la_q
        if return_values:
            if self._la_values is None:
                self._la_values = torch.empty((B, A, P), dtype=torch.float32, device=dev)
            v = self._la_values
        rc = self._lib.policy_two_ply(ctypes.byref(self.desc), _ptr(self.cols), _ptr(self.meta), w, float(death_value),
                                      _ptr(v), _ptr(q), _ptr(self._la_n_bag), _ptr(self._la_action), _ptr(self._la_value),
                                      B, self._hip_stream())
        self._lib.check(rc, "tetris_hip_policy_two_ply")
        n = self._la_n_bag.to(torch.float32)
        out = (self._la_action, self._la_value / n)
        if return_q:
            out += (q / n[:, None],)
        if return_values:
            out += (v,)
        return out

    def fork(self, index, env_offset=None, seed=None):
        """A NEW VecTetris of ``len(index)`` envs, env j a copy of ``self[index[j]]`` (bag included), with this
        env's geometry, pieces, feature_directions, auto_reset, compute_obs and afterstate_layout; ``seed`` and
        ``env_offset`` default to this env's and ``step_idx`` is copied, so ``fork(arange(B))`` plays on exactly
        as this env does.  Every entry must name an env (no ``-1``).

        Replicate one position 4096 times for Monte-Carlo evaluation, or each env K times for a search
        (another ``env_offset`` makes the copies draw different pieces)::

            mc = env.fork(torch.full((4096,), 17), env_offset=1 << 20)
            beam = env.fork(torch.arange(env.batch_size).repeat_interleave(K), env_offset=env.batch_size)"""
        idx = torch.as_tensor(index, device=self.device)
        if idx.dim() != 1 or idx.numel() == 0:
            raise ValueError("fork: index must be a non-empty 1-d tensor")
        if self._stream is not None:
            raise ValueError("fork: an env in replay mode (piece_stream / numpy_seeds) cannot be forked: its stream "
                             "columns do not travel")
        if bool((idx == -1).any()):
            raise ValueError("fork: every entry of index must name an env of this batch (-1 has nothing to keep)")
        child = VecTetris(self.num_columns, self.num_rows, idx.numel(), device=self.device, pieces=list(self.piece_names),
                          auto_reset=self.auto_reset, seed=self.seed if seed is None else seed,
                          feature_directions=self.feature_directions,
                          env_offset=self.env_offset if env_offset is None else env_offset,
                          afterstate_layout=self.afterstate_layout, compute_obs=self.compute_obs)
        child.step_idx = self.step_idx
        return child.copy_envs_from(self, idx)

    def gather_(self, index):
        """In place: ``self[j] := self[index[j]]`` (``-1`` keeps env j; an entry outside the batch keeps it too and
        is counted, see :meth:`check`).  Resample a population after weighting it, or compact the live envs to
        the front::

            env.gather_(torch.multinomial(weights, env.batch_size, replacement=True))

        The kernel cannot permute in place, so the envs are gathered into a spare ``cols`` / ``meta`` pair
        (allocated on first use and kept) which then becomes the env's storage: ``env.cols`` / ``env.meta`` are
        other tensors afterwards, the bound step call is rebuilt and graphs captured before refuse to replay.
        Returns ``self``."""
        if self._stream is not None:
            raise ValueError("gather_: an env in replay mode (piece_stream / numpy_seeds) cannot be permuted: its "
                             "stream columns do not travel")
        idx = self._gather_index(index, "gather_")
        if getattr(self, "_spare", None) is None:
            self._spare = (torch.zeros_like(self.cols), torch.zeros_like(self.meta))
        cols, meta = self._spare
        own = torch.arange(self.batch_size, dtype=torch.int32, device=self.device)
        # kept envs travel as index j; an out-of-range entry is counted by the first call (which leaves the
        # spare's env j alone) and carried over by the second
        self._gather_call(self.cols, self.meta, self.batch_size, cols, meta, torch.where(idx == -1, own, idx), self.status)
        bad = (idx < -1) | (idx >= self.batch_size)
        self._gather_call(self.cols, self.meta, self.batch_size, cols, meta, torch.where(bad, own, torch.full_like(own, -1)), None)
        self._spare = (self.cols, self.meta)
        self.cols, self.meta = cols, meta
        self._invalidate_bound_call()
        return self

    def totals(self):
        """int64 [4] device tensor: (invalid, episodes, lines, steps) summed over the per-wave slots."""
        return (self.status.view(-1, 4).to(torch.int64) & 0xFFFFFFFF).sum(dim=0)

    def stats(self):
        """Counters accumulated by the step kernel (synchronises)."""
        s = self.totals().cpu().numpy()
        return dict(invalid=int(s[0]), episodes=int(s[1]), lines=int(s[2]), steps=int(s[3]))

    def check(self):
        """Raise IndexError if any step so far received an out-of-range action
        (game.py:83 raises it immediately; the batch path reports lazily)."""
        n = self.stats()["invalid"]
        if n:
            raise IndexError("%d out-of-range actions were passed to step()%s" % (
                n, " (or the replay piece_stream ran out of rows)" if self._stream is not None else ""))

    # -- checkpoint / snapshot --------------------------------------------------------------------
    STATE_FORMAT = 3  # 1: plane-major cols, C-bit mask fields; 2: tile-major cols, 12-bit mask fields (unversioned)

    def state_dict(self):
        d = dict(format=self.STATE_FORMAT, abi=_lib.ABI_VERSION, cols=self.cols.clone(), meta=self.meta.clone(), n_valid=self.n_valid.clone(),
                 piece=self.piece.clone(), status=self.status.clone(), step_idx=self.step_idx, seed=self.seed,
                 num_columns=self.num_columns, num_rows=self.num_rows, pieces=list(self.piece_names))
        if self._cursor is not None:
            d["cursor"] = self._cursor.clone()
        return d

    def load_state_dict(self, d):
        if (d["num_columns"], d["num_rows"], list(d["pieces"])) != (self.num_columns, self.num_rows,
                                                                     list(self.piece_names)):
            raise ValueError("state_dict belongs to a different env configuration")
        if d.get("format") != self.STATE_FORMAT:
            raise ValueError("state_dict has storage format %r, this build reads format %d (the layout of `cols` / "
                             "`meta` changed between them; re-create the env and set_boards() from decoded cells)"
                             % (d.get("format"), self.STATE_FORMAT))
        for k in ("cols", "meta", "n_valid", "piece", "status"):
            if tuple(d[k].shape) != tuple(getattr(self, k).shape) or d[k].dtype != getattr(self, k).dtype:
                raise ValueError("state_dict[%r] is %s %s, this env holds %s %s (different batch size?)"
                                 % (k, tuple(d[k].shape), d[k].dtype, tuple(getattr(self, k).shape), getattr(self, k).dtype))
        for k in ("cols", "meta", "n_valid", "piece", "status"):
            getattr(self, k).copy_(d[k])
        if self._cursor is not None and "cursor" in d:
            self._cursor.copy_(d["cursor"])
        self.step_idx = int(d["step_idx"])
        self.seed = int(d["seed"])  # (drops the bound step call and invalidates captured graphs)


class StepGraph:
    """``n_steps`` steps of one VecTetris as a HIP graph (``VecTetris.capture_steps``)."""

    def __init__(self, env, n_steps, action_fn=None):
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        self.env, self.n_steps = env, n_steps
        lib = env._lib
        self._counter = torch.zeros(1, dtype=torch.int64, device=env.device)
        self._counter.fill_(env.step_idx)
        self._expected = env.step_idx
        call = env._step_call if env._step_call is not None else env._bind_step_call()
        self._generation = env._generation
        self._call_buf = env._step_call_buf  # the bound call's memory must outlive every launch enqueued from here

        def launch_stream():  # the stream being captured / the current stream, exactly as step() picks it
            if env._raw_stream is not None:
                return env._raw_stream(env.device.index)
            return env._hip_stream()

        def enqueue():
            if not env._views_own:
                env._own_views()
            for k in range(n_steps):
                a = None
                if action_fn is not None:
                    a = action_fn(env, k)
                    if a.dtype != torch.int32 or not a.is_contiguous() or a.shape != (env.batch_size,):
                        raise ValueError("action_fn must return a contiguous int32 [batch_size] tensor")
                    self._keep.append(a)
                rc = lib.step_call_run_counted(call, None if a is None else a.data_ptr(), self._counter.data_ptr(), k,
                                               launch_stream())
                lib.check(rc, "tetris_hip_step_call_run_counted")
            lib.check(lib.counter_add(self._counter.data_ptr(), n_steps, launch_stream()), "tetris_hip_counter_add")

        self._keep = []
        self._graph = None
        self._enqueue = enqueue
        if env.device.type == "cuda":
            torch.cuda.synchronize(env.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                enqueue()
            self._graph = g

    def replay(self):
        """Advance the env by ``n_steps`` steps (returns the per-step views of the last step)."""
        env = self.env
        if env._generation != self._generation:
            raise RuntimeError("this StepGraph was captured before the env's seed / auto_reset / compute_obs / "
                               "env_offset changed (or load_state_dict / gather_ ran): its launches hold the old values -- "
                               "capture a new one with env.capture_steps()")
        if env.step_idx != self._expected:  # plain step() calls in between: re-seat the device counter
            self._counter.fill_(env.step_idx)
        if not env._views_own:
            env._own_views()
        if self._graph is not None:
            self._graph.replay()
        else:  # no graph support on this device type (CPU test harness): the same launches, eagerly
            self._enqueue()
        env.step_idx += self.n_steps
        self._expected = env.step_idx
        return env.obs, env.reward, env.done, env.lines

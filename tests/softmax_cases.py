"""Shared cases for the softmax linear policy: tetris_hip_policy_softmax_rows and tetris_hip_play_softmax,
VecTetris.sample_actions and VecTetris.play_sampled.  Each takes the torch device: "cuda" (tests/test_softmax_gpu.py,
the HIP kernels) or "cpu" with the harness backend (tests/test_softmax_host.py, the same per-env bodies compiled by
g++ on libm's expf / logf).  The two backends are never compared bit for bit with each other: every numeric
comparison is against float64 NumPy, every bit-for-bit one stays on one backend.

Yardsticks: NumPy float32 for the logits (bit-exact), float64 NumPy on those exact logits and on the features of
get_after_states() for logz / logp / score, an independent uint32 restatement of the header's hash recipe for the
draw, the reference's utils.py through tests/golden/g11_softmax.npz.

Measured tolerances (the largest error over case 2 / case 3 on all four geometries and the three temperatures,
relative to max(1, |value|); for score relative to max(1, max_k |f_k[q]|)):
    logz                  CPU twin 1.57e-07   MI355X 1.57e-07
    logp                  CPU twin 6.18e-07   MI355X 6.18e-07
    score                 CPU twin 9.56e-07   MI355X 9.56e-07   -> TOL   = 2^-16 = 1.53e-05 (8 x 9.56e-07 = 7.65e-06,
                                                                   just above 2^-17, rounded up to a power of two)
    draw (z64 deficit)    CPU twin 0          MI355X 0          -> TOL_Z = 2^-21
(the worst case of each is the same env on both backends: 12x20, standard7)
No env of those cases picked anything but the float64 argmax, so 8 x the measurement is 0; TOL_Z is instead 8 x the
float32 rounding of z itself: z = u - log(-log U) is one float32 subtraction of a float32 u, error <= 2^-24 |z|
plus the error of the double logarithm (a few 2^-24, absolute), and two placements are compared -- 2^-21 relative
to max(1, |z|) is 8 x 2^-24.

On the directed boards (policy_directed_cases.softmax_rows_directed: the oracle's features, nine-piece catalogue, the
three temperatures without and with feature_directions) the same bounds hold unchanged -- s and g are float32 sums of
at most a_max <= 44 same-signed terms, (a_max + 8) x 2^-24 = 3.1e-06 < TOL.  Largest error per kernel variant
(word, storage, chunks) over its geometries, CPU twin | MI355X, and the envs off the float64 argmax:
    u32 packed 2 (11)     logz 2.48e-07 | 2.48e-07   logp 6.19e-07 | 6.19e-07   score 8.81e-07 | 8.81e-07   off 0 | 0
    u32 planes 3 (3)      logz 9.49e-08 | 1.50e-07   logp 5.28e-07 | 5.28e-07   score 8.11e-07 | 8.11e-07   off 0 | 0
    u64 packed 4 (5)      logz 1.08e-07 | 1.30e-07   logp 5.78e-07 | 6.38e-07   score 8.09e-07 | 8.09e-07   off 0 | 0
    u64 planes 5 (2)      logz 7.21e-08 | 1.33e-07   logp 4.26e-07 | 4.26e-07   score 6.60e-07 | 6.60e-07   off 0 | 0
    u64 planes 6 (3)      logz 8.38e-08 | 1.33e-07   logp 5.35e-07 | 5.35e-07   score 9.01e-07 | 9.01e-07   off 0 | 0
(z64 deficit 0 everywhere.)  The six-step sampled games of play_softmax_directed: logp_total within 9.04e-07 and
score_total within 1.07e-06 of the float64 sums on both backends, against the bound 6 x TOL."""
import ctypes
import os

import numpy as np
import pytest
import torch

import footprint_cases as fc
import population_cases as pc
from population_cases import B, BCTS, _t, lanes, random_rows, snapshot, weight_rows

TOL = 2.0 ** -16
TOL_Z = 2.0 ** -21
TEMPERATURES = [0.5, 1.0, 20.0]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_softmax.npz")
# tests/golden/make_golden_softmax.py: (pieces, feature_directions) of fixture config i
GOLDEN_DIRECTIONS = [-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, 1.0, -1.0]
GOLDEN_CONFIGS = [("default", None), (pc.STANDARD7, None), ("default", GOLDEN_DIRECTIONS), (pc.STANDARD7, GOLDEN_DIRECTIONS)]

_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def env_with_edges(device, C, R, pieces, n=B, seed=5, **kw):
    """population_cases._env plus the directed boards: some envs are over, some have a single placement"""
    env = pc._env(device, C, R, pieces, n, seed=seed, **kw)
    assert pc._with_directed_boards(env) >= 20
    return env


class Out:
    """the outputs of one tetris_hip_policy_softmax_rows call, pre-filled with sentinels"""

    def __init__(self, env, n=None, score=True, logz=True, logits=True):
        n, dev = env.batch_size if n is None else n, env.device
        self.action = torch.full((n,), -7, dtype=torch.int32, device=dev)
        self.logp = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
        self.score = torch.full((n, 8), -7.0, dtype=torch.float32, device=dev) if score else None
        self.logz = torch.full((n,), -7.0, dtype=torch.float32, device=dev) if logz else None
        self.logits = torch.full((n, env.a_max), -7.0, dtype=torch.float32, device=dev) if logits else None

    def tensors(self):
        return [t for t in (self.action, self.logp, self.score, self.logz, self.logits) if t is not None]

    def numpy(self):
        return [None if t is None else t.cpu().numpy() for t in (self.action, self.logp, self.score, self.logz, self.logits)]


def raw_softmax(env, weights, rows, temperature, out, status=None, step_idx=None, cols=None, meta=None, env_offset=None,
                n=None):
    rc = env._lib.policy_softmax_rows(ctypes.byref(env.desc), _p(env.cols if cols is None else cols),
                                      _p(env.meta if meta is None else meta), _p(weights), weights.shape[0], _p(rows),
                                      float(temperature), _p(out.action), _p(out.logp), _p(out.score), _p(out.logz),
                                      _p(out.logits), _p(status), env.seed, env.step_idx if step_idx is None else step_idx,
                                      env.env_offset if env_offset is None else env_offset,
                                      env.batch_size if n is None else n, env._hip_stream())
    assert rc == 0, rc
    return out


def raw_play(env, K, weights, rows, temperature, lines, pieces, logp, score, n_valid=None, piece=None, status=None,
             step_idx0=None):
    rc = env._lib.play_softmax(ctypes.byref(env.desc), _p(env.cols), _p(env.meta), K, _p(weights), weights.shape[0], _p(rows),
                               float(temperature), _p(lines), _p(pieces), _p(logp), _p(score), _p(n_valid), _p(piece),
                               _p(status), env.seed, env.step_idx if step_idx0 is None else step_idx0, env.env_offset,
                               env.batch_size, env._hip_stream())
    assert rc == 0, rc


def totals(env):
    n, dev = env.batch_size, env.device
    return (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
            torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros((n, 8), dtype=torch.float32, device=dev))


# ---- NumPy yardsticks ---------------------------------------------------------------------------------------------
def numpy_logits(feats, w, temperature):
    """float32 [B, A]: (sum_q f[q] * w[q], left to right, every operation rounded) * (1.0f / temperature)"""
    assert feats.dtype == np.float32 and w.dtype == np.float32
    acc = feats[:, :, 0] * w[:, None, 0]
    for q in range(1, 8):
        acc = acc + feats[:, :, q] * w[:, None, q]
    inv_t = np.float32(1.0) / np.float32(temperature)
    u = acc * inv_t
    assert u.dtype == np.float32
    return u


_M = 0xFFFFFFFF


def _mix32(x):
    """include/tetris_hip.h's mix32 on uint64 arrays (or ints) holding uint32 values"""
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & _M
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & _M
    return x ^ (x >> 16)


def hash_key(seed, counter):
    k = _mix32((seed & _M) ^ 0x9E3779B9)
    k = _mix32(k ^ ((seed >> 32) & _M))
    k = _mix32(k ^ (counter & _M))
    return _mix32(k ^ ((counter >> 32) & _M))


def uniforms(seed, step_idx, envs, A):
    """float64 [len(envs), A]: U_k of the header's recipe for the global env indices `envs` and rows k < A"""
    key = np.uint64(hash_key(int(seed), 4 * int(step_idx) + 1))
    k1 = ((np.arange(A, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B1)) & np.uint64(_M)
    per_row = _mix32(key ^ k1)
    env = (np.asarray(envs).astype(np.uint64) & np.uint64(_M))[:, None]
    h = ((per_row[None, :] ^ env) * np.uint64(0x9E3779B1)) & np.uint64(_M)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(_M)
    h = h ^ (h >> np.uint64(13))
    return ((h >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def float64_softmax(u, feats, nv):
    """(logz [B], p [B, A], expectation [B, 8]) in float64 from float32 logits u [B, A] and features [B, A, 8];
    rows >= nv carry no mass.  Envs with nv == 0 give logz = -inf, p = 0."""
    valid = np.arange(u.shape[1])[None, :] < nv[:, None]
    u64 = np.where(valid, u.astype(np.float64), -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = u64.max(axis=1)
        e = np.where(valid, np.exp(u64 - np.where(np.isfinite(m), m, 0.0)[:, None]), 0.0)
        s = e.sum(axis=1)
        logz = m + np.log(s)
        p = e / np.where(s > 0, s, 1.0)[:, None]
    return logz, p, np.einsum("ba,baq->bq", p, feats.astype(np.float64))


def rel(err, scale):
    return float(np.max(np.abs(err) / np.maximum(1.0, np.abs(scale)))) if np.size(err) else 0.0


def errors_vs_float64(out, u, feats, nv):
    """the largest errors of logz, logp and score (case 2's measure) of the envs with a placement"""
    action, logp, score, logz, _ = out
    alive = nv > 0
    idx = np.nonzero(alive)[0]
    logz64, p, ef = float64_softmax(u, feats, nv)
    a = action[idx]
    assert np.all((a >= 0) & (a < nv[idx]))
    logp64 = u[idx, a].astype(np.float64) - logz64[idx]
    f64 = feats.astype(np.float64)
    score64 = f64[idx, a] - ef[idx]
    valid = np.arange(u.shape[1])[None, :] < nv[:, None]
    fmax = np.max(np.abs(np.where(valid[:, :, None], f64, 0.0)), axis=1)  # [B, 8]
    return dict(logz=rel(logz[idx] - logz64[idx], logz64[idx]), logp=rel(logp[idx] - logp64, logp64),
                score=rel(score[idx] - score64, fmax[idx]))


def afterstates(env):
    feats, nv = env.get_after_states()
    return feats.cpu().numpy().copy(), nv.cpu().numpy().astype(np.int64)


def check_over_envs(out, nv):
    """env over: -1, 0, 0, 0 and logits all -inf"""
    action, logp, score, logz, logits = out
    over = nv == 0
    assert np.array_equal(action[over], np.full(int(over.sum()), -1, np.int32))
    assert np.array_equal(action >= 0, ~over)
    for t in (logp, score, logz):
        if t is not None:
            assert not np.any(t[over])
    if logits is not None:
        assert np.all(np.isneginf(logits[over]))


# ---- 1. logits bit-exact, 2. logz / logp / score against float64, 3. the draw ------------------------------------
def numerics(device, C, R, pieces, orc=None, report=None):
    env = env_with_edges(device, C, R, pieces)
    W = weight_rows()
    rows = random_rows(B, len(W), seed=B)
    Wm, rows_t = _t(W, device), _t(rows, device)
    feats, nv = afterstates(env)
    assert int((nv == 0).sum()) > 0 or (C, R) != (6, 10)
    if orc is not None:  # the oracle's features
        ofeats, onv, _, _ = pc.oracle_twin(orc, env, pieces).afterstates()
        assert np.array_equal(onv, nv) and np.array_equal(ofeats, feats)
    worst = dict(logz=0.0, logp=0.0, score=0.0, z=0.0, off_argmax=0)
    envs = (env.env_offset + np.arange(B)) & _M
    for T in TEMPERATURES:
        out = raw_softmax(env, Wm, rows_t, T, Out(env), env.status).numpy()
        action, logp, score, logz, logits = out
        # 1. the logits, bit for bit; the padding is -inf
        want_u = numpy_logits(feats, W[rows], T)
        valid = np.arange(env.a_max)[None, :] < nv[:, None]
        assert np.array_equal(logits.view(np.int32)[valid], want_u.view(np.int32)[valid]), "T = %g" % T
        assert np.all(np.isneginf(logits[~valid]))
        check_over_envs(out, nv)
        # 2. float64 on the exact logits and features
        for k, v in errors_vs_float64(out, logits, feats, nv).items():
            worst[k] = max(worst[k], v)
        # 3. the draw: the action's float64 Gumbel value is the maximum, within the float32 rounding of z
        U = uniforms(env.seed, env.step_idx, envs, env.a_max)
        with np.errstate(divide="ignore"):
            z64 = np.where(valid, logits.astype(np.float64) - np.log(-np.log(U)), -np.inf)
        idx = np.nonzero(nv > 0)[0]
        top = z64[idx].max(axis=1)
        mine = z64[idx, action[idx]]
        with np.errstate(invalid="ignore"):
            deficit = np.where(np.isinf(top) & np.isinf(mine), 0.0, top - mine) / np.maximum(1.0, np.abs(np.where(np.isinf(top), 1.0, top)))
        worst["z"] = max(worst["z"], float(deficit.max()))
        worst["off_argmax"] += int((np.argmax(z64[idx], axis=1) != action[idx]).sum())
    assert env.stats()["invalid"] == 0
    print("softmax numerics %s %dx%d: %r" % (device, C, R, worst))
    if report is not None:
        report.append(((C, R), worst))
    assert worst["logz"] <= TOL and worst["logp"] <= TOL and worst["score"] <= TOL, worst
    assert worst["z"] <= TOL_Z, worst
    return worst


# ---- 4. distribution ---------------------------------------------------------------------------------------------------
def chi2_quantile(df, q=1.0 - 1e-6):
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(q, df))
    except ImportError:  # Wilson-Hilferty
        from statistics import NormalDist
        z = NormalDist().inv_cdf(q)
        return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3


def distribution(device, n=4096, T=20.0, seed=41):
    from tetris_amd import VecTetris
    src = pc._env(device, 10, 20, "default", 64, seed=7, steps=14)
    k = int(torch.argmax(src.n_valid.to(torch.int32)))  # a mid-game board with many placements
    env = VecTetris(10, 20, n, device=device, auto_reset=False, seed=seed)
    env.set_boards(src.boards()[k:k + 1].expand(n, -1, -1).contiguous(), src.piece[k:k + 1].expand(n).contiguous())
    assert int(env.boards()[0].sum()) >= 20
    w = _t(BCTS, device)
    action, logp, logits = (t.clone() for t in env.sample_actions(w, temperature=T, score=False, logits=True))
    nv = int(env.n_valid[0])
    assert nv > 8 and bool((env.n_valid == nv).all())
    u = logits.cpu().numpy()
    assert np.array_equal(u, np.tile(u[:1], (n, 1)))  # one board: one row of logits
    u64 = u[0, :nv].astype(np.float64)
    p = np.exp(u64 - u64.max())
    p /= p.sum()
    a = action.cpu().numpy()
    assert a.min() >= 0 and a.max() < nv
    counts = np.bincount(a, minlength=nv).astype(np.float64)
    expect = n * p
    big = expect >= 5
    obs_cells = list(counts[big]) + ([counts[~big].sum()] if (~big).any() else [])
    exp_cells = list(expect[big]) + ([expect[~big].sum()] if (~big).any() else [])
    assert len(exp_cells) >= 4, "the temperature leaves mass on too few placements: %r" % (p,)
    chi2 = float(sum((o - e) ** 2 / e for o, e in zip(obs_cells, exp_cells)))
    bound = chi2_quantile(len(exp_cells) - 1)
    print("softmax distribution %s: chi2 %.2f, dof %d, bound %.2f" % (device, chi2, len(exp_cells) - 1, bound))
    assert chi2 <= bound, (chi2, bound, obs_cells, exp_cells)
    assert np.allclose(logp.cpu().numpy(), np.log(p)[a], atol=1e-4)
    # counter-based: the same step twice is the same draw, the next step another one
    again = env.sample_actions(w, temperature=T, score=False)[0]
    assert torch.equal(again, action)
    env.step_idx += 1
    other = env.sample_actions(w, temperature=T, score=False)[0]
    assert int((other != action).sum()) > n // 4


# ---- 5. limits -----------------------------------------------------------------------------------------------------------
def limits(device, C, R, pieces):
    env = env_with_edges(device, C, R, pieces)
    feats, nv = afterstates(env)
    alive = nv > 0
    zero_rows = torch.zeros(B, dtype=torch.int32, device=device)
    # cold: the sampled action has the greedy policy's value, bit for bit (2^20 scales the fitness exactly)
    Wb = _t(BCTS[None], device)
    cold = raw_softmax(env, Wb, zero_rows, 2.0 ** -20, Out(env)).numpy()
    ba = torch.full((B,), -7, dtype=torch.int32, device=device)
    bv = torch.full((B,), -7.0, dtype=torch.float32, device=device)
    pc.raw_greedy_rows(env, Wb, zero_rows, ba, bv)
    action, logp, score, logz, logits = cold
    fitness = logits[alive, action[alive]] * np.float32(2.0 ** -20)
    assert np.array_equal(fitness.view(np.int32), bv.cpu().numpy()[alive].view(np.int32))
    for t in (logp, score, logz):
        assert np.all(np.isfinite(t))
    valid = np.arange(env.a_max)[None, :] < nv[:, None]
    assert np.all(np.isfinite(logits[valid]))
    check_over_envs(cold, nv)
    # all-zero weights: the uniform distribution
    Wz = torch.zeros((1, 8), dtype=torch.float32, device=device)
    flat = raw_softmax(env, Wz, zero_rows, 1.0, Out(env)).numpy()
    action, logp, score, logz, logits = flat
    want_logp = -np.log(nv[alive].astype(np.float64))
    assert rel(logp[alive] - want_logp, want_logp) <= TOL
    f64 = np.where(valid[:, :, None], feats.astype(np.float64), 0.0)
    mean = f64.sum(axis=1)[alive] / nv[alive, None]
    fmax = np.abs(f64).max(axis=1)[alive]
    idx = np.nonzero(alive)[0]
    assert rel(score[alive] - (f64[idx, action[idx]] - mean), fmax) <= TOL
    check_over_envs(flat, nv)
    # exactly one placement: logp and score are exactly 0, whatever the weights
    Wm = _t(weight_rows(), device)
    rows_t = _t(random_rows(B, 7, seed=6), device)
    one = nv == 1
    for T in TEMPERATURES:
        action, logp, score, logz, logits = raw_softmax(env, Wm, rows_t, T, Out(env)).numpy()
        assert np.array_equal(action[one], np.zeros(int(one.sum()), np.int32))
        assert not np.any(logp[one]) and not np.any(score[one])
        assert np.array_equal(logz[one].view(np.int32), logits[one, 0].view(np.int32))
    return int(one.sum()), int((~alive).sum())


# ---- 6. the reference's utils.py (tests/golden/g11_softmax.npz) ---------------------------------------------------------
def reference_fixture(device):
    from tetris_amd import VecTetris
    g = np.load(GOLDEN)
    assert len(g["piece"]) >= 20
    worst = 0.0
    for ci, (pieces, directions) in enumerate(GOLDEN_CONFIGS):
        sel = np.nonzero(g["config"] == ci)[0]
        n = len(sel)
        assert n >= 4
        temperature = float(g["temperature"][sel[0]])
        assert np.all(g["temperature"][sel] == temperature)
        env = VecTetris(10, 20, n, device=device, pieces=pieces, auto_reset=False, seed=1, feature_directions=directions)
        env.set_boards(_t(g["cells"][sel], device), _t(g["piece"][sel].astype(np.int64), device))
        nv = g["n_valid"][sel].astype(np.int64)
        assert np.array_equal(env.n_valid.cpu().numpy(), nv)
        w32 = g["weights"][sel].astype(np.float32)
        assert np.array_equal(w32.astype(np.float64), g["weights"][sel])
        action, logp, score, logz, logits = raw_softmax(env, _t(w32, device), None, temperature, Out(env)).numpy()
        feats, nv2 = afterstates(env)
        assert np.array_equal(nv2, nv)
        A = min(env.a_max, g["probs"].shape[1])
        assert nv.max() <= A
        valid = np.arange(A)[None, :] < nv[:, None]
        # the float32-versus-float64 difference of the dot product: 8 roundings of at most 2^-24 sum |f_q w_q| each
        # (eight products, seven sums), divided by the temperature
        delta = 8 * 2.0 ** -24 * np.einsum("baq,bq->ba", np.abs(feats[:, :A].astype(np.float64)), np.abs(g["weights"][sel])) / temperature
        delta = np.where(valid, delta, 0.0).max(axis=1)  # per env
        bound = TOL + delta
        probs = np.where(valid, np.exp(logits[:, :A].astype(np.float64) - logz[:, None].astype(np.float64)), 0.0)
        err_p = np.abs(probs - g["probs"][sel][:, :A]).max(axis=1)
        want_score = g["grads"][sel][np.arange(n), action]
        fmax = np.abs(np.where(valid[:, :, None], feats[:, :A].astype(np.float64), 0.0)).max(axis=1)  # [n, 8]
        err_s = (np.abs(score - want_score) / np.maximum(1.0, fmax)).max(axis=1)
        print("softmax fixture %s config %d: p error %.3g, score error %.3g, bound %.3g .. %.3g" %
              (device, ci, err_p.max(), err_s.max(), bound.min(), bound.max()))
        assert np.all(err_p <= bound), (ci, err_p, bound)
        assert np.all(err_s <= bound), (ci, err_s, bound)
        worst = max(worst, float(err_p.max()), float(err_s.max()))
    return worst


# ---- 7. determinism and sharding -----------------------------------------------------------------------------------------
def determinism_and_sharding(device, C, R, pieces):
    env = env_with_edges(device, C, R, pieces, env_offset=1000)
    Wm, rows_t = _t(weight_rows(), device), _t(random_rows(B, 7, seed=8), device)
    one = raw_softmax(env, Wm, rows_t, 1.0, Out(env))
    two = raw_softmax(env, Wm, rows_t, 1.0, Out(env))
    for a, b in zip(one.tensors(), two.tensors()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # two shards of whole tiles: a contiguous slice of the storage, with its env_offset
    cut = 128
    for lo, hi in ((0, cut), (cut, B)):
        part = Out(env, n=hi - lo)
        raw_softmax(env, Wm, rows_t[lo:hi].contiguous(), 1.0, part, cols=env.cols[lo // 64:].contiguous(),
                    meta=env.meta[lo:hi].contiguous(), env_offset=env.env_offset + lo, n=hi - lo)
        for a, b in zip(one.tensors(), part.tensors()):
            assert torch.equal(a[lo:hi].view(torch.int32), b.view(torch.int32)), (lo, hi)
    # the env index keys the draw (a hot policy, so that most envs have more than one likely placement)
    hot = raw_softmax(env, Wm, rows_t, 50.0, Out(env))
    shifted = raw_softmax(env, Wm, rows_t, 50.0, Out(env), env_offset=env.env_offset + 1)
    assert int((shifted.action != hot.action).sum()) > int((env.n_valid > 1).sum()) // 8


# ---- 8. play equals composition ------------------------------------------------------------------------------------------
def _compose(twin, K, Wm, rows_t, T):
    """K x (policy_softmax_rows, then step with those actions): float32 step-order sums over the steps an env placed"""
    n = twin.batch_size
    logp_sum, score_sum = np.zeros(n, np.float32), np.zeros((n, 8), np.float32)
    lines, placed = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for _ in range(K):
        out = raw_softmax(twin, Wm, rows_t, T, Out(twin, logz=False, logits=False))
        action, logp, score = out.action.cpu().numpy(), out.logp.cpu().numpy(), out.score.cpu().numpy()
        ln = twin.step(out.action)[3].cpu().numpy()
        alive = action >= 0
        logp_sum[alive] = logp_sum[alive] + logp[alive]
        score_sum[alive] = score_sum[alive] + score[alive]
        lines += np.where(alive, ln, 0)
        placed += alive
    return logp_sum, score_sum, lines, placed


def play_equals_composition(device, C, R, pieces, n=B, K=24, w=None, T=1.0, split=None):
    env = pc._env(device, C, R, pieces, n, seed=9)
    twin = env.fork(torch.arange(n))
    W = weight_rows() if w is None else np.tile(np.asarray(w, np.float32)[None], (7, 1))
    Wm, rows_t = _t(W, device), _t(random_rows(n, 7, seed=1), device)
    lines, pcs, logp, score = totals(env)
    n_valid, piece = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
    done_k = 0
    for k in (split or [K]):  # chunks compose: the totals carry on
        raw_play(env, k, Wm, rows_t, T, lines, pcs, logp, score, n_valid, piece, env.status, step_idx0=env.step_idx + done_k)
        done_k += k
    assert done_k == K
    want_logp, want_score, want_lines, want_placed = _compose(twin, K, Wm, rows_t, T)
    assert torch.equal(env.cols, twin.cols) and torch.equal(env.meta, twin.meta)
    assert torch.equal(n_valid, twin.n_valid) and torch.equal(piece, twin.piece)
    assert np.array_equal(lines.cpu().numpy().astype(np.int64), want_lines)
    assert np.array_equal(pcs.cpu().numpy().astype(np.int64), want_placed)
    assert np.array_equal(logp.cpu().numpy().view(np.int32), want_logp.view(np.int32))
    assert np.array_equal(score.cpu().numpy().view(np.int32), want_score.view(np.int32))
    got, want = env.status.view(-1, 4), twin.status.view(-1, 4)
    assert torch.equal(got[:, 1:], want[:, 1:])  # episodes, lines, steps
    assert int(got[:, 0].sum()) == 0             # a frozen env is not invalid (the step counts its -1 action)
    frozen = K * n - int(want_placed.sum())
    assert int(want[:, 0].sum()) == frozen
    assert int(want_placed.sum()) > 0 and np.any(want_logp != 0) and np.any(want_score != 0)
    return int(want_placed.sum()), frozen


# ---- 9. rows outside [0, P), footprints ------------------------------------------------------------------------------------
def bad_rows(device, C, R, pieces, n_steps):
    env = pc._env(device, C, R, pieces, B, seed=19)
    W = weight_rows()
    P = len(W)
    rows = random_rows(B, P, seed=3)
    bad = {5: -1, 70: P, B - 1: pc.INT32_MIN}  # wave 0, wave 1, the last lane of the partial tile
    for j, v in bad.items():
        rows[j] = v
    Wm, rows_t = _t(W, device), _t(rows, device)
    bad_idx = torch.as_tensor(sorted(bad), device=device)
    want = np.zeros(env.status.numel() // 4, np.int64)
    for j in bad:
        want[j >> 6] += 1
    good = torch.ones(B, dtype=torch.bool, device=device)
    good[bad_idx] = False
    out = raw_softmax(env, Wm, rows_t, 1.0, Out(env), env.status)
    for t in out.tensors():
        assert bool((t[bad_idx] == -7).all())  # the sentinel: no byte of those envs' outputs was written
    assert bool((out.action[good] != -7).all()) and bool((out.logp[good] != -7.0).all())
    assert bool((out.score[good] != -7.0).all()) and bool((out.logits[good] != -7.0).all())
    assert np.array_equal(env.status.view(-1, 4)[:, 0].cpu().numpy(), want)
    # the play: the env and every output untouched, counted once whatever n_steps is
    env.status.zero_()
    before = snapshot(env)
    lines, pcs = (torch.full((B,), 1000, dtype=torch.int32, device=device) for _ in range(2))
    logp = torch.full((B,), 1000.0, dtype=torch.float32, device=device)
    score = torch.full((B, 8), 1000.0, dtype=torch.float32, device=device)
    nv, pcn = torch.full_like(env.n_valid, 99), torch.full_like(env.piece, 99)
    raw_play(env, n_steps, Wm, rows_t, 1.0, lines, pcs, logp, score, nv, pcn, env.status)
    assert torch.equal(lanes(env.cols, bad_idx), lanes(before["cols"], bad_idx))
    assert torch.equal(env.meta[bad_idx], before["meta"][bad_idx])
    for t, sentinel in ((lines, 1000), (pcs, 1000), (nv, 99), (pcn, 99), (logp, 1000.0)):
        assert t[bad_idx].tolist() == [sentinel] * 3
    assert bool((score[bad_idx] == 1000.0).all())
    alive = good & (before["n_valid"] > 0)
    assert bool((pcs[alive] > 1000).all()) and bool((nv[good] != 99).all())
    assert np.array_equal(env.status.view(-1, 4)[:, 0].cpu().numpy(), want)
    with pytest.raises(IndexError):
        env.check()


SOFTMAX_ROWS_OPTIONAL = ["none", "rows", "score", "logz", "logits", "status"]
PLAY_OPTIONAL = ["none", "rows", "logp_total", "n_valid", "piece", "status"]


def footprint_softmax_rows(device, C, R, n, null_arg):
    from tetris_amd import _lib
    lib = _lib.load()
    geo, st = fc.state(lib, device, C, R, n)
    Wm, rows, bad = pc._population_inputs(n, device, null_arg == "rows")
    k4 = fc._elems(bad, 4)

    def call(A):
        opt = lambda name, nbytes, keep: A.new(name, nbytes, keep=keep) if null_arg != name else None
        A.launch(lib.policy_softmax_rows, geo.d, A.new("cols", init=st["cols"], keep=True), A.new("meta", init=st["meta"], keep=True),
                 A.new("weights", init=Wm, keep=True), Wm.shape[0], A.new("rows", init=rows, keep=True) if rows is not None else None,
                 1.0, A.new("action", 4 * n, keep=k4), A.new("logp", 4 * n, keep=k4), opt("score", 32 * n, fc._elems(bad, 32)),
                 opt("logz", 4 * n, k4), opt("logits", 4 * geo.a_max * n, fc._elems(bad, 4 * geo.a_max)),
                 A.new("status", init=st["status"]) if null_arg != "status" else None, fc.SEED, st["step_idx"], 0, n, None)

    g, _ = fc.footprint(device, call)
    if null_arg not in ("status", "rows"):
        invalid = g.bufs["status"].body.view(torch.int32).view(-1, 4)[:, 0] - st["status"].view(-1, 4)[:, 0]
        assert int(invalid.sum()) == int(bad.sum()) > 0
    action = g.bufs["action"].body.view(torch.int32)
    assert bool(((action[~bad] >= 0) & (action[~bad] < geo.a_max)).all())


def footprint_play(device, C, R, n, null_arg, K=3):
    from tetris_amd import _lib
    lib = _lib.load()
    geo, st = fc.state(lib, device, C, R, n)
    Wm, rows, bad = pc._population_inputs(n, device, null_arg == "rows")
    k1, k4 = fc._elems(bad, 1), fc._elems(bad, 4)
    start = torch.arange(n, dtype=torch.int32, device=device) + 1000
    fstart = torch.arange(n, dtype=torch.float32, device=device) + 0.5

    def call(A):
        A.launch(lib.play_softmax, geo.d, A.new("cols", init=st["cols"], keep=geo.kept_lanes(n, bad, device)),
                 A.new("meta", init=st["meta"], keep=fc._elems(bad, 8)), K, A.new("weights", init=Wm, keep=True), Wm.shape[0],
                 A.new("rows", init=rows, keep=True) if rows is not None else None, 1.0,
                 A.new("lines_total", init=start, keep=k4), A.new("pieces_total", init=start, keep=k4),
                 A.new("logp_total", init=fstart, keep=k4) if null_arg != "logp_total" else None,
                 A.new("score_total", init=fstart[:, None].expand(n, 8).contiguous(), keep=fc._elems(bad, 32)),
                 A.new("n_valid", init=st["n_valid"] + 100, keep=k1) if null_arg != "n_valid" else None,
                 A.new("piece", init=st["piece"] + 100, keep=k1) if null_arg != "piece" else None,
                 A.new("status", init=st["status"]) if null_arg != "status" else None, fc.SEED, st["step_idx"], 0, n, None)

    g, _ = fc.footprint(device, call)
    assert not torch.equal(g.bufs["meta"].body, g.bufs["meta"].before)
    placed = g.bufs["pieces_total"].body.view(torch.int32) - start
    assert int(placed[bad].abs().sum()) == 0 and bool(((placed[~bad] >= 1) & (placed[~bad] <= K)).all())
    assert int(placed.max()) == K


# ---- 11. the facade -------------------------------------------------------------------------------------------------------
def facade(device):
    from tetris_amd import VecTetris
    env = pc._env(device, 10, 20, "default", B, seed=29, steps=3)
    twin = env.fork(torch.arange(B))
    w = _t(BCTS, device)
    # sample_actions then step(action) advances the game; the shared vector is row 0 of a [1, 8] matrix
    action, logp, score = (t.clone() for t in env.sample_actions(w, temperature=4.0))
    out = raw_softmax(twin, w.reshape(1, 8), torch.zeros(B, dtype=torch.int32, device=device), 4.0, Out(twin))
    assert torch.equal(action, out.action) and torch.equal(logp.view(torch.int32), out.logp.view(torch.int32))
    assert torch.equal(score.view(torch.int32), out.score.view(torch.int32))
    assert bool((action >= 0).all()) and bool((logp <= 0).all())
    cells0 = env.boards().clone()
    env.step(action)
    assert env.step_idx == twin.step_idx + 1 and env.stats()["steps"] == B and env.stats()["invalid"] == 0
    assert bool((env.boards() != cells0).flatten(1).any(dim=1).all())
    a2, lp2, sc2, lg2 = env.sample_actions(w, temperature=4.0, logits=True)
    assert lg2.shape == (B, env.a_max) and not torch.equal(a2, action)
    assert len(env.sample_actions(w, score=False)) == 2
    # play_sampled: totals consistent with stats(); afterstates afterwards describe the new boards
    Wm, rows = _t(weight_rows(), device), _t(random_rows(B, 7, seed=4), device)
    s0, idx0 = env.stats(), env.step_idx
    feats_before = env.get_after_states()[0].clone()
    res = env.play_sampled(Wm, rows=rows, temperature=2.0, max_steps=20, chunk=8)
    assert env.step_idx == idx0 + 20
    s1 = env.stats()
    assert s1["steps"] - s0["steps"] == int(res["pieces"].cpu().numpy().astype(np.int64).sum()) > 0
    assert s1["lines"] - s0["lines"] == int(res["lines"].cpu().numpy().astype(np.int64).sum())
    assert s1["episodes"] - s0["episodes"] == int(res["done"].sum()) and s1["invalid"] == 0
    assert res["logp_total"].shape == (B,) and res["score_total"].shape == (B, 8) and res["done"].dtype == torch.bool
    assert bool((res["logp_total"] <= 0).all()) and bool(torch.isfinite(res["score_total"]).all())
    assert torch.equal(res["done"], env.n_valid == 0)
    feats, nv = env.get_after_states()
    fresh = VecTetris(10, 20, B, device=device, auto_reset=False, seed=1)
    fresh.set_boards(env.boards(), env.piece)
    want_feats, want_nv = fresh.get_after_states()
    assert torch.equal(feats.view(torch.int32), want_feats.view(torch.int32)) and torch.equal(nv, want_nv)
    assert torch.equal(nv, env.n_valid) and not torch.equal(feats, feats_before)
    env.check()
    # every game ends under the negated weights: play_sampled stops after whole chunks
    small = VecTetris(6, 10, B, device=device, auto_reset=True, seed=23)
    res = small.play_sampled(_t(-BCTS, device), temperature=1.0, max_steps=4096, chunk=8)
    assert bool(res["done"].all()) and 8 <= small.step_idx < 4096 and small.step_idx % 8 == 0
    assert small.stats()["episodes"] == B
    # refusals of the host
    replay = VecTetris(10, 20, B, device=device, piece_stream=np.zeros((8, B), dtype=np.uint8))
    with pytest.raises(ValueError, match="replay"):
        replay.play_sampled(w)
    for bad_t in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            env.sample_actions(w, temperature=bad_t)
        with pytest.raises(ValueError, match="temperature"):
            env.play_sampled(w, temperature=bad_t)
    for bad_w in (Wm[:, :7], w[:7], BCTS.tolist()):
        with pytest.raises(ValueError):
            env.sample_actions(bad_w)
    with pytest.raises(ValueError):
        env.sample_actions(w, rows=rows)  # a shared vector takes no rows
    with pytest.raises(ValueError):
        env.sample_actions(Wm)  # no rows: needs a row per env

#!/usr/bin/env python3
"""Generate tests/golden/g11_softmax.npz from the LIVE reference (authoring container only, as make_golden.py,
whose import recipe this uses):

    python tests/golden/make_golden_softmax.py

Two dozen states of seeded reference games at 10x20 -- the default pair and standard7, each with and without
feature_directions -- and, for each, what utils.compute_action_probabilities and
utils.grad_of_log_action_probabilities return on the matrix get_after_states() hands them.  Data only:
  cells [N, 24, 10] int8, piece [N] int8 (list index), config [N] int8 (index into CONFIGS below),
  weights [N, 8] float64 holding float32 values, temperature [N] float64,
  n_valid [N] int8, probs [N, A] float64 (zero past n_valid), grads [N, A, 8] float64 (row a = the gradient
  for action a).
"""
import os

import numpy as np

import make_golden as mg

HERE = os.path.dirname(os.path.abspath(__file__))
A = 40
DIRECTIONS = [-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, 1.0, -1.0]
# (piece list or None = the default pair, feature_directions, temperature); tests/test_softmax_*.py mirror this
CONFIGS = [(None, None, 1.0), (mg.STANDARD7, None, 0.5), (None, DIRECTIONS, 20.0), (mg.STANDARD7, DIRECTIONS, 2.0)]
STEPS = [4, 11, 19]   # states recorded after this many random steps of a game
SEEDS = [0, 1]


def main():
    game, _, tetromino = mg.import_reference()
    from tetris import utils
    rec = {k: [] for k in ("cells", "piece", "config", "weights", "temperature", "n_valid", "probs", "grads")}
    wrng = np.random.RandomState(11)
    for ci, (pieces, directions, temperature) in enumerate(CONFIGS):
        for seed in SEEDS:
            env = mg.make_env(game, tetromino, 10, 20, pieces, seed, feature_directions=directions)
            arng = np.random.default_rng(20_000 + seed)
            for t in range(max(STEPS) + 1):
                feats = np.asarray(env.get_after_states()[0])
                n = feats.shape[0]
                assert n > 0
                if t in STEPS:
                    w = (wrng.randn(8) * 8).astype(np.float32).astype(np.float64)
                    if t == STEPS[0]:
                        w = np.asarray([-24.04, -19.77, -13.08, -12.63, -10.49, -9.22, 6.6, -1.61], np.float32).astype(np.float64)
                        if directions is not None:  # the reference's weights are positive on directed features
                            w = w * np.asarray(directions)
                    p = utils.compute_action_probabilities(feats.astype(np.float64), w, temperature)
                    probs, grads = np.zeros(A), np.zeros((A, 8))
                    probs[:n] = p
                    for a in range(n):
                        grads[a] = utils.grad_of_log_action_probabilities(feats.astype(np.float64), p, a)
                    rec["cells"].append(np.asarray(env.current_state.representation).astype(np.int8))
                    rec["piece"].append(env.tetrominos.index(env.current_tetromino))
                    rec["config"].append(ci)
                    rec["weights"].append(w)
                    rec["temperature"].append(temperature)
                    rec["n_valid"].append(n)
                    rec["probs"].append(probs)
                    rec["grads"].append(grads)
                _, _, done, _ = env.step(int(arng.integers(n)))
                assert not done
    out = dict(cells=np.asarray(rec["cells"], np.int8), piece=np.asarray(rec["piece"], np.int8),
               config=np.asarray(rec["config"], np.int8), weights=np.asarray(rec["weights"], np.float64),
               temperature=np.asarray(rec["temperature"], np.float64), n_valid=np.asarray(rec["n_valid"], np.int8),
               probs=np.asarray(rec["probs"], np.float64), grads=np.asarray(rec["grads"], np.float64))
    assert out["cells"].shape == (len(CONFIGS) * len(SEEDS) * len(STEPS), 24, 10)
    assert np.array_equal(out["weights"], out["weights"].astype(np.float32).astype(np.float64))
    np.savez_compressed(os.path.join(HERE, "g11_softmax.npz"), **out)
    print("g11_softmax.npz: %d states, n_valid %s" % (len(out["piece"]), out["n_valid"].tolist()))


if __name__ == "__main__":
    main()

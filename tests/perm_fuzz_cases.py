"""The drawn cases of the permutation tests' sweep (tests/test_gpu_fuzz_perm_tests.py), in the style of stat_fuzz_cases.py: a case
is one call of several groups with its test, alternative, permutations, seed and small-path cap all drawn.  ANOFOX_FUZZ_SCALE
multiplies the number of calls; the default is a few hundred groups."""
import os

import numpy as np

import perm_test_restate as R

SCALE = max(1, int(os.environ.get("ANOFOX_FUZZ_SCALE", "1")))
CALLS = 12 * SCALE
PERMUTATIONS = (0, 1, 37, 64, 100, 129, 300)
CAPS = (0, 7, 16, 64, 300)   # 0: the library's cap


def draw_case(index):
    """-> dict(test, alternative, n_perm, seed, cap, sigma, groups: a list of (v, sample))."""
    rng = np.random.default_rng(90210 + index)
    test = int(rng.integers(0, 3))
    groups = []
    for _ in range(int(rng.integers(15, 30))):
        kind = rng.random()
        top = 120 if test == R.MMD else 400
        n = int(rng.integers(4, 12)) if kind < 0.3 else int(rng.integers(4, top))
        g = R.make_group(rng, n, ties=float(rng.choice([0.0, 0.0, 0.5, 0.9])), nan_share=float(rng.choice([0.0, 0.0, 0.1, 0.4])),
                         shift=float(rng.choice([0.0, 0.3, 1.0])))
        if kind > 0.93:      # one-sided, or with an infinity
            g = (g[0], np.zeros_like(g[1])) if rng.random() < 0.5 else (np.where(np.arange(len(g[0])) == 1, np.inf, g[0]), g[1])
        groups.append(g)
    return dict(test=test, alternative=int(rng.integers(0, 3)) if test == R.T_TEST else 0, n_perm=int(rng.choice(PERMUTATIONS)),
                seed=int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)), cap=int(rng.choice(CAPS)),
                sigma=float(rng.choice([np.nan, np.nan, 0.7])) if test == R.MMD else float("nan"), groups=groups)

"""The inputs of the quantile glue tests (tests/test_gpu_quantile_glue.py) and what the test driver does with them, in numpy
alone, so that tests/test_quantile_glue_cpu.py can check without a GPU that the fixed seeds give every fitted group a unique
optimum (Gaussian X and noise: generically they do; the restatement's certificate decides it for these seeds).

Seeds: GROUP BY p = 3: 20260101, p = 32: 20260102, window: 20260103."""
import numpy as np

import quantile_restate as Q

SPLIT_STRINGS = [None, "train", "Training", "test", "TRAIN", "a-validation-partition-name", "training"]   # quantile_family_capi.cpp
SPLIT_WEIGHTS = [0.05, 0.2, 0.15, 0.1, 0.15, 0.1, 0.25]       # every spelling and NULL occur; three rows in four train
SEED_GROUP_BY, SEED_WIDE, SEED_WINDOW = 20260101, 20260102, 20260103
N_THREADS, VECTOR_SIZE = 4, 64
ONE_ROW_GROUP, NAN_Y_GROUP = 2, 5
PATH_TAUS = [0.9, 0.1, 0.5, 0.5, 1.2]
WINDOW_PRECEDING, TREE_LEAF, TREE_BACK = 12, 8, 2


def group_by_case(wide=False):
    """K groups with shuffled keys; about 10 % NULL y.  Not wide (p = 3, K = 24 groups of 10-40 rows): group ONE_ROW_GROUP has
    exactly one row (it trains), group NAN_Y_GROUP has one row whose y is NaN and not NULL, and every row has a split code."""
    rng = np.random.default_rng(SEED_WIDE if wide else SEED_GROUP_BY)
    K, p, lo, hi = (6, 32, 40, 81) if wide else (24, 3, 10, 41)
    sizes = rng.integers(lo, hi, size=K)
    if not wide:
        sizes[ONE_ROW_GROUP] = 1
    key = np.repeat(np.arange(K), sizes).astype(np.uint32)
    rng.shuffle(key)
    n = len(key)
    X = rng.normal(size=(n, p))
    y = X @ rng.normal(size=p) + 0.7 + rng.normal(size=n)
    y_null = (rng.random(n) < 0.1).astype(np.uint8)
    split = rng.choice(len(SPLIT_STRINGS), size=n, p=SPLIT_WEIGHTS).astype(np.uint8)
    nan_row = -1
    if not wide:
        one = int(np.nonzero(key == ONE_ROW_GROUP)[0][0])
        y_null[one], split[one] = 0, 1
        nan_row = int(np.nonzero(key == NAN_Y_GROUP)[0][3])
        y[nan_row], y_null[nan_row], split[nan_row] = np.nan, 0, 4
    return dict(K=K, p=p, n=n, key=key, X=np.ascontiguousarray(X), y=y, y_null=y_null, split=split, nan_row=nan_row)


def training_mask(case, with_split):
    """The rows the glue flags is_training: y not NULL and, with a split column, a split value that says train."""
    train = case["y_null"] == 0
    if with_split:
        train = train & np.array([SPLIT_STRINGS[c] is not None and SPLIT_STRINGS[c].lower() in ("train", "training") for c in case["split"]])
    return train


def driver_order(key, n_keys, n_threads=N_THREADS, vector_size=VECTOR_SIZE):
    """Output order of a group's rows: thread by thread, within a thread in input order (vector v goes to thread v % n_threads,
    Combine appends thread t's rows after those of the threads before it)."""
    n = len(key)
    thread = (np.arange(n) // vector_size) % n_threads
    return [np.concatenate([np.nonzero((key == g) & (thread == t))[0] for t in range(n_threads)]) for g in range(n_keys)]


def group_batch(case, with_split):
    """What the glue hands the ABI: per group in key order its rows in driver order with y = NaN where the row does not train;
    groups with fewer than 2 training rows are left out.  -> (groups, order, offsets, y_fit, X, train_counts)"""
    train = training_mask(case, with_split)
    order = driver_order(case["key"], case["K"])
    groups = [g for g in range(case["K"]) if int(train[order[g]].sum()) >= 2]
    idx = np.concatenate([order[g] for g in groups])
    offsets = np.concatenate([[0], np.cumsum([len(order[g]) for g in groups])]).astype(np.int64)
    y_fit = np.where(train[idx], case["y"][idx], np.nan)
    counts = np.array([int(train[order[g]].sum()) for g in groups], dtype=np.int64)
    return groups, order, offsets, y_fit, np.ascontiguousarray(case["X"][idx]), counts


def window_case():
    """One partition of 120 rows, p = 2; some NULL y, the current row's among them."""
    rng = np.random.default_rng(SEED_WINDOW)
    n, p = 120, 2
    X = rng.normal(size=(n, p))
    y = X @ [0.7, -1.2] + 0.5 + rng.normal(size=n)
    y_null = (rng.random(n) < 0.1).astype(np.uint8)
    y_null[0], y_null[40] = 0, 1
    return dict(n=n, p=p, X=np.ascontiguousarray(X), y=y, y_null=y_null)


def window_frames(case, tree):
    """[(lo, hi, current)]: the frame's rows [lo, hi) and the row whose x is predicted — ROWS BETWEEN 12 PRECEDING AND CURRENT
    ROW per row, or per leaf of TREE_LEAF rows the leaves [o - TREE_BACK, o] with the last row of the frame as current."""
    n = case["n"]
    if not tree:
        return [(max(0, o - WINDOW_PRECEDING), o + 1, o) for o in range(n)]
    n_leaves = (n + TREE_LEAF - 1) // TREE_LEAF
    return [(max(0, o - TREE_BACK) * TREE_LEAF, min(n, (o + 1) * TREE_LEAF), min(n, (o + 1) * TREE_LEAF) - 1) for o in range(n_leaves)]


def restated_fit(X, y_fit, tau, fit_intercept):
    """The restatement's fit of one group with its certificate: -> (beta over the design's columns, unique and certified)."""
    res = Q.solve(X, y_fit, tau, fit_intercept)
    cert = Q.certify(X, y_fit, tau, fit_intercept, res["b"], res["b0"])
    beta = np.concatenate([[res["b0"]], res["b"]]) if fit_intercept else np.asarray(res["b"])
    return beta, bool(res["unique"] and cert["decided"] and cert["optimal"] and cert["strict"])


def restated_status(X, y_fit, tau, fit_intercept, n_training):
    return Q.rule_status(X, y_fit, tau, fit_intercept, rule_count=n_training)


AGG, PATH, WINDOW = 0, 1, 2
NAME, ALIAS = "anofox_stats_quantile_fit_predict_agg", "quantile_fit_predict_agg"
# (function, options spec, as a MAP, split column, tau, fit_intercept): the four overloads under both names
AGG_RUNS = [
    (NAME, None, False, False, 0.5, True),
    (ALIAS, None, False, False, 0.5, True),
    (NAME, "tau=0.1", False, False, 0.1, True),
    (ALIAS, "tau=0.5;fit_intercept=false", True, False, 0.5, False),
    (NAME, None, False, True, 0.5, True),
    (ALIAS, None, False, True, 0.5, True),
    (NAME, "tau=0.1;intercept=false", False, True, 0.1, False),
    (ALIAS, "TAU=0.1", True, True, 0.1, True),
    (ALIAS, "quantile=0.9", False, False, 0.5, True),          # the reference's example key: ignored
]
PATH_RUNS = [
    ("anofox_stats_quantile_path_fit_predict_agg", "taus=[0.9,0.1,0.5,0.5,1.2]", True, False, True),
    ("quantile_path_fit_predict_agg", "fit_intercept=false;taus=[0.9,0.1,0.5,0.5,1.2]", False, True, False),
]
WINDOW_RUNS = [
    ("anofox_stats_quantile_fit_predict", None, 0.5, True),
    ("quantile_fit_predict", "tau=0.8;max_iter=500", 0.8, True),
]

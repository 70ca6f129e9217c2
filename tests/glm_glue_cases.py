"""The inputs of the GLM glue tests (tests/test_gpu_glm_glue.py) and what the test driver does with them, in numpy alone, so that
tests/test_glm_glue_cpu.py can certify without a GPU that with these fixed seeds every group the row rules let through and the
restatement fits is inside glm_cases.in_conditions (not separated, within the kappa bound, |eta| <= 20).

Seeds: GROUP BY p = 3: 20260301, p = 32: 20260302.  x is uniform in [-1, 1], sum |b| <= 1.8, |intercept| <= 0.5: |eta| <= 2.3 at the
truth.  The same rows carry a Poisson response (means around e) and a 0 / 1 response."""
import numpy as np

import glm_cases as GC
import glm_restate as R

SPLIT_STRINGS = [None, "train", "Training", "test", "TRAIN", "a-validation-partition-name", "training"]   # glm_family_capi.cpp
SPLIT_WEIGHTS = [0.05, 0.2, 0.15, 0.1, 0.15, 0.1, 0.25]       # every spelling and NULL occur; three rows in four train
SEED_GROUP_BY, SEED_WIDE = 20260301, 20260302
N_THREADS, VECTOR_SIZE = 4, 64
ONE_ROW_GROUP, NEGATIVE_Y_GROUP, NULL_ELEMENT_GROUP, NAN_Y_GROUP = 2, 7, 4, 5
POISSON, BINOMIAL = R.POISSON, R.BINOMIAL


def group_by_case(wide=False):
    """K groups with shuffled keys, about 10 % NULL y and 3 % NULL x lists.  Not wide (p = 3, K = 24 groups of 40-130 rows): group
    ONE_ROW_GROUP has exactly one row, NEGATIVE_Y_GROUP a y = -1 (outside both supports: status 1, a NULL group), NULL_ELEMENT_GROUP
    a row whose second x element is NULL, NAN_Y_GROUP a row whose y is NaN and not NULL; every row has a split code.  Wide: p = 32,
    3 groups of at least 12 * 33 rows."""
    rng = np.random.default_rng(SEED_WIDE if wide else SEED_GROUP_BY)
    K, p, lo, hi = (3, 32, 12 * 33 + 4, 12 * 33 + 40) if wide else (24, 3, 40, 131)
    sizes = rng.integers(lo, hi, size=K)
    if not wide:
        sizes[ONE_ROW_GROUP] = 1
    key = np.repeat(np.arange(K), sizes).astype(np.uint32)
    rng.shuffle(key)
    n = len(key)
    X = rng.uniform(-1.0, 1.0, size=(n, p))
    B = rng.normal(size=(K, p))
    B *= (rng.uniform(0.3, 1.8, size=K) / np.abs(B).sum(axis=1))[:, None]
    eta = np.einsum("ij,ij->i", X, B[key]) + rng.uniform(-0.5, 0.5, size=K)[key]
    y = {POISSON: rng.poisson(np.exp(eta + 1.0)).astype(float), BINOMIAL: (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)}
    y_null = (rng.random(n) < 0.1).astype(np.uint8)
    x_null = (rng.random(n) < 0.03).astype(np.uint8)
    xe_null = np.zeros((n, p), dtype=np.uint8)
    split = rng.choice(len(SPLIT_STRINGS), size=n, p=SPLIT_WEIGHTS).astype(np.uint8)
    null_row = nan_row = -1
    if not wide:
        def row_of(g, k):
            return int(np.nonzero(key == g)[0][k])
        one = row_of(ONE_ROW_GROUP, 0)
        y_null[one], x_null[one], split[one] = 0, 0, 1
        neg = row_of(NEGATIVE_Y_GROUP, 5)
        y[POISSON][neg] = y[BINOMIAL][neg] = -1.0
        y_null[neg], x_null[neg], split[neg] = 0, 0, 1
        null_row = row_of(NULL_ELEMENT_GROUP, 6)
        xe_null[null_row, 1], x_null[null_row], y_null[null_row], split[null_row] = 1, 0, 0, 1
        nan_row = row_of(NAN_Y_GROUP, 3)
        y[POISSON][nan_row] = y[BINOMIAL][nan_row] = np.nan
        y_null[nan_row], x_null[nan_row], split[nan_row] = 0, 0, 4
    return dict(K=K, p=p, n=n, key=key, X=np.ascontiguousarray(X), y=y, y_null=y_null, x_null=x_null, xe_null=np.ascontiguousarray(xe_null),
                split=split, null_row=null_row, nan_row=nan_row)


_CASES = {}


def case(wide=False):
    if wide not in _CASES:
        _CASES[wide] = group_by_case(wide)
    return _CASES[wide]


def driver_order(key, n_keys, n_threads=N_THREADS, vector_size=VECTOR_SIZE):
    """Output order of a group's rows: thread by thread, within a thread in input order (vector v goes to thread v % n_threads,
    Combine appends thread t's rows after those of the threads before it)."""
    thread = (np.arange(len(key)) // vector_size) % n_threads
    return [np.concatenate([np.nonzero((key == g) & (thread == t))[0] for t in range(n_threads)]) for g in range(n_keys)]


def training_mask(c, with_split):
    """The rows fit-predict flags is_training: y not NULL and, with a split column, a split value that says train."""
    train = c["y_null"] == 0
    if with_split:
        train = train & np.array([SPLIT_STRINGS[s] is not None and SPLIT_STRINGS[s].lower() in ("train", "training") for s in c["split"]])
    return train


# One run: the function (name or alias), the options spec of the test driver, MAP or STRUCT, the split column, and what the options
# resolve to.  kind: "poisson" / "binomial" / "logistic" fit aggregates, "predict" = poisson_fit_predict_agg.
def _run(fn, spec, as_map, kind, split=False, icpt=True, lam=0.0, inference=False, offset=0, threshold=0.5, z=1.96):
    return dict(fn=fn, spec=spec, as_map=as_map, kind=kind, split=split, icpt=icpt, lam=lam, inference=inference, offset=offset,
                threshold=threshold, z=z, family=BINOMIAL if kind in ("binomial", "logistic") else POISSON)


RUNS = [
    _run("anofox_stats_poisson_fit_agg", None, False, "poisson"),
    _run("poisson_fit_agg", "compute_inference=true;glm_lambda=0.5", True, "poisson", lam=0.5, inference=True),
    _run("poisson_fit_agg", "offset=3;Inference=true;link=log;full_output=1", False, "poisson", inference=True, offset=3),
    _run("anofox_stats_binomial_fit_agg", "intercept=false;binomial_link=logit", False, "binomial", icpt=False),
    _run("binomial_fit_agg", "inference=1;offset=1", True, "binomial", inference=True, offset=1),
    _run("anofox_stats_logistic_fit_agg", None, False, "logistic"),
    _run("logistic_fit_agg", "threshold=0.4;glm_lambda=0.5;compute_inference=true", True, "logistic", lam=0.5, inference=True, threshold=0.4),
    _run("logistic_fit_agg", "offset=2;threshold=0.6", False, "logistic", offset=2, threshold=0.6),
    _run("anofox_stats_poisson_fit_predict_agg", None, False, "predict"),
    _run("poisson_fit_predict_agg", "confidence_level=0.99;glm_lambda=0.5;offset=2;compute_inference=true", False, "predict", lam=0.5, z=2.576),
    _run("poisson_fit_predict_agg", None, False, "predict", split=True),
    _run("anofox_stats_poisson_fit_predict_agg", "confidence=0.9;fit_intercept=0", True, "predict", split=True, icpt=False, z=1.645),
]
WIDE_RUN = _run("poisson_fit_agg", "compute_inference=true", False, "poisson", inference=True)


def run_id(r):
    return "%s-%s-%s%s" % (r["fn"], r["spec"], "map" if r["as_map"] else "struct", "-split" if r["split"] else "")


def group_batch(c, run):
    """What the glue hands the ABI for a run: per group in key order its buffered rows in driver order, the groups the row rules
    turn down left out.  -> dict(groups, rows (per kept group: indices into the case), offsets, y (NaN where the row does not
    train), cols (the features), off (the offset column or None), counts (fit-predict's train_counts), train (mask over the case))"""
    predict = run["kind"] == "predict"
    y = c["y"][run["family"]]
    train = training_mask(c, run["split"])
    buffered = (c["x_null"] == 0) & (predict | (c["y_null"] == 0))
    order = [o[buffered[o]] for o in driver_order(c["key"], c["K"])]
    groups = [g for g in range(c["K"]) if (int(train[order[g]].sum()) if predict else len(order[g])) >= 2]
    idx = np.concatenate([order[g] for g in groups])
    offsets = np.concatenate([[0], np.cumsum([len(order[g]) for g in groups])]).astype(np.int64)
    X = np.where(c["xe_null"][idx] == 1, np.nan, c["X"][idx])
    feat = [j for j in range(c["p"]) if j != run["offset"] - 1] if not predict else list(range(c["p"]))
    off = np.ascontiguousarray(X[:, run["offset"] - 1]) if run["offset"] and not predict else None
    return dict(groups=groups, rows=[order[g] for g in groups], offsets=offsets, y=np.where(train[idx], y[idx], np.nan),
                cols=[np.ascontiguousarray(X[:, j]) for j in feat], off=off,
                counts=np.array([int(train[order[g]].sum()) for g in groups], dtype=np.int64), train=train)


_REFS = {}


def restated(wide, run):
    """The restatement of every group of group_batch(case(wide), run), computed once per distinct fit."""
    predict = run["kind"] == "predict"
    key = (wide, run["family"], run["icpt"], run["lam"], 0 if predict else run["offset"], predict, run["split"])
    if key not in _REFS:
        b = group_batch(case(wide), run)
        X = np.column_stack(b["cols"])
        o = b["offsets"]
        _REFS[key] = [R.fit(run["family"], b["y"][o[i]:o[i + 1]], X[o[i]:o[i + 1]], None if b["off"] is None else b["off"][o[i]:o[i + 1]],
                            run["icpt"], run["lam"]) for i in range(len(b["groups"]))]
    return _REFS[key]


def in_conditions(ref, q):
    return GC.in_conditions(ref, q)

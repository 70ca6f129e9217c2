"""Seeded cases of the GLM window function (csrc/glm_irls.h gi_fit_window, csrc/glm_window.hip), shared by the CPU tier
(tests/tools/glm_window_host.cpp) and the GPU tier.  A plain module: the reference of every frame is tests/glm_restate.py::fit on
the frame's rows, computed once per case; the arrays of a case are read-only.

A CASE is one call: a family, k = p + [intercept] from WIDTHS (1, 2, 9 = the edge of entry class EM = 1, 10 = the first of EM = 4,
21 = its edge, 22, 33 = EM = 10 with p = 32 and an intercept), lambda in {0, 0.5}, the offset on or off, and one frame spec.
  partitions   0, 1, 2, k - 1, k and k + 1 rows, then a long one of max(200 .. 300, 12 k + 40) rows and, for k <= 10, a second one;
  frames       ROWS (30, 0), (UNBOUNDED, 0), (2, -2), (5, 1), (UNBOUNDED, -UNBOUNDED) and the widths 63, 64, 65 and 129 rows
               ((62, 0) .. (128, 0): the 64-row Gram tile and its neighbours), dealt over the widths (SPECS) so that every width meets two
               specs per family and every spec at least two widths; EXPLICIT cases hold monotone overlapping, non-monotone, disjoint and
               empty frames (also with hi < lo and bounds outside the rows);
  patterns     in the first long partition: rows with a NaN / inf y or x that enter and leave the frames; a column that is
               constant over a stretch of rows, so that it is dropped in the frames inside the stretch only; a stretch of
               all-ones (binomial) / all-zero (Poisson) outcomes; and, where the frames start at a bounded distance, one y outside
               the support (with UNBOUNDED PRECEDING every later frame of the partition would hold it).
True coefficients keep |eta| <= 3.3: x in [-1, 1], sum |b| <= 2.2, |intercept| <= 0.8, |offset| <= 0.3.

What is compared: tests/glm_cases.py::check_record's rules and bounds per frame (status, NaN pattern, n_observations; inside the
input conditions the values), with the window's own rule first: fewer than 2 rows with a non-NaN y is status 100.  A frame that
lies wholly inside the all-ones / all-zero stretch is `degenerate` (glm_cases' kind): it has no finite optimum, keeps only its
NaN pattern and is left out of the pooled share of frames outside the input conditions, as glm_cases leaves that kind out."""
import numpy as np

import glm_cases as GC
import glm_fuzz_cases as FC
import glm_restate as R

POISSON, BINOMIAL = R.POISSON, R.BINOMIAL
WIDTHS = (1, 2, 9, 10, 21, 22, 33)
FRAMES = ((30, 0), (None, 0), (2, -2), (5, 1), (None, None), (62, 0), (63, 0), (64, 0), (128, 0))
TOO_FEW = 100
OUTSIDE_CAP = 0.05


# the two frame specs of every width, per family: a spec meets the widths whose k its rows can carry
SPECS = {POISSON: {1: ((30, 0), (2, -2)), 2: ((5, 1), (None, 0)), 9: ((30, 0), (62, 0)), 10: ((63, 0), (None, None)),
                   21: ((64, 0), (None, 0)), 22: ((128, 0), (None, None)), 33: ((None, 0), (128, 0))},
         BINOMIAL: {1: ((5, 1), (62, 0)), 2: ((2, -2), (30, 0)), 9: ((63, 0), (None, 0)), 10: ((64, 0), (30, 0)),
                    21: ((128, 0), (None, None)), 22: ((None, 0), (62, 0)), 33: ((None, None), (128, 0))}}


def calls():
    """(family, k, frame, seed) of every ROWS case: 14 family x width combinations with two frame specs each."""
    out = []
    for family in (POISSON, BINOMIAL):
        for k in WIDTHS:
            for f in SPECS[family][k]:
                out.append((family, k, f, 4000 + len(out)))   # (a seed of its own: the references are cached by it)
    return out


def frame_rows_max(c):
    """The rows of a full frame of a ROWS case (None: the partition)."""
    start, end = c[2]
    return None if start is None or end is None else start - end + 1


def case_id(c):
    family, k, f, seed = c
    name = "explicit" if f == "explicit" else "%s_%s" % tuple("unb" if v is None else v for v in f)
    return "%s-k%d-%s" % ("poisson" if family == POISSON else "binomial", k, name)


EXPLICIT = ((POISSON, 2, "explicit", 4100), (BINOMIAL, 10, "explicit", 4101))


def rows_frames(off, start, end):
    """ROWS BETWEEN start PRECEDING AND end PRECEDING per row, clipped to the partition (None: UNBOUNDED); an empty frame is
    (r, r).  -> (lo, hi) int64."""
    n = int(off[-1])
    lo, hi = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for g in range(len(off) - 1):
        plo, phi = int(off[g]), int(off[g + 1])
        for r in range(plo, phi):
            first = plo if start is None else max(r - start, plo)
            last = phi - 1 if end is None else min(r - end, phi - 1)
            lo[r], hi[r] = (r, r) if last < first else (first, last + 1)
    return lo, hi


def _draw(rng, family, n, p, icpt, with_offset):
    x = rng.uniform(-1.0, 1.0, size=(n, p))
    b = rng.normal(size=p)
    b *= rng.uniform(0.3, 2.2) / max(np.sum(np.abs(b)), 1e-9)
    b0 = (rng.uniform(0.2, 0.8) if family == POISSON else rng.uniform(-0.5, 0.5)) if icpt else 0.0
    o = rng.uniform(-0.3, 0.3, size=n) if with_offset else np.zeros(n)
    eta = x @ b + b0 + o
    assert n == 0 or np.max(np.abs(eta)) <= 3.3
    if family == POISSON:
        y = rng.poisson(np.exp(eta)).astype(float)
    else:
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    return y, x, o


_CASES = {}


def make(c):
    """-> dict(family, p, icpt, lam, offsets, y, x [N, p], off (or None), lo, hi, degenerate (bool per output row), seed)."""
    if c in _CASES:
        return _CASES[c]
    family, k, frame, seed = c
    rng = np.random.default_rng([20261019, seed])
    icpt = bool(rng.integers(0, 2))
    if not 1 <= k - icpt <= 32:
        icpt = not icpt
    p = k - icpt
    lam = 0.5 if (seed >> 1) % 2 else 0.0
    with_offset = bool((seed >> 2) & 1)
    bounded = frame != "explicit" and frame[0] is not None
    ys, xs, offs = [], [], []
    stretch = None
    if frame == "explicit":
        sizes = [320]
    else:
        big = max(200 + int(rng.integers(0, 101)), 12 * k + 40)
        sizes = [0, 1, 2, k - 1, k, k + 1, big] + ([200 + int(rng.integers(0, 101))] if k <= 10 else [])
    for g, n in enumerate(sizes):
        y, x, o = _draw(rng, family, n, p, icpt, with_offset)
        if frame != "explicit" and g == 6:   # the patterns of the first long partition
            a = int(0.12 * n)
            y[a] = np.nan
            x[a + 1, 0] = np.nan
            y[a + 2] = np.inf
            x[a + 3, p - 1] = -np.inf
            if with_offset:
                o[a + 4] = np.nan
            x[int(0.2 * n):int(0.45 * n), p // 2] = 0.75
            if bounded:
                y[int(0.55 * n)] = -1.0 if family == POISSON else 1.5
            s0, s1 = int(0.62 * n), int(0.85 * n)
            y[s0:s1] = 0.0 if family == POISSON else 1.0
            stretch = (sum(sizes[:g]) + s0, sum(sizes[:g]) + s1)
        ys.append(y)
        xs.append(x)
        offs.append(o)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(offsets[-1])
    if frame == "explicit":
        lo, hi = np.empty(N, np.int64), np.empty(N, np.int64)
        w = max(12 * k + 4, 40)
        for e in range(N):
            if e == 0:
                lo[e], hi[e] = 0, w
            elif e < 120:    # monotone, overlapping, both bounds creeping forward by 0 .. 2 rows
                lo[e] = lo[e - 1] + int(rng.integers(0, 3))
                hi[e] = min(max(hi[e - 1] + int(rng.integers(0, 3)), lo[e] + w), N)
            elif e < 200:    # non-monotone: anywhere
                lo[e] = int(rng.integers(0, N - w))
                hi[e] = min(lo[e] + w + int(rng.integers(0, 20)), N)
            elif e < 260:    # disjoint blocks of w rows, each repeated for a few rows
                b = ((e - 200) // 4) * w % (N - w)
                lo[e], hi[e] = b, b + w
            else:            # empty: hi == lo, hi < lo, bounds outside the rows
                lo[e], hi[e] = ((e, e), (e, e - 3), (N + 5, N + 5), (-4, -9))[e % 4]
        y = ys[0]
        y[7] = np.nan
        xs[0][9, 0] = np.inf
    else:
        lo, hi = rows_frames(offsets, *frame)
    deg = np.zeros(N, dtype=bool)
    if stretch is not None:
        deg = (hi > lo) & (lo >= stretch[0]) & (hi <= stretch[1])
    out = dict(family=family, p=p, icpt=icpt, lam=lam, offsets=offsets, y=np.concatenate(ys), x=np.vstack(xs),
               off=np.concatenate(offs) if with_offset else None, lo=lo, hi=hi, degenerate=deg, seed=seed, frame=frame)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[c] = out
    return out


_REF = {}


def frame_rows(case, e):
    lo, hi = int(case["lo"][e]), int(case["hi"][e])
    return slice(lo, hi) if hi > lo else slice(0, 0)


def reference(case):
    """The restatement of every frame (identical frames share one fit), with the window's rule: fewer than 2 rows with a non-NaN
    y -> status TOO_FEW.  mu_all holds the LAST row's mu only, what the window predicts."""
    key = case["seed"]
    if key in _REF:
        return _REF[key]
    memo, out = {}, []
    for e in range(len(case["lo"])):
        s = frame_rows(case, e)
        if (s.start, s.stop) not in memo:
            y = case["y"][s]
            if int(np.sum(~np.isnan(y))) < 2:
                ref = dict(status=TOO_FEW, separated=False, kappa=np.inf, max_abs_eta=np.nan, mu_all=np.full(1, np.nan))
            else:
                ref = dict(R.fit(case["family"], y, case["x"][s], None if case["off"] is None else case["off"][s], case["icpt"], case["lam"]))
                ref["mu_all"] = ref["mu_all"][-1:]
            memo[(s.start, s.stop)] = ref
        out.append(memo[(s.start, s.stop)])
    _REF[key] = out
    return out


def whole_runs(case):
    """One run per non-empty partition."""
    o = case["offsets"]
    return np.array(sorted(set(int(v) for v in o)), dtype=np.int64)


def cut_runs(case, run_length):
    """Runs of exactly run_length rows inside every partition (the test hook's rule)."""
    o, out = case["offsets"], []
    for g in range(len(o) - 1):
        out += list(range(int(o[g]), int(o[g + 1]), run_length))
    return np.array(out + [int(o[-1])], dtype=np.int64)


def host_input(case, tolerance, warm, runs, check_plain=False, interval_z=0.0, max_iterations=100):
    """The bytes tests/tools/glm_window_host.cpp reads."""
    N, p = len(case["y"]), case["p"]
    head = [case["family"], case["icpt"], max_iterations, tolerance, case["lam"], p, N, case["off"] is not None, warm, interval_z,
            check_plain, len(runs) - 1]
    cols = [case["y"][:, None], case["x"]] + ([case["off"][:, None]] if case["off"] is not None else [])
    return np.concatenate([np.array(head, float), runs.astype(float), case["lo"].astype(float), case["hi"].astype(float),
                           np.hstack(cols).ravel()]).tobytes()


def parse_host(text, p, N):
    """-> (rec [N, p + 11], pred [N, 3], started [N], counts [4])."""
    lines = text.strip().split("\n")
    assert len(lines) == N + 1, len(lines)
    body = np.array([[float(t) for t in ln.split()] for ln in lines[:N]]).reshape(N, p + 15)
    return body[:, :p + 11], body[:, p + 11:p + 14], body[:, p + 14].astype(int), np.array([int(t) for t in lines[N].split()])


def check_frame(rec, pred, ref, case, e, tight, errs):
    """One frame's record and prediction against the restatement: glm_cases.check_record (tight) or the long-double objective
    gap of glm_fuzz_cases.check_default_record (default tolerance).  -> whether the values were compared."""
    p = case["p"]
    what = "seed %d frame %d [%d, %d)" % (case["seed"], e, case["lo"][e], case["hi"][e])
    if ref["status"] == TOO_FEW or case["degenerate"][e]:
        status = int(rec[p + 10])
        if ref["status"] == TOO_FEW:
            assert status == TOO_FEW, (what, status)
        else:
            assert status in (0, 3), (what, status)
        if status != 0:
            assert np.all(np.isnan(rec[:p + 10])) and np.all(np.isnan(pred)), what
        return False
    if tight:
        return GC.check_record(rec, None, ref, p, True, errs, pred[:1], what, "plain", case["lam"])
    status, inside = int(rec[p + 10]), GC.in_conditions(ref, p)
    if ref["status"] != 0:
        assert status == ref["status"], (what, status, ref["status"])
    elif inside:
        assert status == 0, (what, status)
    else:
        assert status in (0, 3), (what, status)
    if status != 0:
        assert np.all(np.isnan(rec[:p + 10])) and np.all(np.isnan(pred)), what
        return False
    assert rec[p + 6] == ref["n_obs"] and rec[p + 9] == 1.0, what
    assert np.all(np.isnan(rec[:p])[ref["dropped"]]), what
    if not inside:
        return False
    assert np.array_equal(np.isnan(rec[:p]), np.isnan(ref["coef"])), what
    s = frame_rows(case, e)
    y, x, off = case["y"][s], case["x"][s], None if case["off"] is None else case["off"][s]
    _, obj = FC.objective_longdouble(case["family"], y, x, off, case["icpt"], case["lam"], rec[:p], rec[p])
    _, robj = FC.objective_longdouble(case["family"], y, x, off, case["icpt"], case["lam"], ref["coef"], ref["intercept"])
    gap = float((obj - robj) / (0.1 + obj))
    errs["default_obj_gap"] = max(errs.get("default_obj_gap", 0.0), gap)
    errs["default_obj_gap_min"] = min(errs.get("default_obj_gap_min", 0.0), gap)
    assert -1e-12 <= gap <= 2e-8, (what, float(obj), float(robj), gap)
    return True


def check_starts(case, rec, started, counts, runs, warm):
    """The start rules from the per-frame flags and the walk's counts: warm + cold = the frames; a warm start only right after a
    fitted frame with every coefficient estimated, inside its run, with both bounds non-decreasing and an overlap; every such
    frame IS warm; every frame refitted cold is counted."""
    p, ic = case["p"], int(case["icpt"])
    lo, hi = case["lo"], case["hi"]
    N = len(lo)
    assert counts[0] + counts[1] == N and counts[0] == int(np.sum(started == 0))
    assert counts[2] == int(np.sum(started == 2)) and counts[1] == int(np.sum(started != 0))
    first = set(int(r) for r in runs[:-1])
    for e in range(N):
        prev_ok = e not in first and e > 0 and rec[e - 1, p + 10] == 0 and not np.isnan(rec[e - 1, :p + ic]).any()
        if prev_ok:   # a fit with an |eta| above 30 (near separation) is not carried; a margin keeps rounding out of the test
            s = frame_rows(case, e - 1)
            eta = case["x"][s] @ rec[e - 1, :p] + (rec[e - 1, p] if ic else 0.0) + (0.0 if case["off"] is None else case["off"][s])
            ok = np.isfinite(case["y"][s]) & np.isfinite(eta)
            big = float(np.max(np.abs(eta[ok])))
            if abs(big - 30.0) < 1e-6:
                continue
            prev_ok = big <= 30.0
        may =bool(warm and prev_ok and hi[e] > lo[e] and lo[e] >= lo[e - 1] and hi[e] >= hi[e - 1] and lo[e] < hi[e - 1])
        assert (started[e] != 0) == may, (e, started[e], may)


def pooled_share(cases):
    """-> (outside, pool): over the cases, the fitted frames of at least 12 k rows (degenerate ones excluded) and those of them
    outside the input conditions.  Identical frames count once."""
    outside = pool = 0
    for c in cases:
        case = make(c)
        k = case["p"] + int(case["icpt"])
        seen = set()
        for e, ref in enumerate(reference(case)):
            key = (int(case["lo"][e]), int(case["hi"][e]))
            if key in seen or case["degenerate"][e] or ref["status"] != 0 or key[1] - key[0] < 12 * k:
                continue
            seen.add(key)
            pool += 1
            outside += not GC.in_conditions(ref, case["p"])
    return outside, pool

"""CPU tier of the GLM window function: the walk of csrc/glm_irls.h (gi_fit_window) in its host build
(tests/tools/glm_window_host.cpp, a program of its own compiled under ASan / UBSan, never loaded into python) on every case of
tests/glm_window_cases.py, checked against tests/glm_restate.py per frame.  The program's slabs have exactly the planner's bound
(the longest frame) and hold a stale value before every run."""
import os
import subprocess

import numpy as np
import pytest

import glm_cases as GC
import glm_window_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = WC.calls() + list(WC.EXPLICIT)


@pytest.fixture(scope="module")
def host_window(tmp_path_factory):
    """tests/tools/glm_window_host.cpp as a program of its own, under ASan / UBSan, as test_glm_cpu builds glm_host.cpp: where a
    process-wide LD_PRELOAD is set a sanitizer's runtime could not be the first one loaded, so there the same program is built
    without the sanitizers and the cases still run."""
    exe = str(tmp_path_factory.mktemp("glm_window") / "glm_window_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "glm_window_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case, tolerance, warm, runs, **kw):
        out = subprocess.run([exe], input=WC.host_input(case, tolerance, warm, runs, **kw), capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return WC.parse_host(out.stdout.decode(), case["p"], len(case["y"]))
    return run


def _min_compared(c):
    """A case whose full frames hold at least 4 k rows compares at least 20 frames; narrower frames are mostly separated or
    ill-conditioned, and there the statuses and NaN patterns are what is asserted."""
    rows = None if c[2] == "explicit" else WC.frame_rows_max(c)
    return 20 if rows is None or rows >= 4 * c[1] else 0


def test_generator_covers_the_widths_frames_and_patterns():
    seen_k, seen_f = set(), {}
    for c in WC.calls():
        case = WC.make(c)
        k = case["p"] + int(case["icpt"])
        seen_k.add((c[0], k))
        seen_f.setdefault(c[2], set()).add(k)
        sizes = np.diff(case["offsets"])
        assert list(sizes[:6]) == [0, 1, 2, k - 1, k, k + 1] and sizes[6] >= max(200, 12 * k + 40)
        refs = WC.reference(case)
        st = np.array([r["status"] for r in refs])
        assert (st == WC.TOO_FEW).any() and (st == 0).any()
        if c[2][0] is not None:   # one y outside the support: status 1 in the frames that hold it, and a fitted frame after them
            bad = np.flatnonzero(st == 1)
            assert len(bad) and (st[bad.max() + 1:] == 0).any()
    assert seen_k == {(f, k) for f in (WC.POISSON, WC.BINOMIAL) for k in WC.WIDTHS}
    assert set(seen_f) == set(WC.FRAMES) and all(len(v) >= 2 for v in seen_f.values())
    dropped = sum(bool(r["status"] == 0 and r["dropped"].any()) for c in WC.calls() for r in WC.reference(WC.make(c)))
    assert dropped > 0 and any(WC.make(c)["degenerate"].any() for c in WC.calls())


def test_pooled_input_conditions():
    """On the restatement alone: at most 5 % of the fitted frames of at least 12 k rows are outside the input conditions."""
    outside, pool = WC.pooled_share(CALLS)
    print("%d of %d frames outside the input conditions (%.2f %%)" % (outside, pool, 100.0 * outside / pool))
    assert pool >= 500 and outside <= WC.OUTSIDE_CAP * pool, (outside, pool)


@pytest.mark.parametrize("c", CALLS, ids=WC.case_id)
def test_cold_walk_is_the_plain_fit_bit_for_bit(host_window, c):
    """warm = 0: the program itself fits every frame's rows, gathered, by a plain gi_fit and fails on any byte that differs in the
    record or in mu of the last row; the interval's bounds (Poisson) are covered by the same comparison."""
    case = WC.make(c)
    runs = WC.whole_runs(case)
    z = 1.96 if case["family"] == WC.POISSON else 0.0
    rec, pred, started, counts = host_window(case, 1e-8, 0, runs, check_plain=True, interval_z=z)
    assert (started == 0).all() and counts[0] == len(started) and counts[1] == counts[2] == 0
    ok = rec[:, case["p"] + 10] == 0
    if z:
        m = ok & np.isfinite(pred[:, 0])
        assert m.any() and np.all(pred[m, 1] <= pred[m, 0]) and np.all(pred[m, 0] <= pred[m, 2]) and np.all(np.isnan(pred[~m, 1:]))
    else:
        assert np.all(np.isnan(pred[:, 1:]))
    refs, errs = WC.reference(case), {}
    for e, ref in enumerate(refs):
        WC.check_frame(rec[e], pred[e], ref, case, e, False, errs)


@pytest.mark.parametrize("c", CALLS, ids=WC.case_id)
def test_warm_walk_tight_tolerance(host_window, c):
    """warm = 1, tolerance = 1e-12: glm_cases.check_record's bounds per frame (coefficients, deviances, AIC and mu 1e-9,
    dispersion 1e-6), statuses and NaN patterns exact; and the start rules from the per-frame flags and the counts."""
    case = WC.make(c)
    runs = WC.whole_runs(case)
    rec, pred, started, counts = host_window(case, 1e-12, 1, runs)
    refs, errs, compared = WC.reference(case), {}, 0
    for e, ref in enumerate(refs):
        compared += WC.check_frame(rec[e], pred[e], ref, case, e, True, errs)
    WC.check_starts(case, rec, started, counts, runs, True)
    assert np.all(np.isnan(pred[:, 1:]))
    print(WC.case_id(c), "compared", compared, "warm", counts[1], "refit", counts[2], {k: "%.2e" % v for k, v in errs.items()})
    assert compared >= _min_compared(c) and (counts[1] > 0 or c[2] == (None, None))


@pytest.mark.parametrize("c", CALLS, ids=WC.case_id)
def test_warm_walk_default_tolerance(host_window, c):
    """warm = 1 at the default tolerance 1e-8: the long-double objective gap (obj - obj*) / (0.1 + obj) within -1e-12 .. 2e-8."""
    case = WC.make(c)
    runs = WC.whole_runs(case)
    rec, pred, started, counts = host_window(case, 1e-8, 1, runs)
    refs, errs, compared = WC.reference(case), {}, 0
    for e, ref in enumerate(refs):
        compared += WC.check_frame(rec[e], pred[e], ref, case, e, False, errs)
    WC.check_starts(case, rec, started, counts, runs, True)
    print(WC.case_id(c), "compared", compared, {k: "%.2e" % v for k, v in errs.items()})
    assert compared >= _min_compared(c)


@pytest.mark.parametrize("run_length", [1, 7])
def test_short_runs_keep_statuses_and_bounds(host_window, run_length):
    """Runs of 1 and 7 rows (every run begins cold): the same statuses as whole-partition runs, values within the bounds."""
    c = WC.calls()[0]
    case = WC.make(c)
    whole = host_window(case, 1e-12, 1, WC.whole_runs(case))
    runs = WC.cut_runs(case, run_length)
    rec, pred, started, counts = host_window(case, 1e-12, 1, runs)
    p = case["p"]
    assert np.array_equal(rec[:, p + 10], whole[0][:, p + 10]) and np.array_equal(np.isnan(rec), np.isnan(whole[0]))
    for e, ref in enumerate(WC.reference(case)):
        WC.check_frame(rec[e], pred[e], ref, case, e, True, {})
    WC.check_starts(case, rec, started, counts, runs, True)
    if run_length == 1:
        assert counts[1] == 0


def test_invalid_options_fail_every_row(host_window):
    case = WC.make(WC.calls()[0])
    rec, pred, started, counts = host_window(case, float("nan"), 1, WC.whole_runs(case))
    p = case["p"]
    assert np.all(rec[:, p + 10] == 1) and np.all(np.isnan(rec[:, :p + 10])) and np.all(np.isnan(pred)) and counts[1] == 0


def test_no_convergence_is_refitted_cold_and_stays_a_failure(host_window):
    """max_iterations = 1: no cold fit converges, so no frame ever starts warm and every fitted frame reports status 3."""
    case = WC.make(WC.calls()[0])
    rec, pred, started, counts = host_window(case, 1e-12, 1, WC.whole_runs(case), max_iterations=1)
    p = case["p"]
    st = np.array([r["status"] for r in WC.reference(case)])
    assert np.all(rec[st == 0, p + 10] == 3) and counts[1] == 0 and np.all(np.isnan(pred))

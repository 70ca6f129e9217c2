"""The quantile regression window walk without a GPU: csrc/quantile_solve.h::qs_fit_window compiled as plain C++ under ASan /
UBSan behind a stand-alone main (tests/tools/quantile_window_host.cpp, never loaded into python).  The tool gives every run a
scratch slab of exactly the planner's bound, filled with stale values, and prints next to every frame's record the cold
qs_fit of the same rows.  Every frame is held to tests/quantile_window_cases.py::check_frame against the restatement
(tests/quantile_restate.py::solve) and to the cold fit's loss."""
import os
import subprocess

import numpy as np
import pytest

import quantile_fuzz_cases as qf
import quantile_restate as qr
import quantile_window_cases as qw
from conftest import ROOT
from test_quantile_cpu import _case_text, host_solver  # noqa: F401  (host_solver: the single-fit tool, a fixture)

SAN = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
       "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def window_solver(tmp_path_factory):
    """run(list of (X, y, lo, hi, tau, icpt[, run_length[, max_it]])) -> quantile_window_cases.parse_window_output."""
    exe = str(tmp_path_factory.mktemp("qw") / "quantile_window_host")
    r = subprocess.run(SAN + [os.path.join(ROOT, "tests", "tools", "quantile_window_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(jobs):
        jobs = [tuple(j) + (0, 1000)[len(j) - 6:] for j in jobs]
        text = "".join(qw.window_text(X, y, lo, hi, tau, icpt, L, m) for X, y, lo, hi, tau, icpt, L, m in jobs)
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
        out = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
        return qw.parse_window_output(out.stdout, jobs)
    return run


def assert_same_loss_as_cold(r, p, what):
    """The walk's vertex may differ from the cold fit's where the optimum is not unique; status, n and the loss may not.  Both
    losses are sums of the same n rounded residuals at two optimal vertices: 1e-9 relative, the tolerance check_record holds
    a loss to, plus the 1e-12 max|y| it allows an interpolating fit (|y| <= the loss scale is not known here: the record's own
    loss bounds it from below, so the absolute term uses the cold record's coefficients' scale instead — 1e-12 (1 + loss))."""
    rec, cold = r["rec"], r["cold_rec"]
    assert np.array_equal(rec[:, p + 5], cold[:, p + 5]), f"{what}: status"
    ok = rec[:, p + 5] == 0
    assert np.array_equal(rec[ok, p + 4], cold[ok, p + 4]), f"{what}: n_observations"
    assert (np.abs(rec[ok, p + 2] - cold[ok, p + 2]) <= 1e-9 * cold[ok, p + 2] + 1e-12 * (1.0 + cold[ok, p + 2])).all(), f"{what}: loss"
    assert (r["its"][ok] >= 0).all() and (r["cold_its"][ok] >= 0).all(), f"{what}: a pivot budget ran out"


# ---- a. the walk against cold fits and the restatement, per data kind ------------------------------------------------------
def test_input_conditions_of_the_kinds_case():
    """On the reference alone: the continuous frames outside the coefficient comparison stay within the cap, every non-unique
    reference closed its gap (quantile_fuzz_cases.assert_input_conditions)."""
    off, y, X, kinds = qw.kinds_case()
    lo, hi = qw.rows_frames(off, qw.A_FRAME, 0)
    refs, ks, data = [], [], []
    for g, kind in enumerate(kinds):
        for e in range(int(off[g]), int(off[g + 1])):
            refs.append(qw.frame_ref(X, y, lo[e], hi[e], qw.A_TAU, True))
            ks.append(kind)
            data.append((X[lo[e]:hi[e]], y[lo[e]:hi[e]], True))
    qf.assert_input_conditions(refs, ks, data, "kinds case")
    cont = [r for r, k in zip(refs, ks) if k in qf.CONTINUOUS and r is not None]
    assert len(cont) >= 60 and sum(not qf.in_comparison(r) for r in cont) <= qf.UNCOMPARED_CAP * len(cont)
    assert sum(r is not None for r, k in zip(refs, ks) if k == "lattice") >= 30


@pytest.mark.parametrize("run_length", [0, 7])
def test_walk_against_cold_and_restatement_per_kind(window_solver, run_length, capsys):
    off, y, X, kinds = qw.kinds_case()
    lo, hi = qw.rows_frames(off, qw.A_FRAME, 0)
    (r,) = window_solver([(X, y, lo, hi, qw.A_TAU, True, run_length)])
    p = X.shape[1]
    assert_same_loss_as_cold(r, p, "kinds")
    tally = qf.Tally()
    for g, kind in enumerate(kinds):
        rows = range(int(off[g]), int(off[g + 1]))
        qw.check_partition(X, y, lo, hi, qw.A_TAU, True, r["rec"], r["its"], r["yhat"], kind, f"{kind} L={run_length}", rows, tally)
    with capsys.disabled():
        print("\n  " + tally.line(f"window walk, run length {run_length}"))
    assert tally.outside <= qf.UNCOMPARED_CAP * tally.continuous
    assert tally.lattice >= 30 and tally.aliased >= 60


# ---- b. frame shapes -------------------------------------------------------------------------------------------------------
SHAPES = {"5 preceding": (5, 0), "3 preceding 2 following": (3, -2), "unbounded preceding": (None, 0),
          "unbounded following": (0, None), "narrower than k": (0, 0), "exactly k rows": None}


@pytest.mark.parametrize("icpt", [True, False], ids=["icpt", "noicpt"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_shapes(window_solver, shape, icpt):
    X, y = qw.small_partition()
    n, p = X.shape
    k = p + int(icpt)
    off = np.array([0, n], dtype=np.int64)
    if shape == "exactly k rows":
        Xc, yc = X.copy(), y.copy()
        yc[11], Xc[23] = 0.25, [0.5, 1.5]                    # every row valid: a frame of k rows has exactly k valid rows
        X, y = Xc, yc
        lo, hi = qw.rows_frames(off, k - 1, 0)
    else:
        lo, hi = qw.rows_frames(off, *SHAPES[shape])
    taus = (0.1, 0.5, 0.9)
    runs = window_solver([(X, y, lo, hi, tau, icpt) for tau in taus])
    for tau, r in zip(taus, runs):
        what = f"{shape} icpt={int(icpt)} tau={tau}"
        assert_same_loss_as_cold(r, p, what)
        qw.check_partition(X, y, lo, hi, tau, icpt, r["rec"], r["its"], r["yhat"], "plain", what)
        st = r["rec"][:, p + 5]
        if shape == "narrower than k":
            assert (st != 0).all() and np.isnan(r["yhat"]).all() and (r["its"] == 0).all(), what
        elif shape == "exactly k rows":
            full = hi - lo == k
            assert full.sum() == n - (k - 1) and (st[full] == 0).all() and (st[~full] != 0).all(), what
            assert (r["rec"][full, p + 2] <= 1e-12 * np.max(np.abs(y))).all(), what          # interpolates: the loss is rounding
            assert (r["rec"][full, p + 3] == k).all() and (r["rec"][full, p + 4] == k).all(), what
        elif shape == "3 preceding 2 following":
            assert hi[0] == 3 and lo[n - 1] == n - 4 and hi[n - 1] == n and (hi - 1 != np.arange(n)).sum() == n - 1   # clipped at both ends; x of row hi - 1
            assert (st[6:] == 0).all(), what
        elif shape == "unbounded following":
            assert (np.diff(hi) == 0).all() and (np.diff(lo) == 1).all() and (st[:n - 8] == 0).all(), what
        else:
            assert (st[8:] == 0).all(), what


# ---- c. runs ---------------------------------------------------------------------------------------------------------------
def test_runs_of_1_7_and_the_whole_partition_agree(window_solver):
    X, y = qw.small_partition(seed=1, n=60, p=2)
    n, p = X.shape
    lo, hi = qw.rows_frames(np.array([0, n]), 9, 0)
    whole, seven, one = window_solver([(X, y, lo, hi, 0.5, True, L) for L in (0, 7, 1)])
    assert (one["cold"][hi > lo] == 1).all() and seven["cold"][::7].all() and whole["cold"][0] == 1 and whole["cold"].sum() < seven["cold"].sum() < n
    assert np.array_equal(one["rec"], one["cold_rec"], equal_nan=True) and np.array_equal(one["its"], one["cold_its"])   # runs of one frame ARE cold fits
    for other, name in ((seven, "7"), (one, "1")):
        assert np.array_equal(whole["rec"][:, p + 5], other["rec"][:, p + 5]), name
        ok = whole["rec"][:, p + 5] == 0
        a, b = whole["rec"][ok, p + 2], other["rec"][ok, p + 2]
        assert (np.abs(a - b) <= 1e-9 * b + 1e-12 * np.nanmax(np.abs(y))).all(), name
        for e in np.nonzero(ok)[0]:
            ref = qw.frame_ref(X, y, lo[e], hi[e], 0.5, True)
            if qf.in_comparison(ref) and np.isfinite(X[hi[e] - 1]).all():                    # the vertex is unique: yhat agrees
                a_q = np.concatenate([[1.0], X[hi[e] - 1]])
                s = np.concatenate([[1.0], np.max(np.abs(X[lo[e]:hi[e]][qr.valid_rows(X[lo[e]:hi[e]], y[lo[e]:hi[e]])]), axis=0)])
                want = np.concatenate([[ref["b0"]], ref["b"]])
                tol = 2 * qf.COEF_TOL * float(np.max(np.abs(want) * s)) * float(np.sum(np.abs(a_q) / s))
                assert abs(whole["yhat"][e] - other["yhat"][e]) <= tol, (name, e)


# ---- d. the warm start pays ------------------------------------------------------------------------------------------------
def test_the_walk_spends_fewer_pivots_than_cold_fits(window_solver, capsys):
    rng = np.random.default_rng([20261018, 9])
    n, p = 400, 3
    X = rng.normal(size=(n, p))
    y = X @ [1.0, -2.0, 0.5] + rng.standard_t(3, size=n)
    lo, hi = qw.rows_frames(np.array([0, n]), 40, 0)
    (r,) = window_solver([(X, y, lo, hi, 0.5, True)])
    assert_same_loss_as_cold(r, p, "warm")
    ok = r["rec"][:, p + 5] == 0
    walk, cold = int(np.abs(r["its"][ok]).sum()), int(np.abs(r["cold_its"][ok]).sum())
    with capsys.disabled():
        print(f"\n  pivots  n=400 p=3 frame 40 preceding: walk {walk}  cold {cold}  ratio {walk / cold:.3f}  "
              f"frames begun afresh {int(r['cold'][ok].sum())}/{int(ok.sum())} ({100 * r['cold'][ok].mean():.1f} %), "
              f"of them restarts after a fitted frame {r['restarts']}")
    assert walk < cold
    assert r["restarts"] == int(r["cold"][ok].sum()) - 1      # one run: every fresh start but the first fitted frame's lost a basis row


# ---- e. forced cold starts -------------------------------------------------------------------------------------------------
def test_forced_cold_starts(window_solver):
    rng = np.random.default_rng([20261018, 10])
    n, p, icpt = 40, 2, True
    k = p + 1
    X = rng.normal(size=(n, p))
    y = X @ [1.0, 2.0] + rng.normal(size=n)
    off = np.array([0, n])
    # a frame of k + 1 rows: k of them are the basis, so the row that leaves is a basis row on nearly every step
    lo, hi = qw.rows_frames(off, k, 0)
    # explicit frames: a non-monotone pair (row 21 steps back), disjoint neighbours (row 31), a failed frame (row 35: empty)
    lo2, hi2 = qw.rows_frames(off, 9, 0)
    lo2, hi2 = lo2.copy(), hi2.copy()
    lo2[21], hi2[21] = 2, 14
    lo2[30], hi2[30] = 5, 17
    lo2[31], hi2[31] = 17, 29
    lo2[35], hi2[35] = 35, 35
    leave, odd = window_solver([(X, y, lo, hi, 0.5, icpt), (X, y, lo2, hi2, 0.5, icpt)])
    for r, (a, b), what in ((leave, (lo, hi), "leaving basis row"), (odd, (lo2, hi2), "explicit frames")):
        assert_same_loss_as_cold(r, p, what)
        qw.check_partition(X, y, a, b, 0.5, icpt, r["rec"], r["its"], r["yhat"], "plain", what)
    full = hi - lo == k + 1
    assert leave["cold"][full].mean() >= 0.6              # k of k + 1 rows are in the basis: the oldest row is one of them 3 times in 4
    c = odd["cold"]
    assert c[21] == 1 and c[22] == 1                      # back, and forward again past rows never seen: both bounds must not decrease
    assert c[30] == 1 and c[31] == 1                      # [5, 17) then [17, 29): monotone and disjoint
    assert odd["rec"][35, p + 5] == qr.STATUS_TOO_FEW_ROWS and c[35] == 0 and c[36] == 1      # the frame after a failed one
    assert c[10:21].sum() < 11                            # and between them the walk does carry its vertex


# ---- f. the existing entry points are unchanged ----------------------------------------------------------------------------
def test_golden_output_of_the_single_fit_tool_is_unchanged(host_solver):
    """qs_fit through tests/tools/quantile_solve_host.cpp on every golden case, byte for byte what the parent commit printed:
    the scratch origin and the shared column-size helper change no floating-point operation (tests/golden/quantile/
    solve_host_expected.txt holds the parent's output)."""
    cases = qr.load_cases()
    rows = host_solver("".join(_case_text(c["X"], c["y"], c["tau"], c["fit_intercept"]) for c in cases))
    with open(os.path.join(ROOT, "tests", "golden", "quantile", "solve_host_expected.txt")) as f:
        want = [np.array([float(t) for t in ln.split()]) for ln in f.read().strip().split("\n")]
    assert len(rows) == len(want) == len(cases)
    for c, a, b in zip(cases, rows, want):
        assert a.tobytes() == b.tobytes(), c["name"]

"""Writes tests/golden/quantile/path_cases.json: a handful of data sets, each solved at the seven tau of a decile-and-tails
grid by scipy's HiGHS through make_quantile_cases.solve_lp (the same linear program, the same re-solve of a single vertex,
the same `unique` flag).  The Gaussian data sets are the first n rows and p columns of cases.json's x_base; widths cases.json
has (1, 2, 8, 32) keep its y, p = 4 gets a y of its own, and `tied` is the p = 2 y rounded to whole numbers (many equal y).
high_dim (x_j = j x_1: aliased) and large_data are the reference's integer tables.

Run from the repository root:  python tests/golden/make_quantile_path_cases.py   (needs scipy; the tests do not)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import quantile_restate as qr  # noqa: E402
from make_quantile_cases import solve_lp  # noqa: E402

TAUS = (0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95)


def main():
    with open(qr.GOLDEN) as f:
        doc = json.load(f)
    base = np.array(doc["x_base"], dtype=np.float64).reshape(130, 32)
    y_of = {d["p"]: np.array(d["y"], dtype=np.float64) for d in doc["datasets"] if "X" not in d}
    rng = np.random.default_rng(20250317)
    y4 = np.round(base[:, :4] @ rng.uniform(-2.0, 2.0, size=4) + 1.5 + rng.standard_t(3, size=130), 3)
    tables = qr.reference_tables()
    sets = [("gauss p=1 n=10", base[:10, :1], y_of[1][:10], (True,)),
            ("gauss p=4 n=40", base[:40, :4], y4[:40], (True, False)),
            ("gauss p=8 n=65", base[:65, :8], y_of[8][:65], (True,)),
            ("gauss p=32 n=130", base[:130, :32], y_of[32][:130], (True,)),
            ("tied p=2 n=64", base[:64, :2], np.round(y_of[2][:64]), (True, False))]
    for name in ("high_dim", "large_data"):
        y, X = tables[name]
        ok = np.isfinite(y)
        sets.append((name, X[ok], y[ok], (True,)))
    datasets, cases = [], []
    for name, X, y, icpts in sets:
        from_base = name.startswith(("gauss", "tied"))
        for icpt in icpts:
            d = dict(name=f"{name} icpt={int(icpt)}", p=X.shape[1], n=len(y), fit_intercept=icpt, y=y.tolist())
            if not from_base:
                d["X"] = X.ravel().tolist()
            datasets.append(d)
            for tau in TAUS:
                cases.append(dict(dataset=len(datasets) - 1, tau=tau, **solve_lp(X, y, tau, icpt)))
    out = os.path.join(HERE, "quantile", "path_cases.json")
    dump = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    with open(out, "w") as f:                        # one data set, one case per line
        f.write('{"taus":' + dump(list(TAUS)) + ',\n"datasets":[\n' + ",\n".join(dump(d) for d in datasets) + '\n],"cases":[\n' +
                ",\n".join(dump(c) for c in cases) + "\n]}\n")
    print(f"{len(datasets)} data sets, {len(cases)} cases, {sum(c['unique'] for c in cases)} unique, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()

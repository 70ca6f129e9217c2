"""CPU tier of the host entries' slab cut: csrc/row_slabs.h in tests/tools/row_slabs_host.cpp, a program of its own compiled
under ASan / UBSan and never loaded into python, against a restatement of the loop in Python."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAB_ROWS = 10


def restated(off, slab_rows):
    """The cut, spelt out: [(g0, g1, offsets rebased to the slab's first row)]."""
    out, g0, n = [], 0, len(off) - 1
    while g0 < n:
        g1 = g0 + 1
        while g1 < n and off[g1 + 1] - off[g0] <= slab_rows:
            g1 += 1
        out.append((g0, g1, [off[g] - off[g0] for g in range(g0, g1 + 1)]))
        g0 = g1
    return out


def offsets(sizes, first=0):
    return [first + int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]


def cases():
    named = [("four-threes", offsets([3, 3, 3, 3])), ("exactly-a-slab", offsets([10])), ("one-over", offsets([11])),
             ("oversized-middle", offsets([4, 11, 4])), ("empty-around-cuts", offsets([0, 0, 5, 0, 5, 0, 0])),
             ("empty-after-full", offsets([10, 0, 0, 1])), ("starts-at-7", offsets([3, 8, 0, 2, 9, 1], first=7))]
    rng = np.random.default_rng(20240607)
    for i in range(200):
        named.append(("random-%03d" % i, offsets(rng.integers(0, 16, size=int(rng.integers(1, 25))))))
    return named


CASES = cases()
# the walk of for_each_row_slab with slabs of 4 rows: empty groups at both ends, groups larger than a slab
EACH_SLAB_ROWS, EACH_SIZES = 4, [0, 1, 32, 31, 5, 0]


@pytest.fixture(scope="module")
def slabs_of(tmp_path_factory):
    """Every case through one run of the program (built as tests/test_glm_cpu.py builds its own: without the sanitizers only where
    a process-wide LD_PRELOAD keeps their runtime from being loaded first)."""
    exe = str(tmp_path_factory.mktemp("row_slabs") / "row_slabs_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "row_slabs_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = "".join("%d %d %s\n" % (SLAB_ROWS, len(off) - 1, " ".join(map(str, off))) for _, off in CASES)
    each_off = offsets(EACH_SIZES)
    data += "%d %d %s\n" % (EACH_SLAB_ROWS, len(each_off) - 1, " ".join(map(str, each_off)))
    out = subprocess.run([exe], input=data.encode(), capture_output=True)
    err = out.stderr.decode()
    assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
    got, cur, each, stop = {}, [], [], []
    names = iter([name for name, _ in CASES] + ["each"])
    for ln in out.stdout.decode().split("\n"):
        if ln == "end":
            got[next(names)] = (cur, each, stop)
            cur, each, stop = [], [], []
        elif ln.startswith("each "):
            t = [int(v) for v in ln.split()[1:]]
            each.append((t[0], t[1], t[2], t[3], t[4:]))
        elif ln.startswith("stop "):
            stop.append(int(ln.split()[1]))
        elif ln:
            t = [int(v) for v in ln.split()]
            cur.append((t[0], t[1], t[2:]))
    assert len(got) == len(CASES) + 1
    return got


@pytest.mark.parametrize("name,off", CASES, ids=[c[0] for c in CASES])
def test_slabs(slabs_of, name, off):
    (slabs, each, stop), n = slabs_of[name], len(off) - 1
    # the walk visits the slabs of the cut, and stops after the slab whose callback says so
    assert [(g0, g0 + G, reb) for g0, G, _, _, reb in each] == slabs
    assert all(r0 == off[g0] and R == reb[-1] == off[g0 + G] - off[g0] for g0, G, r0, R, reb in each)
    assert stop == [s[0] for s in slabs[:2]]
    assert slabs == restated(off, SLAB_ROWS)
    # every group in exactly one slab, the slabs contiguous and in order, none empty
    assert slabs[0][0] == 0 and slabs[-1][1] == n
    for (a0, a1, _), (b0, _, _) in zip(slabs, slabs[1:]):
        assert a1 == b0
    for g0, g1, reb in slabs:
        assert g1 > g0 and len(reb) == g1 - g0 + 1 and reb[0] == 0
        assert g1 - g0 == 1 or off[g1] - off[g0] <= SLAB_ROWS


def test_for_each_row_slab_with_slabs_of_four_rows(slabs_of):
    off = offsets(EACH_SIZES)
    slabs, each, stop = slabs_of["each"]
    assert slabs == restated(off, EACH_SLAB_ROWS)
    # every group exactly once and in order
    assert [g for g0, G, _, _, _ in each for g in range(g0, g0 + G)] == list(range(len(EACH_SIZES)))
    for g0, G, r0, R, reb in each:
        # r0 and the rebased offsets are consistent with the caller's offsets
        assert r0 == off[g0] and reb == [off[g] - r0 for g in range(g0, g0 + G + 1)] and R == reb[-1]
        # a group larger than the slab has a slab of its own
        assert R <= EACH_SLAB_ROWS or G == 1
    assert [(g0, G) for g0, G, _, _, _ in each] == [(0, 2), (2, 1), (3, 1), (4, 1), (5, 1)]
    # the walk stopped early: the callback said `false` at the second slab of five
    assert stop == [0, 2]
